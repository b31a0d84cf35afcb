"""The two dropout aggregation kernels of csrc/dropout.hip -- spmm_dropout_p3_kernel<CPL> (gte_spmm_dropout_p3) and
spmm_dropout_bwd_kernel<CPL> (gte_spmm_dropout_bwd) -- through ``ops`` against the masked reference of tests/dropout_ref.py, on the
131-row degree ladder of tests/spmm_ref.py (the backward on a ladder of out-degrees of its own), at one width on either side of
every dispatch threshold and in the second pass of the kernels' column loop.  Run with ``-m gpu`` on an MI355X; ``-s`` prints the
worst error / bound ratio of every bound case.

EXACT cases (integer x and G, weights 0.5 / 1 / 2, p = 0.5 / 0.75: the result is the same in any summation order) are held bit for
bit on every row and column, the image's padding columns to zero, the bytes around every output to their pre-fill; BOUND cases to
    forward   |agg - ref| <= (deg + 5) 2^-24 s (1 / deg) sum |w| |x'|        backward  |dx - ref| <= (deg_out + 3) 2^-24 (|D_self| + sum |w_out| |D_agg|)
both derived in tests/dropout_ref.py and checked by tests/test_dropout_ref_cpu.py against a float32 emulation of each kernel and
eight mutants of it.  The masks of the reference are numpy Philox, not the library's.

NON-FINITE CONFINEMENT: a node whose whole row is +Inf / NaN reaches its own row of the self image (of dx: its self half) and the
rows that name it, there exactly the positions the masks keep; everything else is bit for bit the clean run.

MEASURED on an MI355X, largest error / bound ratio per bound case (worst over p = 0.1, 0.3, 0.9 and both in_drop settings; 'scales'
and 'cancel' alike to three digits: the worst elements sit on rows of degree 1 and 2, which the cancelling twins do not reach, and a
power-of-two column scale changes no relative error):
    producer  F = 13 0.366   F = 259 0.368   F = 1030 0.394
    backward  F = 13 0.356   F = 258 0.410   F = 1030 0.444
digit for digit the float32 emulation's figures (tests/test_dropout_ref_cpu.py).  On the rows without out-edges the backward's dx is
the elementwise product fl32(G s) under the mask, held bit for bit at every p of the bound cases.  Every exact case was bitwise from the first run,
the second column pass, CPL = 2 of the backward, the unweighted branch, the misaligned fp32 rows and the 32-bit cut of the counter
included; nothing in the kernels had to change.  FOUND: both entry points refused an edgeless batch (the empty edge tensors' device
pointer is NULL and their null checks rejected it), and gte_gcnsage_step, which hands them the plan's edge arrays, with them; they
now take NULL edge arrays for a graph without edges (include/gte.h), and the two edgeless tests at the end of this file run.
"""
import functools

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import dropout_ref as dr
from tests import spmm_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 1232.0
FILL = 0x55
INPUTS = ["f32", "f32_pad", "p3", "resident"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counter(step):
    return torch.tensor([step], dtype=torch.int64, device=DEV)


class DeviceGraph:
    def __init__(self, g):
        self.g, self.n = g, g.n
        self.ip, self.ix = dev(g.indptr), dev(g.indices)


@functools.lru_cache(maxsize=None)
def graph(name):
    kind, _, arg = name.partition(":")
    return DeviceGraph({"ladder": dr.ladder_graph, "bwd": dr.bwd_graph, "confine": lambda: dr.confine_graph(int(arg))}[kind]())


# ---- the harness every call shares -------------------------------------------------------------------------------------------------
def x_input(kind, res, rows, n):
    """(what ops.spmm_dropout_p3 takes as x, the batch's rows as numpy) -- res [n_res, f]: the batch is res[:n], or res[rows] through
    a row map into the resident image of all of res"""
    f = res.shape[1]
    if kind == "f32":
        return dev(res[:n]), res[:n]
    if kind == "f32_pad":                # a column slice of a wider buffer: ldx = f + 3, rows that are not 16-byte aligned, NaN around
        buf = torch.full((n + 1, f + 3), NAN, dtype=torch.float32, device=DEV)
        v = buf[:n, 1:1 + f]
        v.copy_(dev(res[:n]))
        assert v.stride(0) == f + 3 and (v.data_ptr() - buf.data_ptr()) == 4
        return v, res[:n]
    if kind == "p3":
        return ops.p3_from_f32(dev(res[:n])), res[:n]
    n_res = res.shape[0]                 # the zero sentinel row behind the image, the map's padding entries naming it
    img = ops.P3.empty(n_res, f, DEV, rows_cap=n_res + 1)
    img.data[n_res:].zero_()
    ops.p3_from_f32(dev(res), out=img)
    rmap = np.full(dr.c16(n) + 1, n_res, dtype=np.int32)
    rmap[:n] = rows
    assert (rows != np.arange(n)).all()
    return ops.P3(img.data, n, f, dev(rmap), n_res), res[rows]


def out_image(n, f, wide):
    rb = int(_lib.load().gte_p3_row_bytes(f))
    return ops.P3(torch.full((n + 1, rb + (32 if wide else 0)), FILL, dtype=torch.uint8, device=DEV), n, f)


def decode(img, what):
    """the image's columns [0, f) as float32 numpy, after checking that the rest of its last 16-column block is zero and that no byte
    past a row's blocks, nor the row behind the last, was written"""
    n, f = img.rows, img.cols
    rb = int(_lib.load().gte_p3_row_bytes(f))
    assert bool((img.data[n] == FILL).all()), what + ": written past the image's last row"
    assert bool((img.data[:n, rb:] == FILL).all()), what + ": written past row_bytes(f) of a row"
    full = ops.p3_to_f32(ops.P3(img.data, n, dr.c16(f))).cpu().numpy()
    assert (sr.bits(full[:, f:]) == 0).all(), what + ": columns f .. the next multiple of 16 must be zeros"
    return full[:, :f]


def run_producer(dg, w, xin, p, seed, rank, step, site, in_drop, wide=True, ctr=None):
    f = xin.cols if isinstance(xin, ops.P3) else xin.shape[1]
    ctr = counter(step) if ctr is None else ctr
    sp, ap = out_image(dg.n, f, wide), out_image(dg.n, f, wide)
    ops.spmm_dropout_p3(dg.ip, dg.ix, None if w is None else dev(w), xin, dg.n, p, seed, rank, ctr, site, in_drop, self_out=sp, agg_out=ap)
    return decode(sp, "self image"), decode(ap, "agg image")


def run_bwd(dg, w, G, agg_col, f, p, seed, rank, step, site, guard=0, ctr=None):
    """dx [n, f]; ``guard``: extra columns of G (NaN) and of dx (sentinel) beyond what the call needs"""
    n4 = dr.c4(f)
    Gd = dev(G)
    assert Gd.stride(0) == G.shape[1] and G.shape[1] >= agg_col + n4
    buf = torch.full((dg.n + 1, n4 + guard), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[:dg.n, :n4]
    ctr = counter(step) if ctr is None else ctr
    got = ops.spmm_dropout_bwd(dg.ip, dg.ix, dev(w), Gd, agg_col, f, p, seed, rank, ctr, site, out=out)
    assert got.data_ptr() == buf.data_ptr()
    assert bool((buf[dg.n] == SENTINEL).all()) and bool((buf[:dg.n, n4:] == SENTINEL).all()), "written outside dx"
    full = out.cpu().numpy()
    assert (sr.bits(full[:, f:]) == 0).all(), "columns f .. round_up(f, 4) of dx must be zeros"
    return full[:, :f]


WORST = {}


def note(entry, r):
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    return r


def report(prefix):
    print("\n    worst error / bound so far: " + "  ".join(f"{e} {v:.3f}" for e, v in sorted(WORST.items()) if e.startswith(prefix)))


def assert_images(got, want, what):
    for name, a, b in (("self", got[0], want[0]), ("agg", got[1], want[1])):
        bad = sr.bits(a) != sr.bits(b)
        assert not bad.any(), (f"{what}: the {name} image differs in {int(bad.sum())} elements, rows {np.flatnonzero(bad.any(axis=1))[:8]}, "
                               f"columns {np.flatnonzero(bad.any(axis=0))[:8]}")


# ---- the producer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", dr.PRODUCER_WIDTHS)
def test_producer_is_exact_at_every_width_and_input(f):
    dg = graph("ladder")
    c = dr.coords(f)
    g, w, res, rows = dr.producer_exact_case(f)
    for i, in_drop in enumerate((False, True)):
        p = dr.EXACT_P[(i + f) % 2]
        want = {}
        for kind in INPUTS:
            xin, x = x_input(kind, res, rows, g.n)
            key = kind == "resident"
            if key not in want:
                want[key] = dr.producer_expect(g, w, x, p, in_drop=in_drop, **c)
            got = run_producer(dg, w, xin, p, in_drop=in_drop, wide=kind != "f32", **c)
            assert_images(got, want[key], f"F={f} in_drop={in_drop} input={kind} p={p}")
    # eweight NULL: unit weights
    _, _, res1, _ = dr.producer_exact_case(f, weights=False)
    xin, x = x_input("f32_pad", res1, rows, g.n)
    for in_drop in (False, True):
        got = run_producer(dg, None, xin, 0.5, in_drop=in_drop, **c)
        assert_images(got, dr.producer_expect(g, np.ones(g.nnz, dtype=np.float32), x, 0.5, in_drop=in_drop, **c), f"F={f} unweighted in_drop={in_drop}")


@pytest.mark.parametrize("seed,rank,step,site", dr.COORDS)
def test_producer_at_every_coordinate(seed, rank, step, site):
    dg = graph("ladder")
    for f in dr.COORD_WIDTHS:
        g, w, res, rows = dr.producer_exact_case(f)
        for in_drop, kind in ((True, "resident"), (False, "f32_pad")):
            xin, x = x_input(kind, res, rows, g.n)
            got = run_producer(dg, w, xin, 0.75, seed, rank, step, site, in_drop)
            assert_images(got, dr.producer_expect(g, w, x, 0.75, seed, rank, step, site, in_drop), f"F={f} seed={seed:#x} rank={rank} step={step} site={site}")


@pytest.mark.parametrize("step", [3, 2 ** 32 - 1])
def test_producer_reads_the_step_from_the_device_at_every_launch(step):
    """the counter is incremented on the device between two launches, with no host round trip: the second draws the next step's masks
    (after 2^32 - 1: step 0, the 32-bit cut)"""
    dg = graph("ladder")
    f = 259
    g, w, res, rows = dr.producer_exact_case(f)
    xin, x = x_input("p3", res, rows, g.n)
    ctr = counter(step)
    c = dict(seed=5, rank=1, site=2)
    first = run_producer(dg, w, xin, 0.5, step=None, in_drop=True, ctr=ctr, **c)
    ctr.add_(1)
    second = run_producer(dg, w, xin, 0.5, step=None, in_drop=True, ctr=ctr, **c)
    assert_images(first, dr.producer_expect(g, w, x, 0.5, step=step, in_drop=True, **c), f"step {step}")
    assert_images(second, dr.producer_expect(g, w, x, 0.5, step=(step + 1) % 2 ** 32, in_drop=True, **c), f"step {step} + 1")
    assert not sr.same_bits(first[1], second[1])


@pytest.mark.parametrize("p", dr.SELF_P)
def test_self_image_is_bit_exact_for_every_p(p):
    """two fp32 products and two selects: the reference's numpy float32 arithmetic is the device's, with the scale taken from the fp32
    value of p (P_SWEPT: the scale from the double p is another float) and at both ends of the threshold"""
    dg = graph("ladder")
    for f in dr.COORD_WIDTHS:
        g, w, x = dr.producer_bound_case(f, "scales")
        assert g is dg.g or np.array_equal(g.indices, dg.g.indices)
        c = dr.coords(f)
        for in_drop in (False, True):
            got_s, got_a = run_producer(dg, w, dev(x), p, in_drop=in_drop, **c)
            ref_s, ref_a = dr.producer_ref(g, w, x, p, in_drop=in_drop, **c)
            assert sr.same_bits(got_s, ref_s), f"F={f} p={p} in_drop={in_drop}: {int((sr.bits(got_s) != sr.bits(ref_s)).sum())} elements differ"
            q = sr.ratio(got_a, ref_a, dr.producer_bound(g, w, x, p, in_drop=in_drop, **c))
            assert q <= 1.0, f"F={f} p={p}: error / bound = {q:.3f}"
    if p == dr.P_LOW:
        assert (got_s != 0).sum() == (x != 0).sum()              # nothing dropped
    if p == dr.P_HIGH:
        assert (got_s != 0).sum() <= 2                           # keep rate 2^-24


@pytest.mark.parametrize("kind", sr.BOUND_KINDS)
@pytest.mark.parametrize("f", dr.PRODUCER_BOUND_WIDTHS)
def test_producer_bound_cases(f, kind):
    g, w, x = dr.producer_bound_case(f, kind)
    dg = graph("ladder") if kind == "scales" else DeviceGraph(g)
    c = dict(dr.BASE)
    for p in dr.BOUND_P:
        for in_drop, inp in ((False, "f32_pad"), (True, "p3")):
            xin, _ = x_input(inp, x, None, g.n)
            got_s, got_a = run_producer(dg, w, xin, p, in_drop=in_drop, **c)
            ref_s, ref_a = dr.producer_ref(g, w, x, p, in_drop=in_drop, **c)
            assert sr.same_bits(got_s, ref_s), f"F={f} {kind} p={p} in_drop={in_drop}: the self image differs"
            q = note(f"producer {kind} F={f}", sr.ratio(got_a, ref_a, dr.producer_bound(g, w, x, p, in_drop=in_drop, **c)))
            print(f"\n    producer {kind} F={f} p={p} in_drop={in_drop}: error / bound = {q:.3f}", end="")
            assert q <= 1.0, f"F={f} {kind} p={p} in_drop={in_drop}: error / bound = {q:.3f}"
    report("producer")


def _poisoned(a, node):
    bad = a.copy()
    bad[node, 0::2], bad[node, 1::2] = np.inf, np.nan
    clean = a.copy()
    clean[node] = 0.0
    return clean, bad


def _assert_confined(got, clean, ref, touched, what):
    """rows outside ``touched`` are the clean run bit for bit; inside, a position is non-finite exactly where the reference is, and
    the clean run's bits elsewhere (a dropped position is 0: masking selects)"""
    assert np.isfinite(clean).all()
    assert sr.same_bits(got[~touched], clean[~touched]), f"{what}: {int((sr.bits(got) != sr.bits(clean))[~touched].any(axis=1).sum())} rows that neither are nor name the node changed"
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), f"{what}: the non-finite positions differ from the reference's in {int((np.isfinite(got) != fin).sum())} places"
    assert (sr.bits(got)[fin] == sr.bits(clean)[fin]).all(), f"{what}: finite positions of the touched rows changed"
    assert (~fin[touched]).any() and fin[touched].any()              # both kinds of position occur: kept (non-finite) and dropped


@pytest.mark.parametrize("in_drop", [False, True])
@pytest.mark.parametrize("f", dr.CONFINE_WIDTHS)
@pytest.mark.parametrize("node", [0, sr.OTHER])
def test_producer_confines_a_non_finite_source(node, f, in_drop):
    dg = graph(f"confine:{node}")
    g = dg.g
    rng = np.random.default_rng(7000 + f)
    w = rng.uniform(0.5, 1.5, g.nnz).astype(np.float32)                       # strictly positive: 0 x Inf is out of scope
    x0, xp = _poisoned(rng.standard_normal((g.n, f)).astype(np.float32), node)
    c = dr.coords(f)
    kind = "f32_pad" if in_drop else "p3"
    clean = run_producer(dg, w, x_input(kind, x0, None, g.n)[0], 0.5, in_drop=in_drop, **c)
    got = run_producer(dg, w, x_input(kind, xp, None, g.n)[0], 0.5, in_drop=in_drop, **c)
    ref = dr.producer_ref(g, w, xp, 0.5, in_drop=in_drop, **c)
    named = g.names(node)
    assert named[38] and g.deg[38] == 5 and (~named & (g.deg % 4 != 0)).any()
    itself = np.arange(g.n) == node
    _assert_confined(got[0], clean[0], ref[0], itself, f"self image, node {node} F={f}")
    _assert_confined(got[1], clean[1], ref[1], named, f"agg image, node {node} F={f}")
    assert not np.isfinite(got[1][38]).all()          # the 5-edge row whose second quad re-reads the node three times at w = 0


# ---- the backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", dr.BWD_WIDTHS)
def test_bwd_is_exact_at_every_width(f):
    dg = graph("bwd")
    c = dr.coords(f)
    n4 = dr.c4(f)
    for i, (agg_col, guard) in enumerate([(dr.c16(f), 0), (n4, 0), (dr.c16(f), 8), (n4 + 4, 12)]):
        g, w, G = dr.bwd_exact_case(f, agg_col, agg_col + n4 + guard)
        p = dr.EXACT_P[(i + f) % 2]
        got = run_bwd(dg, w, G, agg_col, f, p, guard=guard, **c)
        want = dr.bwd_expect(g, w, G, agg_col, f, p, **c)
        bad = sr.bits(got) != sr.bits(want)
        assert not bad.any(), (f"F={f} agg_col={agg_col} guard={guard}: dx differs in {int(bad.sum())} elements, rows "
                               f"{np.flatnonzero(bad.any(axis=1))[:8]}, columns {np.flatnonzero(bad.any(axis=0))[:8]}")


@pytest.mark.parametrize("seed,rank,step,site", dr.COORDS)
def test_bwd_at_every_coordinate(seed, rank, step, site):
    dg = graph("bwd")
    for f in dr.COORD_WIDTHS:
        agg_col = dr.c16(f)
        g, w, G = dr.bwd_exact_case(f, agg_col, 2 * agg_col)
        got = run_bwd(dg, w, G, agg_col, f, 0.75, seed, rank, step, site)
        assert sr.same_bits(got, dr.bwd_expect(g, w, G, agg_col, f, 0.75, seed, rank, step, site)), (f, seed, rank, step, site)


@pytest.mark.parametrize("step", [3, 2 ** 32 - 1])
def test_bwd_reads_the_step_from_the_device_at_every_launch(step):
    dg = graph("bwd")
    f, agg_col = 258, 272
    g, w, G = dr.bwd_exact_case(f, agg_col, 2 * agg_col)
    ctr = counter(step)
    c = dict(seed=5, rank=1, site=2)
    first = run_bwd(dg, w, G, agg_col, f, 0.5, step=None, ctr=ctr, **c)
    ctr.add_(1)
    second = run_bwd(dg, w, G, agg_col, f, 0.5, step=None, ctr=ctr, **c)
    assert sr.same_bits(first, dr.bwd_expect(g, w, G, agg_col, f, 0.5, step=step, **c))
    assert sr.same_bits(second, dr.bwd_expect(g, w, G, agg_col, f, 0.5, step=(step + 1) % 2 ** 32, **c))
    assert not sr.same_bits(first, second)


@pytest.mark.parametrize("kind", sr.BOUND_KINDS)
@pytest.mark.parametrize("f", dr.BWD_BOUND_WIDTHS)
def test_bwd_bound_cases(f, kind):
    agg_col = dr.c16(f)
    g, w, G = dr.bwd_bound_case(f, kind, agg_col, 2 * agg_col)
    dg = graph("bwd") if kind == "scales" else DeviceGraph(g)
    c = dict(dr.BASE)
    for p in dr.BOUND_P:
        got = run_bwd(dg, w, G, agg_col, f, p, **c)
        lone = g.deg == 0                    # rows without out-edges: dx is the elementwise product of the self half, bit for bit
        assert lone.any() and sr.same_bits(got[lone], dr.bwd_self_f32(G, f, p, **c)[lone]), f"F={f} {kind} p={p}: D_self differs"
        q = note(f"bwd {kind} F={f}", sr.ratio(got, dr.bwd_ref(g, w, G, agg_col, f, p, **c), dr.bwd_bound(g, w, G, agg_col, f, p, **c)))
        print(f"\n    bwd {kind} F={f} p={p}: error / bound = {q:.3f}", end="")
        assert q <= 1.0, f"F={f} {kind} p={p}: error / bound = {q:.3f}"
    report("bwd")


@pytest.mark.parametrize("f", dr.CONFINE_WIDTHS)
@pytest.mark.parametrize("node", [0, sr.OTHER])
def test_bwd_confines_a_non_finite_row_of_g(node, f):
    dg = graph(f"confine:{node}")
    g = dg.g
    rng = np.random.default_rng(7100 + f)
    w = rng.uniform(0.5, 1.5, g.nnz).astype(np.float32)
    agg_col = dr.c16(f)
    G = np.zeros((g.n, 2 * agg_col), dtype=np.float32)
    G[:, :f], G[:, agg_col:agg_col + f] = rng.standard_normal((g.n, f)), rng.standard_normal((g.n, f))
    G0, Gp = G.copy(), G.copy()
    for half in (0, agg_col):
        G0[:, half:half + f], Gp[:, half:half + f] = _poisoned(G[:, half:half + f], node)
    c = dr.coords(f)
    clean, got = run_bwd(dg, w, G0, agg_col, f, 0.5, **c), run_bwd(dg, w, Gp, agg_col, f, 0.5, **c)
    touched = g.names(node) | (np.arange(g.n) == node)
    assert touched[38] and (~touched & (g.deg % 4 != 0)).any()
    _assert_confined(got, clean, dr.bwd_ref(g, w, Gp, agg_col, f, 0.5, **c), touched, f"dx, node {node} F={f}")


# ---- the rest ----------------------------------------------------------------------------------------------------------------------
def test_device_mask_with_a_row_stride_leaves_the_guard_bytes():
    n, cols = 131, 517
    buf = torch.full((n, cols + 5), FILL, dtype=torch.uint8, device=DEV)
    got = ops.dropout_mask(0.3, (1 << 40) + 7, 3, 2 ** 32 + 5, 7, n, cols, device=DEV, out=buf[:, :cols])
    assert got.data_ptr() == buf.data_ptr() and bool((buf[:, cols:] == FILL).all()), "guard bytes written"
    m = buf[:, :cols].cpu().numpy()
    np.testing.assert_array_equal(m, ops.dropout_mask(0.3, (1 << 40) + 7, 3, 2 ** 32 + 5, 7, n, cols).numpy())
    np.testing.assert_array_equal(m, dr.keep(0.3, (1 << 40) + 7, 3, 5, 7, n, cols))


@pytest.mark.parametrize("f", [13, 259])
def test_an_edgeless_batch(f):
    """five rows without an edge (a batch of one-word pages): the edge arrays are empty tensors, whose device pointer is NULL.  The
    self image is the masked input, the agg image all zeros, dx = D_self(G)."""
    n = 5
    g = sr.Graph([0] * n, [])
    ip = dev(g.indptr)
    ix = torch.empty(0, dtype=torch.int32, device=DEV)
    ew = torch.empty(0, dtype=torch.float32, device=DEV)
    assert _lib.ptr(ix) == 0 and _lib.ptr(ew) == 0
    c = dr.coords(f)
    rng = np.random.default_rng(f)
    x = rng.integers(-8, 9, (n, f)).astype(np.float32)
    for in_drop in (False, True):
        sp, ap = out_image(n, f, True), out_image(n, f, True)
        ops.spmm_dropout_p3(ip, ix, ew, dev(x), n, 0.5, c["seed"], c["rank"], counter(c["step"]), c["site"], in_drop, self_out=sp, agg_out=ap)
        want_s, want_a = dr.producer_expect(g, None, x, 0.5, in_drop=in_drop, **c)
        assert sr.same_bits(decode(sp, "self image"), want_s) and want_s.any()
        got_a = decode(ap, "agg image")
        assert (sr.bits(got_a) == 0).all() and not want_a.any()
    agg_col = dr.c16(f)
    G = dr.exact_grad(n, f, agg_col, 2 * agg_col)
    buf = torch.full((n + 1, dr.c4(f) + 4), SENTINEL, dtype=torch.float32, device=DEV)
    ops.spmm_dropout_bwd(ip, ix, ew, dev(G), agg_col, f, 0.5, c["seed"], c["rank"], counter(c["step"]), c["site"], out=buf[:n, :dr.c4(f)])
    assert bool((buf[n] == SENTINEL).all()) and bool((buf[:n, dr.c4(f):] == SENTINEL).all())
    got = buf[:n, :dr.c4(f)].cpu().numpy()
    m = dr.keep(0.5, c["seed"], c["rank"], c["step"], c["site"], n, 2 * f)
    assert sr.same_bits(got[:, :f], np.where(m[:, :f] == 1, G[:, :f] * np.float32(2), np.float32(0))) and (sr.bits(got[:, f:]) == 0).all()
    assert sr.same_bits(got[:, :f], dr.bwd_expect(g, None, G, agg_col, f, 0.5, **c))


def test_an_edgeless_batch_trains_with_dropout():
    """the same batch through the one-call plan (gte_gcnsage_step hands the plan's edge arrays to both entry points): one step of a
    dropout model on five one-word pages against the float64 reference on the device's masks, as tests/test_gpu_dropout.py does"""
    import gnn_tableextraction_amd as gte
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from oracle import gcnsage_cpu as oc
    from tests import stepcheck as sc, test_gpu_dropout as tgd
    n, f0, hid, ncls, nl, p = 5, 13, 48, 9, 3, 0.5
    none, w = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((n, f0)).astype(np.float32), (np.arange(n) % ncls).astype(np.int64)
    torch.manual_seed(3)
    model = gte.GcnSAGE(f0, hid, ncls, nl, torch.nn.functional.relu, p)
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    eng = FusedGcnSageStep(model, dropout_seed=77, lr=0.01, weight_decay=5e-4)
    g = tgd._graph(none, none, w, x)
    out3 = eng.step(g, torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    ref, grads, drop = tgd._check_step(eng, model, g, oc.OracleGraph(none, none, n, w), x, y, state0, p, None, 0, n, f0)
    assert 0 < drop[1][:, f0:].sum() < drop[1][:, f0:].size
    assert abs(float(out3[0].item()) - ref["loss"]) < sc.LOSS_ATOL, (float(out3[0].item()), ref["loss"])
    sc.assert_grads(grads, ref["grads"], what="edgeless batch: ")
