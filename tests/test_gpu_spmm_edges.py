"""The aggregation kernels (gte_spmm_csr, gte_spmm_csr_accumulate, gte_spmm_csr_p3, gte_spmm_csr_accumulate_ln's z,
gte_spmm_csr_edge, gte_spmm_csr_tiled) through ``ops`` and the C ABI against the float64 reference of tests/spmm_ref.py, on a degree
ladder (every degree 0 ... 200 at which a lane group's edge loop changes shape, twice, on different lane groups), on segment and tile
graphs placed on the edge-parallel and tiled kernels' thresholds, at one width on either side of every dispatch threshold.  Run with
``-m gpu`` on an MI355X; ``-s`` prints every test's worst error / bound ratio.

EXACT cases (integer x, weights 0.5 / 1 / 2: the result is the same in any summation order) are held bit for bit; BOUND cases
(columns scaled by 2^-30 ... 2^30; rows built to cancel to a thousandth of their terms) to
    |got - ref| <= (deg + 4) 2^-24 mag scale_v  [+ half a bf16 ulp of ref]  [+ 2^-24 (|base| + |ref|) accumulating]
both derived in tests/spmm_ref.py and checked by tests/test_spmm_ref_cpu.py against a float32 emulation of the kernel and five mutants
of it.  Every call reads x through a view with ldx = F + 3 one element off the allocation's start, NaN in the padding columns and in
one extra row no edge names, and writes a view into a sentinel-filled buffer: the sentinel outside the view must survive and no NaN may
appear.

NON-FINITE CONFINEMENT (include/gte.h at gte_spmm_csr): +Inf and NaN in one node's row reach that node's out-neighbours only; every
other row is finite and bit for bit what it is with the two values replaced by 0.

MEASURED on an MI355X (all cases of this module), largest error / bound ratio of the bound cases per entry point:
    gte_spmm_csr f32 0.404   gte_spmm_csr_accumulate f32 0.486   gte_spmm_csr_edge 0.411   gte_spmm_csr_tiled 0.460
    gte_spmm_csr bf16 1.000  gte_spmm_csr_accumulate bf16 1.000  (the bf16 bound is all but the half ulp of the output rounding, and
    among a few hundred thousand results some lie next to a tie; the arithmetic in front of it is the f32 kernels')
gte_spmm_csr_p3 and the z of gte_spmm_csr_accumulate_ln have no ratio of their own: bit for bit the fp32 kernels.  Every exact case of
every entry point was bitwise from the first run, the device's 1.0f / (float)deg being the correctly rounded quotient at every degree
of the ladder, and accumulate with mean stayed inside the bound at the degrees that are no power of two.
FAILED BEFORE A FIX: the confinement test for node 0 at F = 13 and 16 through gte_spmm_csr, gte_spmm_csr_accumulate, gte_spmm_csr_p3
and gte_spmm_csr_accumulate_ln (8 cases; at F = 16 89 of the 131 rows, every degree that is no multiple of 4, were NaN without naming
node 0).  The quad-per-row form of spmm_csr_kernel (G = 4) padded a row's last group of four with (node 0, weight 0) and loaded
x[0]; it now pads with the source of the quad's first lane, an edge of the same row.  Node 77, the wider forms, bf16, the
edge-parallel and the tiled kernels confined from the start.  Cost: profiles/HISTORY.md (within 0.02 us of the parent at F = 9, 13,
16 on a 100-page batch).  Nothing else failed, so nothing else was changed.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import spmm_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, cs, check = _lib.ptr, _lib.current_stream, _lib.check
NAN = float("nan")
SENTINEL = 1232.0                      # a bf16 value no case produces
SUM, MEAN = _lib.REDUCE_SUM, _lib.REDUCE_MEAN


def c16(x):
    return -(-x // 16) * 16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class DeviceGraph:
    def __init__(self, g):
        self.g, self.n, self.nnz = g, g.n, g.nnz
        self.ip, self.ix = dev(g.indptr), dev(g.indices)
        self._plan = None

    @property
    def plan(self):
        if self._plan is None:
            self._plan = ops.build_tile_plan(self.ip, self.ix, self.n)
        return self._plan


@functools.lru_cache(maxsize=None)
def graph(name):
    kind, _, arg = name.partition(":")
    g = {"ladder": sr.ladder_graph, "tile": sr.tile_graph, "segment": lambda: sr.segment_graph(int(arg or 0))}[kind]()
    return DeviceGraph(g)


# ---- the harness every call shares -------------------------------------------------------------------------------------------------
def strided(rows, f, dtype, fill):
    """(flat buffer full of ``fill``, view [rows, f] with row stride f + 3 that starts one element into it)"""
    ld = f + 3
    flat = torch.full((1 + rows * ld + 5,), fill, dtype=dtype, device=DEV)
    return flat, flat[1:1 + rows * ld].view(rows, ld)[:, :f]


def x_view(x, dtype=torch.float32, zero_pad=False):
    """x [n_src, f] behind one more row no edge names; NaN in that row and in the padding columns (zeros for the LayerNorm form at
    widths that are no multiple of 4: its contract reads them)"""
    n, f = x.shape
    flat, v = strided(n + 1, f, dtype, 0.0 if zero_pad else NAN)
    v[:n] = dev(x).to(dtype)
    v[n] = NAN
    return v


def out_view(n, f, dtype=torch.float32, base=None):
    flat, v = strided(n, f, dtype, SENTINEL)
    if base is not None:
        v.copy_(dev(base).to(dtype))
    return flat, v


def result(flat, v, allow_nonfinite=False):
    """the view as float32 numpy, after checking that nothing outside it was written and that no NaN appeared inside"""
    n, f = v.shape
    ld = v.stride(0)
    outside = torch.ones_like(flat, dtype=torch.bool)
    outside[1:1 + n * ld].view(n, ld)[:, :f] = False
    assert bool((flat[outside] == SENTINEL).all()), "written outside the output view"
    got = v.float().cpu().numpy()
    assert allow_nonfinite or np.isfinite(got).all(), "a NaN / Inf / untouched NaN reached the output"
    return got


def w_dev(w):
    return None if w is None else dev(w)


def run_row(dg, w, xv, mean, base=None, dtype=torch.float32, allow_nonfinite=False):
    """gte_spmm_csr (base None) / gte_spmm_csr_accumulate"""
    flat, v = out_view(dg.n, xv.shape[1], dtype, base)
    ops.spmm_csr(dg.ip, dg.ix, w_dev(w), xv, dg.n, mean=mean, out=v, accumulate=base is not None)
    return result(flat, v, allow_nonfinite)


def run_tiled(dg, w, xv, mean, base=None, allow_nonfinite=False):
    flat, v = out_view(dg.n, xv.shape[1], torch.float32, base)
    ops.spmm_csr(dg.ip, dg.ix, w_dev(w), xv, dg.n, mean=mean, out=v, accumulate=base is not None, tiles=dg.plan, force_tiled=True)
    return result(flat, v, allow_nonfinite)


def run_p3(dg, w, xv, mean):
    """gte_spmm_csr_p3 into an image pre-filled with 0x55 that has one row more than the graph -> the decoded image [n, c16(f)]"""
    f = xv.shape[1]
    img = ops.P3.empty(dg.n, f, DEV, rows_cap=dg.n + 1)
    img.data.fill_(0x55)
    ops.spmm_csr_p3(dg.ip, dg.ix, w_dev(w), xv, dg.n, mean=mean, out=img)
    assert bool((img.data[dg.n] == 0x55).all()), "written past the image's last row"
    return ops.p3_to_f32(ops.P3(img.data, dg.n, c16(f))).cpu().numpy()


def run_ln_z(dg, w, xv, mean, base):
    """gte_spmm_csr_accumulate_ln -> z (y and the statistics belong to tests/test_gpu_layernorm.py)"""
    lib = _lib.load()
    f = xv.shape[1]
    fp = -(-f // 4) * 4                          # padded rows: the padding of z is written as zeros
    flat, zp = out_view(dg.n, fp)
    z = zp[:, :f]
    z.copy_(dev(base))
    y = torch.empty(dg.n, fp, device=DEV)
    stats = torch.empty(2 * dg.n, device=DEV)
    gamma, beta = torch.ones(f, device=DEV), torch.zeros(f, device=DEV)
    wd = w_dev(w)
    check(lib.gte_spmm_csr_accumulate_ln(P(dg.ip), P(dg.ix), P(wd), P(xv), xv.stride(0), P(z), z.stride(0), dg.n, f,
                                         MEAN if mean else SUM, P(gamma), P(beta), 1e-5, 0, P(y), y.stride(0), P(stats), cs()),
          "gte_spmm_csr_accumulate_ln")
    got = result(flat, zp, allow_nonfinite=True)
    assert (got[:, f:] == 0).all(), "the padding of z must be written as zeros"
    return got[:, :f]


def run_edge(dg, w, xv, mean, allow_nonfinite=False):
    """gte_spmm_csr_edge on a workspace of exactly gte_spmm_csr_edge_workspace_bytes followed by a sentinel"""
    lib = _lib.load()
    f = xv.shape[1]
    nbytes = int(lib.gte_spmm_csr_edge_workspace_bytes(dg.nnz, f))
    ws = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    flat, v = out_view(dg.n, f)
    wd = w_dev(w)
    check(lib.gte_spmm_csr_edge(P(dg.ip), P(dg.ix), P(wd), P(xv), xv.stride(0), P(v), v.stride(0), dg.n, dg.nnz, f,
                                MEAN if mean else SUM, P(ws), nbytes, cs()), "gte_spmm_csr_edge")
    assert bool((ws[nbytes:] == 0xA5).all()), "written past the workspace"
    return result(flat, v, allow_nonfinite)


WORST = {}


def note(entry, r):
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    return r


def report(*entries):
    print("\n    worst error / bound so far: " + "  ".join(f"{e} {WORST[e]:.3f}" for e in entries if e in WORST))


def check_exact(got, g, w, x, mean, base=None, bf16=False, what=""):
    """bit for bit on the rows whose expectation does not depend on an fma contraction, inside the bound on the others"""
    want = sr.expect_exact(g, w, x, mean, base, bf16)
    rows = sr.exact_rows(g, mean, base is not None)
    assert sr.same_bits(got[rows], want[rows]), f"{what}: exact case differs in {int((sr.bits(got) != sr.bits(want))[rows].sum())} elements"
    if not rows.all():
        r = sr.ref(g.indptr, g.indices, w, x, mean, base)
        assert sr.ratio(got, r, sr.bound(g, w, x, mean, r, base, bf16)) <= 1.0, what


def check_bound(entry, got, g, w, x, mean, base=None, bf16=False, what=""):
    r = sr.ref(g.indptr, g.indices, w, x, mean, base)
    q = note(entry, sr.ratio(got, r, sr.bound(g, w, x, mean, r, base, bf16)))
    assert q <= 1.0, f"{what}: error / bound = {q:.3f}"


# ---- the row kernels ---------------------------------------------------------------------------------------------------------------
def _row_kernel_cases(f, bf16):
    dtype = torch.bfloat16 if bf16 else torch.float32
    tag = "bf16" if bf16 else "f32"
    dg = graph("ladder")
    g = dg.g
    for weights in (True, False):
        w, x, base = sr.exact_case(g, f, bf16, weights=weights)
        xv = x_view(x, dtype)
        for mean in (False, True):
            what = f"F={f} {tag} mean={mean} weights={weights}"
            check_exact(run_row(dg, w, xv, mean, None, dtype), g, w, x, mean, None, bf16, "gte_spmm_csr " + what)
            check_exact(run_row(dg, w, xv, mean, base, dtype), g, w, x, mean, base, bf16, "gte_spmm_csr_accumulate " + what)
    for kind in sr.BOUND_KINDS:
        g2, w, x, base = sr.bound_case(g, f, kind, bf16)
        dg2 = dg if g2 is g else DeviceGraph(g2)
        xv = x_view(x, dtype)
        for mean in (False, True):
            for wv in (w, None):
                what = f"F={f} {tag} {kind} mean={mean} weights={wv is not None}"
                check_bound(f"csr_{tag}", run_row(dg2, wv, xv, mean, None, dtype), g2, wv, x, mean, None, bf16, "gte_spmm_csr " + what)
                check_bound(f"accumulate_{tag}", run_row(dg2, wv, xv, mean, base, dtype), g2, wv, x, mean, base, bf16,
                            "gte_spmm_csr_accumulate " + what)
    report(f"csr_{tag}", f"accumulate_{tag}")


@pytest.mark.parametrize("f", sr.F32_WIDTHS)
def test_row_kernels_f32_on_the_degree_ladder(f):
    _row_kernel_cases(f, False)


@pytest.mark.parametrize("f", sr.BF16_WIDTHS)
def test_row_kernels_bf16_on_the_degree_ladder(f):
    _row_kernel_cases(f, True)


@pytest.mark.parametrize("f", sr.P3_WIDTHS)
def test_image_output_is_the_f32_kernel_bitwise(f):
    dg = graph("ladder")
    g = dg.g
    cases = [(dg,) + sr.exact_case(g, f)[:2]]
    for kind in sr.BOUND_KINDS:
        g2, w, x, _ = sr.bound_case(g, f, kind)
        cases.append((dg if g2 is g else DeviceGraph(g2), w, x))
    for i, (d, w, x) in enumerate(cases):
        xv = x_view(x)
        for mean in (False, True):
            for wv in (w, None):
                img = run_p3(d, wv, xv, mean)
                plain = run_row(d, wv, xv, mean)
                assert sr.same_bits(img[:, :f], plain), f"F={f} case {i} mean={mean}: the image differs from gte_spmm_csr"
                assert (sr.bits(img[:, f:]) == 0).all(), f"F={f}: columns F .. the next multiple of 16 must be zeros"
                if i == 0:
                    check_exact(img[:, :f], d.g, wv, x, mean, what=f"gte_spmm_csr_p3 F={f} mean={mean}")


@pytest.mark.parametrize("f", sr.LN_WIDTHS)
def test_accumulate_ln_z_is_accumulate_bitwise(f):
    dg = graph("ladder")
    g = dg.g
    cases = [(dg,) + sr.exact_case(g, f)]
    for kind in sr.BOUND_KINDS:
        g2, w, x, base = sr.bound_case(g, f, kind)
        cases.append((dg if g2 is g else DeviceGraph(g2), w, x, base))
    for i, (d, w, x, base) in enumerate(cases):
        xv = x_view(x)
        for mean in (False, True):
            for wv in (w, None):
                z = run_ln_z(d, wv, xv, mean, base)
                assert sr.same_bits(z, run_row(d, wv, xv, mean, base)), f"F={f} case {i} mean={mean}: z differs from gte_spmm_csr_accumulate"
                if i == 0:
                    check_exact(z, d.g, wv, x, mean, base, what=f"gte_spmm_csr_accumulate_ln F={f} mean={mean}")


@pytest.mark.parametrize("f,rpw", [(260, 1), (13, 16)])
def test_more_than_one_pass_per_block(f, rpw):
    """launch_g gives a block two passes once one pass of 4 waves x RPW rows would make more than 16 blocks per CU: just above
    2 x 4 RPW x 16 x CUs rows (F = 260: one row per wave; F = 13: sixteen), cycling low degrees, an exact case"""
    lib = _lib.load()
    cus = ctypes.c_int()
    wave, lds = ctypes.c_int(), ctypes.c_int()
    name = ctypes.create_string_buffer(64)
    assert lib.gte_device_info(ctypes.byref(cus), ctypes.byref(wave), ctypes.byref(lds), name, 64) == 0
    assert 64 // sr.row_group(f)[0] == rpw
    n = 2 * 4 * rpw * 16 * cus.value + 1
    assert -(-n // (4 * rpw * 2)) >= 16 * cus.value > -(-n // (4 * rpw * 4))          # two passes, not four
    g = sr.cycle_graph(n)
    dg = DeviceGraph(g)
    w, x, base = sr.exact_case(g, f, n_src=sr.LADDER_N)
    xv = x_view(x)
    for mean in (False, True):
        check_exact(run_row(dg, w, xv, mean), g, w, x, mean, what=f"gte_spmm_csr F={f} n={n} mean={mean}")
    check_exact(run_row(dg, w, xv, False, base), g, w, x, False, base, what=f"gte_spmm_csr_accumulate F={f} n={n}")


# ---- the edge-parallel kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", sr.EDGE_WIDTHS)
def test_edge_parallel_kernel_on_segment_boundaries(f):
    for name in ("segment:0", "segment:1", "segment:2", "ladder"):
        dg = graph(name)
        g = dg.g
        for weights in (True, False):
            w, x, _ = sr.exact_case(g, f, weights=weights)
            xv = x_view(x)
            for mean in (False, True):
                check_exact(run_edge(dg, w, xv, mean), g, w, x, mean, what=f"gte_spmm_csr_edge {name} F={f} mean={mean} weights={weights}")
        for kind in sr.BOUND_KINDS:
            g2, w, x, _ = sr.bound_case(g, f, kind)
            dg2 = dg if g2 is g else DeviceGraph(g2)
            xv = x_view(x)
            inside = sr.inside_one_segment(g2)
            for mean in (False, True):
                what = f"gte_spmm_csr_edge {name} F={f} {kind} mean={mean}"
                got = run_edge(dg2, w, xv, mean)
                check_bound("edge", got, g2, w, x, mean, what=what)
                assert sr.same_bits(got, run_edge(dg2, w, xv, mean)), what + ": not reproducible run to run"
                assert sr.same_bits(got[inside], run_row(dg2, w, xv, mean)[inside]), what + ": rows inside one segment differ from gte_spmm_csr"
    report("edge")


# ---- the tiled kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", sr.TILED_WIDTHS)
def test_tiled_kernels_on_their_thresholds(f):
    for name in ("tile", "ladder"):
        dg = graph(name)
        g = dg.g
        if name == "tile":
            assert dg.plan.max_unique == sr.UMAX + 1
            assert (dg.plan.tile_ptr[1:] - dg.plan.tile_ptr[:-1]).cpu().tolist() == [nu for _, nu in sr.tile_facts(g)]
        cases = [(dg, True) + sr.exact_case(g, f), (dg, True) + sr.exact_case(g, f, weights=False)]
        for kind in sr.BOUND_KINDS:
            g2, w, x, base = sr.bound_case(g, f, kind)
            cases.append((dg if g2 is g else DeviceGraph(g2), False, w, x, base))
        for d, exact, w, x, base in cases:
            xv = x_view(x)
            for mean in (False, True):
                for b in (None, base):
                    what = f"gte_spmm_csr_tiled {name} F={f} mean={mean} accumulate={b is not None} exact={exact}"
                    got = run_tiled(d, w, xv, mean, b)
                    assert sr.same_bits(got, run_row(d, w, xv, mean, b)), what + ": differs from the row kernel"
                    if exact:
                        check_exact(got, d.g, w, x, mean, b, what=what)
                    else:
                        check_bound("tiled", got, d.g, w, x, mean, b, what=what)
    report("tiled")


# ---- non-finite confinement --------------------------------------------------------------------------------------------------------
CONFINE = [(e, f, False) for e in ("csr", "accumulate", "p3", "accumulate_ln", "edge", "tiled", "tiled_accumulate") for f in sr.CONFINE_F32_WIDTHS] + \
          [(e, f, True) for e in ("csr", "accumulate") for f in sr.CONFINE_BF16_WIDTHS]


@pytest.mark.parametrize("node", [0, sr.OTHER])
@pytest.mark.parametrize("entry,f,bf16", CONFINE)
def test_a_non_finite_node_reaches_its_out_neighbours_only(entry, f, bf16, node):
    dtype = torch.bfloat16 if bf16 else torch.float32
    dg = graph("ladder")
    g = dg.g
    rng = np.random.default_rng(7000 + f)
    w = rng.uniform(0.5, 1.5, g.nnz).astype(np.float32)                       # strictly positive: 0 x Inf is out of scope
    x = rng.standard_normal((g.n, f)).astype(np.float32)
    base = rng.standard_normal((g.n, f)).astype(np.float32)
    if bf16:
        x, base = sr.bf16_round(x), sr.bf16_round(base)
    c_inf, c_nan = (0, f - 1) if f < 16 else (5, f - 3)                      # a chunk column and a tail (or last-chunk) column
    x0 = x.copy()
    x0[node, [c_inf, c_nan]] = 0.0
    xp = x.copy()
    xp[node, c_inf], xp[node, c_nan] = np.inf, np.nan

    def run(xa):
        xv = x_view(xa, dtype, zero_pad=(entry == "accumulate_ln"))
        if entry == "csr":
            return run_row(dg, w, xv, True, None, dtype, allow_nonfinite=True)
        if entry == "accumulate":
            return run_row(dg, w, xv, True, base, dtype, allow_nonfinite=True)
        if entry == "p3":
            return run_p3(dg, w, xv, True)[:, :f]
        if entry == "accumulate_ln":
            return run_ln_z(dg, w, xv, True, base)
        if entry == "edge":
            return run_edge(dg, w, xv, True, allow_nonfinite=True)
        return run_tiled(dg, w, xv, True, base if entry == "tiled_accumulate" else None, allow_nonfinite=True)
    clean, got = run(x0), run(xp)
    named = g.names(node)
    assert named.any() and (~named & (g.deg % 4 != 0)).any()
    assert np.isfinite(clean).all()
    leaked = ~named & ~np.isfinite(got).all(axis=1)
    assert not leaked.any(), (f"{entry} F={f}: node {node}'s Inf / NaN reached {int(leaked.sum())} rows that do not name it "
                              f"(degrees {sorted(set(g.deg[leaked].tolist()))})")
    assert sr.same_bits(got[~named], clean[~named]), f"{entry} F={f}: rows that do not name node {node} changed"
    assert not np.isfinite(got[named][:, [c_inf, c_nan]]).any(), f"{entry} F={f}: an out-neighbour of node {node} stayed finite"
    others = np.ones(f, dtype=bool)
    others[[c_inf, c_nan]] = False
    assert sr.same_bits(got[named][:, others], clean[named][:, others]), f"{entry} F={f}: the other columns of the out-neighbours changed"
