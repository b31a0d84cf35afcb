"""The loss and optimiser kernels of the train step against a float64 oracle (tests/lossoptim_ref.py) at their edges:
gte_weighted_ce, the fused head (gte_head_agg_ce + gte_head_dlq_finish), gte_colsum and the three Adam entry points
(gte_adam_step, gte_adam_step_dev, gte_adam_step_dev_images).  The C entry points are called through ``_lib`` directly so that
leading dimensions, alignment and raw pointers are the test's.

Every tolerance is a rounding-error bound derived next to it from the kernel's arithmetic, with eps = 2^-24 (the unit roundoff
of float32), never a figure read off the kernel's output.  Every comparison records error / bound; the largest ratio per
kernel is printed when the module finishes (``pytest -s``).  A ratio above 1 fails.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import lossoptim_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
SENTINEL = 7.5e29                       # what a kernel must neither read (a padding column of an input) nor overwrite
WORST = {}                              # kernel / output -> (largest error / bound seen, the case it was seen in)
BIAS_CORRECTIONS = {"exact": 0, "one_ulp": 0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\nworst error/bound  {k:50s} {WORST[k][0]:.3f}  {WORST[k][1]}", end="")
    print(f"\nbias corrections written by the device: {BIAS_CORRECTIONS}")


def record(name, ratio, case):
    if ratio >= WORST.get(name, (0.0, ""))[0]:
        WORST[name] = (ratio, case)


def within(name, err, bound, case=""):
    """records max(err / bound) under ``name``, then asserts err <= bound elementwise (a zero bound demands a zero error)"""
    err, bound = np.broadcast_arrays(np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64)))
    assert np.isfinite(err).all(), f"{name}: non-finite output"
    ratio = np.zeros(err.shape)
    np.divide(err, bound, out=ratio, where=bound > 0)
    ratio[(bound <= 0) & (err > 0)] = np.inf
    worst = float(ratio.max()) if ratio.size else 0.0
    record(name, worst, case)
    assert worst <= 1.0, f"{name}: error / bound = {worst:.3f} ({case})"


def same_bits(a, b):
    """bit for bit, NaN payloads included (torch.equal calls a NaN unequal to itself)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def dev(a, dtype=None):
    t = torch.as_tensor(a)
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def padded(a, ld, fill=SENTINEL):
    """device buffer [rows, ld] holding ``a`` in its first columns and ``fill`` in the rest"""
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf


# ================================================================ weighted cross-entropy
def make_logits(rng, kind, n, c):
    z = 3 * rng.standard_normal((n, c))
    tied = None
    if kind == "up80":
        z += 80
    elif kind == "down80":
        z -= 80
    elif kind == "spread200":                                            # expf underflows for most classes
        z = rng.uniform(-100, 100, (n, c))
        z[:, 0] = -100
        z[np.arange(n), rng.integers(0, c, n)] = 100
    elif kind == "equal":
        z = np.repeat(np.round(rng.uniform(-3, 3, (n, 1)), 2), c, axis=1)
    elif kind == "ties":                                                 # small integers, the maximum 3 at two or three columns
        z = rng.integers(-3, 3, (n, c)).astype(np.float64)
        tied = np.argsort(rng.random((n, c)), axis=1)[:, :3]
        for k in range(min(3, c)):
            rows = np.arange(n) if k < 2 else np.nonzero(rng.random(n) < 0.5)[0]
            z[rows, tied[rows, k]] = 3
    else:
        assert kind == "normal"
    return z.astype(np.float32), tied


def make_labels(rng, kind, n, c, tied=None):
    y = rng.integers(0, c, n)
    if tied is not None:                                                 # the label is one of the tied maxima: only the first counts
        y = tied[np.arange(n), rng.integers(0, min(2, c), n)]
    outside = np.array([-1, -100, c, c + 7])
    if kind == "some_out":
        out = rng.random(n) < 0.1
        if n > 1:
            out[-1], out[0] = True, False
        y = np.where(out, rng.choice(outside, n), y)
    elif kind == "all_out":
        y = rng.choice(outside, n)
    else:
        assert kind == "valid"
    return y.astype(np.int64)


def make_weights(rng, kind, c, y):
    """class weights (or None) and the labels, which the last kind rewrites: every valid label is the zero-weight class"""
    if kind == "none":
        return None, y
    cw = (0.5 + rng.random(c)).astype(np.float32)
    if kind in ("zero_class", "only_zero_present"):
        cw[c // 2] = 0
        if kind == "only_zero_present":
            y = np.where((y >= 0) & (y < c), c // 2, y)
    else:
        assert kind == "rand"
    return cw, y


def ce_bounds(logits, y, cw, gs, c):
    """Rounding-error bounds of gte_weighted_ce against ref.ce, K = C + 8:

    per node the kernel forms C differences z_j - max and C expf (each exp term <= 1, error absolute in eps), adds them (C - 1
    additions), takes logf, adds the maximum and subtracts the label's logit (two more roundings, each relative to the magnitude of
    its operands: |max|, |lse|, |z_y|), multiplies by the weight, and the block tree and the final division each round once more:
    C + 8 roundings relative to the magnitudes that enter.  So with S = sum_i w_i (|max_i| + |lse_i| + |z_iy|) / sum_w
        |loss - ref| <= K eps S,   |sum_w - ref| <= K eps sum|w|   (sums of non-negative terms: every partial sum <= the total)
    and per element of dlogits, softmax entries being <= 1 with an ABSOLUTE error of (C + a few) eps from the same exp / add chain,
    times the factor w_i grad_scale / sum_w (three more roundings and sum_w's own error):
        |dl_ij - ref| <= K eps |w_i grad_scale / sum_w|."""
    r = ref.ce_rows(logits, y, cw)
    k = c + 8
    sum_w = r["w"].sum()
    if not sum_w > 0:
        return 0.0, 0.0, np.zeros(len(y))
    s = float((r["w"] * (np.abs(r["m"]) + np.abs(r["lse"]) + np.abs(r["zy"]))).sum() / sum_w)
    return k * EPS * s, k * EPS * float(np.abs(r["w"]).sum()), k * EPS * np.abs(r["w"] * gs / sum_w)


def run_weighted_ce(lib, zb, ld, lab, flt, cw, n, c, gs, want_grad, lddl):
    out3 = torch.full((3,), SENTINEL, dtype=torch.float32, device=DEV)
    dl = torch.full((n, lddl), SENTINEL, dtype=torch.float32, device=DEV) if want_grad else None
    ws = torch.empty(int(lib.gte_weighted_ce_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.gte_weighted_ce(_lib.ptr(zb), ld, _lib.ptr(lab), int(flt), _lib.ptr(cw), n, c, gs, _lib.ptr(dl), lddl, _lib.ptr(out3),
                                   _lib.ptr(ws), ws.numel(), _lib.current_stream()), "gte_weighted_ce")
    return out3, dl


# (logits, labels, class weights, grad_scale, float32 labels): every logit kind, label kind, weight kind and grad_scale of the
# issue at least once, and the all-ignored / sum_w == 0 batches with and without weights
CE_SCENARIOS = [
    ("normal", "valid", "none", 1.0, False),
    ("normal", "some_out", "rand", 0.25, True),
    ("up80", "valid", "zero_class", 0.125, False),
    ("down80", "some_out", "rand", 1.0, True),
    ("spread200", "valid", "rand", 0.25, False),
    ("equal", "some_out", "none", 0.125, True),
    ("ties", "valid", "none", 1.0, False),
    ("ties", "some_out", "zero_class", 0.25, True),
    ("normal", "all_out", "rand", 1.0, False),
    ("spread200", "all_out", "none", 0.25, True),
    ("normal", "valid", "only_zero_present", 0.125, True),
    ("up80", "some_out", "only_zero_present", 1.0, False),
]


@pytest.mark.parametrize("c", [1, 2, 9, 13, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 65793])          # 65793 = 256 * 257 + 1: 258 block partials, ce_fold strides
def test_weighted_ce_vs_float64(n, c):
    lib = _lib.load()
    ld, lddl = c + 3, c + 5
    for si, (zkind, ykind, wkind, gs, flt) in enumerate(CE_SCENARIOS):
        rng = np.random.default_rng(1000 * n + 10 * c + si)
        z, tied = make_logits(rng, zkind, n, c)
        cw, y = make_weights(rng, wkind, c, make_labels(rng, ykind, n, c, tied))
        want_loss, want_sw, want_nc, want_dl = ref.ce(z, y, cw, gs)
        b_loss, b_sw, b_dl = ce_bounds(z, y, cw, gs, c)
        zb = padded(z, ld)
        lab = dev(y.astype(np.float32)) if flt else dev(y)
        cwd = None if cw is None else dev(cw)
        out3, dl = run_weighted_ce(lib, zb, ld, lab, flt, cwd, n, c, gs, True, lddl)
        out3_again, dl_again = run_weighted_ce(lib, zb, ld, lab, flt, cwd, n, c, gs, True, lddl)
        out3_nograd, _ = run_weighted_ce(lib, zb, ld, lab, flt, cwd, n, c, gs, False, lddl)
        o, d = out3.cpu().numpy().astype(np.float64), dl.cpu().numpy()
        tag = f"n={n} C={c} {zkind}/{ykind}/{wkind}"
        assert o[2] == want_nc, f"n_correct {o[2]} != {want_nc} ({tag})"
        within("weighted_ce loss", abs(o[0] - want_loss), b_loss, tag)
        within("weighted_ce sum_w", abs(o[1] - want_sw), b_sw, tag)
        within("weighted_ce dlogits", np.abs(d[:, :c].astype(np.float64) - want_dl), b_dl[:, None], tag)
        assert bool((d[:, c:] == np.float32(SENTINEL)).all()), f"dlogits written past column C ({tag})"
        if want_sw == 0:                                                             # all ignored / only zero-weight classes
            assert o[0] == 0 and o[1] == 0 and not d[:, :c].any()
            if ykind == "all_out":
                assert o[2] == 0
        ignored = (y < 0) | (y >= c)
        assert not d[ignored, :c].any()
        assert same_bits(out3, out3_again) and same_bits(dl, dl_again)               # deterministic, bit for bit
        assert same_bits(out3, out3_nograd)                                          # the same fold with and without the gradient


# ================================================================ fused head
def head_graph(rng, n):
    """random multigraph with isolated nodes, a hub with >= 300 in-edges (node 0) and one with >= 300 out-edges (node n - 1); the
    in-edge CSR with its weights and the out-edge CSR with w / in_degree(dst), built on the host"""
    iso = np.zeros(n, dtype=bool)
    if n > 2:
        iso[1:n - 1] = rng.random(n - 2) < 0.1
    ok = np.nonzero(~iso)[0]                                             # no edge touches an isolated node
    pick = lambda k: ok[rng.integers(0, len(ok), k)]
    src = np.concatenate([pick(4 * n), pick(300), np.full(300, n - 1)])
    dst = np.concatenate([pick(4 * n), np.zeros(300, dtype=np.int64), pick(300)])
    w = (0.1 + rng.random(len(src))).astype(np.float32)
    indeg = np.bincount(dst, minlength=n)
    o = np.argsort(dst, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(indeg)]).astype(np.int32)
    o2 = np.argsort(src, kind="stable")
    rindptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int32)
    w_out = (w[o2] / indeg[dst[o2]].astype(np.float32)).astype(np.float32)
    assert indeg[0] >= 300 and np.diff(rindptr)[n - 1] >= 300 and (n < 60 or iso.any())
    return indptr, src[o].astype(np.int32), w[o], rindptr, dst[o2].astype(np.int32), w_out


HEAD_SCENARIOS = [            # labels, class weights, out-edge CSR inside the launch, float32 labels
    ("valid", "rand", True, False),
    ("some_out", "none", False, True),
    ("all_out", "rand", True, True),
    ("some_out", "zero_class", False, False),
    ("valid", "only_zero_present", True, False),
]


@pytest.mark.parametrize("c", [1, 4, 9, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_fused_head_vs_float64(n, c):
    lib, P, st = _lib.load(), _lib.ptr, _lib.current_stream()
    f, gs, ldl = 64, 0.125, c + 3
    rng = np.random.default_rng(100 * n + c)
    indptr, indices, ew, rindptr, rindices, w_out = head_graph(rng, n)
    d_indptr, d_indices, d_ew, d_rindptr, d_rindices, d_wout = (dev(a) for a in (indptr, indices, ew, rindptr, rindices, w_out))
    deg, outdeg = np.diff(indptr), np.diff(rindptr)
    # the output layer's transform on a hidden width of 64: t_self + bias and t_neigh as the head gets them
    h = dev((2 * rng.standard_normal((n, f))).astype(np.float32))
    W = dev((rng.standard_normal((c, 2 * f)) / np.sqrt(f)).astype(np.float32))
    bias = dev(rng.standard_normal(c).astype(np.float32))
    ts, tn = torch.empty((n, c), device=DEV), torch.empty((n, c), device=DEV)
    _lib.check(lib.gte_sage_narrow_fwd(P(h), f, f, P(W), 2 * f, P(bias), c, P(ts), c, P(tn), c, n, st), "gte_sage_narrow_fwd")
    ts_h, tn_h = ts.cpu().numpy(), tn.cpu().numpy()
    k = c + 8
    for ykind, wkind, in_launch, flt in HEAD_SCENARIOS:
        cw, y = make_weights(rng, wkind, c, make_labels(rng, ykind, n, c))
        want = ref.head(indptr, indices, ew, ts_h, tn_h, y, cw, gs, rindptr, rindices, w_out)
        lab = dev(y.astype(np.float32)) if flt else dev(y)
        cwd = None if cw is None else dev(cw)
        lb = padded(ts_h, ldl)
        dlq = torch.full((n, 32), SENTINEL, dtype=torch.float32, device=DEV)
        part = torch.empty(int(lib.gte_head_agg_ce_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        _lib.check(lib.gte_head_agg_ce(P(d_indptr), P(d_indices), P(d_ew), P(tn), c, P(lb), ldl, P(lab), int(flt), P(cwd), n, c,
                                       _lib.REDUCE_MEAN, P(dlq), 32, P(part), part.numel(), st), "gte_head_agg_ce")
        assert bool((lb[:, c:] == SENTINEL).all()) and bool((dlq[:, c:] == SENTINEL).all())
        if not in_launch:                                                 # the caller's q' = A_w^T (norm dl'), columns 16 .. 16 + C
            dlq[:, 16:16 + c] = ops.spmm_csr(d_rindptr, d_rindices, d_wout, dlq[:, :c].contiguous(), n, mean=False)
        img = ops.P3.empty(n, 32, DEV)
        img.data.fill_(0x55)
        out3 = torch.full((3,), SENTINEL, device=DEV)
        gb = torch.full((c,), SENTINEL, device=DEV)
        ws = torch.empty(int(lib.gte_head_dlq_finish_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        csr = (P(d_rindptr), P(d_rindices), P(d_wout)) if in_launch else (None, None, None)
        _lib.check(lib.gte_head_dlq_finish(*csr, P(dlq), 32, n, c, P(part), gs, P(out3), P(img.data), img.ldp, P(gb), P(ws), ws.numel(),
                                           st), "gte_head_dlq_finish")
        got_logits = lb[:, :c].cpu().numpy().astype(np.float64)
        o = out3.cpu().numpy().astype(np.float64)
        image = ops.p3_to_f32(img).cpu().numpy().astype(np.float64)
        got_gb = gb.cpu().numpy().astype(np.float64)
        # logits: a chain of deg fused multiply-adds (each rounds once, relative to the running sum <= sum |terms|), the 1 / deg
        # (one rounding), its product and the addition to t_self: (deg + 3) eps sum|terms|
        b_logit = ((deg + 3) * EPS)[:, None] * want["logits_mag"]
        within("head logits", np.abs(got_logits - want["logits"]), b_logit, f"n={n} C={c}")
        # The CE runs on the DEVICE's float32 logits, the oracle's on its float64 ones: a row's logits off by at most delta_i move
        # its log-sum-exp and its label's logit by at most delta_i each (nll by 2 delta_i) and every softmax entry by a factor
        # exp(+-2 delta_i).  On top of that the bounds of gte_weighted_ce (ce_bounds) with the same K = C + 8: the head runs the
        # same exp / add / logf / weight chain, and alpha = grad_scale / sum_w replaces the per-node factor.
        r = want["rows"]
        delta = b_logit.max(axis=1)
        sw = want["sum_w"]
        if sw > 0:
            s = float((r["w"] * (np.abs(r["m"]) + np.abs(r["lse"]) + np.abs(r["zy"]))).sum() / sw)
            within("head loss", abs(o[0] - want["loss"]), k * EPS * s + 2 * float((r["w"] * delta).sum()) / sw)
        else:
            assert o[0] == 0
        within("head sum_w", abs(o[1] - sw), k * EPS * float(np.abs(r["w"]).sum()))
        # #correct: exact wherever the oracle's arg-max is decided by more than the logits' own error
        z = want["logits"]
        ys = np.where(r["valid"], r["y"], 0)
        zy = z[np.arange(n), ys]
        rest = z.copy()
        rest[np.arange(n), ys] = -np.inf
        sure = r["valid"] & (zy > rest.max(axis=1) + 2 * delta)
        maybe = r["valid"] & (zy >= rest.max(axis=1) - 2 * delta)
        assert int(sure.sum()) <= o[2] <= int(maybe.sum()), (o[2], int(sure.sum()), int(maybe.sum()))
        # image = alpha [dl | q]; per row of dl: (K eps + the softmax's exp(2 delta) - 1) |w_i alpha|
        e_dl = (k * EPS + np.expm1(2 * delta)) * np.abs(r["w"] * want["alpha"])
        within("head image dl", np.abs(image[:, :c] - want["dl"]), e_dl[:, None])
        # q: outdeg fused multiply-adds and the product with alpha, (outdeg + 2) eps sum|terms|, plus the errors of the dl rows it sums
        e_q = np.zeros(n)
        np.add.at(e_q, np.repeat(np.arange(n), outdeg), w_out.astype(np.float64) * e_dl[rindices])
        within("head image q", np.abs(image[:, 16:16 + c] - want["q"]), ((outdeg + 2) * EPS)[:, None] * want["q_mag"] + e_q[:, None])
        assert not image[:, c:16].any() and not image[:, 16 + c:].any()             # columns C .. 15 of each half: exactly 0
        # gbias: 64 lanes by shuffles (6 levels), 4 waves (2), the blocks in order (nb - 1): (7 + nb) eps sum|alpha dl|, plus the rows' errors
        nb = -(-n // 256)
        within("head gbias", np.abs(got_gb - want["gbias"]), (7 + nb) * EPS * np.abs(want["dl"]).sum(axis=0) + e_dl.sum())
        if sw == 0:
            assert not image.any() and not got_gb.any() and not o[:2].any()


# ================================================================ column sums
@pytest.mark.parametrize("cols", [1, 9, 16, 63, 64])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1023, 1024, 1025, 4099])      # 1024 = 256 blocks x 4 waves: the row loop starts to stride
def test_colsum_vs_float64(rows, cols):
    lib, P = _lib.load(), _lib.ptr
    ldx = cols + 1
    for cancel in ((False, True) if cols == 1 else (True,)):
        rng = np.random.default_rng(100 * rows + cols + int(cancel))
        x = rng.standard_normal((rows, cols))
        if cancel:                                                        # a column that cancels: alternating +-1e4 plus a small term
            x[:, cols - 1] = 1e4 * (1 - 2 * (np.arange(rows) % 2)) + 1e-2 * rng.standard_normal(rows)
        x = x.astype(np.float32)
        xb = padded(x, ldx)
        outs = []
        for _ in range(2):
            out = torch.full((cols,), SENTINEL, dtype=torch.float32, device=DEV)
            ws = torch.empty(int(lib.gte_colsum_workspace_bytes(rows, cols)), dtype=torch.uint8, device=DEV)
            _lib.check(lib.gte_colsum(P(xb), ldx, rows, cols, P(out), P(ws), ws.numel(), _lib.current_stream()), "gte_colsum")
            outs.append(out)
        assert same_bits(outs[0], outs[1])
        # a wave adds its rows one after the other (rows_per_thread - 1 additions), the four waves of a block in a tree (2 levels),
        # then the block partials: (rows_per_thread + log2 terms) eps sum|x|, every partial sum being <= sum|x|.  (The fold adds the
        # <= 256 block partials in order, not in a tree: its worst case is nb - 1 roundings; the bound keeps the tighter log2(nb).)
        nb = min(-(-rows // 4), 256)
        rows_per_thread = -(-rows // (4 * nb))
        terms = rows_per_thread + 2 + math.ceil(math.log2(nb))
        within("colsum", np.abs(outs[0].cpu().numpy().astype(np.float64) - ref.colsum(x)), terms * EPS * np.abs(x.astype(np.float64)).sum(axis=0),
               f"rows={rows} cols={cols} terms={terms}")


def test_colsum_refuses_65_columns():
    lib, P = _lib.load(), _lib.ptr
    x, out = torch.zeros((8, 66), device=DEV), torch.zeros(65, device=DEV)
    ws = torch.empty(int(lib.gte_colsum_workspace_bytes(8, 65)) + 4096, dtype=torch.uint8, device=DEV)
    assert lib.gte_colsum(P(x), 66, 8, 65, P(out), P(ws), ws.numel(), _lib.current_stream()) == -1      # GTE_ERR_INVALID_ARGUMENT
    assert lib.gte_colsum(P(x), 66, 8, 64, P(out), P(ws), ws.numel(), _lib.current_stream()) == 0


# ================================================================ Adam
LR, B1, B2, ADAM_EPS = 0.01, 0.9, 0.999, 1e-8
ADAM_SIZES = [1, 3, 4, 5, 4095, 4096, 4097,
              4096 * 31, 4096 * 32, 135168,      # 31 / 32 / 33 workgroups of gte_adam_step_dev: the three sides of the 32 ticket shards
              524293,                            # past the host-scalar kernel's 2048 x 256 threads: its grid-stride loop
              1048581]                           # past gte_adam_step_dev's 256 x 1024 x 4 elements: its grid-stride loop, and a tail


def ulps(a, b):
    return int(abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32))))


def adam_state(wd, gs, t):
    bc1, bc2s = ref.bias_corrections(B1, B2, t)
    return np.array([LR, B1, B2, ADAM_EPS, wd, gs, bc1, bc2s], dtype=np.float32)


def offset_view(a, extra=0):
    """``a`` as a view one element into a larger allocation: 4-byte but not 16-byte aligned"""
    buf = torch.empty(a.numel() + 4 + extra, dtype=a.dtype, device=DEV)
    view = buf[1:1 + a.numel()]
    view.copy_(a)
    assert view.data_ptr() % 16 == 4
    return view


def image_views(n):
    """three sub-matrices of a flat parameter buffer [n]: (offset, rows, cols, ld, transpose) with odd row counts, widths 13 / 16 /
    100 and offsets that are no multiple of 4; the last one ends at the buffer's last element or the one before (the scalar tail)"""
    off3 = n - (8 * 103 + 100)
    off3 -= 1 if off3 % 4 == 0 else 0
    return [(5, 7, 13, 13, 0), (101, 5, 16, 19, 1), (off3, 9, 100, 103, 0)]


def sub_matrix(p, spec):
    off, rows, cols, ld, _ = spec
    return p.as_strided((rows, cols), (ld, 1), p.storage_offset() + off)


def make_images(p, specs):
    """the images of the current parameters (what a training run holds before the step) and their descriptors"""
    imgs = [ops.p3_from_f32(sub_matrix(p, s), transpose=bool(s[4])) for s in specs]
    descs = (_lib.P3Desc * len(specs))(*[
        _lib.P3Desc(p.data_ptr() + 4 * s[0], s[3], img.rows, img.cols, s[4], img.data.data_ptr(), img.ldp) for s, img in zip(specs, imgs)])
    return imgs, descs


class AdamLaunch:
    """one gte_adam_step_dev[_images] launch on copies of (p, g, m, v) with its own state / counter / ticket, and the checks every
    such launch must pass: the counter advanced by exactly one, the ticket back to zero, state[0..5] untouched, state[6..7] the bias
    corrections of step t + 1"""

    def __init__(self, lib, start, g, state, t, unaligned=False, images=None):
        self.lib, self.t = lib, t
        conv = offset_view if unaligned else (lambda a: a.clone())
        self.p, self.m, self.v = (conv(a) for a in start)
        self.g = conv(g)
        self.state_before = np.array(state, dtype=np.float32)
        self.state = dev(self.state_before.copy())
        self.counter = torch.tensor([t - 1], dtype=torch.int64, device=DEV)
        self.ticket = torch.zeros(int(lib.gte_adam_ticket_bytes()) // 4, dtype=torch.int32, device=DEV)
        self.images = images
        self.wrote = None

    def run(self):
        lib, P, n = self.lib, _lib.ptr, self.p.numel()
        args = (P(self.p), P(self.g), P(self.m), P(self.v), n, P(self.state), P(self.counter), P(self.ticket))
        if self.images is None:
            _lib.check(lib.gte_adam_step_dev(*args, _lib.current_stream()), "gte_adam_step_dev")
        else:
            specs = self.images
            self.imgs, descs = make_images(self.p, specs) if specs else ([], None)
            wrote = ctypes.c_int(-1)
            _lib.check(lib.gte_adam_step_dev_images(*args, ctypes.addressof(descs) if specs else None, len(specs), ctypes.byref(wrote),
                                                    _lib.current_stream()), "gte_adam_step_dev_images")
            self.wrote = wrote.value
        self.check_state()
        return self

    def check_state(self):
        assert int(self.counter.item()) == self.t                           # advanced by exactly 1
        assert not self.ticket.any()                                        # every word of the ticket back to 0
        after = self.state.cpu().numpy()
        assert after[:6].tobytes() == self.state_before[:6].tobytes()       # the hyper-parameters are only read
        for got, want in zip(after[6:], ref.bias_corrections(B1, B2, self.t + 1)):
            d = ulps(got, np.float32(want))
            assert d <= 1, f"bias correction for step {self.t + 1}: {got!r} vs {np.float32(want)!r}"
            BIAS_CORRECTIONS["exact" if d == 0 else "one_ulp"] += 1
        self.state_after = after

    def same_bits(self, other):
        return all(same_bits(a, b) for a, b in ((self.p, other.p), (self.m, other.m), (self.v, other.v)))


def adam_bounds(p0, g, m0, v0, t, wd, gs):
    """Rounding-error bounds of ONE Adam step against ref.adam started from the same float32 (p, m, v).

    g' = fmaf(wd, p, gs g): gs is a power of two here (1, 1/8), so gs g is exact and g' rounds ONCE, relative to g' itself even
    where wd p and gs g cancel.  1 - b1 and 1 - b2 are exact in float32 (b within a factor 2 of 1).
    m = fmaf(b1, m, (1 - b1) g'): g' (1), the product (1), the fmaf (1) -- at most 3 eps <= 4 eps, relative to |b1 m| + |(1 - b1) g'|
        (the two terms can cancel, so the magnitudes and not |m| are the scale);
    v = fmaf(b2, v, (1 - b2) g' g'): every term is non-negative, so the bound is relative to v.  With wd == 0, g' = gs g is exact:
        two products and the fmaf, 3 eps <= the 4 eps the bound was set at.  With wd != 0 the rounding of g' enters TWICE (g' g'):
        2 + 2 + 1 = 5 roundings, and they do line up among a million elements (a float32 emulation of these five operations
        reaches 4.5 eps), so 4 eps missed that term: 5 eps there.  The ratio against 4 eps is recorded as well, not asserted;
    p = p - (lr / bc1) (m / denom), denom = sqrtf(v) / bc2_sqrt + eps, division and sqrtf correctly rounded:
        the final subtraction rounds relative to the larger of |p|, |p_new|: eps max(|p|, |p_new|);
        the update term carries m's error (above) and, relative to |m / denom|: v's 4 eps halved by the root (2), sqrtf (1), the
        division by bc2_sqrt (1), bc2_sqrt itself as a float32 that may be one ulp off (1 + 2), + eps (1), m / denom (1), lr / bc1
        (1) with bc1 a float32 that may be one ulp off (1 + 2), the product (1): K = 14."""
    lr, b1, b2, eps, wd, gs = (float(np.float32(x)) for x in (LR, B1, B2, ADAM_EPS, wd, gs))
    p0, g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p0, g, m0, v0))
    p1, m1, v1 = ref.adam(p0, g, m0, v0, t, LR, B1, B2, ADAM_EPS, wd, gs)
    bc1, bc2s = ref.bias_corrections(B1, B2, t)
    gi = gs * g + wd * p0
    b_m = 4 * EPS * (np.abs(b1 * m0) + np.abs((1 - b1) * gi))
    b_v = (4 if wd == 0 else 5) * EPS * v1
    denom = np.sqrt(v1) / bc2s + eps
    b_p = EPS * np.maximum(np.abs(p0), np.abs(p1)) + (lr / bc1) * (b_m + 14 * EPS * np.abs(m1)) / denom
    return (p1, m1, v1), (b_p, b_m, b_v)


def adam_gradient(rng, n, zero):
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 12, n)).astype(np.float32)     # g^2 stays a normal float32
    g[zero] = 0
    return g


ADAM_CASES = [(n, wd, gs) for n in ADAM_SIZES for wd, gs in ((0.0, 0.125), (5e-4, 1.0))] + \
             [(n, wd, gs) for n in ADAM_SIZES if n <= 4097 for wd, gs in ((0.0, 1.0), (5e-4, 0.125))]


@pytest.mark.parametrize("n,wd,gs", ADAM_CASES)
def test_adam_entry_points_vs_float64(n, wd, gs):
    """Five consecutive steps from t = 1 (the device advances its own state), then single steps at t = 1000 and 100000 (the test
    writes the state).  Before every step the oracle restarts from the device's float32 (p, m, v): a bound is one step's rounding."""
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(n + int(1e4 * wd) + int(8 * gs))
    zero = slice(n // 2, n // 2 + min(64, n // 3))                       # g = 0, m = v = 0: the update is exactly 0 when wd == 0
    p0 = rng.standard_normal(n).astype(np.float32)
    start = [dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    specs = image_views(n) if n >= 4095 else None
    state = adam_state(wd, gs, 1)
    for t in (1, 2, 3, 4, 5, 1000, 100000):
        if t >= 1000:
            state = adam_state(wd, gs, t)
        g_h = adam_gradient(rng, n, zero)
        g = dev(g_h)
        start_h = [a.cpu().numpy() for a in start]
        main = AdamLaunch(lib, start, g, state, t).run()
        # the host-scalar kernel on the same inputs and step: the same arithmetic, so (behind the comparison with the oracle) the same
        # bits (p: where the device's state holds the float32 of the host's bias corrections -- always for a state the test wrote)
        hp, hm, hv = (a.clone() for a in start)
        _lib.check(lib.gte_adam_step(P(hp), P(g), P(hm), P(hv), n, LR, B1, B2, ADAM_EPS, wd, t, gs, _lib.current_stream()), "gte_adam_step")
        # against the oracle, from the device's own float32 start
        (p1, m1, v1), (b_p, b_m, b_v) = adam_bounds(*([start_h[0], g_h] + start_h[1:]), t, wd, gs)
        got = [a.cpu().numpy() for a in (main.p, main.m, main.v)]
        case = f"n={n} wd={wd} gs={gs} t={t}"
        for name, kernel_p in (("adam_step_dev", got[0]), ("adam_step", hp.cpu().numpy())):
            within(f"{name} p", np.abs(kernel_p.astype(np.float64) - p1), b_p, case)
        within("adam m", np.abs(got[1].astype(np.float64) - m1), b_m, case)
        within("adam v", np.abs(got[2].astype(np.float64) - v1), b_v, case)
        if wd != 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                r4 = np.nan_to_num(np.abs(got[2].astype(np.float64) - v1) / (4 * EPS * v1)).max()
            record("adam v, wd != 0, against 4 eps (not asserted)", float(r4), case)
        assert same_bits(hm, main.m) and same_bits(hv, main.v)
        if state[6:].tobytes() == adam_state(wd, gs, t)[6:].tobytes():
            assert same_bits(hp, main.p)
        # unaligned buffers (n4 = 0: the scalar loop does everything), the images entry point without images, with three, with 13
        variants = [AdamLaunch(lib, start, g, state, t, unaligned=True).run(), AdamLaunch(lib, start, g, state, t, images=[]).run()]
        assert variants[1].wrote == 0
        if specs:
            variants += [AdamLaunch(lib, start, g, state, t, images=specs).run(),
                         AdamLaunch(lib, start, g, state, t, unaligned=True, images=specs).run(),
                         AdamLaunch(lib, start, g, state, t, images=[specs[0]] * 13).run()]
            assert variants[2].wrote == 1 and variants[3].wrote == 1 and variants[4].wrote == 0
            for launch in variants[2:4]:                                  # byte for byte the conversion of the updated sub-matrix
                for spec, img in zip(specs, launch.imgs):
                    fresh = ops.p3_from_f32(sub_matrix(launch.p, spec), transpose=bool(spec[4]))
                    assert torch.equal(img.data, fresh.data), f"image of sub-matrix {spec} at step {t}"
        for launch in variants:
            assert launch.same_bits(main) and launch.state_after.tobytes() == main.state_after.tobytes()
        if wd == 0:
            assert got[0][zero].tobytes() == start_h[0][zero].tobytes() and not got[1][zero].any() and not got[2][zero].any()
        start, state = [main.p, main.m, main.v], main.state_after
