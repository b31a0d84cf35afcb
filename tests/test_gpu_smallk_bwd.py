"""The one-pass backward of the short-input layer through both of its entry points -- gte_sage_smallk_bwd (csrc/smallk_bwd.hip) and the
epilogue of gte_gemm_p3_nt_smallk_bwd (smallk_bwd_epilogue, csrc/gemm_p3.hip), one per-row arithmetic (csrc/smallk_step.h) -- against
the float64 reference of tests/smallk_ref.py on ill-conditioned rows, at the edges of their templates, tiles and loops.  Run with
``-m gpu`` on an MI355X; ``-s`` shows every case's error / bound ratios.

Both kernels recompute z from the layer's inputs and never store dz, so nothing of theirs can be compared bit for bit.  What is
checked instead (derivations: tests/smallk_ref.py, margins: tests/test_smallk_ref_cpu.py, where a float32 emulation stays inside the
bounds and eight mutants break them by more than 10x):
  * the reference runs on the z that gte_sage_linear_fwd saved and its float32 statistics, so no kappa enters the bounds
        |dz' - dz| <= (2 R + 22) u rstd max|gamma| ||dy_row||_2 (R = 9),  column sums to Kc roundings of the sum of their absolute terms,
        |dW' - dW|_jk <= sum_r B_r |x_rk| + Kc u sum_r (|dz_rj| + B_r) |x_rk|;
  * the mask is float32 fma(xhat, gamma, beta) > 0 on the stored statistics and must equal the forward's y > 0 EVERYWHERE -- nothing is
    neutralised on these inputs; all-zero rows with beta_j == 0 are exact ties and get no gradient.  A backward whose recomputed z
    differed from the forward's in its last bit would move xhat by kappa u (1e-3 on the rows whose mean is 1e4 spreads) and break the
    dW bound there by orders of magnitude;
  * for the epilogue form dy is the device's own gte_gemm_p3_nt product (dyadic operands: exact in any summation order).
Conventions of every call: x and ahn are views with ld = k + 3 and k + 1 that start one element into their allocation, NaN in the
padding columns and in one extra row behind row M - 1; W has ld = K + 2, dy ld = n + 4 (16-byte aligned); outputs go into
sentinel-filled buffers whose sentinel must survive outside the named slices, and no NaN may come out.

Covered: (k1, k2) = (1, 0) .. (14, 14) on both sides of the <16> / <28> instantiations (K = 28 at n = 256 is the largest LDS request),
a2 == NULL, k1 != k2, widths that leave lanes idle (4 .. 252), M around the 2-row step, the 64-row block, the 32-row staging chunk and
the 128-row tile, the grid-stride loop's second trip (M = 512 * 64 + 65), ReLU on and off, each of dgamma / dbeta / dbias NULL, the
fold inside and outside a deferral with lddw = K + 5 in both (the stand-alone kernel's direct fold takes any lddw >= K), the
epilogue's refusal of lddw > K outside one, and every argument error of gte_sage_smallk_bwd with its return code, its message and
untouched outputs.

What failed before the fix.  The first run of this module failed 15 of its 19 tests on the mask assertion, every failure at a width
that is no power of two (n = 100, 200, 252) and on constant rows of z (a zero input row under a constant bias, or (c, 0, ...)): the
forward's y > 0 differed from the mask on the stored statistics at 6 to 105 elements of a case, e.g. at 10 of the 100 elements of
the single row z = 0.5 at n = 100, eps = 1e-12.  There the stored mean was exactly 0.5 and the stored rstd 999937.56 instead of 1e6:
the forward had subtracted an UNROUNDED mean.  sage_smallk_fwd_kernel writes `mean = sum * inv_n` and `z - mean`, and the compiler
contracted the two into fma(-inv_n, sum, z), so xhat was 0.5 - 50 fl(1 / 100) = 1.1e-8 times rstd, which the backward cannot rebuild
from the stats.  z itself was bit-identical; the claim that "the ReLU mask cannot flip" was not.  Fixed in the forward
(gte_ln::ln_mean_rounded, csrc/layernorm.h: the product is rounded before it is subtracted); at n = 2^k, the headline's 256 among
them, 1 / n is exact and no bit of any output changed.  No backward kernel broke a bound, so none was changed.

Measured on an MI355X after the fix (largest error / bound over all cases of this module):
    gte_sage_smallk_bwd          dW 0.030  dgamma 0.084  dbeta 0.064  dbias 0.038
    gte_gemm_p3_nt_smallk_bwd    dW 0.030  dgamma 0.093  dbeta 0.000  dbias 0.011     (dbeta: sums of dyadic dy, exact)
Mask differences between the forward's y > 0 and the reference: 0 of 11 618 816 elements.  Neutralised elements: 0.
"""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import layernorm_cases as lc
from tests import smallk_ref as sk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, cs, check = _lib.ptr, _lib.current_stream, _lib.check
NAN = float("nan")
SENT = 7.0
WORST = {"standalone": [0.0] * 4, "epilogue": [0.0] * 4}
MASKS = {"differ": 0, "elements": 0, "neutralised": 0}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offset_view(a, ld):
    """[m, k] view with leading dimension ld that starts one element into a NaN-filled allocation of m + 1 rows"""
    m, k = a.shape
    buf = torch.full((1 + (m + 1) * ld,), NAN, dtype=torch.float32, device=DEV)
    v = buf[1:].view(m + 1, ld)[:m, :k]
    v.copy_(dev(np.asarray(a, np.float32)))
    return v


def padded(a, ld, extra_row=0):
    m, k = a.shape
    buf = torch.full((m + extra_row, ld), NAN, dtype=torch.float32, device=DEV)
    buf[:m, :k] = dev(np.asarray(a, np.float32))
    return buf


def ld_of(v):
    return v.stride(0)


class Layer:
    """the device side of one case: operands in the module's layout, and the forward's z, y and statistics"""

    def __init__(self, case):
        self.case = case
        self.form, self.k1, self.k2, self.n, self.m, self.relu, self.idx = case
        d = self.d = sk.make_inputs(case)
        k1, k2, n, m = self.k1, self.k2, self.n, self.m
        self.K = k1 + k2
        self.x = offset_view(d["xin"][:, :k1], k1 + 3)
        self.ahn = offset_view(d["xin"][:, k1:], k2 + 1) if k2 else None
        self.Wb = padded(d["W"], self.K + 2)
        self.bias, self.gamma, self.beta = dev(d["bias"]), dev(d["gamma"]), dev(d["beta"])
        self.zb = torch.full((m, n + 4), NAN, device=DEV)
        self.yb = torch.full((m, n + 8), NAN, device=DEV)
        self.stats = torch.full((2 * m,), NAN, device=DEV)
        check(_lib.load().gte_sage_linear_fwd(P(self.x), k1 + 3, k1, P(self.ahn), k2 + 1 if k2 else 0, k2, P(self.Wb), self.K + 2, P(self.bias),
                                              P(self.gamma), P(self.beta), d["eps"], int(self.relu), P(self.zb), n + 4, P(self.stats), P(self.yb),
                                              n + 8, m, n, cs()), "sage_linear_fwd")
        self.z = self.zb.cpu().numpy()[:, :n]
        self.y = self.yb.cpu().numpy()[:, :n]
        st = self.stats.cpu().numpy()
        self.mean, self.rstd = st[:m], st[m:]
        assert np.isfinite(self.z).all() and np.isfinite(self.y).all() and np.isfinite(st).all(), case
        assert bool(torch.isnan(self.zb[:, n:]).all()) and bool(torch.isnan(self.yb[:, n:]).all())
        self.amb = np.zeros((m, n), bool)
        if self.relu:
            m32 = sk.mask32(self.z, self.mean, self.rstd, d["gamma"], d["beta"])
            differ = int(((self.y > 0) != m32).sum())
            MASKS["differ"] += differ
            MASKS["elements"] += m32.size
            assert differ == 0, f"{case}: the forward's y > 0 differs from the mask on the stored statistics at {differ} elements"
            self.amb = sk.ambiguous(self.z, self.mean, self.rstd, d["gamma"], d["beta"])
            tie = lc.zero_rows(self.z)[:, None] & (d["beta"] == 0)[None, :]
            assert (self.y[tie] == 0).all() and not self.amb[tie].any()

    def outputs(self, lddw):
        """sentinel-filled (dW buffer [n + 1, lddw], three [n + 2] buffers whose slices 1 .. n are dgamma, dbeta, dbias)"""
        return torch.full((self.n + 1, lddw), SENT, device=DEV), [torch.full((self.n + 2,), SENT, device=DEV) for _ in range(3)]

    def collect(self, dwb, sums, null=None):
        """the outputs as float64 arrays (None where not asked for), after the sentinel checks"""
        torch.cuda.synchronize()
        n, K = self.n, self.K
        dw = dwb.cpu().numpy()
        assert (dw[n:] == SENT).all() and (dw[:, K:] == SENT).all(), f"{self.case}: dW was written outside [n, K]"
        got = [dw[:n, :K].astype(np.float64)]
        for i, s in enumerate(sums):
            a = s.cpu().numpy()
            assert a[0] == SENT and a[-1] == SENT, f"{self.case}: {sk.NAMES[i + 1]} was written outside its n elements"
            if null == i:
                assert (a == SENT).all()
            got.append(None if null == i else a[1:-1].astype(np.float64))
        assert all(g is None or np.isfinite(g).all() for g in got), f"{self.case}: a non-finite gradient"
        return got

    def judge(self, tag, got, dy):
        r = sk.ratios(self.form, got, dy, self.d["xin"], self.z, self.mean, self.rstd, self.d["gamma"], self.d["beta"], self.relu)
        print(f"{self.form} k=({self.k1}, {self.k2}) n={self.n} M={self.m} relu={int(self.relu)} {tag}: error / bound  "
              + "  ".join(f"{nm} {'-' if v is None else format(v, '.3f')}" for nm, v in zip(sk.NAMES, r)))
        WORST[self.form] = [max(a, b or 0.0) for a, b in zip(WORST[self.form], r)]
        assert all(v is None or v <= 1 for v in r), (self.case, tag, r)
        return r


def in_deferral(fn):
    lib = _lib.load()
    check(lib.gte_fold_defer_begin(cs()), "gte_fold_defer_begin")
    try:
        return fn()
    finally:
        check(lib.gte_fold_defer_flush(), "gte_fold_defer_flush")
        torch.cuda.synchronize()


def report(form):
    print(f"{form}: largest error / bound so far  " + "  ".join(f"{nm} {v:.3f}" for nm, v in zip(sk.NAMES, WORST[form]))
          + f";  mask differences {MASKS['differ']} of {MASKS['elements']} elements, neutralised {MASKS['neutralised']}")


# ------------------------------------------------------------------------------------------------ gte_sage_smallk_bwd
def standalone_args(L, gb, dwb, sums, lddw, ws, ws_bytes, null=None):
    outs = [None if null == i else s[1:] for i, s in enumerate(sums)]                  # (dgamma, dbeta, dbias)
    return [P(gb), ld_of(gb), P(L.x), L.k1 + 3, L.k1, P(L.ahn), L.k2 + 1 if L.k2 else 0, L.k2, P(L.Wb), L.K + 2, P(L.bias), P(L.gamma),
            P(L.beta), P(L.stats), int(L.relu), P(dwb), lddw, P(outs[2]), P(outs[0]), P(outs[1]), L.m, L.n, P(ws), ws_bytes, cs()]


def run_standalone(L, gb, lddw, deferred=False, null=None):
    lib = _lib.load()
    nbytes = int(lib.gte_sage_smallk_bwd_workspace_bytes(L.m, L.K, L.n))
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)              # exactly what the library asks for + a guard
    dwb, sums = L.outputs(lddw)
    call = lambda: check(lib.gte_sage_smallk_bwd(*standalone_args(L, gb, dwb, sums, lddw, ws, nbytes, null)), "gte_sage_smallk_bwd")
    in_deferral(call) if deferred else call()
    got = L.collect(dwb, sums, null)
    assert bool((ws[nbytes:] == 0xA5).all()), f"{L.case}: the workspace was written past its size"
    return got


def check_standalone(case, nulls=False):
    L = Layer(case)
    assert _lib.load().gte_sage_smallk_bwd_supported(L.K, L.n) == 1
    dy, share = lc.neutralise(L.d["dy"], L.amb, L.z)
    MASKS["neutralised"] += int((dy != L.d["dy"]).sum())
    assert share <= lc.AMBIGUOUS_CAP, (case, share)
    gb = padded(dy, L.n + 4, extra_row=1)
    assert gb.data_ptr() % 16 == 0
    got = run_standalone(L, gb, L.K)
    L.judge("direct fold", got, dy)
    L.judge("deferred fold, lddw = K + 5", run_standalone(L, gb, L.K + 5, deferred=True), dy)
    again = run_standalone(L, gb, L.K)                                                  # two runs: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), f"{case}: two runs differ"
    if nulls:
        wide = run_standalone(L, gb, L.K + 5)                                           # the direct fold takes lddw too: the same bits
        assert all(np.array_equal(a, b) for a, b in zip(got, wide)), f"{case}: lddw = K + 5 outside a deferral changed an output"
        for i in range(3):
            part = run_standalone(L, gb, L.K, null=i)
            assert all(b is None or np.array_equal(a, b) for a, b in zip(got, part)), f"{case}: {sk.NAMES[i + 1]} NULL changed another output"


@pytest.mark.parametrize("k1,k2", sk.KLADDER)
def test_standalone_backward_on_ill_conditioned_rows_at_every_edge(k1, k2):
    """sage_smallk_bwd_kernel<16> (K <= 16) and <28>: every M around the 2-row step and the 64-row block at the widths of
    smallk_ref.SA_NS, ReLU on and off, the fold direct and deferred; at M = 65 the direct fold into lddw = K + 5 (legal for this entry
    point outside a deferral too) and dgamma / dbeta / dbias NULL one at a time"""
    for case in sk.cases("standalone", (k1, k2)):
        check_standalone(case, nulls=case[4] == 65)
    report("standalone")


@pytest.mark.parametrize("n", sk.STRIDE_NS)
def test_standalone_backward_takes_a_second_grid_stride_trip(n):
    """M = 512 * 64 + 65: workgroup 0 refills its inputs behind the barrier for rows 32768 .., workgroup 1 for the one row 32832, while
    dy and the statistics of the next step ride in registers; rows of every kind sit at the end of the second trip"""
    check_standalone(sk.stride_case(n))
    report("standalone")


def test_standalone_backward_argument_errors():
    """every refusal of gte_sage_smallk_bwd: its return code, a fragment of gte_last_error, and outputs left alone"""
    lib = _lib.load()
    L = Layer(("standalone", 3, 2, 8, 16, True, 1))
    dy = lc.neutralise(L.d["dy"], L.amb, L.z)[0]
    gb = padded(dy, 12, extra_row=1)
    nbytes = int(lib.gte_sage_smallk_bwd_workspace_bytes(16, 5, 8))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    dwb, sums = L.outputs(L.K)
    base = standalone_args(L, gb, dwb, sums, L.K, ws, nbytes)
    DY, LDDY, A1, LDA1, K1, A2, LDA2, K2, W, LDW, BIAS, GAMMA, BETA, STATS, RELU, DW, LDDW, DBIAS, DGAMMA, DBETA, M, N, WS, WSB, ST = range(25)
    INVALID, TOO_SMALL, UNSUPPORTED = -1, -3, -4
    bad = [("K = 29", {K1: 15, K2: 14}, UNSUPPORTED, b"k1 + k2 <= 28"),
           ("n = 6", {N: 6}, UNSUPPORTED, b"n_out % 4 == 0"), ("n = 260", {N: 260}, UNSUPPORTED, b"n_out <= 256"),
           ("lddy % 4", {LDDY: 13}, INVALID, b"16-byte aligned"), ("dy misaligned", {DY: base[DY] + 4}, INVALID, b"16-byte aligned"),
           ("workspace", {WSB: nbytes - 1}, TOO_SMALL, b"workspace bytes"),
           ("k1 = 0", {K1: 0}, INVALID, b"bad sizes"), ("M < 0", {M: -1}, INVALID, b"bad sizes")]
    bad += [(f"ld {i}", {i: v}, INVALID, b"leading dimension too small") for i, v in ((LDDY, 7), (LDA1, 2), (LDA2, 1), (LDW, 4), (LDDW, 4))]
    bad += [(f"null {i}", {i: 0}, INVALID, b"null pointer") for i in (DY, A1, A2, W, BIAS, GAMMA, BETA, STATS, DW, WS)]
    for what, change, rc, fragment in bad:
        args = list(base)
        for i, v in change.items():
            args[i] = v
        assert lib.gte_sage_smallk_bwd(*args) == rc, what
        assert fragment in lib.gte_last_error(), (what, lib.gte_last_error())
    empty = [0] * 25                                                                    # no rows: OK with nothing looked at
    empty[K1], empty[K2], empty[N], empty[LDDY] = 3, 2, 8, 3
    assert lib.gte_sage_smallk_bwd(*empty) == 0
    torch.cuda.synchronize()
    assert bool((dwb == SENT).all()) and all(bool((s == SENT).all()) for s in sums) and bool((ws == 0).all())
    assert lib.gte_sage_smallk_bwd(*base) == 0                                          # (the unchanged arguments are fine)
    L.judge("after the refusals", L.collect(dwb, sums), dy)


# ------------------------------------------------------------------------------------------------ gte_gemm_p3_nt_smallk_bwd
def run_epilogue(L, a1p, wp, lddw, deferred=False, null=None):
    dwb, sums = L.outputs(lddw)
    outs = [None if null == i else s[1:L.n + 1] for i, s in enumerate(sums)]
    call = lambda: ops.gemm_p3_nt_smallk_bwd(a1p, wp, None, L.x, L.ahn, L.Wb[:, :L.K], L.bias, L.gamma, L.beta, L.stats, L.relu,
                                             dwb[:L.n, :L.K], outs[2], outs[0], outs[1])
    in_deferral(call) if deferred else call()
    return L.collect(dwb, sums, null)


def check_epilogue(case, extras=False):
    L = Layer(case)
    assert _lib.load().gte_gemm_p3_nt_smallk_bwd_supported(L.K, L.n) == 1
    a = L.d["a"].copy()
    rows = L.amb.any(axis=1) & ~lc.const_rows(L.z)
    a[L.amb.any(axis=1)] = 0                                                            # dy cannot be edited: the whole row gets dy = 0
    MASKS["neutralised"] += int(L.amb.any(axis=1).sum()) * L.n
    assert rows.sum() * L.n <= lc.AMBIGUOUS_CAP * L.amb.size, case
    a1p, wp = ops.p3_from_f32(dev(a)), ops.p3_from_f32(dev(L.d["b"]))
    dy = ops.gemm_p3_nt(a1p, wp).cpu().numpy()                                          # the device's own product ...
    assert np.array_equal(dy.astype(np.float64), a.astype(np.float64) @ L.d["b"].astype(np.float64).T)   # ... which is exact
    got = run_epilogue(L, a1p, wp, L.K)
    L.judge("direct fold", got, dy)
    L.judge("deferred fold, lddw = K + 5", run_epilogue(L, a1p, wp, L.K + 5, deferred=True), dy)
    if extras:
        for i in range(3):
            part = run_epilogue(L, a1p, wp, L.K, null=i)
            assert all(b is None or np.array_equal(x, b) for x, b in zip(got, part)), f"{case}: {sk.NAMES[i + 1]} NULL changed another output"
        dwb, sums = L.outputs(L.K + 5)                                                  # outside a deferral dW must be packed
        with pytest.raises(_lib.GteError, match=r"\(-4\).*must be packed"):
            ops.gemm_p3_nt_smallk_bwd(a1p, wp, None, L.x, L.ahn, L.Wb[:, :L.K], L.bias, L.gamma, L.beta, L.stats, L.relu, dwb[:L.n, :L.K],
                                      sums[2][1:L.n + 1], sums[0][1:L.n + 1], sums[1][1:L.n + 1])
        torch.cuda.synchronize()
        assert bool((dwb == SENT).all()) and all(bool((s == SENT).all()) for s in sums)


@pytest.mark.parametrize("k1,k2", sk.KLADDER)
def test_epilogue_backward_on_ill_conditioned_rows_at_every_edge(k1, k2):
    """smallk_bwd_epilogue behind a K = 64 product: every M around the 32-row staging chunk and the 128-row tile at the widths of
    smallk_ref.EP_NS (W^T has stride 256 whatever n), ReLU on and off, the fold direct and deferred; NULL outputs and the refusal
    of lddw > K outside a deferral at M = 129"""
    for case in sk.cases("epilogue", (k1, k2)):
        check_epilogue(case, extras=case[4] == 129)
    report("epilogue")
