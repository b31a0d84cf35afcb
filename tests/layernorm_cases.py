"""Inputs, error bounds and a float32 emulation for the LayerNorm(+ReLU) tests (tests/test_layernorm_ref_cpu.py without a GPU,
tests/test_gpu_layernorm.py on one).  Test infrastructure, numpy only.

Notation: u = 2^-24 (half a float32 ulp, the relative error of one rounding), S = max_j |z_j| of a row, kappa = S / sqrt(var + eps)
(layernorm_ref.kappa), xhat = (z - mean) rstd in exact arithmetic on the float32 row.

R, the row-sum depth of a kernel family: the number of float32 additions an element passes through on its way into a row sum.
Every kernel sums a lane's elements in a chain and the lanes in a tree:
  scalar   ln_relu_fwd_kernel, ln_relu_bwd_kernel<NCH>, ln_relu_bwd_wide_kernel: lane l owns columns l + 64 t, a chain of
           ceil(n / 64) terms, then the 6-level wave tree:                                     R = ceil(n / 64) - 1 + 6
  vec      ln_relu_fwd_vec_kernel<NV, RF, MSK> (both forms: per-chunk validity at n % 4 == 0, per-element validity on padded rows),
           ln_relu_bwd_vec_kernel<NV> and ln_relu_bwd_gen_kernel<NV, RF> (the same two forms as two kernels): lane l owns the
           four columns 4 (l + 64 v) .. + 3 for every v, a chain of 4 ceil(n / 256) terms, the same tree:                       R = 4 ceil(n / 256) - 1 + 6
  spmm     the LNE epilogue of spmm_csr.hip at (G, CPL): 4 CPL terms per lane, log2 G tree levels
  narrow   the LNF kernels of narrow_layer.hip: groups of four ((x + y) + (z + w), 2 levels) in a chain, then cross-lane adds.  The
           256-thread kernel (n % 16 != 0): n / 8 groups, one add: R = n / 8 + 3; the 512-thread kernel: n / 16 groups, two adds:
                                                                                               R = n / 16 + 4
  tile     the epilogue of gemm_p3.hip and sage_smallk_fwd_kernel: four terms per lane (n <= 256), the tree:   R = 3 + 6

Forward.  The row sum errs by at most R u sum_j |z_j| <= R u n S; times 1 / n (the reciprocal and the product, or one division,
round once each): |mean' - mean| = dm <= Dm u S with Dm = R + 2.  The deviations d'_j = z_j - mean' all carry the SAME shift dm
(plus one rounding of their own), and sum_j d_j = 0, so sum_j (d_j - dm)^2 = sum_j d_j^2 + n dm^2: the computed variance is
(var + dm^2)(1 + e), where e collects the rounding of d' (twice, it is squared), the R + 1 roundings of the fused multiply-add chain
and tree, the reciprocal, the product and the addition of eps: |e| <= (R + 6) u.  The square root halves that, rsqrt adds two (one
ulp): with t = dm^2 / (var + eps) <= (Dm u kappa)^2
    |rstd' / rstd - 1| <= Dr u + min(1, t / 2) (1 + Dr u),   Dr = R / 2 + 5                                   (rstd_bound)
(the second term is the variance the mean's own error adds; it is what makes rstd, and with it xhat, meaningless on a constant
row whose |c| u exceeds sqrt(eps) -- the bound says so instead of hiding it).  Then
    xhat' - xhat = d_j (rstd' - rstd) - dm rstd' + roundings (the subtraction, u |xhat|; the product, u |xhat|)
    |xhat' - xhat| <= u [ Dm kappa + |xhat| (Dr + Dm kappa) + 2 |xhat| ]      (min(1, x^2 / 2) <= x for the second-order term)
                   <= D u (1 + kappa) max(1, |xhat|),   D = 2 Dm + Dr + 2 + 1 = 2.5 R + 12   (the + 1: products of two error terms)
and pre' = fma(xhat', gamma, beta) rounds once more, which max(., 0) does not enlarge:
    |y' - y| <= D u |gamma_j| (1 + kappa) max(1, |xhat_j|) + 2^-23 |y_j|                                      (fwd_bound)
    |mean' - mean| <= Dm u S                                                                                (mean_bound)

Backward, reference evaluated on the device's z and the device's float32 stats, so xhat' = fl(fl(z - mean) rstd) is within 2 u |xhat|
of the reference's and NO kappa enters: with G_j = g_j gamma_j, c1 = mean_j G_j, c2 = mean_j G_j xhat_j,
dz_j = rstd ((G_j - c1) - xhat_j c2):
    c1 errs by (R + 3) u mean|G| (G rounded, the sum, the reciprocal, the product), c2 by (R + 6) u mean|G xhat|;
    the five operations of dz_j add 4 u |G_j| + 3 u |c1| + 5 u |xhat_j c2|;
    |G_j|, |c1| and |xhat_j| mean|G xhat| are each at most gmax ||dy_row||_2 (Cauchy-Schwarz with ||xhat||_2 <= sqrt(n)), so
    |dz' - dz| <= Db u rstd max_j|gamma_j| ||dy_row||_2,   Db = 4 + (R + 6) + (R + 11) + 1 = 2 R + 22          (bwd_bound)
The issue that asked for these tests expected a kappa factor here; with the statistics handed in there is none, and the bound
without it is the tighter one.  Column sums over the M rows (colsum_roundings): a wave's chain over its rows, the four waves, the
fold of the block partials -- each at most Kc roundings of the sum of the absolute terms.

ReLU.  Elements whose float64 |pre| is within BAND_FACTOR = 2 forward bounds of zero are "ambiguous": a float32 evaluation may land
on the other side.  The tests give them dy = 0, so that no mask choice moves a gradient, and require the forward's y > 0 to equal
the reference mask everywhere else.  Exactly zero rows are exempt: every kernel computes mean = 0, xhat = 0 and pre = beta_j there
without a rounding, so pre == 0 exactly where beta_j == 0 -- the planted exact tie, which must get no gradient.
"""
import numpy as np

from tests import layernorm_ref as ref

U = 2.0 ** -24
BAND_FACTOR = 2.0
AMBIGUOUS_CAP = 0.01                         # share of a case's elements that may be neutralised (constant rows not counted)

MS = [1, 3, 8, 9, 65]
M_BIG = 4 * 512 * 2 + 5                      # the backward's grid-stride loop and its 512-block cap take a second trip
FWD_SCALAR_NS = [1, 3, 63, 64, 65, 127, 516, 1023, 1024, 1025, 1100]
FWD_VEC_NS = [128, 252, 256, 260, 512]
GEN_NS = [1, 5, 100, 218, 250, 256, 257, 500, 512, 513, 768, 769, 1000, 1024]
BWD_NCH_NS = [1, 64, 65, 126, 129, 255, 513, 1023]
BWD_VEC_NS = FWD_VEC_NS
BWD_WIDE_NS = [1025, 1100]

OFFSETS = {"off1e2": (1e2, 1.0), "off1e3": (1e3, 1.0), "off1e4": (1e4, 1.0), "off1_1e-3": (1.0, 1e-3)}
CONSTANTS = {"const0.75": 0.75, "const-3": -3.0, "const1000": 1000.0}
KINDS = list(OFFSETS) + list(CONSTANTS) + ["zero", "tiny", "single"]


def ceil_div(a, b):
    return -(-a // b)


def depth(family, n, g=64, cpl=1):
    """R of the module docstring"""
    if family == "scalar":
        return ceil_div(n, 64) - 1 + 6
    if family == "vec":
        return 4 * ceil_div(n, 256) - 1 + 6
    if family == "spmm":
        return 4 * cpl - 1 + int(np.log2(g))
    if family == "narrow":
        return n // 16 + 4 if n % 16 == 0 else n // 8 + 3
    if family == "tile":
        return 3 + 6
    raise ValueError(family)


def standalone_family(n, image):
    """row-sum family of the stand-alone kernel that runs width n, forward and backward alike (gte_ln_relu_fwd(_p3), ln_relu_bwd_impl
    of layernorm.hip): the entry points with a P3 image run the 16-byte (vec) kernels at every width, the others at n % 4 == 0 in
    128 .. 512 and the scalar kernels elsewhere"""
    return "vec" if image or (n % 4 == 0 and 128 <= n <= 512) else "scalar"


def spmm_group(n_feat, image):
    """(G, CPL) of the LNE instantiation that runs n_feat columns (spmm_csr.hip accumulate_ln_impl)"""
    nchunk = ceil_div(n_feat, 16 if image else 4) * (4 if image else 1)
    for lim, gc in ((4, (4, 1)), (8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2))):
        if nchunk <= lim:
            return gc
    return 64, 4


def consts(r):
    """(D, Dm, Dr, Db) for a row-sum depth r"""
    return 2.5 * r + 12, r + 2, r / 2 + 5, 2 * r + 22


def fwd_bound(r, z, gamma, eps, xhat, y_ref):
    """elementwise bound on |y - y_ref|; xhat and y_ref from layernorm_ref.fwd on the same z"""
    d = consts(r)[0]
    k = ref.kappa(z, eps)
    return d * U * np.abs(np.asarray(gamma, np.float64)) * (1 + k)[:, None] * np.maximum(1.0, np.abs(xhat)) + 2 * U * np.abs(y_ref)


def mean_bound(r, z):
    return consts(r)[1] * U * np.abs(np.asarray(z, np.float64)).max(axis=1)


def rstd_bound(r, z, eps):
    """bound on |rstd' / rstd - 1| per row"""
    _, dm, dr, _ = consts(r)
    t = (dm * U * ref.kappa(z, eps)) ** 2
    return dr * U + np.minimum(1.0, t / 2) * (1 + dr * U)


def bwd_bound(r, dy, rstd, gamma):
    """per-row bound on |dz - dz_ref|, the reference on the same z and stats"""
    dy = np.asarray(dy, np.float64)
    return consts(r)[3] * U * np.asarray(rstd, np.float64) * np.abs(gamma).max() * np.sqrt((dy * dy).sum(axis=1))


LNB_MAX_BLOCKS = 512


def colsum_roundings(m):
    """Kc: a wave's chain over the rows it owns, the 4 waves of a block, the fold's slice chain and its 16 slices, and 3 for the
    float32 term itself (xhat' and the multiply-add)"""
    nb = min(ceil_div(m, 4), LNB_MAX_BLOCKS)
    return ceil_div(m, 4 * nb) + 3 + ceil_div(nb, 16) + 16 + 3


def band(r, z, gamma, beta, eps):
    """elementwise |pre| band of the ambiguous elements: BAND_FACTOR forward bounds"""
    _, pre, mean, rstd = ref.fwd(z, gamma, beta, eps, False)
    xhat = (np.asarray(z, np.float64) - mean[:, None]) * rstd[:, None]
    return BAND_FACTOR * fwd_bound(r, z, gamma, eps, xhat, pre)


# ------------------------------------------------------------------------------------------------ inputs
def variants(m):
    """row -> planted kind.  Over the variants of a row count every kind is planted and (M > 1) ordinary N(0, 1) rows remain.  The
    kappa = 1e4 rows (some 5 % of THEIR elements are ambiguous) are planted only where the other rows dilute them below the cap."""
    if m == 1:
        return [{}] + [{0: k} for k in KINDS if k != "off1e4"]
    if m == 3:
        return [{0: "off1e3", 2: "zero"}, {1: "const-3", 2: "tiny"}, {0: "single", 1: "off1_1e-3"}]
    if m == 8:
        return [{0: "off1e3", 2: "const0.75", 3: "zero", 5: "single", 7: "off1_1e-3"}]
    if m == 9:
        return [{8: "off1e2", 4: "const1000", 0: "tiny", 1: "zero", 6: "off1e3"}]
    plant = {m - 1: "off1e4", 0: "off1e3", 1: "off1e2", 2: "off1_1e-3", 3: "const0.75", 4: "const-3", 5: "const1000", 6: "zero",
             7: "tiny", 8: "single", m - 2: "zero", m // 2: "single"}
    if m > 4096:
        plant.update({2048: "zero", 2049: "off1e4", 4096: "const1000", m - 3: "tiny"})
    return [plant]


def make_params(n, rng, unit=False):
    """gamma with mixed signs and one exact zero, beta with exact zeros at some columns (never where gamma is zero: that column
    would be an exact tie on EVERY row); unit: gamma = 1, beta = 0 throughout (the initial parameters)"""
    if unit:
        return np.ones(n, np.float32), np.zeros(n, np.float32)
    gamma = (rng.uniform(0.5, 1.5, n) * np.where(rng.random(n) < 0.4, -1.0, 1.0)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(n)).astype(np.float32)
    beta[np.abs(beta) < 0.01] = np.float32(0.01)
    beta[1::5] = 0
    if n >= 3:
        gamma[n // 3] = 0
        beta[n // 3] = np.float32(0.25)
    return gamma, beta


def plant_rows(z, plant, rng):
    """overwrite the planted rows of z in place"""
    n = z.shape[1]
    for row, kind in plant.items():
        if kind in OFFSETS:
            mean, std = OFFSETS[kind]
            z[row] = (mean + std * rng.standard_normal(n)).astype(np.float32)
        elif kind in CONSTANTS:
            z[row] = np.float32(CONSTANTS[kind])
        elif kind == "zero":
            z[row] = 0
        elif kind == "tiny":
            z[row] = (1e-6 * rng.standard_normal(n)).astype(np.float32)
        elif kind == "single":
            z[row] = 0
            z[row, int(rng.integers(0, n))] = np.float32(rng.uniform(0.5, 2.0) * (1 if rng.random() < 0.5 else -1))
        else:
            raise ValueError(kind)
    return z


def make_case(m, n, plant, seed, unit=False):
    """(z, dy, gamma, beta): planted rows among N(0, 1) rows; dy ~ N(0, 1).  In a small matrix ONE ambiguous element is already more
    than AMBIGUOUS_CAP of it, so a small case is drawn again (same generator: deterministic) until the reference's own statistics
    find at most half the cap ambiguous, at eps = 1e-5 and 1e-12 and the deeper of the two stand-alone row-sum families."""
    rng = np.random.default_rng(seed)
    r = max(depth("scalar", n), depth("vec", n))
    for _ in range(200):
        z = rng.standard_normal((m, n)).astype(np.float32)
        dy = rng.standard_normal((m, n)).astype(np.float32)
        gamma, beta = make_params(n, rng, unit)
        plant_rows(z, plant, rng)
        if m * n > 8192:
            break
        worst = 0.0
        for eps in (1e-5, 1e-12):
            e32 = float(np.float32(eps))
            _, _, mean, rstd = ref.fwd(z, gamma, beta, e32, False)
            worst = max(worst, neutralise(dy, ref.ambiguous(z, mean, rstd, gamma, beta, band(r, z, gamma, beta, e32)), z)[1])
        if worst <= AMBIGUOUS_CAP / 2:
            break
    else:
        raise AssertionError(f"no draw of case M={m} n={n} {plant} stays under the ambiguous cap")
    return z, dy, gamma, beta


def const_rows(z):
    """rows whose entries are all one non-zero value (every row of a one-column matrix): xhat is 0 in exact arithmetic and whatever
    the rounding of the mean leaves on a device"""
    return (z == z[:, :1]).all(axis=1) & (z[:, 0] != 0)


def zero_rows(z):
    return (z == 0).all(axis=1)


def cases(ns, big_n=None):
    """(m, n, vi, plant, eps, unit, seed) of one kernel family's widths: every width at every M; eps alternates between 1e-5 and 1e-12
    (both at M = 1 and M = 65); the unit parameters ride on one variant per width; M_BIG at ``big_n`` only."""
    out = []
    for n in ns:
        for m in MS + ([M_BIG] if n == big_n else []):
            for vi, plant in enumerate(variants(m)):
                both = m == 65 or (m == 1 and plant and next(iter(plant.values())) in ("const1000", "const0.75", "zero", "tiny"))
                for ei, eps in enumerate((1e-5, 1e-12) if both else ((1e-5, 1e-12)[(n + m + vi) % 2],)):
                    unit = (m == 8) or (m == 1 and plant.get(0) == "zero" and ei == 1)
                    out.append((m, n, vi, plant, eps, unit, 100000 * ei + 1000 * n + 10 * m + vi))
    return out


def neutralise(dy, amb, z):
    """dy with the ambiguous elements zeroed -- zero rows exempt (exact, module docstring); returns (dy', share of the case's elements
    that were neutralised outside constant rows)"""
    amb = amb.copy()
    amb[zero_rows(z)] = False
    out = np.where(amb, np.float32(0), dy)
    counted = amb.copy()
    counted[const_rows(z)] = False
    return out, float(counted.sum()) / counted.size


# ------------------------------------------------------------------------------------------------ float32 emulation
F32 = np.float32


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _lane_terms(x, layout):
    """the sequence of [M, 64] terms a wave adds up: terms[k][:, l] is lane l's k-th element (zeros where the row has ended)"""
    m, n = x.shape
    if layout == "scalar":
        t = ceil_div(n, 64)
        p = np.zeros((m, 64 * t), F32)
        p[:, :n] = x
        p = p.reshape(m, t, 64)
        return [p[:, k, :] for k in range(t)]
    nv = ceil_div(n, 256)
    p = np.zeros((m, 256 * nv), F32)
    p[:, :n] = x
    p = p.reshape(m, nv, 64, 4)
    return [p[:, v, :, e] for v in range(nv) for e in range(4)]


def _tree(acc):
    for _ in range(6):                       # lane ^ 1, ^ 2, ^ 4, ^ 8, then (r0 + r1) + (r2 + r3): a pairwise tree
        acc = (acc[:, 0::2] + acc[:, 1::2]).astype(F32)
    return acc[:, 0]


def row_sum(x, layout, sequential=False):
    if sequential:
        acc = np.zeros(x.shape[0], F32)
        for j in range(x.shape[1]):
            acc = (acc + x[:, j]).astype(F32)
        return acc
    acc = np.zeros((x.shape[0], 64), F32)
    for t in _lane_terms(x, layout):
        acc = (acc + t).astype(F32)
    return _tree(acc)


def row_dot(a, b, layout):
    """sum_j a_j b_j as the kernels do it: q = fma(a, b, q) along the lane's chain, then the tree"""
    acc = np.zeros((a.shape[0], 64), F32)
    for ta, tb in zip(_lane_terms(a, layout), _lane_terms(b, layout)):
        acc = fma(ta, tb, acc)
    return _tree(acc)


def _rsqrt(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (1.0 / np.sqrt(x.astype(np.float64))).astype(F32)


FWD_MUTANTS = ["onepass", "padded4", "padded16", "nm1", "eps_outside", "mask_xhat"]
BWD_MUTANTS = ["mask_xhat", "no_c2"]


def emulate_fwd(z, gamma, beta, eps, relu, layout, mutant=None, sequential=False):
    """(y, mean, rstd) in float32 with the kernels' arithmetic: two-pass statistics in lane-and-tree order.  layout: "scalar" (mean =
    sum / n), "vec" (mean = sum * (1 / n)), "gen" (vec with z - mean as fma(-1 / n, sum, z)).  ``mutant``: one of FWD_MUTANTS."""
    z = np.asarray(z, F32)
    m, n = z.shape
    lay = "scalar" if layout == "scalar" else "vec"
    n_div = n
    if mutant == "padded4":
        n_div = ceil_div(n, 4) * 4
    if mutant == "padded16":
        n_div = ceil_div(n, 16) * 16
    nf, inv_n, eps32 = F32(n_div), F32(1) / F32(n_div), F32(eps)
    s = row_sum(z, lay, sequential)
    mean = (s / nf).astype(F32) if layout == "scalar" else (s * inv_n).astype(F32)
    if layout == "gen":
        d = fma(np.full_like(z, -inv_n), np.repeat(s[:, None], n, 1), z)
    else:
        d = (z - mean[:, None]).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mutant == "onepass":
            q = row_dot(z, z, lay)
            ez2 = (q / nf).astype(F32) if layout == "scalar" else (q * inv_n).astype(F32)
            var = (ez2 - (mean * mean).astype(F32)).astype(F32)
        else:
            q = row_dot(d, d, lay)
            nv = F32(max(n - 1, 1)) if mutant == "nm1" else nf
            var = (q / nv).astype(F32) if (layout == "scalar" or mutant == "nm1") else (q * inv_n).astype(F32)
        if mutant == "eps_outside":
            rstd = (F32(1) / (np.sqrt(var).astype(F32) + eps32)).astype(F32)
        else:
            rstd = _rsqrt((var + eps32).astype(F32))
        xhat = (d * rstd[:, None]).astype(F32)
        pre = fma(xhat, np.broadcast_to(np.asarray(gamma, F32), z.shape), np.broadcast_to(np.asarray(beta, F32), z.shape))
    if not relu:
        return pre, mean, rstd
    if mutant == "mask_xhat":
        return np.where(xhat > 0, pre, F32(0)).astype(F32), mean, rstd
    return np.maximum(pre, F32(0)), mean, rstd


def emulate_bwd(dy, z, mean, rstd, gamma, beta, relu, layout, mutant=None):
    """dz in float32 with the kernels' arithmetic from the float32 stats handed in.  ``mutant``: one of BWD_MUTANTS."""
    dy, z, mean, rstd = (np.asarray(a, F32) for a in (dy, z, mean, rstd))
    gam, bet = np.broadcast_to(np.asarray(gamma, F32), z.shape), np.broadcast_to(np.asarray(beta, F32), z.shape)
    lay = "scalar" if layout == "scalar" else "vec"
    inv_n = F32(1) / F32(z.shape[1])
    xh = ((z - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    g = dy
    if relu:
        g = np.where((xh if mutant == "mask_xhat" else fma(xh, gam, bet)) <= 0, F32(0), dy)
    dxh = (g * gam).astype(F32)
    c1 = (row_sum(dxh, lay) * inv_n).astype(F32)
    c2 = (row_dot(dxh, xh, lay) * inv_n).astype(F32)
    if mutant == "no_c2":
        c2 = np.zeros_like(c2)
    t1 = (xh * c2[:, None]).astype(F32)
    return (rstd[:, None] * ((dxh - c1[:, None]).astype(F32) - t1).astype(F32)).astype(F32)
