"""float64 reference, inputs, error bounds and a float32 emulation for the one-pass backward of the short-input layer:
gte_sage_smallk_bwd (csrc/smallk_bwd.hip) and the epilogue of gte_gemm_p3_nt_smallk_bwd (smallk_bwd_epilogue, csrc/gemm_p3.hip), which
share csrc/smallk_step.h.  Used by tests/test_smallk_ref_cpu.py without a GPU and by tests/test_gpu_smallk_bwd.py on one.  Test
infrastructure, numpy only; notation and the LayerNorm bounds are those of tests/layernorm_cases.py (u = 2^-24).

The operation.  y = relu?(LN(z)), z = [x | ahn] W^T + bias; from dy the layer's gradients are
    dz = LN'(z)(mask . dy),  dW = dz^T [x | ahn],  dbias = sum_r dz,  dgamma = sum_r (mask . dy) xhat,  dbeta = sum_r mask . dy.
Both kernels RECOMPUTE z and never store dz, so neither can be compared with anything bit for bit.  The reference is therefore
evaluated on what the forward left behind: the z that gte_sage_linear_fwd saved and its float32 (mean, rstd), as layernorm_cases does
for the other backward kernels, so no kappa enters.  For the epilogue form dy is the device's own gte_gemm_p3_nt product taken as
float64; the tests draw the GEMM's operands from small dyadic numbers, so that every float32 summation order gives the same exact
product and no GEMM rounding has to be allowed for.

The mask.  By convention (include/gte.h) the backward's mask is the one on the stored statistics: fma(fl(fl(z - mean) rstd), gamma,
beta) > 0 in float32 (mask32).  The forward computes y from the same registers, so y > 0 must equal mask32 EVERYWHERE, with no
neutralised element: that is the observable half of "the recomputed z is bit-identical, the ReLU mask cannot flip".  The other half
-- the z the BACKWARD recomputes -- shows only in the gradients: a z that differs in its last bit moves xhat by kappa u, i.e. by
1e-3 on a row whose mean is 1e4 spreads, and flips the mask wherever |pre| is below that; both are far outside the bounds below,
which hold no kappa.  The reference takes mask32 as its mask.  Where the float64 value of pre on the same z and stats is within
4 u (|xhat gamma| + |beta|) of zero, mask32 is a coin toss of the reference's own float32 evaluation ("ambiguous"); such elements get
dy = 0 (stand-alone) or a zero GEMM row (epilogue) under layernorm_cases.AMBIGUOUS_CAP.  With both masks on the SAME statistics that
band is some 1e-7 wide: test_smallk_ref_cpu.py counts the elements (none on these inputs).  The planted exact ties -- all-zero rows
of z with beta_j == 0, where pre == 0 without a rounding -- are no coin toss: mask32 is false, y is 0 and they get no gradient.

Bounds.  R = depth("tile") = 9 for both kernels (a lane's four columns in a chain, the 6-level wave tree: gte_smallk_bwd_step), so per
row |dz' - dz| <= Db u rstd max|gamma| ||dy_row||_2 with Db = 2 R + 22 (layernorm_cases.bwd_bound).  A column sum is a float32 sum of
float32 terms: it errs by at most Kc u times the sum of the absolute terms, Kc = the additions an element passes through + 3 for the
term itself (xhat', the multiply-add), exactly as layernorm_cases.colsum_roundings.  Hence
    |dgamma' - dgamma|_j <= Kc u sum_r |g_rj xhat_rj|,      |dbeta' - dbeta|_j <= Kc u sum_r |g_rj|            (g = mask . dy)
    |dbias' - dbias|_j   <= sum_r B_r + Kc u sum_r (|dz_rj| + B_r)                                             (B_r: the dz bound of row r)
    |dW' - dW|_jk        <= sum_r B_r |x_rk| + Kc u sum_r (|dz_rj| + B_r) |x_rk|
(the dz bound carried through sum_r |x_rk|, plus Kc roundings of sum_r |dz_rj x_rk|).

Chain lengths, read off the kernels:
  stand-alone  a workgroup owns 64 rows per trip of its grid-stride loop; its wave w runs 8 steps of 2 rows, so a lane adds 16 rows
               per trip into one accumulator: 16 T additions, T = ceil(ceil(M / 64) / nb) trips of nb = min(ceil(M / 64), 512)
               workgroups.  The four waves meet in LDS as ((w0 + w1) + w2) + w3: 3.  The nb block partials are folded by
               smallk_fold_kernel (four interleaved chains and a pair tree: ceil(nb / 4) + 2) or, inside a fold deferral, by
               gte_fold_batch_kernel (s = 16, 4 or 1 slices at nb >= 128, >= 32, below; a slice's ceil(nb / s) partials in up to
               eight chains and a tree, then the slices in order: at most ceil(nb / s) + 3 + s).  Kc = 16 T + 3 + fold + 3.
  epilogue     a workgroup owns one 128-row tile, staged 32 rows at a time; wave w takes rows 2 w, 2 w + 1, 2 w + 16, 2 w + 17 of a
               chunk: 16 additions over the tile.  The eight waves are added in order from zero: 8.  The nb = ceil(M / 128) tile
               partials are folded by p3_colsum_fold_kernel (one chain: nb) or by the deferral as above.  Kc = 16 + 8 + fold + 3.

Inputs.  W and bias are shared by all rows, so the row kinds of layernorm_cases (OFFSETS, CONSTANTS, zero, tiny, single) are steered
through x: W[:, 0] = 1 (K >= 2) and x[r, 0] carries the row's offset; a row (c, 0, ...) under a constant bias is a constant row; an
all-zero row under a zero bias is a zero row; a row scaled by 1e-4 is tiny; one non-zero input is single.  The bias is zero, constant
or random by the case's index.  gamma has mixed signs and an exact zero, beta exact zeros (layernorm_cases.make_params).
"""
import numpy as np

from tests import layernorm_cases as lc

U = lc.U
F32 = np.float32
R = lc.depth("tile", 256)
BLOCK_ROWS, MAX_BLOCKS, TILE_ROWS, CHUNK_ROWS = 64, 512, 128, 32

KLADDER = [(1, 0), (1, 1), (13, 0), (8, 8), (9, 8), (13, 13), (14, 13), (14, 14)]    # K = 1, 2, 13, 16 | 17, 26, 27, 28: <16> | <28>
SA_MS = [1, 2, 63, 64, 65, 129]
SA_NS = {(1, 0): [4, 100, 256], (1, 1): [8, 252], (13, 0): [64, 200], (8, 8): [4, 100, 256], (9, 8): [8, 200],
         (13, 13): [64, 252, 256], (14, 13): [100, 256], (14, 14): [4, 8, 200, 256]}
M_STRIDE = MAX_BLOCKS * BLOCK_ROWS + 65          # the grid-stride loop's second trip: one full block and one row of the next
EP_MS = [1, 31, 32, 33, 127, 128, 129, 257]
EP_NS = {(1, 0): [4, 256], (1, 1): [100, 252], (13, 0): [200, 256], (8, 8): [4, 252], (9, 8): [100, 256], (13, 13): [200, 256],
         (14, 13): [4, 252], (14, 14): [100, 256]}
GEMM_K = 64                                      # the epilogue form's own GEMM
AMB_FACTOR = 4.0


def cases(form, kk=None):
    """(form, k1, k2, n, m, relu, idx): every M at every (k1, k2, n) of the form's table, ReLU on and off; idx numbers the (k1, k2,
    n, m) and picks the seed, eps, the bias kind and the planted rows"""
    table, ms = (SA_NS, SA_MS) if form == "standalone" else (EP_NS, EP_MS)
    out, idx = [], 0
    for k12 in KLADDER:
        for n in table[k12]:
            for m in ms:
                idx += 1
                if kk is None or tuple(kk) == k12:
                    out += [(form, k12[0], k12[1], n, m, relu, idx) for relu in (True, False)]
    return out


STRIDE_NS = [8, 256]


def stride_case(n):
    """the stand-alone kernel's grid-stride case at width n (one definition for the GPU test and the CPU emulation)"""
    return ("standalone", 13, 13, n, M_STRIDE, True, 9001 + n)


def plants(m, idx):
    """row -> kind"""
    if m == 1:
        return {} if idx % 11 == 10 else {0: lc.KINDS[idx % 10]}
    if m == 2:
        return {idx % 2: lc.KINDS[(idx // 2) % 10]}
    return lc.variants(m if m not in (3, 8, 9) else 10)[0]


def plant_rows(xin, plant, rng):
    """overwrite the planted rows of xin = [x | ahn] in place"""
    k = xin.shape[1]
    for row, kind in plant.items():
        if kind in lc.OFFSETS:
            mean, std = lc.OFFSETS[kind]
            xin[row] = (std * rng.standard_normal(k)).astype(F32)
            xin[row, 0] = F32(mean)
        elif kind in lc.CONSTANTS:
            xin[row] = 0
            xin[row, 0] = F32(lc.CONSTANTS[kind])
        elif kind == "zero":
            xin[row] = 0
        elif kind == "tiny":
            xin[row] = (1e-4 * rng.standard_normal(k)).astype(F32)
        elif kind == "single":
            xin[row] = 0
            xin[row, int(rng.integers(1, k)) if k > 1 else 0] = F32(rng.uniform(0.5, 2.0) * (1 if rng.random() < 0.5 else -1))
        else:
            raise ValueError(kind)
    return xin


def make_inputs(case):
    """dict of float32 arrays: xin [m, K], W [n, K], bias, gamma, beta, dy [m, n] and, for the epilogue form, the dyadic GEMM operands
    a [m, GEMM_K], b [n, GEMM_K] with dy = a b^T exact in float32 in any summation order (multiples of 2^-8 below 2^9)"""
    form, k1, k2, n, m, relu, idx = case
    rng = np.random.default_rng(770000 + 10 * idx + (form == "epilogue"))
    k = k1 + k2
    xin = rng.standard_normal((m, k)).astype(F32)
    w = (rng.standard_normal((n, k)) / np.sqrt(max(k - 1, 1))).astype(F32)
    if k >= 2:
        w[:, 0] = 1
    bias = [np.zeros(n), np.full(n, 0.5), 0.5 * rng.standard_normal(n)][idx % 3].astype(F32)
    gamma, beta = lc.make_params(n, rng)
    plant = plants(m, idx)
    plant_rows(xin, plant, rng)
    out = {"xin": xin, "W": w, "bias": bias, "gamma": gamma, "beta": beta, "eps": (1e-5, 1e-12)[idx % 2], "plant": plant, "k1": k1, "k2": k2}
    if form == "epilogue":
        a = np.clip(np.round(4 * rng.standard_normal((m, GEMM_K))) / 4, -4, 4).astype(F32)
        b = np.clip(np.round(8 * rng.standard_normal((n, GEMM_K))) / 64, -0.5, 0.5).astype(F32)
        out.update(a=a, b=b, dy=(a.astype(np.float64) @ b.astype(np.float64).T).astype(F32))
    else:
        out["dy"] = rng.standard_normal((m, n)).astype(F32)
    return out


# ------------------------------------------------------------------------------------------------ reference and bounds
def mask32(z, mean, rstd, gamma, beta):
    """the backward's mask by convention: float32 fma(fl(fl(z - mean) rstd), gamma, beta) > 0 on the stored statistics"""
    z, mean, rstd = (np.asarray(a, F32) for a in (z, mean, rstd))
    xh = ((z - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    return lc.fma(xh, np.broadcast_to(np.asarray(gamma, F32), z.shape), np.broadcast_to(np.asarray(beta, F32), z.shape)) > 0


def ambiguous(z, mean, rstd, gamma, beta):
    """elements whose float64 pre on the same z and stats is within AMB_FACTOR u (|xhat gamma| + |beta|) of zero, or where mask32
    differs from the float64 mask: the reference's own float32 evaluation cannot be trusted there.  Exact ties (pre == 0 with
    xhat == 0: the zero rows) are not ambiguous."""
    z, mean, rstd, gamma, beta = (np.asarray(a, np.float64) for a in (z, mean, rstd, gamma, beta))
    xhat = (z - mean[:, None]) * rstd[:, None]
    pre = xhat * gamma + beta
    amb = (np.abs(pre) <= AMB_FACTOR * U * (np.abs(xhat * gamma) + np.abs(beta))) | (mask32(z, mean, rstd, gamma, beta) != (pre > 0))
    return amb & ~((xhat == 0) & (beta == 0))


def backward(dy, xin, z, mean, rstd, gamma, beta, relu, mask=None):
    """float64 (dW, dgamma, dbeta, dbias, dz, g, xhat) of the layer from the z and statistics handed in; ``mask``: the ReLU mask to
    take (None: xhat gamma + beta > 0 in float64, no gradient at pre == 0, as torch.relu)"""
    dy, xin, z, mean, rstd, gamma, beta = (np.asarray(a, np.float64) for a in (dy, xin, z, mean, rstd, gamma, beta))
    xhat = (z - mean[:, None]) * rstd[:, None]
    if relu:
        g = np.where((xhat * gamma + beta > 0) if mask is None else mask, dy, 0.0)
    else:
        g = dy
    dxhat = g * gamma
    c1 = dxhat.mean(axis=1)
    c2 = (dxhat * xhat).mean(axis=1)
    dz = rstd[:, None] * (dxhat - c1[:, None] - xhat * c2[:, None])
    return dz.T @ xin, (g * xhat).sum(axis=0), g.sum(axis=0), dz.sum(axis=0), dz, g, xhat


def fold_roundings(nb, direct):
    s = 16 if nb >= 128 else (4 if nb >= 32 else 1)
    return max(direct, lc.ceil_div(nb, s) + 3 + s)


def colsum_roundings(form, m):
    """Kc of the module docstring, the larger of the two folds (the bounds hold inside and outside a fold deferral)"""
    if form == "standalone":
        nbt = lc.ceil_div(m, BLOCK_ROWS)
        nb = min(nbt, MAX_BLOCKS)
        return 16 * lc.ceil_div(nbt, nb) + 3 + fold_roundings(nb, lc.ceil_div(nb, 4) + 2) + 3
    nb = lc.ceil_div(m, TILE_ROWS)
    return 16 + 8 + fold_roundings(nb, nb) + 3


def bounds(form, dy, xin, rstd, gamma, dz, g, xhat):
    """(dW, dgamma, dbeta, dbias) bounds; dz, g, xhat from ``backward``"""
    m = dy.shape[0]
    kc = colsum_roundings(form, m) * U
    rows = lc.bwd_bound(R, dy, rstd, gamma)
    ax = np.abs(np.asarray(xin, np.float64))
    adz = np.abs(dz) + rows[:, None]
    return ((rows @ ax)[None, :] + kc * (adz.T @ ax), kc * (np.abs(g) * np.abs(xhat)).sum(axis=0), kc * np.abs(g).sum(axis=0),
            rows.sum() + kc * adz.sum(axis=0))


def ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0, anything non-finite as infinite"""
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bound)))


NAMES = ("dW", "dgamma", "dbeta", "dbias")


def ratios(form, got, dy, xin, z, mean, rstd, gamma, beta, relu):
    """error / bound of the four outputs ``got`` = (dW, dgamma, dbeta, dbias; None: not asked for) against the reference with mask32"""
    want = backward(dy, xin, z, mean, rstd, gamma, beta, relu, mask32(z, mean, rstd, gamma, beta))
    bnd = bounds(form, dy, xin, rstd, gamma, *want[4:])
    return [None if o is None else ratio(np.abs(np.asarray(o, np.float64) - w), b) for o, w, b in zip(got, want[:4], bnd)]


# ------------------------------------------------------------------------------------------------ float32 emulation
MUTANTS = ["bias_last", "inv_n_padded", "no_c2", "mask_xhat", "clamped_row_counted", "second_trip_skipped", "a2_with_lda1", "pad_column"]


def input_buffers(xin, k1, k2):
    """the two operands as the GPU tests lay them out: [m + 1, k1 + 3] and [m + 1, k2 + 1], NaN in the padding columns and in the row
    behind row m - 1"""
    m = xin.shape[0]
    xb = np.full((m + 1, k1 + 3), np.nan, F32)
    xb[:m, :k1] = xin[:, :k1]
    ab = np.full((m + 1, k2 + 1), np.nan, F32)
    ab[:m, :k2] = xin[:, k1:]
    return xb, ab


def emulate_z(xb, ab, k1, k2, m, w, bias, mutant=None):
    """z of m rows as sage_smallk_fwd_kernel and gte_smallk_bwd_step compute it: the accumulator starts at the bias and takes
    fma(x_k, W_jk, .) for k = 0 .. Kp - 1 in order, the padding k >= K with zeros on both sides.  Returns (z, the staged inputs [m, K])."""
    k = k1 + k2
    kp = (k + 3) & ~3
    x1 = xb[:m, :k1]
    if mutant == "a2_with_lda1":
        flat = ab.ravel()
        x2 = flat[np.minimum(np.arange(m)[:, None] * xb.shape[1] + np.arange(k2)[None, :], flat.size - 1)]
    else:
        x2 = ab[:m, :k2]
    xs = np.zeros((m, kp), F32)
    xs[:, :k1], xs[:, k1:k] = x1, x2
    wt = np.zeros((kp, w.shape[0]), F32)
    wt[:k] = np.asarray(w, F32).T
    if mutant == "pad_column":
        xs[:, k:], wt[k:] = 1, 1
    acc = np.broadcast_to(np.asarray(bias, F32), (m, w.shape[0])).copy()
    if mutant == "bias_last":
        acc[:] = 0
    for kk in range(kp):
        acc = lc.fma(np.repeat(xs[:, kk:kk + 1], w.shape[0], 1), np.repeat(wt[kk][None, :], m, 0), acc)
    if mutant == "bias_last":
        acc = (acc + np.asarray(bias, F32)[None, :]).astype(F32)
    return acc, xs[:, :k]


def emulate_forward(xin, k1, k2, w, bias, gamma, beta, eps, relu):
    """(z, y, mean, rstd) of sage_smallk_fwd_kernel"""
    xb, ab = input_buffers(xin, k1, k2)
    z, _ = emulate_z(xb, ab, k1, k2, xin.shape[0], w, bias)
    y, mean, rstd = lc.emulate_fwd(z, gamma, beta, eps, relu, "vec")
    return z, y, mean, rstd


def _row_order(form, m, mutant):
    """[nb, waves, L] row indices in the order a lane's accumulators take them (-1: nothing)"""
    if form == "standalone":
        nbt = lc.ceil_div(m, BLOCK_ROWS)
        nb = min(nbt, MAX_BLOCKS)
        trips = 1 if mutant == "second_trip_skipped" else lc.ceil_div(nbt, nb)
        b, wv, t, st, u = np.meshgrid(np.arange(nb), np.arange(4), np.arange(trips), np.arange(8), np.arange(2), indexing="ij")
        row = (b + nb * t) * BLOCK_ROWS + (st * 4 + wv) * 2 + u
    else:
        nb = lc.ceil_div(m, TILE_ROWS)
        b, wv, c, h, u = np.meshgrid(np.arange(nb), np.arange(8), np.arange(4), np.arange(2), np.arange(2), indexing="ij")
        row = b * TILE_ROWS + c * CHUNK_ROWS + 2 * wv + 16 * h + u
    row0 = row - u
    if mutant == "clamped_row_counted":
        row = np.where(row0 < m, np.minimum(row, m - 1), -1)
    else:
        row = np.where(row < m, row, -1)
    return row.reshape(nb, row.shape[1], -1)


def _waves(form, acc):
    if form == "standalone":
        return (((acc[:, 0] + acc[:, 1]).astype(F32) + acc[:, 2]).astype(F32) + acc[:, 3]).astype(F32)
    v = np.zeros_like(acc[:, 0])
    for wv in range(acc.shape[1]):
        v = (v + acc[:, wv]).astype(F32)
    return v


def _chain(parts, idx):
    s = np.zeros_like(parts[0])
    for i in idx:
        s = (s + parts[i]).astype(F32)
    return s


def _fold(form, parts, deferred):
    nb = parts.shape[0]
    if not deferred and form == "epilogue":                    # p3_colsum_fold_kernel
        return _chain(parts, range(nb))
    if not deferred:                                           # smallk_fold_kernel
        q = nb - nb % 4
        s = [_chain(parts, list(range(i, q, 4)) + (list(range(q, nb)) if i == 0 else [])) for i in range(4)]
        return ((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32)
    ns = 16 if nb >= 128 else (4 if nb >= 32 else 1)           # gte_fold_batch_kernel, scalar path
    v = np.zeros_like(parts[0])
    for sl in range(ns):
        ks = list(range(sl, nb, ns))
        n8 = len(ks) - len(ks) % 8
        s = [_chain(parts, ks[i:n8:8]) for i in range(8)]
        s = [(s[i] + s[i + 4]).astype(F32) for i in range(4)]
        rest = ks[n8:]
        n4 = len(rest) - len(rest) % 4
        for i in range(4):
            for kx in rest[i:n4:4]:
                s[i] = (s[i] + parts[kx]).astype(F32)
        for kx in rest[n4:]:
            s[0] = (s[0] + parts[kx]).astype(F32)
        v = (v + ((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32)).astype(F32)
    return v


def emulate_backward(form, dy, xin, k1, k2, w, bias, gamma, beta, mean, rstd, relu, deferred=False, mutant=None):
    """(dW, dgamma, dbeta, dbias) in float32 with the kernels' arithmetic and summation order: z recomputed (emulate_z),
    gte_smallk_bwd_step per row, a lane's chain over its rows, the waves, the fold.  ``mutant``: one of MUTANTS."""
    m, n = dy.shape
    dy, mean, rstd = (np.asarray(a, F32) for a in (dy, mean, rstd))
    gam, bet = np.broadcast_to(np.asarray(gamma, F32), (m, n)), np.broadcast_to(np.asarray(beta, F32), (m, n))
    xb, ab = input_buffers(xin, k1, k2)
    z, xs = emulate_z(xb, ab, k1, k2, m, w, bias, mutant)
    inv_n = F32(1) / F32(256 if mutant == "inv_n_padded" else n)
    with np.errstate(invalid="ignore", over="ignore"):
        xh = ((z - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
        g = dy
        if relu:
            g = np.where((xh if mutant == "mask_xhat" else lc.fma(xh, gam, bet)) <= 0, F32(0), dy)
        dxh = (g * gam).astype(F32)
        c1 = (lc.row_sum(dxh, "vec") * inv_n).astype(F32)
        c2 = np.zeros_like(c1) if mutant == "no_c2" else (lc.row_dot(dxh, xh, "vec") * inv_n).astype(F32)
        dz = (rstd[:, None] * ((dxh - c1[:, None]).astype(F32) - (xh * c2[:, None]).astype(F32)).astype(F32)).astype(F32)
        order = _row_order(form, m, mutant)
        nb, nw, steps = order.shape
        k = k1 + k2
        a_dw, a_dg, a_db, a_dbias = np.zeros((nb, nw, n, k), F32), np.zeros((nb, nw, n), F32), np.zeros((nb, nw, n), F32), np.zeros((nb, nw, n), F32)
        for s in range(steps):
            rows = order[:, :, s]
            if (rows < 0).all():
                continue
            live = (rows >= 0)[..., None]
            rc = np.maximum(rows, 0)
            dzr, gr, xhr, xr = np.where(live, dz[rc], F32(0)), np.where(live, g[rc], F32(0)), xh[rc], np.where(live, xs[rc], F32(0))
            a_dw = lc.fma(np.repeat(dzr[..., None], k, -1), np.repeat(xr[:, :, None, :], n, 2), a_dw)
            a_dg = lc.fma(gr, xhr, a_dg)
            a_db = (a_db + gr).astype(F32)
            a_dbias = (a_dbias + dzr).astype(F32)
        return tuple(_fold(form, _waves(form, a), deferred) for a in (a_dw, a_dg, a_db, a_dbias))
