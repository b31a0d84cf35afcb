"""float64 reference, rounding bounds and cases for the class-count-wide output layer (csrc/narrow_layer.hip):

    t_self = h W_s^T + bias,  t_neigh = h W_n^T                                  W = [W_s | W_n], the reference's [C][2 f]
    dh = (alpha dl) W_s + (alpha q) W_n,  dW = [(alpha dl)^T h | (alpha q)^T h],  dbias = colsum(alpha dl)
    out3 = {a / b, b, d},  alpha = grad_scale / b        with (a, b, d) the sums of the per-block partials {sum w nll, sum w, #correct}

numpy only, no device.  tests/test_narrow_ref_cpu.py holds a float32 emulation of every kernel family's summation order (and six
mutants of it) against the bounds below; tests/test_gpu_narrow_layer.py runs the kernels on these cases.

EXACT cases.  h, W, bias integers in [-8, 8], dl, q integers in [-4, 4], alpha a power of two.  Every product and every partial sum
in ANY order is an integer (times alpha) below 2^24: the forward at most 256 * 64 + 8, dh at most 32 * 32, dW at most n * 32 (5.3e5 at
the largest n of the suite).  The float32 result therefore IS the float64 one, whatever the order: held bit for bit.  (Every sum of
the kernels starts at + 0, so no - 0 arises on the device; the reference is brought to + 0 by `+ 0.0`.)

BOUND cases: 'scales' (columns of h and rows of W by powers of two in 2^-20 .. 2^20, W's columns and dl / q by the inverse powers, so
that the terms of one sum keep one magnitude while the outputs spread over 2^+-40), 'cancel' (rows and columns in pairs that cancel
to a thousandth of their terms in every one of the five outputs), 'gauss' (ordinary Gaussian data).  u = 2^-24; a float32 sum of terms t_i whose longest chain of dependent additions has K
links errs by at most K u sum |t_i| to first order, however the terms are spread over chains; a product that is rounded before it
is added (dv * alpha) adds one u of its term.  One u more stands in for the second-order terms.  K per output, as read from
narrow_layer.hip -- each capped by the number of terms, which makes it no looser than the any-order bound (terms + 2) u sum |t|:

    forward   fwd_chain(F, family): the matrix-pipe instructions are counted as one rounding per product they add
                  fma     NJ = ceil(F / 64) fmas per lane, then the 6 levels of the wave butterfly
                  mfma32  F % 8 == 0: k-blocks of 8, even / odd blocks on two accumulator chains: 4 instructions x 2 products per
                          block, ceil(kbs / 2) blocks on the longer chain, one addition joins the chains
                  mfma16  F % 16 == 0: every k on one chain: F
              + 1 for the bias (t_neigh has none; the bound does not use that)
    dh        2 C products on one chain (zero rows of the weight image add exactly) + 1 for dv * alpha
    dW, dbias rows of one workgroup on one chain, then the fold of the workgroups' partials:
                  mfma    32 per row block x the row blocks a workgroup walks (ceil(nblk / grid))
                  fma     rows per wave (ceil(n / 4 grid)) + 3 additions across the four waves
              + fold_chain(grid) + 1 for dv * alpha
"""
import numpy as np

U = 2.0 ** -24

# ---- the launch rules of narrow_layer.hip, named here so that a changed threshold shows up in tests/test_narrow_ref_cpu.py ----------
NC_MAX = 16           # classes
F_MAX = 256           # hidden width
NB_MAX = 512          # workgroups of either backward kernel
FWD_FMA_BLOCKS = 2048         # workgroups of the plain forward (4 rows each): it loops beyond 8 192 rows
FWD_MFMA_BLOCKS = 2048        # workgroups of the matrix-pipe forwards (128 rows each): they loop beyond 262 144 rows
CE_BLOCK = 64                 # rows per cross-entropy partial (3 floats each)

FMA_WIDTHS = {1: [1, 13, 63], 2: [65, 100, 127], 4: [129, 250, 255]}                # NJ -> widths
MFMA32_WIDTHS = [8, 24, 40, 120, 248]                  # F % 8 == 0, F % 16 != 0: odd kbs, the `u + 1 < kbs` edge of the second chain
MFMA16_WIDTHS = [16, 32, 48, 128, 256]
BWD_MFMA_WIDTHS = [8, 56, 64, 72, 128, 136, 192, 200, 256]          # around the 64-column slices of the four waves
PADDED = [(5, 16), (17, 32), (31, 32), (100, 112), (139, 144), (218, 224), (241, 256), (250, 256)]     # (f, n_pad): every f % 4
CLASS_EDGES = [1, 4, 5, 8, 9, 12, 13, 16]
ROWS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]
BOUND_KINDS = ["scales", "cancel", "gauss"]


def nct(c):
    """the compile-time class bound of the instantiation that serves c classes"""
    return 4 if c <= 4 else 8 if c <= 8 else 12 if c <= 12 else 16


def nctm(c):
    """... of the padded-row backward (9 .. 12 classes take the 16-class form)"""
    return 4 if c <= 4 else 8 if c <= 8 else 16


def fwd_family(f):
    return "fma" if f % 8 else "mfma16" if f % 16 == 0 else "mfma32"


def bwd_family(f):
    return "fma" if f % 8 else "mfma"


def nj(f):
    return 1 if f <= 64 else 2 if f <= 128 else 4


def bwd_grid(n, f, cus, ln=False):
    """workgroups of the backward at n rows"""
    if bwd_family(f) == "fma":
        return min(-(-n // 4), NB_MAX)
    return min(-(-n // 32), min(cus * (2 if ln else 1), NB_MAX))


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def fwd(h, W, bias, f_true):
    """h [n, >= f_true] (padded rows: the columns behind f_true are not read), W [C, 2 f_true] -> t_self, t_neigh [n, C]"""
    h, W = _f64(h)[:, :f_true], _f64(W)
    ts = h @ W[:, :f_true].T + 0.0
    if bias is not None:
        ts = ts + _f64(bias)[None, :]
    return ts, h @ W[:, f_true:2 * f_true].T + 0.0


def bwd(dl, q, h, W, alpha=1.0):
    """-> dh [n, f], dW [C, 2 f], dbias [C]; f = W.shape[1] / 2, h [n, >= f]"""
    W = _f64(W)
    f = W.shape[1] // 2
    a = float(np.float32(alpha))
    dl, q, h = _f64(dl) * a, _f64(q) * a, _f64(h)[:, :f]
    dh = dl @ W[:, :f] + q @ W[:, f:] + 0.0
    dW = np.concatenate([dl.T @ h, q.T @ h], axis=1) + 0.0
    return dh, dW, dl.sum(axis=0) + 0.0


def _fold(partials):
    p = _f64(partials).reshape(-1, 3)
    return p[:, 0].sum(), p[:, 1].sum(), p[:, 2].sum()


def out3(partials):
    """csrc/ce_fold.h: a double fold of the float partials; loss = a / b if b > 0 else 0 -> float32[3]"""
    a, b, d = _fold(partials)
    return np.array([a / b if b > 0 else 0.0, b, d], dtype=np.float32)


def alpha(partials, grad_scale):
    """the float32 factor narrow_bwd_mfma_kernel applies to dl and q: grad_scale / (float)wsum if wsum > 0 else 0"""
    wsum = np.float32(_fold(partials)[1])
    return np.float32(np.float32(grad_scale) / wsum) if wsum > 0 else np.float32(0.0)


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def fwd_chain(f, family=None):
    family = family or fwd_family(f)
    if family == "fma":
        k = nj(f) + 6
    elif family == "mfma32":
        k = 8 * (-(-(f // 8) // 2)) + 1
    else:
        k = f
    return min(k, f)


def fold_chain(count):
    """longest chain of the fold of `count` workgroup partials, the larger of the forms that can run:
    narrow_fold16_kernel -- 16 slices, two alternating sums per slice, one addition joins them, the slices are added in order;
    gte_fold_batch_kernel -- 16 / 4 / 1 slices (count >= 128 / >= 32 / below), eight sums per slice (joined by 3 additions, at most 4
    tail terms on one of them), the slices added in order;  narrow_fold_kernel (plain kernels) -- 4 slices, then 3 additions."""
    m16 = -(-count // 16)
    f16 = -(-m16 // 2) + 1 + 16
    s = 16 if count >= 128 else 4 if count >= 32 else 1
    batch = (-(-count // s)) // 8 + 7 + s
    fma = -(-count // 4) + 3
    return min(count, max(f16, batch, fma))


def dw_chain(n, f, cus, ln=False):
    grid = bwd_grid(n, f, cus, ln)
    if bwd_family(f) == "fma":
        k = -(-n // (4 * grid)) + 3
    else:
        k = 32 * (-(-(-(-n // 32)) // grid))
    return min(k + fold_chain(grid), n)


def fwd_bound(h, W, bias, f_true, width=None):
    """-> the bound of t_self and of t_neigh, [n, C] each; width: the width the kernel computes over (padded rows: n_pad, whose
    zero columns add exactly)"""
    k = min(fwd_chain(width or f_true), f_true)
    h, W = np.abs(_f64(h)[:, :f_true]), np.abs(_f64(W))
    b = np.abs(_f64(bias))[None, :] if bias is not None else 0.0
    return (k + 2) * U * (h @ W[:, :f_true].T + b), (k + 2) * U * (h @ W[:, f_true:2 * f_true].T)


def bwd_bound(dl, q, h, W, n_chain, alpha=1.0):
    """-> bounds of dh, dW, dbias; n_chain = dw_chain(...) of the launch"""
    W = np.abs(_f64(W))
    f, c = W.shape[1] // 2, W.shape[0]
    a = abs(float(np.float32(alpha)))
    dl, q, h = np.abs(_f64(dl)) * a, np.abs(_f64(q)) * a, np.abs(_f64(h)[:, :f])
    dh = (2 * c + 2) * U * (dl @ W[:, :f] + q @ W[:, f:])
    dW = (n_chain + 2) * U * np.concatenate([dl.T @ h, q.T @ h], axis=1)
    return dh, dW, (n_chain + 2) * U * dl.sum(axis=0)


def ratio(got, ref, bnd):
    """largest |got - ref| / bound (0 / 0 = 0; a non-finite result is infinitely wrong)"""
    err = np.abs(_f64(got) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bnd))) if err.size else 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all(bits(a) == bits(b)))


def exact32(ref):
    """the float64 reference of an exact case as float32 (it must be representable: an exact case that is not is a broken case)"""
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref), "the case is not exact in float32"
    return r32


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """float32 inputs of one shape: h [n, f], W [c, 2 f], bias [c], dl, q [n, c]"""

    def __init__(self, kind, n, f, c, h, W, bias, dl, q):
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.kind, self.n, self.f, self.c = kind, n, f, c
        self.h, self.W, self.bias, self.dl, self.q = f32(h), f32(W), f32(bias), f32(dl), f32(q)
        self.exact = kind == "exact"

    def padded(self, n_pad):
        """h with zero columns up to n_pad (the padded-row entry points)"""
        hp = np.zeros((self.n, n_pad), dtype=np.float32)
        hp[:, :self.f] = self.h
        return hp


def exact_case(n, f, c, seed=0):
    rng = np.random.default_rng([11, n, f, c, seed])
    iv = lambda lim, *s: rng.integers(-lim, lim + 1, s)
    return Case("exact", n, f, c, iv(8, n, f), iv(8, c, 2 * f), iv(8, c), iv(4, n, c), iv(4, n, c))


def exact_partials(n, log2_wsum=3):
    """ceil(n / 64) partials {sum w nll, sum w, #correct} of small dyadic values whose sums are exact in any order and whose
    sum of weights is 2^log2_wsum"""
    nb = -(-n // CE_BLOCK)
    p = np.zeros((nb, 3), dtype=np.float32)
    p[:, 0] = (np.arange(nb) % 7) * 0.25 + 0.5
    p[:, 1] = 2.0 ** log2_wsum / 2 ** int(np.ceil(np.log2(nb))) if nb > 1 else 2.0 ** log2_wsum
    p[nb - 1, 1] += 2.0 ** log2_wsum - p[:, 1].sum()          # (nb no power of two: the last block takes the rest, a dyadic value)
    p[:, 2] = np.arange(nb) % 5
    assert _fold(p)[1] == 2.0 ** log2_wsum
    return p


def bound_partials(n, seed=0):
    rng = np.random.default_rng([13, n, seed])
    nb = -(-n // CE_BLOCK)
    p = rng.uniform(0.5, 40.0, (nb, 3)).astype(np.float32)
    p[:, 2] = np.floor(p[:, 2])
    return p


def bound_case(kind, n, f, c, seed=0):
    rng = np.random.default_rng([17, BOUND_KINDS.index(kind), n, f, c, seed])
    g = rng.standard_normal
    if kind == "gauss":
        return Case(kind, n, f, c, g((n, f)), g((c, 2 * f)) / np.sqrt(2 * f), g(c), g((n, c)) / n, g((n, c)) / n)
    if kind == "scales":
        # powers of two in 2^-20 .. 2^20: h column k by s_k and W's columns k, f + k by 1 / s_k; W row c and bias c by t_c and dl, q
        # column c by 1 / t_c.  The terms of any one sum keep one magnitude (a dropped term cannot hide behind a larger column) while
        # the outputs spread: t[:, c] ~ t_c, dh[:, k] ~ 1 / s_k, dW[c, k] ~ s_k / t_c, dbias[c] ~ 1 / t_c; the bounds are per element
        p2 = lambda m: 2.0 ** rng.integers(-20, 21, m)
        sk, sc = p2(f), p2(c)
        return Case(kind, n, f, c, g((n, f)) * sk[None, :], g((c, 2 * f)) * sc[:, None] / np.tile(sk, 2)[None, :], g(c) * sc,
                    g((n, c)) / sc[None, :], g((n, c)) / sc[None, :])
    assert kind == "cancel"
    # rows and columns in pairs: h[2i + 1] = h[2i] and dl[2i + 1] = - dl[2i] (1 + 1e-3 d): dW and dbias cancel to a thousandth of
    # their terms; h[:, 2j + 1] = h[:, 2j] and W_s[:, 2j + 1] = - W_s[:, 2j] (1 + 1e-3 d): so does the forward; W_n = 2 W_s and
    # q = - dl (1 + 1e-3 d) / 2: so does dh.  (An odd n, f leaves the last row / column without its partner.)
    pert = lambda *s: 1.0 + 1e-3 * rng.uniform(0.5, 1.0, s)
    hb = g((-(-n // 2), -(-f // 2)))
    h = np.repeat(np.repeat(hb, 2, axis=0), 2, axis=1)[:n, :f]
    wb = g((c, -(-f // 2)))
    ws = np.repeat(wb, 2, axis=1)[:, :f].copy()
    ws[:, 1::2] *= -pert(c, f // 2)
    db = g((-(-n // 2), c))
    dl = np.repeat(db, 2, axis=0)[:n].copy()
    dl[1::2] *= -pert(n // 2, c)
    return Case(kind, n, f, c, h, np.concatenate([ws, 2.0 * ws], axis=1), g(c) * 1e-3, dl, -0.5 * dl * pert(n, c))


def bound_cases(n, f, c, seed=0):
    return [bound_case(k, n, f, c, seed) for k in BOUND_KINDS]
