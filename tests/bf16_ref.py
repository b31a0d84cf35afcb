"""Reference of the GAT's bf16 projection (csrc/gemm_bf16.hip: gte_cast_bf16, gte_gemm_bf16_nt) in numpy: the fp32 -> bf16 rounding
in integer arithmetic on the float32 bits, ELU through float64, the product in float64 with its rounding unit, and the seeded input
makers of tests/test_gpu_bf16_projection.py.  Checked on the CPU by tests/test_bf16_ref_cpu.py.

bf16 values travel as uint16 bit patterns (the storage type of the C ABI), never as a float type of some library.
"""
import numpy as np

BAND_ULPS = 16                          # elu_bf16: half-width of the band around a bf16 rounding midpoint, in fp32 ulps
FLT_MAX_BITS = 0x7F7FFFFF
FIRST_TO_INF_BITS = 0x7F7F8000          # the smallest float32 that rounds to bf16 infinity (a tie at an odd mantissa)


# ---------------------------------------------------------------------------------------------------------------------
# rounding
# ---------------------------------------------------------------------------------------------------------------------
def to_bf16(x32):
    """float32 -> bf16 bits, round to nearest even: (b + 0x7FFF + ((b >> 16) & 1)) >> 16 on the float32 bits b.  Subnormals and the
    sign of zero are kept, what lies above the largest bf16 goes to infinity, a NaN goes to a (quiet) NaN of its sign."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    b = x32.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000          # the carry of the formula would turn 0x7F800001 into inf and 0x7FFFFFFF into -0
    return np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)


def from_bf16(bits):
    """bf16 bits -> float32 (exact)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def is_nan_bf16(bits):
    return (np.asarray(bits, dtype=np.uint16) & 0x7FFF) > 0x7F80


def _ordinal(bits):
    """bf16 bits -> an integer that orders the values (both zeros at 0)."""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    return np.where(b < 0x8000, b, -(b & 0x7FFF))


def _from_ordinal(o):
    return np.where(o >= 0, o, 0x8000 | -o).astype(np.uint16)


def elu_bf16(x32):
    """ELU(v) = v for v > 0, else expm1(v), in float64.  Returns (want, lo, hi, in_band):
    want     the float64 value rounded once to fp32 and then by to_bf16;
    lo, hi   the bf16 neighbours of the float64 value (equal where it is a bf16 value; a zero neighbour is +0);
    in_band  non-positive inputs whose float64 ELU lies within BAND_ULPS fp32 ulps of the midpoint of lo and hi: the device
             computes expm1f in fp32 and rounds that, so only there can a last-ulp difference of expm1f move the bf16 result."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    with np.errstate(all="ignore"):
        v = x32.astype(np.float64)
        e = np.where(v > 0, v, np.expm1(v))
        e32 = e.astype(np.float32)
    want = to_bf16(e32)
    nan = np.isnan(e)
    wv = from_bf16(want).astype(np.float64)
    o = _ordinal(want)
    with np.errstate(invalid="ignore"):
        below, above = (wv < e) & ~nan, (wv > e) & ~nan
    lo = np.where(above, _from_ordinal(o - 1), want)
    hi = np.where(below, _from_ordinal(o + 1), want)
    with np.errstate(all="ignore"):
        mid = 0.5 * (from_bf16(lo).astype(np.float64) + from_bf16(hi).astype(np.float64))
        ulp = np.spacing(np.abs(e32)).astype(np.float64)
        in_band = (below | above) & ~(v > 0) & np.isfinite(e) & (np.abs(e - mid) <= BAND_ULPS * ulp)
    return want, lo, hi, in_band


# ---------------------------------------------------------------------------------------------------------------------
# the product
# ---------------------------------------------------------------------------------------------------------------------
def gemm(a_bits, b_bits):
    """C = A B^T in float64 for A [M, K], B [N, K] given as bf16 bits, and unit = 2^-24 |A| |B|^T: one fp32 rounding at the
    magnitude of the dot product.  Non-finite operands follow IEEE (0 * inf = NaN, inf - inf = NaN): those products are formed
    term by term, a BLAS may skip zeros."""
    a = from_bf16(a_bits).astype(np.float64)
    b = from_bf16(b_bits).astype(np.float64)
    with np.errstate(all="ignore"):
        if np.isfinite(a).all() and np.isfinite(b).all():
            c = a @ b.T
        else:
            c = np.zeros((a.shape[0], b.shape[0]))
            for k in range(a.shape[1]):
                c += a[:, k:k + 1] * b[None, :, k]
        unit = (np.abs(a) @ np.abs(b).T) * 2.0 ** -24
    return c, unit


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def hand_list():
    """float32 edge values of the rounding: every exact tie (low half 0x8000) under every bf16 mantissa -- even ones round down,
    odd ones up -- for both signs at a subnormal, the smallest normal, the unit and the largest exponent (the last one of these
    is FIRST_TO_INF_BITS), the two neighbours of every tie at the unit exponent, and the special values."""
    m = np.arange(128, dtype=np.uint32) << 16
    out = []
    for sign in (0, 0x80000000):
        for exp in (0, 1, 127, 254):
            out.append(sign | (exp << 23) | m | 0x8000)
        out.append(sign | (127 << 23) | m | 0x7FFF)
        out.append(sign | (127 << 23) | m | 0x8001)
    special = [0x3F808000, 0x3F818000,                       # 1 + 2^-8 (tie, down), 1 + 3 * 2^-8 (tie, up)
               FLT_MAX_BITS, 0x80000000 | FLT_MAX_BITS, FIRST_TO_INF_BITS, FIRST_TO_INF_BITS - 1, 0x80000000 | FIRST_TO_INF_BITS,
               0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
               0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001,          # NaNs the bare formula would turn into inf / -0
               0x00000001, 0x80000001, 0x00008000, 0x00008001, 0x00007FFF, 0x00018000, 0x007FFFFF, 0x00800000]
    out.append(np.array(special, dtype=np.uint32))
    vals = np.concatenate(out).astype(np.uint32).view(np.float32)
    named = np.array([1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, -2.0 ** -134, 2.0 ** -149, -2.0 ** -149,
                      -20.0, -25.0, -100.0, -17.0, -16.5, -87.5, -1e30, 1e30, -1.0, 1.0, -0.5, 88.0, -1e-8, 1e-8], dtype=np.float32)
    return np.concatenate([vals, named])


def cast_inputs(rows, cols, seed):
    """3 * randn with the hand list scattered in (all of it where rows * cols allows, else a seeded part of it)."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((rows, cols))).astype(np.float32)
    hand = hand_list()
    n = min(hand.size, rows * cols)
    pos = rng.choice(rows * cols, n, replace=False)
    x.reshape(-1)[pos] = hand[rng.permutation(hand.size)[:n]]
    return x


def _bf(x):
    return to_bf16(np.asarray(x, dtype=np.float32))


def _finite_bf16(rng, shape, spread=20):
    """arbitrary finite bf16 values: random sign, all 128 mantissas, exponents spread over +-spread"""
    e = rng.integers(127 - spread, 127 + spread + 1, shape).astype(np.uint16)
    return ((rng.integers(0, 2, shape).astype(np.uint16) << 15) | (e << 7) | rng.integers(0, 128, shape).astype(np.uint16)).astype(np.uint16)


def integers(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return _bf(rng.integers(-8, 9, (m, k))), _bf(rng.integers(-8, 9, (n, k)))


def one_hot(m, n, k, seed):
    """row i of A is non-zero at k = (7 i) mod K only: every C element is ONE product of two 8-bit significands, exact in fp32,
    and lands on the wrong value as soon as a fragment is routed to another k-slot"""
    rng = np.random.default_rng(seed)
    a = np.zeros((m, k), dtype=np.uint16)
    if k:
        a[np.arange(m), (7 * np.arange(m)) % k] = _finite_bf16(rng, m)
    return a, _finite_bf16(rng, (n, k))


def normal(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return _bf(rng.standard_normal((m, k))), _bf(rng.standard_normal((n, k)))


def wide(m, n, k, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, k)) * 2.0 ** rng.integers(-30, 30, (m, 1))
    return _bf(a), _bf(rng.standard_normal((n, k)))


def cancelling(m, n, k, seed):
    """columns 2 j, 2 j + 1 of A hold +t, -t against equal entries of B: those products cancel exactly, and what is left is one
    small term in the last pair: |C| << sum |a b|"""
    rng = np.random.default_rng(seed)
    t = from_bf16(_bf(rng.standard_normal((m, k // 2)))).astype(np.float64)
    a = np.zeros((m, k))
    a[:, 0::2], a[:, 1::2] = t, -t
    b = np.repeat(rng.standard_normal((n, k // 2)), 2, axis=1)
    a[:, k - 2], a[:, k - 1] = rng.standard_normal(m) * 2.0 ** -12, 0.0
    return _bf(a), _bf(b)


def tiny(e):
    def make(m, n, k, seed):
        rng = np.random.default_rng(seed)
        return _bf(rng.standard_normal((m, k)) * 2.0 ** e), _bf(rng.standard_normal((n, k)) * 2.0 ** e)
    make.__name__ = f"tiny({e})"
    return make


MAKERS = {"integers": integers, "one_hot": one_hot, "normal": normal, "wide": wide, "cancelling": cancelling,
          "tiny(-60)": tiny(-60), "tiny(-70)": tiny(-70)}
