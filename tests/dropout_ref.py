"""Reference, masks and cases for the two dropout aggregation kernels of csrc/dropout.hip: spmm_dropout_p3_kernel<CPL> behind
gte_spmm_dropout_p3 (the producer of a dropout layer's two operand images) and spmm_dropout_bwd_kernel<CPL> behind
gte_spmm_dropout_bwd (the transpose aggregation of its backward).  Test infrastructure without a GPU import; checked by
tests/test_dropout_ref_cpu.py (masks against gte_dropout_mask_host, detection power against a float32 emulation of each kernel and
eight mutants of it); tests/test_gpu_dropout_kernels.py runs the kernels on these cases.  Graphs, exact data and bound data are those
of tests/spmm_ref.py.

MASKS.  keep(...) is Philox4x32-10 in numpy, written from the paper and independent of the library: counter {col / 4, row, step mod
2^32, site}, key {seed_lo, seed_hi ^ rank 0x9E3779B9}, word col % 4 kept iff >= threshold(p).  The ABI takes p as fp32, so
threshold(p) = trunc(fp32(p) 2^32 + 0.5) clamped to [0, 2^32 - 1] and scale_f32(p) = fp32(1 / (1 - fp32(p))), the quotient in double.
Masking is a SELECT, as in the kernels: a dropped element is 0 whatever it held (Inf, NaN).

    x'   = fl32(x s) where kept by the site-0 mask at (BATCH row, col), else 0          (in_drop; x otherwise)
    self = fl32(x' s) under the site mask's columns [0, f)                               elementwise: bit-exact for every p
    agg  = s (1 / deg) sum_e w[e] x'[indices[e]] under the site mask's columns [f, 2 f)  float64; 0 on rows of degree 0
    dx[v] = D_self(G[v, :f]) + sum_{v -> u} w_out D_agg(G[u, agg_col : agg_col + f])     float64; row u's agg mask at columns f + c;
                                                                                         D_agg = fl32(G s) where kept

EXACT cases.  x and G integers in [-8, 8], weights from {0.5, 1, 2}, p in {0.5, 0.75} (fp32 exactly; scale 2 and 4).  With the input
mask |x'| <= 32, a row sum of up to 200 terms stays a multiple of 0.5 below 2^15, and s times anything is exact: every product and
every partial sum in any order is a float32.  Producer: fl32(fl32(sum fl32(1 / deg)) s), the device's 1.0f / (float)deg being the
correctly rounded quotient.  Backward: nothing rounds at all.  The kernels are held to this bit for bit.

BOUND cases (spmm_ref.bound_case 'scales' and 'cancel', p in {0.1, 0.3, 0.9}), first order, u = 2^-24:
    forward   |agg - ref| <= (deg + 5) u s (1 / deg) sum |w| |x'|
        the fma chain rounds deg times, each rounding at most u of a partial sum that is at most sum |w| |x'| (the padded lanes of the
        last quad add w = 0 times a finite value: nothing); fl32(1 / deg), the multiplication by it and the multiplication by s are
        three more; one of slack.  x' enters at its fp32 value (the reference applies the input mask in float32, as an elementwise
        product that the device rounds identically), so the input mask adds no term.
    backward  |dx - ref| <= (deg_out + 3) u (|D_self| + sum |w_out| |D_agg|)
        the fma chain rounds deg_out times, each rounding at most u of a partial sum that is at most sum |w_out| |D_agg|; the product
        G s of the self half rounds once, u |D_self|; the final addition once, u of at most the bracket; one of slack.  As x' in the
        forward, the aggregated operand D_agg enters at its fp32 value fl32(G s) (an elementwise product that the device rounds as
        numpy does), so it adds no term; D_self is the exact product, its rounding is the one counted.  The unit of slack also
        covers a kernel that would aggregate the unrounded G s: u of every term, together u of the sum.
A dropped position has bound 0: anything but an exact zero there is infinitely wrong (spmm_ref.ratio).
"""
import numpy as np

from tests import spmm_ref as sr
from tests.spmm_ref import U, Graph, ladder_graph, LADDER, LADDER_N, OTHER, same_bits, inv_deg_f32, _fma      # noqa: F401 (re-exported)

M32 = 0xFFFFFFFF
WAVE = 64             # lanes of a wave: a lane owns one quarter (4 features) of up to CPL stretches of 256 features
UNROLL = 4            # kEdgeUnroll (dropout.hip)


# ---- masks --------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds (Salmon et al. 2011, the Random123 constants) on uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(M32), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(M32)]
        k0 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32)
        k1 = (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """dropout::threshold of csrc/dropout.h on the fp32 value of p: keep iff word >= round(p 2^32), clamped to [0, 2^32 - 1]"""
    t = float(np.float32(p)) * 4294967296.0 + 0.5
    if not t > 0.0:
        return 0
    if t >= 4294967295.0:
        return M32
    return int(t)


def scale_f32(p):
    """dropout::scale: fp32(1 / (1 - p)) with the quotient in double, from the fp32 value of p"""
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep(p, seed, rank, step, site, n_rows, n_cols, rows=None, col0=0):
    """keep(seed, rank, step, site, row, col) of include/gte.h as uint8 [rows, n_cols]: counter {col / 4, row, step, site}, key
    {seed_lo, seed_hi ^ rank 0x9E3779B9}, word col % 4 kept iff >= round(p 2^32).  ``rows``: the row words (default 0 .. n_rows - 1);
    ``col0``: the first column."""
    thr = threshold(p)
    k0, k1 = seed & M32, ((seed >> 32) & M32) ^ ((rank * 0x9E3779B9) & M32)
    rows = np.arange(n_rows) if rows is None else np.asarray(rows)
    rows = rows.astype(np.uint64)[:, None]
    cols = (np.arange(n_cols, dtype=np.uint64) + np.uint64(col0))[None, :]
    words = philox4x32_10(cols >> np.uint64(2), rows, step, site, k0, k1)
    u = np.choose((cols & np.uint64(3)).astype(np.int64) + 0 * rows.astype(np.int64), words)
    return (u >= thr).astype(np.uint8)


# ---- the contract of the dispatch, named here so that a changed threshold fails tests/test_dropout_ref_cpu.py visibly ---------------
def c16(f):
    return -(-f // 16) * 16


def c4(f):
    return -(-f // 4) * 4


def _cpl(quarters):
    return 1 if quarters <= WAVE else 2 if quarters <= 2 * WAVE else 4


def producer_cpl(f):
    """CPL of gte_spmm_dropout_p3: by the quarters of an image row, nqp = 4 ceil(f / 16)"""
    return _cpl(c16(f) // 4)


def bwd_cpl(f):
    """CPL of gte_spmm_dropout_bwd: by the quarters that hold features, ceil(f / 4)"""
    return _cpl(c4(f) // 4)


def producer_passes(f):
    """trips of the producer's qb loop"""
    return -(-(c16(f) // 4) // (WAVE * producer_cpl(f)))


def bwd_passes(f):
    return -(-(c4(f) // 4) // (WAVE * bwd_cpl(f)))


# ---- the cases of tests/test_gpu_dropout_kernels.py -----------------------------------------------------------------------------------
# one width on either side of 64, 128 and 256 quarters; 6: the residue f % 4 == 2 at one quarter stretch per lane, which the other
# widths up to 256 lack
PRODUCER_WIDTHS = [1, 3, 4, 5, 6, 13, 16, 17, 255, 256, 257, 259, 510, 512, 513, 831, 1023, 1024, 1025, 1030]
BWD_WIDTHS = [1, 3, 6, 13, 255, 256, 257, 258, 511, 512, 513, 1000, 1024, 1025, 1027, 1030]
PRODUCER_BOUND_WIDTHS = [13, 259, 1030]
BWD_BOUND_WIDTHS = [13, 258, 1030]
EXACT_P = [0.5, 0.75]
BOUND_P = [0.1, 0.3, 0.9]
STEPS = [0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 5]        # the last is step 5: the kernels cut the counter to 32 bits
P_LOW = 2.0 ** -34                                       # threshold 0: everything kept, scale 1
P_HIGH = float(np.nextafter(np.float32(1), np.float32(0)))   # 1 - 2^-24: keep rate 2^-24, scale 2^24
# a p = k / 1000 at which fp32(1 / (1 - p)) from the double p differs from scale_f32(p) (tests/test_dropout_ref_cpu.py sweeps them)
P_SWEPT = 0.111
SELF_P = [0.1, 0.2, 0.3, 0.5, 0.9, P_SWEPT, P_LOW, P_HIGH]
BASE = dict(seed=99, rank=0, step=3, site=1)
# (seed, rank, step, site): seeds with the high word set, rank 3, sites 1, 2, 7, every step of STEPS
COORDS = [((0xDEADBEEF << 32) | 5, 0, 3, 1), (2 ** 64 - 1, 3, 0, 2), ((1 << 40) + 7, 3, 1, 7), (42, 0, 2 ** 31, 2),
          (42, 3, 2 ** 32 - 1, 1), ((1 << 63) | 11, 1, 2 ** 32 + 5, 7)]
COORD_WIDTHS = [13, 259]
CONFINE_WIDTHS = [13, 259, 1030]
RES_EXTRA = 51        # resident rows beyond the batch's in the row-map cases


def coords(f):
    """the (seed, rank, step, site) of width f's exact case: the base coordinates with a seed of the width's own"""
    return dict(BASE, seed=BASE["seed"] + 1000003 * f)


def bwd_graph():
    """the out-CSR handed to the backward: a ladder graph of its own (row v lists the nodes u that v feeds; out-degrees 0 ... 200)"""
    return ladder_graph(seed=1)


def confine_graph(node):
    """the ladder graph with ``node`` as the LAST edge of the second 5-edge row (row 38): the second quad of that row re-reads it
    three times at w = 0"""
    g = ladder_graph()
    assert g.deg[38] == 5
    ix = g.indices.copy()
    ix[g.indptr[38] + 4] = node
    return g.with_indices(ix)


def row_map(n, n_res, seed=0):
    """n distinct resident rows in shuffled order with row_map[u] != u for every u"""
    rng = np.random.default_rng(8000 + seed)
    rows = rng.permutation(n_res)[:n]
    spare = np.setdiff1d(np.arange(n, n_res), rows)
    fixed = np.flatnonzero(rows == np.arange(n))
    assert len(fixed) <= len(spare)
    rows[fixed] = spare[:len(fixed)]
    assert (rows != np.arange(n)).all() and len(np.unique(rows)) == n
    return rows.astype(np.int32)


def exact_grad(n, f, agg_col, ldg, seed=0):
    """G [n, ldg] float32: integers in [-8, 8] in the two halves, NaN in every other column (the kernels read whole quarters
    and select: the padding must not matter)"""
    rng = np.random.default_rng(9000 + 17 * f + seed)
    G = np.full((n, ldg), np.nan, dtype=np.float32)
    G[:, :f] = rng.integers(-8, 9, (n, f))
    G[:, agg_col:agg_col + f] = rng.integers(-8, 9, (n, f))
    return G


def bound_grad(x, base, agg_col, ldg):
    n, f = x.shape
    G = np.full((n, ldg), np.nan, dtype=np.float32)
    G[:, :f] = x
    G[:, agg_col:agg_col + f] = base
    return G


def producer_exact_case(f, weights=True):
    """(graph, w or None, res [n + RES_EXTRA, f], rows): the batch's x is res[:n] as plain rows or as an image of its own, and
    res[rows] through the row map into the resident image of res"""
    g = ladder_graph()
    w, res, _ = sr.exact_case(g, f, weights=weights, n_src=g.n + RES_EXTRA)
    return g, w, res, row_map(g.n, g.n + RES_EXTRA, seed=f)


def producer_bound_case(f, kind):
    g, w, x, _ = sr.bound_case(ladder_graph(), f, kind)
    return g, w, x


def bwd_exact_case(f, agg_col, ldg):
    g = bwd_graph()
    return g, sr.exact_case(g, f)[0], exact_grad(g.n, f, agg_col, ldg)


def bwd_bound_case(f, kind, agg_col, ldg):
    g, w, x, base = sr.bound_case(bwd_graph(), f, kind)
    return g, w, bound_grad(x, base, agg_col, ldg)


# ---- reference ----------------------------------------------------------------------------------------------------------------------
def _select(m, a):
    return np.where(m != 0, a, np.zeros((), dtype=a.dtype))


def input_dropped(x, p, seed, rank, step, in_drop):
    """x' as float32: fl32(x s) where the site-0 mask keeps (batch row, col), 0 elsewhere; x itself without input dropout"""
    x = np.asarray(x, dtype=np.float32)
    if not in_drop:
        return x
    with np.errstate(invalid="ignore", over="ignore"):
        return _select(keep(p, seed, rank, step, 0, x.shape[0], x.shape[1]), x * scale_f32(p))


def producer_ref(g, w, x, p, seed, rank, step, site, in_drop):
    """(self float32 [n, f], agg float64 [n, f]) of the module docstring; x holds the n batch rows"""
    n, f = np.shape(x)
    s = scale_f32(p)
    xd = input_dropped(x, p, seed, rank, step, in_drop)
    m = keep(p, seed, rank, step, site, n, 2 * f)
    with np.errstate(invalid="ignore", over="ignore"):
        self_img = _select(m[:, :f], xd * s)
        agg = _select(m[:, f:], float(s) * sr.ref(g.indptr, g.indices, w, xd, True))
    return self_img, agg


def producer_bound(g, w, x, p, seed, rank, step, site, in_drop):
    n, f = np.shape(x)
    xd = input_dropped(x, p, seed, rank, step, in_drop)
    m = keep(p, seed, rank, step, site, n, 2 * f)
    return _select(m[:, f:], (g.deg[:, None] + 5) * U * float(scale_f32(p)) * sr.mag(g.indptr, g.indices, w, xd, True))


def producer_expect(g, w, x, p, seed, rank, step, site, in_drop):
    """the kernel's two images on an exact case, float32"""
    n, f = np.shape(x)
    s = scale_f32(p)
    assert float(s) in (2.0, 4.0), "not an exact case: the scale is no small power of two"
    xd = input_dropped(x, p, seed, rank, step, in_drop)
    m = keep(p, seed, rank, step, site, n, 2 * f)
    return _select(m[:, :f], xd * s), _select(m[:, f:], sr.expect_exact(g, w, xd, True) * s)


def _bwd_halves(G, agg_col, f, p, seed, rank, step, site):
    """(D_self float64: the exact product G s; D_agg: the AGGREGATED operand at its fp32 value fl32(G s), as x' in the producer)"""
    G = np.asarray(G)
    m = keep(p, seed, rank, step, site, G.shape[0], 2 * f)
    s = scale_f32(p)
    with np.errstate(invalid="ignore", over="ignore"):
        return (_select(m[:, :f], G[:, :f].astype(np.float64) * float(s)),
                _select(m[:, f:], (G[:, agg_col:agg_col + f].astype(np.float32) * s).astype(np.float64)))


def bwd_self_f32(G, f, p, seed, rank, step, site):
    """D_self as the kernel holds it, float32: fl32(G s) where kept -- all of dx on a row without out-edges, bit for bit for every p"""
    G = np.asarray(G, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return _select(keep(p, seed, rank, step, site, G.shape[0], f), G[:, :f] * scale_f32(p))


def bwd_ref(g_out, w_out, G, agg_col, f, p, seed, rank, step, site):
    """dx float64 [n, f]"""
    dself, dagg = _bwd_halves(G, agg_col, f, p, seed, rank, step, site)
    with np.errstate(invalid="ignore", over="ignore"):
        return dself + sr.ref(g_out.indptr, g_out.indices, w_out, dagg, False)


def bwd_bound(g_out, w_out, G, agg_col, f, p, seed, rank, step, site):
    dself, dagg = _bwd_halves(G, agg_col, f, p, seed, rank, step, site)
    return (g_out.deg[:, None] + 3) * U * (np.abs(dself) + sr.mag(g_out.indptr, g_out.indices, w_out, dagg, False))


def bwd_expect(g_out, w_out, G, agg_col, f, p, seed, rank, step, site):
    """the kernel's dx on an exact case, float32: nothing rounds"""
    r = bwd_ref(g_out, w_out, G, agg_col, f, p, seed, rank, step, site)
    out = r.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), r), "not an exact case: a result is not a float32"
    return out


# ---- float32 emulations of the two kernels ------------------------------------------------------------------------------------------
MUTANTS = {
    "a": "agg-half mask columns at c instead of f + c",
    "b": "input mask of a source keyed by the resident row instead of the batch row",
    "c": "a tail lane's weight not zeroed",
    "d": "D_0 applied to the destination row only, not to the sources",
    "e": "the unaligned keep4 shift off by one",
    "f": "backward agg mask keyed by the destination v instead of the source u",
    "g": "the column of pass qb > 0 computed as in pass 0",
    "h": "1 / deg taken over the padded quad count",
}
PRODUCER_MUTANTS = ["a", "b", "c", "d", "e", "g", "h"]
BWD_MUTANTS = ["a", "c", "e", "f", "g"]


def _chain(g, w, term, keep_tail_weight):
    """the CSR-order fma chain of both kernels, all columns of a row at once: quads of four edges, the slots past the row's end
    clamped to the last edge at weight 0; term(v, u) is what the lanes hold of source u"""
    wv = np.ones(g.nnz, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    out = None
    for v in range(g.n):
        lo, hi = int(g.indptr[v]), int(g.indptr[v + 1])
        acc = None
        for e0 in range(lo, hi, UNROLL):
            for k in range(UNROLL):
                e = min(e0 + k, hi - 1)
                wk = wv[e] if (e0 + k < hi or keep_tail_weight) else np.float32(0)
                t = term(v, int(g.indices[e]))
                acc = _fma(wk, t, np.zeros_like(t) if acc is None else acc)
        if acc is not None:
            if out is None:
                out = np.zeros((g.n, len(acc)), dtype=np.float32)
            out[v] = acc
    return out


def _mask_halves(p, seed, rank, step, site, n, f, col, mutant):
    m = keep(p, seed, rank, step, site, n, 2 * f + 1)
    off = 0 if mutant == "a" else f
    if mutant == "e" and f % 4 != 0:          # ((lo | hi << 4) >> (s + 1)) & 15: bit j is column col0 + j + 1
        off += 1
    return m[:, col], m[:, off + col]


def emulate_producer(g, w, x, p, seed, rank, step, site, in_drop, x_rows=None, mutant=None):
    """spmm_dropout_p3_kernel in float32 numpy -> (self, agg) [n, f].  ``x`` holds the batch rows (already gathered); ``x_rows`` is
    the row map they came through, which only mutant b looks at."""
    assert mutant is None or mutant in PRODUCER_MUTANTS
    x = np.asarray(x, dtype=np.float32)
    n, f = x.shape
    s = scale_f32(p)
    col = np.arange(f)
    if mutant == "g":
        col = col % (4 * WAVE * producer_cpl(f))
    xc = x[:, col]
    with np.errstate(invalid="ignore", over="ignore"):
        if in_drop:
            x_self = _select(keep(p, seed, rank, step, 0, n, f)[:, col], xc * s)
            src_rows = x_rows if (mutant == "b" and x_rows is not None) else None
            x_src = xc if mutant == "d" else _select(keep(p, seed, rank, step, 0, n, f, rows=src_rows)[:, col], xc * s)
        else:
            x_self = x_src = xc
        ms, ma = _mask_halves(p, seed, rank, step, site, n, f, col, mutant)
        acc = _chain(g, w, lambda v, u: x_src[u], mutant == "c")
        if acc is None:
            acc = np.zeros((n, f), dtype=np.float32)
        deg = (-(-g.deg // UNROLL) * UNROLL) if mutant == "h" else g.deg
        sv = np.where(g.deg > 0, np.float32(1.0) / np.maximum(deg, 1).astype(np.float32), np.float32(0.0)).astype(np.float32)
        return _select(ms, x_self * s), _select(ma, (acc * sv[:, None]) * s)


def emulate_bwd(g_out, w_out, G, agg_col, f, p, seed, rank, step, site, mutant=None):
    """spmm_dropout_bwd_kernel in float32 numpy -> dx [n, f]"""
    assert mutant is None or mutant in BWD_MUTANTS
    G = np.asarray(G, dtype=np.float32)
    n = G.shape[0]
    s = scale_f32(p)
    col = np.arange(f)
    if mutant == "g":
        col = col % (4 * WAVE * bwd_cpl(f))
    ms, ma = _mask_halves(p, seed, rank, step, site, n, f, col, mutant)
    with np.errstate(invalid="ignore", over="ignore"):
        ga = G[:, agg_col + col] * s
        if mutant == "f":
            term = lambda v, u: _select(ma[v], ga[u])
        else:
            dagg = _select(ma, ga)
            term = lambda v, u: dagg[u]
        acc = _chain(g_out, w_out, term, mutant == "c")
        if acc is None:
            acc = np.zeros((n, f), dtype=np.float32)
        return _select(ms, G[:, col] * s) + acc
