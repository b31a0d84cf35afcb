"""float64 reference, graphs and data for the neighbour aggregation kernels (csrc/spmm_csr.hip: the row kernels, the edge-parallel
kernel, the image and LayerNorm forms; csrc/spmm_tiled.hip):

    out[v, :] = scale_v * sum_{e in row v} w[e] * x[indices[e], :]   (+ base[v, :] when accumulating),  scale_v = 1 or 1 / deg(v)

Test infrastructure without a GPU import; pinned to oracle.gcnsage_cpu.spmm_csr_numpy and to torch.sparse_csr in float64, and
checked for detection power against a float32 emulation of the row kernel and five mutants of it, by tests/test_spmm_ref_cpu.py.
tests/test_gpu_spmm_edges.py runs the kernels on these cases.

EXACT cases.  x integer valued, weights from {0.5, 1, 2}: every product, every partial sum in ANY order and every result is a
multiple of 0.5 far below 2^24 (fp32: |x| <= 8, degree <= 200: |sum| <= 3200) or an integer of magnitude <= 256 (bf16: x in
{-1, 0, 1}, w in {1, 2} on rows up to degree 64, w = 1 above, integer base in [-50, 50]), representable in the OUTPUT type.  The
expected result does not depend on the summation order, so the kernels are held to it bit for bit.  mean: fl32(sum * fl32(1 / deg))
(the library is built without fast-math: the device's 1.0f / (float)deg is the correctly rounded quotient), then round-to-nearest-
even to bf16 for bf16.  Accumulating with mean, `o += acc * scale` may or may not be contracted into one fma by the compiler: bitwise
only where scale is a power of two (the product is exact either way), the other rows go under the bound -- exact_rows() says which.

BOUND cases.  Two kinds of data, 'scales' (column j of x scaled by 2^k_j, k_j in [-30, 30]) and 'cancel' (on every odd row each odd
edge repeats the even edge before it with the weight negated and perturbed by 1e-3: the row's sum is a thousandth of its terms).
    |got - ref| <= (deg + 4) 2^-24 mag scale_v  [+ half a bf16 ulp of ref for bf16 output]  [+ 2^-24 (|base| + |ref|) when accumulating]
with mag = sum_e |w[e]| |x[indices[e], :]|.  First order: the fma chain over the row rounds deg times, each rounding at most
2^-24 of a partial sum that is at most mag, in any order including the edge-parallel kernel's 64-edge partials and their sum; 1 / deg
and the multiplication by it are two more; one of slack.  Inputs stay within 2^+-60: no subnormals, no overflow.  bf16 keeps 8
significant bits: half an ulp of ref is 2^(floor(log2 |ref|) - 8), between 2^-9 |ref| (just below a power of two) and 2^-8 |ref|
(just above one).  A flat 2^-9 |ref| would be broken by the correctly rounded result itself (1.00390625 lies 2^-8 from both of its
bf16 neighbours), so the term is the half ulp, computed exactly by bf16_half_ulp().
"""
import numpy as np

U = 2.0 ** -24

# ---- the contract of the kernels, named here so that a changed threshold fails tests/test_spmm_ref_cpu.py visibly ---------------
UNROLL = 4            # kEdgeUnroll (spmm_csr.hip): source rows in flight per lane group
EP_SEG = 64           # edges per segment of the edge-parallel kernel
TILE_R = 32           # destination rows per tile (spmm_tiled.hip)
UMAX = 128            # distinct sources a tile may stage
EMAX = 448            # edges a tile may stage, spmm_tiled_kernel (any width)
EMAX_FULL = 512       # ... spmm_tiled_full_kernel (widths that are a multiple of TILED_FC with at least four chunks)
TILED_FC = 32         # floats per feature chunk of the tiled kernels

LADDER = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
LADDER_N = 131        # rows: the last block is partial for every rows-per-wave count (64 / G, G = 4 ... 64)
OTHER = 77            # the second poisoned node of the confinement tests (node 0 is the first)

# one width on either side of every threshold of dispatch() (fp32: chunks of 4, bf16: of 8; 1027 | 1028 and 2055 | 2056 straddle the
# second 256-chunk feature block of GTE_L(64, 4))
F32_WIDTHS = [1, 3, 13, 16, 19, 20, 35, 36, 67, 68, 131, 132, 259, 260, 515, 516, 831, 1027, 1028]
BF16_WIDTHS = [7, 13, 71, 72, 135, 136, 263, 264, 519, 520, 1031, 1032, 2055, 2056]
P3_WIDTHS = [1, 3, 13, 16, 19, 35, 67, 100, 259, 831]
LN_WIDTHS = [16, 32, 64, 128, 256, 512, 1024]            # one per lane-group form of gte_spmm_csr_accumulate_ln
EDGE_WIDTHS = [1, 13, 64, 255, 256, 257, 512, 513, 831]  # ceil(F / 4) crosses 64 and 128: one, two, four chunks per lane
TILED_WIDTHS = [32, 33, 96, 128, 160, 192, 224, 256]     # generic kernel; full kernel at 4, 5, 6, 7, 8 chunks
CONFINE_F32_WIDTHS = [13, 16, 64, 260]
CONFINE_BF16_WIDTHS = [13]


def row_group(n_feat, bf16=False):
    """(G, CPL) of dispatch() in spmm_csr.hip: lanes per destination row, 16-byte chunks per lane"""
    epc = 8 if bf16 else 4
    nchunk = n_feat // epc
    if nchunk <= 8:
        return (4, 1) if (nchunk <= 4 and not bf16) else (8, 1)
    for limit, form in ((16, (16, 1)), (32, (32, 1)), (64, (32, 2)), (128, (64, 2))):
        if nchunk <= limit:
            return form
    return (64, 4)


def edge_cpl(n_feat):
    nchunk = -(-n_feat // 4)
    return 1 if nchunk <= 64 else 2 if nchunk <= 128 else 4


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
class Graph:
    """CSR over ``n`` destination rows; sources are row numbers of x below ``n`` (the tests append one row no edge names)"""

    def __init__(self, degrees, indices):
        self.deg = np.asarray(degrees, dtype=np.int64)
        self.n = len(self.deg)
        self.indptr = np.concatenate([[0], np.cumsum(self.deg)]).astype(np.int32)
        self.indices = np.asarray(indices, dtype=np.int32)
        assert len(self.indices) == int(self.indptr[-1])
        self.row_of_edge = np.repeat(np.arange(self.n), self.deg)

    @property
    def nnz(self):
        return len(self.indices)

    def names(self, node):
        """per destination row: is ``node`` one of its sources"""
        hit = np.zeros(self.n, dtype=bool)
        hit[self.row_of_edge[self.indices == node]] = True
        return hit

    def with_indices(self, indices):
        return Graph(self.deg, indices)


def ladder_degrees():
    low = [1, 2, 3, 0, 5, 6]
    # the second copy reversed, right behind the first: degree LADDER[i] sits on rows i and 43 - i, an odd distance apart, so its two
    # rows fall on different lane groups of a wave for every rows-per-wave count 2 ... 16
    d = LADDER + LADDER[::-1]
    d += [low[i % len(low)] for i in range(LADDER_N - len(d))]
    return d


def ladder_graph(seed=0):
    rng = np.random.default_rng(1000 + seed)
    deg = ladder_degrees()
    g = Graph(deg, rng.integers(0, LADDER_N, int(np.sum(deg))))
    ix = g.indices.copy()
    # node 0 and node OTHER are sources of some rows and not of others whatever the draw: rows 1 and 3 name node 0, row 2 names OTHER
    # (rows 1, 2, 3 have 1, 2, 3 edges: a quad with 3, 2, 1 lanes past the row end)
    ix[g.indptr[1]] = 0
    ix[g.indptr[2] + 1] = OTHER
    ix[g.indptr[3] + 2] = 0
    lo5, hi5 = g.indptr[5], g.indptr[6]
    ix[lo5:hi5] = np.where(np.isin(ix[lo5:hi5], (0, OTHER)), 5, ix[lo5:hi5])      # the 5-edge row names neither
    return g.with_indices(ix)


SEGMENT_DEGREES = [0, 0, 3, 61, 0, 64, 128, 1, 0, 0, 62, 130, 63, 200, 5, 0]


def segment_graph(extra=0, seed=0):
    """extra 0: 717 edges; 1: one more row of 51 edges (768 = 12 whole segments); 2: and a one-edge row (a one-edge last segment)"""
    deg = SEGMENT_DEGREES + [51, 1][:extra]
    rng = np.random.default_rng(2000 + seed)
    return Graph(deg, rng.integers(0, len(deg), int(np.sum(deg))))


TILE_NAMES = ["e448", "e449", "e512", "e513", "u128", "u129", "empty", "partial"]


def tile_graph(seed=0):
    """eight tiles of TILE_R rows: EMAX, EMAX + 1, EMAX_FULL, EMAX_FULL + 1 edges over at most 96 distinct sources; UMAX and UMAX + 1
    distinct sources (four edges a row); an empty tile; a last tile of seven rows"""
    rng = np.random.default_rng(3000 + seed)
    deg, ix = [], []
    n = 7 * TILE_R + 7
    for t, (per_row, plus) in enumerate([(EMAX // TILE_R, 0), (EMAX // TILE_R, 1), (EMAX_FULL // TILE_R, 0), (EMAX_FULL // TILE_R, 1)]):
        d = [per_row] * TILE_R
        d[(5 * t + 3) % TILE_R] += plus
        deg += d
        ix.append(rng.integers(20 * t, 20 * t + 96, int(np.sum(d))))
    for plus in (0, 1):
        d = [UMAX // TILE_R] * TILE_R
        d[17] += plus
        deg += d
        ix.append(rng.permutation(np.arange(40, 40 + UMAX + plus)))
    deg += [0] * TILE_R
    last = [3, 0, 5, 1, 14, 2, 9]
    deg += last
    ix.append(rng.integers(0, n, int(np.sum(last))))
    return Graph(deg, np.concatenate(ix))


def cycle_graph(n, n_src=LADDER_N, seed=0):
    """``n`` rows of cycling low degrees (the multi-pass launches: more rows than one pass of the grid covers)"""
    rng = np.random.default_rng(4000 + seed)
    deg = np.resize(np.array([0, 1, 2, 3, 4, 5, 1, 2]), n)
    return Graph(deg, rng.integers(0, n_src, int(deg.sum())))


def tile_facts(g):
    """per tile: (edges, distinct sources)"""
    out = []
    for r0 in range(0, g.n, TILE_R):
        lo, hi = g.indptr[r0], g.indptr[min(r0 + TILE_R, g.n)]
        out.append((int(hi - lo), len(np.unique(g.indices[lo:hi]))))
    return out


def inside_one_segment(g):
    """rows whose edges lie inside one EP_SEG-aligned segment (or that have none): the edge-parallel kernel sums them in CSR order"""
    lo, hi = g.indptr[:-1].astype(np.int64), g.indptr[1:].astype(np.int64)
    return (g.deg == 0) | (lo // EP_SEG == (hi - 1) // EP_SEG)


# ---- reference ----------------------------------------------------------------------------------------------------------------------
def _row_sums(indptr, indices, w, x, absolute, block):
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    n, f = len(indptr) - 1, x.shape[1]
    out = np.zeros((n, f))
    if len(indices) == 0:
        return out
    has = np.diff(indptr) > 0
    starts = indptr[:-1][has]
    wv = None if w is None else np.asarray(w, dtype=np.float64)[:, None]
    if absolute and wv is not None:
        wv = np.abs(wv)
    for c0 in range(0, f, block):
        p = x[indices, c0:c0 + block]
        if absolute:
            p = np.abs(p)
        if wv is not None:
            p = p * wv
        out[has, c0:c0 + block] = np.add.reduceat(p, starts, axis=0)
    return out


def _scale(indptr, mean):
    deg = np.diff(np.asarray(indptr, dtype=np.int64))
    if not mean:
        return np.ones(len(deg))
    return np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)


def ref(indptr, indices, w, x, mean, base=None, block=256):
    """float64: scale_v * sum_e w[e] x[indices[e]] (+ base); rows without edges give 0 (base unchanged); w None = unit weights"""
    out = _row_sums(indptr, indices, w, x, False, block) * _scale(indptr, mean)[:, None]
    return out if base is None else out + np.asarray(base, dtype=np.float64)


def mag(indptr, indices, w, x, mean, block=256):
    """float64: scale_v * sum_e |w[e]| |x[indices[e]]|"""
    return _row_sums(indptr, indices, w, x, True, block) * _scale(indptr, mean)[:, None]


def bound(g, w, x, mean, ref_val, base=None, bf16=False):
    b = (g.deg[:, None] + 4) * U * mag(g.indptr, g.indices, w, x, mean)
    if bf16:
        b = b + bf16_half_ulp(ref_val)
    if base is not None:
        b = b + U * (np.abs(np.asarray(base, dtype=np.float64)) + np.abs(ref_val))
    return b


def ratio(got, ref_val, bnd):
    """largest |got - ref| / bound (0 / 0 = 0; a non-finite result is infinitely wrong)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref_val)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bnd))) if err.size else 0.0


# ---- number formats -----------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even) as float32; finite input"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def bf16_half_ulp(a):
    """half the spacing of bf16 (8 significant bits) at |a|: 2^(floor(log2 |a|) - 8); 0 at 0"""
    m, e = np.frexp(np.abs(np.asarray(a, dtype=np.float64)))           # |a| = m 2^e, m in [0.5, 1)
    return np.where(m > 0, np.ldexp(1.0, e - 9), 0.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """bitwise equality of two float32 arrays (no - 0 arises: every sum starts at + 0 and x + (-x) rounds to + 0)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all(bits(a) == bits(b)))


# ---- exact cases --------------------------------------------------------------------------------------------------------------------
def exact_case(g, n_feat, bf16=False, seed=0, weights=True, n_src=None):
    """(w or None, x [n_src or n, n_feat], base [n, n_feat]) as float32 holding values exact in the output type"""
    rng = np.random.default_rng(5000 + 17 * n_feat + seed)
    n_src = g.n if n_src is None else n_src
    if bf16:
        x = rng.integers(-1, 2, (n_src, n_feat))
        w = np.where(g.deg[g.row_of_edge] <= 64, rng.choice([1.0, 2.0], g.nnz), 1.0)
    else:
        x = rng.integers(-8, 9, (n_src, n_feat))
        w = rng.choice([0.5, 1.0, 2.0], g.nnz)
    base = rng.integers(-50, 51, (g.n, n_feat))
    return (w.astype(np.float32) if weights else None), x.astype(np.float32), base.astype(np.float32)


def inv_deg_f32(g):
    d = np.maximum(g.deg, 1).astype(np.float32)
    return np.where(g.deg > 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)


def expect_exact(g, w, x, mean, base=None, bf16=False):
    """the kernels' result on an exact case, float32 (bf16: the bf16 value as float32).  Unfused accumulate: see exact_rows()."""
    s = ref(g.indptr, g.indices, w, x, False)
    out = s.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), s), "not an exact case: a row sum is not a float32"
    if mean:
        out = out * inv_deg_f32(g)[:, None]
    if base is not None:
        out = out + np.asarray(base, dtype=np.float32)
    return bf16_round(out) if bf16 else out


def exact_rows(g, mean, accumulate):
    """rows on which expect_exact() holds bit for bit: all, but accumulating with mean only where 1 / deg is a power of two"""
    if not (mean and accumulate):
        return np.ones(g.n, dtype=bool)
    return (g.deg & (g.deg - 1)) == 0


# ---- bound cases --------------------------------------------------------------------------------------------------------------------
BOUND_KINDS = ["scales", "cancel"]


def bound_case(g, n_feat, kind, bf16=False, seed=0):
    """(graph, w, x, base): 'scales' on ``g`` itself, 'cancel' on a copy whose odd rows repeat every even edge's source"""
    rng = np.random.default_rng(6000 + 17 * n_feat + seed)
    w = rng.uniform(0.5, 1.5, g.nnz)
    x = rng.standard_normal((g.n, n_feat))
    base = rng.standard_normal((g.n, n_feat))
    if kind == "scales":
        col = 2.0 ** rng.integers(-30, 31, n_feat)
        x, base = x * col, base * col
    else:
        pos = np.arange(g.nnz) - g.indptr[:-1].astype(np.int64)[g.row_of_edge]
        twin = (g.row_of_edge % 2 == 1) & (pos % 2 == 1)
        ix = g.indices.copy()
        ix[twin] = ix[np.flatnonzero(twin) - 1]
        w[twin] = -w[np.flatnonzero(twin) - 1] * (1.0 + 1e-3 * rng.standard_normal(int(twin.sum())))
        g = g.with_indices(ix)
    w, x, base = w.astype(np.float32), x.astype(np.float32), base.astype(np.float32)
    if bf16:
        x, base = bf16_round(x), bf16_round(base)
    return g, w, x, base


# ---- float32 emulations of the kernels' summation orders ---------------------------------------------------------------------------
def _fma(a, b, c):
    """float32 fma through float64: the product of two float32 is exact there"""
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


MUTANTS = ["drop_last_mod4", "shift_weight", "mean_deg_plus_1", "tail_reads_col0", "skip_second_trip"]


def emulate_rows(g, w, x, mean, base=None, bf16=False, mutant=None):
    """spmm_csr_kernel in float32 numpy, all columns of a row at once: the row's edges in trips of G (one per lane), inside a trip
    groups of four with the slots past the end clamped to the last edge at weight 0, one fma per slot in CSR order.  ``mutant``
    breaks it in one of the five ways named in MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(x, dtype=np.float32)
    n_feat = x.shape[1]
    G, _ = row_group(n_feat, bf16)
    epc = 8 if bf16 else 4
    ntail0 = (n_feat // epc) * epc
    if mutant == "tail_reads_col0":                       # tail_off = li instead of nchunk * EPC + li
        x = x.copy()
        x[:, ntail0:] = x[:, :n_feat - ntail0]
    wv = np.ones(g.nnz, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    out = np.zeros((g.n, n_feat), dtype=np.float32)
    for v in range(g.n):
        lo, hi = int(g.indptr[v]), int(g.indptr[v + 1])
        deg = hi - lo
        if mutant == "drop_last_mod4" and deg % 4 == 1:
            hi -= 1
        acc = np.zeros(n_feat, dtype=np.float32)
        for eb in range(lo, hi, G):
            if mutant == "skip_second_trip" and eb > lo:
                break
            cnt = min(G, hi - eb)
            for t in range(0, cnt, UNROLL):
                ws = [wv[eb + min(t + k, cnt - 1)] if t + k < cnt else np.float32(0) for k in range(UNROLL)]
                if mutant == "shift_weight":
                    ws = [ws[0]] + ws[:-1]
                for k in range(UNROLL):
                    acc = _fma(ws[k], x[g.indices[eb + min(t + k, cnt - 1)]], acc)
        if mean:
            d = deg + 1 if mutant == "mean_deg_plus_1" else deg
            acc = acc * (np.float32(1.0) / np.float32(d) if deg > 0 else np.float32(0.0))
        out[v] = acc
    if base is not None:
        out = out + np.asarray(base, dtype=np.float32)
    return bf16_round(out) if bf16 else out


def emulate_segments(g, w, x, mean):
    """the edge-parallel kernel's order in float32: a row's edges cut at the EP_SEG-aligned boundaries, one fma chain per piece, the
    pieces added in order, then the scale"""
    x = np.asarray(x, dtype=np.float32)
    wv = np.ones(g.nnz, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    out = np.zeros((g.n, x.shape[1]), dtype=np.float32)
    for v in range(g.n):
        lo, hi = int(g.indptr[v]), int(g.indptr[v + 1])
        total = None
        e = lo
        while e < hi:
            se = min(hi, (e // EP_SEG + 1) * EP_SEG)
            acc = np.zeros(x.shape[1], dtype=np.float32)
            for t in range(e, se):
                acc = _fma(wv[t], x[g.indices[t]], acc)
            total = acc if total is None else total + acc
            e = se
        if total is not None:
            out[v] = total * (np.float32(1.0) / np.float32(hi - lo)) if mean else total
    return out
