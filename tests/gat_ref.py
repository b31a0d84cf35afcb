"""Reference for the GAT attention kernels (csrc/gat.hip, csrc/gat_rows.h): plain numpy, no autograd -- TEST INFRASTRUCTURE.

``forward`` / ``backward`` evaluate the edge softmax and its hand-derived gradient in float64 together with the MAGNITUDE of
every output (the same sums over absolute values): a comparison is scaled by the magnitude of its own element.  The same code
run in float32 (``plain_f32``: accurate exp, two-pass softmax with max subtraction, sequential CSR-order sums) is the yardstick
the device tolerances are expressed in; it is not the code under test.  tests/test_gat_ref_cpu.py checks the float64 path
against torch autograd of the dense formulation.

All edge arrays are in in-edge CSR order (edge e of row v: ``indices[indptr[v] + k]`` -> v).  Two feature inputs: ``zg`` the
values the aggregation gathers (z, or its bf16 rounding) and ``zf`` the fp32 z behind el / er and the column sums -- the
device's rounding points.  ``el`` / ``er`` may be given instead (the device's own scores).

The module also builds the inputs the CPU and GPU tests share: the designed graph and the logit regimes (REGIMES).
"""
import functools

import numpy as np

SLOPE = 0.2
DEGREES = (0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 257)
HUB_DEGREE = 3000


# ------------------------------------------------------------------------------------------------ graphs

def csr_from_coo(key, other, n):
    """stable sort of the COO by ``key``: (indptr, indices = other[perm], perm)"""
    key, other = np.asarray(key, dtype=np.int64), np.asarray(other, dtype=np.int64)
    perm = np.argsort(key, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=n), out=indptr[1:])
    return indptr, other[perm], perm


class Graph:
    """in-edge CSR, out-edge CSR and pos_in (position in the in-CSR of the edge at position i of the out-CSR), on the host"""

    def __init__(self, src, dst, n):
        self.src, self.dst, self.n = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), int(n)
        self.indptr, self.indices, pin = csr_from_coo(self.dst, self.src, n)
        self.rindptr, self.rindices, pout = csr_from_coo(self.src, self.dst, n)
        inv = np.empty_like(pin)
        inv[pin] = np.arange(pin.size)
        self.pos_in = inv[pout]
        self.deg = np.diff(self.indptr)
        self.edst = np.repeat(np.arange(n), self.deg)          # destination of every in-CSR edge


def designed_graph(n=333, hub_order="rising", hub_degree=HUB_DEGREE, seed=0):
    """One node per in-degree of DEGREES (nodes 0 .. 20), a hub of in-degree ``hub_degree`` (node 21: sources drawn with
    repetition, none 16 times; sorted ascending by source id for ``rising``, descending for ``first``), node 22 without any
    edge, node 23 never a source, self-loops, duplicated edges; every other node gets 1 .. 12 random in-edges.  Rows of degree
    >= 17 and the hub contain the lowest and the highest source id.  Returns (Graph, info)."""
    assert n >= 190 and hub_order in ("rising", "first")
    rng = np.random.default_rng(seed)
    hub, isolated, sink = len(DEGREES), len(DEGREES) + 1, len(DEGREES) + 2
    sources = np.array([u for u in range(n) if u not in (isolated, sink)])
    blocks = []
    for v, d in enumerate(DEGREES):
        s = rng.choice(sources, d)
        if d >= 2 and v % 2 == 0:
            s[0] = v                                           # self-loop
        if d in (4, 33):
            s[2] = s[1]                                        # the same edge twice
        if d >= 17:
            s[1], s[d // 2] = sources[0], sources[-1]
        blocks.append((v, s))
    # the highest source once only (a last chunk made of its copies alone would not raise the maximum), the others make up for it
    reps = hub_degree // sources.size
    hs = np.concatenate([np.repeat(sources[:-1], reps), sources[-1:],
                         rng.choice(sources[:-1], hub_degree % sources.size + reps - 1, replace=False)])
    assert hub in hs and hs.size == hub_degree and reps + 1 < 16                # hub -> hub is among them
    hs = np.sort(hs)
    blocks.append((hub, hs if hub_order == "rising" else hs[::-1]))
    for v in range(sink, n):
        blocks.append((v, rng.choice(sources, int(rng.integers(1, 13)))))
    blocks = blocks[::-1]                                      # COO not sorted by destination; edge order inside a row kept
    src = np.concatenate([s for _, s in blocks])
    dst = np.concatenate([np.full(s.size, v) for v, s in blocks])
    info = dict(hub=hub, isolated=isolated, sink=sink, degree_node={d: v for v, d in enumerate(DEGREES)})
    return Graph(src, dst, n), info


# regime of the tests -> (inputs, hub ordering, hub in-degree).  The hub has 3 000 in-edges where the float32 yardstick stays within
# 64 * 2^-24 of float64 (tests/test_gat_ref_cpu.py); its SEQUENTIAL float32 sum over 3 000 edges does not where the large terms
# come first or all terms are of one size (108 / 87 / 60 * 2^-24 measured), so those regimes take a hub of 1 000 (63 chunks).
REGIMES = {"normal": ("normal", "rising", 1000), "wide-rising": ("wide", "rising", 3000), "wide-first": ("wide", "first", 1000),
           "flat": ("flat", "rising", 3000), "negative": ("negative", "rising", 1000)}


@functools.lru_cache(maxsize=None)
def regime_graph(n, regime):
    _, order, hub = REGIMES[regime]
    return designed_graph(n, order, hub)


def regime_inputs(n, regime, H, D):
    g, info = regime_graph(n, regime)
    return (g, info) + make_inputs(REGIMES[regime][0], g, info, H, D)


# ------------------------------------------------------------------------------------------------ inputs

def _targeted(rng, n, H, D, t_l, t_r):
    """z, a_l, a_r (float64) with <a_l[h], z[v,h]> = t_l[v,h] and <a_r[h], z[v,h]> = t_r[v,h]: a_l orthogonal to a_r, noise
    orthogonal to both.  D == 1 cannot hold both: a_r = 0.01 a_l there, so er = 0.01 el."""
    a_l = rng.standard_normal((H, D)) / np.sqrt(D)
    a_l[np.abs(a_l) < 0.1] = 0.3
    if D == 1:
        return (t_l / a_l[:, 0])[:, :, None], a_l, 0.01 * a_l
    a_r = rng.standard_normal((H, D))
    a_r -= (a_r * a_l).sum(1, keepdims=True) / (a_l * a_l).sum(1, keepdims=True) * a_l
    a_r /= np.sqrt((a_r * a_r).sum(1, keepdims=True))
    ul, ur = a_l / (a_l * a_l).sum(1, keepdims=True), a_r / (a_r * a_r).sum(1, keepdims=True)
    noise = rng.standard_normal((n, H, D)) if D >= 3 else np.zeros((n, H, D))
    noise -= (noise * a_l).sum(-1, keepdims=True) * ul + (noise * a_r).sum(-1, keepdims=True) * ur
    return noise + t_l[:, :, None] * ul + t_r[:, :, None] * ur, a_l, a_r


def make_inputs(regime, graph, info, H, D, seed=0):
    """float32 (z [n, H*D], a_l [H*D], a_r [H*D], bias [H*D]) of one logit regime:
    normal    z ~ N(0,1), a ~ N(0,1)/sqrt(D)
    wide      el rises with the node id from -63 to 31, |er| <= 0.65: rows holding the lowest and the highest source spread their
              logits over ~44 units (leaky: -12.7 .. 31.6); -64 < el + er < 32, so the float32 roundings of the sum, of its
              product with the slope and of s - smax together stay below 64 * 2^-24
    flat      a_l = a_r = 0
    negative  el in [-6, -0.5], er in [-3, -0.1]; four edges (first source -> node of degree 5, 17, 33, hub) have both rows zeroed"""
    n = graph.n
    rng = np.random.default_rng([seed, H, D, n])
    bias = rng.standard_normal(H * D)
    if regime in ("normal", "flat"):
        z = rng.standard_normal((n, H, D))
        a_l, a_r = rng.standard_normal((H, D)) / np.sqrt(D), rng.standard_normal((H, D)) / np.sqrt(D)
        if regime == "flat":
            a_l, a_r = np.zeros((H, D)), np.zeros((H, D))
    elif regime == "wide":
        t_l = np.linspace(-63.0, 31.0, n)[:, None] + rng.uniform(-0.1, 0.1, (n, H))
        z, a_l, a_r = _targeted(rng, n, H, D, t_l, rng.uniform(-0.5, 0.5, (n, H)))
    elif regime == "negative":
        z, a_l, a_r = _targeted(rng, n, H, D, rng.uniform(-6.0, -0.5, (n, H)), rng.uniform(-3.0, -0.1, (n, H)))
        for v in [info["degree_node"][d] for d in (5, 17, 33)] + [info["hub"]]:
            z[v] = 0.0
            z[graph.indices[graph.indptr[v]]] = 0.0
    else:
        raise ValueError(regime)
    f = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], -1) if a.ndim == 3 else a.reshape(-1), dtype=np.float32)
    return f(z), f(a_l), f(a_r), bias.astype(np.float32)


def bf16_round(a):
    """float32 array rounded to nearest-even bf16, kept as float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------ the evaluator

def _seq_sum(vals, indptr):
    """out[v] = vals[indptr[v]] + vals[indptr[v] + 1] + ... added one after the other in vals' dtype (zero for an empty row)"""
    n = len(indptr) - 1
    out = np.zeros((n,) + vals.shape[1:], dtype=vals.dtype)
    for v in np.nonzero(np.diff(indptr))[0]:
        out[v] = np.add.accumulate(vals[indptr[v]:indptr[v + 1]], axis=0)[-1]
    return out


def _seg_max(vals, indptr):
    out = np.full((len(indptr) - 1,) + vals.shape[1:], -np.inf, dtype=vals.dtype)
    for v in np.nonzero(np.diff(indptr))[0]:
        out[v] = vals[indptr[v]:indptr[v + 1]].max(0)
    return out


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def scores(zf, a_l, a_r, H, dtype=np.float64):
    """el[v,h] = <a_l[h], z[v,h]>, er likewise, and their magnitudes sum |z| |a|"""
    z3 = np.asarray(zf).astype(dtype).reshape(len(zf), H, -1)
    al, ar = (np.asarray(a).astype(dtype).reshape(H, z3.shape[2]) for a in (a_l, a_r))
    return dict(el=(z3 * al).sum(-1), er=(z3 * ar).sum(-1), mag_el=(np.abs(z3) * np.abs(al)).sum(-1),
                mag_er=(np.abs(z3) * np.abs(ar)).sum(-1))


def forward(g, zg, zf, a_l, a_r, bias, H, elu=False, mean_heads=False, mean_bias=None, el=None, er=None, dtype=np.float64):
    """dict: el, er, x (= el[u] + er[v]), s, smax, ssum, alpha, agg, out ([n, H*D], activated when ``elu``), out_mean ([n, D]
    when ``mean_heads``) and the magnitudes mag_el, mag_er, mag_out, mag_mean."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    n = g.n
    zg3, zf3 = c(zg).reshape(n, H, -1), c(zf).reshape(n, H, -1)
    D = zg3.shape[2]
    al, ar = c(a_l).reshape(H, D), c(a_r).reshape(H, D)
    r = dict(H=H, D=D, dtype=dtype)
    sc = scores(zf, a_l, a_r, H, dtype)
    r["mag_el"], r["mag_er"] = sc["mag_el"], sc["mag_er"]
    r["el"] = el = sc["el"] if el is None else c(el)
    r["er"] = er = sc["er"] if er is None else c(er)
    src, dst = g.indices, g.edst
    r["x"] = x = el[src] + er[dst]
    r["s"] = s = np.where(x > 0, x, dtype(SLOPE) * x)
    r["smax"] = smax = _seg_max(s, g.indptr)
    p = np.exp(s - smax[dst])
    r["ssum"] = ssum = _seq_sum(p, g.indptr)
    r["alpha"] = alpha = p / ssum[dst]
    r["agg"] = agg = _seq_sum(alpha[:, :, None] * zg3[src], g.indptr).reshape(n, H * D)
    mag = _seq_sum(alpha[:, :, None] * np.abs(zg3[src]), g.indptr).reshape(n, H * D)
    b = c(bias)
    pre = agg + b if b is not None else agg
    r["mag_out"] = mag + np.abs(b) if b is not None else mag
    r["pre"] = pre
    r["out"] = out = _elu(pre) if elu else pre
    if mean_heads:
        mb = c(mean_bias)
        m = np.add.accumulate(out.reshape(n, H, D), axis=1)[:, -1] / dtype(H)
        mm = r["mag_out"].reshape(n, H, D).sum(1) / H
        r["out_mean"] = m + mb if mb is not None else m
        r["mag_mean"] = mm + np.abs(mb) if mb is not None else mm
    return r


def dout_prepare(dout, act_out, mean_heads, H, D, dtype=np.float64):
    """gat_dout_prepare_kernel: dfull[v, f] = (mean_heads ? dout[v, f % D] / H : dout[v, f]) * (act_out ? ELU' : 1), ELU' from the
    ACTIVATED output: 1 where it is positive, else out + 1"""
    d = np.asarray(dout).astype(dtype)
    full = np.tile(d / dtype(H), (1, H)) if mean_heads else d
    if act_out is not None:
        o = np.asarray(act_out).astype(dtype)
        full = full * np.where(o > 0, dtype(1), o + dtype(1))
    return full


def backward(g, fw, zg, zf, a_l, a_r, dout, act_out=None, mean_heads=False):
    """From a forward dict: dfull, ds [E, H], der, del [n, H], dz [n, H*D], da_l, da_r, dbias [H*D], each with mag_<name>."""
    dtype, H, D, n = fw["dtype"], fw["H"], fw["D"], g.n
    c = lambda a: np.asarray(a).astype(dtype)
    zg3, zf3 = c(zg).reshape(n, H, D), c(zf).reshape(n, H, D)
    al, ar = c(a_l).reshape(H, D), c(a_r).reshape(H, D)
    src, dst, alpha, x = g.indices, g.edst, fw["alpha"], fw["x"]
    r = {}
    r["dfull"] = dfull = dout_prepare(dout, act_out, mean_heads, H, D, dtype)
    df3 = dfull.reshape(n, H, D)
    dalpha = (df3[dst] * zg3[src]).sum(-1)
    m_dalpha = (np.abs(df3[dst]) * np.abs(zg3[src])).sum(-1)
    t = _seq_sum(alpha * dalpha, g.indptr)
    m_t = _seq_sum(alpha * m_dalpha, g.indptr)
    lk = np.where(x > 0, dtype(1), dtype(SLOPE))               # the kernels' s > 0 ? 1 : slope
    r["ds"] = ds = alpha * (dalpha - t[dst]) * lk
    r["mag_ds"] = m_ds = alpha * (m_dalpha + m_t[dst]) * lk
    r["der"], r["mag_der"] = _seq_sum(ds, g.indptr), _seq_sum(m_ds, g.indptr)
    r["del"], r["mag_del"] = _seq_sum(ds[g.pos_in], g.rindptr), _seq_sum(m_ds[g.pos_in], g.rindptr)
    w = alpha[:, :, None] * df3[dst]
    r["dz"] = (_seq_sum(w[g.pos_in], g.rindptr) + r["del"][:, :, None] * al + r["der"][:, :, None] * ar).reshape(n, H * D)
    r["mag_dz"] = (_seq_sum(np.abs(w)[g.pos_in], g.rindptr) + r["mag_del"][:, :, None] * np.abs(al)
                   + r["mag_der"][:, :, None] * np.abs(ar)).reshape(n, H * D)
    col = lambda a: np.add.accumulate(a, axis=0)[-1].reshape(-1)
    r["da_l"], r["mag_da_l"] = col(r["del"][:, :, None] * zf3), col(r["mag_del"][:, :, None] * np.abs(zf3))
    r["da_r"], r["mag_da_r"] = col(r["der"][:, :, None] * zf3), col(r["mag_der"][:, :, None] * np.abs(zf3))
    r["dbias"], r["mag_dbias"] = col(dfull), col(np.abs(dfull))
    return r


def plain_f32(g, zg, zf, a_l, a_r, bias, H, dout=None, act_out=None, elu=False, mean_heads=False, mean_bias=None, el=None,
              er=None, dout_mean_heads=False):
    """the same formulas in float32: (forward dict, backward dict or None)"""
    fw = forward(g, zg, zf, a_l, a_r, bias, H, elu=elu, mean_heads=mean_heads, mean_bias=mean_bias, el=el, er=er, dtype=np.float32)
    bw = None if dout is None else backward(g, fw, zg, zf, a_l, a_r, dout, act_out=act_out, mean_heads=dout_mean_heads)
    return fw, bw


def ratio(got, want, mag):
    """max |got - want| / max(mag, tiny) over the elements"""
    got, want, mag = (np.asarray(a, dtype=np.float64) for a in (got, want, mag))
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    assert np.isfinite(err).all(), "non-finite value"
    return float((err / np.maximum(mag, 1e-30)).max())


def chunk_rises(s_row, chunk=16):
    """per 16-edge chunk of one row's logits: does the running maximum rise in this chunk"""
    out, run = [], -np.inf
    for c0 in range(0, len(s_row), chunk):
        m = s_row[c0:c0 + chunk].max()
        out.append(bool(m > run))
        run = max(run, m)
    return out
