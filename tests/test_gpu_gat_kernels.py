"""The GAT attention kernels (csrc/gat.hip, csrc/gat_rows.h) against the float64 edge-softmax reference of tests/gat_ref.py, one
kernel family at a time: gte_gat_scores, gte_gat_aggregate_fwd_ex with its epilogues, gte_gat_aggregate_bwd_ex with the fused and
the separate dout preparation, the column-sum / fold pair, and the argument checks.  The C entry points are called through ``_lib``
directly so that strides, padding and NULL outputs are the test's.

Inputs (tests/gat_ref.py, checked on the CPU by tests/test_gat_ref_cpu.py): the designed graph -- one row per in-degree 0, 1, ..
17, .. 65, 257, a hub of 3 000 (1 000 where the float32 yardstick needs it) in-edges, self-loops, duplicates, a node without
in-edges, one without out-edges -- in four logit regimes (normal, wide in both hub orderings, flat, negative with logits at 0).

Every dispatch branch is named by the test ids: ``rows-vec1|2|4`` (head per DPP row), ``lane-nj1|2|4|8|16`` (lane per feature),
``fused`` / ``separate`` prepare, ``fp32`` / ``bf16`` gathers.  ``rows0`` cases run the lane-per-feature kernels at row-layout
shapes through the measurement build (libgte_hip_measure.so): the shipped library has no GTE_GAT_ROWS switch.

Tolerance.  For every compared quantity r = max |got - want| / max(mag, tiny) with the element's own magnitude (the same sum over
absolute values).  r_32 is that ratio for gat_ref.plain_f32 (numpy float32: accurate exp, two-pass softmax, sequential sums), which
knows nothing of the kernels; the device must satisfy  r_dev <= 4 r_32 + 16 * 2^-24.  The factor covers summation order, FMA
contraction and the chunked rescaling; the additive term covers __expf, whose error enters as alpha |s - smax| O(2^-24) with
x e^-x <= 0.37.  The aggregation is compared at the device's own el / er (their error is gte_gat_scores' and is checked there).

ssum of long rows.  ssum[v, h] is ONE running float32 sum of deg positive terms, so both r_dev and r_32 are single draws of the
rounding-error walk of recursive summation: each of the deg - 1 additions errs by at most 2^-24 of the partial sum, independent
and of either sign, which gives sqrt(deg) 2^-24 ssum as the scale of the total (Higham, Accuracy and Stability of Numerical
Algorithms, 4.2 and 4.4) and (deg - 1) 2^-24 ssum as its worst case.  A lucky draw of the yardstick says nothing about the
device's: with the plain bound the lane-per-feature forward (one edge at a time) missed at 1 x 1000, normal regime, hub of 1 000:
r_dev = 36.8 * 2^-24 ~ sqrt(1000) 2^-24 while r_32 = 3.1 * 2^-24 (the same plain_f32 gives 20 .. 33 * 2^-24 on the other hubs; the
row-layout kernel, which sums 16 edges pairwise per chunk, stays below 5).  For ssum the magnitude of a row is therefore taken as
ssum * max(1, sqrt(deg) / 8): unchanged up to 64 in-edges, and the additive term of the bound becomes 2 sqrt(deg) 2^-24 beyond.
No other quantity has a modified scale.

Measured on an MI355X: largest r_dev / the r_32 of that case, in units of 2^-24, per quantity and dispatch branch over all 147
cases of the first test (``pytest -s`` prints every case and this table; ssum in its long-row scale):

quantity      rows-vec1    rows-vec2    rows-vec4     lane-nj1     lane-nj2     lane-nj4     lane-nj8    lane-nj16
el              2.5/2.0      2.7/2.5      3.0/4.0      2.5/2.5      2.4/2.3      2.2/2.0      2.1/2.0      1.9/2.0
er              2.1/2.6      2.2/2.2      1.6/1.3      2.2/2.2      1.8/3.0      1.6/1.3      1.2/1.2      1.0/1.2
out           34.4/31.9    35.9/22.7    26.7/41.7    40.1/31.9    34.9/37.1    29.3/38.3    32.7/28.0    29.2/28.8
ssum            2.7/4.2      3.1/3.3      2.6/6.8      8.4/8.4      6.1/6.1      8.8/5.2      6.8/7.3      9.3/2.7
ds            77.2/53.6    47.5/36.9    42.7/28.2    76.4/49.4    66.8/41.9    55.5/32.7    34.6/23.3    19.4/16.1
der             1.9/6.2      1.1/1.3      0.8/0.8      7.8/7.6      3.7/3.5      3.4/3.4      3.0/3.1      0.8/0.8
del           52.9/36.9    37.4/27.0    20.2/17.9    38.0/25.2    25.3/20.2    26.4/21.8    22.1/11.4      8.8/7.3
dz            10.4/10.4     10.5/9.9    10.9/10.9    10.4/10.4     10.6/9.8    10.9/10.9    11.4/11.4    11.9/12.0
da_l            0.2/0.2      0.1/0.1      0.1/0.1      0.2/0.2      0.1/0.2      0.1/0.1      0.1/0.1      0.1/0.1
da_r            0.1/0.0      0.0/0.1      0.0/0.0      0.1/0.1      0.1/0.1      0.0/0.0      0.1/0.1      0.0/0.0
dbias           1.7/1.1      1.1/2.5      1.5/1.5      1.2/1.9      1.9/1.4      1.6/1.6      2.3/1.8      2.5/2.5

epilogues (heads 1, 2, 3 -> vec1; 4x64 -> vec4; 2x17 -> nj1; 8x32 -> nj4)
quantity         rows-vec1    rows-vec4     lane-nj1     lane-nj4
out+elu          12.5/12.2     8.7/11.6    21.5/17.5    18.0/12.9
mean              12.2/8.9      3.1/3.3     14.9/7.0      4.4/4.1
mean+elu          10.7/8.9      2.7/2.3     11.0/4.8      4.4/3.0
mean-nobias      21.5/23.6      6.7/8.1    26.2/19.0      8.5/8.7

Every entry is within 4 r_32 + 16 (ssum with the long-row scale); the closest is ds on lane-nj4 at 0.38 of its bound.
"""
import ctypes
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from tests import gat_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
SENTINEL = 7.5e29                       # padding columns: never to be used as an input, never to be overwritten
BF16_CANARY = 123.0
WORST = {}                              # (quantity, path) -> (r_dev, r_32, case)

Case = namedtuple("Case", "H D regime pad rows_off bf16 n", defaults=("normal", 0, False, False, 333))


def nj_of(hd):
    return 1 if hd <= 64 else 2 if hd <= 128 else 4 if hd <= 256 else 8 if hd <= 512 else 16


def path_of(H, D, ld_gather, ld_dout, rows_off=False):
    """the dispatch of gte_gat_aggregate_fwd_ex / _bwd_ex restated (gat_rows_vec + GTE_NJ_DISPATCH): names the ids only"""
    vec = 0 if (rows_off or H > 4 or D > 64) else (4 if D > 32 else 2 if D > 16 else 1)
    if vec and (D % vec or ld_gather % vec or ld_dout % vec):
        vec = 0
    return f"rows-vec{vec}" if vec else f"lane-nj{nj_of(H * D)}"


def case_id(c):
    ld = c.H * c.D + c.pad
    return (f"{path_of(c.H, c.D, ld, ld, c.rows_off)}-{c.H}x{c.D}" + (f"+ld{c.pad}" if c.pad else "") + ("-rows0" if c.rows_off else "")
            + f"-{'bf16' if c.bf16 else 'fp32'}-{c.regime}-n{c.n}")


ROW_SHAPES = [(1, 1), (1, 16), (2, 16), (3, 7), (4, 16), (4, 18), (4, 32), (4, 36), (4, 64)]
RULE_SHAPES = [(2, 17), (2, 33)]                                   # dim % vec != 0: the lane kernels
LANE_SHAPES = [(5, 13), (8, 8), (8, 32), (3, 100), (4, 128), (8, 64), (8, 128), (1, 1000)]
BF16_SHAPES = [(4, 64), (4, 18), (3, 7), (8, 64)]
CASES = [Case(H, D, r) for H, D in ROW_SHAPES + RULE_SHAPES + LANE_SHAPES for r in R.REGIMES]
CASES += [Case(4, 64, r, pad=p) for p in (3, 4) for r in R.REGIMES]            # ld = H*D + 3: falls back; + 4: keeps vec 4
CASES += [Case(H, D, r, rows_off=True) for H, D in [(4, 64), (4, 16)] for r in R.REGIMES]
CASES += [Case(H, D, r, bf16=True) for H, D in BF16_SHAPES for r in R.REGIMES]
CASES += [Case(H, D, r, n=203) for H, D in [(4, 64), (4, 18), (3, 7), (8, 32), (1, 1000)] for r in ("normal", "wide-rising")]
CASES += [Case(4, 64, "normal", bf16=True, n=203), Case(4, 64, "normal", pad=4, bf16=True)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nquantity / path: largest r_dev (r_32 of that case), in 2^-24")
    for k in sorted(WORST):
        d, y, case = WORST[k]
        print(f"  {k[0]:8s} {k[1]:10s} r_dev {d / EPS:8.2f}   r_32 {y / EPS:8.2f}   bound {(4 * y + 16 * EPS) / EPS:8.2f}   {case}")


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def padded(a, ld, fill=SENTINEL):
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a, torch.float32)
    return buf


def canary(rows, ld, dtype=torch.float32):
    return torch.full((rows, ld), BF16_CANARY if dtype == torch.bfloat16 else SENTINEL, dtype=dtype, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def padding_untouched(buf, cols):
    fill = BF16_CANARY if buf.dtype == torch.bfloat16 else SENTINEL
    return bool((buf[:, cols:] == fill).all())


def np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


_measure = []


def measure_lib():
    """libgte_hip_measure.so (-DGTE_MEASURE): the build in which GTE_GAT_ROWS=0 turns the row-layout kernels off, read on every call"""
    if not _measure:
        path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgte_hip_measure.so")
        assert os.path.exists(path), "the measurement build is missing: make -C gnn-tableextraction_amd/csrc all"
        lib = ctypes.CDLL(path)
        for name, (res, args) in _lib.SIGNATURES.items():
            if name.startswith("gte_gat") or name == "gte_last_error":
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        _measure.append(lib)
    return _measure[0]


_graphs = {}


def device_graph(n, regime):
    """(host Graph, info, device arrays built exactly as _GatAggregate does); the device CSRs must be the host's stable ones"""
    key = (n, regime)
    if key not in _graphs:
        from gnn_tableextraction_amd import graph as G
        g, info = R.regime_graph(n, regime)
        pg = G.PageGraph(g.src, g.dst, n, device=DEV)
        csr, rcsr = pg.in_csr(), pg.out_csr()
        d = dict(indptr=csr.indptr, indices=csr.indices, rindptr=rcsr.indptr, rindices=rcsr.indices, pos_in=pg.out_to_in_pos())
        for k, want in (("indptr", g.indptr), ("indices", g.indices), ("rindptr", g.rindptr), ("rindices", g.rindices),
                        ("pos_in", g.pos_in)):
            assert d[k].dtype == torch.int32 and np.array_equal(d[k].cpu().numpy(), want), k
        _graphs[key] = (g, info, d)
    return _graphs[key]


def ok(rc, what, lib=None):
    if rc != 0:
        msg = (lib or _lib.load()).gte_last_error()
        raise AssertionError(f"{what} returned {rc}: {msg.decode() if msg else ''}")


def scores(lib, z, a_l, a_r, H, D, zb=None):
    n = z.shape[0]
    el, er = canary(n, H), canary(n, H)
    ok(lib.gte_gat_scores(z.data_ptr(), z.stride(0), a_l.data_ptr(), a_r.data_ptr(), el.data_ptr(), er.data_ptr(), _lib.ptr(zb),
                          0 if zb is None else zb.stride(0), n, H, D, _lib.current_stream()), "gte_gat_scores", lib)
    return el, er


def forward(lib, d, zg, el, er, bias, H, D, ldo=None, activation=0, out=True, out_bf16=False, out_mean=False, mean_bias=None,
            ldob=None, ldom=None):
    n, HD = zg.shape[0], H * D
    ldo, ldob, ldom = ldo or HD + 3, ldob or HD + 5, ldom or D + 3
    r = dict(out=canary(n, ldo) if out else None, out_bf16=canary(n, ldob, torch.bfloat16) if out_bf16 else None,
             out_mean=canary(n, ldom) if out_mean else None, smax=canary(n, H), ssum=canary(n, H))
    P = _lib.ptr
    ok(lib.gte_gat_aggregate_fwd_ex(P(d["indptr"]), P(d["indices"]), P(zg), zg.stride(0),
                                    _lib.GTE_BF16 if zg.dtype == torch.bfloat16 else _lib.GTE_F32, P(el), P(er), P(bias), P(r["out"]), ldo,
                                    P(r["smax"]), P(r["ssum"]), n, H, D, activation, P(r["out_bf16"]), ldob, P(r["out_mean"]), ldom,
                                    P(mean_bias), _lib.current_stream()), "gte_gat_aggregate_fwd_ex", lib)
    return r


def backward(lib, d, zg, zf, fw_el, fw_er, smax, ssum, a_l, a_r, dout, H, D, act_out=None, mean_heads=0, dfull=None, grads=True,
             lddz=None, ws_short=0):
    n, HD, E = zf.shape[0], H * D, d["indices"].numel()
    lddz = lddz or HD + 5
    r = dict(ds=canary(max(E, 1), H), der=canary(n, H), **{"del": canary(n, H)}, dz=canary(n, lddz),
             da_l=canary(1, HD) if grads else None, da_r=canary(1, HD) if grads else None, dbias=canary(1, HD) if grads else None)
    nbytes = lib.gte_gat_bwd_workspace_bytes(n, H, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    P = _lib.ptr
    rc = lib.gte_gat_aggregate_bwd_ex(P(d["indptr"]), P(d["indices"]), P(d["rindptr"]), P(d["rindices"]), P(d["pos_in"]), P(zg),
                                      zg.stride(0), _lib.GTE_BF16 if zg.dtype == torch.bfloat16 else _lib.GTE_F32, P(zf), zf.stride(0),
                                      P(fw_el), P(fw_er), P(smax), P(ssum), P(a_l), P(a_r), P(dout), dout.stride(0), P(act_out),
                                      0 if act_out is None else act_out.stride(0), mean_heads, P(dfull),
                                      0 if dfull is None else dfull.stride(0), P(r["ds"]), P(r["der"]), P(r["del"]), P(r["dz"]), lddz,
                                      P(r["da_l"]), P(r["da_r"]), P(r["dbias"]), n, H, D, P(ws), nbytes - ws_short,
                                      _lib.current_stream())
    if ws_short:
        return rc
    ok(rc, "gte_gat_aggregate_bwd_ex", lib)
    return r


class Check:
    """collects the findings of one case so that every figure is printed before the case fails"""

    def __init__(self, case, path):
        self.case, self.path, self.problems, self.line = case, path, [], []

    def that(self, cond, what):
        if not cond:
            self.problems.append(what)

    def close(self, name, got, want, mag, got32):
        """r_dev <= 4 r_32 + 16 * 2^-24 (module docstring)"""
        try:
            r_dev, r_32 = R.ratio(got, want, mag), R.ratio(got32, want, mag)
        except AssertionError:
            self.problems.append(f"{name}: non-finite")
            return
        self.line.append(f"{name} {r_dev / EPS:.2f}/{r_32 / EPS:.2f}")
        if r_dev >= WORST.get((name, self.path), (-1.0,))[0]:
            WORST[(name, self.path)] = (r_dev, r_32, self.case)
        if not r_dev <= 4 * r_32 + 16 * EPS:
            self.problems.append(f"{name}: r_dev {r_dev / EPS:.2f} > 4 * r_32 ({r_32 / EPS:.2f}) + 16   [2^-24]")

    def done(self):
        print(f"\n{self.case}: r_dev/r_32 [2^-24]  " + "  ".join(self.line), end="")
        assert not self.problems, f"{self.case}: " + "; ".join(self.problems)


def leaky32(el, er, g):
    """the kernels' logit in float32, exactly: one rounded add, one rounded product with 0.2f"""
    x = el.astype(np.float32)[g.indices] + er.astype(np.float32)[g.edst]
    return x, np.where(x > 0, x, np.float32(R.SLOPE) * x)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scores_forward_and_backward_match_float64(case, monkeypatch):
    H, D, HD, n = case.H, case.D, case.H * case.D, case.n
    ld = HD + case.pad
    g, info, d = device_graph(n, case.regime)
    _, _, zf_h, a_l_h, a_r_h, bias_h = R.regime_inputs(n, case.regime, H, D)
    lib = _lib.load()
    if case.rows_off:
        lib = measure_lib()
        monkeypatch.setenv("GTE_GAT_ROWS", "0")
    ck = Check(case_id(case), path_of(H, D, ld, ld, case.rows_off))
    has_in = g.deg > 0
    deg0 = torch.as_tensor(np.nonzero(g.deg == 0)[0], device=DEV)

    # ---- gte_gat_scores: el, er, the bf16 copy
    zf, a_l, a_r, bias = padded(zf_h, ld), dev(a_l_h), dev(a_r_h), dev(bias_h)
    ldzb = ld if case.bf16 else HD + 3
    zb = canary(n, ldzb, torch.bfloat16)
    el, er = scores(lib, zf, a_l, a_r, H, D, zb)
    free, free32 = R.scores(zf_h, a_l_h, a_r_h, H), R.scores(zf_h, a_l_h, a_r_h, H, np.float32)
    ck.close("el", np64(el), free["el"], free["mag_el"], free32["el"])
    ck.close("er", np64(er), free["er"], free["mag_er"], free32["er"])
    ck.that(same_bits(zb[:, :HD], zf[:, :HD].to(torch.bfloat16)), "z_bf16 is not the bf16 rounding of z")
    ck.that(padding_untouched(zb, HD), "z_bf16 padding written")
    el2, er2 = scores(lib, zf, a_l, a_r, H, D, None)                               # without the copy: the same scores
    ck.that(same_bits(el, el2) and same_bits(er, er2), "scores differ without z_bf16")

    # ---- forward at the device's own scores
    zg = zb if case.bf16 else zf
    zg_h = zb[:, :HD].float().cpu().numpy() if case.bf16 else zf_h
    el_h, er_h = el.cpu().numpy(), er.cpu().numpy()
    f1 = forward(lib, d, zg, el, er, bias, H, D)
    f2 = forward(lib, d, zg, el, er, bias, H, D)
    fw = R.forward(g, zg_h, zf_h, a_l_h, a_r_h, bias_h, H, el=el_h, er=er_h)
    ck.that(all(same_bits(f1[k], f2[k]) for k in ("out", "smax", "ssum")), "two forward launches differ")
    ck.that(padding_untouched(f1["out"], HD), "out padding written")
    out = f1["out"][:, :HD]
    smax, ssum = f1["smax"].cpu().numpy(), f1["ssum"].cpu().numpy()
    ck.that(same_bits(out[deg0], bias.expand(len(deg0), HD)), "a row without in-edges is not the bias")
    _, s32 = leaky32(el_h, er_h, g)
    want_max = np.stack([s32[g.indptr[v]:g.indptr[v + 1]].max(0) if has_in[v] else smax[v] for v in range(n)])
    ck.that(np.array_equal(smax.view(np.int32), want_max.astype(np.float32).view(np.int32)), "smax is not the largest float32 logit")
    p64 = np.exp(s32.astype(np.float64) - smax.astype(np.float64)[g.edst])         # sum exp(s - smax) at the DEVICE's smax
    want_sum = R._seq_sum(p64, g.indptr)
    rng = np.random.default_rng([H, D, n])
    dout_h = rng.standard_normal((n, HD)).astype(np.float32)
    fw32, bw32 = R.plain_f32(g, zg_h, zf_h, a_l_h, a_r_h, bias_h, H, dout=dout_h, el=el_h, er=er_h)
    ck.close("out", np64(out), fw["out"], fw["mag_out"], fw32["out"])
    # plain_f32 forms the same float32 logits and the same maximum, so its ssum is the float32 evaluation of want_sum.
    # Rows of more than 64 in-edges: the scale grows as sqrt(deg) / 8 (module docstring, "ssum of long rows")
    long_row = np.maximum(1.0, np.sqrt(g.deg[has_in, None]) / 8)
    ck.close("ssum", ssum[has_in], want_sum[has_in], want_sum[has_in] * long_row, fw32["ssum"][has_in])
    if case.regime == "flat":                                                      # alpha = 1 / deg: the sums are exact
        ck.that(np.array_equal(ssum[has_in], np.repeat(g.deg[has_in, None], H, 1).astype(np.float32)), "flat: ssum != deg")
        ck.that(not smax[has_in].view(np.int32).any(), "flat: smax != +0")

    # ---- backward from the device's own forward outputs
    dout = padded(dout_h, ld)
    args = (lib, d, zg, zf, el, er, f1["smax"], f1["ssum"], a_l, a_r, dout, H, D)
    b1, b2 = backward(*args), backward(*args)
    b3 = backward(*args, grads=False)                                              # da_l, da_r, dbias accept NULL
    keys = ("ds", "der", "del", "dz", "da_l", "da_r", "dbias")
    ck.that(all(same_bits(b1[k], b2[k]) for k in keys), "two backward launches differ")
    ck.that(all(same_bits(b1[k], b3[k]) for k in keys[:4]), "backward differs without da_l / da_r / dbias")
    ck.that(padding_untouched(b1["dz"], HD), "dz padding written")
    bw = R.backward(g, fw, zg_h, zf_h, a_l_h, a_r_h, dout_h)
    E = g.indices.size
    got = {k: np64(b1[k]) for k in keys}
    got["ds"], got["dz"] = got["ds"][:E], got["dz"][:, :HD]
    for k in keys:
        ck.close(k, got[k].reshape(bw[k].shape), bw[k], bw["mag_" + k], bw32[k])
    ck.that(not got["der"][g.deg == 0].any(), "der of a row without in-edges is not 0")
    ck.that(not got["del"][[info["sink"], info["isolated"]]].any(), "del of a node without out-edges is not 0")
    if case.regime == "negative":                                                  # logits AT zero take the slope
        x32, _ = leaky32(el_h, er_h, g)
        ck.that((x32 <= 0).all() and (x32 == 0).sum() >= 4 * H, "negative regime: the device's scores are not <= 0 with zeros")
    ck.done()


EPILOGUE_SHAPES = [(4, 64), (3, 7), (8, 32), (2, 17), (1, 16), (2, 16)]


@pytest.mark.parametrize("H,D", EPILOGUE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("regime", ["normal", "negative"])
def test_forward_epilogues(H, D, regime):
    """ELU, the bf16 copy, the head mean with and without its bias, out == NULL; rows-vec4 / vec1 (idle DPP rows at 1, 2 and 3
    heads) and lane kernels."""
    HD, n = H * D, 333
    g, info, d = device_graph(n, regime)
    _, _, zf_h, a_l_h, a_r_h, bias_h = R.regime_inputs(n, regime, H, D)
    mb_h = np.random.default_rng(3).standard_normal(D).astype(np.float32)
    lib = _lib.load()
    ck = Check(f"epilogue-{path_of(H, D, HD, HD)}-{H}x{D}-{regime}", "epi-" + path_of(H, D, HD, HD))
    zf, a_l, a_r, bias, mb = dev(zf_h), dev(a_l_h), dev(a_r_h), dev(bias_h), dev(mb_h)
    el, er = scores(lib, zf, a_l, a_r, H, D)
    el_h, er_h = el.cpu().numpy(), er.cpu().numpy()
    plain = forward(lib, d, zf, el, er, bias, H, D)
    full = forward(lib, d, zf, el, er, bias, H, D, activation=1, out_bf16=True, out_mean=True, mean_bias=mb)
    for k in ("out", "out_bf16", "out_mean"):
        ck.that(padding_untouched(full[k], D if k == "out_mean" else HD), f"{k} padding written")
        ck.that(bool(torch.isfinite(full[k][:, :D if k == "out_mean" else HD].float()).all()), f"{k} is not finite")
    out0, out1 = plain["out"][:, :HD], full["out"][:, :HD]
    # ELU of the plain launch's output: expm1 within 3 ulp (the OpenCL bound for expm1) + 1 for the reference's rounding to float32
    want = R._elu(np64(out0))
    err = np.abs(np64(out1) - want)
    ck.that(bool((err <= 4 * 2.0 ** -23 * np.abs(want) + 1e-37).all()), f"ELU: {float((err / np.maximum(np.abs(want), 1e-37)).max() / 2.0 ** -23):.2f} ulp")
    deg0 = torch.as_tensor(np.nonzero(g.deg == 0)[0], device=DEV)
    eb = R._elu(bias_h.astype(np.float64))
    ck.that(bool((np.abs(np64(out1[deg0]) - eb) <= 4 * 2.0 ** -23 * np.abs(eb)).all()), "a row without in-edges is not ELU(bias)")
    ck.that(same_bits(out0[deg0], bias.expand(len(deg0), HD)), "a row without in-edges is not the bias")
    ck.that(same_bits(full["out_bf16"][:, :HD], out1.to(torch.bfloat16)), "out_bf16 is not the bf16 rounding of out")
    kw = dict(el=el_h, er=er_h)
    for elu, name in ((True, "mean+elu"), (False, "mean")):
        r = full if elu else forward(lib, d, zf, el, er, bias, H, D, out_mean=True, mean_bias=mb)
        fw = R.forward(g, zf_h, zf_h, a_l_h, a_r_h, bias_h, H, elu=elu, mean_heads=True, mean_bias=mb_h, **kw)
        fw32 = R.forward(g, zf_h, zf_h, a_l_h, a_r_h, bias_h, H, elu=elu, mean_heads=True, mean_bias=mb_h, dtype=np.float32, **kw)
        ck.close(name, np64(r["out_mean"][:, :D]), fw["out_mean"], fw["mag_mean"], fw32["out_mean"])
        if elu:
            ck.close("out+elu", np64(out1), fw["out"], fw["mag_out"], fw32["out"])
        only = forward(lib, d, zf, el, er, bias, H, D, activation=int(elu), out=False, out_mean=True, mean_bias=mb)
        ck.that(same_bits(only["out_mean"], r["out_mean"]), f"{name}: out_mean differs when out is NULL")
        ck.that(same_bits(only["smax"], plain["smax"]) and same_bits(only["ssum"], plain["ssum"]), f"{name}: smax / ssum differ")
    nb = forward(lib, d, zf, el, er, None, H, D, out_mean=True, mean_bias=None)       # neither bias
    fw = R.forward(g, zf_h, zf_h, a_l_h, a_r_h, None, H, mean_heads=True, **kw)
    fw32 = R.forward(g, zf_h, zf_h, a_l_h, a_r_h, None, H, mean_heads=True, dtype=np.float32, **kw)
    ck.close("mean-nobias", np64(nb["out_mean"][:, :D]), fw["out_mean"], fw["mag_mean"], fw32["out_mean"])
    ck.that(not nb["out"][deg0, :HD].view(torch.int32).any() and not nb["out_mean"][deg0, :D].view(torch.int32).any(),
            "without bias a row without in-edges is not +0")
    ck.done()


# (H, D, pad of dout_in / act_out / dfull strides, bf16): pad 0 and 4 fuse in the row-layout kernels, pad 3 forces the separate
# launch at vec 2 and 4 (vec 1 always fuses); the lane kernels always prepare separately
PREPARE = [(4, 64, 0, False), (4, 64, 4, False), (4, 64, 3, False), (4, 64, 0, True), (4, 18, 0, False), (4, 18, 3, False),
           (3, 7, 0, False), (3, 7, 3, True), (1, 16, 0, False), (8, 32, 0, False), (2, 17, 0, False), (8, 64, 0, True)]


def prepare_id(p):
    H, D, pad, bf16 = p
    HD = H * D
    vec = path_of(H, D, HD, HD)                                        # gathers and dfull at ld = H*D
    fused = vec.startswith("rows") and (pad % int(vec[-1]) == 0)
    return f"{'fused' if fused else 'separate'}-{vec}-{H}x{D}+ld{pad}-{'bf16' if bf16 else 'fp32'}"


@pytest.mark.parametrize("p", PREPARE, ids=prepare_id)
@pytest.mark.parametrize("mode", ["elu", "mean", "elu+mean"])
def test_fused_dout_prepare_is_the_separate_prepare_bit_for_bit(p, mode):
    """gte_gat_aggregate_bwd_ex(dfull, act_out, mean_heads) against gte_gat_dout_prepare + gte_gat_aggregate_bwd: dfull and all
    seven outputs bitwise ("gat_dout_prepare_kernel's arithmetic"); and dfull against the float64 formula."""
    H, D, pad, bf16 = p
    HD, n = H * D, 203
    g, info, d = device_graph(n, "normal")
    _, _, zf_h, a_l_h, a_r_h, bias_h = R.regime_inputs(n, "normal", H, D)
    lib = _lib.load()
    zf, a_l, a_r, bias = dev(zf_h), dev(a_l_h), dev(a_r_h), dev(bias_h)
    zb = canary(n, HD, torch.bfloat16) if bf16 else None
    el, er = scores(lib, zf, a_l, a_r, H, D, zb)
    zg = zb if bf16 else zf
    elu, mean = "elu" in mode, "mean" in mode
    f = forward(lib, d, zg, el, er, bias, H, D, ldo=HD + pad, activation=int(elu))
    act = f["out"] if elu else None                                    # the activated output, stride H*D + pad
    cols = D if mean else HD
    dout_h = np.random.default_rng([H, D, pad]).standard_normal((n, cols)).astype(np.float32)
    dout = padded(dout_h, cols + pad)
    dfa, dfb = canary(n, HD + (pad if pad != 3 else 0)), canary(n, HD + (pad if pad != 3 else 0))
    args = (lib, d, zg, zf, el, er, f["smax"], f["ssum"], a_l, a_r)
    a = backward(*args, dout, H, D, act_out=act, mean_heads=int(mean), dfull=dfa)
    ok(lib.gte_gat_dout_prepare(dout.data_ptr(), dout.stride(0), _lib.ptr(act), 0 if act is None else act.stride(0), dfb.data_ptr(),
                                dfb.stride(0), n, H, D, int(mean), _lib.current_stream()), "gte_gat_dout_prepare")
    b = backward(*args, dfb, H, D)
    assert same_bits(dfa, dfb), "dfull differs (padding included)"
    want = R.dout_prepare(dout_h, None if act is None else act[:, :HD].cpu().numpy(), mean, H, D)
    got = np64(dfa[:, :HD])
    assert (np.abs(got - want) <= 4 * EPS * np.abs(want) + 1e-37).all()      # a division, o + 1 and a product: three roundings
    for k in ("ds", "der", "del", "dz", "da_l", "da_r", "dbias"):
        assert same_bits(a[k], b[k]), f"{k} differs between the fused and the separate preparation"


def test_argument_checks_return_their_codes_without_a_launch():
    """every buffer is large enough for the call even if a check were missing"""
    lib, P, st = _lib.load(), _lib.ptr, _lib.current_stream()
    INVALID, SHORT = -1, -3
    n = 4
    f = torch.zeros(n * 2048, dtype=torch.float32, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, q = f.data_ptr(), i.data_ptr()

    def fwd(H=4, D=8, ldo=None, act=0, ob=0, ldob=None, om=0, ldom=None, n=n, out=p):
        return lib.gte_gat_aggregate_fwd_ex(q, q, p, H * D, 0, p, p, p, out, H * D if ldo is None else ldo, p, p, n, H, D, act, ob,
                                            H * D if ldob is None else ldob, om, D if ldom is None else ldom, 0, st)

    def bwd(H=4, D=8, dfull=0, lddf=None, short=0, n=n):
        nb = lib.gte_gat_bwd_workspace_bytes(n, H, D)
        return lib.gte_gat_aggregate_bwd_ex(q, q, q, q, q, p, H * D, 0, p, H * D, p, p, p, p, p, p, p, H * D, 0, 0, 0, dfull,
                                            H * D if lddf is None else lddf, p, p, p, p, H * D, p, p, p, n, H, D, p, nb - short, st)

    torch.cuda.synchronize()
    assert fwd() == 0 and bwd() == 0                                   # the valid calls these are variations of (an edgeless graph)
    assert fwd(H=9) == INVALID and bwd(H=9) == INVALID
    assert fwd(H=1, D=1025) == INVALID and fwd(H=5, D=205) == INVALID and bwd(H=5, D=205) == INVALID
    assert fwd(H=0) == INVALID and fwd(D=0) == INVALID and fwd(n=-1) == INVALID
    assert lib.gte_gat_scores(p, 72, p, p, p, p, 0, 0, n, 9, 8, st) == INVALID
    assert lib.gte_gat_dout_prepare(p, 1025, 0, 0, p, 1025, n, 1, 1025, 0, st) == INVALID
    assert fwd(ldo=31) == INVALID and fwd(om=p, ldom=7) == INVALID and fwd(ob=p, ldob=31) == INVALID
    assert fwd(out=0) == INVALID                                       # neither out nor out_mean
    assert fwd(act=2) == INVALID and fwd(act=-1) == INVALID
    assert bwd(dfull=p, lddf=31) == INVALID
    assert bwd(short=1) == SHORT
    assert fwd(n=0) == 0 and bwd(n=0) == 0 and lib.gte_gat_scores(p, 32, p, p, p, p, 0, 0, 0, 4, 8, st) == 0
    assert fwd(n=0, out=0) == 0                                        # nothing is looked at for an empty graph
    torch.cuda.synchronize()


def test_gat_layer_refuses_elu_on_the_head_mean():
    """GAT never asks for it (ELU is fused into hidden layers only, the mean into the last), GATLayer.forward could: the backward
    would read the [n, D] head mean as the [n, H*D] activated output."""
    import gnn_tableextraction_amd as gte
    from gnn_tableextraction_amd import graph as G
    from gnn_tableextraction_amd.components.graphs.gat import GATLayer
    g, info = R.regime_graph(203, "normal")
    pg = G.PageGraph(g.src, g.dst, g.n, device=DEV)
    layer = GATLayer(6, 5, 3, mean_heads=True).to(DEV)
    x = torch.randn(g.n, 6, device=DEV)
    with pytest.raises(ValueError, match="mean over the heads"):
        layer(pg, x, fuse_elu=True)
    out, _ = layer(pg, x)                                              # and the supported form still runs
    assert out.shape == (g.n, 5) and bool(torch.isfinite(out).all())
    assert gte.GAT(6, 5, 4, n_layers=1, heads=3).to(DEV)(pg, x).shape == (g.n, 4)
