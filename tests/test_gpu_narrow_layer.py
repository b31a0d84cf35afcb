"""The output-layer kernels (csrc/narrow_layer.hip) through the C ABI against the float64 reference of tests/narrow_ref.py at every
instantiation of their dispatch: gte_sage_narrow_fwd, _fwd_pad, _fwd_ln, gte_sage_narrow_bwd (dh given and NULL), _bwd_ce,
_bwd_ln_p3 and _bwd_ln_p3_pad (ce_partial NULL and given, dzp3 NULL and given).  Run with ``-m gpu`` on an MI355X; ``-s`` prints the
worst error / bound ratio per entry point when the module finishes.

EXACT cases (integer h, W, bias, dl, q; alpha a power of two) are held bit for bit to the float64 reference, BOUND cases ('scales',
'cancel', 'gauss') to the rounding bounds derived in tests/narrow_ref.py and checked by tests/test_narrow_ref_cpu.py against a
float32 emulation of every kernel family and six mutants of it.

HARNESS.  Every input is a view with leading dimension width + 3 that starts one element into its allocation, NaN in the padding
columns and in one extra row behind row n - 1 (for W: behind class C - 1); the padded-row entry points get zeros up to n_pad, as
their contract says, and NaN beyond.  Every output is a view into a sentinel-filled buffer: the sentinel must survive outside the
view and no NaN may appear inside.  Workspaces are exactly *_workspace_bytes long between two guards.

WHICH CASE LAUNCHES WHICH INSTANTIATION (test ids name f, n_pad and c; NCT = 4 / 8 / 12 / 16 for c <= 4 / 8 / 12 / 16):
    narrow_fwd_kernel<NJ, NCT>, narrow_bwd_kernel<NJ, NCT>     test_every_class_group_at_every_width[fma-f-c]: NJ = 1 f 1, 13, 63;
                                                               NJ = 2 f 65, 100, 127; NJ = 4 f 129, 250, 255; c over the group edges
                                                               (all of 1 .. 16 at f = 13)
    narrow_fwd_mfma_kernel<false> / <true>                     ...[mfma-f-c], f 8, 24, 40, 56, 72, 120, 136, 200, 248 (fwd / fwd_ln)
    narrow_fwd_mfma16_kernel<false> / <true>                   ...[mfma-f-c], f 16, 32, 48, 64, 128, 192, 256; padded rows: every
                                                               test_padded_rows id (n_pad % 16 == 0)
    narrow_bwd_mfma_kernel<NCT, 0>, <NCT, 2>                   ...[mfma-f-c]: bwd, bwd_ce / bwd_ln_p3; all of 1 .. 16 at f = 24, 48, 64
    narrow_bwd_mfma_kernel<NCTM, 2, true>                      test_padded_rows[f-n_pad-c]: NCTM = 4 c 1, 4; 8 c 5, 8; 16 c 9, 12
                                                               (the 9 .. 12 -> 16 remap), 13, 16; all of 1 .. 16 at (100, 112)
    the grid-stride loops                                      test_grid_stride_loops[...]

CONTRACT OF THE PADDED BACKWARD, pinned here: dz_below is written in whole 16-byte chunks of the true width -- columns n_feat ..
the next multiple of 4 as zeros -- and the columns beyond are the caller's (the one-call plan zero-initialises the buffer once); the
image is written as zeros in all of its padding.

gte_sage_narrow_fwd_ln has no exact case (its input to the products is a LayerNorm output): t_self / t_neigh are held to the bound
against the reference applied to the y the device wrote; y and the statistics are tests/test_gpu_layernorm.py's business and are
held here to gte_ln_relu_fwd at the tolerance test_gpu_parity.py states (neither suite demands bits of them).  dz of the fused
LayerNorm backward is bit for bit gte_sage_narrow_bwd + gte_ln_relu_bwd_p3 where test_gpu_parity.py demands bits (F % 16 == 0,
F >= 128) and inside that suite's tolerance elsewhere; on padded rows the partner forms dh with another kernel, so the 'scales' and
'cancel' kinds add what narrow_ref's dh bound lets through the (linear) LayerNorm backward -- ln_propagated().

MEASURED on an MI355X (256 compute units; all 399 cases: 12.6 s of pytest, 15 s with the interpreter's start), largest error / bound
ratio of the bound cases per entry point:
    gte_sage_narrow_fwd 0.580   _fwd_pad 0.353   _fwd_ln 0.402   gte_sage_narrow_bwd 0.480   _bwd_ce 0.651
    _bwd_ln_p3 0.405 (ce_partial given 0.584, inside a fold deferral 0.019)   _bwd_ln_p3_pad 0.408 (ce_partial given 0.556)
Every exact case of every entry point was bit for bit the float64 reference from the first run, the six grid-stride cases
included; no NaN was read from behind a cut, no sentinel was overwritten, every non-finite row stayed in its row and its columns,
every refused call returned its code and wrote nothing.  Nothing failed, nothing changed in csrc/narrow_layer.hip but two comments;
include/gte.h said of the padded backward that it "writes zeros into the padding of dz_below", which the kernel does only up to the
next multiple of 4: the sentence now says what the kernel guarantees (the one-call plan zero-initialises that buffer once and
nothing else writes it), and run_bwd_ln() pins it with the sentinel.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import narrow_ref as nr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, cs = _lib.ptr, _lib.current_stream
NAN = float("nan")
SENTINEL = 1232.5                      # finite, so that a kernel's own NaN stands out; only what lies OUTSIDE an output is compared with it
EPS_LN = 1e-5
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\n{cus()} compute units; worst error / bound per entry point: " + "   ".join(f"{k} {WORST[k]:.3f}" for k in sorted(WORST)))


def lib():
    return _lib.load()


def check(rc, what):
    _lib.check(rc, what)


@functools.lru_cache(maxsize=None)
def cus():
    n, wave, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    name = ctypes.create_string_buffer(64)
    assert lib().gte_device_info(ctypes.byref(n), ctypes.byref(wave), ctypes.byref(lds), name, 64) == 0
    return n.value


def c16(x):
    return -(-x // 16) * 16


def c4(x):
    return -(-x // 4) * 4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


# ---- the harness every call shares -----------------------------------------------------------------------------------------------------
def guard(a):
    """a [n, w] -> a device view [n, w] with row stride w + 3, one element into its allocation; NaN in the padding columns, in the
    extra row behind row n - 1 and around the whole"""
    a = np.asarray(a, dtype=np.float32)
    n, w = a.shape
    ld = w + 3
    flat = torch.full((1 + (n + 1) * ld + 5,), NAN, dtype=torch.float32, device=DEV)
    v = flat[1:1 + (n + 1) * ld].view(n + 1, ld)
    v[:n, :w] = dev(a)
    return v[:n, :w]


def gvec(a):
    """a [m] -> a device view one element into a NaN-filled allocation"""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    flat = torch.full((a.size + 6,), NAN, dtype=torch.float32, device=DEV)
    flat[1:1 + a.size] = dev(a)
    return flat[1:1 + a.size]


def out2(n, w):
    ld = w + 3
    flat = torch.full((1 + n * ld + 5,), SENTINEL, dtype=torch.float32, device=DEV)
    return flat, flat[1:1 + n * ld].view(n, ld)[:, :w]


def out1(m):
    flat = torch.full((m + 6,), SENTINEL, dtype=torch.float32, device=DEV)
    return flat, flat[1:1 + m]


def done(flat, v, allow_nonfinite=False, untouched=False):
    """the view as numpy, after checking that nothing outside it was written and that no NaN appeared inside"""
    inside = torch.zeros_like(flat, dtype=torch.bool)
    if v.dim() == 2:
        n, w = v.shape
        inside[1:1 + n * v.stride(0)].view(n, v.stride(0))[:, :w] = True
    else:
        inside[1:1 + v.numel()] = True
    assert bool((flat[~inside] == SENTINEL).all()), "written outside the output view"
    if untouched:
        assert bool((flat[inside] == SENTINEL).all()), "an output that was not asked for was written"
        return None
    got = v.cpu().numpy().copy()
    assert allow_nonfinite or np.isfinite(got).all(), "a NaN / Inf reached the output"
    return got


def ld(v):
    return v.stride(0)


class Workspace:
    """exactly ``nbytes`` (``t``) between two guards of one allocation"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.all = torch.full((256 + self.n + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.all[256:256 + self.n]

    def ok(self):
        assert bool((self.all[:256] == 0xA5).all()) and bool((self.all[256 + self.n:] == 0xA5).all()), "written outside the workspace"


def note(entry, r, what):
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, f"{entry} {what}: error / bound = {r:.3f}"


def held(entry, case, what, got, ref, bnd):
    """an exact case bit for bit, a bound case inside its bound"""
    if case.exact:
        want = nr.exact32(ref)
        assert nr.same_bits(got, want), f"{entry} {what}: exact case differs in {int((nr.bits(got) != nr.bits(want)).sum())} elements"
    else:
        note(entry, nr.ratio(got, ref, bnd), what)


# ---- runners ---------------------------------------------------------------------------------------------------------------------------
def run_fwd(h, W, bias, f, n_pad=None, allow_nonfinite=False):
    """gte_sage_narrow_fwd / _fwd_pad (h then has n_pad columns, zeros behind f)"""
    n, c = h.shape[0], W.shape[0]
    hv, Wv, bv = guard(h), guard(W), gvec(bias)
    fs, ts = out2(n, c)
    fn, tn = out2(n, c)
    if n_pad is None:
        check(lib().gte_sage_narrow_fwd(P(hv), ld(hv), f, P(Wv), ld(Wv), P(bv), c, P(ts), ld(ts), P(tn), ld(tn), n, cs()), "fwd")
    else:
        check(lib().gte_sage_narrow_fwd_pad(P(hv), ld(hv), f, n_pad, P(Wv), ld(Wv), P(bv), c, P(ts), ld(ts), P(tn), ld(tn), n, cs()),
              "fwd_pad")
    return done(fs, ts, allow_nonfinite), done(fn, tn, allow_nonfinite)


def run_fwd_ln(z, gamma, beta, relu, W, bias):
    n, f = z.shape
    c = W.shape[0]
    zv, Wv, bv, gv, bev = guard(z), guard(W), gvec(bias), gvec(gamma), gvec(beta)
    fs, ts = out2(n, c)
    fn, tn = out2(n, c)
    fy, y = out2(n, f)
    fst, st = out1(2 * n)
    check(lib().gte_sage_narrow_fwd_ln(P(zv), ld(zv), f, P(gv), P(bev), EPS_LN, int(relu), P(y), ld(y), P(st), P(Wv), ld(Wv), P(bv), c,
                                       P(ts), ld(ts), P(tn), ld(tn), n, cs()), "fwd_ln")
    return done(fy, y), done(fst, st), done(fs, ts), done(fn, tn)


def run_bwd(dl, q, h, W, f, want_dh=True, ce=None, allow_nonfinite=False):
    """gte_sage_narrow_bwd / _bwd_ce (ce = (partials, grad_scale)) -> dh (None when not asked for), dW, dbias, out3"""
    n, c = dl.shape
    dlv, qv, hv, Wv = guard(dl), guard(q), guard(h), guard(W)
    fh, dh = out2(n, f)
    fw, dW = out2(c, 2 * f)
    fb, db = out1(c)
    ws = Workspace(lib().gte_sage_narrow_bwd_workspace_bytes(n, f, c))
    dhp = P(dh) if want_dh else None
    o3 = None
    if ce is None:
        check(lib().gte_sage_narrow_bwd(P(dlv), ld(dlv), P(qv), ld(qv), P(hv), ld(hv), f, P(Wv), ld(Wv), c, dhp, ld(dh), P(dW), ld(dW),
                                        P(db), n, P(ws.t), ws.n, cs()), "bwd")
    else:
        pv = gvec(ce[0])
        fo, o3v = out1(3)
        check(lib().gte_sage_narrow_bwd_ce(P(dlv), ld(dlv), P(qv), ld(qv), P(hv), ld(hv), f, P(Wv), ld(Wv), c, dhp, ld(dh), P(dW), ld(dW),
                                           P(db), n, P(ws.t), ws.n, P(pv), float(ce[1]), P(o3v), cs()), "bwd_ce")
        o3 = done(fo, o3v)
    ws.ok()
    return done(fh, dh, allow_nonfinite, untouched=not want_dh), done(fw, dW, allow_nonfinite), done(fb, db), o3


class LnInputs:
    """z of the layer below [n, width] (zeros behind f on padded rows), its statistics, gamma, beta"""

    def __init__(self, n, f, width, seed):
        rng = np.random.default_rng([23, n, f, seed])
        self.z = np.zeros((n, width), dtype=np.float32)
        self.z[:, :f] = (rng.standard_normal((n, f)) * 1.5 + 0.3).astype(np.float32)
        zt = self.z[:, :f].astype(np.float64)
        self.stats = np.concatenate([zt.mean(1), 1.0 / np.sqrt(zt.var(1) + EPS_LN)]).astype(np.float32)
        self.gamma = (1 + 0.1 * rng.standard_normal(f)).astype(np.float32)
        self.beta = (0.1 * rng.standard_normal(f)).astype(np.float32)


def run_bwd_ln(dl, q, h, W, f, lnin, relu, n_pad=None, ce=None, image=True, defer=False, allow_nonfinite=False):
    """gte_sage_narrow_bwd_ln_p3 / _pad -> dict(dz [n, width] the whole view, img [n, c16(width)] or None, dW, db, dg, dbe, dbi, out3)"""
    n, c = dl.shape
    width = n_pad or f
    dlv, qv, hv, Wv, zv = guard(dl), guard(q), guard(h), guard(W), guard(lnin.z)
    stv, gv, bev = gvec(lnin.stats), gvec(lnin.gamma), gvec(lnin.beta)
    fz, dz = out2(n, width)
    fw, dW = out2(c, 2 * f)
    fb, db = out1(c)
    fg, dg = out1(f)
    fe, dbe = out1(f)
    fi, dbi = out1(f)
    img = None
    if image:
        img = ops.P3.empty(n, width, DEV, rows_cap=n + 1)
        img.data.fill_(0x55)
    ws = Workspace(lib().gte_sage_narrow_bwd_workspace_bytes(n, width, c))
    wl = Workspace(lib().gte_sage_narrow_bwd_ln_workspace_bytes(n, width))
    pv, gs, fo, o3v = None, 1.0, None, None
    if ce is not None:
        pv, gs = gvec(ce[0]), float(ce[1])
        fo, o3v = out1(3)
    if defer:
        check(lib().gte_fold_defer_begin(cs()), "defer_begin")
    head = (P(dlv), ld(dlv), P(qv), ld(qv), P(hv), ld(hv), f)
    tail = (P(Wv), ld(Wv), c, P(dz), ld(dz), P(img.data) if image else None, img.ldp if image else 0, P(dW), ld(dW), P(db), n, P(ws.t), ws.n,
            P(pv), gs, P(o3v), P(zv), ld(zv), P(stv), P(gv), P(bev), int(relu), P(dg), P(dbe), P(dbi), P(wl.t), wl.n, cs())
    try:
        if n_pad is None:
            check(lib().gte_sage_narrow_bwd_ln_p3(*head, *tail), "bwd_ln_p3")
        else:
            check(lib().gte_sage_narrow_bwd_ln_p3_pad(*head, n_pad, *tail), "bwd_ln_p3_pad")
    finally:
        if defer:
            check(lib().gte_fold_defer_flush(), "defer_flush")
    ws.ok()
    wl.ok()
    r = {"dW": done(fw, dW, allow_nonfinite), "db": done(fb, db), "dg": done(fg, dg), "dbe": done(fe, dbe), "dbi": done(fi, dbi),
         "out3": done(fo, o3v) if ce is not None else None, "img": None}
    # padded rows: the columns behind the last 16-byte chunk of the true width are the caller's (the sentinel survives there)
    full = done(fz, dz)
    w4 = c4(f) if n_pad else f
    assert (full[:, f:w4] == 0).all(), "columns n_feat .. the next multiple of 4 of dz_below must be written as zeros"
    assert (full[:, w4:] == SENTINEL).all(), "dz_below was written behind the last 16-byte chunk of the true width"
    r["dz"] = full[:, :f]
    if image:
        assert bool((img.data[n] == 0x55).all()), "written past the image's last row"
        dec = ops.p3_to_f32(ops.P3(img.data, n, c16(width))).cpu().numpy()
        assert (dec[:, f:] == 0).all(), "the padding of the image must be written as zeros"
        r["img"] = dec[:, :f]
    return r


def two_launches(dl, q, h, W, f, lnin, relu, n_pad=None):
    """gte_sage_narrow_bwd + gte_ln_relu_bwd[_p3] on plain buffers at the TRUE width: what the fused call replaces
    -> dz [n, f], image bytes or None, (dgamma, dbeta, dbias), bitwise (does the suite hold the fused call to these bits)"""
    n, c = dl.shape
    width = n_pad or f
    L = lib()
    new = lambda *s: torch.zeros(*s, device=DEV)
    dld, qd, hd, Wd, zd = dev(dl), dev(q), dev(h), dev(W), dev(lnin.z)
    std, gd, bd = dev(lnin.stats), dev(lnin.gamma), dev(lnin.beta)
    dh, dWa, dba = new(n, width), new(c, 2 * f), new(c)
    ws = torch.empty(int(L.gte_sage_narrow_bwd_workspace_bytes(n, width, c)), dtype=torch.uint8, device=DEV)
    check(L.gte_sage_narrow_bwd(P(dld), c, P(qd), c, P(hd), width, f, P(Wd), 2 * f, c, P(dh), width, P(dWa), 2 * f, P(dba), n, P(ws),
                                ws.numel(), cs()), "bwd (two launches)")
    sums = [new(f) for _ in range(3)]
    wl = torch.empty(int(L.gte_ln_relu_bwd_workspace_bytes(n, f)), dtype=torch.uint8, device=DEV)
    use_img = n_pad is not None or (f % 16 == 0 and f >= 128)
    dza = new(n, width)
    if use_img:
        im = ops.P3.empty(n, f, DEV)
        check(L.gte_ln_relu_bwd_p3(P(dh), width, P(zd), width, P(std), P(gd), P(bd), int(relu), P(dza), width, P(im.data), im.ldp,
                                   P(sums[0]), P(sums[1]), P(sums[2]), n, f, P(wl), wl.numel(), cs()), "ln_relu_bwd_p3")
    else:
        check(L.gte_ln_relu_bwd(P(dh), width, P(zd), width, P(std), P(gd), P(bd), int(relu), P(dza), width, P(sums[0]), P(sums[1]),
                                P(sums[2]), n, f, P(wl), wl.numel(), cs()), "ln_relu_bwd")
    bitwise = n_pad is None and f % 16 == 0 and f >= 128            # (what test_gpu_parity.py demands bits of; tolerance otherwise)
    return dza.cpu().numpy()[:, :f], tuple(s.cpu().numpy() for s in sums), bitwise


def close(got, want, what, extra=0.0):
    """the tolerance test_gpu_parity.py / test_gpu_shapes.py hold the fused LayerNorm backward to where they do not demand bits
    (+ extra: see ln_propagated)"""
    err = np.abs(got.astype(np.float64) - want)
    tol = 2e-5 * np.abs(want) + 3e-6 * float(np.abs(want).max()) + 1e-12 + extra
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} elements outside the tolerance, the worst by {float((err / tol).max()):.3g} x"


def ln_propagated(lnin, f, e):
    """The padded-row call and the two launches it is compared with form dh with DIFFERENT kernels (matrix pipe over n_pad columns /
    plain kernels over the true width), each within narrow_ref's dh bound of the true dh: the two dh differ by at most e = 2 x that
    bound, which the existing tolerance (stated on Gaussian data, where it is far below it) does not cover on rows that cancel.
    The LayerNorm backward is linear in dh for a given mask -- g = gamma mask dh, dz = rstd (g - mean(g) - xhat mean(g xhat)),
    dgamma = sum_r mask dh xhat, dbeta = sum_r mask dh, dbias = sum_r dz -- so e reaches its outputs by at most
    -> (dz [n, f], dgamma [f], dbeta [f], dbias [f])"""
    n = lnin.z.shape[0]
    z = lnin.z[:, :f].astype(np.float64)
    mean, rstd = lnin.stats[:n].astype(np.float64)[:, None], lnin.stats[n:].astype(np.float64)[:, None]
    xh = np.abs((z - mean) * rstd)
    eg = np.abs(lnin.gamma.astype(np.float64))[None, :] * e
    dz = rstd * (eg + eg.mean(1, keepdims=True) + xh * (eg * xh).mean(1, keepdims=True))
    return dz, (e * xh).sum(0), e.sum(0), dz.sum(0)


# ---- one shape, every entry point that serves it -----------------------------------------------------------------------------------------
def check_shape(n, f, c, n_pad=None, kinds=("exact",) + tuple(nr.BOUND_KINDS), forward=True, backward=True, ln=True):
    width = n_pad or f
    what0 = f"n={n} f={f} n_pad={n_pad} c={c}"
    for kind in kinds:
        case = nr.exact_case(n, f, c) if kind == "exact" else nr.bound_case(kind, n, f, c)
        what = f"{what0} {kind}"
        h = case.padded(n_pad) if n_pad else case.h
        if forward:
            entry = "fwd_pad" if n_pad else "fwd"
            ts, tn = run_fwd(h, case.W, case.bias, f, n_pad)
            rs, rn = nr.fwd(h, case.W, case.bias, f)
            bs, bn = nr.fwd_bound(h, case.W, case.bias, f, width)
            held(entry, case, what + " t_self", ts, rs, bs)
            held(entry, case, what + " t_neigh", tn, rn, bn)
            if n_pad is None and f % 8 == 0 and not case.exact:
                lnin = LnInputs(n, f, f, 1)
                relu = c % 2 == 1
                y, st, ts, tn = run_fwd_ln(lnin.z, lnin.gamma, lnin.beta, relu, case.W, case.bias)
                rs, rn = nr.fwd(y, case.W, case.bias, f)                     # the reference on the y the device wrote
                bs, bn = nr.fwd_bound(y, case.W, case.bias, f)
                note("fwd_ln", nr.ratio(ts, rs, bs), what + " t_self")
                note("fwd_ln", nr.ratio(tn, rn, bn), what + " t_neigh")
                y2 = torch.empty(n, f, device=DEV)
                st2 = torch.empty(2 * n, device=DEV)
                zd, gd, bd = dev(lnin.z), dev(lnin.gamma), dev(lnin.beta)
                check(lib().gte_ln_relu_fwd(P(zd), f, P(gd), P(bd), EPS_LN, int(relu), P(y2), f, P(st2), n, f, cs()), "ln_relu_fwd")
                np.testing.assert_allclose(y, y2.cpu().numpy(), rtol=2e-6, atol=2e-6, err_msg=what + " y against gte_ln_relu_fwd")
                np.testing.assert_allclose(st, st2.cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=what + " stats")
        if not backward:
            continue
        part = nr.exact_partials(n) if case.exact else nr.bound_partials(n)
        gs = 2.0 if case.exact else 0.37
        al = nr.alpha(part, gs)
        if n_pad is None:
            chain = nr.dw_chain(n, f, cus())
            ref = nr.bwd(case.dl, case.q, h, case.W)
            bnd = nr.bwd_bound(case.dl, case.q, h, case.W, chain)
            dh, dW, db, _ = run_bwd(case.dl, case.q, h, case.W, f)
            for name, g, r, b in zip(("dh", "dW", "dbias"), (dh, dW, db), ref, bnd):
                held("bwd", case, f"{what} {name}", g, r, b)
            _, dW2, db2, _ = run_bwd(case.dl, case.q, h, case.W, f, want_dh=False)
            assert nr.same_bits(dW2, dW) and nr.same_bits(db2, db), what + ": dW / dbias change with dh = NULL"
            if f % 8 == 0:
                ref = nr.bwd(case.dl, case.q, h, case.W, al)
                bnd = nr.bwd_bound(case.dl, case.q, h, case.W, chain, al)
                dh, dW, db, o3 = run_bwd(case.dl, case.q, h, case.W, f, ce=(part, gs))
                for name, g, r, b in zip(("dh", "dW", "dbias"), (dh, dW, db), ref, bnd):
                    held("bwd_ce", case, f"{what} {name}", g, r, b)
                check_out3(o3, part, case, what)
        if not ln or (n_pad is None and f % 8):
            continue
        # ---- the fused LayerNorm backward of the layer below
        entry = "bwd_ln_p3_pad" if n_pad else "bwd_ln_p3"
        lnin = LnInputs(n, f, width, 2)
        relu = c % 2 == 1
        chain = nr.dw_chain(n, width, cus(), ln=True)
        has_img = width % 16 == 0
        ref = nr.bwd(case.dl, case.q, h, case.W)
        bnd = nr.bwd_bound(case.dl, case.q, h, case.W, chain)
        dz2, sums2, bitwise = two_launches(case.dl, case.q, h, case.W, f, lnin, relu, n_pad)
        # (the ill-conditioned kinds on padded rows: the partner's dh comes from another kernel -- ln_propagated)
        extra = ln_propagated(lnin, f, 2 * bnd[0]) if n_pad and kind in ("scales", "cancel") else (0.0,) * 4
        plain = None
        for image in ((True, False) if has_img else (False,)):
            r = run_bwd_ln(case.dl, case.q, h, case.W, f, lnin, relu, n_pad, image=image)
            held(entry, case, what + " dW", r["dW"], ref[1], bnd[1])
            held(entry, case, what + " dbias", r["db"], ref[2], bnd[2])
            if bitwise:
                assert nr.same_bits(r["dz"], dz2), what + ": dz differs from gte_sage_narrow_bwd + gte_ln_relu_bwd_p3"
            else:
                close(r["dz"], dz2, what + " dz", extra[0])
            if image:
                assert np.array_equal(r["img"], r["dz"]), what + ": the image of dz differs from dz"
            for name, g, w_, ex in zip(("dg", "dbe", "dbi"), (r["dg"], r["dbe"], r["dbi"]), sums2, extra[1:]):
                close(g, w_, f"{what} {name}", ex)
            if plain is None:
                plain = r
            else:
                assert all(nr.same_bits(r[k], plain[k]) for k in ("dz", "dW", "db", "dg", "dbe", "dbi")), what + ": results change with dzp3 = NULL"
        # ce_partial given == ce_partial NULL on alpha dl, alpha q (alpha a power of two on the exact case: bit for bit)
        ref = nr.bwd(case.dl, case.q, h, case.W, al)
        bnd = nr.bwd_bound(case.dl, case.q, h, case.W, chain, al)
        r = run_bwd_ln(case.dl, case.q, h, case.W, f, lnin, relu, n_pad, ce=(part, gs), image=has_img)
        held(entry + " ce", case, what + " dW", r["dW"], ref[1], bnd[1])
        held(entry + " ce", case, what + " dbias", r["db"], ref[2], bnd[2])
        check_out3(r["out3"], part, case, what)
        pre = run_bwd_ln((case.dl * al).astype(np.float32), (case.q * al).astype(np.float32), h, case.W, f, lnin, relu, n_pad, image=has_img)
        for k in ("dz", "dW", "db", "dg", "dbe", "dbi") + (("img",) if has_img else ()):
            if case.exact:
                assert nr.same_bits(r[k], pre[k]), f"{what}: {k} with ce_partial differs from the call on alpha dl, alpha q"
            else:
                close(r[k], pre[k], f"{what} {k} with ce_partial")


def check_out3(o3, part, case, what):
    want = nr.out3(part)
    if case.exact:
        assert nr.same_bits(o3, want), f"{what}: out3 {o3} differs from {want}"
    else:       # float partials folded in double in another order: the doubles agree to ~2^-50, their float32 roundings to one ulp
        assert (np.abs(o3.astype(np.float64) - want) <= 2 * nr.U * np.abs(want)).all(), f"{what}: out3 {o3} against {want}"


# ---- every class group at every width ------------------------------------------------------------------------------------------------------
N_SWEEP = 37                # two 32-row blocks, three 16-row blocks, ten 4-row blocks, the last of each partial
ALL_CLASSES_AT = {13, 24, 48, 64}          # one width per family: plain, 32-row forward, 16-row forward, matrix-pipe backward
WIDTHS = sorted(set(sum(nr.FMA_WIDTHS.values(), []) + nr.MFMA32_WIDTHS + nr.MFMA16_WIDTHS + nr.BWD_MFMA_WIDTHS))
WIDTH_CLASS = [(f, c) for f in WIDTHS for c in (range(1, 17) if f in ALL_CLASSES_AT else nr.CLASS_EDGES)]


@pytest.mark.parametrize("f,c", WIDTH_CLASS, ids=[f"{nr.bwd_family(f)}-{f}-{c}" for f, c in WIDTH_CLASS])
def test_every_class_group_at_every_width(f, c):
    check_shape(N_SWEEP, f, c)


PAD_CLASS = [(f, p, c) for f, p in nr.PADDED for c in (range(1, 17) if (f, p) == (100, 112) else nr.CLASS_EDGES)]


@pytest.mark.parametrize("f,n_pad,c", PAD_CLASS, ids=[f"{f}-{p}-{c}" for f, p, c in PAD_CLASS])
def test_padded_rows(f, n_pad, c):
    assert lib().gte_sage_narrow_pad_supported(f, n_pad, c) == 1
    check_shape(N_SWEEP, f, c, n_pad)


ROW_SHAPES = {"fma": (13, None, 5), "mfma32": (24, None, 9), "mfma16": (48, None, 13), "bwd_mfma": (64, None, 9), "padded": (100, 112, 9)}


@pytest.mark.parametrize("n", nr.ROWS)
@pytest.mark.parametrize("family", list(ROW_SHAPES))
def test_row_counts_around_the_blocks(family, n):
    f, n_pad, c = ROW_SHAPES[family]
    check_shape(n, f, c, n_pad)


# ---- the grid-stride loops ---------------------------------------------------------------------------------------------------------------
def _grid_cases():
    return {"fma_fwd": lambda: (8199, 13, 5, dict(backward=False)),
            "fma_bwd": lambda: (nr.NB_MAX * 4 + 7, 13, 5, dict(forward=False)),
            "mfma_bwd": lambda: (32 * min(cus(), nr.NB_MAX) + 45, 64, 9, dict(forward=False, ln=False)),
            "mfma_bwd_ln": lambda: (32 * min(2 * cus(), nr.NB_MAX) + 45, 64, 9, dict(forward=False)),
            "mfma32_fwd": lambda: (262144 + 77, 8, 5, dict(backward=False)),
            "mfma16_fwd": lambda: (262144 + 77, 16, 5, dict(backward=False))}


@pytest.mark.parametrize("which", list(_grid_cases()))
def test_grid_stride_loops(which):
    """one exact case each at the smallest n at which a workgroup takes a second turn"""
    n, f, c, kw = _grid_cases()[which]()
    if which == "fma_fwd":
        assert -(-n // 4) > nr.FWD_FMA_BLOCKS
    elif which in ("mfma32_fwd", "mfma16_fwd"):
        assert -(-n // 128) > nr.FWD_MFMA_BLOCKS
    else:
        assert (-(-n // 32) if f % 8 == 0 else -(-n // 4)) > nr.bwd_grid(n, f, cus(), which == "mfma_bwd_ln")
    check_shape(n, f, c, kinds=("exact",), **kw)


# ---- deferred folds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,n_pad,c", [(64, None, 9), (256, None, 16), (100, 112, 5)])
def test_deferred_folds_equal_the_stand_alone_call(f, n_pad, c):
    n = 300
    width = n_pad or f
    lnin = LnInputs(n, f, width, 3)
    for kind in ("exact",) + tuple(nr.BOUND_KINDS):
        case = nr.exact_case(n, f, c) if kind == "exact" else nr.bound_case(kind, n, f, c)
        h = case.padded(n_pad) if n_pad else case.h
        a = run_bwd_ln(case.dl, case.q, h, case.W, f, lnin, True, n_pad, image=False)
        b = run_bwd_ln(case.dl, case.q, h, case.W, f, lnin, True, n_pad, image=False, defer=True)
        assert nr.same_bits(a["dz"], b["dz"])
        ref = nr.bwd(case.dl, case.q, h, case.W)
        bnd = nr.bwd_bound(case.dl, case.q, h, case.W, nr.dw_chain(n, width, cus(), ln=True))
        for k, i in (("dW", 1), ("db", 2)):
            held("bwd_ln_p3 deferred", case, f"f={f} n_pad={n_pad} c={c} {kind} {k}", b[k], ref[i], bnd[i])
            if case.exact:
                assert nr.same_bits(a[k], b[k])
        for k in ("dg", "dbe", "dbi"):
            close(b[k], a[k], f"deferred {k}")


# ---- non-finite confinement ------------------------------------------------------------------------------------------------------------------
CONFINE = [(13, None, 5), (24, None, 9), (48, None, 13), (64, None, 9), (100, 112, 9)]


@pytest.mark.parametrize("where", ["first", "last", "mid"])
@pytest.mark.parametrize("f,n_pad,c", CONFINE, ids=[f"{f}-{p}-{c}" for f, p, c in CONFINE])
def test_a_non_finite_row_of_h_stays_in_its_row_and_its_columns(f, n_pad, c, where):
    """+Inf and NaN in row r of h.  Forward: only row r of t_self / t_neigh is non-finite, every other row is bit for bit the clean
    run.  Backward: dh (which does not read h) is bit for bit the clean run, and in dW exactly the columns that hold the two values
    are non-finite; the same for dW of the fused LayerNorm backward (plain and padded rows), whose every other output is bit for
    bit the clean run.  A property of the arithmetic: nothing here reads out of bounds."""
    n = 70
    r = {"first": 0, "last": n - 1, "mid": 37}[where]
    case = nr.bound_case("gauss", n, f, c)
    c_inf, c_nan = 0, f - 1 if f < 16 else f - 3
    h0 = case.padded(n_pad) if n_pad else case.h.copy()
    h0[r, [c_inf, c_nan]] = 0.0
    hp = h0.copy()
    hp[r, c_inf], hp[r, c_nan] = np.inf, np.nan
    others = np.arange(n) != r
    clean, got = run_fwd(h0, case.W, case.bias, f, n_pad), run_fwd(hp, case.W, case.bias, f, n_pad, allow_nonfinite=True)
    for name, a, b in zip(("t_self", "t_neigh"), clean, got):
        assert not np.isfinite(b[r]).any(), f"{name}: row {r} stayed finite"
        assert nr.same_bits(a[others], b[others]), f"{name}: rows other than {r} changed"
    bad = np.zeros(2 * f, dtype=bool)
    bad[[c_inf, c_nan, f + c_inf, f + c_nan]] = True

    def dw_confined(dW0, dW1, entry):
        assert not np.isfinite(dW1[:, bad]).any(), f"{entry}: a column of dW that holds Inf / NaN stayed finite"
        assert nr.same_bits(dW1[:, ~bad], dW0[:, ~bad]), f"{entry}: the other columns of dW changed"
    if n_pad is None:
        dh0, dW0, db0, _ = run_bwd(case.dl, case.q, h0, case.W, f)
        dh1, dW1, db1, _ = run_bwd(case.dl, case.q, hp, case.W, f, allow_nonfinite=True)
        assert nr.same_bits(dh1, dh0) and nr.same_bits(db1, db0), "dh / dbias do not read h"
        dw_confined(dW0, dW1, "bwd")
    if n_pad is not None or f % 8 == 0:          # the fused LayerNorm backward: h feeds dW alone, dz and the column sums come from z
        lnin = LnInputs(n, f, n_pad or f, 4)
        a = run_bwd_ln(case.dl, case.q, h0, case.W, f, lnin, True, n_pad, image=False)
        b = run_bwd_ln(case.dl, case.q, hp, case.W, f, lnin, True, n_pad, image=False, allow_nonfinite=True)
        assert all(nr.same_bits(a[k], b[k]) for k in ("dz", "db", "dg", "dbe", "dbi")), "bwd_ln_p3: an output that does not read h changed"
        dw_confined(a["dW"], b["dW"], "bwd_ln_p3")


# ---- unsupported shapes ------------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_return_their_error_codes_without_launching():
    """n_out 0 and 17, n_feat 257, n_pad % 16 != 0, ce_partial with F % 8 != 0, a workspace one byte short, ld < width.  Every buffer is
    large enough for every one of these calls (600 floats a row), so a call that launched after all would stay inside them; the
    outputs are sentinel-filled and must come back untouched."""
    L = lib()
    INVALID, TOO_SMALL, UNSUPPORTED = -1, -3, -4
    n, f, c, LD = 40, 16, 5, 600
    zeros = lambda *s: torch.zeros(*s, device=DEV)
    sent = lambda *s: torch.full(s, SENTINEL, device=DEV)
    h, W, bias, dl, q, z = zeros(n + 1, LD), zeros(18, LD), zeros(32), zeros(n + 1, LD), zeros(n + 1, LD), zeros(n + 1, LD)
    stats, gam, bet, part = zeros(2 * n + 2), zeros(LD), zeros(LD), zeros(3 * n)
    outs = [sent(n + 1, LD) for _ in range(3)] + [sent(18, LD), sent(32), sent(3)]
    ts, tn, dh, dW, db, o3 = outs
    ws = Workspace(L.gte_sage_narrow_bwd_workspace_bytes(n, 256, 16))
    wl = Workspace(L.gte_sage_narrow_bwd_ln_workspace_bytes(n, 256))

    def fwd(nf, no, ldh=LD):
        return L.gte_sage_narrow_fwd(P(h), ldh, nf, P(W), LD, P(bias), no, P(ts), LD, P(tn), LD, n, cs())

    def bwd(nf, no, nbytes=ws.n, ldh=LD):
        return L.gte_sage_narrow_bwd(P(dl), LD, P(q), LD, P(h), ldh, nf, P(W), LD, no, P(dh), LD, P(dW), LD, P(db), n, P(ws.t), nbytes, cs())

    def bwd_ln(nf, ldz=LD, nbytes=wl.n, n_pad=None):
        head = (P(dl), LD, P(q), LD, P(h), LD, nf) + (() if n_pad is None else (n_pad,))
        tail = (P(W), LD, c, P(dh), LD, None, 0, P(dW), LD, P(db), n, P(ws.t), ws.n, None, 1.0, None, P(z), ldz, P(stats), P(gam), P(bet), 1,
                None, None, None, P(wl.t), nbytes, cs())
        return (L.gte_sage_narrow_bwd_ln_p3 if n_pad is None else L.gte_sage_narrow_bwd_ln_p3_pad)(*head, *tail)
    for no in (0, 17):
        assert fwd(f, no) == UNSUPPORTED and bwd(f, no) == UNSUPPORTED and L.gte_sage_narrow_supported(f, no) == 0
    assert fwd(257, c) == UNSUPPORTED and bwd(257, c) == UNSUPPORTED and L.gte_sage_narrow_supported(257, c) == 0
    assert fwd(f, c, ldh=f - 1) == INVALID and bwd(f, c, ldh=f - 1) == INVALID
    assert bwd(f, c, nbytes=int(L.gte_sage_narrow_bwd_workspace_bytes(n, f, c)) - 1) == TOO_SMALL
    # padded rows: n_pad must be a multiple of 16
    assert L.gte_sage_narrow_pad_supported(13, 24, c) == 0
    assert L.gte_sage_narrow_fwd_pad(P(h), LD, 13, 24, P(W), LD, P(bias), c, P(ts), LD, P(tn), LD, n, cs()) == UNSUPPORTED
    assert bwd_ln(13, n_pad=24) == UNSUPPORTED
    # ce_partial needs the matrix-pipe kernels: F % 8 == 0
    assert L.gte_head_supported(13, c) == 0
    assert L.gte_sage_narrow_bwd_ce(P(dl), LD, P(q), LD, P(h), LD, 13, P(W), LD, c, P(dh), LD, P(dW), LD, P(db), n, P(ws.t), ws.n, P(part), 1.0,
                                    P(o3), cs()) == UNSUPPORTED
    # the fused LayerNorm backward: its own workspace one byte short, a z narrower than the rows
    assert bwd_ln(f, nbytes=int(L.gte_sage_narrow_bwd_ln_workspace_bytes(n, f)) - 1) == TOO_SMALL
    assert bwd_ln(f, ldz=f - 1) == INVALID
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs), "a refused call wrote an output"
    ws.ok()
    wl.ok()
