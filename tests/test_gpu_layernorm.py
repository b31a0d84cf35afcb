"""Every LayerNorm(+ReLU) kernel through the C ABI against the float64 reference (tests/layernorm_ref.py, pinned to torch autograd
by tests/test_layernorm_ref_cpu.py) on ill-conditioned rows: a mean far above the spread, constant rows, all-zero rows with exact
ReLU ties, a variance far below eps, one non-zero entry, eps = 1e-5 and 1e-12, gamma with mixed signs and an exact zero, beta with
exact zeros.  Run with ``-m gpu`` on an MI355X; ``-s`` shows every case's worst error / bound ratio and its ambiguous count.

Bounds: derived in tests/layernorm_cases.py (module docstring) per row-sum family, checked there against a float32 emulation of the
kernels and against mutants (one-pass variance, padded width, n - 1, eps outside the root, mask on xhat, no c2 term), each of which
breaks them by more than 10x on these inputs.
    forward   |y - ref| <= D u |gamma_j| (1 + kappa) max(1, |xhat_j|) + 2^-23 |ref|,  |mean - ref| <= Dm u max|z_row|,
              |rstd / ref - 1| <= Dr u + min(1, (Dm u kappa)^2 / 2)
    backward  |dz - ref| <= Db u rstd max|gamma| ||dy_row||_2, the reference on the device's z and stats; column sums to Kc roundings
              of the sum of their absolute terms
with u = 2^-24 and (D, Dm, Dr, Db) = (2.5 R + 12, R + 2, R / 2 + 5, 2 R + 22) for a row-sum depth R.

ReLU masks: the backward kernels rebuild xhat from the STORED mean and rstd, the 16-byte forward (and the planes-GEMM epilogue) use
fma(-1 / n, sum, z); the two differ by about kappa u, so the masks can differ within the ambiguous band (|pre| <= 2 forward bounds).
The tests give those elements dy = 0 (at most 1 % of a case, asserted), print how many there are, and require the forward's y > 0 to
be the reference mask everywhere else.  The backward's mask is, by convention, the one on the stored stats (include/gte.h).  Exact
ties (zero rows, beta_j == 0) are computed without a rounding by every kernel: y == 0 and no gradient.

Out of scope: magnitudes at which (z - mean)^2 overflows float32; the fused backward forms gte_gemm_p3_nt_ln_bwd and
gte_sage_narrow_bwd_ln_p3(_pad), which consume stats rather than compute them and are held bit for bit to gte_ln_relu_bwd(_p3) by
tests/test_gemm_p3.py and tests/test_gpu_parity.py; gte_sage_smallk_bwd and the epilogue of gte_gemm_p3_nt_smallk_bwd, which recompute z
and never store dz, so that nothing of theirs can be held bit for bit: tests/test_gpu_smallk_bwd.py pins them to a float64 reference on
the same row kinds.

Largest error / bound ratios measured on an MI355X (all cases of this module):
    gte_ln_relu_fwd      y 0.077  mean 0.274  rstd 0.983      gte_ln_relu_bwd      dz 0.090  dgamma 0.134  dbeta 0.090  dbias 0.027
    gte_ln_relu_fwd_p3   y 0.057  mean 0.181  rstd 0.979      gte_ln_relu_bwd_p3   dz 0.042  dgamma 0.135  dbeta 0.103  dbias 0.023
    gte_spmm_csr_accumulate_ln(_p3)  y 0.039  mean 0.128  rstd 0.127      gte_sage_narrow_fwd_ln  y 0.030  mean 0.107  rstd 0.131
    gte_gemm_p3_nt_ln_fwd            y 0.023  mean 0.093  rstd 0.168      gte_sage_linear_fwd     y 0.022  mean 0.093  rstd 0.139
(rstd near 1 is the constant row 1000 at eps = 1e-12, where the bound's min(1, .) term is at its cap: the mean's rounding IS the
variance there.)  Largest neutralised share of a case 0.50 %.  Forward and backward masks differed at 589 (fwd / bwd) and 6641
(fwd_p3 / bwd_p3) of some 2.5 million elements each, every one inside the ambiguous band and all but 2 on constant rows, where xhat is
rounding noise in both kernels; the 16-byte forward differs from the stored-mean form in both of its forms (per-chunk validity at
n = 252, 260 as much as per-element validity on padded rows: one body, ln_relu_fwd_vec_kernel<NV, RF, MSK> of csrc/layernorm.hip), the
scalar forward does not.  No kernel broke a bound, so none was changed.  (gte_sage_linear_fwd has since been made to subtract the
rounded mean it stores, see tests/test_gpu_smallk_bwd.py; its figures above were measured again after that and are the same to the
digits shown, its cases having n = 4, 128 and 256, where the two forms are the same bits.)
"""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import layernorm_cases as lc
from tests import layernorm_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, cs, check = _lib.ptr, _lib.current_stream, _lib.check
NAN = float("nan")

PLAIN_NS = sorted(set(lc.FWD_SCALAR_NS + lc.FWD_VEC_NS + lc.BWD_NCH_NS + lc.BWD_VEC_NS + lc.BWD_WIDE_NS))
PLAIN_BIG = {65, 129, 256}                   # M_BIG at one width per backward kernel family: scalar NCH<2>, NCH<4>, vec
IMAGE_NS = sorted(set(lc.GEN_NS + [128]))    # (128: the backward's per-chunk form with an image next to the per-element forward)
IMAGE_BIG = {218}


def f32eps(eps):
    return float(np.float32(eps))            # what the float argument of the ABI holds


def c4(x):
    return -(-x // 4) * 4


def c16(x):
    return -(-x // 16) * 16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def padded(a, ld, fill=NAN):
    m, n = a.shape
    buf = torch.full((m, ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :n] = dev(np.asarray(a, np.float32))
    return buf


def nan_buf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def ratio(err, bound):
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bound)))


def image_f32(img, m, n):
    """the whole padded image row [m, c16(n)] as fp32.  The image is compared with the fp32 output as decoded VALUES: x = h + m + l
    gives + 0 for the planes of - 0 (which dz produces on all-tie rows), every other float32 comes back bit for bit."""
    return ops.p3_to_f32(ops.P3(img.data, m, c16(n))).cpu().numpy()


def poisoned_image(m, n):
    img = ops.P3.empty(m, n, DEV)
    img.data.fill_(0x55)
    return img


def run_fwd(zb, n, gd, bd, eps, relu, image, yb=None):
    """gte_ln_relu_fwd (image False) or gte_ln_relu_fwd_p3 -> (y buffer, image or None, stats)"""
    lib = _lib.load()
    m, ld = zb.shape
    yb = nan_buf(m, ld) if yb is None else yb
    stats = nan_buf(2 * m)
    if image:
        img = poisoned_image(m, n)
        check(lib.gte_ln_relu_fwd_p3(P(zb), ld, P(gd), P(bd), eps, int(relu), P(yb), yb.shape[1], P(img.data), img.ldp, P(stats), m, n,
                                     cs()), "ln_relu_fwd_p3")
        return yb, img, stats
    check(lib.gte_ln_relu_fwd(P(zb), ld, P(gd), P(bd), eps, int(relu), P(yb), yb.shape[1], P(stats), m, n, cs()), "ln_relu_fwd")
    return yb, None, stats


def run_bwd(gb, zb, stats, n, gd, bd, relu, image, dzb=None):
    """gte_ln_relu_bwd / gte_ln_relu_bwd_p3 -> (dz buffer, image or None, dgamma, dbeta, dbias)"""
    lib = _lib.load()
    m, ld = gb.shape
    dzb = nan_buf(m, ld) if dzb is None else dzb
    sums = [nan_buf(n) for _ in range(3)]
    nbytes = int(lib.gte_ln_relu_bwd_workspace_bytes(m, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if image:
        img = poisoned_image(m, n)
        check(lib.gte_ln_relu_bwd_p3(P(gb), ld, P(zb), zb.shape[1], P(stats), P(gd), P(bd), int(relu), P(dzb), dzb.shape[1], P(img.data),
                                     img.ldp, P(sums[0]), P(sums[1]), P(sums[2]), m, n, P(ws), nbytes, cs()), "ln_relu_bwd_p3")
        return (dzb, img) + tuple(sums)
    check(lib.gte_ln_relu_bwd(P(gb), ld, P(zb), zb.shape[1], P(stats), P(gd), P(bd), int(relu), P(dzb), dzb.shape[1], P(sums[0]),
                              P(sums[1]), P(sums[2]), m, n, P(ws), nbytes, cs()), "ln_relu_bwd")
    return (dzb, None) + tuple(sums)


def check_padding(buf, n, image, what):
    """columns n .. the next multiple of 4 are written as zeros by the padded-row (image) forms; everything else is untouched"""
    a = buf.cpu().numpy()
    n4 = c4(n) if image else n
    assert (a[:, n:n4] == 0).all(), f"{what}: columns n .. n4 must be written as zeros"
    assert np.isnan(a[:, n4:]).all(), f"{what}: the padding was written"
    return a[:, :n]


def check_forward(tag, r, z, gamma, beta, e32, relu, y, mean, rstd):
    """y and the stats of any forward form against the reference on the same z; returns (band, ambiguous by the reference)"""
    y_ref, pre_ref, mean_ref, rstd_ref = ref.fwd(z, gamma, beta, e32, relu)
    xhat = (z.astype(np.float64) - mean_ref[:, None]) * rstd_ref[:, None]
    assert np.isfinite(y).all() and np.isfinite(mean).all() and np.isfinite(rstd).all(), tag
    ry = ratio(np.abs(y - y_ref), lc.fwd_bound(r, z, gamma, e32, xhat, y_ref))
    rm = ratio(np.abs(mean - mean_ref), lc.mean_bound(r, z))
    rr = ratio(np.abs(rstd / rstd_ref - 1), lc.rstd_bound(r, z, e32))
    band = lc.band(r, z, gamma, beta, e32)
    amb = ref.ambiguous(z, mean_ref, rstd_ref, gamma, beta, band)
    print(f"{tag}: error / bound  y {ry:.3f}  mean {rm:.3f}  rstd {rr:.3f};  ambiguous by the reference {int(amb.sum())} of {amb.size}")
    assert ry <= 1 and rm <= 1 and rr <= 1, (tag, ry, rm, rr)
    if relu:
        assert ((y > 0) == (pre_ref > 0))[~amb].all(), f"{tag}: the forward's ReLU mask differs where the reference is unambiguous"
    zr = lc.zero_rows(z)                                                  # exact: mean 0, rstd 1 / sqrt(eps) rounded once, y = relu?(beta)
    want = np.maximum(beta, 0) if relu else beta
    assert (mean[zr] == 0).all() and (y[zr] == want).all(), f"{tag}: a zero row is not exact"
    return band


def check_standalone(case, image, relu):
    m, n, vi, plant, eps, unit, seed = case
    z, dy, gamma, beta = lc.make_case(m, n, plant, seed, unit)
    e32 = f32eps(eps)
    r = lc.depth(lc.standalone_family(n, image), n)
    ld = c4(n) + 4 if image else n + (8 if n % 4 == 0 and m % 2 else 5)
    tag = f"{'p3' if image else 'f32'} M={m} n={n} v{vi} eps={eps} relu={int(relu)}"
    gd, bd = dev(gamma), dev(beta)
    zb = padded(z, ld)
    # ---------------- forward
    yb, img, stats = run_fwd(zb, n, gd, bd, eps, relu, image)
    y = check_padding(yb, n, image, "y")
    st = stats.cpu().numpy()
    mean, rstd = st[:m], st[m:]
    band = check_forward("fwd " + tag, r, z, gamma, beta, e32, relu, y, mean, rstd)
    if image:
        im = image_f32(img, m, n)
        assert np.array_equal(im[:, :n], y) and (im[:, n:] == 0).all(), "image of y"
    yb2, img2, stats2 = run_fwd(zb, n, gd, bd, eps, relu, image)                           # two runs: the same bits
    assert torch.equal(yb2[:, :n], yb[:, :n]) and torch.equal(stats2, stats)
    if image:
        assert torch.equal(img2.data, img.data)
    else:
        zin = zb.clone()                                                                   # in place (gte_ln_relu_fwd allows y == z)
        _, _, stats3 = run_fwd(zin, n, gd, bd, eps, relu, False, yb=zin)
        assert torch.equal(zin[:, :n], yb[:, :n]) and torch.equal(stats3, stats) and bool(torch.isnan(zin[:, n:]).all())
    # ---------------- backward: the reference on the device's stats, ambiguous elements get dy = 0
    share, n_amb, n_dis, n_dis_nc = 0.0, 0, 0, 0
    if relu:
        amb = ref.ambiguous(z, mean, rstd, gamma, beta, band)
        # the backward's own mask (float32 pre on the stored stats) against the forward's y > 0: on record, and inside the band
        xh32 = ((z - mean[:, None]).astype(np.float32) * rstd[:, None]).astype(np.float32)
        pre32 = lc.fma(xh32, np.broadcast_to(gamma, z.shape), np.broadcast_to(beta, z.shape))
        dis = (y > 0) != (pre32 > 0)
        n_dis, n_dis_nc = int(dis.sum()), int(dis[~lc.const_rows(z)].sum())
        assert not (dis & ~amb).any(), f"{tag}: forward and backward masks disagree outside the ambiguous band"
        dy, share = lc.neutralise(dy, amb, z)
        n_amb = int(amb.sum())
        assert share <= lc.AMBIGUOUS_CAP, (tag, share)
    gb = padded(dy, ld)
    dzb, dimg, dgd, dbd, dbiasd = run_bwd(gb, zb, stats, n, gd, bd, relu, image)
    dz = check_padding(dzb, n, image, "dz")
    assert np.isfinite(dz).all()
    dz_ref, dg_ref, db_ref, dbias_ref = ref.bwd(dy, z, mean, rstd, gamma, beta, relu)
    rb_rows = lc.bwd_bound(r, dy, rstd, gamma)
    rb = ratio(np.abs(dz - dz_ref), rb_rows[:, None])
    kc = lc.colsum_roundings(m) * lc.U
    xhat = (z.astype(np.float64) - mean[:, None].astype(np.float64)) * rstd[:, None].astype(np.float64)
    g = np.abs(np.where(xhat * gamma.astype(np.float64) + beta > 0, dy, 0) if relu else dy).astype(np.float64)
    dgam, dbet, dbias = (t.cpu().numpy().astype(np.float64) for t in (dgd, dbd, dbiasd))
    rg = ratio(np.abs(dgam - dg_ref), kc * (g * np.abs(xhat)).sum(0))
    rbt = ratio(np.abs(dbet - db_ref), kc * g.sum(0))
    rbi = ratio(np.abs(dbias - dbias_ref), rb_rows.sum() + kc * (np.abs(dz_ref) + rb_rows[:, None]).sum(0))
    print(f"bwd {tag}: error / bound  dz {rb:.3f}  dgamma {rg:.3f}  dbeta {rbt:.3f}  dbias {rbi:.3f};  ambiguous on the device's stats "
          f"{n_amb} ({100 * share:.3f} % neutralised outside constant rows), forward / backward masks differ at {n_dis} ({n_dis_nc} outside constant rows)")
    assert rb <= 1 and rg <= 1 and rbt <= 1 and rbi <= 1, (tag, rb, rg, rbt, rbi)
    zr = lc.zero_rows(z)
    if relu and zr.any():                                                 # the planted exact ties carry a non-zero dy and get none of it
        tie = zr[:, None] & (beta == 0)[None, :]
        assert tie.any() == bool((beta == 0).any()) and (dy[tie] != 0).all()
        if unit:                                                          # gamma = 1, beta = 0: the whole row is a tie
            assert (dz[zr] == 0).all()
        if zr.all():                                                      # nothing but tied rows: those columns of dbeta stay empty
            assert (dbet[beta == 0] == 0).all()
    if image:
        im = image_f32(dimg, m, n)
        assert np.array_equal(im[:, :n], dz) and (im[:, n:] == 0).all(), "image of dz"
    out2 = run_bwd(gb, zb, stats, n, gd, bd, relu, image)                                  # two runs: the same bits
    assert torch.equal(out2[0][:, :n], dzb[:, :n]) and all(torch.equal(a, b) for a, b in zip(out2[2:], (dgd, dbd, dbiasd)))
    if n <= 1024:                                                                          # in place over dy
        gin = gb.clone()
        out3 = run_bwd(gin, zb, stats, n, gd, bd, relu, image, dzb=gin)
        assert torch.equal(gin[:, :n], dzb[:, :n]) and all(torch.equal(a, b) for a, b in zip(out3[2:], (dgd, dbd, dbiasd)))
        check_padding(gin, n, image, "dz in place")


@pytest.mark.parametrize("n", PLAIN_NS)
def test_ln_relu_fwd_and_bwd_on_ill_conditioned_rows(n):
    """gte_ln_relu_fwd (scalar and vector kernels) and gte_ln_relu_bwd (NCH, vector and wide kernels)"""
    for case in lc.cases([n], n if n in PLAIN_BIG else None):
        for relu in (True, False):
            check_standalone(case, False, relu)


@pytest.mark.parametrize("n", IMAGE_NS)
def test_ln_relu_fwd_p3_and_bwd_p3_on_ill_conditioned_rows(n):
    """gte_ln_relu_fwd_p3 (the MSK form of the 16-byte kernel, every (NV, RF)) and gte_ln_relu_bwd_p3 (gen kernel; vec kernel with an
    image at n % 16 == 0 in 128 .. 512) on padded rows"""
    for case in lc.cases([n], n if n in IMAGE_BIG else None):
        for relu in (True, False):
            check_standalone(case, True, relu)


# ------------------------------------------------------------------------------------------------ plain against image entry points
SAME_BITS_NS = [128, 132, 252, 256, 260, 500, 512]     # multiples of 4 in 128 .. 512, both sides of the NV step, some multiples of 16
SAME_BITS_MS = [1, 3, 9]
SAME_BITS_BIG = 260


def same_bits_plants(m):
    """row -> kind so that every kind of layernorm_cases.KINDS is planted at every row count, with ordinary rows in between"""
    if m > 9:
        return lc.variants(m)                          # (every kind in one matrix)
    rows = list(range(0, m, 2))
    return [dict(zip(rows, lc.KINDS[i:i + len(rows)])) for i in range(0, len(lc.KINDS), len(rows))]


@pytest.mark.parametrize("n", SAME_BITS_NS)
def test_plain_and_image_entry_points_agree_bit_for_bit(n):
    """gte_ln_relu_fwd against gte_ln_relu_fwd_p3 and gte_ln_relu_bwd against gte_ln_relu_bwd_p3 on the same padded rows: the same y,
    stats, dz and column sums to the bit at every width both accept.  At n % 16 == 0 both backward entry points launch the same
    instantiation; elsewhere the plain entry runs the per-chunk-mask kernel and the image entry the per-element-mask kernel.  The forward
    is one body with both forms (csrc/layernorm.hip); this test holds the forms together in both directions."""
    ld = n + 4
    for m in SAME_BITS_MS + ([lc.M_BIG] if n == SAME_BITS_BIG else []):
        plants = same_bits_plants(m)
        assert {k for p in plants for k in p.values()} == set(lc.KINDS)
        for pi, plant in enumerate(plants):
            rng = np.random.default_rng(31000 + 100 * n + 10 * min(m, 10) + pi)
            z = lc.plant_rows(rng.standard_normal((m, n)).astype(np.float32), plant, rng)
            dy = rng.standard_normal((m, n)).astype(np.float32)
            gamma, beta = lc.make_params(n, rng)
            gd, bd, zb, gb = dev(gamma), dev(beta), padded(z, ld), padded(dy, ld)
            eps = (1e-5, 1e-12)[(m + pi) % 2]
            for relu in (True, False):
                tag = f"n={n} M={m} plant {pi} relu={int(relu)}"
                y0, _, st0 = run_fwd(zb, n, gd, bd, eps, relu, False)
                y1, _, st1 = run_fwd(zb, n, gd, bd, eps, relu, True)
                assert bool(torch.isfinite(y0[:, :n]).all()) and bool(torch.isfinite(st0).all()), tag
                assert torch.equal(y0[:, :n], y1[:, :n]), f"y {tag}"
                assert torch.equal(st0[:m], st1[:m]) and torch.equal(st0[m:], st1[m:]), f"stats {tag}"
                out0 = run_bwd(gb, zb, st0, n, gd, bd, relu, False)
                out1 = run_bwd(gb, zb, st0, n, gd, bd, relu, True)
                assert bool(torch.isfinite(out0[0][:, :n]).all()), tag
                assert torch.equal(out0[0][:, :n], out1[0][:, :n]), f"dz {tag}"
                for name, a, b in zip(("dgamma", "dbeta", "dbias"), out0[2:], out1[2:]):
                    assert torch.equal(a, b), f"{name} {tag}"


# ------------------------------------------------------------------------------------------------ the fused forward forms
def fused_rows(n, rng, offset):
    """the smallest matrix with an offset row, a constant row, a zero row and a random row; ``offset``: what the form's carrier (bias,
    t_self) adds to every column"""
    z = rng.standard_normal((4, n)).astype(np.float32)
    z[0] = (offset + rng.standard_normal(n)).astype(np.float32)
    z[1] = np.float32(-3.0)
    z[2] = 0
    return z


def fused_params(n, rng):
    gamma, beta = lc.make_params(n, rng)
    return gamma, beta, dev(gamma), dev(beta)


def check_fused(tag, r, zb, n, gamma, beta, eps, relu, yb, stats, img=None, n_pad=None):
    """y / stats of a fused form against the reference on the z the device wrote"""
    m = zb.shape[0]
    z = zb.cpu().numpy()[:, :n]
    assert np.isfinite(z).all()
    y = yb.cpu().numpy()
    st = stats.cpu().numpy()
    check_forward(tag, r, z, gamma, beta, f32eps(eps), relu, y[:, :n], st[:m], st[m:])
    if n_pad is not None:                                                  # padded rows: zeros up to n_pad, nothing behind
        for name, a in (("z", zb.cpu().numpy()), ("y", y)):
            assert (a[:, n:n_pad] == 0).all() and np.isnan(a[:, n_pad:]).all(), f"{tag}: padding of {name}"
    if img is not None:
        im = image_f32(img, m, n)
        assert np.array_equal(im[:, :n], y[:, :n]) and (im[:, n:] == 0).all(), f"{tag}: image of y"
    return z


@pytest.mark.parametrize("image", [False, True], ids=["accumulate_ln", "accumulate_ln_p3"])
@pytest.mark.parametrize("n", [16, 32, 64, 128, 256, 512, 1000, 218])
def test_aggregation_with_layernorm_epilogue_on_ill_conditioned_rows(n, image):
    """gte_spmm_csr_accumulate_ln(_p3): one width per (G, CPL) instantiation and 218 for MASK (1000 is masked too with an image).  The
    offset rides on t_self; row 0 is a hub, rows 1 and 2 (constant, zero) are empty, row 4 is a second offset row under the hub's weight."""
    lib = _lib.load()
    rng = np.random.default_rng(7000 + n)
    m = 6
    t_self = np.concatenate([fused_rows(n, rng, 1e3), rng.standard_normal((2, n)).astype(np.float32)])
    t_self[4] += np.float32(100.0)
    t_neigh = rng.standard_normal((m, n)).astype(np.float32)
    deg = [40, 0, 0, 3, 5, 2]                                             # row 0: hub (sources repeat), rows 1, 2: empty
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    indices = rng.integers(0, m, indptr[-1]).astype(np.int32)
    w = rng.uniform(0.1, 1, indptr[-1]).astype(np.float32)
    gamma, beta, gd, bd = fused_params(n, rng)
    n_pad = c16(n) if image else c4(n)
    ld = n_pad + 4
    g, cpl = lc.spmm_group(n, image)
    r = lc.depth("spmm", n, g, cpl)
    xb = padded(t_neigh, ld, fill=0.0)                                    # the padding of x is read and must hold zeros
    for eps, relu in ((1e-5, True), (1e-12, False)):
        zb, yb, stats = padded(t_self, ld), nan_buf(m, ld), nan_buf(2 * m)
        img = poisoned_image(m, n) if image else None
        ip, ix, wd = dev(indptr), dev(indices), dev(w)
        if image:
            check(lib.gte_spmm_csr_accumulate_ln_p3(P(ip), P(ix), P(wd), P(xb), ld, P(zb), ld, m, n, 1, P(gd), P(bd), eps, int(relu), P(yb),
                                                    ld, P(img.data), img.ldp, P(stats), cs()), "accumulate_ln_p3")
        else:
            check(lib.gte_spmm_csr_accumulate_ln(P(ip), P(ix), P(wd), P(xb), ld, P(zb), ld, m, n, 1, P(gd), P(bd), eps, int(relu), P(yb), ld,
                                                 P(stats), cs()), "accumulate_ln")
        z = check_fused(f"spmm{'_p3' if image else ''} n={n} (G={g}, CPL={cpl}) eps={eps} relu={int(relu)}", r, zb, n, gamma, beta, eps,
                        relu, yb, stats, img, n_pad)
        assert np.array_equal(z[1:3], t_self[1:3])                        # empty rows: z is t_self, the constant and the zero row exact
        agg = np.zeros((m, n))
        for v in range(m):
            e = slice(indptr[v], indptr[v + 1])
            if deg[v]:
                agg[v] = (w[e, None].astype(np.float64) * t_neigh[indices[e]]).sum(0) / deg[v]
        assert np.abs(z - (t_self + agg)).max() <= 1e-6 * (np.abs(t_self).max() + 8)


@pytest.mark.parametrize("n", [8, 128, 256])
def test_narrow_forward_with_layernorm_on_ill_conditioned_rows(n):
    """gte_sage_narrow_fwd_ln: the 256-thread kernel (n % 16 != 0: 8) and the 512-thread kernel (128, 256); t_self / t_neigh against
    float64 y W^T on the y the device wrote"""
    lib = _lib.load()
    rng = np.random.default_rng(8000 + n)
    m, c = 4, 9
    z = fused_rows(n, rng, 1e3)
    gamma, beta, gd, bd = fused_params(n, rng)
    W = (rng.standard_normal((c, 2 * n)) / np.sqrt(2 * n)).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    Wd, biasd = dev(W), dev(bias)
    r = lc.depth("narrow", n)
    for eps, relu in ((1e-5, True), (1e-12, False)):
        zb = padded(z, n + 4)
        yb, stats, ts, tn = nan_buf(m, n + 4), nan_buf(2 * m), nan_buf(m, c + 3), nan_buf(m, c + 3)
        check(lib.gte_sage_narrow_fwd_ln(P(zb), n + 4, n, P(gd), P(bd), eps, int(relu), P(yb), n + 4, P(stats), P(Wd), 2 * n, P(biasd), c,
                                         P(ts), c + 3, P(tn), c + 3, m, cs()), "narrow_fwd_ln")
        check_fused(f"narrow n={n} eps={eps} relu={int(relu)}", r, zb, n, gamma, beta, eps, relu, yb, stats)
        assert bool(torch.isnan(yb[:, n:]).all()) and bool(torch.isnan(ts[:, c:]).all()) and bool(torch.isnan(tn[:, c:]).all())
        y = yb.cpu().numpy()[:, :n].astype(np.float64)
        for name, got, want, sc in (("t_self", ts, y @ W[:, :n].T.astype(np.float64) + bias, np.abs(y) @ np.abs(W[:, :n]).T + np.abs(bias)),
                                    ("t_neigh", tn, y @ W[:, n:].T.astype(np.float64), np.abs(y) @ np.abs(W[:, n:]).T)):
            # an fp32 dot product of n terms: at most n + 1 roundings of the sum of the absolute terms
            assert (np.abs(got.cpu().numpy()[:, :c] - want) <= (n + 1) * lc.U * sc + 1e-30).all(), name


def _gemm_operands(m, n, k, rng, zero_row):
    x = rng.standard_normal((m, k)).astype(np.float32)
    x[zero_row] = 0
    kp = c16(k)
    wb = np.zeros((n, kp), np.float32)
    wb[:, :k] = rng.standard_normal((n, k)).astype(np.float32) / np.sqrt(k)
    return x, wb


@pytest.mark.parametrize("n", [5, 100, 218, 256])
def test_planes_gemm_with_layernorm_epilogue_on_ill_conditioned_rows(n):
    """gte_gemm_p3_nt_ln_fwd: the offset rides on the bias.  bias = 1000 in every column makes the rows of random operands offset rows
    and the row of a zero operand a constant row; bias = 0 makes them random rows and a zero row."""
    from tests.test_gemm_p3 import _weights
    rng = np.random.default_rng(9000 + n)
    m, k = 3, 32                                                         # (two K blocks: a block-major image with a block stride)
    x, wb = _gemm_operands(m, n, k, rng, zero_row=1)
    a1 = ops.p3_from_f32(dev(x))
    w = ops.P3(ops.p3_from_f32(dev(wb)).data, n, wb.shape[1])
    gamma, beta, gd, bd = fused_params(n, rng)
    r = lc.depth("tile", n)
    ld = c4(n) + 4
    for bias_value, eps, relu, block_major in ((1000.0, 1e-5, True, False), (0.0, 1e-12, False, True), (0.0, 1e-5, True, False)):
        bias = dev(np.full(n, bias_value, np.float32))
        zb, yb, stats, img = nan_buf(m, ld), nan_buf(m, ld), nan_buf(2 * m), poisoned_image(m, n)
        ops.gemm_p3_nt_ln_fwd(a1, _weights(w, block_major), None, bias, gd, bd, eps, relu, zb, y=yb, yp3=img, stats=stats)
        z = check_fused(f"gemm_p3 n={n} bias={bias_value} eps={eps} relu={int(relu)}", r, zb, n, gamma, beta, eps, relu, yb, stats, img, c4(n))
        assert (z[1] == np.float32(bias_value)).all()                     # the constant / the zero row, exact
        want = x.astype(np.float64) @ wb[:, :k].T.astype(np.float64) + bias_value
        assert np.abs(z - want).max() <= 1e-5 * (1 + abs(bias_value))


@pytest.mark.parametrize("k1,k2,n", [(1, 1, 4), (13, 13, 128), (32, 32, 256), (1, 1, 256), (32, 32, 4), (13, 13, 256)])
def test_short_input_layer_one_pass_form_on_ill_conditioned_rows(k1, k2, n):
    """gte_sage_linear_fwd where it runs linear + LayerNorm + ReLU in one pass (sage_smallk_fwd_kernel): k1 + k2 in {2, 26, 64}, n_out in
    {4, 128, 256}; the offset rides on the bias as in the planes-GEMM test."""
    lib = _lib.load()
    assert lib.gte_sage_linear_fwd_fuses_ln(k1 + k2, n) == 1
    rng = np.random.default_rng(9500 + 10 * n + k1)
    m = 3
    a1 = rng.standard_normal((m, k1)).astype(np.float32)
    a2 = rng.standard_normal((m, k2)).astype(np.float32)
    a1[1], a2[1] = 0, 0
    W = (rng.standard_normal((n, k1 + k2)) / np.sqrt(k1 + k2)).astype(np.float32)
    gamma, beta, gd, bd = fused_params(n, rng)
    a1d, a2d, Wd = padded(a1, k1 + 3, fill=NAN), padded(a2, k2 + 1, fill=NAN), padded(W, k1 + k2 + 2, fill=NAN)
    r = lc.depth("tile", n)
    for bias_value, eps, relu in ((1000.0, 1e-5, True), (0.0, 1e-12, False), (0.0, 1e-5, True)):
        bias = dev(np.full(n, bias_value, np.float32))
        zb, yb, stats = nan_buf(m, n + 4), nan_buf(m, n + 8), nan_buf(2 * m)
        check(lib.gte_sage_linear_fwd(P(a1d), k1 + 3, k1, P(a2d), k2 + 1, k2, P(Wd), k1 + k2 + 2, P(bias), P(gd), P(bd), eps, int(relu),
                                      P(zb), n + 4, P(stats), P(yb), n + 8, m, n, cs()), "sage_linear_fwd")
        z = check_fused(f"smallk k={k1 + k2} n={n} bias={bias_value} eps={eps} relu={int(relu)}", r, zb, n, gamma, beta, eps, relu, yb, stats)
        assert bool(torch.isnan(zb[:, n:]).all()) and bool(torch.isnan(yb[:, n:]).all())
        assert (z[1] == np.float32(bias_value)).all()
        want = np.concatenate([a1, a2], 1).astype(np.float64) @ W.T.astype(np.float64) + bias_value
        assert np.abs(z - want).max() <= 1e-5 * (1 + abs(bias_value))
