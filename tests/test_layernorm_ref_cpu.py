"""The float64 LayerNorm reference (tests/layernorm_ref.py), the error bounds of tests/layernorm_cases.py and the inputs of
tests/test_gpu_layernorm.py, checked without a GPU:

  * the reference against torch.nn.functional.layer_norm + autograd in float64 on every input family;
  * a float32 numpy emulation of the kernels' arithmetic (two-pass statistics, the row summed in lane-and-tree order, the three forms
    of z - mean) stays within the bounds derived in tests/layernorm_cases.py on every case the GPU tests run -- its worst ratio to the
    bound is printed and is at most 1;
  * mutants of that emulation (a one-pass variance, statistics over the padded width, n - 1, eps outside the square root, the ReLU
    mask on xhat, the backward without its c2 term) each break the bound by at least 10x on at least one of those cases -- so a kernel
    that made one of these mistakes would fail tests/test_gpu_layernorm.py;
  * the share of elements the GPU tests neutralise as ambiguous (dy = 0) stays under 1 % in every case.
Run with ``-s`` to see the ratios."""
import numpy as np
import pytest
import torch

from tests import layernorm_cases as lc
from tests import layernorm_ref as ref

# (widths, emulated layout, row-sum family of the bound, width that also runs M_BIG)
FAMILIES = {
    "fwd_scalar": (lc.FWD_SCALAR_NS, "scalar", "scalar", 65),
    "fwd_vec": (lc.FWD_VEC_NS, "vec", "vec", 256),
    "gen": (lc.GEN_NS, "gen", "vec", 218),
    "bwd_nch": (lc.BWD_NCH_NS, "scalar", "scalar", 129),
    "bwd_wide": (lc.BWD_WIDE_NS, "scalar", "scalar", None),
}


def _ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0, anything non-finite as infinite"""
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q))


def _all_cases():
    for fam, (ns, layout, rfam, big) in FAMILIES.items():
        for case in lc.cases(ns, big):
            yield fam, layout, rfam, case


def _torch_ln(z, gamma, beta, eps, relu, dy):
    zt = torch.from_numpy(np.asarray(z, np.float64)).requires_grad_(True)
    gt = torch.from_numpy(np.asarray(gamma, np.float64)).requires_grad_(True)
    bt = torch.from_numpy(np.asarray(beta, np.float64)).requires_grad_(True)
    y = torch.nn.functional.layer_norm(zt, (z.shape[1],), gt, bt, eps)
    y = y.relu() if relu else y
    y.backward(torch.from_numpy(np.asarray(dy, np.float64)))
    return y.detach().numpy(), zt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("relu", [True, False])
def test_reference_matches_torch_layer_norm_and_autograd_in_float64(relu):
    """1e-12 relative to the conditioning scale of each quantity: |gamma| (1 + kappa) max(1, |xhat|) + |y| forward,
    rstd max|gamma| ||dy_row|| (1 + kappa) backward (float64 has its own kappa u); near ties (|pre| < 1e-9) get dy = 0."""
    worst = 0.0
    for n in (1, 3, 65, 218, 256, 1100):
        for m, _, vi, plant, eps, unit, seed in lc.cases([n]):
            z, dy, gamma, beta = lc.make_case(m, n, plant, seed, unit)
            y, pre, mean, rstd = ref.fwd(z, gamma, beta, eps, relu)
            dy = np.where(np.abs(pre) < 1e-9, 0, dy).astype(np.float64)
            dz, dgamma, dbeta, dbias = ref.bwd(dy, z, mean, rstd, gamma, beta, relu)
            ty, tdz, tdg, tdb = _torch_ln(z, gamma, beta, eps, relu, dy)
            k = ref.kappa(z, eps)
            xhat = (z.astype(np.float64) - mean[:, None]) * rstd[:, None]
            fs = np.abs(gamma.astype(np.float64)) * (1 + k)[:, None] * np.maximum(1, np.abs(xhat)) + np.abs(y)
            bs = (rstd * np.abs(gamma).max() * np.sqrt((dy * dy).sum(1)) * (1 + k))[:, None]
            worst = max(worst, _ratio(np.abs(y - ty), 1e-12 * fs), _ratio(np.abs(dz - tdz), 1e-12 * bs))
            assert (np.abs(y - ty) <= 1e-12 * fs).all(), (m, n, vi, eps)
            assert (np.abs(dz - tdz) <= 1e-12 * bs).all(), (m, n, vi, eps)
            gx = np.abs(np.where(pre > 0, dy, 0) if relu else dy)
            assert (np.abs(dgamma - tdg) <= 1e-12 * ((gx * np.maximum(1, np.abs(xhat)) * (1 + k)[:, None]).sum(0) + 1e-300)).all()
            assert (np.abs(dbeta - tdb) <= 1e-12 * (gx.sum(0) + 1e-300)).all()
            assert (np.abs(dbias - tdz.sum(0)) <= 1e-12 * (np.abs(tdz) + bs).sum(0)).all()
    print(f"reference vs torch float64, relu={relu}: worst error / (1e-12 scale) = {worst:.3e}")


def test_reference_conventions():
    z = np.array([[0, 0, 0, 0], [1, 2, 3, 6]], np.float32)
    gamma, beta = np.array([1, -1, 2, 0], np.float32), np.array([0, 0, 0.5, 0], np.float32)
    y, pre, mean, rstd = ref.fwd(z, gamma, beta, 1e-5, True)
    assert (pre[0] == beta).all() and (y[0] == [0, 0, 0.5, 0]).all() and mean[0] == 0 and rstd[0] == 1 / np.sqrt(1e-5)
    var = ((z[1].astype(np.float64) - 3) ** 2).mean()                              # biased, over the 4 columns
    assert mean[1] == 3 and abs(rstd[1] - 1 / np.sqrt(var + 1e-5)) < 1e-15
    dz, dgamma, dbeta, dbias = ref.bwd(np.ones((2, 4)), z, mean, rstd, gamma, beta, True)
    # pre == 0 gets no gradient: row 0 is out of columns 0, 1 and 3 (row 1 has pre < 0, > 0 and == 0 there), in of column 2
    assert dbeta.tolist() == [0, 1, 2, 0] and np.allclose(dbias, dz.sum(0))
    assert np.allclose(ref.kappa(z, 1e-5), [0, 6 / np.sqrt(var + 1e-5)])
    amb = ref.ambiguous(z, mean, rstd, gamma, beta, np.array([0.0, 0.1]))
    assert amb[0].tolist() == [True, True, False, True] and amb[1, 3]


def _emulated(layout, rfam, case, mutant=None, relu=True):
    """(forward ratio, mean ratio, rstd ratio, backward ratio, neutralised share) of the emulation to the bounds on one case"""
    m, n, vi, plant, eps, unit, seed = case
    z, dy, gamma, beta = lc.make_case(m, n, plant, seed, unit)
    r = lc.depth(rfam, n)
    eps32 = float(np.float32(eps))
    y_ref, pre_ref, mean_ref, rstd_ref = ref.fwd(z, gamma, beta, eps32, relu)
    xhat = (z.astype(np.float64) - mean_ref[:, None]) * rstd_ref[:, None]
    fm = mutant if mutant in lc.FWD_MUTANTS else None
    y, mean, rstd = lc.emulate_fwd(z, gamma, beta, eps, relu, layout, fm)
    rf = _ratio(np.abs(y - y_ref), lc.fwd_bound(r, z, gamma, eps32, xhat, y_ref))
    rm = _ratio(np.abs(mean - mean_ref), lc.mean_bound(r, z))
    rr = _ratio(np.abs(rstd / rstd_ref - 1), lc.rstd_bound(r, z, eps32))
    # backward on the FAITHFUL forward's stats, the ambiguous elements neutralised
    _, mean0, rstd0 = lc.emulate_fwd(z, gamma, beta, eps, relu, layout)
    amb = ref.ambiguous(z, mean0, rstd0, gamma, beta, lc.band(r, z, gamma, beta, eps32))
    dyn, share = lc.neutralise(dy, amb, z)
    bm = mutant if mutant in lc.BWD_MUTANTS else None
    dz = lc.emulate_bwd(dyn, z, mean0, rstd0, gamma, beta, relu, layout, bm)
    dz_ref = ref.bwd(dyn, z, mean0, rstd0, gamma, beta, relu)[0]
    rb = _ratio(np.abs(dz - dz_ref), lc.bwd_bound(r, dyn, rstd0, gamma)[:, None])
    return rf, rm, rr, rb, share


def test_faithful_emulation_stays_within_the_bounds_on_every_gpu_case():
    worst = {}
    for fam, layout, rfam, case in _all_cases():
        for relu in (True, False):
            rf, rm, rr, rb, share = _emulated(layout, rfam, case, relu=relu)
            w = worst.setdefault(fam, [0.0] * 5)
            worst[fam] = [max(a, b) for a, b in zip(w, (rf, rm, rr, rb, share))]
            assert max(rf, rm, rr, rb) <= 1.0, (fam, case, relu, rf, rm, rr, rb)
            assert share <= lc.AMBIGUOUS_CAP, (fam, case, share)
    for fam, (rf, rm, rr, rb, share) in worst.items():
        print(f"faithful emulation, {fam}: worst ratio to the bound  y {rf:.3f}  mean {rm:.3f}  rstd {rr:.3f}  dz {rb:.3f};  "
              f"largest neutralised share {100 * share:.3f} %")


@pytest.mark.parametrize("mutant", ["onepass", "padded4", "padded16", "nm1", "eps_outside", "mask_xhat", "no_c2"])
def test_every_mutant_breaks_a_bound_by_ten_times(mutant):
    worst, where = 0.0, None
    for fam, layout, rfam, case in _all_cases():
        n = case[1]
        if (mutant == "padded4" and n % 4 == 0) or (mutant == "padded16" and n % 16 == 0) or (mutant == "nm1" and n == 1):
            continue
        rf, _, _, rb, _ = _emulated(layout, rfam, case, mutant)
        if max(rf, rb) > worst:
            worst, where = max(rf, rb), (fam,) + tuple(case[:3]) + (case[4],)
        if worst == np.inf:
            break
    print(f"mutant {mutant}: worst ratio to the bound {worst:.3e} at (family, M, n, variant, eps) = {where}")
    assert worst >= 10.0
