"""The machinery of tests/stepcheck.py on the CPU: the float64 oracle with given ReLU masks, the host's copy of the backward's mask
formula, and the power of the row-localised probe comparison (each one-row corruption of the reference is rejected)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gcnsage_cpu as oc
from tests import stepcheck as sc


def _case(f0=63, hid=96, n=600, seed=0):
    rng = np.random.default_rng(seed)
    e = 6 * n
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    w = rng.uniform(0, 1, e).astype(np.float32)
    x = rng.standard_normal((n, f0)).astype(np.float32)
    y = rng.integers(0, 9, n)
    state = oc.init_state(f0, hid, 9, 3, seed=seed)
    state["layers.0.lynorm.weight"] = torch.from_numpy(rng.uniform(0.5, 1.5, hid).astype(np.float32))
    state["layers.1.lynorm.bias"] = torch.from_numpy(rng.uniform(-0.2, 0.2, hid).astype(np.float32))
    return oc.OracleGraph(src, dst, n, w), x, y, state


def test_fp64_oracle_given_its_own_relu_masks_is_the_unmasked_fp64_oracle_exactly():
    og, x, y, state = _case()
    cw = torch.rand(9, generator=torch.Generator().manual_seed(1)) + 0.5
    s64 = {k: v.double() for k, v in state.items()}
    _, hidden = oc.gcnsage_forward(s64, og, torch.from_numpy(x).double(), return_hidden=True)
    masks = [(h > 0).numpy() for h in hidden[:-1]]
    assert 0.2 < masks[0].mean() < 0.8
    plain = sc.reference_step(state, og, x, y, None, cw)
    masked = sc.reference_step(state, og, x, y, masks, cw)
    assert plain["loss"] == masked["loss"]
    assert np.array_equal(plain["logits"], masked["logits"])
    for k in plain["grads"]:
        assert np.array_equal(plain["grads"][k], masked["grads"][k]), k
        assert np.array_equal(plain["state"][k], masked["state"][k]), k


def test_oracle_default_is_unchanged_by_the_mask_argument():
    og, x, y, state = _case(n=300)
    a = oc.OracleTrainer(state)
    b = oc.OracleTrainer(state)
    la, ga = a.step(og, torch.from_numpy(x), torch.from_numpy(y))
    lb, gb = b.step(og, torch.from_numpy(x), torch.from_numpy(y), masks=None)
    assert la == lb and torch.equal(ga, gb) and all(torch.equal(a.grads()[k], b.grads()[k]) for k in a.grads())


def test_host_mask_formula_is_relus_decision_except_within_one_ulp_of_zero():
    """host_relu_mask (the backward's fmaf decision) against torch.relu on fp32 LayerNorm outputs computed as xh * gamma + beta
    (two roundings): they may differ only where the exact xh * gamma + beta lies within one ulp (of the product) of zero.
    Near-ties are planted on purpose (beta = -fp32(xh * gamma))."""
    rng = np.random.default_rng(7)
    n, f = 4000, 96
    z = (rng.standard_normal((n, f)) * rng.uniform(0.1, 10, (n, 1))).astype(np.float32)
    mean = z.mean(1, dtype=np.float32)
    rstd = (1.0 / np.sqrt(z.var(1, dtype=np.float32) + np.float32(1e-5))).astype(np.float32)
    gamma = rng.uniform(0.3, 1.7, f).astype(np.float32)
    xh = (z - mean[:, None]) * rstd[:, None]
    beta = rng.uniform(-0.3, 0.3, f).astype(np.float32)
    keep = sc.host_relu_mask(z, mean, rstd, gamma, beta)
    y = torch.from_numpy(xh) * torch.from_numpy(gamma) + torch.from_numpy(beta)
    relu_keep = (torch.relu(y) > 0).numpy()
    exact = xh.astype(np.float64) * gamma.astype(np.float64) + beta.astype(np.float64)
    ulp = np.spacing(np.abs((xh * gamma).astype(np.float32)))
    assert np.array_equal(keep, exact > 0)
    assert (keep == relu_keep)[np.abs(exact) > ulp].all()
    # planted ties: row 0's beta cancels the rounded product -> torch gets 0 (dropped), the fma keeps the product's rounding error
    b0 = -(xh[0] * gamma).astype(np.float32)
    k0 = sc.host_relu_mask(z[:1], mean[:1], rstd[:1], gamma, b0)[0]
    e0 = xh[0].astype(np.float64) * gamma + b0.astype(np.float64)
    r0 = (torch.relu(torch.from_numpy(xh[:1]) * torch.from_numpy(gamma) + torch.from_numpy(b0)) > 0).numpy()[0]
    assert np.array_equal(k0, e0 > 0) and not r0.any() and k0.any()          # the branch exists, and the host takes the fma's side
    assert (np.abs(e0[k0 != r0]) <= np.spacing(np.abs((xh[0] * gamma).astype(np.float32)))[k0 != r0]).all()


def test_probe_pages_place_their_probes_and_weights():
    m, tile = 2000, sc.one_round_tile(2000, 16)
    assert tile == 128 and sc.one_round_tile(8192, 256) == 32 and sc.one_round_tile(8193, 256) == 64
    assert sc.one_round_tile(24576, 256) == 96 and sc.one_round_tile(24577, 256) == 128
    pages, probes, off = sc.probe_pages(63, m, tile)
    from gnn_tableextraction_amd.data import synthetic as S
    src, dst, w, feat, label, off2 = S.concat_pages(pages)
    assert int(off2[-1]) == m and np.array_equal(off, off2)
    assert np.array_equal(np.nonzero(label == 0)[0], np.asarray(probes))
    deg = np.bincount(dst, minlength=m)
    assert {0, m - 1, tile - 1, tile}.issubset(probes)
    assert (deg[probes] == 0).any() and deg[probes].max() >= 300
    assert any(r in off[1:-1] and r - 1 in probes for r in probes)


@pytest.fixture(scope="module")
def probe_case():
    """A probe batch of one of the GPU probe shapes, (831, 256), with 3 000 nodes; the clean fp64 reference and an fp32 run of the
    same masked oracle (a stand-in for the device: honest fp32 rounding)."""
    f0, hid, m = 831, 256, 3000
    tile = sc.one_round_tile(m, 16)
    pages, probes, off = sc.probe_pages(f0, m, tile, seed=1)
    from gnn_tableextraction_amd.data import synthetic as S
    src, dst, w, feat, label, _ = S.concat_pages(pages)
    og = oc.OracleGraph(src, dst, m, w)
    torch.manual_seed(0)
    state = oc.init_state(f0, hid, 9, 3, seed=3)
    s64 = {k: v.double() for k, v in state.items()}
    _, hidden = oc.gcnsage_forward(s64, og, torch.from_numpy(feat).double(), return_hidden=True)
    masks = [(h > 0).numpy() for h in hidden[:-1]]
    cw = sc.probe_class_weights()
    ref = sc.reference_step(state, og, feat, label, masks, cw)
    f32 = sc.reference_step(state, og, feat, label, masks, cw, dtype=torch.float32)
    return dict(state=state, og=og, feat=feat, label=label, masks=masks, cw=cw, ref=ref, f32=f32, probes=probes)


def test_probe_comparison_passes_an_honest_fp32_step(probe_case):
    c = probe_case
    errs = sc.assert_grads(c["f32"]["grads"], c["ref"]["grads"])
    assert max(errs.values()) < 0.5, errs
    assert sc.loss_error(c["f32"]["loss"], c["ref"]["loss"]) < 1


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("kind", ["dz_scale", "stats_swap", "dz_zero"])
def test_probe_comparison_rejects_a_reference_corrupted_in_one_probe_row(probe_case, kind, layer):
    """One probe row (the first row of the second row tile) corrupted in one hidden layer: the fp32 run must fail the comparison
    against that reference by at least 3x the tolerance -- the probes keep their power if the tolerance is loosened a little."""
    c = probe_case
    row = sorted(c["probes"])[3]
    bad = sc.reference_step(c["state"], c["og"], c["feat"], c["label"], c["masks"], c["cw"],
                            layer_norm=sc.corrupted_layer_norm(kind, layer, row))
    errs = sc.grad_errors(c["f32"]["grads"], bad["grads"])
    worst = max(max(errs.values()), sc.loss_error(c["f32"]["loss"], bad["loss"]))
    assert worst >= 3.0, f"{kind} at layer {layer}, row {row}: rejected by only {worst:.2f} x the tolerance ({errs})"
    with pytest.raises(AssertionError):
        sc.assert_grads(c["f32"]["grads"], bad["grads"])
