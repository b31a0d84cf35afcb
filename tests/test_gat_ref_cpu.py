"""tests/gat_ref.py is not self-certified: its float64 forward and hand-derived backward against torch float64 autograd of the
dense formulation (per destination row: softmax over its in-edges, as in test_oracle_gat_layer_matches_dense_fp64, extended
with ELU and the head mean), the designed graph and the logit regimes against the properties tests/test_gpu_gat_kernels.py
relies on, and the float32 yardstick against the float64 reference.  CPU only."""
import numpy as np
import pytest
import torch

from tests import gat_ref as R

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def graphs():
    return {(n, o): R.designed_graph(n, o) for n in (333, 203) for o in ("rising", "first")}       # hubs of 3 000


def _dense_autograd(g, zg, zf, a_l, a_r, bias, mean_bias, H, dout, elu, mean_heads):
    """torch float64; zg enters the aggregation with identity gradient onto z (the straight-through form of oracle/gat_cpu.py)"""
    n = g.n
    z = torch.from_numpy(zf).double().requires_grad_(True)
    al, ar = (torch.from_numpy(a).double().requires_grad_(True) for a in (a_l, a_r))
    b = torch.from_numpy(bias).double().requires_grad_(True)
    z3 = z.view(n, H, -1)
    D = z3.shape[2]
    zgat = z3 + (torch.from_numpy(zg).double().view(n, H, D) - z3).detach()
    el, er = (z3 * al.view(H, D)).sum(-1), (z3 * ar.view(H, D)).sum(-1)
    el.retain_grad(); er.retain_grad()
    x = el[torch.from_numpy(g.indices)] + er[torch.from_numpy(g.edst)]
    x.retain_grad()
    rows = []
    for v in range(n):
        lo, hi = int(g.indptr[v]), int(g.indptr[v + 1])
        if hi == lo:
            rows.append(torch.zeros(H, D, dtype=torch.float64))
            continue
        a = torch.softmax(torch.nn.functional.leaky_relu(x[lo:hi], 0.2), 0)                  # [deg, H]
        rows.append((a[:, :, None] * zgat[torch.from_numpy(g.indices[lo:hi])]).sum(0))       # duplicate edges count twice
    out = torch.stack(rows).reshape(n, H * D) + b
    pre = out
    if elu:
        out = torch.nn.functional.elu(out)
    res = out
    if mean_heads:
        res = out.view(n, H, D).mean(1) + torch.from_numpy(mean_bias).double()
    (res * torch.from_numpy(dout).double()).sum().backward()
    return dict(out=out.detach().numpy(), pre=pre.detach().numpy(), res=res.detach().numpy(), ds=x.grad.numpy(), der=er.grad.numpy(),
                **{"del": el.grad.numpy()}, dz=z.grad.numpy(), da_l=al.grad.numpy(), da_r=ar.grad.numpy(), dbias=b.grad.numpy())


@pytest.mark.parametrize("elu,mean_heads,round_gather", [(False, False, False), (True, False, False), (False, True, False),
                                                         (True, True, False), (True, False, True)])
@pytest.mark.parametrize("regime", ["normal", "negative"])
def test_reference_matches_float64_autograd_of_the_dense_formulation(graphs, regime, elu, mean_heads, round_gather):
    g, info = graphs[(203, "rising")]
    H, D = 3, 5
    zf, a_l, a_r, bias = R.make_inputs(regime, g, info, H, D)
    zg = R.bf16_round(zf) if round_gather else zf
    rng = np.random.default_rng(5)
    mean_bias = rng.standard_normal(D).astype(np.float32)
    dout = rng.standard_normal((g.n, D if mean_heads else H * D)).astype(np.float32)
    want = _dense_autograd(g, zg, zf, a_l, a_r, bias, mean_bias, H, dout, elu, mean_heads)
    fw = R.forward(g, zg, zf, a_l, a_r, bias, H, elu=elu, mean_heads=mean_heads, mean_bias=mean_bias)
    bw = R.backward(g, fw, zg, zf, a_l, a_r, dout, act_out=fw["out"] if elu else None, mean_heads=mean_heads)
    tol = dict(rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(fw["out"], want["out"], **tol)
    np.testing.assert_allclose(fw["out_mean"] if mean_heads else fw["out"], want["res"], **tol)
    for k in ("ds", "der", "del", "dz", "da_l", "da_r", "dbias"):
        np.testing.assert_allclose(bw[k], want[k].reshape(bw[k].shape), err_msg=k, **tol)
    b64 = bias.astype(np.float64)
    for v in (info["degree_node"][0], info["isolated"]):                  # no in-edge: bias only, and nothing flows to er
        assert np.array_equal(fw["pre"][v], b64) and not bw["der"][v].any()
    for v in (info["sink"], info["isolated"]):                            # no out-edge: del = 0, dz = der a_r
        assert not bw["del"][v].any()
        np.testing.assert_allclose(bw["dz"][v], (bw["der"][v][:, None] * a_r.reshape(H, D).astype(np.float64)).reshape(-1), **tol)
    if regime == "negative":                                              # the derivative AT zero is the slope
        zero = fw["x"] == 0
        assert zero.sum() >= 4 * H and (fw["x"] <= 0).all()
    assert (fw["mag_out"] >= np.abs(fw["pre"]) - 1e-12).all() and (bw["mag_dz"] >= np.abs(bw["dz"]) - 1e-12).all()


@pytest.mark.parametrize("n", [333, 203])
def test_designed_graph_has_the_degrees_and_nodes_the_kernel_tests_rely_on(graphs, n):
    g, info = graphs[(n, "rising")]
    g2, _ = graphs[(n, "first")]
    assert n % 8 and n % 256 and g.indices.size <= 6500
    assert set(R.DEGREES) <= set(g.deg.tolist())
    for d, v in info["degree_node"].items():
        assert g.deg[v] == d
    hub = info["hub"]
    assert g.deg[hub] == R.HUB_DEGREE == 3000 and hub in g.indices[g.indptr[hub]:g.indptr[hub + 1]]
    assert (g.src == g.dst).sum() >= 5                                    # self-loops
    pairs = np.stack([g.src, g.dst], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                     # duplicated edges
    assert info["sink"] not in g.src and g.deg[info["sink"]] > 0
    assert info["isolated"] not in g.src and g.deg[info["isolated"]] == 0
    assert np.array_equal(g.deg, g2.deg)                                  # the two orderings: the same multigraph
    assert np.array_equal(np.sort(g.indices[g.indptr[hub]:g.indptr[hub + 1]]), np.sort(g2.indices[g2.indptr[hub]:g2.indptr[hub + 1]]))
    # pos_in really maps the out-CSR onto the in-CSR
    assert np.array_equal(g.indices[g.pos_in], np.repeat(np.arange(n), np.diff(g.rindptr)))
    assert np.array_equal(g.edst[g.pos_in], g.rindices)


@pytest.mark.parametrize("H,D", [(1, 1), (3, 7), (4, 64), (8, 32), (1, 1000)])
@pytest.mark.parametrize("n", [333, 203])
def test_wide_inputs_spread_the_logits_without_overflow(n, H, D):
    for regime in ("wide-rising", "wide-first"):
        order = R.REGIMES[regime][1]
        g, info, zf, a_l, a_r, bias = R.regime_inputs(n, regime, H, D)
        fw32, _ = R.plain_f32(g, zf, zf, a_l, a_r, bias, H)
        fw = R.forward(g, zf, zf, a_l, a_r, bias, H)
        for f in (fw, fw32):
            assert np.abs(f["s"]).max() <= 80.0
            assert np.isfinite(f["ssum"]).all() and (f["ssum"][g.deg > 0] >= 1.0).all()
        rows = [info["hub"]] + [info["degree_node"][d] for d in R.DEGREES if d >= 17]
        for v in rows:
            s = fw["s"][g.indptr[v]:g.indptr[v + 1]]
            spread = s.max(0) - s.min(0)
            assert (spread >= 40.0).all() and (spread <= 80.0).all(), (v, spread)
        hub = info["hub"]
        for h in range(H):
            for f in (fw, fw32):                                          # also at the float32 rounding of the scores
                rises = R.chunk_rises(f["s"][g.indptr[hub]:g.indptr[hub + 1], h])
                assert len(rises) == -(-g.deg[hub] // 16) >= 63
                assert all(rises) if order == "rising" else (rises[0] and not any(rises[1:]))


CASES = [(1, 1), (1, 16), (2, 16), (3, 7), (4, 16), (4, 18), (4, 32), (4, 36), (4, 64), (2, 17), (2, 33), (5, 13), (8, 8), (8, 32),
         (3, 100), (4, 128), (8, 64), (8, 128), (1, 1000)]


@pytest.mark.parametrize("H,D", CASES)
def test_float32_yardstick_stays_near_the_float64_reference(H, D):
    """64 * 2^-24 of the element's magnitude, forward and backward, every regime and both orderings; the kernel tests use the
    same inputs (bf16 gathers included where they are tested)."""
    worst = {}
    for regime, n in [(r, 333) for r in R.REGIMES] + [("normal", 203), ("wide-rising", 203)]:
        g, info, zf, a_l, a_r, bias = R.regime_inputs(n, regime, H, D)
        dout = np.random.default_rng(9).standard_normal((g.n, H * D)).astype(np.float32)
        for zg in [zf] + ([R.bf16_round(zf)] if (H, D) in ((4, 64), (4, 18), (3, 7), (8, 64)) and regime != "flat" else []):
            fw32, bw32 = R.plain_f32(g, zg, zf, a_l, a_r, bias, H, dout=dout)
            free = R.forward(g, zg, zf, a_l, a_r, bias, H)
            # the aggregation is compared at ONE set of scores, as on the device (the kernels are fed the device's own el / er)
            fw = R.forward(g, zg, zf, a_l, a_r, bias, H, el=fw32["el"], er=fw32["er"])
            bw = R.backward(g, fw, zg, zf, a_l, a_r, dout)
            pairs = [("el", free, fw32, "mag_el"), ("er", free, fw32, "mag_er"), ("out", fw, fw32, "mag_out"), ("ssum", fw, fw32, "ssum")]
            pairs += [(k, bw, bw32, "mag_" + k) for k in ("ds", "der", "del", "dz", "da_l", "da_r", "dbias")]
            for k, a, b, mag in pairs:
                worst[k] = max(worst.get(k, 0.0), R.ratio(b[k], a[k], a[mag]))
    print(f"\nplain_f32 vs float64, H={H} D={D}: " + " ".join(f"{k}={v / EPS:.1f}eps" for k, v in worst.items()), end="")
    for k, v in worst.items():
        assert v <= 64 * EPS, (k, v / EPS)
