"""The reference's OWN run shapes on the planes path (run_multiple_train.sh:8-113 of the reference: --h_layer_dim=1000, or
--mode_params=scaled --params_no=100000 -> int(calculate_hidden) = 218 / 206 / 157 / 149 / 100 / 96, with F0 = 13 ... 831).

* the general-width row kernels (padded rows, LayerNorm over the true width) against torch / the CPU oracle;
* the one-call plan (gte_gcnsage_step / gte_gcnsage_forward: transform-first planes layers of any width <= 1024, the
  aggregate-first input layer, the output layer on the planes GEMMs) against the reference-generated ``shape_*`` fixtures:
  logits 1e-5, loss 1e-5, gradients 1e-4, post-step parameters / logits per tests/poststep.py;
* the exact path ``bench.py`` times (ResidentPages.enable_p3 + BatchPipeline + run_steps, one 100-page step at F0 = 831,
  hidden 256) and ``forward_logits`` against the oracle directly.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import _lib, graph as G, ops
from gnn_tableextraction_amd.data import synthetic as S
from oracle import gcnsage_cpu as oc
from tests import poststep, stepcheck
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "shape_*.npz")))
WIDTHS = [5, 13, 96, 100, 139, 149, 157, 206, 218, 256, 300, 520, 1000, 1024]


def dev(a, dtype=None):
    t = torch.as_tensor(a)
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def c16(x):
    return -(-x // 16) * 16


def _graph(rng, n, deg=6):
    e = n * deg
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    dst[: n // 50 + 1] = 0                                            # a hub row; some rows stay empty
    w = rng.uniform(0, 1, e).astype(np.float32)
    return oc.OracleGraph(src, dst, n, w)


def _padded(a, ld):
    """device copy of ``a`` [n, f] in a zero buffer with ``ld`` floats per row (a view of the first f columns is returned too)"""
    buf = torch.zeros((a.shape[0], ld), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("relu", [True, False])
def test_aggregate_layernorm_kernel_on_any_width(f, relu):
    """gte_spmm_csr_accumulate_ln_p3 on padded rows: z = t_self + mean-aggregate(t_neigh) (the oracle's CSR SpMM, same order),
    LayerNorm over the f TRUE columns, ReLU; y as fp32 and as a P3 image; padding written as zeros."""
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(f)
    n = 777
    g = _graph(rng, n)
    ld = c16(f)
    t_self = rng.standard_normal((n, f)).astype(np.float32)
    t_neigh = rng.standard_normal((n, f)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, f).astype(np.float32), rng.standard_normal(f).astype(np.float32)
    t = torch.zeros((n, 2 * ld), dtype=torch.float32, device=DEV)
    t[:, :f], t[:, ld:ld + f] = dev(t_self), dev(t_neigh)
    y = torch.full((n, ld), 7.0, dtype=torch.float32, device=DEV)
    yp = ops.P3.empty(n, f, DEV)
    yp.data.fill_(0x55)
    stats = torch.zeros(2 * n, dtype=torch.float32, device=DEV)
    indptr, indices, w, dgam, dbet = dev(g.indptr), dev(g.indices), dev(g.weight), dev(gamma), dev(beta)
    _lib.check(lib.gte_spmm_csr_accumulate_ln_p3(P(indptr), P(indices), P(w), P(t) + 4 * ld, 2 * ld, P(t), 2 * ld, n, f, 1, P(dgam),
                                                 P(dbet), 1e-5, int(relu), P(y), ld, P(yp.data), yp.ldp, P(stats),
                                                 _lib.current_stream()), "accumulate_ln_p3")
    agg = oc.spmm_csr_numpy(g.indptr, g.indices, g.weight, t_neigh) * g.norm
    z = t_self + agg
    np.testing.assert_allclose(t[:, :f].cpu().numpy(), z, rtol=1e-6, atol=1e-6)
    zt = torch.from_numpy(z).double()
    want = torch.nn.functional.layer_norm(zt, (f,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), 1e-5)
    want = (want.relu() if relu else want).numpy()
    got = y.cpu().numpy()
    np.testing.assert_allclose(got[:, :f], want, rtol=1e-5, atol=1e-5)
    assert (got[:, f:] == 0).all()                                    # (with the image: the whole 16-column block is written)
    img = ops.p3_to_f32(ops.P3(yp.data, n, ld)).cpu().numpy()         # the whole padded image row
    np.testing.assert_array_equal(img[:, :f], got[:, :f])
    assert (img[:, f:] == 0).all()
    np.testing.assert_allclose(stats[:n].cpu().numpy(), z.mean(1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(stats[n:].cpu().numpy(), 1.0 / np.sqrt(z.astype(np.float64).var(1) + 1e-5), rtol=2e-5)


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("relu", [True, False])
def test_layernorm_forward_and_backward_kernels_on_any_width(f, relu):
    """gte_ln_relu_fwd_p3 and gte_ln_relu_bwd_p3 on padded rows against torch autograd in fp64."""
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(100 + f)
    m, ld = 531, c16(f)
    z = rng.standard_normal((m, f)).astype(np.float32) * 2 + 0.3
    dy = rng.standard_normal((m, f)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, f).astype(np.float32), rng.standard_normal(f).astype(np.float32) * 0.3
    zt = torch.from_numpy(z).double().requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    yt = torch.nn.functional.layer_norm(zt, (f,), gt, bt, 1e-5)
    yt = yt.relu() if relu else yt
    yt.backward(torch.from_numpy(dy).double())
    zb = _padded(z, ld)
    zb[:, f:] = 3.0                                                   # garbage in the padding of z must not matter
    y = torch.zeros((m, ld), dtype=torch.float32, device=DEV)
    yp = ops.P3.empty(m, f, DEV)
    yp.data.fill_(0x55)
    stats = torch.zeros(2 * m, dtype=torch.float32, device=DEV)
    dg, db = dev(gamma), dev(beta)
    _lib.check(lib.gte_ln_relu_fwd_p3(P(zb), ld, P(dg), P(db), 1e-5, int(relu), P(y), ld, P(yp.data), yp.ldp, P(stats), m, f,
                                      _lib.current_stream()), "ln_relu_fwd_p3")
    np.testing.assert_allclose(y[:, :f].cpu().numpy(), yt.detach().numpy(), rtol=1e-5, atol=1e-5)
    img = ops.p3_to_f32(ops.P3(yp.data, m, ld)).cpu().numpy()
    np.testing.assert_array_equal(img[:, :f], y[:, :f].cpu().numpy())
    assert (img[:, f:] == 0).all()
    # backward: dz in place of dy, as fp32 + image; column sums
    dyb = _padded(dy, ld)
    dyb[:, f:] = -2.0
    dzp = ops.P3.empty(m, f, DEV)
    dzp.data.fill_(0x55)
    dgam, dbet, dbias = (torch.zeros(f, dtype=torch.float32, device=DEV) for _ in range(3))
    ws = torch.empty(int(lib.gte_ln_relu_bwd_workspace_bytes(m, f)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.gte_ln_relu_bwd_p3(P(dyb), ld, P(zb), ld, P(stats), P(dg), P(db), int(relu), P(dyb), ld, P(dzp.data), dzp.ldp,
                                      P(dgam), P(dbet), P(dbias), m, f, P(ws), ws.numel(), _lib.current_stream()), "ln_relu_bwd_p3")
    want_dz = zt.grad.numpy()
    scale = np.abs(want_dz).max()
    np.testing.assert_allclose(dyb[:, :f].cpu().numpy(), want_dz, rtol=1e-4, atol=1e-5 * scale)
    img = ops.p3_to_f32(ops.P3(dzp.data, m, ld)).cpu().numpy()
    np.testing.assert_array_equal(img[:, :f], dyb[:, :f].cpu().numpy())
    assert (img[:, f:] == 0).all()
    np.testing.assert_allclose(dgam.cpu().numpy(), gt.grad.numpy(), rtol=1e-4, atol=1e-4 * np.abs(gt.grad.numpy()).max())
    np.testing.assert_allclose(dbet.cpu().numpy(), bt.grad.numpy(), rtol=1e-4, atol=1e-4 * np.abs(bt.grad.numpy()).max())
    np.testing.assert_allclose(dbias.cpu().numpy(), want_dz.sum(0), rtol=1e-4, atol=1e-4 * np.abs(want_dz).sum(0).max())


@pytest.mark.parametrize("f", [1, 3, 9, 13, 16, 63, 100, 218, 313, 363, 1000, 1100])
@pytest.mark.parametrize("mean", [False, True])
def test_aggregation_into_an_image_is_bitwise_the_fp32_aggregation(f, mean):
    """gte_spmm_csr_p3 for any width: the image holds exactly the values gte_spmm_csr writes, zeros up to the 16-column block."""
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(200 + f)
    n = 1234
    g = _graph(rng, n)
    x = dev(rng.standard_normal((n, f)).astype(np.float32))
    indptr, indices, w = dev(g.indptr), dev(g.indices), dev(g.weight)
    out = torch.empty((n, f), dtype=torch.float32, device=DEV)
    _lib.check(lib.gte_spmm_csr(P(indptr), P(indices), P(w), P(x), f, P(out), f, n, f, 0, int(mean), _lib.current_stream()), "spmm")
    img = ops.P3.empty(n, f, DEV)
    img.data.fill_(0x55)
    _lib.check(lib.gte_spmm_csr_p3(P(indptr), P(indices), P(w), P(x), f, P(img.data), img.ldp, n, f, int(mean), _lib.current_stream()),
               "spmm_p3")
    got = ops.p3_to_f32(ops.P3(img.data, n, c16(f)))
    assert torch.equal(got[:, :f], out) and bool((got[:, f:] == 0).all())


def test_colsum_is_deterministic_and_exact_on_integers():
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(5)
    for m, c, ld in ((1, 9, 32), (1000, 9, 32), (24437, 16, 16), (70000, 1, 5)):
        x = torch.zeros((m, ld), dtype=torch.float32, device=DEV)
        vals = rng.integers(-8, 9, (m, c)).astype(np.float32)
        x[:, :c] = dev(vals)
        out = torch.full((c,), 99.0, dtype=torch.float32, device=DEV)
        ws = torch.empty(int(lib.gte_colsum_workspace_bytes(m, c)), dtype=torch.uint8, device=DEV)
        _lib.check(lib.gte_colsum(P(x), ld, m, c, P(out), P(ws), ws.numel(), _lib.current_stream()), "colsum")
        np.testing.assert_array_equal(out.cpu().numpy(), vals.sum(0))
    assert lib.gte_colsum(None, 4, 10, 4, None, None, 0, None) == -1


# ---------------------------------------------------------------- whole model on the reference's run shapes
@pytest.fixture(params=["split_bf16", "f32"])
def both_gemm_modes(request):
    prev = ops.set_gemm_mode(request.param)
    try:
        yield request.param
    finally:
        ops.set_gemm_mode(prev)


def _case_graph(src, dst, w, x):
    g = G.PageGraph(src, dst, len(x), device=DEV)
    g.ndata["feat"], g.edata["feat"] = dev(x), dev(w)
    return g


@pytest.mark.parametrize("name", SHAPE_CASES)
def test_run_shape_step_matches_reference_golden(name, both_gemm_modes):
    """One optimisation step of the step engine (in the default GEMM mode: the one-call plan on the planes kernels -- asserted)
    on a shape the reference's runs use, against the fixture generated from the reference's models.py."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    z, src, dst, w, x, y, state0, model = poststep.trimmed_case(GOLDEN_DIR, name)
    n, f0, hid = (int(v) for v in z["meta"][:3])
    model = model.to(DEV)
    g = _case_graph(src, dst, w, x)
    fused = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
    on_plan = fused._planes_on()
    if on_plan:
        kinds = fused._plan_kinds(f0, n)
        assert kinds is not None, "every run shape of the reference is on the one-call plan"
        gen, out_gemm = fused._plan_mode(kinds, f0)
        assert kinds[1:] == [0] * (len(kinds) - 1) and kinds[0] == (0 if 4 * hid <= 5 * f0 else 2)
        assert out_gemm == (hid > 256)       # (widths that are not a multiple of 8: the narrow kernels on padded rows, round 5)
    logits = fused.forward_logits(g).cpu().numpy()                  # gte_gcnsage_forward on the plan (module path in fp32 mode)
    np.testing.assert_allclose(logits, z["logits"], rtol=1e-5, atol=1e-5)
    out3 = fused.step(g, dev(y).float())
    if on_plan:
        ran = fused.plan_buffers(g)
        assert ran is not None and ran[0].get("_plans") and (ran[1], ran[2]) == (kinds, out_gemm), "the step ran on the one-call plan"
    grads = {k: fused._gslice[id(p)].cpu().numpy() for k, p in model.named_parameters()}
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    after = fused.forward_logits(g).cpu().numpy()
    og = oc.OracleGraph(src, dst, len(x), w)
    ref_after = oc.gcnsage_forward({k: torch.from_numpy(v) for k, v in params.items()}, og, torch.from_numpy(x)).numpy()
    poststep.check_headline(z, logits, [], float(out3[0]), grads, params, after, state0, oracle_after=ref_after)
    assert int(out3[2]) == int((z["logits"].argmax(1) == y).sum())


@pytest.mark.parametrize("name", ["shape_f13_h218", "shape_f363_h149", "shape_f63_h1000"])
def test_run_shape_module_forward_matches_reference_golden(name, both_gemm_modes):
    """``model(g)`` (autograd path) on the same shapes: logits and hidden activations at the north_star tolerance."""
    z, src, dst, w, x, y, state0, model = poststep.trimmed_case(GOLDEN_DIR, name)
    model = model.to(DEV)
    g = _case_graph(src, dst, w, x)
    hidden = []
    hooks = [l.register_forward_hook(lambda m, i, o: hidden.append(o.detach().cpu().numpy())) for l in model.layers]
    with torch.no_grad():
        logits = model(g).cpu().numpy()
    for h in hooks:
        h.remove()
    np.testing.assert_allclose(logits, z["logits"], rtol=1e-5, atol=1e-5)
    for i, h in enumerate(hidden[:2]):
        np.testing.assert_allclose(h[::16], z[f"hidden_rows16.{i}"], rtol=1e-5, atol=2e-5)


def _resident(pages, tr, f0):
    graphs = []
    for p in pages:
        g = gte.PageGraph(p.src, p.dst, p.num_nodes)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
        g.edata["feat"] = torch.from_numpy(p.weight)
        graphs.append(g)
    return G.ResidentPages(graphs, DEV)


@pytest.mark.parametrize("f0,hid,image_mode", [(831, 256, True), (13, 218, True), (831, 256, False)])
def test_batches_assembled_in_stream_order_train_bitwise_as_on_the_side_stream(f0, hid, image_mode, monkeypatch):
    """BatchPipeline assembles a row-map batch in the caller's stream order (no events) and a batch that copies fp32 rows on its side
    stream under the step before; either placement forced (side_stream=False / True) over several load()s of different lengths --
    metadata uploads in between, both buffer sets reused -- must train bit for bit the same parameters."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    if not image_mode:
        monkeypatch.setenv("GTE_PLANES", "0")            # fp32 feature rows: the batches copy them
    pages = S.make_pages(60, in_feats=f0)
    rng = np.random.default_rng(3)
    chunks = [[rng.permutation(60)[:k] for k in ks] for ks in ([9, 14, 5], [20], [7, 7, 7, 11], [3, 25])]
    results = []
    for side in (True, False, None):
        torch.manual_seed(11)
        model = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0).to(DEV)
        fused = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
        pipe = BatchPipeline(_resident(pages, fused, f0), side_stream=side)
        losses = []
        for chunk in chunks:
            out3 = run_steps(fused, pipe, chunk)
            losses.append(out3.clone())
        torch.cuda.synchronize()
        assert pipe._same == ((not side) if side is not None else (pipe.res.p3_mode == "rows"))
        results.append((torch.stack(losses).cpu(), torch.cat([p.detach().flatten() for p in model.parameters()]).cpu()))
    for got in results[1:]:
        assert torch.equal(got[0], results[0][0]) and torch.equal(got[1], results[0][1])


@pytest.mark.parametrize("f0,hid", [(831, 256), (831, 96), (63, 206), (13, 218), (363, 149)])
def test_the_kernel_timer_schedule_runs_on_the_loops_image_batches(f0, hid):
    """bench.py's per-kernel HIP-event pass (ops.enable_kernel_timers) switches the engine to its launch-by-launch schedule on
    the SAME resident pages -- which, in image mode, hand over batches without fp32 rows, and with the aggregate image the
    one-call plan wanted.  That schedule takes layer 0 as planes for fewer shapes than the plan: it must convert such a batch
    back (exactly) instead of reading a feature tensor that is not there, and reach the one-call step's loss."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    pages = S.make_pages(30, in_feats=f0)
    ids = [np.arange(0, 14), np.arange(14, 30)]
    losses = []
    for timers in (False, True):
        torch.manual_seed(7)
        model = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0).to(DEV)
        fused = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
        pipe = BatchPipeline(_resident(pages, fused, f0))
        run_steps(fused, pipe, ids[:1])                  # the one-call plan sets the resident pages up (image mode where it wants it)
        ops.enable_kernel_timers(timers)
        try:
            out3 = run_steps(fused, pipe, ids[1:])
            torch.cuda.synchronize()
            if timers:
                assert ops.kernel_timer_report()
        finally:
            ops.enable_kernel_timers(False)
        losses.append(float(out3[0]))
    assert np.isfinite(losses).all() and abs(losses[0] - losses[1]) < 2e-5, losses


@pytest.mark.parametrize("cached", [True, False], ids=["cached_agg", "no_cache"])
@pytest.mark.parametrize("f0,hid,n_pages", [(831, 256, 100), (831, 96, 40), (63, 1000, 16), (13, 218, 40), (831, 1000, 12), (781, 100, 40),
                                            (313, 157, 40), (63, 206, 40), (363, 1000, 12)])
def test_the_loop_bench_times_matches_the_oracle_step(f0, hid, n_pages, cached):
    """The path ``bench.py`` and ``train()`` run -- ResidentPages (features as a P3 image + row map where layer 0 takes one),
    BatchPipeline, run_steps, the one-call step with Adam in the fold launch -- for ONE step on n_pages pages against the CPU
    oracle's step on the same pages: logits 1e-5 (forward_logits on the assembled batch), loss 1e-5, every gradient 1e-4,
    parameters / post-step logits per tests/poststep.py.  (831, 256, 100 pages) is the headline configuration at full size.
    The step's reference is the float64 oracle run on the ReLU masks the device's backward used (tests/stepcheck.py): a LayerNorm
    output within rounding of zero has no branch left to disagree on, so every case is checked at the full strength."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    pages = S.make_pages(n_pages + 7, in_feats=f0)
    ids = np.arange(3, 3 + n_pages)
    src, dst, w, feat, label, off = S.concat_pages([pages[i] for i in ids])
    n = int(off[-1])
    torch.manual_seed(42)
    model = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0)
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    og = oc.OracleGraph(src, dst, n, w)
    xt, yt = torch.from_numpy(feat), torch.from_numpy(label)
    want_logits = oc.gcnsage_forward(state0, og, xt).numpy()

    model = model.to(DEV)
    fused = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
    assert fused._plan_kinds(f0, n) is not None
    res = _resident(pages, fused, f0)
    pipe = BatchPipeline(res)
    seen = {}

    def on_step(s, g, out3):
        seen["n"] = g.num_nodes()
    # forward only, on the batch the pipeline assembles (row-map batch in image mode)
    # ``cached``: layer 0 on the resident image of the input's mean aggregate (GTE_LAYER_CACHED: what run_steps sets up by
    # default); False: the image is not built, layer 0 aggregates in the step
    fused.cache_input_agg = cached
    if cached and not fused.wants_agg_image(f0):
        pytest.skip("layer 0 of this shape does not run on the cached aggregate (short input, or a hidden width below 128)")
    if fused.wants_resident_images(f0) if cached else fused.wants_p3_features(f0):
        res.enable_p3(agg=cached)
        assert res.p3_mode == "rows" and (res.agg_p3 is not None) == cached
        b0 = res.batch(ids)
        assert fused._plan_kinds(f0, n, fused._batch_cached(b0))[0] == (3 if cached else 0)
    logits = fused.forward_logits(res.batch(ids)).cpu().numpy()
    np.testing.assert_allclose(logits, want_logits, rtol=1e-5, atol=1e-5)
    out3 = run_steps(fused, pipe, [ids], on_step=on_step)
    torch.cuda.synchronize()
    assert seen["n"] == n and fused.adam_fused_steps == 1
    masks = stepcheck.device_relu_masks(fused, res.batch(ids), state0)      # (read before forward_logits reuses the buffers)
    ref = stepcheck.reference_step(state0, og, feat, label, masks, lr=0.01, weight_decay=5e-4)
    assert abs(float(out3[0]) - ref["loss"]) < 1e-5
    grads = {k: fused._gslice[id(p)].cpu().numpy() for k, p in model.named_parameters()}
    stepcheck.assert_grads(grads, ref["grads"], rel=1e-4)
    for k, g in grads.items():
        np.testing.assert_allclose(g, ref["grads"][k], rtol=1e-4, atol=1e-6 + 1e-4 * np.abs(ref["grads"][k]).max(), err_msg=k)
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    after = fused.forward_logits(res.batch(ids)).cpu().numpy()
    stepcheck.check_poststep(ref, params, state0, og, feat, after, atol=1e-4)


@pytest.mark.parametrize("mode", ["split_bf16", "f32"])
@pytest.mark.parametrize("f0,hid", [(831, 256), (13, 218)])
def test_the_loop_follows_the_oracle_over_eight_steps(f0, hid, mode):
    """A TRAJECTORY of the loop ``train()`` and ``bench.py`` run (reference model_train.py:283-340: forward, CE, backward, Adam, next
    batch) against the CPU oracle: eight consecutive DIFFERENT 40-page batches through ONE ``run_steps`` call with the default
    switches -- resident images + row maps, cached input aggregate where the plan takes it, the next batch assembled inside the fold
    launch, Adam (t = 1 ... 8) and the next step's weight images written by the fold launch -- against eight ``OracleTrainer.step``
    calls on the same batches.  The loss of every step within 1e-4 of the oracle's, the logits of a held-out batch after the eight
    steps within 1e-3 (every single-step test starts from equal parameters; here steps 2 ... 8 start from the loop's OWN state)."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    prev = ops.set_gemm_mode(mode)
    try:
        n_steps, per = 8, 40
        pages = S.make_pages(n_steps * per + per, in_feats=f0)
        rng = np.random.default_rng(5)
        order = rng.permutation(n_steps * per)
        steps = [np.sort(order[i * per:(i + 1) * per]) for i in range(n_steps)]
        held = np.arange(n_steps * per, n_steps * per + per)
        torch.manual_seed(42)
        model = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0)
        state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        tr_o = oc.OracleTrainer(state0, lr=0.01, weight_decay=5e-4)
        want = []
        for ids in steps:
            src, dst, w, feat, label, off = S.concat_pages([pages[i] for i in ids])
            loss, _ = tr_o.step(oc.OracleGraph(src, dst, int(off[-1]), w), torch.from_numpy(feat), torch.from_numpy(label))
            want.append(loss)
        src, dst, w, feat, label, off = S.concat_pages([pages[i] for i in held])
        want_held = oc.gcnsage_forward({k: v.detach() for k, v in tr_o.state.items()}, oc.OracleGraph(src, dst, int(off[-1]), w),
                                       torch.from_numpy(feat)).numpy()

        model = model.to(DEV)
        fused = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
        res = _resident(pages, fused, f0)
        pipe = BatchPipeline(res)
        got = []
        out3 = run_steps(fused, pipe, steps, on_step=lambda s, g, o: got.append(o.clone()))
        torch.cuda.synchronize()
        got = [float(o[0]) for o in got]
        assert len(got) == n_steps
        if mode == "split_bf16" and f0 == 831:
            assert res.p3_mode == "rows" and res.agg_p3 is not None and fused.adam_fused_steps == n_steps     # the default switches
        assert np.isfinite(got).all() and want[0] > want[-1]   # (it trains)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)
        after = fused.forward_logits(res.batch(held)).cpu().numpy()
        np.testing.assert_allclose(after, want_held, rtol=0, atol=1e-3)
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.parametrize("n,C", [(24437, 9), (300, 16), (1, 3), (257, 9)])
def test_head_dlq_finish_scales_images_and_sums(n, C):
    """gte_head_dlq_finish: out3 from the CE partials, alpha [dl | q] as one image [n][32], gbias = colsum(alpha dl) -- against the
    same quantities computed with torch from the unscaled inputs; inside and outside a fold deferral."""
    lib, P, st = _lib.load(), _lib.ptr, _lib.current_stream()
    g = torch.Generator(device=DEV).manual_seed(n + C)
    dlq = torch.full((n, 32), 3e30, device=DEV)                       # columns C .. 15 / 16 + C .. 31 hold no data
    dlq[:, :C] = torch.randn(n, C, device=DEV, generator=g)
    dlq[:, 16:16 + C] = torch.randn(n, C, device=DEV, generator=g)
    nb = -(-n // 64)
    part = torch.rand(nb, 3, device=DEV, generator=g) + 0.5           # {sum w nll, sum w, #correct} per 64-node block
    wsum = float(part[:, 1].double().sum())
    grad_scale = 0.37
    alpha = grad_scale / wsum
    want = torch.zeros(n, 32, device=DEV)
    want[:, :C] = dlq[:, :C] * np.float32(alpha)
    want[:, 16:16 + C] = dlq[:, 16:16 + C] * np.float32(alpha)
    ws = torch.empty(int(lib.gte_head_dlq_finish_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    for deferred in (False, True):
        img = ops.P3.empty(n, 32, DEV)
        img.data.fill_(0x55)
        out3, gb = torch.full((3,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)
        if deferred:
            _lib.check(lib.gte_fold_defer_begin(st), "begin")
        _lib.check(lib.gte_head_dlq_finish(None, None, None, P(dlq), 32, n, C, P(part), grad_scale, P(out3), P(img.data), img.ldp, P(gb),
                                           P(ws), ws.numel(), st), "gte_head_dlq_finish")
        if deferred:
            _lib.check(lib.gte_fold_defer_flush(), "flush")
        got = ops.p3_to_f32(img)
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=3e-7, atol=0)     # (alpha in fp32 on both sides)
        np.testing.assert_allclose(out3.cpu().numpy(), [float(part[:, 0].double().sum()) / wsum, wsum, float(part[:, 2].double().sum())],
                                   rtol=1e-6)
        np.testing.assert_allclose(gb.double().cpu().numpy(), want[:, :C].double().sum(0).cpu().numpy(), rtol=1e-5,
                                   atol=1e-6 * float(want[:, :C].abs().sum(0).max()) + 1e-12)
    assert lib.gte_head_dlq_finish(None, None, None, P(dlq), 32, n, 17, P(part), grad_scale, P(out3), P(img.data), img.ldp, P(gb), P(ws),
                                   ws.numel(), st) == -1
    # with the out-edge CSR the launch forms q = A_w^T dl itself: bit for bit the aggregation kernel's q, then scaled
    rng = np.random.default_rng(n)
    e = 6 * n
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    rip, rix, _, rw = ops.coo_to_csr(dev(src, torch.int32), dev(dst, torch.int32), n, dev(rng.random(e).astype(np.float32)))
    q = ops.spmm_csr(rip, rix, rw, dlq[:, :C].contiguous(), n, mean=False)
    img2 = ops.P3.empty(n, 32, DEV)
    _lib.check(lib.gte_head_dlq_finish(P(rip), P(rix), P(rw), P(dlq), 32, n, C, P(part), grad_scale, P(out3), P(img2.data), img2.ldp, P(gb),
                                       P(ws), ws.numel(), st), "gte_head_dlq_finish")
    got2 = ops.p3_to_f32(img2)
    assert torch.equal(got2[:, :C], got[:, :C])
    assert torch.equal(got2[:, 16:16 + C], q * np.float32(alpha)) or torch.allclose(got2[:, 16:16 + C], q * np.float32(alpha), rtol=3e-7, atol=0)


# ---------------------------------------------------------------- edge-parallel aggregation (hub rows)
def _hub_graph(rng, n, hubs, hub_deg, base_deg=5):
    src = [rng.integers(0, n, n * base_deg)]
    dst = [np.repeat(np.arange(n), base_deg)]
    for h in hubs:
        src.append(rng.integers(0, n, hub_deg))
        dst.append(np.full(hub_deg, h))
    src, dst = np.concatenate(src), np.concatenate(dst)
    dst[dst == n // 3] = 0                                           # a row without in-edges in the middle
    w = rng.uniform(0, 1, len(src)).astype(np.float32)
    return oc.OracleGraph(src, dst, n, w)


@pytest.mark.parametrize("f", [9, 13, 64, 256, 831, 1100])
@pytest.mark.parametrize("kind", ["hub3000", "powerlaw", "tiny"])
def test_edge_parallel_aggregation_matches_the_oracle_and_is_reproducible(f, kind):
    """gte_spmm_csr_edge (one wave per 64-edge segment, segmented by destination row, two-pass carry): oracle parity at 1e-5
    relative to the row's magnitude, bit-identical run to run, rows without edges zero; rows inside one segment bit-equal to the
    row kernel."""
    rng = np.random.default_rng(hash(kind) % 1000 + f)
    if kind == "hub3000":
        n = 5000
        g = _hub_graph(rng, n, hubs=[7, 2500, n - 1], hub_deg=3000)
    elif kind == "powerlaw":
        n = 20000
        deg = np.minimum((rng.pareto(1.2, n) * 3).astype(np.int64), 4000)
        dst = np.repeat(np.arange(n), deg)
        src = rng.integers(0, n, len(dst))
        g = oc.OracleGraph(src, dst, n, rng.uniform(0, 1, len(dst)).astype(np.float32))
    else:
        n = 3
        g = oc.OracleGraph(np.array([0, 1, 2, 2]), np.array([1, 1, 1, 0]), n, np.array([0.5, 1.0, 0.25, 2.0], np.float32))
    x = rng.standard_normal((n, f)).astype(np.float32)
    indptr, indices, w, xd = dev(g.indptr), dev(g.indices), dev(g.weight), dev(x)
    for mean in (False, True):
        a = ops.spmm_csr_edge(indptr, indices, w, xd, n, mean=mean)
        b = ops.spmm_csr_edge(indptr, indices, w, xd, n, mean=mean)
        assert torch.equal(a, b)
        want = oc.spmm_csr_numpy(g.indptr, g.indices, g.weight, x)
        mag = oc.spmm_csr_numpy(g.indptr, g.indices, g.weight, np.abs(x))
        if mean:
            want, mag = want * g.norm, mag * g.norm
        assert (np.abs(a.cpu().numpy() - want) <= 1e-5 * mag + 1e-7).all()
        row = ops.spmm_csr(indptr, indices, w, xd, n, mean=mean)
        deg = np.diff(g.indptr)
        inside = (g.indptr[:-1] // 64) == ((g.indptr[1:] - 1) // 64)          # rows whose edges lie in one 64-edge segment
        inside |= deg == 0
        assert torch.equal(a[torch.from_numpy(inside).to(DEV)], row[torch.from_numpy(inside).to(DEV)])
    # the module path picks it by the graph's largest row
    gg = G.PageGraph(g.indices[np.argsort(np.argsort(np.arange(len(g.indices))))], np.repeat(np.arange(n), np.diff(g.indptr)), n, device=DEV)
    assert gg.max_in_degree() == int(np.diff(g.indptr).max())


def test_edge_parallel_aggregation_of_a_graph_without_edges_zeroes_its_rows_only():
    n, f = 37, 20
    buf = torch.full((n, f + 5), 7.0, device=DEV)
    indptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    indices = torch.zeros(0, dtype=torch.int32, device=DEV)
    out = ops.spmm_csr_edge(indptr, indices, None, torch.randn(n, f, device=DEV), n, mean=True, out=buf[:, :f])
    assert float(out.abs().sum()) == 0.0 and bool((buf[:, f:] == 7.0).all())       # nothing written past the rows


def test_edge_parallel_aggregation_beats_the_row_kernel_on_hub_rows():
    """A graph with 3 000-edge hubs: the row kernel's time is the hub's serial walk; the edge-parallel kernel spreads it over 47
    waves.  (north_star: "wavefront-level segmented reduction"; verdict r03: at least 3x on the hub graph.)"""
    rng = np.random.default_rng(1)
    n, f = 24000, 256
    g = _hub_graph(rng, n, hubs=[5, 9000, 23000], hub_deg=3000)
    x = dev(rng.standard_normal((n, f)).astype(np.float32))
    indptr, indices, w = dev(g.indptr), dev(g.indices), dev(g.weight)

    def t(fn):
        for _ in range(3):
            fn()
        best = None
        for _ in range(4):                                           # (the best of four: a shared box stalls now and then)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 10
            best = ms if best is None else min(best, ms)
        return best
    t_row = t(lambda: ops.spmm_csr(indptr, indices, w, x, n))
    t_edge = t(lambda: ops.spmm_csr_edge(indptr, indices, w, x, n))
    print(f"hub graph: row kernel {t_row * 1e3:.1f} us, edge-parallel {t_edge * 1e3:.1f} us")
    assert t_edge * 3 <= t_row


# ---------------------------------------------------------------- host-resident training sets (models/residency.py)
@pytest.mark.parametrize("f0,hid,gemm_mode,delay,late,agg", [(831, 256, None, 0, "1", True), (831, 256, None, 0, "1", False),
                                                             (13, 256, None, 0, "1", False), (63, 200, None, 0, "1", False),
                                                             (831, 256, None, 60_000_000, "1", True), (363, 149, None, 60_000_000, "0", True),
                                                             (63, 200, None, 60_000_000, "0", False),
                                                             (63, 64, "f32", 60_000_000, "1", False), (63, 64, "f32", 60_000_000, "0", False)])
def test_windowed_run_is_bitwise_the_all_resident_run_on_the_same_step_stream(f0, hid, gemm_mode, delay, late, agg, monkeypatch):
    """A training set kept in pinned host memory with a two-slot window in HBM (uploads on a copy stream while the previous
    window trains, image conversion on the device, row-map batches) against the SAME step stream run on the all-resident set:
    losses and parameters bit for bit after three sweeps' worth of steps.

    ``delay``: every upload is held back by a ~30 ms spin on the copy stream (longer than all the steps of a window take), so a
    reader that is not ordered behind the window's `ready` event reads a slot that has not arrived -- round 4's assembly stream
    was such a reader (it waited for its own buffer events only; advisor finding): page tables, CSRs, labels and, in fp32 'copy'
    mode (``gemm_mode='f32'``), the feature rows.  ``late='0'``: GTE_PIPE_LATE=0, every assembly starts ahead of its step.
    ``agg``: the windows carry the image of the input's mean aggregate (computed per upload on the copy stream) and layer 0 runs
    on it (GTE_LAYER_CACHED), as on the all-resident set with its one image."""
    monkeypatch.setenv("GTE_PIPE_LATE", late)
    if gemm_mode is not None:
        prev_mode = ops.set_gemm_mode(gemm_mode)
        try:
            return _windowed_vs_resident(f0, hid, delay, agg)
        finally:
            ops.set_gemm_mode(prev_mode)
    _windowed_vs_resident(f0, hid, delay, agg)


def _windowed_vs_resident(f0, hid, delay, agg=False):
    from gnn_tableextraction_amd.models import residency as R
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    pages = S.make_pages(48, in_feats=f0)
    graphs = []
    for p in pages:
        g = gte.PageGraph(p.src, p.dst, p.num_nodes)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
        g.edata["feat"] = torch.from_numpy(p.weight)
        graphs.append(g)
    B, n_steps = 5, 40

    def fresh():
        torch.manual_seed(9)
        m = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0).to(DEV)
        return FusedGcnSageStep(m, lr=0.01, weight_decay=5e-4)
    # windowed
    tr = fresh()
    want_p3 = tr.wants_p3_features(f0)
    host = R.HostPages(graphs, DEV, chunk_bytes=1 << 20)                # (several construction chunks)
    agg = bool(agg and want_p3 and tr.wants_agg_image(f0))
    total = host.feature_bytes() * ((3.0 if agg else 1.5) if want_p3 else 1.0)
    wp = R.WindowedPages(host, budget_bytes=total * 0.9, want_p3=want_p3, want_agg=agg)     # two slots of < half the set: >= 3 windows
    assert len(wp.ranges) >= 3
    wp.delay_cycles = delay
    stream = R.WindowStream(wp.ranges, B, passes=2, seed=5)
    wp.prefetch(stream.peek_window())
    pipe = BatchPipeline(wp.acquire(stream.peek_window()))
    losses_w = []
    R.run_windowed(tr, pipe, wp, stream, n_steps, on_step=lambda s, g, o: losses_w.append(o[:1].clone()))
    torch.cuda.synchronize()
    assert wp.uploaded_bytes > host.feature_bytes()                         # windows were revisited: more than one sweep
    # all-resident, the same stream in global page ids
    tr2 = fresh()
    res = G.ResidentPages(graphs, DEV)
    if want_p3:
        res.enable_p3(agg=agg)
    pipe2 = BatchPipeline(res)
    stream2 = R.WindowStream(wp.ranges, B, passes=2, seed=5)
    losses_r = []
    for w, steps in stream2.take(n_steps):
        p0 = wp.ranges[w][0]
        run_steps(tr2, pipe2, [ids + p0 for ids in steps], on_step=lambda s, g, o: losses_r.append(o[:1].clone()))
    torch.cuda.synchronize()
    assert len(losses_w) == len(losses_r) == n_steps
    assert torch.equal(torch.cat(losses_w), torch.cat(losses_r))
    assert torch.equal(tr.flat_param, tr2.flat_param) and torch.equal(tr.exp_avg_sq, tr2.exp_avg_sq)


@pytest.mark.parametrize("f0", [831, 63, 16])
def test_resident_agg_image_is_the_mean_aggregate_of_every_page(f0):
    """ResidentPages.build_agg_image: the P3 image of norm . A_w x over all resident pages (made once; the cached operand of
    GTE_LAYER_CACHED) holds exactly the fp32 values gte_spmm_csr (mean) computes on the batched graph of all pages -- which is
    pinned on the oracle -- and row n_nodes of the allocation is zero."""
    pages = S.make_pages(23, in_feats=f0)
    graphs = []
    for p in pages:
        g = gte.PageGraph(p.src, p.dst, p.num_nodes)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
        g.edata["feat"] = torch.from_numpy(p.weight)
        graphs.append(g)
    res = G.ResidentPages(graphs, DEV)
    img = res.build_agg_image()
    whole = res.batch(np.arange(len(pages)))
    csr = whole.in_csr()
    want = ops.spmm_csr(csr.indptr, csr.indices, whole.in_weights(whole.edata["feat"]), res.feat, res.n_nodes, mean=True)
    got = ops.p3_to_f32(ops.P3(img.data, res.n_nodes, f0))
    assert torch.equal(got, want)
    src, dst, w, feat, label, off = S.concat_pages(pages)
    ref = oc.OracleGraph(src, dst, int(off[-1]), w)
    ah = oc._SpMM.apply(torch.from_numpy(feat), ref) * torch.from_numpy(ref.norm)            # models.py:53-57, 74-78
    np.testing.assert_allclose(got.cpu().numpy(), ah.numpy(), rtol=1e-5, atol=1e-5 * float(np.abs(feat).max()))
    assert img.data.shape[0] == res.n_nodes + 1 and not img.data[res.n_nodes].any()


@pytest.mark.parametrize("f", [100, 139, 149, 157, 206, 218, 5, 250])
@pytest.mark.parametrize("n,relu", [(3000, True), (77, False)])
def test_narrow_output_kernels_on_padded_rows(f, n, relu):
    """gte_sage_narrow_fwd_pad / gte_sage_narrow_bwd_ln_p3_pad (hidden widths that are not a multiple of 8, rows padded with zeros
    to 16 floats: the one-call plan's layout) against the plain-FMA narrow kernels + gte_ln_relu_bwd_p3 at the true width: the
    same sums in another order; W / dW in the reference's [C][2 f] layout; the padding of dz and of its image written as zeros."""
    lib, P, cs, check = _lib.load(), _lib.ptr, _lib.current_stream, _lib.check
    c, ld = 9, c16(f)
    assert lib.gte_sage_narrow_pad_supported(f, ld, c) == 1
    rng = np.random.default_rng(n + f)
    t = torch.zeros((n, 2 * ld), device=DEV)                          # z = the left half of t (padding zero), as the planes layer keeps it
    t[:, :f] = dev(rng.standard_normal((n, f)).astype(np.float32))
    t[:, ld:ld + f] = dev(rng.standard_normal((n, f)).astype(np.float32))
    gam, bet = dev(1 + 0.1 * rng.standard_normal(f).astype(np.float32)), dev(0.1 * rng.standard_normal(f).astype(np.float32))
    h, stats = torch.zeros((n, ld), device=DEV), torch.zeros(2 * n, device=DEV)
    check(lib.gte_ln_relu_fwd_p3(P(t), 2 * ld, P(gam), P(bet), 1e-5, int(relu), P(h), ld, None, 0, P(stats), n, f, cs()), "ln fwd")
    assert not h[:, f:].any()
    W = dev((rng.standard_normal((c, 2 * f)) / np.sqrt(2 * f)).astype(np.float32))
    bias = dev(rng.standard_normal(c).astype(np.float32))
    # forward
    ts_a, tn_a, ts_b, tn_b = (torch.zeros((n, c), device=DEV) for _ in range(4))
    check(lib.gte_sage_narrow_fwd(P(h), ld, f, P(W), 2 * f, P(bias), c, P(ts_a), c, P(tn_a), c, n, cs()), "fwd")
    check(lib.gte_sage_narrow_fwd_pad(P(h), ld, f, ld, P(W), 2 * f, P(bias), c, P(ts_b), c, P(tn_b), c, n, cs()), "fwd_pad")
    for got, want in ((ts_b, ts_a), (tn_b, tn_a)):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(want.abs().max()) + 1e-7)
    # backward: two launches at the true width
    dl, q = dev(rng.standard_normal((n, c)).astype(np.float32) / n), dev(rng.standard_normal((n, c)).astype(np.float32) / n)
    wsn = torch.empty(int(lib.gte_sage_narrow_bwd_workspace_bytes(n, ld, c)), dtype=torch.uint8, device=DEV)
    dh, dWa, dba = torch.zeros((n, ld), device=DEV), torch.zeros((c, 2 * f), device=DEV), torch.zeros(c, device=DEV)
    check(lib.gte_sage_narrow_bwd(P(dl), c, P(q), c, P(h), ld, f, P(W), 2 * f, c, P(dh), ld, P(dWa), 2 * f, P(dba), n, P(wsn), wsn.numel(),
                                  cs()), "bwd")
    dga, dbea, dbia = (torch.zeros(f, device=DEV) for _ in range(3))
    dza, dzp_a = torch.zeros((n, ld), device=DEV), ops.P3.empty(n, f, DEV)
    wl = torch.empty(int(lib.gte_ln_relu_bwd_workspace_bytes(n, f)), dtype=torch.uint8, device=DEV)
    check(lib.gte_ln_relu_bwd_p3(P(dh), ld, P(t), 2 * ld, P(stats), P(gam), P(bet), int(relu), P(dza), ld, P(dzp_a.data), dzp_a.ldp, P(dga),
                                 P(dbea), P(dbia), n, f, P(wl), wl.numel(), cs()), "ln bwd p3")
    # one launch on the padded rows
    dzb = torch.full((n, ld), 7.0, device=DEV)
    dzb[:, (f + 3) // 4 * 4:] = 0                                       # (the padding beyond the row's last 16-byte chunk is the buffer's)
    dWb, dbb = torch.zeros((c, 2 * f), device=DEV), torch.zeros(c, device=DEV)
    dgb, dbeb, dbib = (torch.zeros(f, device=DEV) for _ in range(3))
    dzp_b = ops.P3.empty(n, f, DEV)
    dzp_b.data.fill_(0x55)
    wln = torch.empty(int(lib.gte_sage_narrow_bwd_ln_workspace_bytes(n, ld)), dtype=torch.uint8, device=DEV)
    check(lib.gte_sage_narrow_bwd_ln_p3_pad(P(dl), c, P(q), c, P(h), ld, f, ld, P(W), 2 * f, c, P(dzb), ld, P(dzp_b.data), dzp_b.ldp,
                                            P(dWb), 2 * f, P(dbb), n, P(wsn), wsn.numel(), None, 1.0, None, P(t), 2 * ld, P(stats), P(gam),
                                            P(bet), int(relu), P(dgb), P(dbeb), P(dbib), P(wln), wln.numel(), cs()), "bwd_ln_p3_pad")
    ref = dza.cpu().numpy()
    np.testing.assert_allclose(dzb.cpu().numpy()[:, :f], ref[:, :f], rtol=2e-5, atol=3e-6 * float(np.abs(ref).max()))
    assert not dzb[:, f:].any()
    img = ops.p3_to_f32(ops.P3(dzp_b.data, n, ld))                      # the whole padded image row
    assert torch.equal(img[:, :f], dzb[:, :f]) and not img[:, f:].any()
    for got, want in ((dWb, dWa), (dbb, dba), (dgb, dga), (dbeb, dbea), (dbib, dbia)):
        r = want.cpu().numpy()
        np.testing.assert_allclose(got.cpu().numpy(), r, rtol=2e-5, atol=3e-6 * np.abs(r).max() + 1e-12)


@pytest.mark.parametrize("f0,hid", [(831, 256), (363, 149), (831, 1000)])
def test_a_graph_with_its_own_cached_images_runs_the_cached_input_layer(f0, hid):
    """engine.attach_feature_image (what train() does to the validation graph): the graph keeps the P3 image of its features AND of
    their mean aggregate, made once; forward_logits then runs layer 0 as ONE launch on [x | ahn] (GTE_LAYER_CACHED without a row map)
    -- logits against the CPU oracle at 1e-5 -- and a training step on such a graph matches the step on the plain graph."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    pages = S.make_pages(9, in_feats=f0)
    src, dst, w, feat, label, off = S.concat_pages(pages)
    n = int(off[-1])
    torch.manual_seed(7)
    model = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0)
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    og = oc.OracleGraph(src, dst, n, w)
    want = oc.gcnsage_forward(state0, og, torch.from_numpy(feat)).numpy()

    def graph():
        g = gte.PageGraph(src, dst, n, device=DEV)
        g.ndata["feat"], g.edata["feat"] = dev(feat), dev(w)
        return g
    fused = FusedGcnSageStep(model.to(DEV), lr=0.01, weight_decay=5e-4)
    g = graph()
    assert fused.attach_feature_image(g) and g.agg_p3 is not None
    assert fused._plan_kinds(f0, n, fused._batch_cached(g))[0] == 3
    np.testing.assert_allclose(fused.forward_logits(g).cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    y = dev(label).float()
    out_c = fused.step(g, y).clone()
    p_c = fused.flat_param.detach().clone()
    # the same step on the plain graph (layer 0 aggregates in the step)
    torch.manual_seed(7)
    m2 = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0).to(DEV)
    f2 = FusedGcnSageStep(m2, lr=0.01, weight_decay=5e-4)
    out_p = f2.step(graph(), y)
    assert abs(float(out_c[0]) - float(out_p[0])) < 1e-5
    d = (p_c - f2.flat_param).abs()
    assert float(d.max()) <= 0.0201 and float((d > 1e-4).float().mean()) < 0.03        # (Adam's first step: lr where a gradient is noise)
