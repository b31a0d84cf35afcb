"""Dropout on the fused train step (GTE_LAYER_DROPOUT, csrc/dropout.hip) on an MI355X.

The masks are counter-based (csrc/dropout.h), so the float64 reference below runs on the DEVICE's masks -- read back through
gte_dropout_mask at the step's counter -- and on the device's ReLU masks (tests/stepcheck.py): no branch is left to disagree on.
The reference is plain torch float64 autograd of models.py:46-66 / :105-113 in training mode with those masks given.
"""
import numpy as np
import pytest
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import graph as G, ops
from gnn_tableextraction_amd.data import synthetic as S
from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
from oracle import gcnsage_cpu as oc
from tests import poststep, stepcheck as sc
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _scale(p):
    return float(np.float32(1.0 / (1.0 - p)))


def _graph(src, dst, w, x):
    g = G.PageGraph(src, dst, len(x), device=DEV)
    g.ndata["feat"], g.edata["feat"] = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(w).to(DEV)
    return g


# ------------------------------------------------------------------------------------------------------------ the masks
@pytest.mark.parametrize("n,c", [(1, 1), (37, 13), (130, 17), (1001, 1662), (4097, 219), (24577, 26)])
def test_device_mask_equals_host_mask(n, c):
    for p, seed, rank, step, site in [(0.1, 42, 0, 0, 0), (0.5, 2 ** 63 + 11, 3, 77777, 2)]:
        d = ops.dropout_mask(p, seed, rank, step, site, n, c, device=DEV).cpu().numpy()
        h = ops.dropout_mask(p, seed, rank, step, site, n, c).numpy()
        np.testing.assert_array_equal(d, h)


# ------------------------------------------------------------------------------------------------------ the producer
def _page_graph(n_pages, f0, seed=0):
    pages = [S.make_page(seed + j, in_feats=f0) for j in range(n_pages)]
    src, dst, w, feat, label, off = S.concat_pages(pages)
    return src, dst, w, feat, label, int(off[-1])


def _ref_operands(src, dst, w, x, p, seed, step, site, in_drop):
    """D_site([x' | norm A_w x']) in fp32 (x' = D_0(x) when in_drop), from the host masks; aggregation in float64."""
    n, f = x.shape
    sc_ = np.float32(_scale(p))
    xd = x.astype(np.float32)
    if in_drop:
        xd = np.where(ops.dropout_mask(p, seed, 0, step, 0, n, f).numpy() == 1, xd * sc_, np.float32(0))
    og = oc.OracleGraph(src, dst, n, w)
    agg = oc.spmm_csr_torch(og.indptr, og.indices, og.weight.astype(np.float64), torch.from_numpy(xd.astype(np.float64))).numpy()
    deg = np.diff(og.indptr)
    agg = agg / np.maximum(deg, 1)[:, None] * (deg > 0)[:, None]
    m = ops.dropout_mask(p, seed, 0, step, site, n, 2 * f).numpy() == 1
    self_ = np.where(m[:, :f], xd * sc_, np.float32(0))
    agg = np.where(m[:, f:], agg * float(sc_), 0.0)
    return self_, agg


@pytest.mark.parametrize("f0,in_drop,resident", [(831, True, True), (831, True, False), (13, True, True), (218, False, False),
                                                 (1000, False, False), (100, True, False)])
def test_producer_images_equal_the_masked_aggregate(f0, in_drop, resident):
    src, dst, w, x, _, n = _page_graph(4, f0, seed=f0)
    p, seed, step, site = 0.3, 99, 5, 1 if in_drop else 2
    g = _graph(src, dst, w, x)
    csr = g.in_csr()
    counter = torch.tensor([step], dtype=torch.int64, device=DEV)
    if resident:
        # the rows of a larger resident image through a row map (the train loop's batches on resident feature images)
        rng = np.random.default_rng(f0)
        res = rng.standard_normal((n + 333, f0)).astype(np.float32)
        rows = rng.permutation(n + 333)[:n].astype(np.int32)
        x = res[rows]
        img = ops.p3_from_f32(torch.from_numpy(res).to(DEV))
        pad = -(-n // 16) * 16 + 1
        rmap = torch.full((pad,), n + 333, dtype=torch.int32)
        rmap[:n] = torch.from_numpy(rows)
        xin = ops.P3(img.data, n, f0, rmap.to(DEV), n + 333)
    else:
        xin = torch.from_numpy(x).to(DEV)
    sp, ap = ops.spmm_dropout_p3(csr.indptr, csr.indices, g.in_weights(g.edata["feat"]), xin, n, p, seed, 0, counter, site, in_drop)
    want_s, want_a = _ref_operands(src, dst, w, x, p, seed, step, site, in_drop)
    got_s, got_a = ops.p3_to_f32(sp).cpu().numpy(), ops.p3_to_f32(ap).cpu().numpy()
    np.testing.assert_array_equal(got_s, want_s)                     # (two fp32 products: exact)
    err = np.abs(got_a - want_a).max() / max(np.abs(want_a).max(), 1e-30)
    assert err <= 1e-6, err
    # the image's padding columns up to the next multiple of 16 are zeros
    kp = -(-f0 // 16) * 16
    if kp > f0:
        full = ops.p3_to_f32(ops.P3(ap.data, n, kp)).cpu().numpy()
        assert not full[:, f0:].any()


@pytest.mark.parametrize("f", [13, 218, 256, 1000])
def test_backward_aggregation_through_the_masks(f):
    src, dst, w, x, _, n = _page_graph(3, 8, seed=f)
    p, seed, step, site = 0.5, 7, 3, 2
    g = _graph(src, dst, w, x)
    rcsr = g.out_csr()
    kp = -(-f // 16) * 16
    Gm = torch.randn(n, 2 * kp, dtype=torch.float32)
    Gm[:, f:kp] = 0
    Gm[:, kp + f:] = 0
    counter = torch.tensor([step], dtype=torch.int64, device=DEV)
    got = ops.spmm_dropout_bwd(rcsr.indptr, rcsr.indices, g.out_weights(g.edata["feat"], True), Gm.to(DEV), kp, f, p, seed, 0,
                               counter, site).cpu().numpy()
    m = ops.dropout_mask(p, seed, 0, step, site, n, 2 * f).numpy() == 1
    s = np.float32(_scale(p))
    G64 = Gm.numpy().astype(np.float64)
    dself = np.where(m[:, :f], G64[:, :f] * s, 0.0)
    dagg = np.where(m[:, f:], G64[:, kp:kp + f] * s, 0.0)
    og = oc.OracleGraph(src, dst, n, w)
    deg = np.diff(og.indptr).astype(np.float64)
    want = dself.copy()
    np.add.at(want, og.src, (og.eweight.astype(np.float64) / deg[og.dst])[:, None] * dagg[og.dst])
    assert np.abs(got[:, :f] - want).max() <= 1e-5 * np.abs(want).max()
    assert not got[:, f:].any()


# ---------------------------------------------------------------------------------------------------- the whole step
def reference_dropout_step(state0, og, x, labels, relu_masks, drop_masks, p, class_weights=None, lr=0.01, weight_decay=5e-4):
    """One float64 step of GcnSAGE in training mode (models.py:46-66, :105-113) with the given dropout masks (drop_masks[0]: the
    input [n, f0], drop_masks[i + 1]: hidden layer i over [n, 2 fin]) and ReLU masks; loss, gradients and the Adam step."""
    st = {k: torch.as_tensor(v).detach().to(torch.float64).clone().requires_grad_(True) for k, v in state0.items()}
    opt = torch.optim.Adam(list(st.values()), lr=lr, weight_decay=weight_decay)
    scale = _scale(p)
    nl = 1 + max(int(k.split(".")[1]) for k in st)
    norm = torch.from_numpy(og.norm).to(torch.float64)
    h = torch.as_tensor(np.asarray(x)).to(torch.float64) * torch.from_numpy(drop_masks[0]).to(torch.float64) * scale
    for i in range(nl):
        W, b = st[f"layers.{i}.linear.weight"], st[f"layers.{i}.linear.bias"]
        a = torch.cat((h, oc._SpMM.apply(h, og) * norm), dim=1)
        if i < nl - 1:
            a = a * torch.from_numpy(drop_masks[i + 1]).to(torch.float64) * scale
            z = torch.nn.functional.linear(a, W, b)
            z = torch.nn.functional.layer_norm(z, (z.shape[1],), st[f"layers.{i}.lynorm.weight"], st[f"layers.{i}.lynorm.bias"], 1e-5)
            h = z * torch.from_numpy(np.asarray(relu_masks[i])).to(torch.float64)
        else:
            h = torch.nn.functional.linear(a, W, b)
    cw = None if class_weights is None else torch.as_tensor(class_weights).to(torch.float64)
    loss = torch.nn.functional.cross_entropy(h, torch.as_tensor(np.asarray(labels)).long(), weight=cw)
    opt.zero_grad()
    loss.backward()
    grads = {k: v.grad.detach().numpy().copy() for k, v in st.items()}
    opt.step()
    return {"loss": float(loss), "grads": grads, "state": {k: v.detach().numpy() for k, v in st.items()}}


def device_dropout_masks(engine, n, dims, step):
    p, seed, rank = engine.dropout_p, engine.dropout_seed, engine.rank
    out = [ops.dropout_mask(p, seed, rank, step, 0, n, dims[0], device=DEV).cpu().numpy()]
    for i in range(len(dims) - 2):
        out.append(ops.dropout_mask(p, seed, rank, step, i + 1, n, 2 * dims[i], device=DEV).cpu().numpy())
    return out


def _check_step(engine, model, batch, og, x, labels, state0, p, cw, step, n, f0):
    torch.cuda.synchronize()
    dims = [f0] + [l.out_feats for l in model.layers]
    kinds = engine._plan_kinds(f0, n, engine._batch_cached(batch))
    assert kinds == [4] * (len(dims) - 2), kinds
    relu = sc.device_relu_masks(engine, batch, state0)
    drop = device_dropout_masks(engine, n, dims, step)
    grads = {k: engine._gslice[id(q)].cpu().numpy() for k, q in model.named_parameters()}
    ref = reference_dropout_step(state0, og, x, labels, relu, drop, p, cw)
    return ref, grads, drop


SHAPES = ["shape_f13_h218", "shape_f831_h96", "shape_f363_h149", "shape_f63_h1000", "shape_f831_h1000"]


# (a dropout step runs the planes GEMMs in either GEMM mode -- the one-call plan is its only path: the "f32" cases check that the
# mode switch leaves the dropout step intact, not a second arithmetic)
@pytest.mark.parametrize("mode", ["split_bf16", "f32"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", SHAPES)
def test_dropout_step_matches_the_masked_fp64_reference_on_run_shapes(name, p, mode):
    z, src, dst, w, x, y, state0, _ = poststep.trimmed_case(GOLDEN_DIR, name)
    meta = [int(v) for v in z["meta"]]
    n, f0, hid, ncls, nl = meta[:5]
    prev = ops.set_gemm_mode(mode)
    try:
        model = gte.GcnSAGE(f0, hid, ncls, nl, torch.nn.functional.relu, p)
        model.load_state_dict(state0)
        model = model.to(DEV)
        eng = FusedGcnSageStep(model, dropout_seed=1234 + n, lr=0.01, weight_decay=5e-4)
        g = _graph(src, dst, w, x)
        labels = torch.from_numpy(y).to(DEV)
        out3 = eng.step(g, labels)
        torch.cuda.synchronize()
        assert eng._step_dev_host == 1 and int(eng._step_dev.item()) == 1
        og = oc.OracleGraph(src, dst, n, w)
        ref, grads, _ = _check_step(eng, model, g, og, x, y, state0, p, None, 0, n, f0)
        assert abs(float(out3[0].item()) - ref["loss"]) < sc.LOSS_ATOL, (float(out3[0].item()), ref["loss"])
        sc.assert_grads(grads, ref["grads"], what=f"{name} p={p} {mode}: ")
        params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        with torch.no_grad():
            after = eng.forward_logits(g).cpu().numpy()
        sc.check_poststep(ref, params, state0, og, x, after)
    finally:
        ops.set_gemm_mode(prev)


def _resident(pages):
    graphs = []
    for pg in pages:
        g = gte.PageGraph(pg.src, pg.dst, pg.num_nodes)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(pg.feat), torch.from_numpy(pg.label.astype(np.float32))
        g.edata["feat"] = torch.from_numpy(pg.weight)
        graphs.append(g)
    return G.ResidentPages(graphs, DEV)


@pytest.mark.parametrize("f0,hid,m,p,mode,nl", [(831, 256, 24577, 0.1, "split_bf16", 3), (831, 256, 16385, 0.5, "f32", 3),
                                                (13, 218, 8193, 0.1, "split_bf16", 3), (63, 206, 8193, 0.1, "split_bf16", 4)])
def test_dropout_step_on_probe_pages_through_the_train_loop(f0, hid, m, p, mode, nl):
    """cfg2-size batches through the loop (ResidentPages + BatchPipeline + run_steps): layer 0 reads the resident feature image
    through the batch's row map; probes at the row-tile boundaries (tests/stepcheck.probe_pages)."""
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    pages, probes, off = sc.probe_pages(f0, m, sc.one_round_tile(m, 256), seed=m)
    src, dst, w, feat, label, _ = S.concat_pages(pages)
    og = oc.OracleGraph(src, dst, m, w)
    torch.manual_seed(42)
    # (nl = 4: two dropout layers above layer 0 -- the mask backward of layer 2 writes dy of layer 1, itself a dropout layer)
    state0 = {k: v.detach().clone() for k, v in gte.GcnSAGE(f0, hid, sc.N_CLASSES, nl, torch.nn.functional.relu, 0).state_dict().items()}
    prev = ops.set_gemm_mode(mode)
    try:
        model = gte.GcnSAGE(f0, hid, sc.N_CLASSES, nl, torch.nn.functional.relu, p)
        model.load_state_dict(state0)
        model = model.to(DEV)
        eng = FusedGcnSageStep(model, dropout_seed=m, lr=0.01, weight_decay=5e-4, class_weights=sc.probe_class_weights().to(DEV))
        res = _resident(pages)
        pipe = BatchPipeline(res)
        ids = np.arange(len(pages))
        out3 = run_steps(eng, pipe, [ids])
        torch.cuda.synchronize()
        batch = res.batch(ids)
        assert getattr(batch, "feat_p3", None) is not None and batch.feat_p3.row_map is not None
        ref, grads, _ = _check_step(eng, model, batch, og, feat, label, state0, p, sc.probe_class_weights(), 0, m, f0)
        assert abs(float(out3[0]) - ref["loss"]) < sc.LOSS_ATOL
        sc.assert_grads(grads, ref["grads"], what=f"probe f0={f0} hid={hid} m={m} p={p} {mode}: ")
    finally:
        ops.set_gemm_mode(prev)


# ----------------------------------------------------------------------------------------------- captured graph, eval
def _layer0_self_image(eng, g, private_key=None):
    b = eng.plan_buffers(g, private_key)[0]
    return ops.p3_to_f32(b["hp"][0].view_rows(g.ndata["feat"].shape[0])).cpu().numpy()


def test_captured_replays_draw_fresh_masks_and_equal_the_eager_step():
    z, src, dst, w, x, y, state0, _ = poststep.trimmed_case(GOLDEN_DIR, "shape_f831_h96")
    n, f0, hid, ncls, nl = [int(v) for v in z["meta"]][:5]
    p, seed = 0.2, 31337
    s = np.float32(_scale(p))

    def engine():
        model = gte.GcnSAGE(f0, hid, ncls, nl, torch.nn.functional.relu, p)
        model.load_state_dict(state0)
        model = model.to(DEV)
        return model, FusedGcnSageStep(model, dropout_seed=seed, lr=0.01, weight_decay=5e-4)
    ma, a = engine()
    ga = _graph(src, dst, w, x)
    la = torch.from_numpy(y).to(DEV)
    replay = a.capture(ga, la)
    want = []
    for c in range(2):
        m0 = ops.dropout_mask(p, seed, 0, c, 0, n, f0).numpy() == 1
        m1 = ops.dropout_mask(p, seed, 0, c, 1, n, 2 * f0).numpy() == 1
        xd = np.where(m0, x.astype(np.float32) * s, np.float32(0))
        want.append(np.where(m1[:, :f0], xd * s, np.float32(0)))
    got = []
    params_after_1 = None
    for c in range(2):
        replay()
        torch.cuda.synchronize()
        assert int(a._step_dev.item()) == c + 1
        got.append(_layer0_self_image(a, ga, id(ga)))
        if c == 0:
            params_after_1 = {k: v.detach().cpu().clone() for k, v in ma.state_dict().items()}
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert not np.array_equal(got[0], got[1])
    # the eager step at counter 0 computes what the first replay computed, bit for bit
    mb, b = engine()
    gb = _graph(src, dst, w, x)
    b.step(gb, torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_layer0_self_image(b, gb), want[0])
    for k, v in mb.state_dict().items():
        assert torch.equal(v.detach().cpu(), params_after_1[k]), k
    a.release()


@pytest.mark.parametrize("name", ["shape_f831_h96", "shape_f13_h218", "shape_f831_h1000"])
def test_evaluation_applies_no_dropout(name):
    z, src, dst, w, x, y, state0, _ = poststep.trimmed_case(GOLDEN_DIR, name)
    n, f0, hid, ncls, nl = [int(v) for v in z["meta"]][:5]
    outs = []
    for p in (0.5, 0.0):
        model = gte.GcnSAGE(f0, hid, ncls, nl, torch.nn.functional.relu, p)
        model.load_state_dict(state0)
        model = model.to(DEV)
        eng = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
        model.train()                                  # (forward_logits applies no mask whatever the module's mode)
        g = _graph(src, dst, w, x)
        outs.append((eng.forward_logits(g).clone().cpu().numpy(), eng.forward_logits(g).clone().cpu().numpy()))
        model.eval()
        with torch.no_grad():
            outs[-1] = outs[-1] + (model(g).cpu().numpy(),)
    (d1, d2, dm), (r1, r2, rm) = outs
    np.testing.assert_array_equal(d1, d2)
    np.testing.assert_array_equal(d1, r1)               # the same evaluation plan: bit for bit
    np.testing.assert_array_equal(dm, rm)
    np.testing.assert_allclose(d1, z["logits"], rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------- train()
@pytest.mark.parametrize("p", [0.2, 0.0])
def test_train_with_dropout_runs_fused_learns_and_resumes_bitwise(p, tmp_path, monkeypatch, capsys):
    """p = 0 as well: a resumed run restores the device's bias corrections (engine._sync_adam_state), dropout or not."""
    import re
    from gnn_tableextraction_amd.models import model_train
    from gnn_tableextraction_amd.utils.config import logs_from_config
    from tests.test_gpu_train_entry import learnable_pages, make_cfg
    monkeypatch.setenv("GTE_KEEP_LAST_RUN", "1")
    data = learnable_pages(48)

    def run(d, epochs, resume=False):
        cfg = make_cfg(d, n_epochs=epochs, dropout=p, **({"from_checkpoint": "true"} if resume else {}))
        model_train.train(data, cfg)
        ck = torch.load(d / "checkpoints" / logs_from_config(cfg), weights_only=False)
        return ck, model_train.LAST_RUN["step"]
    capsys.readouterr()
    full, st = run(tmp_path / "a", 4)
    assert isinstance(st, FusedGcnSageStep) and st.dropout_p == pytest.approx(p) and st.adam_fused_steps > 0
    losses = [float(v) for v in re.findall(r"Train: Loss ([0-9.]+)", capsys.readouterr().out)]
    assert len(losses) == 4 and losses[-1] < losses[0], losses
    assert full.get("dropout_seed") == (42 if p > 0 else None)
    run(tmp_path / "b", 2)
    resumed, _ = run(tmp_path / "b", 4, resume=True)
    assert resumed["epoch"] == 4
    for k, v in full["state_dict"].items():
        assert torch.equal(v, resumed["state_dict"][k]), k
