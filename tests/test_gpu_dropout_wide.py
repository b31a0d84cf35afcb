"""Dropout on the fused train step at any batch size: the WIDE addressing form (gte_dropout_set_wide, csrc/gemm_p3.hip store_tile,
csrc/step.hip layer_wide) against the 32-bit form, the float64 oracle, a batch past the old 2 GB bound, the C ABI's row bound, and
``test()`` with a dropout configuration on the resident path.

The wide form changes WHERE a buffer window starts, never a value or a summation order: every comparison between the two forms is
``torch.equal``.  The oracle comparisons reuse tests/test_gpu_dropout.py's reference on the device's dropout and ReLU masks and its
tolerances (gradients 1e-4 of each tensor's largest entry, post-step state through poststep.hybrid_state).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import _lib, graph as G, ops
from gnn_tableextraction_amd.data import synthetic as S
from gnn_tableextraction_amd.models.engine import DROPOUT_MAX_ROWS, FusedGcnSageStep
from oracle import gcnsage_cpu as oc
from tests import stepcheck as sc
from tests.test_gpu_dropout import _check_step, _graph, _resident

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 0.1
N_CLASSES = 9


class forced_wide:
    """gte_dropout_set_wide(on) on THIS thread for the block (the hook is thread-local: every step below is issued from here)."""
    def __init__(self, on):
        self.on = int(bool(on))

    def __enter__(self):
        _lib.check(_lib.load().gte_dropout_set_wide(self.on), "gte_dropout_set_wide")
        assert _lib.load().gte_dropout_get_wide() == self.on

    def __exit__(self, *exc):
        _lib.load().gte_dropout_set_wide(0)


def _pages(n_pages, f0, seed, variant=None):
    pages = [S.make_page(seed + j, in_feats=f0) for j in range(n_pages)]
    if variant == "zero_in":                      # node 2 of the first page loses its in-edges
        q = pages[0]
        keep = q.dst != 2
        q.src, q.dst, q.weight = q.src[keep], q.dst[keep], q.weight[keep]
    if variant == "dup":                          # the first 40 edges of the last page once more
        q = pages[-1]
        q.src, q.dst, q.weight = (np.concatenate([q.src, q.src[:40]]), np.concatenate([q.dst, q.dst[:40]]),
                                  np.concatenate([q.weight, q.weight[:40]]))
    return pages


def _state0(f0, hid, nl, seed=7):
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in gte.GcnSAGE(f0, hid, N_CLASSES, nl, torch.nn.functional.relu, 0).state_dict().items()}


def _engine(f0, hid, nl, state0, seed):
    model = gte.GcnSAGE(f0, hid, N_CLASSES, nl, torch.nn.functional.relu, P)
    model.load_state_dict(state0)
    model = model.to(DEV)
    return model, FusedGcnSageStep(model, dropout_seed=seed, lr=0.01, weight_decay=5e-4)


def _site_masks(eng, n, dims, step):
    out = [ops.dropout_mask(eng.dropout_p, eng.dropout_seed, eng.rank, step, 0, n, dims[0], device=DEV)]
    for i in range(len(dims) - 2):
        out.append(ops.dropout_mask(eng.dropout_p, eng.dropout_seed, eng.rank, step, i + 1, n, 2 * dims[i], device=DEV))
    return out


def _two_steps(f0, hid, nl, pages, wide, how="eager"):
    """Two optimisation steps from the same seed and state; what they left: losses, flat gradient after step 1, flat parameters after
    step 2, the masks of every site at both steps."""
    state0 = _state0(f0, hid, nl)
    all_bits = (1 << (nl - 1)) - 1
    with forced_wide(wide):
        model, eng = _engine(f0, hid, nl, state0, seed=4242)
        losses, grad1 = [], None
        if how == "resident":
            from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
            res = _resident(pages)
            pipe = BatchPipeline(res)
            ids = np.arange(len(pages))
            for c in range(2):
                losses.append(run_steps(eng, pipe, [ids]).clone())
                if c == 0:
                    grad1 = eng.flat_grad.clone()
            g = res.batch(ids)
            assert g.feat_p3 is not None and g.feat_p3.row_map is not None          # layer 0 through the row map
            n = g.feat_p3.rows
        else:
            src, dst, w, x, y, off = S.concat_pages(pages)
            n = int(off[-1])
            g = _graph(src, dst, w, x)
            labels = torch.from_numpy(y).to(DEV)
            if how == "capture":
                replay = eng.capture(g, labels)
                for c in range(2):
                    losses.append(replay().clone())
                    if c == 0:
                        grad1 = eng.flat_grad.clone()
            else:
                for c in range(2):
                    losses.append(eng.step(g, labels).clone())
                    if c == 0:
                        grad1 = eng.flat_grad.clone()
        torch.cuda.synchronize()
        assert int(eng._step_dev.item()) == 2
        assert eng.wide_layers(g) == (all_bits if wide else 0)                      # the form the steps took
        dims = [f0] + [l.out_feats for l in model.layers]
        masks = _site_masks(eng, n, dims, 0) + _site_masks(eng, n, dims, 1)
        out = {"loss": torch.stack(losses).cpu(), "grad": grad1.cpu(), "param": eng.flat_param.detach().clone().cpu(),
               "masks": [m.cpu() for m in masks]}
        if how == "capture":
            eng.release()
    return out


def _assert_same(a, b):
    assert torch.equal(a["loss"], b["loss"]), (a["loss"], b["loss"])
    assert torch.equal(a["grad"], b["grad"]), float((a["grad"] - b["grad"]).abs().max())
    assert torch.equal(a["param"], b["param"]), float((a["param"] - b["param"]).abs().max())
    assert len(a["masks"]) == len(b["masks"])
    for ma, mb in zip(a["masks"], b["masks"]):
        assert torch.equal(ma, mb)
    assert bool(a["grad"].abs().max() > 0) and bool(torch.isfinite(a["param"]).all())


# -------------------------------------------------------------------------------------- 1. wide == narrow, bit for bit
MODELS = [(13, 218, 3), (831, 256, 3), (63, 1000, 3), (13, 96, 2)]


@pytest.mark.parametrize("n_pages,variant", [(2, "zero_in"), (5, "dup")])
@pytest.mark.parametrize("f0,hid,nl", MODELS)
def test_wide_path_equals_the_narrow_path_bitwise(f0, hid, nl, n_pages, variant):
    pages = lambda: _pages(n_pages, f0, seed=11 * n_pages + f0, variant=variant)
    _assert_same(_two_steps(f0, hid, nl, pages(), False), _two_steps(f0, hid, nl, pages(), True))


def test_wide_path_equals_the_narrow_path_through_the_resident_row_map():
    f0, hid, nl = 831, 256, 3
    _assert_same(_two_steps(f0, hid, nl, _pages(5, f0, 3), False, "resident"), _two_steps(f0, hid, nl, _pages(5, f0, 3), True, "resident"))


def test_wide_path_equals_the_narrow_path_captured_and_replayed_twice():
    f0, hid, nl = 63, 1000, 3
    narrow = _two_steps(f0, hid, nl, _pages(2, f0, 5), False, "capture")
    _assert_same(narrow, _two_steps(f0, hid, nl, _pages(2, f0, 5), True, "capture"))
    _assert_same(narrow, _two_steps(f0, hid, nl, _pages(2, f0, 5), False, "eager"))     # (and the replays are the eager steps)


# ------------------------------------------------------------------------------------------ 2. wide against the oracle
@pytest.mark.parametrize("f0,hid,nl", [(13, 218, 3), (831, 256, 3)])
def test_wide_step_matches_the_masked_fp64_reference(f0, hid, nl):
    src, dst, w, x, y, off = S.concat_pages(_pages(5, f0, seed=f0 + 1, variant="zero_in"))
    n = int(off[-1])
    state0 = _state0(f0, hid, nl)
    with forced_wide(True):
        model, eng = _engine(f0, hid, nl, state0, seed=1234 + n)
        g = _graph(src, dst, w, x)
        out3 = eng.step(g, torch.from_numpy(y).to(DEV))
        torch.cuda.synchronize()
        assert eng.wide_layers(g) == (1 << (nl - 1)) - 1
        og = oc.OracleGraph(src, dst, n, w)
        ref, grads, _ = _check_step(eng, model, g, og, x, y, state0, P, None, 0, n, f0)
        loss = float(out3[0].item())
        errs = sc.grad_errors(grads, ref["grads"])
        print(f"wide ({f0}, {hid}, {nl}) n={n}: loss {loss:.7f} ref {ref['loss']:.7f}; worst gradient {max(errs.values()):.3f} of the tolerance")
        assert abs(loss - ref["loss"]) < sc.LOSS_ATOL, (loss, ref["loss"])
        sc.assert_grads(grads, ref["grads"], what=f"wide ({f0}, {hid}): ")
        params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        with torch.no_grad():
            after = eng.forward_logits(g).cpu().numpy()
        sc.check_poststep(ref, params, state0, og, x, after)


# --------------------------------------------------------------------------------- 3. a batch past the old 2 GB bound
def test_step_past_the_old_two_gigabyte_bound_takes_the_wide_path_and_matches_the_oracle():
    """GcnSAGE(13, 1024, 3, 2) on the smallest graph the 32-bit form's bound excluded: (n + 256) x 2 x 1024 x 4 >= 2^31."""
    f0, hid, ncls, nl, deg = 13, 1024, 3, 2, 4
    n = -(-(1 << 31) // (2 * hid * 4)) - 256
    assert (n + 256) * 2 * hid * 4 >= 1 << 31 > (n - 1 + 256) * 2 * hid * 4
    rng = np.random.default_rng(2024)
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    src = rng.integers(0, n, n * deg, dtype=np.int64)
    w = rng.uniform(0.05, 1.0, n * deg).astype(np.float32)
    x = rng.standard_normal((n, f0)).astype(np.float32)
    y = rng.integers(0, ncls, n).astype(np.int64)
    torch.manual_seed(9)
    state0 = {k: v.detach().clone() for k, v in gte.GcnSAGE(f0, hid, ncls, nl, torch.nn.functional.relu, 0).state_dict().items()}
    model = gte.GcnSAGE(f0, hid, ncls, nl, torch.nn.functional.relu, P)
    model.load_state_dict(state0)
    model = model.to(DEV)
    eng = FusedGcnSageStep(model, dropout_seed=77, lr=0.01, weight_decay=5e-4)
    g = G.from_edge_index(torch.from_numpy(np.stack([src, dst])).to(DEV), n, torch.from_numpy(w).to(DEV))
    g.ndata["feat"] = torch.from_numpy(x).to(DEV)
    assert _lib.load().gte_dropout_get_wide() == 0                       # hook off: the step's own choice
    out3 = eng.step(g, torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    assert eng.wide_layers(g) == 1
    og = oc.OracleGraph(src.astype(np.int32), dst.astype(np.int32), n, w)
    ref, grads, _ = _check_step(eng, model, g, og, x, y, state0, P, None, 0, n, f0)
    loss = float(out3[0].item())
    errs = sc.grad_errors(grads, ref["grads"])
    print(f"n={n}: loss {loss:.7f} ref {ref['loss']:.7f} (rel {abs(loss - ref['loss']) / abs(ref['loss']):.2e}); gradients in units of "
          f"the tolerance {({k: round(v, 3) for k, v in errs.items()})}")
    assert abs(loss - ref["loss"]) <= 1e-4 * abs(ref["loss"]), (loss, ref["loss"])
    sc.assert_grads(grads, ref["grads"], rel=1e-4, what=f"n={n}: ")
    # the mask's row word is the whole row index: rows from 2^18 on repeat neither row 0 nor the row 2^18 below them.  (This batch
    # ends 256 rows short of 2^18; the hook draws any row count, so it is asked for 4096 rows past it, 256 columns wide: two rows
    # agree by chance with probability 0.82^256.)
    lo = 1 << 18
    m = ops.dropout_mask(P, eng.dropout_seed, eng.rank, 0, 1, lo + 4096, 256, device=DEV)
    assert bool((m[lo:] != m[0]).any(dim=1).all())
    assert bool((m[lo:] != m[:4096]).any(dim=1).all())


# ------------------------------------------------------------------------------------------------ 4. the C ABI's bound
def _sizes_only_plan(n_nodes):
    fake = 0x1000                                      # never dereferenced: the plan check precedes every launch
    plan = _lib.StepPlan()
    plan.n_hidden, plan.n_nodes = 1, n_nodes
    plan.out_fin, plan.n_classes = 64, 9
    plan.dropout_p, plan.dropout_seed, plan.rank = 0.1, 1, 0
    plan.step_counter = fake
    L = plan.layer[0]
    L.kind, L.fin, L.fout = _lib.LAYER_DROPOUT, 13, 64
    for f in ("W", "bias", "gamma", "beta", "x", "hp", "ahnp", "wimg_fwd", "dzp", "t", "y", "dy", "stats"):
        setattr(L, f, fake)
    L.ldx = 13
    return plan


def test_c_abi_refuses_a_dropout_plan_past_the_row_bound_before_any_launch():
    lib = _lib.load()
    plan = _sizes_only_plan(DROPOUT_MAX_ROWS + 1)
    fused = ctypes.c_int(0)
    torch.cuda.synchronize()
    rc = lib.gte_gcnsage_step(ctypes.addressof(plan), 0, ctypes.byref(fused), _lib.current_stream())
    assert rc == -4, rc                                # GTE_ERR_UNSUPPORTED
    msg = lib.gte_last_error().decode()
    assert "2^30" in msg and str(DROPOUT_MAX_ROWS + 1) in msg, msg
    torch.cuda.synchronize()                           # (nothing was queued: no fault to surface)
    # the plan query on sizes alone: narrow at a bench-size batch, wide from the old bound on, and under the hook
    plan.n_nodes = 24576
    assert lib.gte_gcnsage_step_wide_layers(ctypes.addressof(plan)) == 0
    plan.layer[0].fout = 1024
    plan.n_nodes = 261888
    assert lib.gte_gcnsage_step_wide_layers(ctypes.addressof(plan)) == 1
    plan.n_nodes = 261887
    assert lib.gte_gcnsage_step_wide_layers(ctypes.addressof(plan)) == 0
    with forced_wide(True):
        assert lib.gte_gcnsage_step_wide_layers(ctypes.addressof(plan)) == 1
    # the producers themselves hold the same bound
    rc = lib.gte_spmm_dropout_p3(0x1000, 0x1000, None, 0x1000, 13, None, 0, None, 0, 1, 0.1, 1, 0, 0x1000, 1, 0x1000, 96, 0x1000, 96,
                                 DROPOUT_MAX_ROWS + 1, 13, _lib.current_stream())
    assert rc == -4 and "2^30" in lib.gte_last_error().decode()
    assert lib.gte_dropout_set_wide(2) == -1


# ------------------------------------------------------------------------------------------- 5. test() after --dropout
def test_predict_entry_takes_the_resident_path_for_a_dropout_config(tmp_path, monkeypatch):
    from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
    from gnn_tableextraction_amd.models import model_predict
    from gnn_tableextraction_amd.utils.config import logs_from_config
    from tests.test_gpu_train_entry import make_cfg
    torch.manual_seed(3)
    data = PrebuiltPages.synthetic(6, in_feats=13)
    state = gte.GcnSAGE(13, 64, 9, 3, torch.nn.functional.relu, 0).state_dict()
    calls = []
    real = model_predict.predict_resident

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(model_predict, "predict_resident", counting)
    flat = {}
    for p in (0.1, 0.0):
        d = tmp_path / f"p{p}"
        cfg = make_cfg(d, batch_size=4, dropout=p)
        assert float(cfg.TRAINING.dropout) == p
        os.makedirs(d / "weights", exist_ok=True)
        torch.save(state, d / "weights" / f"{logs_from_config(cfg)}.pt")
        before = len(calls)
        out = model_predict.test(data, cfg)
        assert len(calls) == before + 1, f"dropout {p}: test() did not take predict_resident"
        flat[p] = np.concatenate(out["all_pred"])
    np.testing.assert_array_equal(flat[0.1], flat[0.0])
    assert len(flat[0.1]) == sum(g.num_nodes() for g in data.graphs)
