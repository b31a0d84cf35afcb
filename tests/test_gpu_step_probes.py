"""Row-localised probes of the whole train step at the row-tile boundaries of its launches.

Class weights [1, 0, ..., 0] and label 0 on a few chosen probe nodes only (labels 1 ... 8 everywhere else): the step runs the same
kernels over the whole batch, but its loss and every dz are non-zero only in the probes' receptive field -- a wrong row among them
is a large part of each gradient instead of 1 / 24 000 of it.  Batch sizes straddle the thresholds of the one-round row tile
(csrc/gemm_p3.hip one_round_row_tile / lnb_row_tile: 32 / 64 / 96 rows up to 32 / 64 / 96 x #CUs rows, 128 above), asserted
through gte_gemm_p3_nt_plan; probes sit at row 0 and the last row, both sides of the first tile boundary, in the final partial
tile, on both sides of a page boundary, on an in-degree-0 node and on a hub with a few hundred in-edges
(tests/stepcheck.probe_pages).  The step is the loop's (ResidentPages + BatchPipeline + run_steps), in the default GEMM mode and
in f32; gradients against the float64 oracle run on the device's own ReLU masks (tests/stepcheck.py) at 1e-4 of each tensor's
largest entry, the loss at 1e-5.
"""
import ctypes

import numpy as np
import pytest
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import _lib, graph as G, ops
from gnn_tableextraction_amd.data import synthetic as S
from oracle import gcnsage_cpu as oc
from tests import stepcheck as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = [8191, 8193, 16383, 16385, 24575, 24577, 33000]
# the tile rule governs launches of at most 256 columns: every size on the narrower widths; the H = 1000 shapes on one size per
# side of the outer thresholds (the fp64 oracle at 33 k x 1 000 is the expensive part of a case)
CASES = ([(831, 256, m) for m in SIZES] + [(13, 218, m) for m in SIZES]
         + [(63, 1000, m) for m in (8193, 33000)] + [(831, 1000, m) for m in (8191, 24577)])


def _cus() -> int:
    lib = _lib.load()
    cu, wave, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    name = ctypes.create_string_buffer(64)
    assert lib.gte_device_info(ctypes.byref(cu), ctypes.byref(wave), ctypes.byref(lds), name, 64) == 0
    return cu.value


def _plan_tile(m: int, cus: int) -> int:
    """Row tile of the dX + LayerNorm-backward product ([m x 256], K = 2 x 256, block-major weights) for m rows on cus CUs."""
    rt = ctypes.c_int(-1)
    assert _lib.load().gte_gemm_p3_nt_plan(m, 256, 256, 256, 1, 1, cus, ctypes.byref(rt)) == 1
    return rt.value


def _resident(pages):
    graphs = []
    for p in pages:
        g = gte.PageGraph(p.src, p.dst, p.num_nodes)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
        g.edata["feat"] = torch.from_numpy(p.weight)
        graphs.append(g)
    return G.ResidentPages(graphs, DEV)


def _device_step(pages, state0, f0, hid, mode):
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    prev = ops.set_gemm_mode(mode)
    try:
        model = gte.GcnSAGE(f0, hid, sc.N_CLASSES, 3, torch.nn.functional.relu, 0)
        model.load_state_dict(state0)
        model = model.to(DEV)
        fused = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4, class_weights=sc.probe_class_weights().to(DEV))
        res = _resident(pages)
        pipe = BatchPipeline(res)
        ids = np.arange(len(pages))
        out3 = run_steps(fused, pipe, [ids])
        torch.cuda.synchronize()
        batch = res.batch(ids)
        masks = sc.device_relu_masks(fused, batch, state0)           # (before anything else runs on the step's buffers)
        grads = {k: fused._gslice[id(p)].cpu().numpy() for k, p in model.named_parameters()}
        return float(out3[0]), grads, masks, fused._plan_kinds(f0, batch.num_nodes(), fused._batch_cached(batch))
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.parametrize("f0,hid,m", CASES)
def test_probe_rows_at_row_tile_boundaries_match_the_masked_fp64_oracle(f0, hid, m):
    cus = _cus()
    tile = _plan_tile(m, cus)
    assert tile == sc.one_round_tile(m, cus)
    if cus == 256:                 # MI355X: the thresholds the sizes were chosen for
        assert tile == {8191: 32, 8193: 64, 16383: 64, 16385: 96, 24575: 96, 24577: 128, 33000: 128}[m]
    pages, probes, off = sc.probe_pages(f0, m, tile, seed=m)
    src, dst, w, feat, label, _ = S.concat_pages(pages)
    assert int(off[-1]) == m and (label == 0).sum() == len(probes) >= 7
    og = oc.OracleGraph(src, dst, m, w)
    torch.manual_seed(42)
    state0 = {k: v.detach().clone() for k, v in gte.GcnSAGE(f0, hid, sc.N_CLASSES, 3, torch.nn.functional.relu, 0).state_dict().items()}
    ref, ref_masks, report = None, None, {}
    for mode in ("split_bf16", "f32"):
        loss, grads, masks, kinds = _device_step(pages, state0, f0, hid, mode)
        if ref is None or not all(np.array_equal(a, b) for a, b in zip(masks, ref_masks)):
            ref, ref_masks = sc.reference_step(state0, og, feat, label, masks, sc.probe_class_weights()), masks
        assert abs(loss - ref["loss"]) < sc.LOSS_ATOL, f"{mode}: loss {loss} against {ref['loss']}"
        errs = sc.assert_grads(grads, ref["grads"], what=f"{mode} (kinds {kinds}, tile {tile}, probes {probes}): ")
        report[mode] = round(max(errs.values()), 3)
    print(f"probe f0={f0} hid={hid} m={m} cus={cus} tile={tile} worst grad error / tol: {report}")
