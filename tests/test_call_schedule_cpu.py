"""Host side of the call-by-call schedule (models/call_schedule.py): what needs no device."""
import pytest
import torch


def test_backward_rest_without_its_forward_is_refused_before_any_launch():
    """The state a pass hands from its forward to its backward lives in one record kept with the buffer set, not on the engine:
    backward_rest() on a batch no forward_backward(..., upto_layer=k) ran on says so -- before it asks for device tensors or
    calls the library."""
    import gnn_tableextraction_amd as gte
    from gnn_tableextraction_amd import graph as G
    from gnn_tableextraction_amd._lib import GteError
    from gnn_tableextraction_amd.data import synthetic as S
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    torch.manual_seed(0)
    eng = FusedGcnSageStep(gte.GcnSAGE(13, 64, 9, 3, torch.nn.functional.relu, 0))
    eng.use_c_step = False
    for name in ("_head_scale", "_ln_p3_done", "_smallk_done"):
        assert not hasattr(eng, name)
    p = S.make_pages(1, in_feats=13)[0]
    g = G.PageGraph(p.src, p.dst, p.num_nodes)
    g.ndata["feat"], g.edata["feat"] = torch.from_numpy(p.feat), torch.from_numpy(p.weight)

    class NoCalls:                                  # any call into the library would be a launch on stale buffers
        def __getattr__(self, name):
            raise AssertionError(f"library call {name} before the refusal")
    eng.lib = NoCalls()
    with pytest.raises(RuntimeError, match="no forward of this batch is recorded") as e:
        eng.backward_rest(g, 1)
    assert not isinstance(e.value, GteError)
