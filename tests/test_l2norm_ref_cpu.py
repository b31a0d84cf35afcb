"""The float64 reference of ReLU + row L2-normalise (tests/l2norm_ref.py) is right: against torch autograd of
``F.normalize(F.relu(z), eps=eps)`` in float64, rows clamped by a large eps and degenerate rows included.  And what needs no GPU
of the feature itself: the library exports the kernel pair's entry points, and ``MeanSAGE.forward`` takes a graph alone."""
import inspect

import numpy as np
import pytest
import torch

from tests import l2norm_ref as ref


def _case(seed, m=9, n=7):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((m, n))
    z[1] = -np.abs(z[1]) - 0.1                 # an all-negative row
    z[2] = 0.0                                 # an all-zero row
    z[3] *= 0.05                               # norm ~ 0.1: clamped at eps = 0.5 (and at 3.0)
    z[4, :] = -1.0
    z[4, 2] = 0.7                              # a single positive entry
    dy = rng.standard_normal((m, n))
    return z, dy


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("eps", [1e-12, 0.5, 3.0])
def test_reference_matches_torch_autograd_in_float64(eps, relu):
    z, dy = _case(int(eps * 10) + int(relu))
    zt = torch.from_numpy(z.copy()).requires_grad_(True)
    yt = torch.nn.functional.normalize(torch.relu(zt) if relu else zt, p=2.0, dim=1, eps=eps)
    yt.backward(torch.from_numpy(dy))
    y, norm = ref.fwd(z, relu, eps)
    dz, dbias = ref.bwd(dy, y, norm, relu, eps)
    assert np.abs(y - yt.detach().numpy()).max() <= 1e-12
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12
    assert np.abs(dbias - zt.grad.numpy().sum(axis=0)).max() <= 1e-12
    # the cases are what they claim to be
    r = np.maximum(z, 0) if relu else z
    assert np.array_equal(norm, np.sqrt((r * r).sum(1)))
    if eps == 0.5:
        assert norm[3] < eps < norm[0]                                    # clamped and unclamped rows in one case
    if eps == 3.0:
        assert (norm < eps).sum() >= 3
    if relu:
        assert norm[1] == 0 and norm[2] == 0 and (y[1] == 0).all() and (dz[1] == 0).all() and (dz[2] == 0).all()
        assert y[4, 2] == (1.0 if eps <= 0.7 else 0.7 / eps)
        if eps <= 0.7:
            assert (dz[4] == 0).all()                                     # the projection removes the one live direction


def test_clamped_rows_take_no_projection_term():
    """norm < eps: y = r / eps and dz = dy / eps on the live entries -- a pure scaling, torch's clamp_min passes nothing to the norm."""
    z, dy = _case(11)
    z[0] *= 3.0 / np.sqrt((z[0] ** 2).sum()) * 2                          # one row of norm 6: not clamped
    y, norm = ref.fwd(z, False, 3.0)
    dz, _ = ref.bwd(dy, y, norm, False, 3.0)
    clamped = norm < 3.0
    assert clamped.any() and not clamped.all()
    np.testing.assert_allclose(dz[clamped], dy[clamped] / 3.0, rtol=1e-15)
    np.testing.assert_allclose(y[clamped], z[clamped] / 3.0, rtol=1e-15)


def test_library_exports_the_l2norm_entry_points():
    from gnn_tableextraction_amd import _lib
    lib = _lib.load()
    for name in ("gte_relu_l2norm_fwd", "gte_relu_l2norm_bwd_workspace_bytes", "gte_relu_l2norm_bwd"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    # host logic only: sizes, and the argument checks that return before anything is launched
    assert lib.gte_relu_l2norm_bwd_workspace_bytes(1000, 256) >= 250 * 256 * 4
    assert lib.gte_relu_l2norm_bwd_workspace_bytes(10 ** 6, 256) == lib.gte_relu_l2norm_bwd_workspace_bytes(10 ** 7, 256)
    assert lib.gte_relu_l2norm_fwd(None, 8, 1, 1e-12, None, 8, None, 0, 8, None) == 0            # M == 0
    assert lib.gte_relu_l2norm_fwd(None, 8, 1, 1e-12, None, 8, None, 4, 8, None) == -1           # null pointers
    assert lib.gte_relu_l2norm_fwd(None, 8, 1, 0.0, None, 8, None, 0, 8, None) == -1             # eps <= 0
    assert b"eps" in lib.gte_last_error()


def test_meansage_forward_takes_a_graph_alone():
    import gnn_tableextraction_amd as gte
    sig = inspect.signature(gte.MeanSAGE.forward)
    sig.bind(None, "g")                                                   # (self, g)
    sig.bind(None, "g", "h", "w")                                         # the reference's call keeps working
    assert list(sig.parameters)[1:] == ["g", "h", "w"]
    lsig = inspect.signature(gte.WeightedMeanSAGELayer.forward)
    assert lsig.parameters["l2norm"].default is False
    assert callable(gte.ops.relu_l2norm)
