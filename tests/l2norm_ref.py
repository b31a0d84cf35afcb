"""float64 numpy reference of ReLU + row L2-normalise (gte_relu_l2norm_fwd / gte_relu_l2norm_bwd of include/gte.h):
``torch.nn.functional.normalize(relu?(z), p=2, dim=1, eps)`` and its autograd backward.  Test infrastructure; pinned against
torch autograd in float64 by tests/test_l2norm_ref_cpu.py."""
import numpy as np


def fwd(z, relu=True, eps=1e-12):
    """(y, norm): r = relu ? max(z, 0) : z; norm = sqrt(sum r^2) per row (unclamped); y = r / max(norm, eps)."""
    z = np.asarray(z, dtype=np.float64)
    r = np.maximum(z, 0.0) if relu else z
    norm = np.sqrt((r * r).sum(axis=1))
    return r / np.maximum(norm, eps)[:, None], norm


def bwd(dy, y, norm, relu=True, eps=1e-12):
    """(dz, dbias) from the forward's y and norm.  A clamped norm (norm < eps) gets no gradient (torch's clamp_min), so the
    projection term is dropped there; the ReLU mask is y > 0 and it is a select: dr may be huge (d = eps) where y == 0."""
    dy, y, norm = (np.asarray(a, dtype=np.float64) for a in (dy, y, norm))
    d = np.maximum(norm, eps)
    proj = np.where(norm >= eps, (y * dy).sum(axis=1), 0.0)
    dr = (dy - y * proj[:, None]) / d[:, None]
    dz = np.where(y > 0, dr, 0.0) if relu else dr
    return dz, dz.sum(axis=0)
