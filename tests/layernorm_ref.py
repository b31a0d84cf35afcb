"""float64 numpy reference of LayerNorm(+ReLU) over the rows of a matrix (gte_ln_relu_fwd / gte_ln_relu_bwd of include/gte.h and
every fused form of them): ``torch.nn.functional.layer_norm(z, (n,), gamma, beta, eps)`` (+ ``relu``) and its autograd backward.
Biased variance over the true n columns, eps inside the square root, the ReLU mask taken on pre = xhat gamma + beta with a zero
gradient at pre == 0.  Test infrastructure; pinned against torch autograd in float64 by tests/test_layernorm_ref_cpu.py."""
import numpy as np


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


def fwd(z, gamma, beta, eps, relu):
    """(y, pre, mean, rstd): mean and biased variance per row, rstd = 1 / sqrt(var + eps), pre = xhat gamma + beta,
    y = max(pre, 0) when relu else pre."""
    z, gamma, beta = _f64(z, gamma, beta)
    mean = z.mean(axis=1)
    d = z - mean[:, None]
    var = (d * d).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + float(eps))
    pre = d * rstd[:, None] * gamma + beta
    return (np.maximum(pre, 0.0) if relu else pre), pre, mean, rstd


def bwd(dy, z, mean, rstd, gamma, beta, relu):
    """(dz, dgamma, dbeta, dbias) from the statistics handed in (the GPU tests hand in the device's float32 stats).  The mask is
    pre > 0: no gradient at pre == 0, as torch.relu.  dbias is the column sum of dz."""
    dy, z, mean, rstd, gamma, beta = _f64(dy, z, mean, rstd, gamma, beta)
    xhat = (z - mean[:, None]) * rstd[:, None]
    g = np.where(xhat * gamma + beta > 0, dy, 0.0) if relu else dy
    dxhat = g * gamma
    c1 = dxhat.mean(axis=1)
    c2 = (dxhat * xhat).mean(axis=1)
    dz = rstd[:, None] * (dxhat - c1[:, None] - xhat * c2[:, None])
    return dz, (g * xhat).sum(axis=0), g.sum(axis=0), dz.sum(axis=0)


def kappa(z, eps):
    """per-row condition number of the normalisation: max_j |z_j| / sqrt(var + eps)"""
    z, = _f64(z)
    var = ((z - z.mean(axis=1)[:, None]) ** 2).mean(axis=1)
    return np.abs(z).max(axis=1) / np.sqrt(var + float(eps))


def ambiguous(z, mean, rstd, gamma, beta, band):
    """boolean mask of the elements whose float64 |pre| is at most ``band`` (a per-row array, or anything that broadcasts against
    [M, n]): where a float32 evaluation of pre may land on the other side of the ReLU"""
    z, mean, rstd, gamma, beta, band = _f64(z, mean, rstd, gamma, beta, band)
    pre = (z - mean[:, None]) * rstd[:, None] * gamma + beta
    if band.ndim == 1:
        band = band[:, None]
    return np.abs(pre) <= band
