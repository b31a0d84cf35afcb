"""EM for a one-dimensional Gaussian mixture, the iterations on the HIP device (csrc/gmm.hip; every formula is stated in
include/gte.h): ``sklearn.mixture.GaussianMixture(K, covariance_type='full', weights_init=, means_init=, precisions_init=)`` of
scikit-learn 1.7.2 on ONE feature ("soft"), and the hard-assignment variant of the reference's ``HardEMGaussianMixture``
(src/components/tables/gmm/gmm_hardem.py) ("hard"), which ``Preprocessor.train_gmm`` of the reference fits to the corpus's
numerals on the host.  Two public stages, as components/tables/affinity.py and tsne.py are built:

  ``prepare``   host: scikit-learn's checks with its messages, ``pc = sqrt(precisions_init)``, the initial parameter block
  ``run``       device: one upload of the samples, the iterations in chunks, stopped by the device

``prepare`` touches no device, nothing here imports scikit-learn, and this module initialises nothing by itself: all three
``*_init`` are required (``init_from_prototypes`` restates the reference's own initialisation).  Deviations, all deliberate:
one feature, ``covariance_type='full'``, ``n_init=1``, no ``warm_start``; sums over the samples in the kernels' fixed order
(two runs give the same bits; scikit-learn's BLAS order differs in the last digits); ``predict_proba`` / ``predict`` /
``score_samples`` compute in float64 whatever the points' dtype (the reference passes float32 points, and scikit-learn then
computes the log-densities in float32) and ``predict_proba`` returns the soft responsibilities ``exp(wlp - lse)`` for a hard
fit too (``HardEMGaussianMixture`` inherits scikit-learn's, and its ``predict`` is the arg-max of the same)."""
from __future__ import annotations

import warnings
from typing import NamedTuple

import numpy as np

from ... import _lib

CONVERGENCE_TEXT = ("Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or check "
                    "for degenerate data.")
ILL_DEFINED_TEXT = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
                    "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale "
                    "the input data.")


class GmmConvergenceWarning(UserWarning):
    """The fit ran ``max_iter`` iterations without ``|change| < tol`` (scikit-learn's ConvergenceWarning is a UserWarning too)."""


class Prepared(NamedTuple):
    """Outcome of ``prepare``: ``x`` float64 [n], ``P`` float64 [4, K] = (weights, means, covariances, precisions_cholesky) ahead
    of the first E step (the covariances, which no E step reads, as 1 / precisions), and the numbers of the fit."""
    x: np.ndarray
    P: np.ndarray
    hard: bool
    tol: float
    reg_covar: float
    max_iter: int


class GmmResult(NamedTuple):
    """The fitted attributes, named and shaped as scikit-learn's."""
    weights_: np.ndarray                # [K]
    means_: np.ndarray                  # [K, 1]
    covariances_: np.ndarray            # [K, 1, 1]
    precisions_cholesky_: np.ndarray    # [K, 1, 1]
    converged_: bool
    n_iter_: int
    lower_bound_: float
    hard: bool

    @property
    def precisions_(self):
        return self.precisions_cholesky_ ** 2

    def parameter_block(self) -> np.ndarray:
        """float64 [4, K] as the kernels read it."""
        return np.ascontiguousarray(np.stack([self.weights_.reshape(-1), self.means_.reshape(-1), self.covariances_.reshape(-1),
                                              self.precisions_cholesky_.reshape(-1)]).astype(np.float64))


def _samples(x, what="X") -> np.ndarray:
    x = np.asarray(x)
    if x.dtype == object or x.dtype.kind not in "fiub":
        raise ValueError(f"gmm: {what} must be numeric, got dtype {x.dtype}")
    if x.ndim == 2 and x.shape[1] == 1:
        x = x.reshape(-1)
    elif x.ndim != 1:
        raise ValueError(f"gmm: {what} must be 1-D or [n, 1] (one feature), got shape {x.shape}")
    x = np.ascontiguousarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        raise ValueError(f"Input {what} contains NaN or infinity.")
    return x


def _check_shape(param, shape, name):
    if param.shape != shape:
        raise ValueError("The parameter '%s' should have the shape of %s, but got %s" % (name, shape, param.shape))


def prepare(x, weights_init, means_init, precisions_init, *, hard=False, tol=1e-3, reg_covar=1e-6, max_iter=100) -> Prepared:
    """Everything ``BaseMixture.fit_predict`` does ahead of its loop for given ``*_init``: ``ValueError`` -- with scikit-learn's
    text where it has one -- for samples that are not finite, not 1-D or [n, 1], fewer than 2 or fewer than the components; for
    weights outside [0, 1] or not summing to 1 within 1e-8; for wrong shapes (weights [K], means [K, 1] or [K], precisions
    [K, 1, 1] or [K]); for precisions that are not positive; for numbers outside scikit-learn's ranges and sizes above the kernels'
    limits (``gte_gmm_max_components()`` components, 2^31 - 1 samples).  Then ``pc = sqrt(precisions_init)``
    (``_compute_precision_cholesky_from_precisions`` for one feature).  No device call."""
    if weights_init is None or means_init is None or precisions_init is None:
        raise ValueError("gmm: weights_init, means_init and precisions_init are all required (init_from_prototypes makes them)")
    for name, v in (("tol", tol), ("reg_covar", reg_covar)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not v >= 0 or v == float("inf"):
            raise ValueError(f"gmm: {name} must be a finite number >= 0, got {v!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"gmm: max_iter must be an integer >= 1, got {max_iter!r}")
    x = _samples(x)
    n = x.shape[0]
    if n < 2:
        raise ValueError(f"Found array with {n} sample(s) (shape=({n}, 1)) while a minimum of 2 is required.")
    means = np.asarray(means_init, dtype=np.float64)
    if means.ndim == 1:
        means = means.reshape(-1, 1)
    K = means.shape[0] if means.ndim else 0
    weights = np.asarray(weights_init, dtype=np.float64)
    _check_shape(weights, (K,), "weights")
    if K < 1 or K > _lib.load().gte_gmm_max_components():
        raise ValueError(f"gmm: {K} components, the kernels take 1 .. {_lib.load().gte_gmm_max_components()}")
    if n >= 2 ** 31:
        raise ValueError(f"gmm: {n} samples, the kernels take 2^31 - 1")
    if n < K:
        raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d" % (K, n))
    if not np.isfinite(weights).all():
        raise ValueError("Input contains NaN or infinity.")
    if (weights < 0.0).any() or (weights > 1.0).any():
        raise ValueError("The parameter 'weights' should be in the range [0, 1], but got max value %.5f, min value %.5f"
                         % (np.min(weights), np.max(weights)))                # (scikit-learn's own order of the two numbers)
    if not np.allclose(np.abs(1.0 - np.sum(weights)), 0.0, atol=1e-8):
        raise ValueError("The parameter 'weights' should be normalized, but got sum(weights) = %.5f" % np.sum(weights))
    _check_shape(means, (K, 1), "means")
    prec = np.asarray(precisions_init, dtype=np.float64)
    if prec.ndim == 1:
        prec = prec.reshape(-1, 1, 1)
    _check_shape(prec, (K, 1, 1), "full precision")
    if not (np.isfinite(means).all() and np.isfinite(prec).all()):
        raise ValueError("Input contains NaN or infinity.")
    if (prec <= 0.0).any():
        raise ValueError("'full precision' should be symmetric, positive-definite")
    prec = prec.reshape(-1)
    P = np.stack([weights, means.reshape(-1), 1.0 / prec, np.sqrt(prec)])
    return Prepared(x, np.ascontiguousarray(P), bool(hard), float(tol), float(reg_covar), int(max_iter))


def run(prepared: Prepared, device=None, chunk=8) -> GmmResult:
    """The iterations on the HIP device: one upload of the samples and ``P``, then ``gmm_iterate`` in chunks of ``chunk``
    iterations, the 64-byte state read back after each -- the only synchronisation.  The stop is the device's, so ``chunk``
    changes no bit.  Warns ``GmmConvergenceWarning`` with scikit-learn's text when ``max_iter`` iterations pass without
    convergence; ``ValueError`` with scikit-learn's "ill-defined empirical covariance" text when a covariance is not finite or
    not positive."""
    import torch
    from ... import graph as G
    device = _lib.default_device(device)
    if device.type != "cuda":
        _lib.require_device(torch.empty(0, device=device), "gmm.run")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"gmm.run: chunk must be >= 1, got {chunk}")
    n, K = prepared.x.shape[0], prepared.P.shape[1]
    with torch.cuda.device(device):
        ws = G.gmm_workspace(n, K, device)
        x = torch.from_numpy(prepared.x).to(device)
        P = torch.from_numpy(prepared.P).to(device)
        state = torch.tensor([0, 0, 0, 0, -np.inf, -np.inf, 0, 0], dtype=torch.float64, device=device)
        done, stopped, st = 0, 0, None
        while not stopped and done < prepared.max_iter:
            G.gmm_iterate(x, P, prepared.hard, prepared.tol, prepared.reg_covar, prepared.max_iter,
                          min(chunk, prepared.max_iter - done), ws, state)
            st = state.tolist()
            done, stopped = int(st[0]), int(st[1])
        out = P.cpu().numpy()
    if st[3]:
        raise ValueError(ILL_DEFINED_TEXT)
    converged = bool(st[2])
    if not converged:
        warnings.warn(CONVERGENCE_TEXT, GmmConvergenceWarning, stacklevel=2)
    return GmmResult(out[0].copy(), out[1].reshape(K, 1).copy(), out[2].reshape(K, 1, 1).copy(), out[3].reshape(K, 1, 1).copy(),
                     converged, done, float(st[4]), prepared.hard)


def gaussian_mixture(x, weights_init, means_init, precisions_init, *, hard=False, tol=1e-3, reg_covar=1e-6, max_iter=100, device=None,
                     chunk=8) -> GmmResult:
    """``GaussianMixture(K, weights_init=, means_init=, precisions_init=, tol=, reg_covar=, max_iter=).fit(x)`` (``hard``: the
    reference's ``HardEMGaussianMixture``) on the HIP device: ``prepare`` -> ``run``."""
    return run(prepare(x, weights_init, means_init, precisions_init, hard=hard, tol=tol, reg_covar=reg_covar, max_iter=max_iter),
               device, chunk)


def _posterior(result: GmmResult, points, device, **want):
    import torch
    from ... import graph as G
    pts = _samples(points, "points")
    K = result.weights_.shape[0]
    if pts.shape[0] == 0:
        return np.zeros((0, K)), np.zeros(0), np.zeros(0, dtype=np.int32)
    device = _lib.default_device(device)
    if device.type != "cuda":
        _lib.require_device(torch.empty(0, device=device), "gmm: posterior")
    with torch.cuda.device(device):
        r, s, lab = G.gmm_posterior(torch.from_numpy(pts).to(device), torch.from_numpy(result.parameter_block()).to(device), **want)
        return tuple(None if t is None else t.cpu().numpy() for t in (r, s, lab))


def predict_proba(result: GmmResult, points, device=None) -> np.ndarray:
    """float64 [m, K]: the responsibilities ``exp(wlp - lse)`` of ``points`` (1-D or [m, 1]) under the fitted mixture, in float64
    on the device (gte_gmm_posterior: the E step of the fit)."""
    return _posterior(result, points, device, resp=True)[0]


def predict(result: GmmResult, points, device=None) -> np.ndarray:
    """int [m]: the first-index arg-max of ``wlp - lse``: the component of every point."""
    return _posterior(result, points, device, resp=False, label=True)[2].astype(np.int64)


def score_samples(result: GmmResult, points, device=None) -> np.ndarray:
    """float64 [m]: ``lse``, the log-likelihood of every point."""
    return _posterior(result, points, device, resp=False, lse=True)[1]


def init_from_prototypes(data, prototypes, min_sigma=1e-6, chunk=1 << 16):
    """``(weights [K], means [K, 1], precisions [K, 1, 1])`` as the reference's ``train_gmm`` makes them from prototypes
    (preprocessor.py:193-211), host numpy, its quirks kept:
      * every cluster list starts with one ``0``, which enters the mean, the standard deviation and the count;
      * a sample belongs to the nearest prototype, the first index on a tie (``np.argmin``);
      * the "covariance" is the POPULATION STANDARD DEVIATION of the list (``np.std``), not a variance, and
        ``precision = 1 / std`` (``np.linalg.inv`` of a 1 x 1 matrix);
      * ``weights = len / sum(len)``, the lengths counting the leading ``0``.
      * a prototype that wins no sample keeps the lone ``0``: mean 0, ``min_sigma`` in place of its standard deviation.
    The distance matrix is formed in chunks of ``chunk`` samples, never [n, K] at once.  A zero standard deviation -- a list of
    zeros only -- raises ``ValueError`` (the reference's ``np.linalg.inv`` raises LinAlgError there)."""
    data = _samples(data, "data")
    mus = np.asarray(prototypes, dtype=np.float64).reshape(-1)
    K = mus.shape[0]
    if K < 1 or not np.isfinite(mus).all():
        raise ValueError(f"init_from_prototypes: prototypes must be a non-empty finite vector, got {prototypes!r}")
    amin = np.empty(data.shape[0], dtype=np.int64)
    for a in range(0, data.shape[0], int(chunk)):
        amin[a:a + chunk] = np.argmin(np.abs(data[a:a + chunk] - mus[:, None]), axis=0)
    means, stds, lens = np.empty(K), np.empty(K), np.empty(K, dtype=np.int64)
    for k in range(K):
        cluster = np.concatenate([[0.0], data[amin == k]])               # (sample order inside a cluster is the data's, as there)
        means[k] = np.mean(cluster)
        stds[k] = np.std(cluster) if cluster.shape[0] > 1 else min_sigma
        lens[k] = cluster.shape[0]
    if (stds == 0.0).any():
        raise ValueError(f"init_from_prototypes: clusters {np.flatnonzero(stds == 0.0).tolist()} have zero standard deviation "
                         f"(singular matrix in the reference's np.linalg.inv)")
    return lens / np.sum(lens), means.reshape(-1, 1), (1.0 / stds).reshape(-1, 1, 1)
