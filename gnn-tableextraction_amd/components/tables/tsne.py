"""Exact t-SNE on a precomputed distance matrix, its numerical stages on the HIP device (csrc/tsne.hip; every formula is stated in
include/gte.h): ``sklearn.manifold.TSNE(method='exact', metric='precomputed', init='random')`` of scikit-learn 1.7.2, which
``Preprocessor.train_repr`` of the reference runs on the host.  Two public stages, as components/tables/affinity.py is built:

  ``prepare``   host: scikit-learn's checks with its messages, ``D ** 2``, the float32 cast, the initial embedding, the learning rate
  ``run``       device: conditional and joint probabilities, then the two phases of the descent, stopped by the device

``prepare`` touches no device, and nothing here imports scikit-learn.  t-SNE's descent is chaotic: parity with scikit-learn is
bounded rounding per stage and per step and the quality reached (the KL divergence), not the coordinates.  Deviations, all
deliberate (include/gte.h): the embedding, ``update`` and ``gains`` are float64 throughout; the exact method has no limit of 3
components; the results are the same bits from run to run; with ``max_iter`` <= 250 the error reported is phase 1's (scikit-learn
reports ``np.finfo(float).max`` from a second phase that runs no iteration) and ``n_iter`` is the last iteration that ran."""
from __future__ import annotations

import numbers
from typing import NamedTuple

import numpy as np

from ... import _lib
from .affinity import check_random_state

EXPLORATION_ITER = 250                                                     # TSNE._EXPLORATION_MAX_ITER
CHECK_EVERY = 50                                                           # TSNE._N_ITER_CHECK
STOP_REASONS = {0: None, 1: "no progress", 2: "gradient norm"}


class Prepared(NamedTuple):
    """Outcome of ``prepare``: ``sq_dist`` float32 [n, n], ``init`` float64 [n, d], and the numbers of the descent."""
    sq_dist: np.ndarray
    init: np.ndarray
    perplexity: float
    early_exaggeration: float
    learning_rate: float
    max_iter: int
    n_iter_without_progress: int
    min_grad_norm: float


def _number(name, value, low, *, integer=False, closed=True):
    kind = numbers.Integral if integer else numbers.Real
    if isinstance(value, bool) or not isinstance(value, kind) or not (value >= low if closed else value > low) or value != value \
            or value == float("inf"):
        raise ValueError(f"tsne: {name} must be {'an integer' if integer else 'a finite number'} {'>=' if closed else '>'} {low}, "
                         f"got {value!r}")
    return int(value) if integer else float(value)


def prepare(D, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
            n_iter_without_progress=300, min_grad_norm=1e-7, init="random", random_state=None) -> Prepared:
    """Everything ``TSNE._fit`` does ahead of ``_joint_probabilities`` and ``_tsne`` for a dense precomputed ``D`` (distances, NOT
    squared): ``ValueError`` -- with scikit-learn's text where it has one -- for a matrix that is not square, holds NaN or
    infinity or a negative entry, for ``perplexity`` >= n, for parameters outside scikit-learn's ranges and for sizes above the
    kernels' limits (``gte_tsne_max_n()`` samples, ``gte_tsne_max_components()`` components); then ``D ** 2`` as float32, the
    init ``1e-4 * check_random_state(random_state).standard_normal((n, d)).astype(np.float32)`` (numpy's bits; an ndarray ``init``
    is taken as given) as float64, and ``learning_rate='auto'`` -> ``max(n / early_exaggeration / 4, 50)``.  No device call."""
    d = _number("n_components", n_components, 1, integer=True)
    perplexity = _number("perplexity", perplexity, 0, closed=False)
    early_exaggeration = _number("early_exaggeration", early_exaggeration, 1)
    max_iter = _number("max_iter", max_iter, EXPLORATION_ITER, integer=True)
    n_iter_without_progress = _number("n_iter_without_progress", n_iter_without_progress, -1, integer=True)
    min_grad_norm = _number("min_grad_norm", min_grad_norm, 0)
    if not (isinstance(learning_rate, str) and learning_rate == "auto"):
        learning_rate = _number("learning_rate", learning_rate, 0, closed=False)
    if not isinstance(init, np.ndarray) and not (isinstance(init, str) and init == "random"):
        raise ValueError(f"tsne: init must be 'random' or an ndarray [n, n_components] (init='pca' cannot be used with a precomputed "
                         f"matrix), got {init!r}")
    D = np.asarray(D)
    if D.ndim != 2:
        raise ValueError(f"Expected 2D array, got {D.ndim}D array instead")
    if D.shape[0] != D.shape[1]:
        raise ValueError("X should be a square distance matrix")
    n = D.shape[0]
    lib = _lib.load()
    if n > lib.gte_tsne_max_n():
        raise ValueError(f"t-SNE of {n} samples: the kernels take {lib.gte_tsne_max_n()}")
    if d > lib.gte_tsne_max_components():
        raise ValueError(f"t-SNE with {d} components: the kernels take {lib.gte_tsne_max_components()}")
    if n < 2:
        raise ValueError(f"t-SNE needs at least 2 samples, got {n}")
    if perplexity >= n:
        raise ValueError(f"perplexity ({perplexity}) must be less than n_samples ({n})")
    if D.dtype not in (np.float32, np.float64):
        D = D.astype(np.float64)
    if not np.isfinite(D).all():
        raise ValueError("Input X contains NaN or infinity.")
    if (D < 0).any():
        raise ValueError("Negative values in data passed to TSNE.fit(). With metric='precomputed', X should contain positive distances.")
    with np.errstate(over="ignore"):
        sq_dist = (D ** 2).astype(np.float32, copy=False)                  # (_fit: distances **= 2; _joint_probabilities: the cast)
    if not np.isfinite(sq_dist).all():
        raise ValueError("tsne: a squared distance does not fit float32")
    if isinstance(learning_rate, str):
        learning_rate = float(np.maximum(n / early_exaggeration / 4, 50))
    if isinstance(init, np.ndarray):
        if init.shape != (n, d) or not np.isfinite(init).all():
            raise ValueError(f"tsne: init must be a finite [{n}, {d}] array, got shape {init.shape}")
        y0 = init.astype(np.float64)
    else:
        y0 = (1e-4 * check_random_state(random_state).standard_normal(size=(n, d)).astype(np.float32)).astype(np.float64)
    return Prepared(np.ascontiguousarray(sq_dist), np.ascontiguousarray(y0), perplexity, early_exaggeration, learning_rate, max_iter,
                    n_iter_without_progress, min_grad_norm)


def phases(prepared: Prepared, first_end=None):
    """``(first iteration or None, end, momentum, exaggeration, n_iter_without_progress)`` of the two calls of ``_gradient_descent``
    in ``TSNE._tsne``; the second starts behind the last iteration of the first (None: known only then)."""
    return ((0, EXPLORATION_ITER, 0.5, prepared.early_exaggeration, EXPLORATION_ITER),
            (first_end, prepared.max_iter, 0.8, 1.0, prepared.n_iter_without_progress))


def run(prepared: Prepared, device=None):
    """The device stages: one upload of the squared distances and the init, ``tsne_cond_p`` -> ``tsne_joint_p``, then the two
    phases.  Inside a phase the host enqueues up to the next check iteration (every 50th) or the phase end and reads the 64-byte
    state back there: the one synchronisation per 50 iterations.  Returns ``(Y float64 [n, d], info)``, ``info`` =
    ``{'kl_divergence', 'n_iter', 'learning_rate', 'stop_reason'}``."""
    import torch
    from ... import graph as G
    device = _lib.default_device(device)
    if device.type != "cuda":
        _lib.require_device(torch.empty(0, device=device), "tsne.run")
    n, d = prepared.init.shape
    with torch.cuda.device(device):
        ws = G.tsne_workspace(n, device)
        C, _ = G.tsne_cond_p(torch.from_numpy(prepared.sq_dist).to(device), prepared.perplexity)
        P = G.tsne_joint_p(C, ws)
        del C
        Y = torch.zeros((2, n, d), dtype=torch.float64, device=device)
        Y[0].copy_(torch.from_numpy(prepared.init))
        update = torch.empty((n, d), dtype=torch.float64, device=device)
        gains = torch.empty((n, d), dtype=torch.float64, device=device)
        big = float(np.finfo(float).max)
        it, cur, error, reason = 0, 0, big, 0
        for first, end, momentum, exaggeration, patience in phases(prepared):
            first = it if first is None else first
            if first >= end:
                continue
            update.zero_()
            gains.fill_(1.0)
            state = torch.tensor([first, 0, 0, first, cur, big, big, 0], dtype=torch.float64, device=device)
            it, stopped = first, 0
            while not stopped and it < end:
                upto = min((it // CHECK_EVERY + 1) * CHECK_EVERY, end)
                G.tsne_iterate(P, Y, update, gains, prepared.learning_rate, momentum, exaggeration, patience, prepared.min_grad_norm,
                               end, upto - it, ws, state)
                it, stopped, reason, _, cur, error, _, _ = state.tolist()
                it, cur = int(it), int(cur)
        out = Y[cur].cpu().numpy()
    return out, {"kl_divergence": float(error), "n_iter": it - 1, "learning_rate": prepared.learning_rate,
                 "stop_reason": STOP_REASONS[int(reason)]}


def tsne(D, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
         n_iter_without_progress=300, min_grad_norm=1e-7, init="random", random_state=None, device=None, return_info=False):
    """``TSNE(n_components, method='exact', metric='precomputed', init=init, ...).fit_transform(D)`` on the HIP device: ``prepare``
    -> ``run``.  ``D`` [n, n]: distances, squared here as scikit-learn squares them.  Returns the float64 [n, n_components]
    embedding and, with ``return_info``, ``{'kl_divergence', 'n_iter', 'learning_rate'}`` behind it (``kl_divergence_``, ``n_iter_``
    and ``learning_rate_`` of the estimator).  ``device``: the HIP device (None: the current one).  ``ValueError`` before any
    device call for what ``prepare`` rejects.  The exact method takes any ``n_components`` up to ``gte_tsne_max_components()``:
    the limit of 3 is Barnes-Hut's."""
    prepared = prepare(D, n_components, perplexity=perplexity, early_exaggeration=early_exaggeration, learning_rate=learning_rate,
                       max_iter=max_iter, n_iter_without_progress=n_iter_without_progress, min_grad_norm=min_grad_norm, init=init,
                       random_state=random_state)
    Y, info = run(prepared, device)
    if return_info:
        return Y, {k: info[k] for k in ("kl_divergence", "n_iter", "learning_rate")}
    return Y
