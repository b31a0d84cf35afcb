"""Affinity propagation on a precomputed similarity matrix with scikit-learn's results, its sweeps on the HIP device
(csrc/affprop.hip; the sweep is stated in include/gte.h): ``sklearn.cluster.affinity_propagation`` of
sklearn/cluster/_affinity_propagation.py, which ``Preprocessor.train_repr`` of the reference runs through
src/utils/matrixes.py: affinity.  Three public stages, as the extractors of components/graphs/postprocessing.py are built:

  ``prepare``   host: what scikit-learn does before its loop -- checks, the preference, the degenerate cases, the noise
  ``run``       device: the sweeps, in chunks, stopped by the device
  ``finish``    host: exemplars -> centres and labels (n x K work whose result depends on its order)

``prepare`` and ``finish`` touch no device and need no scikit-learn.  Parity with scikit-learn is equality: the noise bits are
numpy's, and every operation of a sweep is rounded as numpy rounds it, the column sums in numpy's order."""
from __future__ import annotations

import numbers
import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np

from ... import _lib

DEGENERATE_TEXT = "All samples have mutually equal similarities. Returning arbitrary cluster center(s)."
NOT_CONVERGED_TEXT = "Affinity propagation did not converge, this model may return degenerate cluster centers and labels."
NO_CENTERS_TEXT = "Affinity propagation did not converge and this model will not have any cluster centers."


class AffinityConvergenceWarning(UserWarning):
    """What scikit-learn reports as ``ConvergenceWarning``: the sweeps ended without a stable exemplar set."""


class Prepared(NamedTuple):
    """Outcome of ``prepare``.  ``S``: the matrix the sweeps run on (preference on the diagonal, noise added), or None when the
    input was degenerate; then ``result`` = (centers, labels, n_iter = 0) is the answer and nothing is to be launched."""
    S: Optional[np.ndarray]
    result: Optional[Tuple[np.ndarray, np.ndarray, int]]


def check_random_state(seed) -> np.random.RandomState:
    """``sklearn.utils.check_random_state``: None is numpy's global generator, an int seeds a fresh one, an instance is used."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def square_float64(S) -> np.ndarray:
    """``S`` as a float64 array; ``ValueError`` unless it is a non-empty square matrix.  (No copy of a float64 array, no pass
    over the values: the size can be judged before anything is allocated.)"""
    S = np.asarray(S)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError(f"The matrix of similarities must be a square array. Got {S.shape} instead.")
    if S.shape[0] < 1:
        raise ValueError("affinity propagation needs at least one sample")
    return S if S.dtype == np.float64 else S.astype(np.float64)


def prepare(S, preference=None, random_state=None) -> Prepared:
    """Everything ``_affinity_propagation`` does ahead of its loop, on a copy of ``S`` (float64): NaN or infinity is a
    ``ValueError``; ``preference`` (a scalar or one value per sample) defaults to ``np.median(S)``; one sample, or equal
    similarities with equal preferences, is answered here with scikit-learn's warning; otherwise the preference goes on the
    diagonal and the noise ``(eps * S + tiny * 100) * rs.standard_normal((n, n))`` is added, ``rs = check_random_state(
    random_state)``.  The generator is not touched in the degenerate case, as there."""
    S = square_float64(S)
    if not np.isfinite(S).all():
        raise ValueError("Input contains NaN or infinity: the similarity matrix must be finite")
    S = S.copy()
    n = S.shape[0]
    preference = np.asarray(np.median(S) if preference is None else preference, dtype=np.float64)
    if preference.ndim > 1 or (preference.ndim == 1 and preference.shape[0] != n):
        raise ValueError(f"preference must be a scalar or hold one value per sample ({n}), got shape {preference.shape}")
    if not np.isfinite(preference).all():
        raise ValueError("preference must be finite")

    def all_equal():
        if not np.all(preference == preference.flat[0]):
            return False
        mask = np.ones(S.shape, dtype=bool)
        np.fill_diagonal(mask, 0)
        off = S[mask]
        return bool(np.all(off == off[0]))

    if n == 1 or all_equal():
        warnings.warn(DEGENERATE_TEXT)
        if preference.flat[0] > S.flat[n - 1]:
            return Prepared(None, (np.arange(n), np.arange(n), 0))
        return Prepared(None, (np.array([0]), np.array([0] * n), 0))
    S.flat[::n + 1] = preference
    rs = check_random_state(random_state)
    S += (np.finfo(S.dtype).eps * S + np.finfo(S.dtype).tiny * 100) * rs.standard_normal(size=(n, n))
    return Prepared(S, None)


def run(S_noisy: np.ndarray, damping: float, convergence_iter: int, max_iter: int, device=None, chunk: int = 16,
        return_messages: bool = False):
    """The sweeps on the HIP device: one upload of ``S_noisy``, zeroed ``A``, ``R``, ring and state, then ``affprop_iterate`` in
    chunks of ``chunk`` sweeps.  After each chunk the 16-byte state is read back (the one synchronisation per chunk) and the
    loop is left when the device has stopped; the sweeps of a chunk that lie behind the stopping one change nothing, so
    ``chunk`` does not change a bit of the result.  Returns ``(E bool [n], n_iter, converged)`` and, with
    ``return_messages``, ``A`` and ``R`` (numpy float64 [n, n]) behind them."""
    import torch
    from ... import graph as G
    S_noisy = np.ascontiguousarray(S_noisy, dtype=np.float64)
    n = S_noisy.shape[0]
    if S_noisy.shape != (n, n) or n < 1:
        raise ValueError(f"affinity.run: S must be a non-empty square matrix, got {S_noisy.shape}")
    if chunk < 1:
        raise ValueError(f"affinity.run: chunk {chunk} < 1")
    device = _lib.default_device(device)
    if device.type != "cuda":
        _lib.require_device(torch.empty(0, device=device), "affinity.run")
    with torch.cuda.device(device):
        S_d = torch.from_numpy(S_noisy if S_noisy.flags.writeable else S_noisy.copy()).to(device)
        A = torch.zeros((n, n), dtype=torch.float64, device=device)
        R = torch.zeros((n, n), dtype=torch.float64, device=device)
        E = torch.zeros(n, dtype=torch.uint8, device=device)
        ws = G.affprop_workspace(n, convergence_iter, device)
        state = torch.zeros(4, dtype=torch.int32, device=device)
        enqueued, stopped = 0, 0
        while not stopped and enqueued < max_iter:
            sweeps = min(int(chunk), max_iter - enqueued)
            G.affprop_iterate(S_d, A, R, damping, convergence_iter, max_iter, sweeps, E, ws, state)
            enqueued += sweeps
            n_iter, stopped, converged, _ = state.tolist()
        out = (E.cpu().numpy().astype(bool), int(n_iter), bool(converged))
        if return_messages:
            out += (A.cpu().numpy(), R.cpu().numpy())
    return out


def finish(S_noisy: np.ndarray, E, converged: bool):
    """Lines 135-170 of scikit-learn's file, on the host: the exemplars ``E`` (bool [n]) of the last sweep -> ``(centers,
    labels)``.  Every sample joins its most similar exemplar, each cluster's exemplar is re-chosen as the member with the
    largest similarity sum inside the cluster, the samples are assigned again, and the labels are made gapless.  No exemplar:
    labels all -1, no centres.  Both endings that scikit-learn reports with a ``ConvergenceWarning`` warn with
    ``AffinityConvergenceWarning`` and the same text."""
    S = S_noisy
    n = S.shape[0]
    I = np.flatnonzero(np.asarray(E))
    K = I.size
    if K == 0:
        warnings.warn(NO_CENTERS_TEXT, AffinityConvergenceWarning)
        return np.empty(0, dtype=np.intp), np.array([-1] * n)
    if not converged:
        warnings.warn(NOT_CONVERGED_TEXT, AffinityConvergenceWarning)
    c = np.argmax(S[:, I], axis=1)
    c[I] = np.arange(K)
    for k in range(K):
        ii = np.asarray(c == k).nonzero()[0]
        j = np.argmax(np.sum(S[ii[:, np.newaxis], ii], axis=0))
        I[k] = ii[j]
    c = np.argmax(S[:, I], axis=1)
    c[I] = np.arange(K)
    labels = I[c]
    centers = np.unique(labels)
    return centers, np.searchsorted(centers, labels)


def check_parameters(n: int, damping: float, convergence_iter: int, max_iter: int) -> None:
    """``ValueError`` for what scikit-learn's parameter validation rejects and for what the kernels do not take; no device call."""
    if not (isinstance(damping, numbers.Real) and 0.5 <= damping < 1.0):
        raise ValueError(f"damping must be a number in [0.5, 1.0), got {damping!r}")
    for name, value in (("convergence_iter", convergence_iter), ("max_iter", max_iter)):
        if not isinstance(value, numbers.Integral) or value < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {value!r}")
    lib = _lib.load()
    if n > lib.gte_affprop_max_n():
        raise ValueError(f"affinity propagation of {n} samples: the kernels take {lib.gte_affprop_max_n()}")
    if convergence_iter > lib.gte_affprop_max_convergence_iter():
        raise ValueError(f"convergence_iter {convergence_iter}: the exemplar ring holds {lib.gte_affprop_max_convergence_iter()} sweeps")


def affinity_propagation(S, *, preference=None, convergence_iter: int = 15, max_iter: int = 200, damping: float = 0.5,
                         random_state=None, device=None, return_n_iter: bool = False):
    """``sklearn.cluster.affinity_propagation(S, ...)`` for a precomputed ``S`` with its return values -- ``(centers, labels)``,
    and ``n_iter`` behind them on request -- equal to scikit-learn's for the same ``random_state``: ``prepare`` -> ``run`` ->
    ``finish``.  ``device``: the HIP device of the sweeps (None: the current one).  ``ValueError`` before any device call for a
    matrix that is not square or not finite, ``damping`` outside [0.5, 1), ``convergence_iter`` or ``max_iter`` below 1, and
    sizes above the kernels' limits (``gte_affprop_max_n()`` samples, ``gte_affprop_max_convergence_iter()`` ring slots).
    Without an exemplar the centres are an empty integer array (scikit-learn: an empty list)."""
    S = square_float64(S)
    check_parameters(S.shape[0], damping, convergence_iter, max_iter)
    prepared = prepare(S, preference=preference, random_state=random_state)
    if prepared.S is None:
        centers, labels, n_iter = prepared.result
    else:
        E, n_iter, converged = run(prepared.S, damping, convergence_iter, max_iter, device)
        centers, labels = finish(prepared.S, E, converged)
    return (centers, labels, n_iter) if return_n_iter else (centers, labels)
