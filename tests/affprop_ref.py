"""Affinity propagation in numpy, written from the contract of gte_affprop_iterate in include/gte.h: the oracle of
tests/test_gpu_affprop.py, pinned on scikit-learn itself by tests/test_affprop_ref_cpu.py.  One sweep follows the formulas there
operation by operation; the column sum is an explicit row-by-row accumulation.  ``prepare`` and ``finish`` restate what
scikit-learn does around its loop.  Nothing of the package is imported.  The inputs that the CPU and the GPU tests share are made
here as well, and the reference runs are cached: each is computed once per process."""
import functools
import random
import warnings

import numpy as np

from tests import lev_ref

SIGNS = "wx.,-%()/"
SEED = 7                                                                   # random_state of every case


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def sweep(S, A, R, d, omd, last_index=False, strict_second=False):
    """One sweep in place on A and R; returns E.  Two deliberately different rules for the tie test: ``last_index`` takes the
    LAST index of the maximum, ``strict_second`` takes as Y2 the largest entry strictly below Y."""
    n = S.shape[0]
    ind = np.arange(n)
    t = A + S
    I = n - 1 - np.argmax(t[:, ::-1], axis=1) if last_index else np.argmax(t, axis=1)
    Y = t[ind, I]
    t[ind, I] = -np.inf
    if strict_second:
        t[t == Y[:, None]] = -np.inf
    Y2 = t.max(axis=1)
    new = S - Y[:, None]
    new[ind, I] = S[ind, I] - Y2
    R[...] = (R * d) + (new * omd)
    Rp = np.where(R > 0, R, 0.0)
    Rp[ind, ind] = R[ind, ind]
    cs = Rp[0].copy()
    for i in range(1, n):                                                  # strictly in row order
        cs = cs + Rp[i]
    u = Rp - cs
    dia = u[ind, ind].copy()
    u = np.where(u > 0, u, 0.0)
    u[ind, ind] = dia
    A[...] = (A * d) - (u * omd)
    return (A[ind, ind] + R[ind, ind]) > 0


class Run:
    """The iteration with its stop rule.  ``advance(k)`` performs up to k more sweeps, fewer when it stops: what k enqueued
    sweeps leave on the device.  ``state()`` = (n_iter_done, stopped, converged, K)."""

    def __init__(self, S, damping, convergence_iter, max_iter, last_index=False, strict_second=False):
        n = S.shape[0]
        self.S, self.d, self.omd = np.array(S, dtype=np.float64), float(damping), 1.0 - float(damping)
        self.ci, self.max_iter, self.rule = int(convergence_iter), int(max_iter), (last_index, strict_second)
        self.A, self.R = np.zeros((n, n)), np.zeros((n, n))
        self.E = np.zeros(n, dtype=bool)
        self.ring = np.zeros((self.ci, n), dtype=np.int64)
        self.done, self.stopped, self.converged, self.K = 0, 0, 0, 0

    def advance(self, sweeps):
        n = self.S.shape[0]
        for _ in range(sweeps):
            if self.stopped or self.done >= self.max_iter:
                break
            it = self.done
            self.E = sweep(self.S, self.A, self.R, self.d, self.omd, *self.rule)
            self.ring[it % self.ci] = self.E
            self.K = int(self.E.sum())
            self.done = it + 1
            se = self.ring.sum(axis=0)
            if it >= self.ci and int(((se == self.ci) | (se == 0)).sum()) == n and self.K > 0:
                self.stopped, self.converged = 1, 1
            elif self.done >= self.max_iter:
                self.stopped = 1
        return self

    def state(self):
        return [self.done, self.stopped, self.converged, self.K]

    def snapshot(self):
        return {"A": self.A.copy(), "R": self.R.copy(), "E": self.E.copy(), "state": self.state()}


def check_random_state(seed):
    if seed is None:
        return np.random.mtrand._rand
    return seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)


def prepare(S, preference=None, random_state=None):
    """(the noisy matrix, None) or (None, (centers, labels, 0)) for the degenerate inputs, as scikit-learn treats them."""
    S = np.array(S, dtype=np.float64)
    n = S.shape[0]
    preference = np.asarray(np.median(S) if preference is None else preference, dtype=np.float64)
    off = S[~np.eye(n, dtype=bool)]
    if n == 1 or (np.all(preference == preference.flat[0]) and np.all(off == off[0])):
        warnings.warn("All samples have mutually equal similarities. Returning arbitrary cluster center(s).")
        if preference.flat[0] > S.flat[n - 1]:
            return None, (np.arange(n), np.arange(n), 0)
        return None, (np.array([0]), np.array([0] * n), 0)
    S.flat[::n + 1] = preference
    rs = check_random_state(random_state)
    S += (np.finfo(np.float64).eps * S + np.finfo(np.float64).tiny * 100) * rs.standard_normal(size=(n, n))
    return S, None


def finish(S, E):
    """(centers, labels) from the exemplars of the last sweep (no warnings here)."""
    n = S.shape[0]
    I = np.flatnonzero(E)
    K = I.size
    if K == 0:
        return np.empty(0, dtype=np.intp), np.full(n, -1)
    c = np.argmax(S[:, I], axis=1)
    c[I] = np.arange(K)
    for k in range(K):
        ii = np.flatnonzero(c == k)
        I[k] = ii[np.argmax(S[np.ix_(ii, ii)].sum(axis=0))]
    c = np.argmax(S[:, I], axis=1)
    c[I] = np.arange(K)
    labels = I[c]
    centers = np.unique(labels)
    return centers, np.searchsorted(centers, labels)


def affinity_propagation(S, preference=None, convergence_iter=15, max_iter=200, damping=0.5, random_state=None):
    """(centers, labels, n_iter) end to end on the reference sweep."""
    noisy, result = prepare(S, preference, random_state)
    if noisy is None:
        return result
    run = Run(noisy, damping, convergence_iter, max_iter).advance(max_iter)
    return (*finish(noisy, run.E), run.done)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blobs(n, seed=0):
    """Negative squared distances of n points around three 2-D centres."""
    rng = np.random.default_rng(1000 * seed + n)
    centres = np.array([[0.0, 0.0], [6.0, 1.0], [2.0, 7.0]])
    x = centres[rng.integers(0, 3, n)] + rng.normal(size=(n, 2))
    diff = x[:, None, :] - x[None, :, :]
    S = -(diff * diff).sum(axis=2)
    S.setflags(write=False)
    return S


def shape_words(n, seed=0):
    rnd, words = random.Random(1000 * seed + n), []
    while len(words) < n:
        w = "".join(rnd.choice(SIGNS) for _ in range(rnd.randint(1, 6)))
        if w not in words:
            words.append(w)
    return words


@functools.lru_cache(maxsize=None)
def lev(n, seed=0):
    """Negative unit-cost Levenshtein distances of n distinct random shape words."""
    S = lev_ref.similarity(shape_words(n, seed), lev_ref.uniform())
    S.setflags(write=False)
    return S


def small_rc(n=50, seed=3):
    """Representation counts for train_repr (the generator of tests/test_lev_host.py)."""
    rnd = random.Random(seed)
    rc = {}
    while len(rc) < n - 1:
        rc.setdefault("".join(rnd.choice(SIGNS) for _ in range(rnd.randint(1, 6))), rnd.randint(1, 40))
    items = list(rc.items())
    items.insert(n // 2, ("<UNK_W>", 1))
    return dict(items)


FAMILIES = {"blobs": blobs, "lev": lev}


def asymmetric2():
    """2 x 2 with different off-diagonal entries: not degenerate, so the sweeps run."""
    return np.array([[0.0, -1.0], [-3.0, 0.0]])


def preference_ramp(n):
    """An array-valued preference: one value per sample, none equal."""
    return -np.linspace(2.0, 30.0, n)


class Case:
    """One problem: family, n, damping, convergence_iter, max_iter, preference ('median' or 'ramp')."""

    def __init__(self, family, n, damping, ci, max_iter=200, preference="median"):
        self.family, self.n, self.damping, self.ci, self.max_iter, self.preference = family, n, damping, ci, max_iter, preference

    @property
    def id(self):
        tail = "" if self.preference == "median" else f"-{self.preference}"
        return f"{self.family}-n{self.n}-d{self.damping}-c{self.ci}-m{self.max_iter}{tail}"

    def S(self):
        return asymmetric2() if self.family == "asym" else FAMILIES[self.family](self.n)

    def pref(self):
        return None if self.preference == "median" else preference_ramp(self.n)

    def noisy(self):
        return _noisy(self.family, self.n, self.preference)

    def reference(self):
        """Snapshots of the reference after 1, 2, convergence_iter and max_iter REQUESTED sweeps (keys: those counts)."""
        return _reference(self.family, self.n, self.damping, self.ci, self.max_iter, self.preference)

    def requests(self):
        return sorted({1, 2, self.ci, self.max_iter})


@functools.lru_cache(maxsize=None)
def _noisy(family, n, preference):
    case = Case(family, n, 0.5, 3, preference=preference)
    noisy, result = prepare(case.S(), case.pref(), SEED)
    assert result is None
    noisy.setflags(write=False)
    return noisy


@functools.lru_cache(maxsize=None)
def _reference(family, n, damping, ci, max_iter, preference):
    case = Case(family, n, damping, ci, max_iter, preference)
    run, out, done = Run(case.noisy(), damping, ci, max_iter), {}, 0
    for total in case.requests():
        run.advance(total - done)
        done = total
        out[total] = run.snapshot()
    return out


SIZES = (3, 63, 64, 65, 130, 257)
GRID = [Case(f, n, d, c) for f in ("blobs", "lev") for n in SIZES for d in (0.5, 0.9) for c in (3, 15)]
TWO = [Case("asym", 2, d, c) for d in (0.5, 0.9) for c in (3, 15)]
# cut short: fewer sweeps than the problem needs (the tests assert that the full run needs more); K = 0: two sweeps of a damped
# start leave no exemplar (asserted there as well); an array-valued preference
CUT_SHORT = [Case("lev", 130, 0.9, 15, max_iter=30), Case("blobs", 65, 0.9, 15, max_iter=40)]
NO_EXEMPLAR = [Case("blobs", 65, 0.9, 15, max_iter=20), Case("blobs", 64, 0.9, 3, max_iter=2)]
RAMP = [Case("lev", 65, 0.9, 15, preference="ramp"), Case("blobs", 130, 0.5, 3, preference="ramp")]
CASES = GRID + TWO + CUT_SHORT + NO_EXEMPLAR + RAMP
