"""The one-dimensional self-organising map of ``Preprocessor.train_som``: the reference's ``MiniSom(prototypes, 1, 1)``
(src/components/tables/som/som.py) trained by ``train_random``, restated for a map of x units in a row and one input feature.
Host numpy, and deliberately so: every update reads the weights the previous one wrote and the map is ten numbers wide, so there
is nothing for a device to run in parallel.  The arithmetic is the reference's operation by operation and the random draws are
its ``RandomState`` stream, so the weights are equal, not close (tests/golden/som_cases.json)."""
from __future__ import annotations

import numpy as np


def train_som_1d(data, n_units: int = 10, sigma: float = 0.03, learning_rate: float = 0.3, num_iteration: int = 10000,
                 random_seed=None) -> np.ndarray:
    """float64 [n_units]: the weights of ``MiniSom(n_units, 1, 1, sigma, learning_rate, random_seed=random_seed)`` after
    ``train_random(data, num_iteration)``; ``data`` [n] or [n, 1].  In ``np.random.RandomState(random_seed)``'s stream, as there:
    the weights ``rand(n_units, 1, 1) * 2 - 1``; the ten ``rand`` draws of ``_weight_diff_list`` (used for nothing else); then per
    iteration t one ``randint(len(data))`` for the sample x and
        winner c   = the FIRST index of the minimum of sqrt((x - w) * (x - w))           (``fast_norm``, ``argmin``)
        eta, sig   = learning_rate / (1 + t / (T / 2)),  sigma / (1 + t / (T / 2)),  T = num_iteration   (``asymptotic_decay``)
        g          = exp(-(j - c)^2 / (2 * pi * sig * sig)) * exp(-0 / d) * eta  for unit j  (``_gaussian``: d is NOT 2 sig^2)
        w_j       += g_j * (x - w_j)"""
    data = np.asarray(data, dtype=np.float64).reshape(-1)
    n_units, num_iteration = int(n_units), int(num_iteration)
    if num_iteration < 1:
        raise ValueError("num_iteration must be > 1")                     # (the reference's text; it accepts 1)
    if n_units < 1 or data.shape[0] < 1:
        raise ValueError(f"train_som_1d: needs at least one unit and one sample, got {n_units} units, {data.shape[0]} samples")
    rng = np.random.RandomState(random_seed)
    w = (rng.rand(n_units, 1, 1) * 2 - 1).reshape(n_units)
    rng.rand(10)
    neigx = np.arange(n_units)
    for t in range(num_iteration):
        x = data[rng.randint(len(data))]
        s = x - w
        c = int(np.argmin(np.sqrt(s * s)))
        eta = learning_rate / (1 + t / (num_iteration / 2))
        sig = sigma / (1 + t / (num_iteration / 2))
        d = 2 * np.pi * sig * sig
        ax = np.exp(-np.power(neigx - c, 2) / d)
        ay = np.exp(-np.power(np.arange(1) - 0, 2) / d)
        g = np.outer(ax, ay).reshape(n_units) * eta
        w += g * (x - w)
    return w
