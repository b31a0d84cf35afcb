"""The numeral samples that ``Preprocessor.train_som`` and ``train_gmm`` of the reference work on
(src/components/tables/preprocessor.py:99-114, 142-168), from numeral counts ``nc`` (numeral string -> count).  Counting ``nc`` from
a corpus is NOT restated: the reference's ``Manager`` / ``bs4`` chain is the caller's, as components/tables/vocabulator.py says
for ``rc``.  Host only."""
from __future__ import annotations

import math
import random
from typing import Dict, List, Optional, Tuple

import numpy as np


def to_numeral(token) -> Optional[np.float32]:
    """``np.float32(token)``, or None when that raises ValueError or is NaN or an infinity (src/utils/nums.py:130-138): the
    parse is float32's, so '1e39' is invalid and '16777217' is 16777216."""
    try:
        with np.errstate(over="ignore"):
            num = np.float32(token)
    except ValueError:
        return None
    if num == np.float32("inf") or num == np.float32("-inf") or math.isnan(num):
        return None
    return num


def weighted_log(x):
    """``log(x) + 1`` above 1, ``-(log|x| + 1)`` below -1, ``x`` itself on [-1, 1] (som_interpolate.py:84-96), in the type of
    ``x``: the reference applies it to np.float32 numerals, and so does ``numeral_samples``."""
    if x > 1:
        x = np.log(x) + 1
    elif x < -1:
        x = -1 * (np.log(np.abs(x)) + 1)
    return x


def valid_numerals(nc: Dict[str, int]) -> Tuple[List[str], List[np.float32]]:
    """The keys of ``nc`` that ``to_numeral`` takes, in dictionary order, and their float32 values."""
    keys, values = [], []
    for k in nc:
        v = to_numeral(k)
        if v is not None:
            keys.append(k)
            values.append(v)
    return keys, values


def numeral_samples(nc: Dict[str, int], random_state: int = 42, cap: Optional[int] = 2_000_000, log_space: bool = False) -> np.ndarray:
    """float64 [n]: ``nc`` unfolded in dictionary order (numeral k ``nc[k]`` times, invalid numerals skipped), shuffled by
    ``random.Random(random_state).shuffle`` -- the stream ``random.shuffle`` has after the reference's ``set_seeds(42)`` -- cut to
    the first ``cap`` (None: no cut; ``train_som`` has none), then ``weighted_log`` in float32 when ``log_space``.  The values are
    the reference's float32 numerals, widened exactly."""
    data: List[np.float32] = []
    for k, v in nc.items():
        num = to_numeral(k)
        if num is not None:
            data += [num] * int(v)
    random.Random(random_state).shuffle(data)
    if cap is not None and len(data) > cap:
        data = data[:cap]
    out = np.array(data, dtype=np.float32).reshape(-1)
    if log_space:
        with np.errstate(divide="ignore", invalid="ignore"):             # (weighted_log, all samples at once: the same float32 steps)
            mag = np.log(np.abs(out)) + 1
        out = np.where(out > 1, mag, np.where(out < -1, -1 * mag, out)).astype(np.float32)
    return out.astype(np.float64)
