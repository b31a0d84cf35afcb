"""numpy oracle of the area-weighted document evaluation (``metrics.area_confusion`` -> gte_doc_eval, ``metrics.doc_prf``), written
from the contract in include/gte.h and the docstrings of utils/metrics.py -- not from the kernel and not from the reference's text.

With ``P_c`` the nodes predicted ``c`` and ``G_c`` those labelled ``c`` (node order), ``T_c`` their intersection, ``t_c = |T_c|``:
``lead[0][c]`` is the area of the nodes of ``P_c \\ T_c`` at a 0-based position ``< t_c`` within ``P_c`` and ``lead[1][c]`` the same
for ``G_c``: what the reference's evaluate_doc drops from its false positives / negatives besides the true positives."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "doceval_cases.json")


def areas(bbox):
    b = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def area_confusion(gt, pred, bbox, n_classes):
    """-> (area int64 [C+1, C+1], count int64 [C+1, C+1], lead int64 [2, C]); index C = none of the classes."""
    C = int(n_classes)
    gt = np.asarray(gt, dtype=np.int64).reshape(-1)
    pred = np.asarray(pred, dtype=np.int64).reshape(-1)
    a = areas(bbox)
    g = np.where((gt >= 0) & (gt < C), gt, C)
    p = np.where((pred >= 0) & (pred < C), pred, C)
    area = np.zeros((C + 1, C + 1), dtype=np.int64)
    count = np.zeros((C + 1, C + 1), dtype=np.int64)
    np.add.at(area, (g, p), a)
    np.add.at(count, (g, p), 1)
    lead = np.zeros((2, C), dtype=np.int64)
    for c in range(C):
        t = int(count[c, c])
        for side, mine, other in ((0, p, g), (1, g, p)):
            members = np.flatnonzero(mine == c)                     # the list, in node order
            head = members[:t]                                       # positions 0 .. t - 1
            lead[side, c] = a[head[other[head] != c]].sum()
    return area, count, lead


def doc_prf(area, count, lead, mode='reference'):
    """The six arrays of ``metrics.doc_prf``, as a dict."""
    area, lead = np.asarray(area, dtype=np.int64), np.asarray(lead, dtype=np.int64)
    C = area.shape[0] - 1
    tp = np.diagonal(area)[:C].copy()
    fp = area[:, :C].sum(axis=0) - tp
    fn = area[:C, :].sum(axis=1) - tp
    if mode == 'reference':
        fp, fn = fp - lead[0], fn - lead[1]
    elif mode != 'docbank':
        raise ValueError(mode)
    with np.errstate(divide='ignore', invalid='ignore'):
        p = tp / (tp + fp)
        r = tp / (tp + fn)
        f1 = (2 * p * r) / (p + r)
    return {'precision': p, 'recall': r, 'f1': f1, 'tp_area': tp, 'fp_area': fp, 'fn_area': fn}


def docbank_sets(gt, pred, bbox, n_classes):
    """The DocBank sums by python sets, one class at a time: (tp, fp, fn) int lists."""
    a = [int(v) for v in areas(bbox)]
    gt, pred = [int(v) for v in np.asarray(gt).reshape(-1)], [int(v) for v in np.asarray(pred).reshape(-1)]
    out = ([], [], [])
    for c in range(n_classes):
        P = {i for i, v in enumerate(pred) if v == c}
        G = {i for i, v in enumerate(gt) if v == c}
        for acc, nodes in zip(out, (P & G, P - G, G - P)):
            acc.append(sum(a[i] for i in nodes))
    return out


def random_case(rng, n, C, accuracy=0.8, outside=0.05, odd_boxes=0.1):
    """gt, pred int32 [n] and bbox int32 [n, 4]: labels in [0, C) with ``pred == gt`` at about ``accuracy``; a share ``outside``
    of both carries -1, C or C + 5; a share ``odd_boxes`` of the boxes is inverted or empty."""
    gt = rng.integers(0, C, n)
    pred = np.where(rng.random(n) < accuracy, gt, rng.integers(0, C, n))
    for arr in (gt, pred):
        m = rng.random(n) < outside
        arr[m] = rng.choice([-1, C, C + 5], int(m.sum()))
    lo = rng.integers(0, 2000, (n, 2))
    size = rng.integers(1, 300, (n, 2))
    kind = rng.random(n)
    size[kind < odd_boxes] *= -1                                     # both corners inverted: a positive area all the same
    size[(kind >= odd_boxes) & (kind < 1.5 * odd_boxes), 0] *= -1    # one axis inverted: negative
    size[(kind >= 1.5 * odd_boxes) & (kind < 2 * odd_boxes), 1] = 0  # empty
    bbox = np.concatenate([lo, lo + size], axis=1)
    return gt.astype(np.int32), pred.astype(np.int32), np.ascontiguousarray(bbox.astype(np.int32))


def golden_cases():
    """The reference's recorded answers (tools/make_doceval_golden.py)."""
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def assert_equals_golden(got, case):
    """``got`` (a ``doc_prf`` dict, mode 'reference') equals what the reference computed: the areas exactly, precision / recall /
    F1 bit for bit, NaN in the same places."""
    for key in ("tp_area", "fp_area", "fn_area"):
        assert got[key].dtype == np.int64 and got[key].tolist() == case[key], (case["name"], key)
    for key in ("precision", "recall", "f1"):
        want = np.asarray([float(v) for v in case[key]], dtype=np.float64)      # float('nan'), float('inf') for the strings
        assert got[key].dtype == np.float64 and got[key].shape == want.shape, (case["name"], key)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[key]), nan), (case["name"], key)
        assert np.array_equal(got[key][~nan].view(np.int64), want[~nan].view(np.int64)), (case["name"], key, got[key], want)
