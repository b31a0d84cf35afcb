"""CPU-only: tests/boxeval_float_ref.py against the reference's own answers on float documents
(tests/golden/boxeval_float_cases.json, written by tools/make_boxeval_float_golden.py), mutants of the IoU that the stored bits
must catch, and hand cases."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import boxeval_float_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxeval_float_cases.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _pairs(golden):
    """every (prediction, ground truth, stored IoU) of every paired cell"""
    for case in golden["cases"]:
        for kind, pages in case["iou"].items():
            for page, m in pages.items():
                for p, row in zip(case["pred"][kind][page]["bboxes"], m):
                    for t, v in zip(case["gt"][kind][page], row):
                        yield p, t, v


def test_the_fixture_is_what_its_generator_describes(golden):
    assert len(golden["cases"]) >= 12 and golden["iou_thrs"] == [float(t) for t in np.linspace(0.5, 0.95, 10)]
    assert os.path.getsize(GOLDEN) < 160 * 1024
    stored = list(_pairs(golden))
    assert len(stored) > 800 and sum(v > 0.5 for _, _, v in stored) > 150
    boxes = [b for case in golden["cases"] for e in case["pred"]["table"].values() for b in e["bboxes"]]
    assert any(v != int(v) for b in boxes for v in b)                    # floats: an integer cast would truncate them
    assert all(len(e["scores"]) <= 8 for case in golden["cases"] for k in case["pred"].values() for e in k.values())


def test_the_restatement_reproduces_every_stored_iou_bit_for_bit(golden):
    n = 0
    for p, t, v in _pairs(golden):
        assert ref.iou(p, t) == v, (p, t)
        n += 1
    assert n > 800
    for case in golden["cases"]:
        for kind, pages in case["iou"].items():
            for page, m in pages.items():
                assert ref.iou_matrix(case["pred"][kind][page]["bboxes"], case["gt"][kind][page]).tolist() == m


def test_the_restatement_reproduces_every_curve(golden):
    for case in golden["cases"]:
        for kind in golden["kinds"]:
            for j, t in enumerate(golden["iou_thrs"]):
                got = ref.avg_precision_at_iou(case["gt"][kind], case["pred"][kind], t)
                assert got["precisions"] == case["ref"][kind]["precisions"][j] and got["recalls"] == case["ref"][kind]["recalls"][j]
                assert abs(got["avg_prec"] - case["ref"][kind]["avg_prec"][j]) <= 1e-12
        doc = ref.evaluate_doc_ref(case["pred"], case["gt"])
        assert doc["table"]["precisions"] == case["ref"]["table"]["precisions"]


def _fma(a, b, c):
    """a * b + c with ONE rounding (float(Fraction) rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _iou_parts(p, t):
    px0, py0, px1, py1 = p
    tx0, ty0, tx1, ty1 = t
    w, h = (min(tx1, px1) - max(tx0, px0)) + 1.0, (min(ty1, py1) - max(ty0, py0)) + 1.0
    return w, h, ((tx1 - tx0) + 1.0) * ((ty1 - ty0) + 1.0), ((px1 - px0) + 1.0) * ((py1 - py0) + 1.0)


def _iou_union_contracted(p, t):
    """what a compiler left to contract makes of (true_area + pred_area) - w * h: the product never rounds"""
    w, h, ta, pa = _iou_parts(p, t)
    return (w * h) / _fma(-w, h, ta + pa)


def _iou_one_after_the_product(p, t):
    """the + 1 applied to the product, not to the extents"""
    px0, py0, px1, py1 = p
    tx0, ty0, tx1, ty1 = t
    inter = (min(tx1, px1) - max(tx0, px0)) * (min(ty1, py1) - max(ty0, py0)) + 1.0
    ta, pa = (tx1 - tx0) * (ty1 - ty0) + 1.0, (px1 - px0) * (py1 - py0) + 1.0
    return inter / ((ta + pa) - inter)


@pytest.mark.parametrize("mutant", [_iou_union_contracted, _iou_one_after_the_product], ids=lambda f: f.__name__)
def test_a_mutant_of_the_iou_misses_stored_bits(golden, mutant):
    overlapping = [(p, t, v) for p, t, v in _pairs(golden) if v > 0.0]
    missed = sum(mutant(p, t) != v for p, t, v in overlapping)
    print(f"{mutant.__name__}: {missed} of {len(overlapping)} stored IoUs missed")
    assert missed >= 1
    assert all(ref.iou(p, t) == v for p, t, v in overlapping)


def test_hand_cases_touching_threshold_equality_and_a_shared_tie():
    assert ref.iou([0, 0, 10, 10], [10, 0, 20, 10]) == 11 / 231                          # touching boxes overlap
    assert ref.iou([0.0, 0.0, 10.0, 10.0], [10.25, 0.0, 20.0, 10.0]) == 0.0              # a quarter pixel apart: disjoint
    assert ref.iou([0, 0, 9, 9], [0, 0, 9, 4]) == 0.5                                    # 50 / 100
    assert ref.match_count([[0, 0, 9, 9]], [[0, 0, 9, 4]], 0.5) == 0                     # iou == thr is no match
    assert ref.match_count([[0, 0, 9, 9]], [[0, 0, 9, 4]], 0.4999) == 1
    # prediction 0 ties on both ground truths (IoU 0.5 each); the larger pair index (ground truth 1) takes it, which leaves
    # ground truth 0 without a partner at 0.45 -- the other order would match both predictions
    pred, gt = [[0.0, 0.0, 9.0, 19.0], [0.0, 10.0, 9.0, 39.0]], [[0.0, 0.0, 9.0, 9.0], [0.0, 10.0, 9.0, 19.0]]
    m = ref.iou_matrix(pred, gt)
    assert m[0, 0] == m[0, 1] == 0.5 and m[1, 0] == 0.0 and 0.3 < m[1, 1] < 0.4
    assert ref.has_shared_tie(pred, gt, 0.3) and ref.candidates(pred, gt, 0.3)[0] == (0.5, 1)
    assert ref.match_count(pred, gt, 0.3) == 1
    tp = ref.box_match_ref(np.asarray(pred), [0, 2], np.asarray(gt), [0, 2], [0.3, 0.45])
    assert tp.tolist() == [[1, 1], [1, 0]]


def test_a_malformed_box_overlaps_nothing():
    good = [0.0, 0.0, 9.0, 9.0]
    for bad in ([float("nan"), 0, 9, 9], [0, 0, float("inf"), 9], [9, 0, 0, 9], [0, 9, 9, 0], [0, 0, 9, 2.0 ** 24 + 2], [-2.0 ** 25, 0, 9, 9]):
        assert ref.iou(bad, good) == 0.0 and ref.iou(good, bad) == 0.0
        assert not ref.iou_matrix([bad, good], [good, bad])[[0, 1], [0, 1]].any()
    assert ref.iou([0, 0, 2.0 ** 24, 9], good) > 0.0                                      # the bound itself is inside
    assert ref.iou_matrix([good], [good])[0, 0] == 1.0


def test_box_match_ref_equals_match_count_after_every_pruning(golden):
    case = golden["cases"][0]
    for kind in golden["kinds"]:
        for page, boxes in case["gt"][kind].items():
            if page not in case["pred"][kind]:
                continue
            pred = case["pred"][kind][page]["bboxes"]
            tp, flat = ref.box_match_ref(pred, [0, len(pred)], boxes, [0, len(boxes)], golden["iou_thrs"], return_iou=True)
            assert flat.tolist() == [v for row in case["iou"][kind][page] for v in row]
            for j, t in enumerate(golden["iou_thrs"]):
                assert tp[j].tolist() == [ref.match_count(pred[k:], boxes, t) for k in range(len(pred))]
