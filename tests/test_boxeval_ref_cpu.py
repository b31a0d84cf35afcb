"""CPU-only: tests/boxeval_ref.py (the oracle of gte_box_match and metrics.evaluate_regions) against the reference's own
answers in tests/golden/boxeval_cases.json (tools/make_boxeval_golden.py: get_avg_precision_at_iou of the reference on generated
documents without order-dependent ties), and hand cases of the rules the fixtures cannot isolate."""
import json
import os

import numpy as np
import pytest

from tests import boxeval_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxeval_cases.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_the_cases_it_is_there_for(golden):
    cases = golden["cases"]
    assert len(cases) >= 30 and len(golden["iou_thrs"]) == 10
    lag = unpaired = equal = empty = 0
    for c in cases:
        for kind in golden["kinds"]:
            gt, pred = c["gt"][kind], c["pred"][kind]
            paired = [p for p in gt if p in pred]
            lag += any(len(set(pred[p]["scores"])) >= 3 for p in paired)
            unpaired += any(p not in gt for p in pred) or (bool(pred) and any(p not in pred for p in gt))
            sets = [set(pred[p]["scores"]) for p in paired]
            equal += any(sets[a] & sets[b] for a in range(len(sets)) for b in range(a + 1, len(sets)))
            empty += bool(gt) and not pred
            for p in paired:
                assert not ref.has_shared_tie(pred[p]["bboxes"], gt[p], golden["iou_thrs"][0])
    assert min(lag, unpaired, equal, empty) >= 5


def test_the_restatement_reproduces_every_fixture(golden):
    for i, c in enumerate(golden["cases"]):
        for kind in golden["kinds"]:
            want = c["ref"][kind]
            for j, thr in enumerate(golden["iou_thrs"]):
                got = ref.avg_precision_at_iou(c["gt"][kind], c["pred"][kind], thr)
                assert got["precisions"] == want["precisions"][j], (i, kind, thr)
                assert got["recalls"] == want["recalls"][j], (i, kind, thr)
                assert abs(got["avg_prec"] - want["avg_prec"][j]) <= 1e-12, (i, kind, thr)


def test_evaluate_doc_ref_is_the_same_numbers_per_kind(golden):
    c = golden["cases"][0]
    out = ref.evaluate_doc_ref(c["pred"], c["gt"], golden["iou_thrs"])
    for kind in golden["kinds"]:
        assert out[kind]["precisions"] == c["ref"][kind]["precisions"] and out[kind]["recalls"] == c["ref"][kind]["recalls"]
        np.testing.assert_allclose(out[kind]["ap"], c["ref"][kind]["avg_prec"], rtol=0, atol=1e-12)
        assert out[kind]["map"] == float(np.mean(out[kind]["ap"]))
    assert out["map"] == float(np.mean([out[k]["map"] for k in golden["kinds"]]))


def test_a_touching_pair_counts_as_overlapping():
    # the boxes share the pixel column x = 10: 1 x 11 pixels of 11 x 11 + 11 x 11 - 11
    assert ref.iou([0, 0, 10, 10], [10, 0, 20, 10]) == 11 / 231
    assert ref.iou([0, 0, 10, 10], [11, 0, 20, 10]) == 0.0
    assert ref.match_count([[0, 0, 10, 10]], [[10, 0, 20, 10]], 0.04) == 1
    assert ref.match_count([[0, 0, 10, 10]], [[11, 0, 20, 10]], 0.0) == 0


def test_iou_equal_to_the_threshold_is_not_a_match():
    # 10 x 10 and 10 x 20 pixels, the first inside the second: IoU = 100 / 200 = 0.5 exactly
    p, t = [0, 0, 9, 9], [0, 0, 9, 19]
    assert ref.iou(p, t) == 0.5
    assert ref.match_count([p], [t], 0.5) == 0
    assert ref.match_count([p], [t], np.nextafter(0.5, 0.0)) == 1


def test_a_tie_that_shares_a_prediction_goes_to_the_larger_pair_index():
    # prediction 0 has IoU 0.5 with both ground truths; prediction 1 overlaps ground truth 1 only, with a smaller IoU.  The tie
    # goes to pair 0 * 2 + 1 (the larger index): prediction 1 finds its only partner taken -> ONE match; the other order gives two
    pred = [[0, 0, 9, 19], [0, 10, 9, 39]]
    gt = [[0, 0, 9, 9], [0, 10, 9, 19]]
    assert ref.iou(pred[0], gt[0]) == ref.iou(pred[0], gt[1]) == 0.5
    assert 0.3 < ref.iou(pred[1], gt[1]) < 0.5 and ref.iou(pred[1], gt[0]) == 0.0
    assert ref.has_shared_tie(pred, gt, 0.3)
    assert [c[1] for c in ref.candidates(pred, gt, 0.3)] == [1, 0, 3]
    assert ref.match_count(pred, gt, 0.3) == 1
    assert ref.match_count(pred[1:], gt, 0.3) == 1        # after pruning prediction 0 the second one matches
    np.testing.assert_array_equal(ref.box_match_ref(pred, [0, 2], gt, [0, 2], [0.3, 0.4]), [[1, 1], [1, 0]])


def test_the_lag_keeps_a_low_box_until_the_pages_next_own_score():
    # page a: scores 0.2 (a stray) and 0.9 (a hit); page b: one hit at 0.5.  At threshold 0.5 page a is NOT re-pruned (0.5 is not
    # one of its scores): its stray still counts as a false positive -> precision 2 / 3, where the textbook sweep gives 1
    gt = {"a": [[0, 0, 9, 9]], "b": [[0, 0, 9, 9]]}
    pred = {"a": {"bboxes": [[0, 0, 9, 9], [50, 50, 59, 59]], "scores": [0.9, 0.2]}, "b": {"bboxes": [[0, 0, 9, 9]], "scores": [0.5]}}
    out = ref.avg_precision_at_iou(gt, pred, 0.5)
    assert out["model_thrs"] == [0.2, 0.5, 0.9]
    assert out["precisions"] == [2 / 3, 2 / 3, 1.0] and out["recalls"] == [1.0, 1.0, 1.0]
    unpaired = ref.avg_precision_at_iou(dict(gt, c=[[0, 0, 5, 5]]), pred, 0.5, count_unpaired=True)
    assert unpaired["recalls"] == [2 / 3, 2 / 3, 2 / 3]


def test_region_scores_ref_on_a_hand_case():
    comp = np.array([0, 0, -1, 3])
    group = np.array([4, 4, -1, 1])
    logits = np.log(np.array([[0.5, 0.25, 0.25], [0.2, 0.4, 0.4], [1.0, 1.0, 1.0], [0.1, 0.6, 0.3]]))
    got = ref.region_scores_ref(comp, group, logits, [-1, 4, 4])
    np.testing.assert_allclose(got, [(0.5 + 0.8) / 2, 0.0, 0.0, 0.0], rtol=0, atol=1e-15)      # kind 1 has no class: score 0
    logits[1, 0] = np.nan
    np.testing.assert_allclose(ref.region_scores_ref(comp, group, logits, [-1, 4, 4])[0], 0.25, rtol=0, atol=1e-15)


def test_the_fast_reference_is_the_definition():
    """box_match_ref (one IoU matrix and one sorted list per cell) against match_count on every pruned suffix; iou_matrix against
    iou() bit for bit.  Boxes from a small lattice: equal IoUs that share a box are frequent."""
    rng = np.random.default_rng(4)
    for _ in range(40):
        r, g = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        x0, y0 = rng.integers(0, 4, r + g) * 5, rng.integers(0, 4, r + g) * 5
        box = np.stack([x0, y0, x0 + rng.integers(4, 12, r + g), y0 + rng.integers(4, 12, r + g)], axis=1)
        pred, gt = box[:r], box[r:]
        m = ref.iou_matrix(pred, gt)
        assert m.shape == (r, g) and all(m[i, j] == ref.iou(pred[i], gt[j]) for i in range(r) for j in range(g))
        thrs = [0.1, 0.3, 0.5]
        want = [[ref.match_count(pred[k:].tolist(), gt.tolist(), t) for k in range(r)] for t in thrs]
        np.testing.assert_array_equal(ref.box_match_ref(pred, [0, r], gt, [0, g], thrs), np.asarray(want, dtype=np.int32).reshape(3, r))
