"""CPU-only: tests/doceval_ref.py, the numpy oracle of the area-weighted document evaluation, against the reference's own recorded
answers (tests/golden/doceval_cases.json, tools/make_doceval_golden.py) and against a direct set formulation."""
import numpy as np
import pytest

from tests import doceval_ref as ref

golden_cases, assert_equals_golden = ref.golden_cases, ref.assert_equals_golden


def test_the_fixture_holds_the_cases_it_was_made_for():
    cases = {c["name"]: c for c in golden_cases()}
    assert len(cases) >= 12 and all(len(c["gt"]) <= 200 for c in cases.values())
    assert {c["n_classes"] for c in cases.values()} >= {1, 2, 9, 13}
    assert cases["non_tp_ahead_of_tp"]["lead_total"] > 0 and cases["tp_ahead_of_non_tp"]["lead_total"] == 0
    assert any("nan" in c["precision"] for c in cases.values()) and any("nan" in c["recall"] for c in cases.values())
    assert any(min(c["tp_area"] + c["fp_area"] + c["fn_area"]) < 0 for c in cases.values())
    assert max(cases["predictions_above_max_gt"]["pred"]) > max(cases["predictions_above_max_gt"]["gt"])


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_oracle_reproduces_the_reference(case):
    area, count, lead = ref.area_confusion(case["gt"], case["pred"], case["bbox"], case["n_classes"])
    assert int(count.sum()) == len(case["gt"]) and int(area.sum()) == int(ref.areas(case["bbox"]).sum())
    assert_equals_golden(ref.doc_prf(area, count, lead, mode="reference"), case)


def test_the_reference_differs_from_docbank_exactly_by_lead():
    """the deletion behaviour is real: on the case built for it the reference's numbers are not the formula's"""
    case = {c["name"]: c for c in golden_cases()}["non_tp_ahead_of_tp"]
    area, count, lead = ref.area_confusion(case["gt"], case["pred"], case["bbox"], case["n_classes"])
    bank = ref.doc_prf(area, count, lead, mode="docbank")
    assert bank["fp_area"].tolist() != case["fp_area"] and bank["fn_area"].tolist() != case["fn_area"]
    assert (bank["fp_area"] - lead[0]).tolist() == case["fp_area"] and (bank["fn_area"] - lead[1]).tolist() == case["fn_area"]
    assert bank["tp_area"].tolist() == case["tp_area"]


def test_docbank_mode_equals_the_set_formulation():
    rng = np.random.default_rng(5)
    for trial in range(40):
        n, C = int(rng.integers(1, 400)), int(rng.integers(1, 17))
        gt, pred, bbox = ref.random_case(rng, n, C, accuracy=float(rng.uniform(0.3, 1.0)))
        area, count, lead = ref.area_confusion(gt, pred, bbox, C)
        got = ref.doc_prf(area, count, lead, mode="docbank")
        tp, fp, fn = ref.docbank_sets(gt, pred, bbox, C)
        assert (got["tp_area"].tolist(), got["fp_area"].tolist(), got["fn_area"].tolist()) == (tp, fp, fn), trial
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.asarray(tp, dtype=np.int64) / (np.asarray(tp, dtype=np.int64) + np.asarray(fp, dtype=np.int64))
        assert np.array_equal(got["precision"], p, equal_nan=True)
        assert int(count.sum()) == n and np.array_equal(np.diagonal(count)[:C], [int(((gt == c) & (pred == c)).sum()) for c in range(C)])


def test_lead_is_zero_when_the_true_positives_come_first():
    rng = np.random.default_rng(6)
    gt, pred, bbox = ref.random_case(rng, 500, 7, accuracy=0.7, outside=0.0)
    order = np.argsort(gt != pred, kind="stable")                                 # every true positive ahead of every other node
    area, count, lead = ref.area_confusion(gt[order], pred[order], bbox[order], 7)
    assert not lead.any() and (gt != pred).sum() > 50
    same = ref.doc_prf(area, count, lead, "reference"), ref.doc_prf(area, count, lead, "docbank")
    assert all(np.array_equal(same[0][k], same[1][k], equal_nan=True) for k in same[0])
    # and the other way round every wrong node of a class that stands in its first t_c positions is lost
    area, count, lead = ref.area_confusion(gt[order[::-1]], pred[order[::-1]], bbox[order[::-1]], 7)
    assert lead.any()
