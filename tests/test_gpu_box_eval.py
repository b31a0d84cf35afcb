"""The box-level evaluation end to end (metrics.evaluate_regions, test(..., region_scores / box_eval)) against the reference's
own answers (tests/golden/boxeval_cases.json) and tests/boxeval_ref.py."""
import json
import os

import numpy as np
import pytest

from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.models import model_predict
from gnn_tableextraction_amd.utils import metrics
from tests import boxeval_ref as ref
from tests.predict_setup import config_and_weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxeval_cases.json")


def _assert_same_evaluation(got, want, kinds):
    for kind in kinds:
        assert got[kind]["thresholds"] == want[kind]["thresholds"], kind
        assert got[kind]["precisions"] == want[kind]["precisions"], kind
        assert got[kind]["recalls"] == want[kind]["recalls"], kind
        np.testing.assert_allclose(got[kind]["ap"], want[kind]["ap"], rtol=0, atol=1e-12, err_msg=kind)
        assert abs(got[kind]["map"] - want[kind]["map"]) <= 1e-12
    assert abs(got["map"] - want["map"]) <= 1e-12


def test_evaluate_regions_reproduces_the_references_curves_on_every_fixture():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["cases"]) >= 30
    for i, c in enumerate(golden["cases"]):
        out = metrics.evaluate_regions(c["pred"], c["gt"], golden["iou_thrs"])
        for kind in golden["kinds"]:
            assert out[kind]["precisions"] == c["ref"][kind]["precisions"], (i, kind)
            assert out[kind]["recalls"] == c["ref"][kind]["recalls"], (i, kind)
            np.testing.assert_allclose(out[kind]["ap"], c["ref"][kind]["avg_prec"], rtol=0, atol=1e-12, err_msg=f"{i} {kind}")
            assert out[kind]["map"] == float(np.mean(out[kind]["ap"]))
        assert out["map"] == float(np.mean([out[k]["map"] for k in golden["kinds"]]))
    # the pages that only one side knows, counted (not the reference: tests/boxeval_ref.py states the rule)
    c = golden["cases"][0]
    _assert_same_evaluation(metrics.evaluate_regions(c["pred"], c["gt"], golden["iou_thrs"], count_unpaired=True),
                            ref.evaluate_doc_ref(c["pred"], c["gt"], golden["iou_thrs"], count_unpaired=True), golden["kinds"])


def test_test_entry_point_scores_evaluates_and_keeps_the_plain_regions(tmp_path):
    """test(data, config, box_eval=True) on 6 synthetic pages: the regions carry the device's scores, the JSON carries them,
    result['box_eval'] is tests/boxeval_ref.py applied to those regions and the label regions; predictions equal to the labels
    evaluate to AP 1.0; regions=True alone still returns 3-tuples and writes 1.0 scores."""
    data = PrebuiltPages.synthetic(6, in_feats=13)
    cfg, _, logs = config_and_weights(tmp_path)

    out = model_predict.test(data, cfg, box_eval=True)
    assert all(len(t) == 4 and isinstance(t[3], float) and 0.0 < t[3] <= 1.0 for page in out["regions"] for t in page)
    assert sum(len(page) for page in out["regions"]) > 0
    # the scores are the reference's on the device's own logits-free inputs: kinds, boxes and counts are the unscored regions
    plain_regions = PP.extract_regions(data, out["all_pred"], batch_pages=4)
    assert [[t[:3] for t in page] for page in out["regions"]] == plain_regions
    doc = json.load(open(tmp_path / "regions" / f"{logs}.json"))
    assert doc == PP.regions_json(data, out["regions"])
    assert sorted(s for kind in doc.values() for e in kind.values() for s in e["scores"]) == \
        sorted(t[3] for page in out["regions"] for t in page)
    labels = [p.label for p in data.page_arrays]
    gt_doc = PP.regions_gt_json(data, PP.extract_regions(data, labels, batch_pages=4))
    kinds = list(PP.GROUP_NAMES.values())
    assert set(out["box_eval"]) == set(kinds) | {"map"}
    _assert_same_evaluation(out["box_eval"], ref.evaluate_doc_ref(doc, gt_doc), kinds)

    # predictions equal to the labels: every kind that has a region is found completely at every threshold
    label_doc = PP.regions_json(data, PP.extract_regions(data, labels, batch_pages=4))
    perfect = metrics.evaluate_regions(label_doc, gt_doc)
    present = [k for k in kinds if gt_doc[k]]
    assert len(present) >= 2
    for kind in present:
        assert perfect[kind]["ap"] == [1.0] * 10 and perfect[kind]["map"] == 1.0
    _assert_same_evaluation(perfect, ref.evaluate_doc_ref(label_doc, gt_doc), kinds)

    scored = model_predict.test(data, cfg, save_predictions=False, region_scores=True)
    assert scored["regions"] == out["regions"] and set(scored) == set(out) - {"box_eval"}
    unscored = model_predict.test(data, cfg, regions=True)
    assert unscored["regions"] == plain_regions and set(unscored) == set(scored)
    doc1 = json.load(open(tmp_path / "regions" / f"{logs}.json"))
    assert all(s == 1.0 for kind in doc1.values() for e in kind.values() for s in e["scores"])
    assert {k: {p: e["bboxes"] for p, e in v.items()} for k, v in doc1.items()} == {k: {p: e["bboxes"] for p, e in v.items()} for k, v in doc.items()}
