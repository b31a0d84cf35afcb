"""``model_predict.test(..., doc_eval=True)``: the area-weighted evaluation of the run's own predictions equals
tests/doceval_ref.py on them, and nothing else of the result changes."""
import numpy as np
import pytest

from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.models import model_predict
from tests import doceval_ref as ref
from tests.predict_setup import config_and_weights

pytestmark = pytest.mark.gpu

PLAIN_KEYS = {"accuracy", "accuracy_nodes", "precision", "recall", "f1", "confusion", "all_pred", "all_pred_flat"}


def same(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_doc_eval_of_the_entry_point_equals_the_oracle_and_keeps_the_plain_result(tmp_path, capsys):
    data = PrebuiltPages.synthetic(6, in_feats=13)
    cfg, _, _ = config_and_weights(tmp_path, seed=4)
    plain = model_predict.test(data, cfg, save_predictions=False)
    assert set(plain) == PLAIN_KEYS
    capsys.readouterr()
    out = model_predict.test(data, cfg, save_predictions=False, doc_eval=True)
    printed = capsys.readouterr().out
    assert set(out) == PLAIN_KEYS | {"doc_eval"}
    assert all(same(out[k], plain[k]) for k in PLAIN_KEYS)

    gt = np.concatenate([g.ndata["label"].long().cpu().numpy() for g in data.graphs])
    pred = np.concatenate(out["all_pred"])
    bbox = np.concatenate([np.asarray(p["bboxs"], dtype=np.int64).reshape(-1, 4) for p in data.pages])
    ev = out["doc_eval"]
    C = int(gt.max()) + 1
    assert ev["n_classes"] == C and len(gt) == len(pred) == len(bbox) > 100
    want = ref.area_confusion(gt, pred, bbox, C)
    assert all(np.array_equal(ev[k], w) for k, w in zip(("area", "count", "lead"), want))
    assert int(ev["count"].sum()) == len(gt) and int(ev["area"].sum()) == int(ref.areas(bbox).sum()) > 0
    for mode in ("reference", "docbank"):
        w = ref.doc_prf(*want, mode=mode)
        assert sorted(ev[mode]) == sorted(w)
        assert all(np.array_equal(ev[mode][k], w[k], equal_nan=True) and ev[mode][k].dtype == w[k].dtype for k in w)
    tp, fp, fn = ref.docbank_sets(gt, pred, bbox, C)
    assert (ev["docbank"]["tp_area"].tolist(), ev["docbank"]["fp_area"].tolist(), ev["docbank"]["fn_area"].tolist()) == (tp, fp, fn)
    assert sum(line.startswith("class ") for line in printed.splitlines()) == C

    del data.pages[2]["bboxs"]
    with pytest.raises(ValueError, match="page 2 carries no 'bboxs'"):
        model_predict.test(data, cfg, save_predictions=False, doc_eval=True)
