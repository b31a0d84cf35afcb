"""The block route's evaluation end to end: metrics.evaluate_regions(..., float_boxes=True) against the reference's own curves
(tests/golden/boxeval_float_cases.json), extract_blocks(..., logits=...) against tests/blockscore_ref.py, and
test(..., block_scores=True / block_eval=True)."""
import json
import os

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from gnn_tableextraction_amd.models import model_predict
from gnn_tableextraction_amd.utils import metrics
from tests import blockscore_ref
from tests import boxeval_float_ref as fref
from tests import boxeval_ref as iref
from tests.predict_setup import config_and_weights
from tests.test_gpu_blocks_predict import PLAIN_KEYS, SF, _expected, _pages_with_blocks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxeval_float_cases.json")
BOUND = 2.0 ** -18                                         # tests/test_gpu_block_scores.py: the derived bound of a block's score


def test_evaluate_regions_on_float_boxes_reproduces_the_references_curves_on_every_fixture():
    with open(GOLDEN) as f:
        golden = json.load(f)
    for case in golden["cases"]:
        got = metrics.evaluate_regions(case["pred"], case["gt"], float_boxes=True)
        for kind in golden["kinds"]:
            assert got[kind]["precisions"] == case["ref"][kind]["precisions"] and got[kind]["recalls"] == case["ref"][kind]["recalls"]
            np.testing.assert_allclose(got[kind]["ap"], case["ref"][kind]["avg_prec"], rtol=0, atol=1e-12)
    # the integer path stays what it was: it truncates the same document (tests/boxeval_ref.py casts with int())
    case = golden["cases"][0]
    whole, want = metrics.evaluate_regions(case["pred"], case["gt"]), iref.evaluate_doc_ref(case["pred"], case["gt"])
    assert all(whole[k]["precisions"] == want[k]["precisions"] and whole[k]["recalls"] == want[k]["recalls"] for k in golden["kinds"])
    unpaired = metrics.evaluate_regions(case["pred"], case["gt"], float_boxes=True, count_unpaired=True)
    want = fref.evaluate_doc_ref(case["pred"], case["gt"], count_unpaired=True)
    assert all(unpaired[k]["precisions"] == want[k]["precisions"] and unpaired[k]["recalls"] == want[k]["recalls"] for k in golden["kinds"])


def _want_scores(data, pred, logits, result, rescale=True):
    """the float64 reference of every page's final blocks: word coordinates = the unscaled block / 0.36"""
    out, off = [], 0
    for page, r in zip(data.pages, result):
        n = len(page["bboxs"])
        box = np.asarray(r["blocks"], dtype=np.float64).reshape(-1, 4)
        s, c = blockscore_ref.score_page(page["bboxs"], logits[off:off + n], box if rescale else box / SF, r["labels"], PP.category_class_masks())
        out.append((s, c))
        off += n
    return out


def test_extract_blocks_with_logits_on_20_synthetic_pages_equals_the_references():
    data, pred = _pages_with_blocks(20, 31)
    data.pages[4]["blocks"], data.pages[11]["images"] = [], []
    rng = np.random.default_rng(31)
    n = sum(len(p) for p in pred)
    logits = (2.0 * rng.standard_normal((n, 9))).astype(np.float32)
    logits[np.arange(n), np.concatenate(pred)] += 3.0                                     # the predictions are the arg-max, mostly
    logits[7, 2] = np.nan
    plain = PP.extract_blocks(data, pred, batch_pages=7)
    assert plain == _expected(data, pred) and all("scores" not in r for r in plain)      # without logits nothing changes
    for rescale, batch_pages in ((True, 7), (False, 64)):
        got = PP.extract_blocks(data, pred, batch_pages=batch_pages, rescale=rescale, logits=torch.from_numpy(logits).to(DEV))
        base = _expected(data, pred, rescale=rescale)
        assert [{k: v for k, v in r.items() if k not in ("scores", "n_words")} for r in got] == base
        worst, scored = 0.0, 0
        for r, (s, c) in zip(got, _want_scores(data, pred, logits.astype(np.float64), base, rescale)):
            assert r["n_words"] == c and len(r["scores"]) == len(r["blocks"])
            assert all(isinstance(v, float) for v in r["scores"]) and all(isinstance(v, int) for v in r["n_words"])
            if s:
                worst = max(worst, float(np.abs(np.asarray(r["scores"]) - np.asarray(s)).max()))
            scored += sum(k > 0 for k in c)
        print(f"rescale={rescale}: {scored} blocks with words, max |score - ref| = {worst:.3e}")
        assert worst <= BOUND and scored > 100
        assert all(s == 1.0 for r in got for s, k in zip(r["scores"], r["n_words"]) if k == 0)        # no word: the reference's constant
    doc = PP.blocks_json(data, got)
    assert min(s for kind in doc.values() for e in kind.values() for s in e["scores"]) < 0.9
    with pytest.raises(ValueError, match="logits must be a tensor"):
        PP.extract_blocks(data, pred, logits=torch.from_numpy(logits[:-1]).to(DEV))


def _annotate(data, seed):
    """annotations for every page: its layout blocks in the document's coordinates (points / 0.36) moved by a few quarter pixels,
    as TEXT, TABLE or FIGURE rows [x0, y0, x1, y1, category]"""
    rng = np.random.default_rng(seed)
    for page in data.pages:
        rows = []
        for b in page["blocks"]:
            q = np.round(np.asarray(b) / SF * 4) / 4 + rng.integers(-8, 9, 4) / 4
            rows.append([float(q[0]), float(q[1]), float(max(q[2], q[0])), float(max(q[3], q[1])), int(rng.choice([1, 4, 5]))])
        page["annotations"] = rows


def test_test_entry_point_scores_and_evaluates_the_block_document(tmp_path):
    data, _ = _pages_with_blocks(6, 23)
    _annotate(data, 23)
    cfg, _, logs = config_and_weights(tmp_path, seed=4)

    assert set(model_predict.test(data, cfg, save_predictions=False)) == PLAIN_KEYS      # defaults: the keys it returned before
    plain = model_predict.test(data, cfg, blocks=True)
    assert set(plain) == PLAIN_KEYS | {"blocks"} and all("scores" not in r for r in plain["blocks"])
    doc = json.load(open(tmp_path / "blocks" / f"{logs}.json"))
    assert all(s == 1.0 for kind in doc.values() for e in kind.values() for s in e["scores"])      # defaults: a document of 1.0s

    scored = model_predict.test(data, cfg, block_scores=True)                             # implies blocks
    assert set(scored) == PLAIN_KEYS | {"blocks"}
    strip = lambda rs: [{k: v for k, v in r.items() if k not in ("scores", "n_words")} for r in rs]
    assert strip(scored["blocks"]) == plain["blocks"]
    assert all(len(r["scores"]) == len(r["blocks"]) == len(r["n_words"]) for r in scored["blocks"])
    doc = json.load(open(tmp_path / "blocks" / f"{logs}.json"))
    assert doc == PP.blocks_json(data, scored["blocks"]) and list(doc) == list(PP.CATEGORY_NAMES)
    flat = [s for kind in doc.values() for e in kind.values() for s in e["scores"]]
    assert len(flat) > 6 and min(flat) < 1.0 and all(0.0 <= s <= 1.0 for s in flat)       # the document carries the confidences

    out = model_predict.test(data, cfg, save_predictions=False, block_eval=True)          # implies block_scores and blocks
    assert set(out) == PLAIN_KEYS | {"blocks", "block_eval"}
    assert out["blocks"] == scored["blocks"]
    gt = PP.blocks_gt_json(data)
    assert set(gt) == {"text", "table", "figure"}
    want = fref.evaluate_doc_ref(doc, gt)
    got = out["block_eval"]
    assert set(got) == set(PP.CATEGORY_NAMES) | {"map"} and list(got)[:3] == list(gt)
    for kind in PP.CATEGORY_NAMES:
        assert got[kind]["precisions"] == want[kind]["precisions"] and got[kind]["recalls"] == want[kind]["recalls"], kind
        np.testing.assert_allclose(got[kind]["ap"], want[kind]["ap"], rtol=0, atol=1e-12)
    assert abs(got["map"] - want["map"]) <= 1e-12
    print(f"block_eval: map = {got['map']:.4f}, per kind {[round(got[k]['map'], 4) for k in gt]}")
    mine = model_predict.test(data, cfg, save_predictions=False, block_eval={"text": gt["text"]})      # a ground-truth document of the caller's
    assert mine["block_eval"]["text"]["precisions"] == got["text"]["precisions"] and list(mine["block_eval"])[0] == "text"
    del data.pages[2]["annotations"]
    with pytest.raises(ValueError, match="carries no 'annotations'"):
        model_predict.test(data, cfg, save_predictions=False, block_eval=True)
