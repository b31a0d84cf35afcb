"""The block route end to end (postprocessing.block_vote / extract_blocks, test(..., blocks=True)) against
tests/blocks_ref.py and the reference's own answers (tests/golden/blocks_cases.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.models import model_predict
from tests import blocks_ref as ref
from tests.predict_setup import config_and_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blocks_cases.json")
SF = 0.36
PLAIN_KEYS = {"accuracy", "accuracy_nodes", "precision", "recall", "f1", "confusion", "all_pred", "all_pred_flat"}


def _pages_with_blocks(n_pages, seed):
    """Synthetic pages that carry layout blocks and images, and predictions that are coherent inside a block's grid cell (so
    the votes name table classes for whole blocks and the assembly has tables to build), a tenth of them flipped."""
    rng = np.random.default_rng(seed)
    data = PrebuiltPages.synthetic(n_pages, in_feats=13)
    pred = []
    for i, page in enumerate(data.pages):
        b = np.asarray(page["bboxs"], dtype=np.int64).reshape(-1, 4)
        page["blocks"] = ref.synthetic_blocks(b, rng)
        page["images"] = [{"bbox": (30.7, 40.2, 200.9, 50.1 + 3 * i)}, [10.0, 700.5, 90.0, 790.9], (5.0, 5.0, 50.0, 15.0)]
        cell = ((b[:, 0] + b[:, 2]) // 2 // 260) * 5 + ((b[:, 1] + b[:, 3]) // 2 // 170) * 7 + i
        p = cell % 9
        flip = rng.random(len(p)) < 0.1
        p[flip] = rng.integers(0, 9, int(flip.sum()))
        pred.append(p)
    return data, pred


def _expected(data, pred, rescale=True):
    """extract_blocks' answer computed on the host: tests/blocks_ref.py's vote, assemble_tables, the figure rule, the rescale."""
    out = []
    for page, p in zip(data.pages, pred):
        cats = [PP.DEFAULT_CLASS_CATEGORY[int(c)] for c in p]
        blocks = [[float(v) for v in b] for b in page["blocks"]]
        word_block, votes, voted = ref.vote_page(page["bboxs"], cats, np.asarray(blocks, dtype=np.float64).reshape(-1, 4) / SF)
        new_blocks, new_labels, headers = PP.assemble_tables(blocks, voted)
        for img in page["images"]:
            box = img["bbox"] if isinstance(img, dict) else img
            if box[3] - box[1] > 10:
                new_blocks.append([int(v) for v in box])
                new_labels.append(5)
        if rescale:
            new_blocks = [[v / SF for v in b] for b in new_blocks]
        out.append({"blocks": new_blocks, "labels": new_labels, "voted_labels": voted, "headers": headers, "word_block": word_block,
                    "votes": votes})
    return out


def test_block_vote_wrapper_equals_the_reference_and_checks_its_arguments():
    rng = np.random.default_rng(21)
    data, pred = _pages_with_blocks(5, 21)
    bbox = np.concatenate([np.asarray(p["bboxs"], dtype=np.int32).reshape(-1, 4) for p in data.pages])
    cats = np.asarray(PP.DEFAULT_CLASS_CATEGORY, dtype=np.int32)[np.concatenate(pred)]
    cats[rng.random(len(cats)) < 0.05] = -1
    blocks = np.concatenate([np.asarray(p["blocks"], dtype=np.float64).reshape(-1, 4) for p in data.pages]) / SF
    node_off = np.concatenate([[0], np.cumsum([len(p["bboxs"]) for p in data.pages])])
    block_off = np.concatenate([[0], np.cumsum([len(p["blocks"]) for p in data.pages])])
    t = lambda a: torch.from_numpy(a).to(DEV)
    got = PP.block_vote(t(bbox), node_off, t(cats), t(blocks), block_off)
    assert isinstance(got, PP.BlockVote) and all(x.is_cuda and x.dtype == torch.int32 for x in got)
    want = ref.vote_batch(bbox, node_off, cats, blocks, block_off)
    np.testing.assert_array_equal(got.word_block.cpu().numpy(), want[0])
    np.testing.assert_array_equal(got.votes.cpu().numpy(), want[1])
    np.testing.assert_array_equal(got.label.cpu().numpy(), want[2])
    assert tuple(got.votes.shape) == (len(blocks), 13) and (want[0] >= 0).sum() > 0.8 * len(bbox) and len(set(want[2].tolist())) > 4
    plain = PP.block_vote(t(bbox), node_off, t(cats), t(blocks), block_off, n_cat=16, double_cat=-1)
    np.testing.assert_array_equal(plain.votes.cpu().numpy(), ref.vote_batch(bbox, node_off, cats, blocks, block_off, 16, -1)[1])

    with pytest.raises(ValueError, match="float64"):
        PP.block_vote(t(bbox), node_off, t(cats), t(blocks.astype(np.float32)), block_off)
    with pytest.raises(ValueError, match="int32"):
        PP.block_vote(t(bbox.astype(np.int64)), node_off, t(cats), t(blocks), block_off)
    with pytest.raises(ValueError, match="word_cat"):
        PP.block_vote(t(bbox), node_off, t(cats[:-1]), t(blocks), block_off)
    with pytest.raises(ValueError, match="do not partition"):
        PP.block_vote(t(bbox), node_off[:-1], t(cats), t(blocks), block_off[:-1])
    with pytest.raises(ValueError, match="n_cat"):
        PP.block_vote(t(bbox), node_off, t(cats), t(blocks), block_off, n_cat=17)
    with pytest.raises(_lib.GteError):
        PP.block_vote(torch.from_numpy(bbox), node_off, t(cats), t(blocks), block_off)
    many = np.tile(np.asarray([[0.0, 0.0, 1.0, 1.0]]), (_lib.load().gte_block_vote_max_page_blocks() + 1, 1))
    with pytest.raises(_lib.GteError, match="exceeds"):
        PP.block_vote(t(bbox[:3]), [0, 3], t(cats[:3]), t(many), [0, len(many)])


def test_extract_blocks_on_20_synthetic_pages_equals_the_host_computation():
    data, pred = _pages_with_blocks(20, 22)
    data.pages[4]["blocks"], data.pages[11]["images"] = [], []
    want = _expected(data, pred)
    assert sum(r["labels"].count(4) for r in want) >= 10 and sum(len(r["headers"]) for r in want) >= 10
    # page 1: both images above 10 high, truncated with int(); page 0's first image is 9.9 high; the third never counts
    assert want[1]["blocks"][-2:] == [[30 / SF, 40 / SF, 200 / SF, 53 / SF], [10 / SF, 700 / SF, 90 / SF, 790 / SF]]
    assert [len(r["labels"]) - len(PP.assemble_tables(p["blocks"], r["voted_labels"])[1])
            for r, p in zip(want[:3] + want[11:12], data.pages[:3] + data.pages[11:12])] == [1, 2, 2, 0]
    assert sum(j < 0 for r in want for j in r["word_block"]) > 20
    got = PP.extract_blocks(data, pred, batch_pages=7)
    assert got == want
    assert PP.extract_blocks(data, pred) == want                               # one batch
    unscaled = PP.extract_blocks(data, pred, batch_pages=3, rescale=False)
    assert unscaled == _expected(data, pred, rescale=False)
    # the arguments in place of the pages' own entries; a map that sends every class to TEXT
    flat = PP.extract_blocks(data, pred, class_category=[1] * 9, blocks=[p["blocks"] for p in data.pages],
                                        images=[[] for _ in data.pages])
    assert all(set(r["voted_labels"]) <= {0, 1} and r["labels"] == r["voted_labels"] and r["headers"] == [] for r in flat)
    assert [r["word_block"] for r in flat] == [r["word_block"] for r in want]


def test_extract_blocks_gives_the_references_objects_for_the_fixture_pages():
    """the golden vote cases as pages: blocks, labels and coordinates of the reference's vote + get_tables_bbox + / sf"""
    with open(GOLDEN) as f:
        cases = [c for c in json.load(f)["votes"] if c["ref"]["objects"] is not None]
    assert len(cases) >= 30
    data = SimpleNamespace(graphs=[None] * len(cases),
                           pages=[{"page": c["name"], "bboxs": c["bboxs"], "blocks": c["blocks"]} for c in cases])
    got = PP.extract_blocks(data, [c["cats"] for c in cases], class_category=list(range(13)), batch_pages=16)
    for r, c in zip(got, cases):
        assert r["blocks"] == c["ref"]["objects"]["blocks"], c["name"]
        assert r["labels"] == c["ref"]["objects"]["labels"], c["name"]
        assert r["voted_labels"] == c["ref"]["labels"] and r["word_block"] == c["ref"]["word_block"], c["name"]
        assert r["votes"] == c["ref"]["counters"], c["name"]
    doc = PP.blocks_json(data, got)
    assert sum(len(e["bboxes"]) for kind in doc.values() for e in kind.values()) == sum(len(c["ref"]["objects"]["blocks"]) for c in cases)


def test_test_entry_point_writes_the_block_document_and_keeps_its_plain_result(tmp_path):
    data, _ = _pages_with_blocks(6, 23)
    cfg, _, logs = config_and_weights(tmp_path, seed=4)

    plain = model_predict.test(data, cfg)
    assert set(plain) == PLAIN_KEYS and not os.path.exists(tmp_path / "blocks")
    out = model_predict.test(data, cfg, blocks=True)
    assert set(out) == PLAIN_KEYS | {"blocks"}
    assert all(np.array_equal(a, b) for a, b in zip(out["all_pred"], plain["all_pred"])) and out["accuracy"] == plain["accuracy"]
    assert out["blocks"] == _expected(data, out["all_pred"])
    assert sum(len(r["blocks"]) for r in out["blocks"]) > 6
    doc = json.load(open(tmp_path / "blocks" / f"{logs}.json"))
    assert doc == PP.blocks_json(data, out["blocks"]) and list(doc) == list(PP.CATEGORY_NAMES)
    assert set(doc["figure"]) == {p["page"] for p in data.pages}
    assert all(s == 1.0 for kind in doc.values() for e in kind.values() for s in e["scores"])
    quiet = model_predict.test(data, cfg, save_predictions=False, blocks=True, regions=True)
    assert quiet["blocks"] == out["blocks"] and set(quiet) == PLAIN_KEYS | {"blocks", "regions"}
    missing = PrebuiltPages.synthetic(6, in_feats=13)
    with pytest.raises(ValueError, match="carries no 'blocks'"):
        model_predict.test(missing, cfg, save_predictions=False, blocks=True)
