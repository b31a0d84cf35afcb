"""CPU-only: the limits and argument checks of gte_box_match_f64 and gte_block_scores (every call returns before a launch: the
device pointers are dummies), and the host stages of the block route's evaluation -- region_cells(float_boxes=True),
category_class_masks, pack_final_blocks / attach_block_scores, blocks_json, blocks_gt_json -- on the fixtures, with the CPU
references in place of the launches."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from gnn_tableextraction_amd.utils import metrics
from tests import blocks_ref, blockscore_ref
from tests import boxeval_float_ref as fref

HERE = os.path.dirname(os.path.abspath(__file__))
_P = 0x10000          # a dummy 16-byte aligned address: never dereferenced, no call below reaches a launch
INVALID, UNSUPPORTED = -1, -4


def _match(lib, thr=(0.5, 0.75), **change):
    thr = np.asarray(thr, dtype=np.float64)
    args = dict(pred_box=_P, pred_off=_P, gt_box=_P, gt_off=_P, n_cells=4, max_pred=10, max_gt=10,
                iou_thr=thr.ctypes.data_as(ctypes.c_void_p), n_thr=thr.size, tp=_P, cell_status=_P, iou=None, iou_off=None, stream=None)
    assert set(change) <= set(args)
    args.update(change)
    return lib.gte_box_match_f64(*args.values())


def _scores(lib, **change):
    args = dict(bbox=_P, node_off=_P, logits=_P, ld_logits=9, n_classes=9, block_box=_P, block_off=_P, block_cat=_P, cat_classes=_P,
                n_cat=13, n_pages=3, n_nodes=100, n_blocks=20, max_page_words=50, max_page_blocks=10, score=_P, n_words=_P, stream=None)
    assert set(change) <= set(args)
    args.update(change)
    return lib.gte_block_scores(*args.values())


def test_the_limits():
    lib = _lib.load()
    assert lib.gte_block_scores_max_page_blocks() == 512 and lib.gte_block_scores_max_page_words() == 4096
    assert lib.gte_block_scores_max_classes() == 16 and lib.gte_block_scores_max_categories() == 16
    assert lib.gte_block_scores_max_page_words() * 2 ** 19 <= 2 ** 32 - 1                # the fixed-point sum fits 32 bits


def test_box_match_f64_returns_error_codes_without_launching():
    lib = _lib.load()
    limit = lib.gte_box_match_max_boxes()
    assert _match(lib, n_cells=-1) == INVALID and _match(lib, max_pred=-1) == INVALID and _match(lib, max_gt=-1) == INVALID
    assert _match(lib, n_thr=0) == INVALID and b"box_match_f64" in lib.gte_last_error() and b"thresholds" in lib.gte_last_error()
    assert _match(lib, thr=np.linspace(0.1, 0.9, 17)) == INVALID and b"thresholds" in lib.gte_last_error()
    assert _match(lib, iou_thr=None) == INVALID and b"null" in lib.gte_last_error()
    assert _match(lib, thr=(0.75, 0.5)) == INVALID and b"ascending" in lib.gte_last_error()
    assert _match(lib, thr=(0.5, float("nan"))) == INVALID and _match(lib, thr=(-0.5, 0.5)) == INVALID
    assert _match(lib, max_pred=limit + 1) == UNSUPPORTED and b"exceeds" in lib.gte_last_error()
    assert _match(lib, max_gt=limit + 1) == UNSUPPORTED
    assert _match(lib, max_gt=limit + 1, tp=None) == UNSUPPORTED               # the check that stands first
    for name in ("pred_box", "pred_off", "gt_box", "gt_off", "tp", "cell_status"):
        assert _match(lib, **{name: None}) == INVALID and b"null" in lib.gte_last_error(), name
    assert _match(lib, iou=_P, iou_off=None) == INVALID and b"null" in lib.gte_last_error()        # an IoU output needs its offsets
    assert _match(lib, pred_box=_P + 8) == INVALID and b"aligned" in lib.gte_last_error()            # 16 bytes, not a double's 8
    assert _match(lib, gt_box=_P + 8) == INVALID
    assert _match(lib, iou=_P + 4, iou_off=_P) == INVALID and b"aligned" in lib.gte_last_error()
    assert _match(lib, n_cells=0, cell_status=None) == 0                       # nothing to do
    with pytest.raises(_lib.GteError):
        _lib.check(_match(lib, n_thr=17), "probe")


def test_block_scores_returns_error_codes_without_launching():
    lib = _lib.load()
    for name in ("n_pages", "n_nodes", "n_blocks", "max_page_words", "max_page_blocks"):
        assert _scores(lib, **{name: -1}) == INVALID and b"sizes" in lib.gte_last_error(), name
    assert _scores(lib, n_classes=0) == INVALID and _scores(lib, n_cat=0) == INVALID and b"classes" in lib.gte_last_error()
    assert _scores(lib, n_classes=17, ld_logits=17) == UNSUPPORTED and b"classes exceed" in lib.gte_last_error()
    assert _scores(lib, n_cat=17) == UNSUPPORTED and b"categories exceed" in lib.gte_last_error()
    assert _scores(lib, ld_logits=8) == INVALID and b"stride" in lib.gte_last_error()
    assert _scores(lib, max_page_blocks=513) == UNSUPPORTED and b"blocks exceeds" in lib.gte_last_error()
    assert _scores(lib, max_page_words=4097) == UNSUPPORTED and b"words exceeds" in lib.gte_last_error()
    assert _scores(lib, max_page_words=4097, score=None) == UNSUPPORTED         # the limits stand before the pointers
    for name in ("bbox", "node_off", "logits", "block_box", "block_off", "block_cat", "cat_classes", "score", "n_words"):
        assert _scores(lib, **{name: None}) == INVALID and b"null" in lib.gte_last_error(), name
    assert _scores(lib, bbox=_P + 4) == INVALID and b"aligned" in lib.gte_last_error()
    assert _scores(lib, block_box=_P + 4) == INVALID and _scores(lib, logits=_P + 2) == INVALID
    assert _scores(lib, n_pages=0, n_nodes=0, n_blocks=0, score=None) == 0      # nothing to do
    assert _scores(lib, n_blocks=0, score=None, n_words=None, block_box=None, block_cat=None) == 0       # no block: nothing to write
    with pytest.raises(_lib.GteError, match="exceeds"):
        _lib.check(_scores(lib, max_page_blocks=513), "probe")


def test_the_wrappers_refuse_host_tensors_and_arguments_that_do_not_fit():
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype)
    with pytest.raises(_lib.GteError):
        metrics.box_match(z((1, 4), torch.float64), [0, 1], z((1, 4), torch.float64), [0, 1], [0.5], float_boxes=True)
    with pytest.raises(_lib.GteError):
        PP.block_scores(z((2, 4), torch.int32), [0, 2], z((2, 9), torch.float32), z((1, 4), torch.float64), [0, 1], z(1, torch.int32),
                        PP.category_class_masks())
    data = SimpleNamespace(graphs=[None], pages=[{"page": "a", "bboxs": [[0, 0, 5, 5]], "blocks": [[0.0, 0.0, 9.0, 9.0]]}])
    with pytest.raises(ValueError, match=r"logits must be a tensor \[1 nodes"):
        PP.extract_blocks(data, [[1]], logits=torch.zeros((2, 9)), device="cpu")
    with pytest.raises(ValueError, match="logits must be a tensor"):
        PP.extract_blocks(data, [[1]], logits=np.zeros((1, 9)), device="cpu")
    with pytest.raises(ValueError, match="non-finite"):
        metrics.evaluate_regions({"t": {"p": {"bboxes": [[0.0, 0.0, float("nan"), 9.0]], "scores": [1.0]}}}, {"t": {"p": [[0, 0, 9, 9]]}},
                                 device="cpu", float_boxes=True)


def test_region_cells_keeps_float_boxes_and_refuses_malformed_ones():
    pred = {"table": {"p": {"bboxes": [[10 / 0.36, 20 / 0.36, 300 / 0.36, 400 / 0.36], [0.5, 0.25, 9.75, 9.5]], "scores": [0.5, 0.25]}}}
    gt = {"table": {"p": [[27.75, 55.5, 833.25, 1111.0]], "q": [[0.0, 0.0, 1.0, 1.0]]}}
    cells = metrics.region_cells(pred, gt, float_boxes=True)
    assert cells.pred_box.dtype == np.float64 and cells.gt_box.dtype == np.float64
    assert cells.pred_box.tolist() == [[0.5, 0.25, 9.75, 9.5], [10 / 0.36, 20 / 0.36, 300 / 0.36, 400 / 0.36]]      # ascending score
    assert cells.gt_box.tolist() == gt["table"]["p"] and cells.pred_off == [0, 2] and cells.gt_off == [0, 1]
    plain = metrics.region_cells(pred, gt)                                               # today's path: the integer cast
    assert plain.pred_box.dtype == np.int32 and plain.pred_box.tolist() == [[0, 0, 9, 9], [27, 55, 833, 1111]]
    assert plain.thresholds["table"].tolist() == cells.thresholds["table"].tolist() == [0.25, 0.5]
    empty = metrics.region_cells({}, {}, float_boxes=True)
    assert empty.pred_box.shape == (0, 4) and empty.pred_box.dtype == np.float64
    edge = float(1 << 24)
    metrics.region_cells({"table": {"p": {"bboxes": [[-edge, 0.0, edge, 1.0]], "scores": [1.0]}}}, gt, float_boxes=True)      # the bound is inside
    for bad in ([0.0, 0.0, float("nan"), 1.0], [0.0, 0.0, float("inf"), 1.0], [2.0, 0.0, 1.0, 1.0], [0.0, 2.0, 1.0, 1.0],
                [0.0, 0.0, edge + 2.0, 1.0], [-edge - 2.0, 0.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="table / p: a predicted box"):
            metrics.region_cells({"table": {"p": {"bboxes": [bad], "scores": [1.0]}}}, gt, float_boxes=True)
        with pytest.raises(ValueError, match="table / p: a ground-truth box"):
            metrics.region_cells(pred, {"table": {"p": [bad]}}, float_boxes=True)


def test_the_evaluation_stages_reproduce_the_float_fixtures_with_the_cpu_reference_as_the_launch():
    with open(os.path.join(HERE, "golden", "boxeval_float_cases.json")) as f:
        golden = json.load(f)
    for case in golden["cases"]:
        cells = metrics.region_cells(case["pred"], case["gt"], float_boxes=True)
        tp = fref.box_match_ref(cells.pred_box, cells.pred_off, cells.gt_box, cells.gt_off, golden["iou_thrs"])
        got = metrics.average_precisions(cells, tp)
        for kind in golden["kinds"]:
            assert got[kind]["precisions"] == case["ref"][kind]["precisions"] and got[kind]["recalls"] == case["ref"][kind]["recalls"]
            np.testing.assert_allclose(got[kind]["ap"], case["ref"][kind]["avg_prec"], rtol=0, atol=1e-12)
    # the integer path on the same document truncates the boxes: another answer
    case = golden["cases"][0]
    cells = metrics.region_cells(case["pred"], case["gt"])
    assert cells.pred_box.dtype == np.int32


def test_blocks_json_writes_the_scores_of_a_page_that_has_them():
    data = SimpleNamespace(pages=[{"page": "a.pdf"}, {"page": "b.pdf"}])
    result = [{"blocks": [[1, 2, 3, 4], [5.5, 6.0, 7.25, 8.0], [9.0, 9.0, 10.0, 10.0]], "labels": [1, 4, 1], "scores": [0.25, 0.625, 1.0],
               "n_words": [3, 7, 0]},
              {"blocks": [[0.0, 0.0, 2.0, 2.0]], "labels": [1]}]
    doc = PP.blocks_json(data, result)
    assert list(doc) == list(PP.CATEGORY_NAMES)
    assert doc["text"] == {"a.pdf": {"bboxes": [[1.0, 2.0, 3.0, 4.0], [9.0, 9.0, 10.0, 10.0]], "scores": [0.25, 1.0]},
                           "b.pdf": {"bboxes": [[0.0, 0.0, 2.0, 2.0]], "scores": [1.0]}}
    assert doc["table"] == {"a.pdf": {"bboxes": [[5.5, 6.0, 7.25, 8.0]], "scores": [0.625]}}
    assert json.loads(json.dumps(doc)) == doc


def test_blocks_gt_json_keeps_the_annotations_per_category():
    data = SimpleNamespace(pages=[{"page": "a.pdf", "annotations": [[1, 2, 30, 40, 4], [5.5, 6, 7, 8, 1], [0, 0, 9, 9, 4]]},
                                  {"page": "b.pdf", "annotations": []},
                                  {"page": "c.pdf", "annotations": [[1, 1, 2, 2, 1]]}])
    doc = PP.blocks_gt_json(data)
    assert doc == {"text": {"a.pdf": [[5.5, 6.0, 7.0, 8.0]], "c.pdf": [[1.0, 1.0, 2.0, 2.0]]},
                   "table": {"a.pdf": [[1.0, 2.0, 30.0, 40.0], [0.0, 0.0, 9.0, 9.0]]}}
    assert list(doc) == ["text", "table"]
    with pytest.raises(ValueError, match=r"page 1 \(b.pdf\) carries no 'annotations'"):
        PP.blocks_gt_json(SimpleNamespace(pages=[data.pages[0], {"page": "b.pdf"}]))
    for row in ([1, 2, 3, 4], [1, 2, 3, 4, 13], [1, 2, 3, 4, -1], [1, 2, 3, 4, 1.5]):
        with pytest.raises(ValueError, match="is no"):
            PP.blocks_gt_json(SimpleNamespace(pages=[{"page": "a.pdf", "annotations": [row]}]))


def test_the_block_stages_on_the_fixture_pages_with_the_cpu_references_as_the_launches():
    """pack_blocks -> (tests/blocks_ref.py) -> blocks_to_pages -> pack_final_blocks -> (tests/blockscore_ref.py) ->
    attach_block_scores -> blocks_json, for both settings of rescale: the final blocks enter the score stage in word coordinates."""
    with open(os.path.join(HERE, "golden", "blocks_cases.json")) as f:
        cases = [c for c in json.load(f)["votes"] if c["ref"]["objects"] is not None][:12]
    data = SimpleNamespace(graphs=[None] * len(cases), pages=[{"page": c["name"], "bboxs": c["bboxs"], "blocks": c["blocks"]} for c in cases])
    cats = [c["cats"] for c in cases]
    rng = np.random.default_rng(5)
    masks = PP.category_class_masks(list(range(13)))
    assert masks.tolist() == [1 << k if k != 4 else (1 << 4) | (1 << 7) | (1 << 8) | (1 << 10) for k in range(13)]
    batches = PP.pack_blocks(data, cats, class_category=list(range(13)), batch_pages=5)
    logits = [rng.standard_normal((int(b.node_off[-1]), 13)) for b in batches]
    docs = {}
    for rescale in (True, False):
        out, packed = [], []
        for b, rows in zip(batches, logits):
            vote = blocks_ref.vote_batch(b.bbox, b.node_off, b.word_cat, b.block_box, b.block_off, b.n_cat)
            pages = PP.blocks_to_pages(data, b, *vote, rescale=rescale)
            final = PP.pack_final_blocks(pages, 0.36, rescaled=rescale)
            score, n_words = blockscore_ref.block_scores_ref(b.bbox, b.node_off, rows, final.block_box, final.block_off, final.block_cat, masks)
            out += PP.attach_block_scores(pages, final, score, n_words)
            packed.append(final)
        docs[rescale] = (out, packed)
    (scaled, packed_a), (unscaled, packed_b) = docs[True], docs[False]
    for fa, fb in zip(packed_a, packed_b):                                    # the same launch arguments, bit for bit
        assert fa.block_box.tobytes() == fb.block_box.tobytes() and fa.block_cat.tolist() == fb.block_cat.tolist()
        assert fa.block_box.dtype == np.float64 and fa.block_cat.dtype == np.int32 and fa.block_off.tolist() == fb.block_off.tolist()
    assert packed_a[0].block_box.tolist() == [b for r in scaled[:5] for b in r["blocks"]]          # rescale=True: the output coordinates
    n_blocks = 0
    for r, u, c in zip(scaled, unscaled, cases):
        assert r["blocks"] == c["ref"]["objects"]["blocks"] and r["labels"] == c["ref"]["objects"]["labels"]
        assert r["scores"] == u["scores"] and r["n_words"] == u["n_words"] and len(r["scores"]) == len(r["blocks"]) == len(r["n_words"])
        assert all(isinstance(s, float) and 0.0 <= s <= 1.0 for s in r["scores"]) and all(isinstance(k, int) for k in r["n_words"])
        assert all(s == 1.0 for s, k in zip(r["scores"], r["n_words"]) if k == 0)
        n_blocks += len(r["blocks"])
    assert sum(k > 0 for r in scaled for k in r["n_words"]) > n_blocks // 2
    doc = PP.blocks_json(data, scaled)
    flat = [s for kind in doc.values() for e in kind.values() for s in e["scores"]]
    assert len(flat) == n_blocks and sorted(flat) == sorted(s for r in scaled for s in r["scores"]) and min(flat) < 0.9
