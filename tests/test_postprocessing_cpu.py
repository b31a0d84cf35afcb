"""CPU-only: the host stages of evaluate_regions, extract_blocks and extract_regions composed by hand, with the CPU oracle of the
launch (tests/boxeval_ref.py, blocks_ref.py, regions_ref.py) in its place, against the reference's own answers
(tests/golden/boxeval_cases.json, blocks_cases.json) and the oracles' compacted forms."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.data import synthetic as S
from gnn_tableextraction_amd.utils import metrics
from tests import blocks_ref, boxeval_ref, regions_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _evaluate_on_the_host(pred_doc, gt_doc, iou_thrs, count_unpaired=False):
    cells = metrics.region_cells(pred_doc, gt_doc, count_unpaired)
    tp = boxeval_ref.box_match_ref(cells.pred_box, cells.pred_off, cells.gt_box, cells.gt_off, [float(t) for t in iou_thrs])
    return metrics.average_precisions(cells, tp)


def test_box_evaluation_stages_reproduce_the_references_curves_on_every_fixture():
    with open(os.path.join(GOLDEN, "boxeval_cases.json")) as f:
        golden = json.load(f)
    assert len(golden["cases"]) >= 30
    for i, c in enumerate(golden["cases"]):
        out = _evaluate_on_the_host(c["pred"], c["gt"], golden["iou_thrs"])
        for kind in golden["kinds"]:
            assert out[kind]["precisions"] == c["ref"][kind]["precisions"], (i, kind)
            assert out[kind]["recalls"] == c["ref"][kind]["recalls"], (i, kind)
            np.testing.assert_allclose(out[kind]["ap"], c["ref"][kind]["avg_prec"], rtol=0, atol=1e-12, err_msg=f"{i} {kind}")
            assert out[kind]["map"] == float(np.mean(out[kind]["ap"]))
        assert out["map"] == float(np.mean([out[k]["map"] for k in golden["kinds"]]))
        # the pages that only one side knows, counted (not the reference: tests/boxeval_ref.py states the rule)
        got = _evaluate_on_the_host(c["pred"], c["gt"], golden["iou_thrs"], count_unpaired=True)
        want = boxeval_ref.evaluate_doc_ref(c["pred"], c["gt"], golden["iou_thrs"], count_unpaired=True)
        for kind in golden["kinds"]:
            assert got[kind]["thresholds"] == want[kind]["thresholds"], (i, kind)
            assert got[kind]["precisions"] == want[kind]["precisions"], (i, kind)
            assert got[kind]["recalls"] == want[kind]["recalls"], (i, kind)
            np.testing.assert_allclose(got[kind]["ap"], want[kind]["ap"], rtol=0, atol=1e-12, err_msg=f"{i} {kind}")
            assert abs(got[kind]["map"] - want[kind]["map"]) <= 1e-12
        assert abs(got["map"] - want["map"]) <= 1e-12


def test_block_stages_give_the_references_objects_for_the_fixture_pages():
    """the golden vote cases as pages, 16 to a batch: blocks, labels and coordinates of the reference's vote + get_tables_bbox + / sf"""
    with open(os.path.join(GOLDEN, "blocks_cases.json")) as f:
        cases = [c for c in json.load(f)["votes"] if c["ref"]["objects"] is not None]
    assert len(cases) >= 30
    data = SimpleNamespace(graphs=[None] * len(cases),
                           pages=[{"page": c["name"], "bboxs": c["bboxs"], "blocks": c["blocks"]} for c in cases])
    batches = PP.pack_blocks(data, [c["cats"] for c in cases], class_category=list(range(13)), batch_pages=16)
    assert len(batches) >= 2 and [len(b.ids) for b in batches[:-1]] == [16] * (len(batches) - 1)
    got = []
    for b in batches:
        assert b.block_box.dtype == np.float64 and b.bbox.dtype == np.int32 and b.word_cat.dtype == np.int32
        vote = blocks_ref.vote_batch(b.bbox, b.node_off, b.word_cat, b.block_box, b.block_off, b.n_cat, 2)
        got += PP.blocks_to_pages(data, b, *vote)
    assert len(got) == len(cases)
    for r, c in zip(got, cases):
        assert r["blocks"] == c["ref"]["objects"]["blocks"], c["name"]
        assert r["labels"] == c["ref"]["objects"]["labels"], c["name"]
        assert r["voted_labels"] == c["ref"]["labels"] and r["word_block"] == c["ref"]["word_block"], c["name"]
        assert r["votes"] == c["ref"]["counters"], c["name"]
    doc = PP.blocks_json(data, got)
    assert sum(len(e["bboxes"]) for kind in doc.values() for e in kind.values()) == sum(len(c["ref"]["objects"]["blocks"]) for c in cases)


@pytest.fixture(scope="module")
def six_pages():
    """6 synthetic pages with their labels as predictions, and tests/regions_ref.py's answer on the pages' own arrays."""
    data = PrebuiltPages.synthetic(6, in_feats=13)
    src, dst, _, _, label, off = S.concat_pages(data.page_arrays)
    bbox = np.concatenate([p.bbox for p in data.page_arrays]).astype(np.int32)
    group = np.asarray(PP.DEFAULT_CLASS_GROUP, dtype=np.int32)[label.astype(np.int64)]
    indptr, indices = regions_ref.in_csr(src, dst, int(off[-1]))
    return data, off, group, regions_ref.page_regions_ref(indptr, indices, off, group, bbox)


@pytest.mark.parametrize("min_words", [1, 2])
def test_region_stages_equal_the_union_find_on_6_synthetic_pages(six_pages, min_words):
    """4 pages to a batch: the batch's in-CSR, kinds and boxes as stage one packs them go through tests/regions_ref.py, its
    full-length answer is compacted as page_regions compacts the device's, and stage three lists it."""
    data, all_off, all_group, all_ref = six_pages
    got = []
    for ids, g, group, bbox in PP.region_batches(data, [p.label for p in data.page_arrays], batch_pages=4, device="cpu"):
        assert g.ndata == {} and g.edata == {} and group.dtype == torch.int32 and tuple(bbox.shape) == (g.num_nodes(), 4)
        csr, off = g.in_csr(), np.concatenate([[0], np.cumsum(g.batch_num_nodes_)])
        comp, box, count = regions_ref.page_regions_ref(csr.indptr.numpy(), csr.indices.numpy(), off, group.numpy(), bbox.numpy())
        root = np.nonzero(count)[0]
        reg = PP.PageRegions(*(torch.from_numpy(a) for a in (comp, root, np.searchsorted(off[1:], root, side="right"),
                                                             group.numpy()[root], box[root], count[root])))
        got += PP.region_tuples(reg, len(ids), min_words)
    want = regions_ref.regions_list(*all_ref, all_off, all_group, min_words=min_words)
    assert got == want and len(got) == 6 and sum(len(p) for p in want) > 6
