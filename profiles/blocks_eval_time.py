"""The two launches of the block route's evaluation on ONE cfg2-sized synthetic batch (100 pages), by the method of
profiles/boxeval_time.py -- per case 20 warm-up launches, then 200 launches between one event pair:
  gte_box_match_f64 at 10 thresholds on the cells of boxeval_time.py (the scored regions of the predictions against the label
      regions, the same boxes as doubles), with and without the IoU output, beside gte_box_match on the integers;
  gte_block_scores on the pages' FINAL blocks (layout blocks from tests/blocks_ref.py's synthetic_blocks through extract_blocks)
      with the logits of boxeval_time.py, beside gte_block_vote on the input blocks of the same pages.
Both are off the step path: information, not a criterion.
usage: python profiles/blocks_eval_time.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib                               # noqa: E402
from gnn_tableextraction_amd.components.graphs import postprocessing as PP      # noqa: E402
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages      # noqa: E402
from gnn_tableextraction_amd.data import synthetic as S                # noqa: E402
from gnn_tableextraction_amd.utils import metrics                      # noqa: E402
from tests import blocks_ref                                           # noqa: E402

WARMUP, LAUNCHES, SF = 20, 200, 0.36
dev = torch.device("cuda", 0)
lib, P = _lib.load(), _lib.ptr
data = PrebuiltPages.synthetic(100, in_feats=13)
pages = data.page_arrays
_, _, _, _, label, off = S.concat_pages(pages)
n = int(off[-1])
rng = np.random.default_rng(7)                                         # boxeval_time.py's logits: the label three times out of four
logits_h = rng.standard_normal((n, 9)).astype(np.float32)
logits_h[np.arange(n), np.where(rng.random(n) < 0.75, label, rng.integers(0, 9, n))] += 3.0
logits = torch.from_numpy(logits_h).to(dev)
pred_h = logits_h.argmax(axis=1)
off_l = off.tolist()
all_pred = [pred_h[off_l[i]:off_l[i + 1]] for i in range(len(pages))]


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1000.0 * e0.elapsed_time(e1) / LAUNCHES, 2)


# ---- the matching: boxeval_time.py's cells ------------------------------------------------------------------------------------
regions = PP.extract_regions(data, all_pred, batch_pages=100, logits=logits)
pred_doc = PP.regions_json(data, regions)
gt_doc = PP.regions_gt_json(data, PP.extract_regions(data, [p.label for p in pages], batch_pages=100))
cells = metrics.region_cells(pred_doc, gt_doc)
n_cells = len(cells.kind)
po, go = np.asarray(cells.pred_off, dtype=np.int64), np.asarray(cells.gt_off, dtype=np.int64)
io = np.concatenate([[0], np.cumsum(np.diff(po) * np.diff(go))]).astype(np.int64)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_pb, d_gb, d_pf, d_gf = t(cells.pred_box), t(cells.gt_box), t(cells.pred_box.astype(np.float64)), t(cells.gt_box.astype(np.float64))
d_po, d_go, d_io = t(po.astype(np.int32)), t(go.astype(np.int32)), t(io)
thr = np.linspace(0.5, 0.95, 10)
tp_i = torch.empty((10, int(po[-1])), dtype=torch.int32, device=dev)
tp_f = torch.empty_like(tp_i)
status = torch.empty(n_cells, dtype=torch.int32, device=dev)
iou = torch.empty(int(io[-1]), dtype=torch.float64, device=dev)
max_r, max_g = int(np.diff(po).max()), int(np.diff(go).max())


def match_int():
    _lib.check(lib.gte_box_match(P(d_pb), P(d_po), P(d_gb), P(d_go), n_cells, max_r, max_g, thr.ctypes.data, 10, P(tp_i), P(status),
                                 _lib.current_stream()), "gte_box_match")


def match_f64(with_iou):
    _lib.check(lib.gte_box_match_f64(P(d_pf), P(d_po), P(d_gf), P(d_go), n_cells, max_r, max_g, thr.ctypes.data, 10, P(tp_f), P(status),
                                     P(iou) if with_iou else None, P(d_io) if with_iou else None, _lib.current_stream()),
               "gte_box_match_f64")


out = {"pages": len(pages), "nodes": n, "launches": LAUNCHES, "cells": n_cells, "predicted_boxes": int(po[-1]),
       "ground_truth_boxes": int(go[-1]), "largest_cell": [max_r, max_g], "pairs": int(io[-1]),
       "box_match_10_thresholds_us": timed(match_int), "box_match_f64_10_thresholds_us": timed(lambda: match_f64(False)),
       "box_match_f64_with_iou_us": timed(lambda: match_f64(True))}
torch.cuda.synchronize()
out["f64_equal_to_int_on_integer_boxes"] = bool(torch.equal(tp_i, tp_f))

# ---- the block confidences: the final blocks of the same pages ---------------------------------------------------------------------
rng = np.random.default_rng(7)
for page in data.pages:
    page["blocks"] = blocks_ref.synthetic_blocks(page["bboxs"], rng)
batch = PP.pack_blocks(data, all_pred, batch_pages=100)[0]
d_bbox, d_no = t(batch.bbox), t(batch.node_off.astype(np.int32))
d_cat, d_in, d_bo_in = t(batch.word_cat), t(batch.block_box), t(batch.block_off.astype(np.int32))
nb_in = int(batch.block_off[-1])
word_block = torch.empty(n, dtype=torch.int32, device=dev)
votes = torch.empty((nb_in, batch.n_cat), dtype=torch.int32, device=dev)
voted = torch.empty(nb_in, dtype=torch.int32, device=dev)
largest_in = int(np.diff(batch.block_off).max())


def vote():
    _lib.check(lib.gte_block_vote(P(d_bbox), P(d_no), P(d_cat), P(d_in), P(d_bo_in), len(pages), n, nb_in, largest_in, batch.n_cat, 2,
                                  P(word_block), P(votes), P(voted), _lib.current_stream()), "gte_block_vote")


vote()
torch.cuda.synchronize()
final = PP.pack_final_blocks(PP.blocks_to_pages(data, batch, word_block.cpu().numpy(), votes.cpu().numpy(), voted.cpu().numpy()), SF)
nb = int(final.block_off[-1])
d_fb, d_fo, d_fc = t(final.block_box), t(final.block_off.astype(np.int32)), t(final.block_cat)
d_masks = t(PP.category_class_masks(None, batch.n_cat).view(np.int32))
score = torch.empty(nb, dtype=torch.float32, device=dev)
n_words = torch.empty(nb, dtype=torch.int32, device=dev)
largest_words, largest_blocks = int(np.diff(batch.node_off).max()), int(np.diff(final.block_off).max())


def scores():
    _lib.check(lib.gte_block_scores(P(d_bbox), P(d_no), P(logits), 9, 9, P(d_fb), P(d_fo), P(d_fc), P(d_masks), batch.n_cat, len(pages), n,
                                    nb, largest_words, largest_blocks, P(score), P(n_words), _lib.current_stream()), "gte_block_scores")


out.update({"input_blocks": nb_in, "final_blocks": nb, "largest_page_words": largest_words, "largest_page_final_blocks": largest_blocks,
            "block_vote_us": timed(vote), "block_scores_us": timed(scores)})
torch.cuda.synchronize()
out["mean_words_per_final_block"] = round(float(n_words.float().mean()), 1)
out["mean_score"] = round(float(score.mean()), 4)
print(json.dumps(out), flush=True)
