"""The two launches of the word labels on ONE cfg2-sized synthetic batch (100 pages, their word boxes; the annotations are the
pages' layout blocks from tests/blocks_ref.py's synthetic_blocks in word coordinates, with seeded random categories -- the batch of
profiles/block_vote_time.py): microseconds per launch of gte_word_labels and of gte_word_labels_compact -- 20 warm-up launches,
then the MEDIAN of 200 launches each between its own event pair -- and that the answers equal tests/wordlabels_ref.py.
Both are off the step path: information, not a criterion.
usage: python profiles/word_labels_time.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib                               # noqa: E402
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages      # noqa: E402
from tests import blocks_ref, wordlabels_ref                           # noqa: E402

WARMUP, LAUNCHES, SF, N_CAT = 20, 200, 0.36, 13
SKIP_MASK = sum(1 << c for c in wordlabels_ref.SKIP)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(7)
data = PrebuiltPages.synthetic(100, in_feats=13)
anns = [np.asarray(blocks_ref.synthetic_blocks(page["bboxs"], rng), dtype=np.float64).reshape(-1, 4) / SF for page in data.pages]
sizes, n_anns = [len(p["bboxs"]) for p in data.pages], [len(a) for a in anns]
node_off_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
ann_off_h = np.concatenate([[0], np.cumsum(n_anns)]).astype(np.int32)
n, na, pages = int(node_off_h[-1]), int(ann_off_h[-1]), len(sizes)
bbox_h = np.concatenate([np.asarray(p["bboxs"], dtype=np.int32).reshape(-1, 4) for p in data.pages])
ann_box_h = np.ascontiguousarray(np.concatenate(anns))
ann_cat_h = rng.integers(0, N_CAT, na).astype(np.int32)
t = lambda a: torch.from_numpy(a).to(dev)
bbox, node_off, ann_box, ann_cat, ann_off = t(bbox_h), t(node_off_h), t(ann_box_h), t(ann_cat_h), t(ann_off_h)
word_label = torch.empty(n, dtype=torch.int32, device=dev)
word_ann = torch.empty(n, dtype=torch.int32, device=dev)
counts = torch.empty((pages, 2), dtype=torch.int32, device=dev)
lib, P = _lib.load(), _lib.ptr


def labels():
    _lib.check(lib.gte_word_labels(P(bbox), P(node_off), P(ann_box), P(ann_cat), P(ann_off), pages, n, na, N_CAT, SKIP_MASK,
                                   wordlabels_ref.FIGURE, P(word_label), P(word_ann), P(counts), _lib.current_stream()), "gte_word_labels")


labels()
torch.cuda.synchronize()
out_off_h = np.concatenate([[0], np.cumsum(counts.cpu().numpy().sum(1))]).astype(np.int32)
n_out = int(out_off_h[-1])
out_off = t(out_off_h)
out_bbox = torch.empty((n_out, 4), dtype=torch.int32, device=dev)
out_label = torch.empty(n_out, dtype=torch.int32, device=dev)
out_src = torch.empty(n_out, dtype=torch.int32, device=dev)
status = torch.empty(pages, dtype=torch.int32, device=dev)


def compact():
    _lib.check(lib.gte_word_labels_compact(P(bbox), P(node_off), P(word_label), P(ann_box), P(ann_cat), P(ann_off), P(out_off), None,
                                           pages, n, na, N_CAT, wordlabels_ref.FIGURE, n_out, P(out_bbox), P(out_label), P(out_src),
                                           P(status), _lib.current_stream()), "gte_word_labels_compact")


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(LAUNCHES)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return round(1000.0 * float(np.median([e0.elapsed_time(e1) for e0, e1 in pairs])), 2)


out = {"nodes": n, "pages": pages, "annotations": na, "largest_page_annotations": max(n_anns), "out_rows": n_out, "launches": LAUNCHES,
       "word_labels_us_median": timed(labels), "word_labels_compact_us_median": timed(compact)}
torch.cuda.synchronize()
want = wordlabels_ref.label_batch(bbox_h, node_off_h, ann_box_h, ann_cat_h, ann_off_h)
boxes, want_label, want_src, want_off = wordlabels_ref.compact_batch(bbox_h, node_off_h, ann_box_h, ann_cat_h, ann_off_h, want[0])
out["labelled_words"] = int((want[0] > 0).sum())
out["equal_to_ref"] = bool(np.array_equal(word_label.cpu().numpy(), want[0]) and np.array_equal(word_ann.cpu().numpy(), want[1])
                           and np.array_equal(counts.cpu().numpy(), want[2]) and not status.cpu().numpy().any()
                           and np.array_equal(out_off_h, want_off) and np.array_equal(out_bbox.cpu().numpy(), boxes)
                           and np.array_equal(out_label.cpu().numpy(), want_label) and np.array_equal(out_src.cpu().numpy(), want_src))
print(json.dumps(out), flush=True)
