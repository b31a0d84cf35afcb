"""Region confidences and box matching on ONE cfg2-sized synthetic batch (100 pages, their k-NN edges and boxes): microseconds per
launch of gte_page_regions against gte_page_regions_scored (kinds from DEFAULT_CLASS_GROUP over the arg-max of random logits; a
torch softmax over the same logits timed beside them: what a separate pass would cost), and of gte_box_match at 10 thresholds on
the cells of those regions against the label regions -- per case 20 warm-up launches, then 200 launches between one event pair.
Host wall time of metrics.evaluate_regions against tests/boxeval_ref.py on the same documents beside it.
usage: python profiles/boxeval_time.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib, graph as G                   # noqa: E402
from gnn_tableextraction_amd.components.graphs import postprocessing as PP      # noqa: E402
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages      # noqa: E402
from gnn_tableextraction_amd.data import synthetic as S                # noqa: E402
from gnn_tableextraction_amd.utils import metrics                      # noqa: E402
from tests import boxeval_ref                                          # noqa: E402

WARMUP, LAUNCHES = 20, 200
dev = torch.device("cuda", 0)
data = PrebuiltPages.synthetic(100, in_feats=13)
pages = data.page_arrays
src, dst, _, _, label, off = S.concat_pages(pages)
n = int(off[-1])
g = G.PageGraph(src, dst, n, device=dev)
g.batch_num_nodes_ = [p.num_nodes for p in pages]
csr = g.in_csr()
bbox = torch.from_numpy(np.concatenate([p.bbox for p in pages]).astype(np.int32)).to(dev)
node_off = torch.from_numpy(off.astype(np.int32)).to(dev)
table = torch.tensor(PP.DEFAULT_CLASS_GROUP, dtype=torch.int32, device=dev)
# logits that agree with the label three times out of four: regions of realistic sizes with scores below 1
rng = np.random.default_rng(7)
logits_h = rng.standard_normal((n, 9)).astype(np.float32)
logits_h[np.arange(n), np.where(rng.random(n) < 0.75, label, rng.integers(0, 9, n))] += 3.0
logits = torch.from_numpy(logits_h).to(dev)
pred = logits.argmax(dim=1)
group = table[pred]
comp = torch.empty(n, dtype=torch.int32, device=dev)
rbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
count = torch.empty(n, dtype=torch.int32, device=dev)
score = torch.empty(n, dtype=torch.float32, device=dev)
lib, P = _lib.load(), _lib.ptr
max_page = max(p.num_nodes for p in pages)


def plain():
    _lib.check(lib.gte_page_regions(P(csr.indptr), P(csr.indices), P(node_off), len(pages), n, max_page, P(group), P(bbox), P(comp),
                                    P(rbox), P(count), _lib.current_stream()), "gte_page_regions")


def scored():
    _lib.check(lib.gte_page_regions_scored(P(csr.indptr), P(csr.indices), P(node_off), len(pages), n, max_page, P(group), P(bbox),
                                           P(logits), 9, P(table), P(comp), P(rbox), P(count), P(score), _lib.current_stream()),
               "gte_page_regions_scored")


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


out = {"nodes": n, "pages": len(pages), "largest_page": max_page, "launches": LAUNCHES,
       "page_regions_us": timed(plain), "page_regions_scored_us": timed(scored),
       "torch_softmax_us": timed(lambda: torch.softmax(logits, dim=1))}

# ---- the documents: scored regions of the predictions against the regions of the labels ----------------------------------
off_l = off.tolist()
pred_h = pred.cpu().numpy()
regions = PP.extract_regions(data, [pred_h[off_l[i]:off_l[i + 1]] for i in range(len(pages))], batch_pages=100, logits=logits)
pred_doc = PP.regions_json(data, regions)
gt_doc = PP.regions_gt_json(data, PP.extract_regions(data, [p.label for p in pages], batch_pages=100))
cells, pb, gb, po, go = 0, [], [], [0], [0]
for kind, gts in gt_doc.items():
    for page, boxes in gts.items():
        if page in pred_doc[kind]:
            e = pred_doc[kind][page]
            order = np.argsort(np.asarray(e["scores"]), kind="stable")
            pb.append(np.asarray(e["bboxes"], dtype=np.int32)[order])
            gb.append(np.asarray(boxes, dtype=np.int32))
            po.append(po[-1] + len(order))
            go.append(go[-1] + len(boxes))
            cells += 1
d_pb, d_gb = torch.from_numpy(np.concatenate(pb)).to(dev), torch.from_numpy(np.concatenate(gb)).to(dev)
d_po, d_go = torch.tensor(po, dtype=torch.int32, device=dev), torch.tensor(go, dtype=torch.int32, device=dev)
thr = np.linspace(0.5, 0.95, 10)
tp = torch.empty((10, po[-1]), dtype=torch.int32, device=dev)
status = torch.empty(cells, dtype=torch.int32, device=dev)
max_r, max_g = int(np.diff(po).max()), int(np.diff(go).max())


def match():
    _lib.check(lib.gte_box_match(P(d_pb), P(d_po), P(d_gb), P(d_go), cells, max_r, max_g, thr.ctypes.data, 10, P(tp), P(status),
                                 _lib.current_stream()), "gte_box_match")


out.update({"cells": cells, "predicted_boxes": po[-1], "ground_truth_boxes": go[-1], "largest_cell": [max_r, max_g],
            "box_match_10_thresholds_us": timed(match)})
metrics.evaluate_regions(pred_doc, gt_doc)
t0 = time.perf_counter()
for _ in range(5):
    got = metrics.evaluate_regions(pred_doc, gt_doc)
torch.cuda.synchronize()
out["evaluate_regions_ms_host"] = round(1e3 * (time.perf_counter() - t0) / 5, 2)
t0 = time.perf_counter()
want = boxeval_ref.evaluate_doc_ref(pred_doc, gt_doc)
out["boxeval_ref_ms_host"] = round(1e3 * (time.perf_counter() - t0), 1)
out["map"] = round(got["map"], 6)
out["equal_to_ref"] = all(got[k]["precisions"] == want[k]["precisions"] and got[k]["recalls"] == want[k]["recalls"] for k in gt_doc)
print(json.dumps(out), flush=True)
