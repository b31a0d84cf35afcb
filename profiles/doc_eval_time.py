"""The area-weighted confusion at the validation set's size (478 000 nodes, C = 9, labels 85 % right, a few outside the classes):
microseconds per gte_doc_eval call (one memset + three launches) -- 20 warm-up calls, then the MEDIAN of 200 calls each between
its own event pair, inputs resident on the device -- beside the same quantities (area, count, lead) computed by numpy on this
machine's host (tests/doceval_ref.py: area_confusion; the median of 5 runs, wall clock), which is the baseline, and beside the
wall time of metrics.area_confusion from host arrays (copies in, the call, copies out).  The results are compared entry by entry.
usage: python profiles/doc_eval_time.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib                               # noqa: E402
from gnn_tableextraction_amd.utils import metrics                      # noqa: E402
from tests import doceval_ref as ref                                   # noqa: E402

WARMUP, CALLS, N, C = 20, 200, 478_000, 9
dev = torch.device("cuda", 0)
gt_h, pred_h, bbox_h = ref.random_case(np.random.default_rng(12), N, C, accuracy=0.85, outside=0.02, odd_boxes=0.02)
gt, pred, bbox = (torch.from_numpy(a).to(dev) for a in (gt_h, pred_h, bbox_h))
area = torch.empty((C + 1) * (C + 1), dtype=torch.int64, device=dev)
count = torch.empty_like(area)
lead = torch.empty(2 * C, dtype=torch.int64, device=dev)
lib, P = _lib.load(), _lib.ptr
ws = torch.empty(lib.gte_doc_eval_workspace_bytes(N, C), dtype=torch.uint8, device=dev)


def call():
    _lib.check(lib.gte_doc_eval(P(gt), P(pred), P(bbox), N, C, P(area), P(count), P(lead), P(ws), ws.numel(), _lib.current_stream()),
               "gte_doc_eval")


for _ in range(WARMUP):
    call()
torch.cuda.synchronize()
pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
for e0, e1 in pairs:
    e0.record()
    call()
    e1.record()
torch.cuda.synchronize()
us = [1000.0 * e0.elapsed_time(e1) for e0, e1 in pairs]


def wall_ms(fn, runs=5):
    fn()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        result = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(times)), 3), result


numpy_ms, want = wall_ms(lambda: ref.area_confusion(gt_h, pred_h, bbox_h, C))
wrapper_ms, got = wall_ms(lambda: metrics.area_confusion(gt_h, pred_h, bbox_h, C, device=dev))
out = {"nodes": N, "classes": C, "chunks": -(-N // lib.gte_doc_eval_chunk_nodes()), "calls": CALLS,
       "doc_eval_us_median": round(float(np.median(us)), 2), "doc_eval_us_min": round(float(np.min(us)), 2),
       "numpy_host_ms_median": numpy_ms, "area_confusion_from_host_ms_median": wrapper_ms,
       "equal_to_numpy": bool(all(np.array_equal(a, b) for a, b in zip(got, want))
                              and np.array_equal(area.cpu().numpy().reshape(C + 1, C + 1), want[0])
                              and np.array_equal(lead.cpu().numpy().reshape(2, C), want[2])),
       "lead_nonzero": bool(want[2].all())}
print(json.dumps(out), flush=True)
