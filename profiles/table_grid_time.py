"""The table grids of ONE batch of 64 synthetic pages (tests/table_grid_ref.synthetic_page: one R x C table per page, R in 1 .. 7,
C in 1 .. 6, under a line of text words; the 'auto' column gap): microseconds per launch of gte_table_grid -- 20 warm-up launches,
then the MEDIAN of 200 launches each between its own event pair -- beside the host wall time of tests/table_grid_ref.py (numpy
occupancy arrays) on the same arguments, and of postprocessing.tables_from_grids on the launch's outputs.
usage: python profiles/table_grid_time.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib                               # noqa: E402
from gnn_tableextraction_amd.components.graphs import postprocessing as PP      # noqa: E402
from tests import table_grid_ref as ref                                # noqa: E402

WARMUP, LAUNCHES, PAGES = 20, 200, 64
dev = torch.device("cuda", 0)
rng = np.random.default_rng(64)
pages = [ref.synthetic_page(rng, int(rng.integers(1, 8)), int(rng.integers(1, 7))) for _ in range(PAGES)]
off_h = np.concatenate([[0], np.cumsum([len(p["text"]) for p in pages])]).astype(np.int32)
root_h = np.asarray([off_h[k] + np.nonzero(p["member"])[0][0] for k, p in enumerate(pages)], dtype=np.int32)
table_h = np.concatenate([np.where(p["member"], root_h[k], -1) for k, p in enumerate(pages)]).astype(np.int32)
bbox_h = np.concatenate([p["bbox"] for p in pages]).astype(np.int32)
role_h = np.concatenate([p["role"] for p in pages]).astype(np.int32)
page_h = np.arange(PAGES, dtype=np.int32)
gap_h = np.asarray([[ref.auto_gap(p["bbox"][p["member"]]), 0] for p in pages], dtype=np.int32)
n = int(off_h[-1])
t = lambda a: torch.from_numpy(a).to(dev)
bbox, off, table, role, root, page, gap = t(bbox_h), t(off_h), t(table_h), t(role_h), t(root_h), t(page_h), t(gap_h)
cols, rows = PP.role_mask(PP.DEFAULT_COL_ROLES), PP.role_mask(PP.DEFAULT_ROW_ROLES)
cell = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
cell_box = torch.zeros((n, 4), dtype=torch.int32, device=dev)
shape = torch.empty((PAGES, 2), dtype=torch.int32, device=dev)
box = torch.empty((PAGES, 4), dtype=torch.int32, device=dev)
words = torch.empty(PAGES, dtype=torch.int32, device=dev)
status = torch.empty(PAGES, dtype=torch.int32, device=dev)
lib, P = _lib.load(), _lib.ptr


def kernel():
    _lib.check(lib.gte_table_grid(P(bbox), P(off), PAGES, n, P(table), P(role), P(root), P(page), P(gap), PAGES, cols, rows, P(cell),
                                  P(cell_box), P(shape), P(box), P(words), P(status), _lib.current_stream()), "gte_table_grid")


for _ in range(WARMUP):
    kernel()
torch.cuda.synchronize()
pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(LAUNCHES)]
for e0, e1 in pairs:
    e0.record()
    kernel()
    e1.record()
torch.cuda.synchronize()
times = np.asarray([e0.elapsed_time(e1) for e0, e1 in pairs]) * 1000.0
got = [a.cpu().numpy() for a in (cell, cell_box, shape, box, words, status)]

t0 = time.perf_counter()
want = ref.table_grid_ref(bbox_h, off_h, table_h, role_h, root_h, page_h, gap_h, cols, rows)
ref_ms = 1e3 * (time.perf_counter() - t0)
t0 = time.perf_counter()
tables = PP.tables_from_grids(table_h, bbox_h, role_h, off_h, root_h, page_h, got, [p["text"] for p in pages])
host_ms = 1e3 * (time.perf_counter() - t0)
print(json.dumps({"pages": PAGES, "tables": PAGES, "nodes": n, "table_words": int(got[4].sum()), "launches": LAUNCHES,
                  "table_grid_us_median": round(float(np.median(times)), 2), "table_grid_us_min": round(float(times.min()), 2),
                  "table_grid_us_p90": round(float(np.percentile(times, 90)), 2), "numpy_ref_ms_host": round(ref_ms, 1),
                  "tables_from_grids_ms_host": round(host_ms, 2),
                  "equal_to_ref": all(np.array_equal(g, w) for g, w in zip(got, want)),
                  "grids_exact": all(tab[0]["grid"] == p["cell_text"] for tab, p in zip(tables, pages))}), flush=True)
