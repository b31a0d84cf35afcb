"""gte_page_regions on ONE cfg2-sized synthetic batch (100 pages, their k-NN edges and boxes): microseconds per launch, kinds from
DEFAULT_CLASS_GROUP over predictions equal to the labels / uniform over the 9 classes / all one kind (every page ONE region: the
most rounds and the most contended accumulators) -- per case 20 warm-up launches, then 200 launches between one event pair.
The torch compaction behind postprocessing.page_regions (nonzero + gathers, one synchronisation) is timed beside it from the host.
usage: python profiles/regions_time.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib, graph as G                   # noqa: E402
from gnn_tableextraction_amd.components.graphs import postprocessing as PP      # noqa: E402
from gnn_tableextraction_amd.data import synthetic as S                # noqa: E402

WARMUP, LAUNCHES = 20, 200
dev = torch.device("cuda", 0)
pages = S.make_pages(100, in_feats=13)
src, dst, _, _, label, off = S.concat_pages(pages)
n = int(off[-1])
g = G.PageGraph(src, dst, n, device=dev)
g.batch_num_nodes_ = [p.num_nodes for p in pages]
csr = g.in_csr()
bbox = torch.from_numpy(np.concatenate([p.bbox for p in pages]).astype(np.int32)).to(dev)
node_off = torch.from_numpy(off.astype(np.int32)).to(dev)
table = torch.tensor(PP.DEFAULT_CLASS_GROUP, dtype=torch.int32, device=dev)
groups = {"labels": table[torch.from_numpy(label).to(dev)],
          "uniform": table[torch.from_numpy(np.random.default_rng(7).integers(0, 9, n)).to(dev)],
          "one_kind": torch.ones(n, dtype=torch.int32, device=dev)}
comp = torch.empty(n, dtype=torch.int32, device=dev)
rbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
count = torch.empty(n, dtype=torch.int32, device=dev)
lib, P = _lib.load(), _lib.ptr
max_page = max(p.num_nodes for p in pages)


def launch(group):
    _lib.check(lib.gte_page_regions(P(csr.indptr), P(csr.indices), P(node_off), len(pages), n, max_page, P(group), P(bbox), P(comp),
                                    P(rbox), P(count), _lib.current_stream()), "gte_page_regions")


out = {"nodes": n, "pages": len(pages), "entries": int(csr.indices.numel()), "largest_page": max_page, "launches": LAUNCHES}
for name, group in groups.items():
    for _ in range(WARMUP):
        launch(group)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        launch(group)
    e1.record()
    torch.cuda.synchronize()
    for _ in range(3):
        PP.page_regions(g, group, bbox)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        reg = PP.page_regions(g, group, bbox)
    torch.cuda.synchronize()
    out[name] = {"kernel_us": round(1000.0 * e0.elapsed_time(e1) / LAUNCHES, 2), "regions": int(reg.root.numel()),
                 "largest_region_words": int(reg.n_words.max()) if reg.root.numel() else 0,
                 "page_regions_call_us_host": round(1e6 * (time.perf_counter() - t0) / 20, 1)}
print(json.dumps(out), flush=True)
