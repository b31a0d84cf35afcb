"""The block vote on ONE cfg2-sized synthetic batch (100 pages, their word boxes, layout blocks from tests/blocks_ref.py's
synthetic_blocks, categories from random predictions): microseconds per launch of gte_block_vote -- 20 warm-up launches, then the
MEDIAN of 200 launches each between its own event pair -- beside a plain torch formulation of the same vote on the same tensors
(pages padded to [pages, words, blocks], the closed test as one boolean tensor, first hit by argmax, counters by scatter_add:
what one would write without the kernel), timed the same way.  Host wall time of postprocessing.extract_blocks on these pages
against the same pages through the pure-Python loop of tests/blocks_ref.py (+ the same assemble_tables) beside it.
usage: python profiles/block_vote_time.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib                               # noqa: E402
from gnn_tableextraction_amd.components.graphs import postprocessing as PP      # noqa: E402
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages      # noqa: E402
from tests import blocks_ref                                           # noqa: E402

WARMUP, LAUNCHES, SF, N_CAT = 20, 200, 0.36, 13
dev = torch.device("cuda", 0)
rng = np.random.default_rng(7)
data = PrebuiltPages.synthetic(100, in_feats=13)
pred = []
for page in data.pages:
    page["blocks"] = blocks_ref.synthetic_blocks(page["bboxs"], rng)
    pred.append(rng.integers(0, 9, len(page["bboxs"])))
sizes = [len(p["bboxs"]) for p in data.pages]
n_blocks = [len(p["blocks"]) for p in data.pages]
node_off_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
block_off_h = np.concatenate([[0], np.cumsum(n_blocks)]).astype(np.int32)
n, nb = int(node_off_h[-1]), int(block_off_h[-1])
bbox_h = np.concatenate([np.asarray(p["bboxs"], dtype=np.int32).reshape(-1, 4) for p in data.pages])
cat_h = np.asarray(PP.DEFAULT_CLASS_CATEGORY, dtype=np.int32)[np.concatenate(pred)]
blocks_h = np.concatenate([np.asarray(p["blocks"], dtype=np.float64).reshape(-1, 4) for p in data.pages]) / SF
t = lambda a: torch.from_numpy(a).to(dev)
bbox, cat, blocks, node_off, block_off = t(bbox_h), t(cat_h), t(blocks_h), t(node_off_h), t(block_off_h)
word_block = torch.empty(n, dtype=torch.int32, device=dev)
votes = torch.empty((nb, N_CAT), dtype=torch.int32, device=dev)
label = torch.empty(nb, dtype=torch.int32, device=dev)
lib, P = _lib.load(), _lib.ptr
largest = max(n_blocks)


def kernel():
    _lib.check(lib.gte_block_vote(P(bbox), P(node_off), P(cat), P(blocks), P(block_off), len(sizes), n, nb, largest, N_CAT, 2,
                                  P(word_block), P(votes), P(label), _lib.current_stream()), "gte_block_vote")


# ---- the plain torch formulation: padded pages (built once, outside the timing) ------------------------------------------------
W, B = max(sizes), largest
page_of_word = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev))
slot_of_word = torch.arange(n, device=dev) - node_off.long()[page_of_word]
page_of_block = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(n_blocks, device=dev))
slot_of_block = torch.arange(nb, device=dev) - block_off.long()[page_of_block]
wpad = torch.zeros((len(sizes), W, 4), dtype=torch.float64, device=dev)
wpad[page_of_word, slot_of_word] = bbox.double()
cpad = torch.full((len(sizes), W), -1, dtype=torch.int64, device=dev)
cpad[page_of_word, slot_of_word] = cat.long()
bpad = torch.full((len(sizes), B, 4), float("nan"), dtype=torch.float64, device=dev)
bpad[page_of_block, slot_of_block] = blocks


def plain_torch():
    wlo, whi = torch.minimum(wpad[..., :2], wpad[..., 2:]), torch.maximum(wpad[..., :2], wpad[..., 2:])
    blo, bhi = torch.minimum(bpad[..., :2], bpad[..., 2:]), torch.maximum(bpad[..., :2], bpad[..., 2:])
    meet = ((blo[:, None, :, :] <= whi[:, :, None, :]) & (wlo[:, :, None, :] <= bhi[:, None, :, :])).all(dim=-1)      # [P, W, B]
    first = meet.to(torch.int8).argmax(dim=-1)
    hit = meet.any(dim=-1) & (cpad >= 0)
    counters = torch.zeros((len(sizes), B, N_CAT), dtype=torch.int32, device=dev)
    flat = (torch.arange(len(sizes), device=dev)[:, None] * B + first) * N_CAT + cpad.clamp(min=0)
    weight = torch.where(cpad == 2, 2, 1).to(torch.int32) * hit
    counters.view(-1).scatter_add_(0, flat.view(-1), weight.view(-1))
    return first, counters, counters.argmax(dim=-1)


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


out = {"nodes": n, "pages": len(sizes), "blocks": nb, "largest_page_blocks": largest, "launches": LAUNCHES,
       "block_vote_us_median": timed(kernel), "plain_torch_us_median": timed(plain_torch)}
first, counters, _ = plain_torch()
torch.cuda.synchronize()
out["plain_torch_equal_counters"] = bool((counters[page_of_block, slot_of_block] == votes).all())

PP.extract_blocks(data, pred, batch_pages=100)
t0 = time.perf_counter()
for _ in range(5):
    got = PP.extract_blocks(data, pred, batch_pages=100)
out["extract_blocks_ms_host"] = round(1e3 * (time.perf_counter() - t0) / 5, 2)
t0 = time.perf_counter()
want = []
for page, p in zip(data.pages, pred):
    cats = [PP.DEFAULT_CLASS_CATEGORY[int(c)] for c in p]
    wb, v, voted = blocks_ref.vote_page(page["bboxs"], cats, np.asarray(page["blocks"], dtype=np.float64).reshape(-1, 4) / SF)
    new_blocks, new_labels, _ = PP.assemble_tables([[float(x) for x in b] for b in page["blocks"]], voted)
    want.append(([[x / SF for x in b] for b in new_blocks], new_labels, wb))
out["python_loop_ms_host"] = round(1e3 * (time.perf_counter() - t0), 1)
t0 = time.perf_counter()
for page, r in zip(data.pages, got):
    PP.assemble_tables([[float(x) for x in b] for b in page["blocks"]], r["voted_labels"])
out["assemble_tables_ms_host"] = round(1e3 * (time.perf_counter() - t0), 2)
out["equal_to_ref"] = all(r["blocks"] == w[0] and r["labels"] == w[1] and r["word_block"] == w[2] for r, w in zip(got, want))
print(json.dumps(out), flush=True)
