"""Token pooling at the headline size (24.3 k words, D = 768, V = 31 090, width 15; a seeded table and seeded ids, one to six
pieces per word and [SEP] behind all but the longest words): microseconds per launch of gte_token_pool_f32 beside the reference's
own formulation in torch on the same device -- the embedding lookup to [N, 16, 768], the product with the expanded mask, the sum
over the positions and the division by the clamped mask sum (src/components/nlp/scibert.py:53-58, 156-157), for all pages at once.
The two ALTERNATE: 20 warm-up rounds, then 100 rounds of one call each, every call between its own event pair; the medians, and
the 10th / 90th percentiles, are reported.  The kernel is timed in three layouts: a packed [N, 768] result (16-byte accesses),
columns 64 .. 832 of an 832-float row (16-byte) and columns 63 .. 831 of an 831-float row (dword accesses: the real feature matrix).
usage: python profiles/token_pool_time.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import _lib, graph as G                   # noqa: E402

WARMUP, ROUNDS = 20, 100
N, D, V, W = 24300, 768, 31090, 15
CLS, SEP, PAD = 102, 103, 0
dev = torch.device("cuda", 0)
rng = np.random.default_rng(11)
table = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(V, D)).astype(np.float32)).to(dev))
pieces = rng.integers(1, 7, size=N)
pieces[rng.random(N) < 0.02] = 14
page = np.repeat(np.arange(N // 243), 243)                              # 100 pages of 243 words
longest = np.zeros(N // 243, dtype=np.int64)
np.maximum.at(longest, page, pieces)
ids_h = np.full((N, W + 1), PAD, dtype=np.int64)                        # the reference's rows ...
mask_h = np.zeros((N, W + 1), dtype=np.int64)                           # ... and its modified mask
tok_h = np.full((N, W), -1, dtype=np.int32)
for i in range(N):
    m = int(pieces[i])
    row = [CLS] + rng.integers(1000, V, size=m).tolist() + [SEP]
    ids_h[i, :m + 2] = row
    mask_h[i, 1:min(m + 2, int(longest[page[i]]) + 1)] = 1              # column 0 and the page's last column cleared
    tok_h[i] = np.where(mask_h[i, 1:] == 1, ids_h[i, 1:], -1)
ids, mask, tok = (torch.from_numpy(a).to(dev) for a in (ids_h, mask_h, tok_h))
packed = torch.empty((N, D), dtype=torch.float32, device=dev)
wide832 = torch.zeros((N, 832), dtype=torch.float32, device=dev)
wide831 = torch.zeros((N, 831), dtype=torch.float32, device=dev)
lib = _lib.load()


def kernel(out):
    return lambda: G.token_pool(tok, table, mode="mean", out=out)


def plain_torch():
    emb = torch.nn.functional.embedding(ids, table)                     # [N, 16, 768]
    expanded = mask.unsqueeze(-1).expand(emb.size()).float()
    return torch.sum(emb * expanded, 1) / torch.clamp(expanded.sum(1), min=1e-9)


variants = {"token_pool_packed": kernel(packed), "token_pool_ldo832_col64": kernel(wide832[:, 64:]),
            "token_pool_ldo831_col63": kernel(wide831[:, 63:]), "plain_torch": plain_torch}
for _ in range(WARMUP):
    for fn in variants.values():
        fn()
torch.cuda.synchronize()
times = {k: [] for k in variants}
events = []
for _ in range(ROUNDS):
    for name, fn in variants.items():                                   # alternating: one call of each per round
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        events.append((name, e0, e1))
torch.cuda.synchronize()
for name, e0, e1 in events:
    times[name].append(1000.0 * e0.elapsed_time(e1))
rows_read = int((tok_h >= 0).sum())
out = {"words": N, "dim": D, "vocab": V, "width": W, "rows_read": rows_read, "rounds": ROUNDS,
       "bytes_needed_MB": round((rows_read * D * 4 + N * D * 4 + tok_h.nbytes) / 1e6, 1)}
for name, t in times.items():
    out[name + "_us"] = {"median": round(float(np.median(t)), 1), "p10": round(float(np.percentile(t, 10)), 1),
                         "p90": round(float(np.percentile(t, 90)), 1)}
want = plain_torch()
torch.cuda.synchronize()
out["access_bytes"] = {"packed": lib.gte_token_pool_access_bytes(_lib.ptr(table), D, _lib.ptr(packed), D),
                       "ldo832_col64": lib.gte_token_pool_access_bytes(_lib.ptr(table), D, _lib.ptr(wide832[:, 64:]), 832),
                       "ldo831_col63": lib.gte_token_pool_access_bytes(_lib.ptr(table), D, _lib.ptr(wide831[:, 63:]), 831)}
out["max_abs_diff_to_plain_torch"] = float((packed - want).abs().max())
out["layouts_bit_equal"] = bool(torch.equal(packed, wide832[:, 64:]) and torch.equal(packed, wide831[:, 63:]))
out["packed_GBps"] = round(out["bytes_needed_MB"] / 1e3 / (out["token_pool_packed_us"]["median"] * 1e-6), 1)
print(json.dumps(out), flush=True)
