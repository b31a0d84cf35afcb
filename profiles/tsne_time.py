"""Exact t-SNE (3 components, the setting of train_repr) on the Levenshtein similarity matrix of 2000 synthetic word shapes under the
reference's costs, cleaned as train_repr cleans it (squared, NaN and infinities replaced) -- the stage of train_repr that follows
profiles/affprop_time.py.  JSON lines, each printed as soon as it is known:
  (a) the device route of components/tables/tsne.py under ONE pair of events: prepare (host), upload, the two probability kernels,
      the two phases with their state read-backs (one per 50 iterations), the read-back of the embedding; and the time of ONE
      iteration from 3 calls of 50 iterations each between their own event pairs (the median);
  (b) sklearn.manifold.TSNE on the same matrix on this machine's host cores, wall time of fit(): the default (Barnes-Hut), then
      method='exact'; with their kl_divergence_ and n_iter_.
A record of one run, no threshold.
usage: python profiles/tsne_time.py [--no-sklearn] [--no-exact]"""
import json
import os
import random
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import graph as G                         # noqa: E402
from gnn_tableextraction_amd.components.tables import levenshtein as L, tsne as T  # noqa: E402

N, D, SEED = 2000, 3, 0
dev = torch.device("cuda", 0)
SIGNS = "wx.,-%()/:+'#"


def shapes(lo, hi, seed):
    rnd, words = random.Random(seed), ["<UNK_W>"]
    while len(words) < N:
        w = "".join(rnd.choice(SIGNS) for _ in range(rnd.randint(lo, hi)))
        if w not in words:
            words.append(w)
    return words


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    warnings.simplefilter("ignore")
    sim = L.LevenshteinSimilitudes().init_weights().calculate_similarity(shapes(1, 12, 1), device=dev)
    matrix = np.square(sim)                                            # (train_repr's cleaning)
    finite = matrix[matrix != np.inf]
    matrix = np.nan_to_num(matrix, nan=np.nanmean(finite), posinf=np.nanmax(finite), neginf=np.nanmax(finite))

    T.tsne(matrix[:64, :64], D, perplexity=10, random_state=SEED, device=dev)          # warm-up: library, kernels, allocator
    torch.cuda.synchronize()
    (Y, info), route_ms = timed(lambda: T.run(T.prepare(matrix, D, random_state=SEED), dev))

    prepared = T.prepare(matrix, D, random_state=SEED)
    ws = G.tsne_workspace(N, dev)
    P = G.tsne_joint_p(G.tsne_cond_p(torch.from_numpy(prepared.sq_dist).to(dev), prepared.perplexity)[0], ws)
    Yb = torch.zeros((2, N, D), dtype=torch.float64, device=dev)
    Yb[0].copy_(torch.from_numpy(prepared.init))
    update, gains = torch.zeros((N, D), dtype=torch.float64, device=dev), torch.ones((N, D), dtype=torch.float64, device=dev)
    state = torch.tensor([0, 0, 0, 0, 0, 1.7e308, 1.7e308, 0], dtype=torch.float64, device=dev)
    per_iter = []
    for _ in range(4):
        _, ms = timed(lambda: G.tsne_iterate(P, Yb, update, gains, prepared.learning_rate, 0.5, 12.0, 10 ** 6, 0.0, 10 ** 6, 50, ws, state))
        per_iter.append(ms / 50)
    per_iter = per_iter[1:]
    record = {"words": N, "n_components": D, "perplexity": prepared.perplexity, "learning_rate": prepared.learning_rate,
              "device_route_ms": round(route_ms, 1), "device_n_iter": info["n_iter"], "device_kl_divergence": round(info["kl_divergence"], 5),
              "device_stop_reason": info["stop_reason"], "device_ms_per_iteration_median": round(float(np.median(per_iter)), 4),
              "device_ms_per_iteration_all": [round(x, 4) for x in per_iter], "embedding_finite": bool(np.isfinite(Y).all())}
    print(json.dumps(record), flush=True)
    if "--no-sklearn" in sys.argv:
        return
    from sklearn.manifold import TSNE
    for method in ["barnes_hut"] + ([] if "--no-exact" in sys.argv else ["exact"]):
        t0 = time.perf_counter()
        est = TSNE(n_components=D, metric="precomputed", init="random", random_state=SEED, method=method).fit(matrix)
        ms = 1e3 * (time.perf_counter() - t0)
        print(json.dumps({"sklearn_method": method, "sklearn_fit_ms_host_wall": round(ms, 1), "sklearn_n_iter": int(est.n_iter_),
                          "sklearn_kl_divergence": round(float(est.kl_divergence_), 5), "host_cpus": len(os.sched_getaffinity(0))}),
              flush=True)


main()
