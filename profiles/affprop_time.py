"""Affinity propagation (damping 0.9, the setting of train_repr) on the Levenshtein similarity matrix of 2000 synthetic word shapes
under the reference's costs -- the stage of train_repr that follows profiles/lev_matrix_time.py.  One JSON line with
  (a) the device route of components/tables/affinity.py: prepare (host), upload, the sweep loop between one pair of events (the
      loop of ``run``: chunks of 16 sweeps, the 16-byte state read back after each), finish (host); and the time of ONE sweep,
      from 3 launches of 32 sweeps each between their own event pairs on fresh buffers that cannot stop (max_iter far away),
      the median;
  (b) sklearn.cluster.AffinityPropagation on the same matrix on this machine's host cores, wall time of fit();
  (c) the sweep counts of both, and whether centres and labels are equal.
A record of one run, no threshold.
usage: python profiles/affprop_time.py [--no-sklearn]"""
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
from gnn_tableextraction_amd.components.tables import affinity as AP, levenshtein as L  # noqa: E402

N, DAMPING, CONV, MAX_ITER, CHUNK, SEED = 2000, 0.9, 15, 200, 16, 0
dev = torch.device("cuda", 0)
SIGNS = "wx.,-%()/:+'#"


def shapes(lo, hi, seed):
    rnd, words = random.Random(seed), ["<UNK_W>"]
    while len(words) < N:
        w = "".join(rnd.choice(SIGNS) for _ in range(rnd.randint(lo, hi)))
        if w not in words:
            words.append(w)
    return words


def buffers(n, ci=CONV):
    return (torch.zeros((n, n), dtype=torch.float64, device=dev), torch.zeros((n, n), dtype=torch.float64, device=dev),
            torch.zeros(n, dtype=torch.uint8, device=dev), G.affprop_workspace(n, ci, dev), torch.zeros(4, dtype=torch.int32, device=dev))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    sim = L.LevenshteinSimilitudes().init_weights().calculate_similarity(shapes(1, 12, 1), device=dev)
    warnings.simplefilter("ignore")
    t0 = time.perf_counter()
    prepared = AP.prepare(sim, random_state=SEED)
    prepare_ms = 1e3 * (time.perf_counter() - t0)
    S_h = torch.from_numpy(prepared.S)

    # one sweep: 32 sweeps per launch group on fresh buffers, far from any stop (a warm-up group first)
    S_d = S_h.to(dev)
    per_sweep = []
    for _ in range(4):
        A, R, E, ws, state = buffers(N, 32)
        _, ms = timed(lambda: G.affprop_iterate(S_d, A, R, DAMPING, 32, 10 ** 6, 32, E, ws, state))   # ring of 32: no stop within 32 sweeps
        per_sweep.append(ms / 32)
    per_sweep = per_sweep[1:]
    del S_d

    # the route as ``run`` takes it
    torch.cuda.synchronize()
    (S_d), upload_ms = timed(lambda: S_h.to(dev))
    A, R, E, ws, state = buffers(N)

    def loop():
        enqueued, st = 0, [0, 0, 0, 0]
        while not st[1] and enqueued < MAX_ITER:
            sweeps = min(CHUNK, MAX_ITER - enqueued)
            G.affprop_iterate(S_d, A, R, DAMPING, CONV, MAX_ITER, sweeps, E, ws, state)
            enqueued += sweeps
            st = state.tolist()
        return st
    st, loop_ms = timed(loop)
    exemplars = E.cpu().numpy().astype(bool)
    t0 = time.perf_counter()
    centers, labels = AP.finish(prepared.S, exemplars, bool(st[2]))
    finish_ms = 1e3 * (time.perf_counter() - t0)
    record = {"words": N, "damping": DAMPING, "convergence_iter": CONV, "max_iter": MAX_ITER, "chunk": CHUNK,
              "device_sweeps": st[0], "device_converged": bool(st[2]), "clusters": int(len(centers)),
              "prepare_ms_host": round(prepare_ms, 1), "upload_ms": round(upload_ms, 2), "device_loop_ms": round(loop_ms, 2),
              "finish_ms_host": round(finish_ms, 1), "device_ms_per_sweep_median": round(float(np.median(per_sweep)), 4),
              "device_ms_per_sweep_all": [round(x, 4) for x in per_sweep]}
    if "--no-sklearn" not in sys.argv:
        from sklearn.cluster import AffinityPropagation
        t0 = time.perf_counter()
        est = AffinityPropagation(affinity="precomputed", damping=DAMPING, random_state=SEED).fit(sim)
        sk_ms = 1e3 * (time.perf_counter() - t0)
        record.update({"sklearn_fit_ms_host_wall": round(sk_ms, 1), "sklearn_sweeps": int(est.n_iter_),
                       "sklearn_ms_per_sweep": round(sk_ms / est.n_iter_, 2), "host_cpus": len(os.sched_getaffinity(0)),
                       "equal_to_sklearn": bool(np.array_equal(centers, est.cluster_centers_indices_) and np.array_equal(labels, est.labels_))})
    print(json.dumps(record), flush=True)


main()
