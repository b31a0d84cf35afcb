"""The Gaussian mixture of train_gmm at the reference's size: 2 000 000 synthetic numerals, 20 components, 100 EM iterations forced
(tol = 0), soft and hard.  One JSON line with
  (a) the device route of components/tables/gmm.py between ONE pair of events: the upload of the samples and the parameter block,
      the iterations in chunks of 8 with the 64-byte state read back after each, the download of the parameters, and the
      posterior of 50 000 points (upload, one launch, download); and the time of ONE iteration, from 3 groups of 10 iterations each
      between their own event pairs (a warm-up group first), the median;
  (b) sklearn.mixture.GaussianMixture.fit on the same samples and initial parameters on this machine's host cores, wall time
      (soft only: scikit-learn has no hard variant), and how far the two fits are apart.
A record of one run, no threshold.  Not measured: other n or K, the hard variant on the host, the reference's own machine.
usage: python profiles/gmm_time.py [--no-sklearn] [--n N] [--iters I]"""
import contextlib
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import graph as G                         # noqa: E402
from gnn_tableextraction_amd.components.tables import gmm as M         # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


N, K, ITERS, CHUNK, POINTS, GROUP = arg("--n", 2_000_000), 20, arg("--iters", 100), 8, 50_000, 10
dev = torch.device("cuda", 0)
INIT_STATE = [0, 0, 0, 0, -np.inf, -np.inf, 0, 0]


def numerals():
    """Numeral-like samples: a mixture of magnitudes, rounded to float32 as parsed numerals are."""
    rng = np.random.RandomState(0)
    centres, widths = rng.uniform(0.0, 200.0, size=12), rng.uniform(0.5, 8.0, size=12)
    which = rng.randint(12, size=N)
    x = (centres[which] + widths[which] * rng.standard_normal(N)).astype(np.float32).astype(np.float64)
    return x, rng.choice(x, K)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    warnings.simplefilter("ignore")
    x, prototypes = numerals()
    w, mu, prec = M.init_from_prototypes(x, prototypes)
    points = np.ascontiguousarray(x[:POINTS])
    record = {"samples": N, "components": K, "iterations": ITERS, "chunk": CHUNK, "posterior_points": POINTS}
    results = {}
    for kind in ("soft", "hard"):
        prepared = M.prepare(x, w, mu, prec, hard=kind == "hard", tol=0.0, max_iter=ITERS)
        # one iteration: groups of GROUP iterations on fresh parameters, max_iter far away (a warm-up group first)
        x_d = torch.from_numpy(prepared.x).to(dev)
        ws = G.gmm_workspace(N, K, dev)
        per_iter = []
        for _ in range(4):
            P_d = torch.from_numpy(prepared.P).to(dev)
            state = torch.tensor(INIT_STATE, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            _, ms = timed(lambda: G.gmm_iterate(x_d, P_d, prepared.hard, 0.0, prepared.reg_covar, 10 ** 6, GROUP, ws, state))
            per_iter.append(ms / GROUP)
        per_iter = per_iter[1:]
        del x_d, ws, P_d
        torch.cuda.synchronize()

        # the route as train_gmm takes it
        def route():
            result = M.run(prepared, dev, chunk=CHUNK)
            return result, M.predict_proba(result, points, dev)
        (result, proba), route_ms = timed(route)
        results[kind] = result
        record.update({f"{kind}_device_route_ms": round(route_ms, 1), f"{kind}_device_ms_per_iteration_median": round(float(np.median(per_iter)), 3),
                       f"{kind}_device_ms_per_iteration_all": [round(v, 3) for v in per_iter], f"{kind}_n_iter": result.n_iter_,
                       f"{kind}_lower_bound": result.lower_bound_, f"{kind}_posterior_row_sum_off": float(np.abs(proba.sum(axis=1) - 1).max())})
    if "--no-sklearn" not in sys.argv:
        from sklearn.mixture import GaussianMixture
        print("device side:", json.dumps(record), file=sys.stderr, flush=True)      # (the host fit takes minutes: progress on stderr)
        est = GaussianMixture(K, weights_init=w, means_init=mu, precisions_init=prec, tol=0.0, max_iter=ITERS, verbose=2, verbose_interval=10)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):
            est.fit(x.reshape(-1, 1))
        sk_ms = 1e3 * (time.perf_counter() - t0)
        r = results["soft"]
        rel = lambda a, b: float(np.max(np.abs(np.ravel(a) - np.ravel(b)) / np.abs(np.ravel(b))))
        record.update({"sklearn_fit_ms_host_wall": round(sk_ms, 1), "sklearn_n_iter": int(est.n_iter_),
                       "sklearn_ms_per_iteration": round(sk_ms / est.n_iter_, 1), "host_cpus": len(os.sched_getaffinity(0)),
                       "soft_vs_sklearn_rel": {"weights": rel(r.weights_, est.weights_), "means": rel(r.means_, est.means_),
                                               "covariances": rel(r.covariances_, est.covariances_),
                                               "lower_bound": rel([r.lower_bound_], [est.lower_bound_])}})
    print(json.dumps(record), flush=True)


main()
