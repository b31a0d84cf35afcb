"""Per-launch time of the stand-alone LayerNorm(+ReLU) entry points, for A/B runs of two builds of the library.

    GTE_LIB_PATH=/path/to/libgte_hip.so python profiles/ln_launch_time.py --out times_A_1.json     (one process per library and round)
    python profiles/ln_launch_time.py --summarise A=times_A_*.json B=times_B_*.json               (no GPU)

Rows x widths: 24 300 x {256, 218, 512, 1000}; gte_ln_relu_fwd, gte_ln_relu_fwd_p3, gte_ln_relu_bwd, gte_ln_relu_bwd_p3 (the plain
entry points on the same padded rows; at 218 and 1000 they run the scalar kernels).  Per configuration: 20 warm-up launches, then
200 launches between ONE pair of events; us per launch.  The backward's time includes its column-sum fold launch.  --summarise
prints every run, B's median and A's slowest run per configuration, and "pass" where B's median is not above A's slowest.
"""
import argparse
import glob
import json
import os
import statistics
import sys

ROWS, WIDTHS, LAUNCHES, WARMUP = 24300, (256, 218, 512, 1000), 200, 20


def measure(out):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gnn_tableextraction_amd import _lib, ops
    lib, P, cs, check = _lib.load(), _lib.ptr, _lib.current_stream, _lib.check
    dev = "cuda:0"
    torch.manual_seed(3)
    res = {}
    for n in WIDTHS:
        ld = -(-n // 16) * 16
        z = torch.randn(ROWS, ld, device=dev)
        dy = torch.randn(ROWS, ld, device=dev)
        z[:, n:] = 0
        dy[:, n:] = 0
        gamma, beta = torch.rand(n, device=dev) + 0.5, torch.randn(n, device=dev)
        y, dz, stats = torch.empty_like(z), torch.empty_like(z), torch.empty(2 * ROWS, device=dev)
        sums = [torch.empty(n, device=dev) for _ in range(3)]
        img = ops.P3.empty(ROWS, n, dev)
        nbytes = int(lib.gte_ln_relu_bwd_workspace_bytes(ROWS, n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        calls = {
            "fwd": lambda: lib.gte_ln_relu_fwd(P(z), ld, P(gamma), P(beta), 1e-5, 1, P(y), ld, P(stats), ROWS, n, cs()),
            "fwd_p3": lambda: lib.gte_ln_relu_fwd_p3(P(z), ld, P(gamma), P(beta), 1e-5, 1, P(y), ld, P(img.data), img.ldp, P(stats), ROWS, n,
                                                     cs()),
            "bwd": lambda: lib.gte_ln_relu_bwd(P(dy), ld, P(z), ld, P(stats), P(gamma), P(beta), 1, P(dz), ld, P(sums[0]), P(sums[1]),
                                               P(sums[2]), ROWS, n, P(ws), nbytes, cs()),
            "bwd_p3": lambda: lib.gte_ln_relu_bwd_p3(P(dy), ld, P(z), ld, P(stats), P(gamma), P(beta), 1, P(dz), ld, P(img.data), img.ldp,
                                                     P(sums[0]), P(sums[1]), P(sums[2]), ROWS, n, P(ws), nbytes, cs()),
        }
        for name, call in calls.items():
            for _ in range(WARMUP):
                check(call(), name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                call()
            e1.record()
            torch.cuda.synchronize()
            check(call(), name)
            res[f"{name} n={n}"] = 1e3 * e0.elapsed_time(e1) / LAUNCHES
    torch.cuda.synchronize()
    json.dump(res, open(out, "w"), indent=1)
    print(out, " ".join(f"{k}: {v:.2f}" for k, v in res.items()))


def summarise(groups):
    runs = {}
    for g in groups:
        tag, pattern = g.split("=", 1)
        runs[tag] = [json.load(open(f)) for f in sorted(glob.glob(pattern))]
    assert len(runs) == 2 and all(runs.values()), "two tags, at least one file each"
    (ta, a), (tb, b) = runs.items()
    assert all(r.keys() == a[0].keys() for r in a + b), "every run measures the same configurations"
    for key in a[0]:
        va, vb = [r[key] for r in a], [r[key] for r in b]
        med, slow = statistics.median(vb), max(va)
        print(f"{key:16s} {ta} " + " ".join(f"{v:7.2f}" for v in va) + f"   slowest {slow:7.2f}, spread {100 * (max(va) / min(va) - 1):.1f} %")
        print(f"{'':16s} {tb} " + " ".join(f"{v:7.2f}" for v in vb) + f"   median  {med:7.2f}   {'pass' if med <= slow else 'FAIL'}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--summarise", nargs=2, metavar="TAG=GLOB")
    a = ap.parse_args()
    summarise(a.summarise) if a.summarise else measure(a.out)
