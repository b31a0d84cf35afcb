"""One sha256 per call of the stand-alone LayerNorm(+ReLU) entry points on the inputs of tests/layernorm_cases.py: a restructuring of
the kernels behind them leaves this file's output unchanged, byte for byte.

    GTE_LIB_PATH=/path/to/libgte_hip.so python profiles/ln_hash_dump.py --out hashes.txt

Entry points: gte_ln_relu_fwd, gte_ln_relu_bwd at the widths PLAIN_NS of tests/test_gpu_layernorm.py, gte_ln_relu_fwd_p3,
gte_ln_relu_bwd_p3 at IMAGE_NS, gte_ln_relu_bwd_workspace_bytes (its value) at both; rows MS of layernorm_cases, M_BIG at the widths
that module runs it at; every case (planted kinds, eps) of layernorm_cases.cases with ReLU on and off.  Hashed per call: EVERY output
buffer whole -- y / dz with their padding columns (NaN before the call: a stray write shows), the statistics, the three column sums
and the P3 image with its padding.  The backward reads the statistics the same library's forward wrote.  Uses only the C ABI and
the test helpers, so the same file runs on any commit; one process per library (GTE_LIB_PATH is read at import).
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tableextraction_amd import _lib                                 # noqa: E402
from tests import layernorm_cases as lc                                  # noqa: E402
from tests import test_gpu_layernorm as T                                # noqa: E402


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    lib = _lib.load()
    lines = []
    for image, ns, big in ((False, T.PLAIN_NS, T.PLAIN_BIG), (True, T.IMAGE_NS, T.IMAGE_BIG)):
        sfx = "_p3" if image else ""
        for n in ns:
            for m, _, vi, plant, eps, unit, seed in lc.cases([n], n if n in big else None):
                z, dy, gamma, beta = lc.make_case(m, n, plant, seed, unit)
                ld = T.c4(n) + 4 if image else n + (8 if n % 4 == 0 and m % 2 else 5)
                gd, bd, zb, gb = T.dev(gamma), T.dev(beta), T.padded(z, ld), T.padded(dy, ld)
                kinds = ",".join(f"{r}:{k}" for r, k in sorted(plant.items())) or "-"
                for relu in (1, 0):
                    tag = f"n={n} M={m} v{vi} [{kinds}] eps={eps} unit={int(unit)} relu={relu}"
                    yb, img, stats = T.run_fwd(zb, n, gd, bd, eps, relu, image)
                    lines.append(f"gte_ln_relu_fwd{sfx} {tag} {sha(yb, stats, img.data if image else None)}")
                    dzb, dimg, dg, db, dbias = T.run_bwd(gb, zb, stats, n, gd, bd, relu, image)
                    lines.append(f"gte_ln_relu_bwd{sfx} {tag} {sha(dzb, dimg.data if image else None, dg, db, dbias)}")
                    lines.append(f"gte_ln_relu_bwd_workspace_bytes n={n} M={m} {int(lib.gte_ln_relu_bwd_workspace_bytes(m, n))}")
    torch.cuda.synchronize()
    lines = list(dict.fromkeys(lines))                                    # (the workspace size repeats per case)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {a.out}: sha256 {hashlib.sha256(open(a.out, 'rb').read()).hexdigest()}")


if __name__ == "__main__":
    main()
