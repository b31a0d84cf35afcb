"""The C-ABI calls of ONE eager training step, by name and non-pointer arguments: a refactor of the host schedule leaves this
file's output unchanged.

    GTE_C_STEP=0 python profiles/call_trace.py --in-feats 831 --hidden 256 --out trace.txt      (appends one section to --out)

Wraps ``engine.lib`` in a recorder and touches nothing else of the engine, so the same file runs on any commit.  An argument is a
pointer where ``_lib.SIGNATURES`` says c_void_p (device addresses, streams, by-reference outputs): skipped.  Calls that do not go
through ``engine.lib`` (the ops module's own) are not seen.  The library reads its GEMM mode at load: one process per
configuration (the switches -- GTE_C_STEP, GTE_GEMM_MODE, GTE_TRANSFORM_FIRST, GTE_PLANES -- come from the environment and are
written into the section header).  Records host-side calls only; no profiler is attached.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_tableextraction_amd as gte                                   # noqa: E402
from gnn_tableextraction_amd import _lib, graph as G                     # noqa: E402
from gnn_tableextraction_amd.data import synthetic as S                  # noqa: E402
from gnn_tableextraction_amd.models.engine import FusedGcnSageStep       # noqa: E402

SCALARS = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float)     # everything else in a signature is a pointer
SWITCHES = ("GTE_C_STEP", "GTE_GEMM_MODE", "GTE_TRANSFORM_FIRST", "GTE_PLANES")


class Recorder:
    """Stands in for the loaded library: every attribute is the library's function behind a wrapper that notes the call."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = _lib.SIGNATURES.get(name)
        if sig is None:
            return fn
        types = sig[1]

        def call(*args):
            vals = [repr(float(a)) if t is ctypes.c_float else str(int(a)) for a, t in zip(args, types) if t in SCALARS]
            self.calls.append(f"{name}({', '.join(vals)})")
            return fn(*args)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-feats", type=int, default=831)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--pages", type=int, default=12)
    ap.add_argument("--resident", action="store_true", help="a batch of resident pages (image features where the engine wants them)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dev = "cuda:0"
    pages = S.make_pages(a.pages, in_feats=a.in_feats)
    torch.manual_seed(7)
    model = gte.GcnSAGE(a.in_feats, a.hidden, 9, 3, torch.nn.functional.relu, 0).to(dev)
    eng = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
    if a.resident:
        graphs = []
        for p in pages:
            pg = gte.PageGraph(p.src, p.dst, p.num_nodes)
            pg.ndata["feat"], pg.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
            pg.edata["feat"] = torch.from_numpy(p.weight)
            graphs.append(pg)
        res = G.ResidentPages(graphs, dev)
        if eng.wants_p3_features(a.in_feats):
            res.enable_p3()
        g = res.batch(list(range(a.pages)))
        y = g.ndata["label"]
    else:
        src, dst, w, feat, label, off = S.concat_pages(pages)
        g = G.PageGraph(src, dst, int(off[-1]), device=dev)
        g.ndata["feat"], g.edata["feat"] = torch.from_numpy(feat).to(dev), torch.from_numpy(w).to(dev)
        y = torch.from_numpy(label).to(dev)
    rec = eng.lib = Recorder(eng.lib)
    out3 = eng.step(g, y)
    torch.cuda.synchronize()
    assert np.isfinite(out3.cpu().numpy()).all()
    env = " ".join(f"{k}={os.environ[k]}" for k in SWITCHES if k in os.environ)
    with open(a.out, "a") as f:
        f.write(f"== in_feats {a.in_feats} hidden {a.hidden} pages {a.pages}{' resident' if a.resident else ''} {env}: "
                f"{len(rec.calls)} calls\n")
        f.write("\n".join(rec.calls) + "\n")
    print(f"{len(rec.calls)} calls -> {a.out}")


if __name__ == "__main__":
    main()
