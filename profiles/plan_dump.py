"""The gte_step_plan of every one-call step / forward of a short run, field by field: a refactor of the plan's host side (buffer
sets, weight images, the binder) leaves this file's output unchanged.

    python profiles/plan_dump.py --in-feats 831 --hidden 256 --resident --out plans.txt      (appends one section to --out)

Wraps ``engine.lib`` and reads ``_lib.StepPlan.from_address`` at each gte_gcnsage_step / gte_gcnsage_forward call; touches nothing
else of the engine, so the same file runs on any commit.  Written per call: every non-pointer field of the plan and of
layer[0 .. n_hidden) by name; every pointer field as 0 or pN, N numbering the distinct addresses by first appearance in field
order (null patterns and aliasing, not addresses); tn - logits and q_out - dl in bytes where the plan makes them halves of one
buffer (out_gemm; otherwise they are allocations of their own, whose distance is the allocator's, not the plan's: "separate",
or "overlap" within one class-count-wide row buffer); every weight-image descriptor with its
source as an offset from flat_param and its destination as pN + offset against the nearest plan pointer at or below it.  Runs:
two eager steps; ``--forward``: attach_feature_image + forward_logits; ``--capture``: capture (warm-up and captured calls) and one
replay.  One process per configuration (the library reads its GEMM mode at load).
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


def dump_plan(addr: int, param0: int) -> list:
    plan = _lib.StepPlan.from_address(addr)
    names = {}                                           # address -> N

    def show(struct, prefix, out):
        for name, typ in struct._fields_:
            v = getattr(struct, name)
            if name == "layer":
                for i in range(plan.n_hidden):
                    show(v[i], f"layer[{i}].", out)
            elif typ is ctypes.c_void_p:
                out.append(f"{prefix}{name} = " + ("0" if not v else f"p{names.setdefault(v, len(names))}"))
            else:
                out.append(f"{prefix}{name} = {v!r}")
    out = []
    show(plan, "", out)
    for hi, lo in (("tn", "logits"), ("q_out", "dl")):
        d = (getattr(plan, hi) or 0) - (getattr(plan, lo) or 0)
        own = "separate" if abs(d) >= 4 * plan.n_nodes * plan.n_classes else "overlap"
        out.append(f"{hi} - {lo} = {d if plan.out_gemm else own}")
    descs = (_lib.P3Desc * max(plan.n_wimg_descs, 0)).from_address(plan.wimg_descs) if plan.wimg_descs else []
    for j, d in enumerate(descs):
        base = max((a for a in names if a <= d.dst), default=None)
        dst = "?" if base is None else f"p{names[base]} + {d.dst - base}"
        out.append(f"wimg[{j}] rows {d.rows} cols {d.cols} transpose {d.transpose} ld {d.ld} ldp {d.ldp} src param + {d.src - param0} "
                   f"dst {dst}")
    return out


class PlanDumper:
    """Stands in for the loaded library: the two plan entry points note their plan before they run."""

    def __init__(self, lib, param0):
        self._lib, self._param0, self.lines = lib, param0, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("gte_gcnsage_step", "gte_gcnsage_forward"):
            return fn

        def call(addr, *rest):
            phase = f" phase {int(rest[0])}" if name == "gte_gcnsage_step" else ""
            self.lines.append(f"-- {name}{phase}")
            self.lines += dump_plan(addr, self._param0)
            return fn(addr, *rest)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-feats", type=int, default=831)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--resident", action="store_true", help="a batch of resident pages (the images the engine wants)")
    ap.add_argument("--forward", action="store_true", help="attach_feature_image + forward_logits instead of steps")
    ap.add_argument("--capture", action="store_true", help="capture the batch and replay it once instead of eager steps")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dev = "cuda:0"
    pages = S.make_pages(a.pages, in_feats=a.in_feats)
    torch.manual_seed(7)
    model = gte.GcnSAGE(a.in_feats, a.hidden, 9, a.layers, torch.nn.functional.relu, a.dropout).to(dev)
    eng = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4, dropout_seed=11)
    if a.resident:
        graphs = []
        for p in pages:
            pg = gte.PageGraph(p.src, p.dst, p.num_nodes)
            pg.ndata["feat"], pg.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
            pg.edata["feat"] = torch.from_numpy(p.weight)
            graphs.append(pg)
        res = G.ResidentPages(graphs, dev)
        if eng.wants_resident_images(a.in_feats):
            res.enable_p3(agg=bool(eng.wants_agg_image(a.in_feats)))
        g = res.batch(list(range(a.pages)))
        y = g.ndata["label"]
    else:
        src, dst, w, feat, label, off = S.concat_pages(pages)
        g = G.PageGraph(src, dst, int(off[-1]), device=dev)
        g.ndata["feat"], g.edata["feat"] = torch.from_numpy(feat).to(dev), torch.from_numpy(w).to(dev)
        y = torch.from_numpy(label).to(dev)
    rec = eng.lib = PlanDumper(eng.lib, eng.flat_param.data_ptr())
    if a.forward:
        eng.attach_feature_image(g)
        out = eng.forward_logits(g)
    elif a.capture:
        replay = eng.capture(g, y)
        out = replay()
    else:
        eng.step(g, y)
        out = eng.step(g, y)
    torch.cuda.synchronize()
    assert np.isfinite(out.float().cpu().numpy()).all()
    n_calls = sum(ln.startswith("-- ") for ln in rec.lines)
    flags = "".join(f" {k}" for k in ("resident", "forward", "capture") if getattr(a, k))
    with open(a.out, "a") as f:
        f.write(f"== in_feats {a.in_feats} hidden {a.hidden} layers {a.layers} pages {a.pages} dropout {a.dropout}{flags}: "
                f"{n_calls} plan calls\n")
        f.write("\n".join(rec.lines) + "\n")
    print(f"{n_calls} plan calls -> {a.out}")


if __name__ == "__main__":
    main()
