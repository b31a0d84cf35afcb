"""Train-loop ms/step with dropout (MI355X): the fused step (FusedGcnSageStep, GTE_LAYER_DROPOUT layers) at p = 0 / 0.1 / 0.5
against the autograd path (TrainStep) at p = 0.1, on the bench workload (100 pages per step, GcnSAGE(f0, hidden, 9, 3)).

Every variant has its own resident page set (the form its engine asks for: fp32 rows, the feature image, or feature + cached
aggregate images) and is warmed up first; the timed rounds then ALTERNATE the variants, ``--rounds`` times, so that the spread of
each figure is known.  A round = ``--steps`` steps of models/loop.run_steps (the loop train() runs), synchronised at both ends.
usage: python profiles/r07/dropout_step.py [--shapes 831x256,831x1000,13x218] [--steps 30] [--rounds 3] [--only VARIANT]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import distributed as D, graph as G
from gnn_tableextraction_amd.data import synthetic as S
from gnn_tableextraction_amd.models import loop
from gnn_tableextraction_amd.models.engine import FusedGcnSageStep, TrainStep

VARIANTS = [("fused", 0.0), ("fused", 0.1), ("fused", 0.5), ("trainstep", 0.1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="831x256,831x1000,13x218")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pages", type=int, default=600)
    ap.add_argument("--only", default=None, help="one variant, e.g. fused-0.1 (profiler runs)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    variants = [v for v in VARIANTS if args.only is None or f"{v[0]}-{v[1]}" == args.only]
    out = {"device": torch.cuda.get_device_name(0), "steps_per_round": args.steps, "rounds": args.rounds, "shapes": {}}
    for shape in args.shapes.split(","):
        f0, hid = (int(v) for v in shape.split("x"))
        pages = S.make_pages(args.pages, in_feats=f0)
        gs = []
        for p in pages:
            g = G.PageGraph(p.src, p.dst, p.num_nodes)
            g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
            g.edata["feat"] = torch.from_numpy(p.weight)
            gs.append(g)
        runs = {}
        for kind, p in variants:
            torch.manual_seed(42)
            model = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, p).to(dev)
            step = (FusedGcnSageStep(model, dropout_seed=42, lr=0.01, weight_decay=5e-4) if kind == "fused"
                    else TrainStep(model, lr=0.01, weight_decay=5e-4))
            res = G.ResidentPages(gs, dev)
            pipe = loop.BatchPipeline(res)
            sizes = res.page_sizes()
            plan = [r[0] for ep in range(200) for r in D.plan_epoch(sizes, 100, 1, seed=42, epoch=ep)]
            runs[(kind, p)] = {"step": step, "pipe": pipe, "plan": plan, "pos": 0, "ms": [], "nodes": [], "sizes": np.asarray(sizes)}
        for key, r in runs.items():                       # warm-up: buffers, plans, images, compiled paths
            loop.run_steps(r["step"], r["pipe"], r["plan"][:8])
            r["pos"] = 8
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for key, r in runs.items():
                chunk = r["plan"][r["pos"]:r["pos"] + args.steps]
                r["pos"] += args.steps
                nodes = int(sum(r["sizes"][np.asarray(ids)].sum() for ids in chunk))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop.run_steps(r["step"], r["pipe"], chunk)
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) / len(chunk) * 1e3)
                r["nodes"].append(nodes / len(chunk))
        res_shape = {}
        for (kind, p), r in runs.items():
            ms = np.asarray(r["ms"])
            st = r["step"]
            res_shape[f"{kind} p={p}"] = {
                "ms_per_step": [round(float(v), 4) for v in ms], "median_ms": round(float(np.median(ms)), 4),
                "spread_ms": round(float(ms.max() - ms.min()), 4), "nodes_per_step": round(float(np.mean(r["nodes"])), 1),
                "plan_kinds": (st._plan_kinds(f0, int(np.mean(r["nodes"]))) if isinstance(st, FusedGcnSageStep) else None)}
        base = res_shape.get("fused p=0.0", {}).get("median_ms")
        for k, v in res_shape.items():
            if base:
                v["vs_fused_p0"] = round(v["median_ms"] / base, 3)
        ts = res_shape.get("trainstep p=0.1", {}).get("median_ms")
        for k, v in res_shape.items():
            if ts and k.startswith("fused"):
                v["vs_trainstep_p0.1"] = round(v["median_ms"] / ts, 3)
        out["shapes"][f"GcnSAGE({f0}, {hid}, 9, 3)"] = res_shape
        del runs
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
