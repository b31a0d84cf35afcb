"""One gte_predict_head launch (class + confidence, and with the softmax row) beside the torch formulation of the same quantities
-- torch.argmax(logits, 1, out=...) + torch.softmax(logits, 1).max(1) (and the softmax kept, for the row) -- on the SAME logits
tensor, at the validation set's size (478 000 nodes, C = 9) and at one batch of 100 pages (21 532 nodes): 20 warm-up rounds, then
200 rounds in which the formulations ALTERNATE, each call between its own event pair; medians in microseconds.  The predictions
are compared exactly, the confidences by their largest difference (torch's softmax is float32).
usage: python profiles/predict_head_time.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from gnn_tableextraction_amd import ops                                # noqa: E402

WARMUP, ROUNDS, C = 20, 200, 9
dev = torch.device("cuda", 0)


def measure(n):
    g = torch.Generator(device="cpu").manual_seed(13)
    logits = (3.0 * torch.randn((n, C), generator=g)).to(dev)
    pred = torch.empty(n, dtype=torch.int64, device=dev)
    conf = torch.empty(n, dtype=torch.float32, device=dev)
    prob = torch.empty((n, C), dtype=torch.float32, device=dev)
    t_pred = torch.empty(n, dtype=torch.int64, device=dev)
    keep = {}

    def head():
        ops.predict_head(logits, out_pred=pred, out_conf=conf)

    def head_prob():
        ops.predict_head(logits, out_pred=pred, out_conf=conf, out_prob=prob)

    def torch_form():
        torch.argmax(logits, dim=1, out=t_pred)
        keep["prob"] = torch.softmax(logits, dim=1)
        keep["conf"] = keep["prob"].max(dim=1).values

    forms = {"predict_head": head, "predict_head_with_prob": head_prob, "torch_argmax_softmax_max": torch_form}
    for _ in range(WARMUP):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    pairs = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {"nodes": n, "classes": C, "rounds": ROUNDS}
    for k, evs in pairs.items():
        us = [1000.0 * a.elapsed_time(b) for a, b in evs]
        out[k + "_us_median"] = round(float(np.median(us)), 2)
        out[k + "_us_min"] = round(float(np.min(us)), 2)
    out["pred_equal_to_torch"] = bool(torch.equal(pred, t_pred))
    out["conf_max_abs_diff_to_torch_f32"] = float((conf - keep["conf"]).abs().max())
    out["prob_max_abs_diff_to_torch_f32"] = float((prob - keep["prob"]).abs().max())
    return out


for n in (478_000, 21_532):
    print(json.dumps(measure(n)), flush=True)
