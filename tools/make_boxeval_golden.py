"""Golden cases of the box-level evaluation  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the reference tree).

Runs the REFERENCE's own functions -- calc_iou_individual, get_single_image_results, calc_precision_recall,
get_model_scores_map and get_avg_precision_at_iou of src/utils/metrics.py, cut out of their file with ``ast`` at run time (the
module imports matplotlib / pandas / seaborn at its top and cannot be imported here); none of their text is held in this
repository -- on generated documents and writes tests/golden/boxeval_cases.json: the documents plus the reference's
``precisions``, ``recalls`` and ``avg_prec`` per IoU threshold.

A document is kept only if, in every paired cell (page x kind), no two candidates of equal IoU share a prediction or a ground
truth at the lowest threshold (hence at every threshold and after every pruning: those candidates are subsets): the
reference orders equal IoUs by ``np.argsort(ious)[::-1]``, which is unspecified, and with this filter its answer does not depend
on that order.

    python tools/make_boxeval_golden.py [reference/src]        # writes tests/golden/boxeval_cases.json
"""
import ast
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import boxeval_ref as ref                                   # noqa: E402

NAMES = ("calc_iou_individual", "get_single_image_results", "calc_precision_recall", "get_model_scores_map", "get_avg_precision_at_iou")
IOU_THRS = np.linspace(0.5, 0.95, 10)
KINDS = ("table", "text", "figure")
SCORES = (0.25, 0.5, 0.75, 1.0)                            # few values: equal scores across pages are the rule


def reference_functions(src_root):
    """The five functions, compiled together in ONE namespace (they call each other) that holds what their bodies use."""
    path = os.path.join(src_root, "utils", "metrics.py")
    text = open(path).read()
    ns = {"np": np, "deepcopy": copy.deepcopy}
    found = {}
    for node in ast.parse(text).body:
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            found[node.name] = ast.get_source_segment(text, node)
    assert set(found) == set(NAMES), sorted(set(NAMES) - set(found))
    for name in NAMES:
        exec(compile(found[name], f"{path}:{name}", "exec"), ns)
    return ns


def make_document(rng):
    """Pages of ground-truth boxes on a jittered grid, predictions = jittered copies (some exact) of a part of them plus strays;
    per kind some pages carry only ground truth or only predictions; one kind has no prediction at all."""
    n_pages = int(rng.integers(3, 5))
    empty_kind = KINDS[int(rng.integers(0, len(KINDS)))]
    gt, pred = {k: {} for k in KINDS}, {k: {} for k in KINDS}
    for kind in KINDS:
        for p in range(n_pages):
            page = f"doc_{p}.png"
            cols, rows = int(rng.integers(1, 4)), int(rng.integers(1, 3))
            boxes = []
            for c in range(cols):
                for r in range(rows):
                    x0, y0 = 40 + 300 * c + int(rng.integers(0, 30)), 50 + 400 * r + int(rng.integers(0, 40))
                    boxes.append([x0, y0, x0 + int(rng.integers(60, 250)), y0 + int(rng.integers(40, 330))])
            role = rng.random()
            if role >= 0.1:                                             # (below: a page with predictions only)
                gt[kind][page] = boxes
            if kind == empty_kind or 0.1 <= role < 0.2:                 # (a page with ground truth only)
                continue
            pb, ps = [], []
            for b in boxes:
                if rng.random() < 0.8:
                    j = rng.integers(-18, 19, 4) if rng.random() < 0.75 else np.zeros(4, dtype=np.int64)
                    q = [b[0] + int(j[0]), b[1] + int(j[1]), b[2] + int(j[2]), b[3] + int(j[3])]
                    pb.append(q)
                    ps.append(SCORES[int(rng.integers(1, len(SCORES)))])
            for _ in range(int(rng.integers(0, 3))):                    # strays, low scores
                x0, y0 = int(rng.integers(0, 900)), int(rng.integers(0, 900))
                pb.append([x0, y0, x0 + int(rng.integers(20, 200)), y0 + int(rng.integers(20, 200))])
                ps.append(SCORES[int(rng.integers(0, 2))])
            if pb:
                order = rng.permutation(len(pb))
                pred[kind][page] = {"bboxes": [pb[i] for i in order], "scores": [ps[i] for i in order]}
    return gt, pred, empty_kind


def tie_free(gt, pred):
    for kind in KINDS:
        for page, boxes in gt[kind].items():
            if page in pred[kind] and ref.has_shared_tie(pred[kind][page]["bboxes"], boxes, float(IOU_THRS[0])):
                return False
    return True


def main(src_root):
    fn = reference_functions(src_root)
    rng = np.random.default_rng(20260)
    cases, restated = [], 0
    seen = dict(lag=0, unpaired_gt=0, unpaired_pred=0, equal_across_pages=0, empty_kind=0)
    for _ in range(200):
        gt, pred, empty_kind = make_document(rng)
        if not tie_free(gt, pred):
            continue
        want = {}
        for kind in KINDS:
            res = [fn["get_avg_precision_at_iou"](copy.deepcopy(gt[kind]), copy.deepcopy(pred[kind]), iou_thr=float(t)) for t in IOU_THRS]
            want[kind] = {"precisions": [[float(v) for v in r["precisions"]] for r in res],
                          "recalls": [[float(v) for v in r["recalls"]] for r in res], "avg_prec": [float(r["avg_prec"]) for r in res]}
            # the restatement of tests/boxeval_ref.py, re-verified on every document that is written
            for r, t in zip(res, IOU_THRS):
                mine = ref.avg_precision_at_iou(gt[kind], pred[kind], float(t))
                assert mine["precisions"] == [float(v) for v in r["precisions"]] and mine["recalls"] == [float(v) for v in r["recalls"]]
                assert abs(mine["avg_prec"] - float(r["avg_prec"])) <= 1e-12
                restated += 1
            paired = [pg for pg in gt[kind] if pg in pred[kind]]
            seen["lag"] += any(len(set(pred[kind][pg]["scores"])) >= 3 for pg in paired)
            seen["unpaired_gt"] += any(pg not in pred[kind] for pg in gt[kind]) and bool(pred[kind])
            seen["unpaired_pred"] += any(pg not in gt[kind] for pg in pred[kind])
            sets = [set(pred[kind][pg]["scores"]) for pg in paired]
            seen["equal_across_pages"] += any(sets[a] & sets[b] for a in range(len(sets)) for b in range(a + 1, len(sets)))
        seen["empty_kind"] += not pred[empty_kind] and bool(gt[empty_kind])
        cases.append({"gt": gt, "pred": pred, "ref": want})
        if len(cases) == 30:
            break
    assert len(cases) >= 30, len(cases)
    assert all(v >= 5 for v in seen.values()), seen
    out = os.path.join(ROOT, "tests", "golden", "boxeval_cases.json")
    with open(out, "w") as f:
        json.dump({"iou_thrs": [float(t) for t in IOU_THRS], "kinds": list(KINDS), "cases": cases}, f, separators=(",", ":"))
    print(f"{out}: {len(cases)} documents, {os.path.getsize(out)} bytes, {restated} curves restated exactly, coverage {seen}")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        from oracle.make_aux_golden import REF                          # where the other golden tools read the reference
        main(REF)
