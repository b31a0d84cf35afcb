"""Golden cases of the box-level evaluation on FLOAT boxes  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the
reference tree).

The method of tools/make_boxeval_golden.py: the REFERENCE's own functions of src/utils/metrics.py, cut out of their file with
``ast`` at run time (none of their text is held in this repository), on generated documents; here the documents hold floats, as
the block route's document does, and the file -- tests/golden/boxeval_float_cases.json -- stores beside the reference's
``precisions``, ``recalls`` and ``avg_prec`` per IoU threshold the reference's own IoU (calc_iou_individual) of every pair of every
paired cell, ``iou[kind][page][prediction][ground truth]`` in document order: on floats every intermediate of the IoU rounds, and
these are the bits a device kernel has to reproduce.  JSON floats round-trip exactly (repr).

Documents: predictions are integer boxes divided by 0.36 (what the block route emits), ground truths carry quarter-pixel offsets,
scores are sevenths (equal scores across pages are the rule), at most 8 predictions per page and kind (the reference sorts scores
with np.argsort's default kind, order-preserving only for short arrays).  A document with a shared tie at the lowest threshold
in a paired cell is dropped (tools/make_boxeval_golden.py's filter, with the float IoU).  The restatement of
tests/boxeval_float_ref.py is verified on CHECKED documents, of which the first KEPT are written.

    python tools/make_boxeval_float_golden.py [reference/src]        # writes tests/golden/boxeval_float_cases.json
"""
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import boxeval_float_ref as ref                             # noqa: E402
from tools.make_boxeval_golden import reference_functions             # noqa: E402

IOU_THRS = np.linspace(0.5, 0.95, 10)
KINDS = ("table", "text", "figure")
SF = 0.36
CHECKED, KEPT = 60, 16


def make_document(rng):
    """Pages of ground-truth boxes on a jittered grid, rounded to quarter pixels of the document's coordinates, predictions = jittered integer copies (some
    exact before the division) of a part of them plus strays, all divided by 0.36; per kind some pages carry only ground truth or
    only predictions; one kind has no prediction at all."""
    n_pages = int(rng.integers(3, 5))
    empty_kind = KINDS[int(rng.integers(0, len(KINDS)))]
    gt, pred = {k: {} for k in KINDS}, {k: {} for k in KINDS}
    for kind in KINDS:
        for p in range(n_pages):
            page = f"doc_{p}.png"
            cols, rows = int(rng.integers(1, 4)), int(rng.integers(1, 3))
            boxes, whole = [], []
            for c in range(cols):
                for r in range(rows):
                    x0, y0 = 40 + 300 * c + int(rng.integers(0, 30)), 50 + 400 * r + int(rng.integers(0, 40))
                    b = [x0, y0, x0 + int(rng.integers(60, 250)), y0 + int(rng.integers(40, 330))]
                    whole.append(b)
                    boxes.append([round(v / SF * 4) / 4 for v in b])         # document coordinates, on quarter pixels
            role = rng.random()
            if role >= 0.1:                                             # (below: a page with predictions only)
                gt[kind][page] = boxes
            if kind == empty_kind or 0.1 <= role < 0.2:                 # (a page with ground truth only)
                continue
            pb, ps = [], []
            for b in whole:
                if rng.random() < 0.8:
                    j = rng.integers(-18, 19, 4) if rng.random() < 0.75 else np.zeros(4, dtype=np.int64)
                    pb.append([b[0] + int(j[0]), b[1] + int(j[1]), b[2] + int(j[2]), b[3] + int(j[3])])
                    ps.append(int(rng.integers(3, 8)) / 7)
            for _ in range(int(rng.integers(0, 3))):                    # strays, low scores
                x0, y0 = int(rng.integers(0, 900)), int(rng.integers(0, 900))
                pb.append([x0, y0, x0 + int(rng.integers(20, 200)), y0 + int(rng.integers(20, 200))])
                ps.append(int(rng.integers(1, 4)) / 7)
            if pb:
                assert len(pb) <= 8
                order = rng.permutation(len(pb))
                pred[kind][page] = {"bboxes": [[v / SF for v in pb[i]] for i in order], "scores": [ps[i] for i in order]}
    return gt, pred, empty_kind


def tie_free(gt, pred):
    for kind in KINDS:
        for page, boxes in gt[kind].items():
            if page in pred[kind] and ref.has_shared_tie(pred[kind][page]["bboxes"], boxes, float(IOU_THRS[0])):
                return False
    return True


def main(src_root):
    fn = reference_functions(src_root)
    rng = np.random.default_rng(20261)
    cases, restated, pairs, dropped = [], 0, 0, 0
    seen = dict(lag=0, unpaired_gt=0, unpaired_pred=0, equal_across_pages=0, empty_kind=0)
    for _ in range(400):
        gt, pred, empty_kind = make_document(rng)
        if not tie_free(gt, pred):
            dropped += 1
            continue
        keep = len(cases) < KEPT
        want, ious = {}, {}
        for kind in KINDS:
            res = [fn["get_avg_precision_at_iou"](copy.deepcopy(gt[kind]), copy.deepcopy(pred[kind]), iou_thr=float(t)) for t in IOU_THRS]
            want[kind] = {"precisions": [[float(v) for v in r["precisions"]] for r in res],
                          "recalls": [[float(v) for v in r["recalls"]] for r in res], "avg_prec": [float(r["avg_prec"]) for r in res]}
            # the restatement of tests/boxeval_float_ref.py, re-verified on every document
            for r, t in zip(res, IOU_THRS):
                mine = ref.avg_precision_at_iou(gt[kind], pred[kind], float(t))
                assert mine["precisions"] == [float(v) for v in r["precisions"]] and mine["recalls"] == [float(v) for v in r["recalls"]]
                assert abs(mine["avg_prec"] - float(r["avg_prec"])) <= 1e-12
                restated += 1
            paired = [pg for pg in gt[kind] if pg in pred[kind]]
            ious[kind] = {}
            for pg in paired:
                m = [[float(fn["calc_iou_individual"](p, t)) for t in gt[kind][pg]] for p in pred[kind][pg]["bboxes"]]
                assert m == [[ref.iou(p, t) for t in gt[kind][pg]] for p in pred[kind][pg]["bboxes"]]          # every pair's bits
                assert m == ref.iou_matrix(pred[kind][pg]["bboxes"], gt[kind][pg]).tolist()
                pairs += sum(len(row) for row in m)
                ious[kind][pg] = m
            if keep:
                seen["lag"] += any(len(set(pred[kind][pg]["scores"])) >= 3 for pg in paired)
                seen["unpaired_gt"] += any(pg not in pred[kind] for pg in gt[kind]) and bool(pred[kind])
                seen["unpaired_pred"] += any(pg not in gt[kind] for pg in pred[kind])
                sets = [set(pred[kind][pg]["scores"]) for pg in paired]
                seen["equal_across_pages"] += any(sets[a] & sets[b] for a in range(len(sets)) for b in range(a + 1, len(sets)))
        if keep:
            seen["empty_kind"] += not pred[empty_kind] and bool(gt[empty_kind])
        cases.append({"gt": gt, "pred": pred, "ref": want, "iou": ious})
        if len(cases) == CHECKED:
            break
    assert len(cases) >= CHECKED, len(cases)
    assert all(v >= 5 for v in seen.values()), seen
    out = os.path.join(ROOT, "tests", "golden", "boxeval_float_cases.json")
    with open(out, "w") as f:
        json.dump({"iou_thrs": [float(t) for t in IOU_THRS], "kinds": list(KINDS), "cases": cases[:KEPT]}, f, separators=(",", ":"))
    again = json.load(open(out))
    assert again["cases"] == json.loads(json.dumps(cases[:KEPT]))          # floats round-trip exactly
    print(f"{out}: {KEPT} of {len(cases)} documents ({dropped} dropped for shared ties), {os.path.getsize(out)} bytes, "
          f"{restated} curves restated exactly, {pairs} IoUs equal in every bit, coverage of the kept {seen}")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        from oracle.make_aux_golden import REF                          # where the other golden tools read the reference
        main(REF)
