"""Golden cases of the area-weighted document evaluation  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the
reference tree).

Runs the REFERENCE's own arithmetic: models/evaluate.py cannot be imported (``audioop``, the missing ``predictions`` package), so
the class loop of ``evaluate_doc`` -- the ``for cls in range(...)`` statement -- is cut out of the file with ``ast`` at run time and
executed on the case's ``gt``, ``preds`` and ``areas``, in a namespace whose ``np`` forwards to numpy and records every ``np.sum``
result: the three areas per class, next to the loop's own ``precision`` / ``recall`` / ``f1`` lists.  None of the reference's text
is held in this repository.  It writes tests/golden/doceval_cases.json: inputs and recorded outputs only, a float that JSON
cannot hold (NaN, +-inf) written as a string.  The tool asserts that tests/doceval_ref.py reproduces every case.

    python tools/make_doceval_golden.py [reference/src]        # writes tests/golden/doceval_cases.json
"""
import ast
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import doceval_ref as ref                                   # noqa: E402


class RecordingNumpy:
    """numpy, with the results of ``sum`` kept in call order."""
    def __init__(self):
        self.sums = []

    def sum(self, *args, **kwargs):
        out = np.sum(*args, **kwargs)
        self.sums.append(out)
        return out

    def __getattr__(self, name):
        return getattr(np, name)


def reference_loop(src_root):
    """-> run(gt, preds, areas): the reference's class loop on numpy arrays; (sums, precision, recall, f1)."""
    path = os.path.join(src_root, "models", "evaluate.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "evaluate_doc"][0]
    loops = [n for n in fn.body if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "cls"]
    assert len(loops) == 1, len(loops)
    code = compile(ast.Module(body=loops, type_ignores=[]), f"{path}:evaluate_doc", "exec")

    def run(gt, preds, areas):
        rec = RecordingNumpy()
        ns = {"np": rec, "gt": gt, "preds": preds, "areas": areas, "precision": [], "recall": [], "f1": [],
              "print": lambda *a, **k: None}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                            # 0 / 0
            exec(code, ns)
        return rec.sums, ns["precision"], ns["recall"], ns["f1"]
    return run


def boxes_for(rng, n, odd=False):
    lo = rng.integers(0, 1500, (n, 2))
    size = rng.integers(1, 200, (n, 2))
    if odd:                                                            # a third each: empty, one axis inverted, as it was
        kind = rng.integers(0, 3, n)
        size[kind == 0, 0] = 0
        size[kind == 1, 1] *= -1
    return np.concatenate([lo, lo + size], axis=1)


def cases():
    rng = np.random.default_rng(20270)
    out = []

    def add(name, gt, pred, bbox=None, odd=False):
        gt, pred = np.asarray(gt, dtype=np.int64), np.asarray(pred, dtype=np.int64)
        out.append((name, gt, pred, boxes_for(rng, gt.size, odd) if bbox is None else np.asarray(bbox, dtype=np.int64)))

    def noisy(n, C, acc):
        gt = rng.integers(0, C, n)
        gt[rng.integers(0, n)] = C - 1                                 # max(gt) + 1 == C
        return gt, np.where(rng.random(n) < acc, gt, rng.integers(0, C, n))

    for C, n, acc in ((1, 40, 0.95), (2, 120, 0.6), (9, 200, 0.8), (13, 200, 0.7)):
        add(f"random_c{C}_acc{int(acc * 100)}", *noisy(n, C, acc))
    gt = rng.integers(0, 5, 90)
    add("all_correct", gt, gt.copy())
    add("all_wrong", gt, (gt + 1 + rng.integers(0, 4, 90)) % 5)
    gt, pred = noisy(150, 6, 0.8)
    pred[pred == 2] = 3
    add("class_absent_from_pred", gt, pred)
    gt, pred = noisy(150, 7, 0.8)
    gt[gt == 4] = 5                                                    # below max(gt) = 6; pred still names 4
    add("class_absent_from_gt", gt, pred)
    gt, pred = noisy(150, 4, 0.75)
    pred[rng.random(150) < 0.2] = 6                                    # max(gt) = 3
    pred[rng.random(150) < 0.1] = 9
    add("predictions_above_max_gt", gt, pred)
    add("zero_and_negative_areas", *noisy(160, 5, 0.7), odd=True)
    # class 1: every node that is predicted 1 wrongly, or labelled 1 and missed, stands AHEAD of the class's true positives
    gt = np.array([0] * 10 + [1] * 10 + [1] * 12 + [0] * 6 + [2] * 5)
    pred = np.array([1] * 10 + [0] * 5 + [2] * 5 + [1] * 12 + [0] * 6 + [2] * 5)
    add("non_tp_ahead_of_tp", gt, pred)
    add("tp_ahead_of_non_tp", gt[::-1].copy(), pred[::-1].copy())
    add("one_node", [0], [0])
    return out


def jfloat(v):
    v = float(v)
    return v if np.isfinite(v) else ("nan" if v != v else ("inf" if v > 0 else "-inf"))


def main(src_root):
    run = reference_loop(src_root)
    data = {"numpy_version": np.__version__, "cases": []}
    for name, gt, pred, bbox in cases():
        areas = np.array([(int(b[2]) - int(b[0])) * (int(b[3]) - int(b[1])) for b in bbox])       # evaluate.py:164
        sums, p, r, f1 = run(gt, pred, areas)
        C = int(gt.max()) + 1
        assert len(sums) == 3 * C and len(p) == len(r) == len(f1) == C, (name, len(sums), C)
        rec = {"name": name, "gt": gt.tolist(), "pred": pred.tolist(), "bbox": bbox.tolist(), "n_classes": C,
               "tp_area": [int(v) for v in sums[0::3]], "fp_area": [int(v) for v in sums[1::3]],
               "fn_area": [int(v) for v in sums[2::3]], "precision": [jfloat(v) for v in p], "recall": [jfloat(v) for v in r],
               "f1": [jfloat(v) for v in f1]}
        got = ref.doc_prf(*ref.area_confusion(gt, pred, bbox, C), mode="reference")
        for key in ("tp_area", "fp_area", "fn_area"):
            assert got[key].tolist() == rec[key], (name, key, got[key].tolist(), rec[key])
        for key, want in (("precision", p), ("recall", r), ("f1", f1)):
            assert np.array_equal(got[key], np.asarray(want, dtype=np.float64), equal_nan=True), (name, key)
        lead = ref.area_confusion(gt, pred, bbox, C)[2]
        rec["lead_total"] = int(np.abs(lead).sum())
        data["cases"].append(rec)
    by_name = {c["name"]: c for c in data["cases"]}
    assert by_name["non_tp_ahead_of_tp"]["lead_total"] > 0 and by_name["tp_ahead_of_non_tp"]["lead_total"] == 0
    assert any("nan" in c["precision"] for c in data["cases"])
    out = os.path.join(ROOT, "tests", "golden", "doceval_cases.json")
    with open(out, "w") as f:
        json.dump(data, f, separators=(",", ":"))
    assert json.load(open(out)) == data                                  # JSON floats round-trip exactly
    print(f"{out}: numpy {np.__version__}, {len(data['cases'])} cases, {sum(len(c['gt']) for c in data['cases'])} nodes, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        from oracle.make_aux_golden import REF                          # where the other golden tools read the reference
        main(REF)
