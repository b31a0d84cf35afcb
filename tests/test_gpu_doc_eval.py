"""gte_doc_eval (csrc/doc_eval.hip) against tests/doceval_ref.py: integers, compared exactly, on outputs and a workspace that are
prefilled with a sentinel; then ``metrics.area_confusion`` / ``evaluate_doc`` on the reference's recorded cases."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.utils import metrics
from tests import doceval_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A5A5A5A5B
INVALID, TOO_SMALL, UNSUPPORTED = -1, -3, -4


def chunk_nodes():
    return _lib.load().gte_doc_eval_chunk_nodes()


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def call(gt, pred, bbox, C, ws_bytes=None, null=(), box_shift=0):
    """One gte_doc_eval call on sentinel-filled outputs and workspace -> (rc, area, count, lead) as the call left them.
    ``null``: argument names handed over as NULL; ``box_shift``: int32 elements by which the box pointer is moved."""
    lib = _lib.load()
    n = len(gt)
    side = max(C, 0) + 1
    out = {"area": torch.full((side * side,), SENTINEL, dtype=torch.int64, device=DEV),
           "count": torch.full((side * side,), SENTINEL, dtype=torch.int64, device=DEV),
           "lead": torch.full((2 * max(C, 1),), SENTINEL, dtype=torch.int64, device=DEV)}
    need = int(lib.gte_doc_eval_workspace_bytes(n, C))
    ws = torch.full((max(need, 4096) // 8 + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    d_box = dev(np.concatenate([np.asarray(bbox, dtype=np.int32).reshape(-1), np.zeros(4, dtype=np.int32)]))
    args = {"gt": dev(gt), "pred": dev(pred), "ws": ws, **out}
    ptr = {k: (0 if k in null else v.data_ptr()) for k, v in args.items()}
    ptr["bbox"] = 0 if "bbox" in null else d_box.data_ptr() + 4 * box_shift
    rc = lib.gte_doc_eval(ptr["gt"], ptr["pred"], ptr["bbox"], n, C, ptr["area"], ptr["count"], ptr["lead"], ptr["ws"],
                          need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out["area"].cpu().numpy(), out["count"].cpu().numpy(), out["lead"].cpu().numpy()


def check(gt, pred, bbox, C):
    """The call equals the oracle, entry by entry; -> the oracle's (area, count, lead)."""
    rc, area, count, lead = call(gt, pred, bbox, C)
    assert rc == 0, _lib.load().gte_last_error()
    want = ref.area_confusion(gt, pred, bbox, C)
    np.testing.assert_array_equal(area.reshape(C + 1, C + 1), want[0])
    np.testing.assert_array_equal(count.reshape(C + 1, C + 1), want[1])
    np.testing.assert_array_equal(lead[:2 * C].reshape(2, C), want[2])
    return want


def test_limits():
    lib = _lib.load()
    assert lib.gte_doc_eval_max_classes() == 16 and chunk_nodes() >= 256 and chunk_nodes() % 64 == 0
    assert lib.gte_doc_eval_workspace_bytes(0, 1) > 0
    assert lib.gte_doc_eval_workspace_bytes(10 * chunk_nodes(), 9) > lib.gte_doc_eval_workspace_bytes(chunk_nodes(), 9)
    assert lib.gte_doc_eval_workspace_bytes(478_000, 9) < 1 << 20


SIZES = ["0", "1", "63", "64", "65", "chunk-1", "chunk", "chunk+1", "3*chunk+7"]


@pytest.mark.parametrize("C", [1, 9, 16])
@pytest.mark.parametrize("size", SIZES)
def test_equals_the_oracle_on_random_labels(size, C):
    """labels -1, C and C + 5 on both sides, inverted and empty boxes (tests/doceval_ref.py: random_case)"""
    n = eval(size, {"chunk": chunk_nodes()})
    rng = np.random.default_rng(1000 * C + n)
    gt, pred, bbox = ref.random_case(rng, n, C, accuracy=0.8, outside=0.1, odd_boxes=0.15)
    area, count, lead = check(gt, pred, bbox, C)
    assert int(count.sum()) == n
    if n >= 63:
        assert count[C].sum() > 0 and count[:, C].sum() > 0 and (ref.areas(bbox) <= 0).sum() > 2
    if n >= chunk_nodes() - 1 and C > 1:
        assert lead.all()                                                        # every class loses something on both sides


@pytest.mark.parametrize("t", ["1", "64", "65", "chunk//4", "chunk//4+1", "chunk", "chunk+1", "2*chunk"])
def test_the_boundary_position_between_sub_tiles_waves_and_chunks(t):
    """Every node is predicted 0, so a node's position within P_0 is its index, and exactly t of them are labelled 0: the
    positions t - 1 and t -- the last that the reference loses and the first that it keeps -- are the nodes t - 1 and t.  They
    fall into different 64-node tiles, different waves of one chunk (a wave takes a quarter of a chunk) or different chunks.
    The labelled side mirrors it with the roles exchanged."""
    chunk = chunk_nodes()
    t = eval(t, {"chunk": chunk})
    n = 2 * chunk + 70
    rng = np.random.default_rng(t)
    label = np.ones(n, dtype=np.int32)
    label[rng.choice(n, t, replace=False)] = 0
    label[[t - 1, t]] = 1                                                        # both sides of the boundary are wrong nodes ...
    spare = np.flatnonzero(label == 1)
    spare = spare[(spare != t - 1) & (spare != t)]
    label[rng.choice(spare, t - int((label == 0).sum()), replace=False)] = 0     # ... and there are still exactly t right ones
    assert int((label == 0).sum()) == t
    zeros = np.zeros(n, dtype=np.int32)
    bbox = ref.random_case(rng, n, 2, odd_boxes=0.0)[2]
    a = ref.areas(bbox)
    for gt, pred, side in ((label, zeros, 0), (zeros, label, 1)):
        area, count, lead = check(gt, pred, bbox, 2)
        assert count[0, 0] == t
        assert lead[side, 0] == a[:t][label[:t] == 1].sum() and lead[side, 0] >= a[t - 1] > 0
        assert lead[1 - side, 0] == 0


def test_a_class_whose_boundary_lies_in_a_later_chunk_than_anothers():
    """three classes with t_c in chunks 0, 1 and 2 of their lists: the chunks' early exit must hold for all classes at once"""
    chunk = chunk_nodes()
    n = 3 * chunk + 7
    rng = np.random.default_rng(8)
    pred = (np.arange(n) % 3).astype(np.int32)
    gt = pred.copy()
    for c, keep in ((0, 40), (1, chunk // 3 + 100), (2, 2 * chunk // 3 + 100)):      # t_c true positives, scattered
        members = np.flatnonzero(pred == c)
        wrong = rng.permutation(members)[keep:]
        gt[wrong] = rng.choice([(c + 1) % 3, 3, -1], wrong.size)
    bbox = ref.random_case(rng, n, 3)[2]
    area, count, lead = check(gt, pred, bbox, 3)
    assert np.diagonal(count)[:3].tolist() == [40, chunk // 3 + 100, 2 * chunk // 3 + 100] and lead[0].all()


def test_every_node_in_one_cell():
    n = 3 * chunk_nodes() + 7
    rng = np.random.default_rng(9)
    bbox = ref.random_case(rng, n, 2)[2]
    for label, C in ((2, 9), (-1, 9), (0, 1)):
        area, count, lead = check(np.full(n, label, dtype=np.int32), np.full(n, label, dtype=np.int32), bbox, C)
        cell = C if label < 0 else label
        assert count[cell, cell] == n and count.sum() == n and area[cell, cell] == ref.areas(bbox).sum() and not lead.any()
    # one off-diagonal cell: every node of P_0 and of G_1 is wrong, t = 0, nothing is lost
    area, count, lead = check(np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32), bbox, 2)
    assert count[1, 0] == n and not lead.any()


def test_areas_are_64_bit_products():
    big = 1 << 30
    bbox = np.asarray([[-big, -big, 0, 0], [5, 5, 5 + big, 5 + big], [0, 0, big, -big], [3, 4, 3, 900], [7, 7, -big, big - 1]],
                      dtype=np.int64)
    gt, pred = np.asarray([0, 0, 1, 1, 0], dtype=np.int32), np.asarray([0, 1, 1, 0, 0], dtype=np.int32)
    area, count, lead = check(gt, pred, bbox, 2)
    assert area[0, 0] == big * big + (-big - 7) * (big - 8) and area[0, 1] == big * big and area[1, 1] == -big * big and area[1, 0] == 0


def test_refused_calls_launch_nothing_and_write_nothing():
    lib = _lib.load()
    rng = np.random.default_rng(10)
    gt, pred, bbox = ref.random_case(rng, 300, 9)

    def untouched(result, code):
        rc, area, count, lead = result
        assert rc == code, (rc, lib.gte_last_error())
        assert (area == SENTINEL).all() and (count == SENTINEL).all() and (lead == SENTINEL).all()
    untouched(call(gt, pred, bbox, 17, ws_bytes=1 << 16), UNSUPPORTED)
    assert b"exceed" in lib.gte_last_error()
    need = lib.gte_doc_eval_workspace_bytes(300, 9)
    untouched(call(gt, pred, bbox, 9, ws_bytes=need - 1), TOO_SMALL)
    untouched(call(gt, pred, bbox, 9, ws_bytes=0), TOO_SMALL)
    for name in ("gt", "pred", "bbox", "area", "count", "lead", "ws"):
        untouched(call(gt, pred, bbox, 9, null=(name,)), INVALID)
    untouched(call(gt, pred, bbox, 9, box_shift=1), INVALID)                     # a box row must be one 16-byte load
    untouched(call(gt, pred, bbox, 0), INVALID)
    assert lib.gte_doc_eval(0, 0, 0, -1, 9, 0, 0, 0, 0, 0, 0) == INVALID
    assert lib.gte_doc_eval_workspace_bytes(-1, 9) < 0 and lib.gte_doc_eval_workspace_bytes(10, 17) < 0
    # no node: the inputs may be NULL, and every output entry is a zero
    rc, area, count, lead = call(gt[:0], pred[:0], bbox[:0], 9, null=("gt", "pred", "bbox"))
    assert rc == 0 and not area.any() and not count.any() and not lead[:18].any()


def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(11)
    gt, pred, bbox = ref.random_case(rng, 5 * chunk_nodes() + 123, 9, accuracy=0.7, outside=0.1)
    first, second = call(gt, pred, bbox, 9), call(gt, pred, bbox, 9)
    assert first[0] == 0 and second[0] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], second[1:]))
    assert np.array_equal(first[3][:18].reshape(2, 9), ref.area_confusion(gt, pred, bbox, 9)[2]) and first[3][:18].all()


def test_area_confusion_wrapper_takes_arrays_and_tensors():
    rng = np.random.default_rng(12)
    gt, pred, bbox = ref.random_case(rng, chunk_nodes() + 300, 5)
    want = ref.area_confusion(gt, pred, bbox, 5)
    for got in (metrics.area_confusion(gt, pred, bbox, 5),
                metrics.area_confusion(torch.from_numpy(gt).to(DEV), torch.from_numpy(pred), bbox.astype(np.int64), 5, device=DEV)):
        assert all(isinstance(a, np.ndarray) and a.dtype == np.int64 for a in got)
        assert [a.shape for a in got] == [(6, 6), (6, 6), (2, 5)]
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(_lib.GteError, match="exceed"):
        metrics.area_confusion(gt, pred, bbox, 17)
    with pytest.raises(ValueError, match="predictions"):
        metrics.area_confusion(gt, pred[:-1], bbox, 5)


@pytest.mark.parametrize("case", ref.golden_cases(), ids=lambda c: c["name"])
def test_evaluate_doc_gives_the_references_numbers(case):
    out = metrics.evaluate_doc(case["gt"], case["pred"], case["bbox"], device=DEV)
    assert sorted(out) == ["area", "count", "docbank", "lead", "n_classes", "reference"] and out["n_classes"] == case["n_classes"]
    ref.assert_equals_golden(out["reference"], case)
    want = ref.area_confusion(case["gt"], case["pred"], case["bbox"], case["n_classes"])
    assert all(np.array_equal(out[k], w) for k, w in zip(("area", "count", "lead"), want))
    tp, fp, fn = ref.docbank_sets(case["gt"], case["pred"], case["bbox"], case["n_classes"])
    bank = out["docbank"]
    assert (bank["tp_area"].tolist(), bank["fp_area"].tolist(), bank["fn_area"].tolist()) == (tp, fp, fn)
