"""CPU-only: the host stages of ``metrics.evaluate_doc`` -- ``doc_cells`` and ``doc_prf`` -- with tests/doceval_ref.py in place of
the C call; no device is touched."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd.utils import metrics
from tests import doceval_ref as ref


def pages(rng, sizes, C=5):
    parts = [ref.random_case(rng, n, C) for n in sizes]
    return [p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]


def test_doc_cells_concatenates_pages_and_takes_flat_arrays():
    rng = np.random.default_rng(1)
    gt, pred, box = pages(rng, [30, 0, 17, 1])
    cells = metrics.doc_cells(gt, pred, box)
    assert isinstance(cells, metrics.DocCells)
    assert cells.gt.dtype == cells.pred.dtype == cells.bbox.dtype == np.int32 and cells.bbox.shape == (48, 4)
    assert cells.bbox.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(cells.gt, np.concatenate(gt))
    np.testing.assert_array_equal(cells.pred, np.concatenate(pred))
    np.testing.assert_array_equal(cells.bbox, np.concatenate(box))
    assert cells.n_classes == int(np.concatenate(gt).max()) + 1
    flat = metrics.doc_cells(np.concatenate(gt), np.concatenate(pred).tolist(), np.concatenate(box).astype(np.float64), n_classes=3)
    assert flat.n_classes == 3 and all(np.array_equal(a, b) for a, b in zip(flat[:3], cells[:3]))
    # lists of python lists, tuples and tensors per page; integral floats are integers
    mixed = metrics.doc_cells([g.tolist() for g in gt], tuple(torch.from_numpy(p) for p in pred), [b.astype(np.float32).tolist() for b in box])
    assert all(np.array_equal(a, b) for a, b in zip(mixed[:3], cells[:3])) and mixed.n_classes == cells.n_classes
    one = metrics.doc_cells([4], [2], [[0, 0, 3, 2]])
    assert one.n_classes == 5 and one.bbox.shape == (1, 4)


def test_doc_cells_refuses_what_it_cannot_evaluate():
    rng = np.random.default_rng(2)
    gt, pred, box = pages(rng, [12, 9])
    with pytest.raises(ValueError, match="pages"):
        metrics.doc_cells(gt, pred[:1], box)                                     # a page count mismatch
    with pytest.raises(ValueError, match="pages"):
        metrics.doc_cells(gt, pred, np.concatenate(box))                         # pages of labels, flat boxes
    with pytest.raises(ValueError, match="page 1 has 9 labels, 8 predictions"):
        metrics.doc_cells(gt, [pred[0], pred[1][:-1]], box)
    with pytest.raises(ValueError, match="page 0 has 12 labels, 12 predictions, 11 boxes"):
        metrics.doc_cells(gt, pred, [box[0][:-1], box[1]])
    with pytest.raises(ValueError, match="21 labels, 20 predictions"):
        metrics.doc_cells(np.concatenate(gt), np.concatenate(pred)[:-1], np.concatenate(box))
    with pytest.raises(ValueError, match="rows of 4"):
        metrics.doc_cells(np.concatenate(gt), np.concatenate(pred), np.concatenate(box).reshape(-1)[:-2])
    half = np.concatenate(box).astype(np.float64)
    half[3, 2] += 0.5
    with pytest.raises(ValueError, match="boxes are not integral"):
        metrics.doc_cells(np.concatenate(gt), np.concatenate(pred), half)
    half[3, 2] = np.nan
    with pytest.raises(ValueError, match="boxes are not integral"):
        metrics.doc_cells(np.concatenate(gt), np.concatenate(pred), half)
    with pytest.raises(ValueError, match="predictions are not integral"):
        metrics.doc_cells(np.concatenate(gt), np.concatenate(pred) + 0.25, np.concatenate(box))
    with pytest.raises(ValueError, match="labels do not fit 32 bits"):
        metrics.doc_cells(np.concatenate(gt).astype(np.int64) + (1 << 31), np.concatenate(pred), np.concatenate(box))
    with pytest.raises(ValueError, match="n_classes"):
        metrics.doc_cells(np.concatenate(gt), np.concatenate(pred), np.concatenate(box), n_classes=0)
    with pytest.raises(ValueError, match="n_classes"):
        metrics.doc_cells(np.full(21, -1), np.concatenate(pred), np.concatenate(box))          # max(gt) + 1 == 0
    with pytest.raises(ValueError, match="no node"):
        metrics.doc_cells(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 4), dtype=np.int64))
    empty = metrics.doc_cells(np.zeros(0, dtype=np.int64), [], np.zeros((0, 4)), n_classes=2)
    assert empty.gt.shape == (0,) and empty.bbox.shape == (0, 4) and empty.n_classes == 2


def test_the_overflow_guard_is_max_area_times_n_below_2_to_the_62():
    def run(width, height, n):
        box = np.tile(np.asarray([[0, 0, 1, 1]], dtype=np.int64), (n, 1))
        box[n // 2] = [-5, -7, width - 5, height - 7]
        return metrics.doc_cells(np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), box)
    run(1 << 30, 1 << 30, 3)                                                     # 2^60 * 3 < 2^62
    with pytest.raises(ValueError, match="2\\^62"):
        run(1 << 30, 1 << 30, 4)                                                 # 2^60 * 4
    with pytest.raises(ValueError, match="2\\^62"):
        run(1 << 30, -(1 << 30), 4)                                              # the magnitude counts
    run((1 << 31) - 1, (1 << 31) - 1, 1)                                         # (2^31 - 1)^2 < 2^62
    with pytest.raises(ValueError, match="2\\^62"):
        run((1 << 31) - 1, (1 << 31) - 1, 2)
    wide = np.asarray([[-(1 << 31), -(1 << 31), (1 << 31) - 1, (1 << 31) - 1]], dtype=np.int64)  # 2^64 - ...: past int64 itself
    with pytest.raises(ValueError, match="2\\^62"):
        metrics.doc_cells([0], [0], wide)
    run(1000, 1000, 478_000)                                                     # a validation set's worth of large words


@pytest.mark.parametrize("case", ref.golden_cases(), ids=lambda c: c["name"])
def test_doc_prf_gives_the_references_numbers_on_the_golden_cases(case):
    cells = metrics.doc_cells(case["gt"], case["pred"], case["bbox"])
    assert cells.n_classes == case["n_classes"]
    sums = ref.area_confusion(cells.gt, cells.pred, cells.bbox, cells.n_classes)             # in place of the C call
    got = metrics.doc_prf(*sums)                                                             # 'reference' is the default
    assert sorted(got) == ["f1", "fn_area", "fp_area", "precision", "recall", "tp_area"]
    ref.assert_equals_golden(got, case)
    bank = metrics.doc_prf(*sums, mode="docbank")
    tp, fp, fn = ref.docbank_sets(case["gt"], case["pred"], case["bbox"], case["n_classes"])
    assert (bank["tp_area"].tolist(), bank["fp_area"].tolist(), bank["fn_area"].tolist()) == (tp, fp, fn)
    assert bank["fp_area"].dtype == np.int64 and bank["f1"].dtype == np.float64


def test_doc_prf_checks_shapes_and_mode():
    area, count, lead = ref.area_confusion(*ref.random_case(np.random.default_rng(3), 50, 4), 4)
    with pytest.raises(ValueError, match="mode"):
        metrics.doc_prf(area, count, lead, mode="textbook")
    with pytest.raises(ValueError, match="lead"):
        metrics.doc_prf(area, count, lead[:, :3])
    with pytest.raises(ValueError, match="count"):
        metrics.doc_prf(area, count[:4], lead)
    nan = metrics.doc_prf(np.zeros((3, 3), dtype=np.int64), np.zeros((3, 3), dtype=np.int64), np.zeros((2, 2), dtype=np.int64))
    assert all(np.isnan(nan[k]).all() for k in ("precision", "recall", "f1"))                # 0 / 0, and no warning turned error
