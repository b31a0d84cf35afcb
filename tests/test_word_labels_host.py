"""Host side of PrebuiltPages.from_boxes(page_annotations=...): the validation runs before any device requirement, so all of it
is checked here without a GPU; the page_labels path keeps its signature and still refuses a CPU device."""
import inspect

import numpy as np
import pytest

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.components.graphs import loader
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages

BOXES = [[[10, 10, 30, 20], [40, 10, 60, 20]], [[5, 5, 9, 9]]]
SIZES = [(100, 100), (100, 100)]
TEXTS = [["a", "b"], ["c"]]
GOOD = [[[0, 0, 35, 25, 1], [38, 8, 62, 22, 5]], []]


def build(ann, **kw):
    return PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, None, "cpu", page_annotations=ann, **kw)


def test_both_label_sources_or_neither():
    with pytest.raises(ValueError, match="exactly one of page_labels and page_annotations.*both"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, [[1, 1], [1]], "cpu", page_annotations=GOOD)
    with pytest.raises(ValueError, match="exactly one of page_labels and page_annotations.*neither"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, None, "cpu")


@pytest.mark.parametrize("row", [[0, 0, 10, 10], [0, 0, 10, 10, 1, 1], [0, 0, "10", 10, 1], [0, 0, None, 10, 1], 7,
                                 [0, 0, 10, True, 1]])
def test_a_row_that_is_not_five_numbers_names_its_page(row):
    with pytest.raises(ValueError, match=r"page 1: .*not five numbers"):
        build([GOOD[0], [[1, 1, 8, 8, 2], row]])


@pytest.mark.parametrize("cat", [-1, 13, 2.5, float("nan"), float("inf"), 1e9])
def test_a_category_that_is_no_integer_in_0_12_names_its_page(cat):
    with pytest.raises(ValueError, match=r"page 0: .*category is not an integer in 0 \.\. 12"):
        build([[[0, 0, 35, 25, cat]], []])


def test_integral_float_categories_pass_the_validation():
    box, cat, off = PrebuiltPages.check_annotations([[[0.5, 0, 35, 25, 1.0], [1, 2, 3, 4, 12]], [np.array([0, 0, 9, 9, 5.0])]], 2)
    assert cat.tolist() == [1, 12, 5] and cat.dtype == np.int32
    assert off.tolist() == [0, 2, 3]
    assert box.dtype == np.float64 and box.tolist() == [[0.5, 0, 35, 25], [1, 2, 3, 4], [0, 0, 9, 9]]
    box, cat, off = PrebuiltPages.check_annotations([[], []], 2)
    assert box.shape == (0, 4) and cat.shape == (0,) and off.tolist() == [0, 0, 0]


@pytest.mark.parametrize("row", [[0.5, 0, 10, 10, 5], [0, 0, 10, float("nan"), 5], [0, 0, 2 ** 30 + 1, 10, 5],
                                 [-2 ** 30 - 1, 0, 10, 10, 5], [0, float("inf"), 10, 10, 5]])
def test_a_figure_that_cannot_be_a_node_names_its_page(row):
    with pytest.raises(ValueError, match=r"page 1: FIGURE annotation .*whole numbers within \+-2\^30"):
        build([GOOD[0], [row]])


def test_other_categories_may_have_any_rectangle():
    PrebuiltPages.check_annotations([[[0.5, float("nan"), 2 ** 40, -3.25, 1], [-2 ** 30, -2 ** 30, 2 ** 30, 2 ** 30, 5]]], 1)


def test_page_count_must_match():
    with pytest.raises(ValueError, match="page_annotations names 1 pages, page_boxes 2"):
        build([GOOD[0]])


def test_per_word_extra_feats_cannot_line_up():
    extra = [np.zeros((2, 3), dtype=np.float32), np.zeros((1, 3), dtype=np.float32)]
    with pytest.raises(ValueError, match="callable.*cannot line up"):
        build(GOOD, extra_feats=extra)


def test_valid_annotations_reach_the_device_requirement():
    """Nothing is computed on the host in place of the kernels: a CPU device is refused only after the validation passed."""
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        build(GOOD)
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        build(GOOD, extra_feats=lambda texts, boxes: [np.zeros((len(t), 1)) for t in texts], converted=False)


def test_page_labels_path_keeps_its_signature():
    sig = inspect.signature(PrebuiltPages.from_boxes)
    names = list(sig.parameters)
    assert names[:11] == ["page_boxes", "page_sizes", "page_texts", "page_labels", "device", "k", "max_dist", "bidirectional",
                          "range_island", "extra_feats", "mode"]
    assert names[11:] == ["page_annotations", "converted", "kw"]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert all(d[n] is inspect.Parameter.empty for n in names[:5])
    assert (d["k"], d["max_dist"], d["bidirectional"], d["range_island"], d["extra_feats"], d["mode"]) == (5, 500, True, 0, None, "knn")
    assert d["page_annotations"] is None and d["converted"] is True
    with pytest.raises(_lib.GteError, match="no CPU fallback"):                  # as before: the graph stage needs the device
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, [[1, 1], [1]], "cpu")


def test_label_words_needs_the_device_and_the_abi_declares_the_calls():
    import torch
    from gnn_tableextraction_amd import graph as G
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        G.label_words(torch.zeros((1, 4), dtype=torch.int32), [0, 1], np.zeros((0, 4)), np.zeros(0, dtype=np.int32), [0, 0])
    for name in ("gte_word_labels_chunk", "gte_word_labels", "gte_word_labels_compact"):
        assert name in _lib.SIGNATURES
    assert loader.SKIPPED == (4, 9, 11, 12) and loader.FIGURE == 5
    assert [c for c, v in loader.ORIGIN_TO_CONV.items() if v is None] == list(loader.SKIPPED)
