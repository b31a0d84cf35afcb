"""Host side of the label-free route: the argument checks of PrebuiltPages.from_boxes(unlabeled=True) run before any device call,
and train() / test() refuse pages without labels on their first line -- all of it checked here without a GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.data import synthetic as S
from gnn_tableextraction_amd.models import model_predict, model_train

BOXES = [[[10, 10, 30, 20], [40, 10, 60, 20]], [[5, 5, 9, 9]]]
SIZES = [(100, 100), (100, 100)]
TEXTS = [["a", "b"], ["c"]]


def test_unlabeled_takes_no_labels_and_no_annotations():
    with pytest.raises(ValueError, match="unlabeled=True takes neither page_labels nor page_annotations.*page_labels"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, [[1, 1], [1]], "cpu", unlabeled=True)
    with pytest.raises(ValueError, match="unlabeled=True takes neither page_labels nor page_annotations.*page_annotations"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, None, "cpu", page_annotations=[[[0, 0, 35, 25, 1]], []], unlabeled=True)


@pytest.mark.parametrize("range_island", [1, 2, -1])
def test_unlabeled_has_no_island_removal(range_island):
    with pytest.raises(ValueError, match="unlabeled=True needs range_island 0"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, None, "cpu", range_island=range_island, unlabeled=True)


def test_neither_without_the_flag_is_still_an_error():
    with pytest.raises(ValueError, match="exactly one of page_labels and page_annotations.*neither"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, None, "cpu")
    with pytest.raises(ValueError, match="exactly one of page_labels and page_annotations.*neither"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, None, "cpu", unlabeled=False)


def test_valid_unlabeled_arguments_reach_the_device_requirement():
    """Nothing is computed on the host in place of the kernels: a CPU device is refused only after the checks passed."""
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        PrebuiltPages.from_boxes(BOXES, SIZES, TEXTS, None, "cpu", unlabeled=True)


def test_train_and_test_refuse_pages_without_labels():
    stub = SimpleNamespace(labeled=False)                     # nothing else is read before the refusal
    with pytest.raises(ValueError, match=r"test\(\): .*no labels.*predict\(\)"):
        model_predict.test(stub, None)
    with pytest.raises(ValueError, match=r"train\(\): .*no labels"):
        model_train.train(stub, None)


def test_a_set_without_labels_on_the_host(tmp_path):
    """The dataset object itself needs no device: no 'label', zero counts, save / load round trip; a labelled set is as before."""
    made = S.make_pages(3, in_feats=13)
    pages = [S.Page(p.src, p.dst, p.weight, p.feat, None, p.bbox) for p in made]
    data = PrebuiltPages(pages, num_classes=7, labeled=False)
    assert data.labeled is False and data.num_classes == 7 and len(data) == 3
    assert data.stats == {'numbers': [0] * 7, 'percentages': [0.0] * 7}
    assert all(set(g.ndata) == {'feat'} and 'feat' in g.edata for g in data.graphs)
    assert [p['texts'] for p in data.pages] == [None] * 3
    assert all(np.array_equal(pg['bboxs'], p.bbox) for pg, p in zip(data.pages, made))
    train, val, (ti, vi) = data.split()
    assert len(train) == 2 and len(val) == 1 and sorted(ti + vi) == [0, 1, 2]
    data.save(str(tmp_path / "u.npz"))
    assert 'label' not in np.load(tmp_path / "u.npz").files
    back = PrebuiltPages.load(str(tmp_path / "u.npz"))
    assert back.labeled is False and back.num_classes == 7 and back.stats == data.stats
    for g, h, p in zip(back.graphs, data.graphs, back.page_arrays):
        assert p.label is None and 'label' not in g.ndata
        assert all(np.array_equal(a, b) for a, b in zip(g.edges(), h.edges()))
        assert np.array_equal(g.ndata['feat'], h.ndata['feat']) and np.array_equal(g.edata['feat'], h.edata['feat'])

    labelled = PrebuiltPages(made)
    assert labelled.labeled is True and 'label' in labelled.graphs[0].ndata and sum(labelled.stats['numbers']) == sum(p.num_nodes for p in made)
    labelled.save(str(tmp_path / "l.npz"))
    back = PrebuiltPages.load(str(tmp_path / "l.npz"))
    assert back.labeled is True and back.stats == labelled.stats and 'label' in np.load(tmp_path / "l.npz").files
