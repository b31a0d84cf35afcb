"""PrebuiltPages.from_boxes(page_annotations=...) end to end on the device: it must equal from_boxes(page_labels=...) fed with the
node list that tests/wordlabels_ref.py (the restatement of the reference's get_nodes) makes of the same pages -- edges, edge
weights, features, labels, stats and the pages' boxes and texts, all compared exactly."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from tests import wordlabels_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OTHER, TEXT, TITLE, LIST, TABLE, FIGURE, CAPTION, COLH, SP, GCELL, TCELL, COL, ROW = range(13)
SIZE = (1000, 1400)


def make_page(rng, with_figure=True):
    """-> (word boxes [n, 4], texts [n], annotation rows): a title, two paragraphs, a table (the enclosing TABLE, its rows and
    columns listed BEFORE the cells), a figure over a few words with a caption, and stray words that no annotation holds."""
    words, ann = [], []

    def line(x, y, n, w=48, gap=8):
        for i in range(n):
            words.append([x + i * (w + gap), y, x + i * (w + gap) + w - int(rng.integers(0, 12)), y + 14])

    line(300, 40, 5)
    ann.append([290, 30, 720, 64, TITLE])
    for top in (100, 330):
        for r in range(int(rng.integers(4, 8))):
            line(60, top + r * 22, int(rng.integers(9, 15)))
        ann.append([50.5, top - 8.5, 950.5, top + 8 * 22 + 0.5, TEXT])
    t0, rows, cols = 560, int(rng.integers(3, 6)), int(rng.integers(3, 6))
    ann.append([55, t0 - 6, 60 + cols * 150, t0 + rows * 30, TABLE])
    ann += [[55, t0 - 6 + r * 30, 60 + cols * 150, t0 + r * 30 + 24, ROW] for r in range(rows)]
    ann += [[55 + c * 150, t0 - 6, 55 + c * 150 + 145, t0 + rows * 30, COL] for c in range(cols)]
    for r in range(rows):
        for c in range(cols):
            line(70 + c * 150, t0 + r * 30, int(rng.integers(1, 3)), w=40, gap=6)
            ann.append([60 + c * 150, t0 + r * 30 - 4, 60 + c * 150 + 140, t0 + r * 30 + 20, COLH if r == 0 else TCELL])
    if with_figure:
        ann.append([100, 800, 600, 1100, FIGURE])
        for r in range(3):
            line(150, 850 + r * 60, 4)                                   # axis labels inside the figure: dropped
        line(100, 1110, 6)
        ann.append([90, 1104, 700, 1130, CAPTION])
        ann.append([700, 800, 900, 1000, FIGURE])                        # a second figure without words
    line(60, 1300, 3)                                                    # page footer: no annotation -> OTHER
    line(800, 1250, 2)
    texts = [f"w{i}" if i % 5 else f"{i}.5" for i in range(len(words))]
    return np.asarray(words, dtype=np.int32), texts, ann


@pytest.fixture(scope="module")
def pages():
    rng = np.random.default_rng(77)
    made = [make_page(rng), make_page(rng, with_figure=False), make_page(rng)]
    return [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]


def reference_node_lists(boxes, texts, anns, cat_map):
    """The reference's node list per page (figures first, then the kept words) from tests/wordlabels_ref.py."""
    out = []
    for b, t, a in zip(boxes, texts, anns):
        a = np.asarray(a, dtype=np.float64).reshape(-1, 5)
        labels, _ = ref.label_page(b, a[:, :4], a[:, 4].astype(np.int32))
        nb, nl, src = ref.nodes_page(b, a[:, :4], a[:, 4].astype(np.int32), labels, cat_map)
        out.append((np.asarray(nb, dtype=np.int32).reshape(-1, 4), nl, ["IMAGE!" if s < 0 else t[s] for s in src]))
    return out


def assert_same_dataset(got, want, want_texts):
    assert got.num_classes == want.num_classes and got.stats == want.stats and len(got) == len(want)
    for a, b in zip(got.whole.edges(), want.whole.edges()):
        assert torch.equal(a, b)
    assert torch.equal(got.whole.edata['feat'], want.whole.edata['feat'])
    for key in ('feat', 'label', 'bbox'):
        assert torch.equal(got.whole.ndata[key], want.whole.ndata[key]), key
    assert got.whole.batch_num_nodes_ == want.whole.batch_num_nodes_
    for g, w, pg, pw, texts in zip(got.graphs, want.graphs, got.pages, want.pages, want_texts):
        for a, b in zip(g.edges(), w.edges()):
            assert torch.equal(a, b)
        assert torch.equal(g.edata['feat'], w.edata['feat'])
        assert torch.equal(g.ndata['feat'], w.ndata['feat']) and torch.equal(g.ndata['label'], w.ndata['label'])
        np.testing.assert_array_equal(pg['bboxs'], pw['bboxs'])
        assert pg['texts'] == texts


@pytest.mark.parametrize("mode,range_island", [("knn", 0), ("knn", 2), ("visibility", 0), ("visibility", 2)])
def test_annotations_equal_labels_of_the_reference_node_list(pages, mode, range_island):
    boxes, texts, anns = pages
    nodes = reference_node_lists(boxes, texts, anns, ref.CAT_MAP)
    assert all(t[:2] == ["IMAGE!", "IMAGE!"] for _, _, t in (nodes[0], nodes[2])) and "IMAGE!" not in nodes[1][2]
    assert sum(len(n[0]) for n in nodes) < sum(len(b) for b in boxes) + 4            # words inside the figures are gone
    kw = dict(k=5, max_dist=500, range_island=range_island, mode=mode)
    got = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, None, DEV, page_annotations=anns, **kw)
    # the labels path says which nodes island removal kept through an extra feature column: the node's index in its page
    index = [np.arange(len(n[0]), dtype=np.float32).reshape(-1, 1) for n in nodes]
    want = PrebuiltPages.from_boxes([n[0] for n in nodes], [SIZE] * 3, [n[2] for n in nodes], [n[1] for n in nodes], DEV,
                                    extra_feats=index, **kw)
    kept = [g.ndata['feat'][:, -1].numpy().astype(np.int64) for g in want.graphs]
    want_texts = [[n[2][i] for i in k] for n, k in zip(nodes, kept)]
    if range_island:
        assert sum(len(k) for k in kept) < sum(len(n[0]) for n in nodes)             # island removal did remove something
    plain = PrebuiltPages.from_boxes([n[0] for n in nodes], [SIZE] * 3, [n[2] for n in nodes], [n[1] for n in nodes], DEV, **kw)
    assert_same_dataset(got, plain, want_texts)
    assert all(p['texts'] is None and 'annotations' not in p for p in plain.pages)    # the labels path is what it was
    assert [p['annotations'] for p in got.pages] == anns
    assert sorted(c for c, n in enumerate(got.stats['numbers']) if n) == sorted({ref.CAT_MAP[c] for c in
                                                                               (OTHER, TEXT, TITLE, FIGURE, CAPTION, COLH, TCELL)})
    gt = PP.blocks_gt_json(got)                                          # the evaluation reads the same object
    assert list(gt) == [PP.CATEGORY_NAMES[c] for c in (TEXT, TITLE, TABLE, FIGURE, CAPTION, COLH, TCELL, COL, ROW)]
    assert sum(len(v) for v in gt[PP.CATEGORY_NAMES[FIGURE]].values()) == 4


def test_the_extra_feats_callable_receives_the_final_node_lists(pages):
    boxes, texts, anns = pages
    seen = {}

    def extra(page_texts, page_boxes):
        seen['texts'], seen['boxes'] = page_texts, page_boxes
        return [np.stack([np.full(len(t), 7.0), np.asarray([len(s) for s in t], dtype=np.float64)], axis=1).reshape(len(t), 2)
                for t in page_texts]

    got = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, None, DEV, page_annotations=anns, range_island=2, extra_feats=extra)
    assert seen['texts'] == [p['texts'] for p in got.pages]
    for b, p, g in zip(seen['boxes'], got.pages, got.graphs):
        np.testing.assert_array_equal(b, p['bboxs'])
        assert g.ndata['feat'].shape[1] == 15
        assert (g.ndata['feat'][:, 13] == 7.0).all()
        assert g.ndata['feat'][:, 14].tolist() == [float(len(s)) for s in p['texts']]
    assert seen['texts'][0][:2] == ["IMAGE!", "IMAGE!"]


def test_converted_false_gives_original_ids(pages):
    boxes, texts, anns = pages
    got = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, None, DEV, page_annotations=anns, converted=False)
    assert got.num_classes == 13 and len(got.stats['numbers']) == 13
    nodes = reference_node_lists(boxes, texts, anns, None)
    for g, n, p in zip(got.graphs, nodes, got.pages):
        assert g.ndata['label'].tolist() == [float(v) for v in n[1]]
        np.testing.assert_array_equal(p['bboxs'], n[0])
        assert p['texts'] == n[2]
    labels = {int(v) for g in got.graphs for v in g.ndata['label'].tolist()}
    assert labels == {OTHER, TEXT, TITLE, FIGURE, CAPTION, COLH, TCELL}
    conv = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, None, DEV, page_annotations=anns)
    for g, c in zip(got.graphs, conv.graphs):
        assert c.ndata['label'].tolist() == [float(ref.CAT_MAP[int(v)]) for v in g.ndata['label'].tolist()]
