"""PrebuiltPages.from_boxes(..., repr_embedder=Repr(...)) end to end on the device, on both routes (ready labels, page
annotations): [BBOX 13 | REPR 50 | extra] columns, the BBOX columns bit-equal to the run without the embedder, the REPR columns
equal to tests/repr_ref.py on the node texts, also after island removal and with figure nodes; and ``Repr.__call__`` against the
reference's recorded tensors (tests/golden/repr_cases.json)."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.components.nlp.repr import Repr
from tests import repr_ref as ref
from tests import wordlabels_ref as wl
from tests.test_gpu_from_annotations import SIZE, make_page, reference_node_lists

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DATA = ref.golden()
CASE = [s for s in DATA["sets"] if s["name"] == "normal_c47_d3_p50"][0]
WORDS = ["banana33", "p-value", "33", "1.1", "(1.1,", "Table", "2:", "end.", "45%", "3-5", "-5", "results", "New York", "?", "7"]


@pytest.fixture(scope="module")
def embedder():
    return Repr(CASE["repr2idx"], CASE["embeddings"], CASE["prototypes"], CASE["i_embedding"], device=DEV)


@pytest.fixture(scope="module")
def pages():
    """Three synthetic pages: word boxes, texts over the fixture's vocabulary, annotations (two of the pages with figures)."""
    rng = np.random.default_rng(77)
    made = [make_page(rng), make_page(rng, with_figure=False), make_page(rng)]
    texts = [[WORDS[int(i)] for i in rng.integers(0, len(WORDS), size=len(m[0]))] for m in made]
    return [m[0] for m in made], texts, [m[2] for m in made]


def expected(embedder, tok):
    want, bound = ref.features(tok, CASE["embeddings"], CASE["prototypes"], CASE["i_embedding"])
    assert not bound.any()
    return want.astype(np.float32)


@pytest.mark.parametrize("range_island", [0, 2])
def test_annotations_route(pages, embedder, range_island):
    boxes, texts, anns = pages
    kw = dict(page_annotations=anns, range_island=range_island)
    got = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, None, DEV, repr_embedder=embedder, **kw)
    plain = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, None, DEV, **kw)
    feat, base = got.whole.ndata['feat'], plain.whole.ndata['feat']
    n = sum(got.whole.batch_num_nodes_)
    assert tuple(feat.shape) == (n, 63) and tuple(base.shape) == (n, 13)
    assert torch.equal(feat[:, :13], base)                               # bit-equal BBOX columns
    final = [p['texts'] for p in got.pages]
    assert final == [p['texts'] for p in plain.pages]
    if not range_island:
        assert sum("IMAGE!" in t for t in final) == 2                    # figure nodes among them
    else:
        assert n < sum(len(n_[0]) for n_ in reference_node_lists(boxes, texts, anns, wl.CAT_MAP))     # island removal removed something
    tok = embedder.token_ids(final)                                      # no empty word: a node's token is its own text's
    assert (tok >= 0).all()
    np.testing.assert_array_equal(feat[:, 13:].cpu().numpy(), expected(embedder, tok))
    o = 0
    for g, b in zip(got.graphs, plain.graphs):                           # the per-page host copies carry the same rows
        k = g.ndata['feat'].shape[0]
        assert torch.equal(g.ndata['feat'], feat[o:o + k].cpu()) and torch.equal(g.ndata['feat'][:, :13], b.ndata['feat'])
        o += k
    for a, b in zip(got.whole.edges(), plain.whole.edges()):
        assert torch.equal(a, b)
    assert torch.equal(got.whole.ndata['label'], plain.whole.ndata['label'])


@pytest.mark.parametrize("range_island", [0, 2])
def test_labels_route_tokens_are_aligned_before_island_removal(pages, embedder, range_island):
    boxes, texts, anns = pages
    nodes = reference_node_lists(boxes, texts, anns, wl.CAT_MAP)
    nb, nl = [n[0] for n in nodes], [n[1] for n in nodes]
    nt = [list(n[2]) for n in nodes]
    nt[0][5], nt[2][9], nt[2][-1] = "", "", "a\tb"                       # empty words shift the tokens of their page; a surplus token
    index = [np.arange(len(b), dtype=np.float32).reshape(-1, 1) for b in nb]
    kw = dict(range_island=range_island, extra_feats=index)
    got = PrebuiltPages.from_boxes(nb, [SIZE] * 3, nt, nl, DEV, repr_embedder=embedder, **kw)
    plain = PrebuiltPages.from_boxes(nb, [SIZE] * 3, nt, nl, DEV, **kw)
    feat, base = got.whole.ndata['feat'], plain.whole.ndata['feat']
    assert tuple(feat.shape) == (base.shape[0], 13 + 50 + 1)
    assert torch.equal(feat[:, :13], base[:, :13]) and torch.equal(feat[:, 63], base[:, 13])      # [BBOX | REPR | extra]
    off = np.concatenate([[0], np.cumsum([len(b) for b in nb])])
    sizes = got.whole.batch_num_nodes_
    page_of = np.repeat(np.arange(3), sizes)
    kept = off[page_of] + feat[:, 63].cpu().numpy().astype(np.int64)     # the nodes that island removal kept, in the given lists
    if range_island:
        assert len(kept) < off[-1]
    tok = embedder.token_ids(nt)                                         # on the lists as given
    assert tok[off[1] - 1] == -1 and tok[off[3] - 1] >= 0 and (tok[off[2]:off[3]] >= 0).all()
    np.testing.assert_array_equal(feat[:, 13:63].cpu().numpy(), expected(embedder, tok)[kept])
    assert PrebuiltPages.from_boxes(nb, [SIZE] * 3, nt, nl, DEV, repr_embedder=None, **kw).whole.ndata['feat'].equal(base)


@pytest.mark.parametrize("case", DATA["sets"], ids=[s["name"] for s in DATA["sets"]])
def test_call_returns_the_rows_of_the_recorded_reference_tensor(case):
    emb = Repr(case["repr2idx"], case["embeddings"], case["prototypes"], case["i_embedding"], device=DEV)
    pages = case["pages"]
    tok = emb.token_ids(pages)
    for mode, combined in (("hard", False), ("combined", True)):
        got = emb(None, pages, None, combined=combined)
        assert emb._online_batch_(None, pages, None)[0].equal(emb(None, pages, None)[0])
        assert [tuple(t.shape) for t in got] == [(len(p), emb.n_out) for p in pages] and all(t.is_cuda for t in got)
        want, bound = ref.features(tok, case["embeddings"], case["prototypes"], case["i_embedding"], 1.0, combined)
        o = 0
        for rows, t, p in zip(case[mode], got, pages):
            mine = t.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(mine - want[o:o + len(p)]) <= bound[o:o + len(p)])
            # hard mode: bound is 0, the rows are EQUAL.  Combined: the recorded rows are within `bound` of the exact sum
            # (tests/test_repr_ref_cpu.py) and so are ours (the line above): the two are 2 * bound apart at the most
            assert np.all(np.abs(mine[:len(rows)] - rows.astype(np.float64)) <= 2 * bound[o:o + len(rows)])
            assert not mine[len(rows):].any()                            # beyond the reference's tensor: nodes without a token
            o += len(p)
