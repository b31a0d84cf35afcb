"""PrebuiltPages.from_boxes(..., repr_embedder=Repr(...), scibert_embedder=SciBERT(...)) end to end on the device, on both routes
(ready labels in both graph modes, page annotations with figures): [BBOX 13 | REPR 50 | SCIBERT 12 | extra] columns, everything but
the SCIBERT columns identical to the run without the embedder, the SCIBERT columns equal to tests/scibert_ref.py on the ids of the
node lists (those from before island removal: the longest word of a page decides which words pool their ``[SEP]``); and
``SciBERT.__call__`` against the reference's recorded tensors (tests/golden/scibert_cases.json)."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.components.nlp.repr import Repr
from gnn_tableextraction_amd.components.nlp.scibert import SciBERT
from tests import repr_ref
from tests import scibert_ref as ref
from tests import wordlabels_ref as wl
from tests.test_gpu_from_annotations import SIZE, make_page, reference_node_lists

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DATA = ref.golden()
REPR_CASE = [s for s in repr_ref.golden()["sets"] if s["name"] == "normal_c47_d3_p50"][0]
WORDS = ["banana33", "p-value", "33", "1.1", "(1.1,", "Table", "2:", "results", "Caf" + chr(0xE9), "a", "New York", "IMAGE!", "x[SEP]y",
         "b1c2d3f4g5h6j7k8l9", "a" + chr(0x4E2D) + "b", chr(0xB5) + "m", "7"]
N_PAGES = 6
D = DATA["embeddings"].shape[1]


@pytest.fixture(scope="module", params=["mean", "max"])
def embedder(request):
    return SciBERT(DATA["vocab"], DATA["embeddings"], device=DEV, pooling=request.param)


@pytest.fixture(scope="module")
def repr_embedder():
    return Repr(REPR_CASE["repr2idx"], REPR_CASE["embeddings"], REPR_CASE["prototypes"], REPR_CASE["i_embedding"], device=DEV)


@pytest.fixture(scope="module")
def pages():
    """Six synthetic pages: word boxes, texts over the fixture's vocabulary, annotations (four of the pages with figures).  Page 1
    holds short words only: no word of it is as long as the fourteen-piece one, so page by page other words pool [SEP]."""
    rng = np.random.default_rng(78)
    made = [make_page(rng, with_figure=(i % 3 != 1)) for i in range(N_PAGES)]
    texts = [[WORDS[int(i)] for i in rng.integers(0, len(WORDS), size=len(m[0]))] for m in made]
    texts[1] = [["a", "7", "33", "Table"][i % 4] for i in range(len(texts[1]))]
    return [m[0] for m in made], texts, [m[2] for m in made]


def expected(embedder, node_texts):
    tok = embedder.token_ids(node_texts)
    return ref.pool(tok, embedder.table.cpu().numpy(), embedder.pooling)


def same_but_for_the_scibert_columns(got, plain, at):
    feat, base = got.whole.ndata['feat'], plain.whole.ndata['feat']
    assert feat.shape[0] == base.shape[0] and feat.shape[1] == base.shape[1] + D
    assert torch.equal(feat[:, :at], base[:, :at]) and torch.equal(feat[:, at + D:], base[:, at:])
    for a, b in zip(got.whole.edges(), plain.whole.edges()):
        assert torch.equal(a, b)
    assert torch.equal(got.whole.edata['feat'], plain.whole.edata['feat'])
    assert torch.equal(got.whole.ndata['label'], plain.whole.ndata['label'])
    assert got.whole.batch_num_nodes_ == plain.whole.batch_num_nodes_
    o = 0
    for g in got.graphs:                                                 # the per-page host copies carry the same rows
        k = g.ndata['feat'].shape[0]
        assert torch.equal(g.ndata['feat'], feat[o:o + k].cpu())
        o += k
    return feat


@pytest.mark.parametrize("range_island", [0, 2])
@pytest.mark.parametrize("mode", ["knn", "visibility"])
def test_labels_route(pages, embedder, repr_embedder, mode, range_island):
    boxes, texts, anns = pages
    nodes = reference_node_lists(boxes, texts, anns, wl.CAT_MAP)
    nb, nl = [n[0] for n in nodes], [n[1] for n in nodes]
    nt = [list(n[2]) for n in nodes]
    nt[0][5], nt[2][9], nt[4][0] = "", " ", ""                          # empty words: [SEP] alone
    index = [np.arange(len(b), dtype=np.float32).reshape(-1, 1) for b in nb]
    kw = dict(range_island=range_island, extra_feats=index, mode=mode, repr_embedder=repr_embedder)
    got = PrebuiltPages.from_boxes(nb, [SIZE] * N_PAGES, nt, nl, DEV, scibert_embedder=embedder, **kw)
    plain = PrebuiltPages.from_boxes(nb, [SIZE] * N_PAGES, nt, nl, DEV, **kw)
    feat = same_but_for_the_scibert_columns(got, plain, 63)
    assert feat.shape[1] == 13 + 50 + D + 1
    off = np.concatenate([[0], np.cumsum([len(b) for b in nb])])
    page_of = np.repeat(np.arange(N_PAGES), got.whole.batch_num_nodes_)
    kept = off[page_of] + feat[:, 63 + D].cpu().numpy().astype(np.int64)     # the nodes that island removal kept, in the given lists
    if range_island:
        assert len(kept) < off[-1]
    else:
        assert len(kept) == off[-1]
    want = expected(embedder, nt)                                        # on the lists as given
    np.testing.assert_array_equal(feat[:, 63:63 + D].cpu().numpy(), want[kept])
    assert PrebuiltPages.from_boxes(nb, [SIZE] * N_PAGES, nt, nl, DEV, scibert_embedder=None, **kw).whole.ndata['feat'].equal(
        plain.whole.ndata['feat'])
    alone = PrebuiltPages.from_boxes(nb, [SIZE] * N_PAGES, nt, nl, DEV, scibert_embedder=embedder, range_island=range_island, mode=mode)
    assert tuple(alone.whole.ndata['feat'].shape) == (len(kept), 13 + D)                   # [BBOX | SCIBERT]
    np.testing.assert_array_equal(alone.whole.ndata['feat'][:, 13:].cpu().numpy(), want[kept])
    assert torch.equal(alone.whole.ndata['feat'][:, :13], feat[:, :13])


@pytest.mark.parametrize("range_island", [0, 2])
def test_annotations_route_with_figures(pages, embedder, repr_embedder, range_island):
    boxes, texts, anns = pages
    kw = dict(page_annotations=anns, range_island=range_island, repr_embedder=repr_embedder)
    got = PrebuiltPages.from_boxes(boxes, [SIZE] * N_PAGES, texts, None, DEV, scibert_embedder=embedder, **kw)
    plain = PrebuiltPages.from_boxes(boxes, [SIZE] * N_PAGES, texts, None, DEV, **kw)
    feat = same_but_for_the_scibert_columns(got, plain, 63)
    final = [p['texts'] for p in got.pages]
    assert final == [p['texts'] for p in plain.pages]
    node_texts = [list(n[2]) for n in reference_node_lists(boxes, texts, anns, wl.CAT_MAP)]          # figures first, words inside dropped
    assert sum(t[0] == "IMAGE!" for t in node_texts) == 4
    want = expected(embedder, node_texts)
    if not range_island:
        assert final == node_texts
        np.testing.assert_array_equal(feat[:, 63:].cpu().numpy(), want)
    else:                                                                # the kept nodes: a subsequence of each page's list
        assert sum(len(t) for t in final) < sum(len(t) for t in node_texts)
        want_pages = np.split(want, np.cumsum([len(t) for t in node_texts])[:-1])
        got_pages = np.split(feat[:, 63:].cpu().numpy(), np.cumsum([len(t) for t in final])[:-1])
        for w, g, before, after in zip(want_pages, got_pages, node_texts, final):
            j = 0
            for row, text in zip(g, after):                              # rows follow the kept texts in order
                while before[j] != text or not np.array_equal(w[j], row):
                    j += 1
                j += 1


@pytest.mark.parametrize("pooling", ["mean", "max"])
def test_call_returns_the_recorded_reference_tensors(pooling):
    emb = SciBERT(DATA["vocab"], DATA["embeddings"], device=DEV, pooling=pooling)
    pages = [p["words"] for p in DATA["pages"]] + [[]]
    got = emb(None, pages, None)
    assert [tuple(t.shape) for t in got] == [(len(p), D) for p in pages] and all(t.is_cuda for t in got)
    assert emb._online_batch_(None, pages, None)[3].equal(got[3])
    worst = 0.0
    for page, t in zip(DATA["pages"], got):
        mine = t.cpu().numpy().astype(np.float64)
        tok = emb.token_ids([page["words"]])
        bound = ref.mean_bound(tok, DATA["normalized"], page[pooling])
        err = np.abs(mine - page[pooling])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        print(f"{pooling} {page['name']}: max |d| {err.max():.3e}, max |d| / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert np.all(err <= bound), (page["name"], float(err.max()), float((err - bound).max()))
    assert worst <= 1.0
