"""Page regions on the device (gte_page_regions, postprocessing.page_regions / extract_regions, test(regions=True)) against
the CPU union-find of tests/regions_ref.py.  Every output is an integer: all comparisons are exact."""
import json

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd import graph as G
from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.data import synthetic as S
from gnn_tableextraction_amd.models import model_predict
from tests import regions_ref as ref
from tests.predict_setup import config_and_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A


def _abi(indptr, indices, node_off, group, bbox):
    """One direct call of gte_page_regions on outputs prefilled with a sentinel -> (comp, box, count) as numpy arrays."""
    lib, P = _lib.load(), _lib.ptr
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(DEV)
    n = len(group)
    d_indptr, d_indices, d_off, d_group, d_bbox = t(indptr), t(indices), t(node_off), t(group), t(np.asarray(bbox).reshape(-1, 4))
    comp = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    box = torch.full((n, 4), SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    sizes = np.diff(np.asarray(node_off))
    _lib.check(lib.gte_page_regions(P(d_indptr), P(d_indices), P(d_off), len(sizes), n, int(sizes.max()), P(d_group), P(d_bbox),
                                    P(comp), P(box), P(count), _lib.current_stream()), "gte_page_regions")
    torch.cuda.synchronize()
    return comp.cpu().numpy(), box.cpu().numpy(), count.cpu().numpy()


def _assert_equal_ref(got, indptr, indices, node_off, group, bbox):
    want = ref.page_regions_ref(indptr, indices, node_off, group, bbox)
    for name, g, w in zip(("comp", "region_box", "region_count"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=name)
    return want


def _full_from_compact(reg, n):
    """(comp, box [n, 4], count [n]) rebuilt from the compacted result of postprocessing.page_regions."""
    box, count = np.zeros((n, 4), dtype=np.int32), np.zeros(n, dtype=np.int32)
    root = reg.root.cpu().numpy()
    assert (np.diff(root) > 0).all()                      # ascending root order
    box[root], count[root] = reg.box.cpu().numpy(), reg.n_words.cpu().numpy()
    return reg.comp.cpu().numpy(), box, count


def _boxes(rng, n):
    x0, y0 = rng.integers(0, 1500, n), rng.integers(0, 2200, n)
    return np.stack([x0, y0, x0 + rng.integers(1, 120, n), y0 + rng.integers(1, 40, n)], axis=1).astype(np.int32)


def test_hand_cases_through_page_regions():
    # path 0-1-2-3-4-5 (bidirected), groups [4, 4, -1, 4, 1, 1]: components {0, 1}, {3}, {4, 5}, node 2 in none
    src, dst = [0, 1, 1, 2, 2, 3, 3, 4, 4, 5], [1, 0, 2, 1, 3, 2, 4, 3, 5, 4]
    group = np.array([4, 4, -1, 4, 1, 1], dtype=np.int32)
    bbox = _boxes(np.random.default_rng(0), 6)
    g = G.PageGraph(src, dst, 6, device=DEV)
    reg = PP.page_regions(g, torch.from_numpy(group).to(DEV), torch.from_numpy(bbox).to(DEV))
    indptr, indices = ref.in_csr(src, dst, 6)
    _assert_equal_ref(_full_from_compact(reg, 6), indptr, indices, [0, 6], group, bbox)
    assert reg.comp.tolist() == [0, 0, -1, 3, 4, 4] and reg.root.tolist() == [0, 3, 4]
    assert reg.group.tolist() == [4, 4, 1] and reg.n_words.tolist() == [2, 1, 2] and reg.page.tolist() == [0, 0, 0]
    # a directed-only entry 2 -> 0 joins its endpoints; node 1 (no edge at all) is a region of one word; two pages
    g2 = G.batch([G.PageGraph([2], [0], 4, device=DEV), G.PageGraph([0], [1], 2, device=DEV)])
    group2 = np.array([3, 3, 3, -1, 0, 0], dtype=np.int32)
    reg2 = PP.page_regions(g2, torch.from_numpy(group2).to(DEV), torch.from_numpy(bbox).to(DEV))
    indptr2, indices2 = ref.in_csr([2, 4], [0, 5], 6)
    _assert_equal_ref(_full_from_compact(reg2, 6), indptr2, indices2, [0, 4, 6], group2, bbox)
    assert reg2.comp.tolist() == [0, 1, 0, -1, 4, 4] and reg2.root.tolist() == [0, 1, 4] and reg2.page.tolist() == [0, 0, 1]


def test_direct_call_over_page_sizes_one_empty_small_two_passes_and_the_limit():
    """pages of 1, 0, 7, 300 and 4096 nodes: a single node, an empty page, below and above one workgroup's 256 threads, and
    gte_region_max_page_nodes(); random edges inside pages, groups from {-1, 0, 1, 2}; every output row prefilled."""
    lib = _lib.load()
    limit = lib.gte_region_max_page_nodes()
    assert limit == 4096
    rng = np.random.default_rng(11)
    sizes = [1, 0, 7, 300, limit]
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    src, dst = [], []
    for p, s in enumerate(sizes):
        e = int(0.7 * s)                                  # sparse: many components of many sizes
        src.append(off[p] + rng.integers(0, max(s, 1), e))
        dst.append(off[p] + rng.integers(0, max(s, 1), e))
    src, dst = np.concatenate(src), np.concatenate(dst)
    group = rng.integers(-1, 3, n).astype(np.int32)
    bbox = _boxes(rng, n)
    indptr, indices = ref.in_csr(src, dst, n)
    got = _abi(indptr, indices, off, group, bbox)
    want = _assert_equal_ref(got, indptr, indices, off, group, bbox)
    assert want[2].max() > 3 and (want[0] == -1).any()    # the case has real components and nodes outside every region


@pytest.fixture(scope="module")
def random_path():
    rng = np.random.default_rng(5)
    n = 4096
    order = rng.permutation(n)                            # the path visits the nodes in this order
    return n, order, _boxes(rng, n)


@pytest.mark.parametrize("bidirected", [False, True])
def test_one_long_path_in_random_node_order_converges_to_one_region(random_path, bidirected):
    n, order, bbox = random_path
    src, dst = order[:-1], order[1:]
    if bidirected:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    indptr, indices = ref.in_csr(src, dst, n)
    comp, box, count = _abi(indptr, indices, [0, n], np.zeros(n, dtype=np.int32), bbox)
    assert (comp == 0).all() and count[0] == n and not count[1:].any()
    assert box[0].tolist() == [bbox[:, 0].min(), bbox[:, 1].min(), bbox[:, 2].max(), bbox[:, 3].max()] and not box[1:].any()


def test_the_path_with_the_kind_alternating_every_64_positions_gives_64_regions(random_path):
    n, order, bbox = random_path
    group = np.empty(n, dtype=np.int32)
    group[order] = (np.arange(n) // 64) % 2
    indptr, indices = ref.in_csr(order[:-1], order[1:], n)
    got = _abi(indptr, indices, [0, n], group, bbox)
    want = _assert_equal_ref(got, indptr, indices, [0, n], group, bbox)
    assert int((want[2] > 0).sum()) == 64 and (want[2][want[2] > 0] == 64).all()


def test_self_loops_and_doubled_entries_change_nothing():
    rng = np.random.default_rng(3)
    n = 500
    src, dst = rng.integers(0, n, 350), rng.integers(0, n, 350)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    group = rng.integers(-1, 3, n).astype(np.int32)
    bbox = _boxes(rng, n)
    indptr, indices = ref.in_csr(src, dst, n)
    simple = _abi(indptr, indices, [0, n], group, bbox)
    _assert_equal_ref(simple, indptr, indices, [0, n], group, bbox)
    loops = np.arange(n)
    indptr2, indices2 = ref.in_csr(np.concatenate([src, src, loops]), np.concatenate([dst, dst, loops]), n)
    for a, b in zip(simple, _abi(indptr2, indices2, [0, n], group, bbox)):
        np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def realistic():
    data = PrebuiltPages.synthetic(20, in_feats=13)
    src, dst, _, _, label, off = S.concat_pages(data.page_arrays)
    n = int(off[-1])
    bbox = np.concatenate([p.bbox for p in data.page_arrays]).astype(np.int32)
    indptr, indices = ref.in_csr(src, dst, n)
    preds = {"random": np.random.default_rng(7).integers(0, 9, n), "labels": label.astype(np.int64)}
    table = np.asarray(PP.DEFAULT_CLASS_GROUP, dtype=np.int32)
    want = {k: ref.page_regions_ref(indptr, indices, off, table[p], bbox) for k, p in preds.items()}
    return data, off, bbox, preds, want


@pytest.mark.parametrize("which", ["random", "labels"])
@pytest.mark.parametrize("through", ["batch", "resident"])
def test_synthetic_pages_with_their_knn_edges(realistic, which, through):
    """20 synthetic pages (their own k-NN edges and boxes), predictions uniform over the 9 classes / equal to the labels, kinds
    from DEFAULT_CLASS_GROUP, through graph.batch and through a ResidentBatch."""
    data, off, bbox, preds, want = realistic
    n = int(off[-1])
    if through == "batch":
        g = G.batch([pg.to(DEV) for pg in data.graphs])
    else:
        g = G.ResidentPages(data.graphs, DEV).batch(list(range(len(data.graphs))))
    table = torch.tensor(PP.DEFAULT_CLASS_GROUP, dtype=torch.int32, device=DEV)
    group = table[torch.from_numpy(preds[which]).to(DEV)]
    reg = PP.page_regions(g, group, torch.from_numpy(bbox).to(DEV))
    for name, a, b in zip(("comp", "region_box", "region_count"), _full_from_compact(reg, n), want[which]):
        np.testing.assert_array_equal(a, b, err_msg=name)
    roots = reg.root.cpu().numpy()
    np.testing.assert_array_equal(reg.page.cpu().numpy(), np.searchsorted(off[1:], roots, side="right"))
    np.testing.assert_array_equal(reg.group.cpu().numpy(), group.cpu().numpy()[roots])
    assert len(roots) > len(data.graphs)


def test_test_entry_point_returns_and_writes_the_regions(tmp_path):
    """test(data, config, regions=True) on 6 synthetic pages: result['regions'] is the CPU reference applied to result['all_pred'],
    the JSON file parses back to the same boxes, and regions=False returns exactly the keys it returned before."""
    data = PrebuiltPages.synthetic(6, in_feats=13)
    cfg, _, logs = config_and_weights(tmp_path)
    out = model_predict.test(data, cfg, regions=True)
    src, dst, _, _, _, off = S.concat_pages(data.page_arrays)
    n = int(off[-1])
    bbox = np.concatenate([p.bbox for p in data.page_arrays]).astype(np.int32)
    indptr, indices = ref.in_csr(src, dst, n)
    group = np.asarray(PP.DEFAULT_CLASS_GROUP, dtype=np.int32)[np.concatenate(out["all_pred"])]
    comp, box, count = ref.page_regions_ref(indptr, indices, off, group, bbox)
    want = ref.regions_list(comp, box, count, off, group)
    assert out["regions"] == want
    # a model that has not been trained may put every word into 'other': the same pages with their labels as predictions
    by_label = PP.extract_regions(data, [p.label for p in data.page_arrays], min_words=2, batch_pages=4)
    lgroup = np.asarray(PP.DEFAULT_CLASS_GROUP, dtype=np.int32)[np.concatenate([p.label for p in data.page_arrays])]
    lwant = ref.regions_list(*ref.page_regions_ref(indptr, indices, off, lgroup, bbox), off, lgroup, min_words=2)
    assert by_label == lwant and sum(len(p) for p in lwant) > 6
    doc = json.load(open(tmp_path / "regions" / f"{logs}.json"))
    assert set(doc) >= {"text", "title", "list", "table", "figure", "caption"}
    names = {4: "table", 1: "text", 2: "title", 3: "list", 5: "figure", 6: "caption"}
    for i, page in enumerate(want):
        for kind, name in names.items():
            boxes = [b for k, b, _ in page if k == kind]
            entry = doc[name].get(data.pages[i]["page"], {"bboxes": [], "scores": []})
            assert entry["bboxes"] == boxes and entry["scores"] == [1.0] * len(boxes)
    plain = model_predict.test(data, cfg, save_predictions=False)
    assert set(plain) == {"accuracy", "accuracy_nodes", "precision", "recall", "f1", "confusion", "all_pred", "all_pred_flat"}
    assert set(out) == set(plain) | {"regions"}
    for a, b in zip(out["all_pred"], plain["all_pred"]):
        np.testing.assert_array_equal(a, b)
