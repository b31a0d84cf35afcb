"""The CPU reference of gte_page_regions (tests/regions_ref.py) against hand cases and scipy's connected components."""
import numpy as np
import pytest

from tests import regions_ref as ref


def _boxes(n):
    i = np.arange(n, dtype=np.int32)
    return np.stack([10 * i, 7 * i + 3, 10 * i + 8, 7 * i + 9], axis=1)


def test_path_with_two_kinds_and_a_node_outside_every_region():
    # path 0-1-2-3-4-5, bidirected
    src = [0, 1, 1, 2, 2, 3, 3, 4, 4, 5]
    dst = [1, 0, 2, 1, 3, 2, 4, 3, 5, 4]
    indptr, indices = ref.in_csr(src, dst, 6)
    group = np.array([4, 4, -1, 4, 1, 1])
    bbox = _boxes(6)
    comp, box, count = ref.page_regions_ref(indptr, indices, [0, 6], group, bbox)
    assert comp.tolist() == [0, 0, -1, 3, 4, 4]           # {0, 1}, {3}, {4, 5}; node 2 belongs to no region
    assert count.tolist() == [2, 0, 0, 1, 2, 0]
    assert box[0].tolist() == [0, 3, 18, 16] and box[3].tolist() == bbox[3].tolist() and box[4].tolist() == [40, 31, 58, 44]
    assert not box[[1, 2, 5]].any()
    regs = ref.regions_list(comp, box, count, [0, 6], group)
    assert regs == [[(4, [0, 3, 18, 16], 2), (4, bbox[3].tolist(), 1), (1, [40, 31, 58, 44], 2)]]
    assert ref.regions_list(comp, box, count, [0, 6], group, min_words=2) == [[(4, [0, 3, 18, 16], 2), (1, [40, 31, 58, 44], 2)]]


def test_a_directed_only_edge_joins_its_endpoints_and_an_isolated_node_is_a_region_of_one_word():
    indptr, indices = ref.in_csr([2], [0], 4)             # the one entry 2 -> 0; nodes 1 and 3 have no edge at all
    group = np.array([3, 3, 3, -1])
    comp, box, count = ref.page_regions_ref(indptr, indices, [0, 4], group, _boxes(4))
    assert comp.tolist() == [0, 1, 0, -1]
    assert count.tolist() == [2, 1, 0, 0]
    assert box[0].tolist() == [0, 3, 28, 23] and box[1].tolist() == _boxes(4)[1].tolist()
    # the same entry the other way round: the same answer
    indptr2, indices2 = ref.in_csr([0], [2], 4)
    for a, b in zip((comp, box, count), ref.page_regions_ref(indptr2, indices2, [0, 4], group, _boxes(4))):
        np.testing.assert_array_equal(a, b)


def test_an_entry_that_leaves_its_page_is_skipped_and_empty_pages_are_legal():
    indptr, indices = ref.in_csr([0, 2, 1], [1, 1, 2], 3)  # pages {0, 1}, {}, {2}: 2 -> 1 and 1 -> 2 cross pages
    comp, _, count = ref.page_regions_ref(indptr, indices, [0, 2, 2, 3], np.zeros(3, dtype=np.int64), _boxes(3))
    assert comp.tolist() == [0, 0, 2] and count.tolist() == [2, 0, 1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_equals_scipy_connected_components_on_random_graphs(seed):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(seed)
    sizes = [1, 0, 40, 150, 9]
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    src, dst = [], []
    for p, s in enumerate(sizes):
        e = int(0.8 * s)
        src.append(off[p] + rng.integers(0, max(s, 1), e))
        dst.append(off[p] + rng.integers(0, max(s, 1), e))
    src, dst = np.concatenate(src), np.concatenate(dst)
    group = rng.integers(-1, 3, n)
    bbox = rng.integers(0, 2000, (n, 4)).astype(np.int32)
    indptr, indices = ref.in_csr(src, dst, n)
    comp, box, count = ref.page_regions_ref(indptr, indices, off, group, bbox)
    keep = (group[src] == group[dst]) & (group[src] >= 0)
    a = sp.coo_matrix((np.ones(int(keep.sum())), (src[keep], dst[keep])), shape=(n, n))
    _, lab = connected_components(a, directed=False)
    for c in np.unique(lab):
        members = np.nonzero(lab == c)[0]
        if group[members[0]] < 0:
            assert len(members) == 1 and comp[members[0]] == -1 and count[members[0]] == 0
            continue
        r = members.min()
        assert (comp[members] == r).all() and count[r] == len(members) and not count[members[members != r]].any()
        want = [bbox[members, 0].min(), bbox[members, 1].min(), bbox[members, 2].max(), bbox[members, 3].max()]
        assert box[r].tolist() == want
