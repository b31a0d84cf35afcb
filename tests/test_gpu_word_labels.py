"""Word labels and figure nodes on the device (gte_word_labels, gte_word_labels_compact) against tests/wordlabels_ref.py and the
reference's own answers (tests/golden/word_labels_cases.json): direct ABI calls on sentinel-prefilled outputs.  Every output is an
integer: all comparisons are exact."""
import json
import os

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from tests import wordlabels_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "word_labels_cases.json")
OTHER, TEXT, TITLE, LIST, TABLE, FIGURE, CAPTION, COLH, SP, GCELL, TCELL, COL, ROW = range(13)
SKIP_MASK = sum(1 << c for c in ref.SKIP)
INVALID_ARGUMENT = -1                                                   # GTE_ERR_INVALID_ARGUMENT of include/gte.h
NAN = float("nan")


def _pack(pages):
    """pages = [(word boxes [n, 4], annotation rows [a, 5] = r0, r1, r2, r3, category)] -> the ABI's five input arrays (numpy)."""
    bbox = np.concatenate([np.asarray(w, dtype=np.int64).reshape(-1, 4) for w, _ in pages]).astype(np.int32)
    rows = [np.asarray(a, dtype=np.float64).reshape(-1, 5) for _, a in pages]
    ann_box = np.ascontiguousarray(np.concatenate(rows)[:, :4])
    ann_cat = np.concatenate(rows)[:, 4].astype(np.int32)
    node_off = np.concatenate([[0], np.cumsum([len(np.asarray(w).reshape(-1, 4)) for w, _ in pages])]).astype(np.int32)
    ann_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return bbox, node_off, ann_box, ann_cat, ann_off


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _full(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)


def _label(arrays, n_cat=13, skip_mask=SKIP_MASK, figure_cat=FIGURE):
    """One direct call of gte_word_labels on sentinel-prefilled outputs -> (code, word_label, word_ann, page_counts, device inputs)."""
    lib, P = _lib.load(), _lib.ptr
    bbox, node_off, ann_box, ann_cat, ann_off = arrays
    d = [_dev(a) for a in arrays]
    n_pages = len(node_off) - 1
    word_label, word_ann, counts = _full((len(bbox),)), _full((len(bbox),)), _full((n_pages, 2))
    code = lib.gte_word_labels(P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d[4]), n_pages, len(bbox), len(ann_cat), n_cat, skip_mask,
                               figure_cat, P(word_label), P(word_ann), P(counts), _lib.current_stream())
    torch.cuda.synchronize()
    return code, word_label, word_ann, counts, d


def _compact(arrays, d, word_label, out_off, n_out, cat_map=None, n_cat=13, figure_cat=FIGURE, slack=3):
    """One direct call of gte_word_labels_compact; the outputs have ``slack`` rows beyond n_out -> (code, bbox, label, src, status)."""
    lib, P = _lib.load(), _lib.ptr
    bbox, node_off, ann_box, ann_cat, ann_off = arrays
    n_pages = len(node_off) - 1
    out_bbox, out_label, out_src = _full((n_out + slack, 4)), _full((n_out + slack,)), _full((n_out + slack,))
    status = _full((n_pages,))
    d_off = _dev(np.asarray(out_off, dtype=np.int32))
    d_map = None if cat_map is None else _dev(np.asarray(cat_map, dtype=np.int32))
    code = lib.gte_word_labels_compact(P(d[0]), P(d[1]), P(word_label), P(d[2]), P(d[3]), P(d[4]), P(d_off), P(d_map), n_pages,
                                       len(bbox), len(ann_cat), n_cat, figure_cat, n_out, P(out_bbox), P(out_label), P(out_src),
                                       P(status), _lib.current_stream())
    torch.cuda.synchronize()
    return code, out_bbox.cpu().numpy(), out_label.cpu().numpy(), out_src.cpu().numpy(), status.cpu().numpy()


def _assert_equal_ref(pages, cat_map=None, n_cat=13, skip=ref.SKIP, figure_cat=FIGURE):
    """Both calls on ``pages`` against the reference -> (word_label, word_ann, page_counts, out_bbox, out_label, out_src, out_off)."""
    arrays = _pack(pages)
    want = ref.label_batch(*arrays, n_cat, skip, figure_cat)
    code, word_label, word_ann, counts, d = _label(arrays, n_cat, sum(1 << c for c in skip), figure_cat)
    assert code == 0
    np.testing.assert_array_equal(word_label.cpu().numpy(), want[0])
    np.testing.assert_array_equal(word_ann.cpu().numpy(), want[1])
    np.testing.assert_array_equal(counts.cpu().numpy(), want[2])
    boxes, labels, srcs, off = ref.compact_batch(*arrays, want[0], cat_map, n_cat, figure_cat)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(want[2].sum(1))]))
    m = int(off[-1])
    code, out_bbox, out_label, out_src, status = _compact(arrays, d, word_label, off, m, cat_map, n_cat, figure_cat)
    assert code == 0
    np.testing.assert_array_equal(status, np.zeros(len(pages), dtype=np.int32))
    np.testing.assert_array_equal(out_bbox[:m], boxes)
    np.testing.assert_array_equal(out_label[:m], labels)
    np.testing.assert_array_equal(out_src[:m], srcs)
    for a in (out_bbox[m:], out_label[m:], out_src[m:]):                 # rows at and beyond n_out keep the sentinel
        np.testing.assert_array_equal(a, np.full_like(a, SENTINEL))
    return want[0], want[1], want[2], boxes, labels, srcs, off


def _golden_pages():
    with open(GOLDEN) as f:
        g = json.load(f)
    pages = [(c["words"], [[NAN if v is None else v for v in r] for r in c["annotations"]]) for c in g["cases"]]
    return g["cases"], pages


def _words(rng, n, width=1600, height=2200):
    x0, y0 = rng.integers(0, width, n), rng.integers(0, height, n)
    return np.stack([x0, y0, x0 + rng.integers(0, 120, n), y0 + rng.integers(0, 30, n)], axis=1).astype(np.int32)


# ---- golden ------------------------------------------------------------------------------------------------------------------
def test_every_golden_case_alone():
    cases, pages = _golden_pages()
    assert len(cases) >= 40
    for c, page in zip(cases, pages):
        label, ann, counts, boxes, labels, srcs, _ = _assert_equal_ref([page])
        assert label.tolist() == c["word_label"] and ann.tolist() == c["word_ann"], c["name"]
        assert counts.tolist() == [[len(c["figures"]), sum(c["kept"])]], c["name"]
        assert labels.tolist() == c["node_labels"], c["name"]
        assert srcs.tolist() == [-1 - j for j in c["figures"]] + [w for w in c["node_words"] if w >= 0], c["name"]
        assert boxes.tolist() == [[int(v) for v in b] for b in c["node_boxes"]], c["name"]


def test_all_golden_cases_in_one_batch_change_nothing():
    cases, pages = _golden_pages()
    label, ann, counts, boxes, labels, srcs, off = _assert_equal_ref(pages, cat_map=ref.CAT_MAP)
    _, node_off, _, _, ann_off = _pack(pages)
    for k, c in enumerate(cases):
        assert label[node_off[k]:node_off[k + 1]].tolist() == c["word_label"], c["name"]
        assert ann[node_off[k]:node_off[k + 1]].tolist() == [ann_off[k] + j if j >= 0 else -1 for j in c["word_ann"]], c["name"]
        assert labels[off[k]:off[k + 1]].tolist() == [ref.CAT_MAP[v] for v in c["node_labels"]], c["name"]
        assert boxes[off[k]:off[k + 1]].tolist() == [[int(v) for v in b] for b in c["node_boxes"]], c["name"]


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_centre_truncation():
    big = 2 ** 31 - 1
    # odd and even sums: centres 5 and 5 (11 / 2 truncated); the rectangle holds 5 only
    got = _assert_equal_ref([([[0, 0, 10, 10], [0, 0, 11, 11], [0, 0, 12, 12]], [[4.5, 4.5, 5.5, 5.5, TEXT]])])
    assert got[0].tolist() == [TEXT, TEXT, OTHER]
    # negative sums: -11 / 2 is -5 (towards zero), floor would say -6
    got = _assert_equal_ref([([[-11, -11, 0, 0], [-12, -12, 0, 0], [-1, -1, 0, 0]],
                              [[-5.5, -5.5, -4.5, -4.5, TEXT], [-6.5, -6.5, -5.5, -5.5, TITLE], [-0.5, -0.5, 0.5, 0.5, LIST]])])
    assert got[0].tolist() == [TEXT, TITLE, LIST]
    # a zero-size word is its own centre
    got = _assert_equal_ref([([[7, 7, 7, 7], [8, 8, 8, 8]], [[6, 6, 8, 8, CAPTION]])])
    assert got[0].tolist() == [CAPTION, OTHER]
    # sums that need 64 bits: 2 * (2^31 - 1), 2 * -2^31, and -2^31 + 2^31 - 1 = -1 -> 0
    got = _assert_equal_ref([([[big, big, big, big], [-big - 1, -big - 1, -big - 1, -big - 1], [-big - 1, -big - 1, big, big],
                               [big - 1, big - 1, big, big]],
                              [[big - 0.5, big - 0.5, big + 0.5, big + 0.5, TEXT], [-big - 1.5, -big - 1.5, -big - 0.5, -big - 0.5, TITLE],
                               [-0.5, -0.5, 0.5, 0.5, LIST], [big - 1.5, big - 1.5, big - 0.5, big - 0.5, SP]])])
    assert got[0].tolist() == [TEXT, TITLE, LIST, SP]


def test_strictness():
    rect = [[10, 10, 30, 30, TEXT]]
    on_edges = [[10, 20, 10, 20], [30, 20, 30, 20], [20, 10, 20, 10], [20, 30, 20, 30], [10, 10, 10, 10], [30, 30, 30, 30]]
    inside = [[11, 20, 11, 20], [29, 20, 29, 20], [20, 11, 20, 11], [20, 29, 20, 29]]
    got = _assert_equal_ref([(on_edges + inside, rect)])
    assert got[0].tolist() == [OTHER] * 6 + [TEXT] * 4
    assert got[1].tolist() == [-1] * 6 + [0] * 4
    # half-integer edges: (10.5, 11.5) holds 11 only; (9.5, 10.5) holds 10 only
    got = _assert_equal_ref([([[10, 10, 10, 10], [11, 11, 11, 11], [12, 12, 12, 12], [9, 9, 9, 9]],
                              [[10.5, 10.5, 11.5, 11.5, TITLE], [9.5, 9.5, 10.5, 10.5, LIST]])])
    assert got[0].tolist() == [LIST, TITLE, OTHER, OTHER]


def test_order_and_exclusion():
    word = [[5, 5, 15, 15]]
    a, b = [0, 0, 20, 20, TEXT], [5, 5, 15, 15, TITLE]
    assert _assert_equal_ref([(word, [a, b])])[0].tolist() == [TEXT]
    assert _assert_equal_ref([(word, [b, a])])[0].tolist() == [TITLE]
    # TABLE (and its grid cells, columns, rows) listed first are passed over: the cell wins
    table = [[0, 0, 100, 100, TABLE], [0, 0, 100, 100, GCELL], [0, 0, 100, 100, COL], [0, 0, 100, 100, ROW], [2, 2, 18, 18, TCELL]]
    got = _assert_equal_ref([(word, table)])
    assert got[0].tolist() == [TCELL] and got[1].tolist() == [4]
    # FIGURE first: dropped (the figure is a node, the word is not); TEXT first, then FIGURE: kept as TEXT
    got = _assert_equal_ref([(word, [[0, 0, 20, 20, FIGURE], a])])
    assert got[0].tolist() == [-1] and got[2].tolist() == [[1, 0]] and got[5].tolist() == [-1]
    got = _assert_equal_ref([(word, [a, [0, 0, 20, 20, FIGURE]])])
    assert got[0].tolist() == [TEXT] and got[2].tolist() == [[1, 1]] and got[5].tolist() == [-2, 0]
    # a category outside [0, n_cat) never wins -- nor does it reach past the mask's 32 bits
    got = _assert_equal_ref([(word, [[0, 0, 20, 20, 13], [0, 0, 20, 20, -1], [0, 0, 20, 20, 45], [0, 0, 20, 20, 2 ** 31 - 1], b])])
    assert got[0].tolist() == [TITLE] and got[1].tolist() == [4]
    assert _assert_equal_ref([(word, [[0, 0, 20, 20, 7], b])], n_cat=7)[0].tolist() == [TITLE]
    # NaN and inverted rectangles never win
    bad = [[NAN, 0, 20, 20, TEXT], [0, NAN, 20, 20, TEXT], [0, 0, NAN, 20, TEXT], [0, 0, 20, NAN, TEXT], [20, 20, 0, 0, LIST],
           [20, 0, 0, 20, LIST], [0, 20, 20, 0, LIST]]
    assert _assert_equal_ref([(word, bad)])[0].tolist() == [OTHER]
    got = _assert_equal_ref([(word, bad + [b])])
    assert got[0].tolist() == [TITLE] and got[1].tolist() == [7]


# ---- chunks ------------------------------------------------------------------------------------------------------------------
def _far(n, cat=TEXT):
    """n annotations that hold no word of these tests (they lie left of x = -100)."""
    k = np.arange(n, dtype=np.float64)
    return np.stack([-1000 - k, -1000 - k, -200 - k % 7, -200 - k % 5, np.full(n, cat, dtype=np.float64)], axis=1)


def test_chunk_boundaries():
    C = _lib.load().gte_word_labels_chunk()
    assert 4 <= C <= 48 * 1024 // 32
    hold = lambda x, cat: [x - 2, 0, x + 2, 10, cat]                     # holds a word centred at (x, 5)
    word = lambda x: [x - 1, 4, x + 1, 6]
    pages = []
    for n in (C - 1, C, C + 1, 2 * C + 1):                                # the only winner is the last annotation
        ann = _far(n)
        ann[-1] = hold(50, LIST)
        pages.append(([word(50), word(90)], ann))
    ann = _far(2 * C)                                                    # annotation 5 and annotation C + 3 hold the word: 5
    ann[5], ann[C + 3] = hold(50, TITLE), hold(50, LIST)
    pages.append(([word(50)], ann))
    ann = _far(C + 2)                                                    # only annotation C, the first of the second chunk
    ann[C] = hold(50, CAPTION)
    pages.append(([word(50)], ann))
    ann = _far(2 * C + 9)                                                # chunk 1 for some words, chunk 3 for others, none for the rest
    ann[3], ann[2 * C + 5], ann[2 * C + 6] = hold(50, TITLE), hold(70, SP), hold(50, LIST)
    words = [word(50), word(70), word(90)] * 400                         # more words than threads: LDS is restaged per tile
    pages.append((words, ann))
    for page in pages[:-1]:                                              # alone (the last one is checked inside the batch)
        _assert_equal_ref([page])
    got = _assert_equal_ref(pages)
    off = np.concatenate([[0], np.cumsum([len(w) for w, _ in pages])])
    a_off = np.concatenate([[0], np.cumsum([len(a) for _, a in pages])])
    for k, n in enumerate((C - 1, C, C + 1, 2 * C + 1)):
        assert got[0][off[k]:off[k + 1]].tolist() == [LIST, OTHER]
        assert got[1][off[k]:off[k + 1]].tolist() == [a_off[k] + n - 1, -1]
    assert got[0][off[4]] == TITLE and got[1][off[4]] == a_off[4] + 5
    assert got[0][off[5]] == CAPTION and got[1][off[5]] == a_off[5] + C
    assert got[0][off[6]:off[6] + 3].tolist() == [TITLE, SP, OTHER]
    assert got[1][off[6]:off[6] + 3].tolist() == [a_off[6] + 3, a_off[6] + 2 * C + 5, -1]


# ---- compaction --------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def _page_with_pattern(n, pattern, n_fig, rng):
    """n words in a row, the dropped ones (by ``pattern``) inside one of ``n_fig`` figures interleaved with other annotations."""
    i = np.arange(n)
    drop = {"all": np.zeros(n, bool), "none": np.ones(n, bool), "alternating": i % 2 == 1, "one_per_wave": i % 64 == 17}[pattern]
    if n_fig == 0:
        drop[:] = False
    x = 10 * i
    words = np.stack([x, np.where(drop, 1000, 0) + 2, x + 4, np.where(drop, 1000, 0) + 8], axis=1)
    ann = [[-5, 20, 10 * n, 40, TEXT]]
    for f in range(n_fig):                                               # every figure spans the row of dropped words
        ann.append([-5 - f, 990 - f, 10 * n + f, 1020 + f, FIGURE])
        ann.append([int(rng.integers(0, 10 * n)), -3, int(rng.integers(0, 10 * n)) + 30, 12, int(rng.choice([TEXT, TITLE, TABLE, TCELL]))])
    return words, ann


@pytest.mark.parametrize("pattern,n_fig", [("all", 0), ("all", 1), ("none", 1), ("none", 70), ("alternating", 1),
                                           ("alternating", 70), ("one_per_wave", 1), ("one_per_wave", 70)])
def test_compaction_keeps_the_order(pattern, n_fig):
    rng = np.random.default_rng(11)
    pages = [_page_with_pattern(n, pattern, n_fig, rng) for n in SIZES]
    got = _assert_equal_ref(pages, cat_map=ref.CAT_MAP)
    off, node_off = got[6], np.concatenate([[0], np.cumsum(SIZES)])
    for k, n in enumerate(SIZES):
        src = got[5][off[k]:off[k + 1]]
        assert (src[:n_fig] < 0).all() and (np.diff(src[:n_fig]) == -2).all()            # figures first, in annotation order
        words = src[n_fig:]
        assert (words >= node_off[k]).all() and (words < node_off[k + 1]).all() and (np.diff(words) > 0).all()
        if pattern == "none" and n_fig:
            assert len(words) == 0
        if pattern == "all" or n_fig == 0:
            assert len(words) == n
        if pattern == "one_per_wave" and n_fig:
            assert len(words) == n - len(range(17, n, 64))
    assert (got[4][got[5] < 0] == ref.CAT_MAP[FIGURE]).all()


def test_cat_map_identity_and_the_references():
    rng = np.random.default_rng(5)
    words = _words(rng, 300, 400, 400)
    ann = [[float(x), float(y), float(x + 90), float(y + 90), c] for c, (x, y) in
           zip([TEXT, TITLE, LIST, FIGURE, CAPTION, COLH, SP, TCELL, TABLE, ROW, OTHER],
               [(0, 0), (100, 0), (200, 0), (300, 0), (0, 100), (100, 100), (200, 100), (300, 100), (0, 0), (0, 200), (100, 200)])]
    same = _assert_equal_ref([(words, ann)], cat_map=None)
    conv = _assert_equal_ref([(words, ann)], cat_map=ref.CAT_MAP)
    assert set(same[4].tolist()) >= {TEXT, TITLE, LIST, FIGURE, CAPTION, COLH, SP, TCELL, OTHER}
    assert conv[4].tolist() == [ref.CAT_MAP[c] for c in same[4].tolist()]
    assert same[4][0] == FIGURE and conv[4][0] == 4                      # FIGURE 5 -> 4
    assert (conv[4] >= 0).all()                                          # the categories without a class never label a node


def test_empty_shapes():
    fig, text = [0, 0, 9, 9, FIGURE], [0, 0, 9, 9, TEXT]
    got = _assert_equal_ref([([], [fig, text])])                        # no words
    assert got[2].tolist() == [[1, 0]] and got[5].tolist() == [-1]
    got = _assert_equal_ref([([[1, 2, 3, 4], [5, 6, 7, 8]], [])])        # no annotations
    assert got[0].tolist() == [0, 0] and got[1].tolist() == [-1, -1] and got[5].tolist() == [0, 1]
    got = _assert_equal_ref([([[1, 1, 3, 3]], [fig, [20, 20, 30, 30, FIGURE]])])        # only figures are left
    assert got[5].tolist() == [-1, -2] and got[3].tolist() == [[0, 0, 9, 9], [20, 20, 30, 30]]
    got = _assert_equal_ref([([], []), ([[1, 1, 3, 3]], [text]), ([], []), ([], [fig])])
    assert got[6].tolist() == [0, 0, 1, 1, 2]
    lib = _lib.load()                                                    # zero pages: nothing to launch, no pointer needed
    assert lib.gte_word_labels(0, 0, 0, 0, 0, 0, 0, 0, 13, SKIP_MASK, FIGURE, 0, 0, 0, _lib.current_stream()) == 0
    assert lib.gte_word_labels_compact(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 13, FIGURE, 0, 0, 0, 0, 0, _lib.current_stream()) == 0


def test_figure_boxes_are_clamped_not_undefined():
    """The ABI is defined for every double (the host refuses such figures before they get here)."""
    ann = [[-1e300, 1e300, NAN, 2.0 ** 30 + 5, FIGURE], [-2.75, 2.75, float("inf"), float("-inf"), FIGURE]]
    got = _assert_equal_ref([([[1, 1, 3, 3]], ann)])
    assert got[3].tolist() == [[-2 ** 30, 2 ** 30, 0, 2 ** 30], [-2, 2, 2 ** 30, -2 ** 30], [1, 1, 3, 3]]


# ---- contract edges ----------------------------------------------------------------------------------------------------------
def test_a_wrong_out_off_run_leaves_its_page_untouched():
    rng = np.random.default_rng(3)
    pages = [(_words(rng, 70), [[0, 0, 800, 1100, TEXT], [0, 0, 50, 50, FIGURE]]) for _ in range(4)]
    arrays = _pack(pages)
    want_label = ref.label_batch(*arrays)[0]
    boxes, labels, srcs, off = ref.compact_batch(*arrays, want_label)
    code, word_label, _, _, d = _label(arrays)
    assert code == 0
    m = int(off[-1])
    for wrong in ([off[0], off[1], off[2] - 1, off[3], off[4]],          # page 1 one row short, page 2 one row long
                  [off[0], off[1], off[2], off[3], m + 1],               # page 3 runs past n_out
                  [off[0], off[2], off[1], off[3], off[4]]):             # page 1 descending, pages 0 and 2 wrong with it
        code, out_bbox, out_label, out_src, status = _compact(arrays, d, word_label, wrong, m)
        assert code == 0
        good = [int(wrong[p] == off[p] and wrong[p + 1] == off[p + 1]) for p in range(4)]
        assert status.tolist() == [0 if g else 2 for g in good]
        assert 0 < sum(good) < 4
        for p in range(4):
            rows = slice(off[p], off[p + 1])
            if good[p]:
                np.testing.assert_array_equal(out_bbox[rows], boxes[rows])
                np.testing.assert_array_equal(out_label[rows], labels[rows])
                np.testing.assert_array_equal(out_src[rows], srcs[rows])
            else:
                for a in (out_bbox[rows], out_label[rows], out_src[rows]):
                    np.testing.assert_array_equal(a, np.full_like(a, SENTINEL))


def test_null_and_misaligned_pointers_are_refused_before_any_launch():
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(4)
    arrays = _pack([(_words(rng, 40), [[0, 0, 800, 1100, TEXT], [0, 0, 50, 50, FIGURE]])])
    d = [_dev(a) for a in arrays]
    n, na = len(arrays[0]), len(arrays[3])
    outs = [_full((n + 1,)), _full((n + 1,)), _full((1, 2))]
    stream = _lib.current_stream()

    def label(ptrs, o, n_cat=13, figure_cat=FIGURE, sizes=(1, n, na)):
        return lib.gte_word_labels(*ptrs, *sizes, n_cat, SKIP_MASK, figure_cat, *o, stream)

    ins, o = [P(t) for t in d], [P(t) for t in outs]
    for k in range(5):
        assert label(ins[:k] + [0] + ins[k + 1:], o) == INVALID_ARGUMENT
    for k in range(3):
        assert label(ins, o[:k] + [0] + o[k + 1:]) == INVALID_ARGUMENT
    assert label([ins[0] + 4] + ins[1:], o) == INVALID_ARGUMENT                      # bbox is read 16 bytes at a time
    assert label(ins[:2] + [ins[2] + 4] + ins[3:], o) == INVALID_ARGUMENT            # doubles
    assert label(ins, [o[0] + 2] + o[1:]) == INVALID_ARGUMENT
    assert label(ins, o, n_cat=0) == INVALID_ARGUMENT and label(ins, o, n_cat=33) == INVALID_ARGUMENT
    assert label(ins, o, figure_cat=13) == INVALID_ARGUMENT and label(ins, o, figure_cat=-1) == INVALID_ARGUMENT
    assert label(ins, o, sizes=(-1, n, na)) == INVALID_ARGUMENT and label(ins, o, sizes=(1, 2 ** 31, na)) == INVALID_ARGUMENT
    assert b"word_labels" in lib.gte_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert (t == SENTINEL).all()

    code, word_label, _, counts, _ = _label(arrays)
    assert code == 0
    m = int(counts.sum())
    d_off = _dev(np.array([0, m], dtype=np.int32))
    c_outs = [_full((m + 1, 4)), _full((m + 1,)), _full((m + 1,)), _full((1,))]
    c_ins = [ins[0], ins[1], P(word_label), ins[2], ins[3], ins[4], P(d_off)]

    def compact(ptrs, o, cat_map=0, n_out=m):
        return lib.gte_word_labels_compact(*ptrs, cat_map, 1, n, na, 13, FIGURE, n_out, *o, stream)

    co = [P(t) for t in c_outs]
    for k in range(7):
        assert compact(c_ins[:k] + [0] + c_ins[k + 1:], co) == INVALID_ARGUMENT
    for k in range(4):
        assert compact(c_ins, co[:k] + [0] + co[k + 1:]) == INVALID_ARGUMENT
    assert compact(c_ins, [co[0] + 4] + co[1:]) == INVALID_ARGUMENT                  # out_bbox is written 16 bytes at a time
    assert compact(c_ins, co, cat_map=P(d_off) + 2) == INVALID_ARGUMENT
    assert compact(c_ins, co, n_out=-1) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    for t in c_outs:
        assert (t == SENTINEL).all()
    assert compact(c_ins, co) == 0                                                   # and the same call with nothing wrong
    torch.cuda.synchronize()
    assert int(c_outs[3][0]) == 0 and (c_outs[2][:m] != SENTINEL).all() and (c_outs[2][m:] == SENTINEL).all()


def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(9)
    pages = []
    for n in (700, 1500, 3):
        ann = [[float(x), float(y), float(x + w), float(y + h), int(c)] for x, y, w, h, c in
               zip(rng.integers(0, 1500, 40), rng.integers(0, 2000, 40), rng.integers(50, 600, 40), rng.integers(50, 600, 40),
                   rng.integers(0, 13, 40))]
        pages.append((_words(rng, n), ann))
    arrays = _pack(pages)
    runs = []
    for _ in range(2):
        code, word_label, word_ann, counts, d = _label(arrays)
        assert code == 0
        off = np.concatenate([[0], np.cumsum(counts.cpu().numpy().sum(1))])
        out = _compact(arrays, d, word_label, off, int(off[-1]), ref.CAT_MAP)
        assert out[0] == 0
        runs.append([word_label.cpu().numpy(), word_ann.cpu().numpy(), counts.cpu().numpy()] + list(out[1:]))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    _assert_equal_ref(pages, cat_map=ref.CAT_MAP)
