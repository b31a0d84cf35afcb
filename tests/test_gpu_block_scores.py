"""Block confidences on the device (gte_block_scores, postprocessing.block_scores) against tests/blockscore_ref.py.  n_words is
an integer and compared exactly.

The score bound is derived, not measured -- it is the one of tests/test_gpu_region_scores.py, for the same per-word function
(csrc/word_score.h): a word's q is p * 2^19 rounded (<= 2^-20), p comes from an fp32 max-subtracted softmax (expf and at most 16
additions: far below 2^-19), the mean of exact integers is one fp64 division and one rounding to fp32 (<= 2^-25 at a score
<= 1) -- in all below 2^-18."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from tests import blockscore_ref as ref
from tests import scan_group_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
SCORE_SENTINEL = 12345.0
BOUND = 2.0 ** -18


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def _abi(bbox, node_off, logits, block_box, block_off, block_cat, masks, max_words=None, max_blocks=None, expect=0):
    """One direct call of gte_block_scores on sentinel-prefilled outputs -> (score [B], n_words [B]) as numpy arrays."""
    lib, P = _lib.load(), _lib.ptr
    logits = np.asarray(logits, dtype=np.float32)
    d_bbox, d_no, d_logits = _t(np.asarray(bbox).reshape(-1, 4), np.int32), _t(node_off, np.int32), _t(logits, np.float32)
    d_box, d_bo, d_cat = _t(np.asarray(block_box).reshape(-1, 4), np.float64), _t(block_off, np.int32), _t(block_cat, np.int32)
    d_masks = _t(np.asarray(masks, dtype=np.uint32).view(np.int32), np.int32)
    nb = len(block_cat)
    score = torch.full((max(nb, 1),), SCORE_SENTINEL, dtype=torch.float32, device=DEV)
    n_words = torch.full((max(nb, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    sizes, blocks = np.diff(np.asarray(node_off)), np.diff(np.asarray(block_off))
    rc = lib.gte_block_scores(P(d_bbox), P(d_no), P(d_logits), logits.shape[1], logits.shape[1], P(d_box), P(d_bo), P(d_cat), P(d_masks),
                              len(masks), len(sizes), len(d_bbox), nb, int(sizes.max()) if max_words is None else max_words,
                              int(blocks.max()) if max_blocks is None else max_blocks, P(score), P(n_words), _lib.current_stream())
    assert rc == expect, lib.gte_last_error()
    torch.cuda.synchronize()
    return score.cpu().numpy()[:nb], n_words.cpu().numpy()[:nb]


def _words(rng, n, extent=2000):
    x0, y0 = rng.integers(0, extent, n), rng.integers(0, extent, n)
    return np.stack([x0, y0, x0 + rng.integers(1, 120, n), y0 + rng.integers(1, 40, n)], axis=1).astype(np.int32)


def _blocks(rng, n, extent=2000, size=(200, 900)):
    """layout blocks as the route packs them: PDF points / 0.36, free to overlap"""
    x0, y0 = rng.integers(0, extent, n), rng.integers(0, extent, n)
    pts = np.stack([x0, y0, x0 + rng.integers(*size, n), y0 + rng.integers(*size, n)], axis=1).astype(np.float64) * 0.36
    return pts / 0.36


def _masks(rng, n_classes, n_cat=13):
    m = rng.integers(0, 1 << n_classes, n_cat).astype(np.uint32)
    m[0], m[1] = (1 << n_classes) - 1, 0                   # every class / no class
    return m


@pytest.fixture(scope="module")
def pages():
    """(words, blocks) per page: (0, 5), (1, 0), (1023, 1), (1024, 4), (1025, 512), (300, 37) -- no word, one word, below / at /
    above one pass of the strided loop; no block, one block, a whole scan group, a group and one, the limit; two ordinary pages
    of different counts.  Some corners are the other way round, one block has a NaN corner, some categories lie outside the
    mask table."""
    rng = np.random.default_rng(17)
    sizes, counts = [0, 1, 1023, 1024, 1025, 300], [5, 0, 1, 4, 512, 37]
    node_off, block_off = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(counts)])
    n, nb = int(node_off[-1]), int(block_off[-1])
    bbox, blocks = _words(rng, n), _blocks(rng, nb)
    blocks[5] = [0.0, 0.0, 2200.0, 2200.0]                 # page 2's one block takes all of its words
    flip = rng.random(n) < 0.05
    bbox[flip] = bbox[flip][:, [2, 3, 0, 1]]
    blocks[12] = blocks[12][[2, 1, 0, 3]]
    blocks[20, 1] = np.nan
    cats = rng.integers(0, 13, nb).astype(np.int32)
    cats[rng.random(nb) < 0.03] = 13
    cats[15] = -1
    return dict(node_off=node_off, block_off=block_off, bbox=bbox, blocks=blocks, cats=cats, n=n, nb=nb)


@pytest.mark.parametrize("n_classes", [1, 9, 16])
def test_scores_over_page_sizes_block_counts_and_class_counts(pages, n_classes):
    """The bound 2^-18 is the derived one of this module's docstring; the measured maximum is printed."""
    g = pages
    rng = np.random.default_rng(200 + n_classes)
    masks = _masks(rng, n_classes)
    logits = (4.0 * rng.standard_normal((g["n"], n_classes))).astype(np.float32)
    bad = rng.choice(g["n"], 40, replace=False)
    logits[bad[:20], rng.integers(0, n_classes, 20)] = np.nan
    logits[bad[20:], rng.integers(0, n_classes, 20)] = np.inf
    args = (g["bbox"], g["node_off"], logits, g["blocks"], g["block_off"], g["cats"], masks)
    score, n_words = _abi(*args)
    want, want_words = ref.block_scores_fast(*args)
    np.testing.assert_array_equal(n_words, want_words)
    err = float(np.abs(score.astype(np.float64) - want).max())
    print(f"n_classes={n_classes}: max |score - ref| = {err:.3e} = {err * 2 ** 19:.3f} units of 2^-19; words per block up to {n_words.max()}")
    assert err <= BOUND
    assert score.dtype == np.float32 and (score >= 0).all() and (score <= 1).all()
    assert n_words[5] == 1023 and n_words[20] == 0 and score[20] == 1.0                   # the block of all words; the NaN corner
    assert (n_words[:5] == 0).all() and (score[:5] == 1.0).all()                          # the page without words
    assert (n_words > 1).sum() > 300 and (n_words == 0).sum() > 5
    if n_classes > 1:
        for outside in (1, 13, -1):                                                        # the empty mask, categories outside the table
            assert (score[(g["cats"] == outside) & (n_words > 0)] == 0.0).all()
        assert len(set(score.tolist())) > 300
    again = _abi(*args)
    assert score.tobytes() == again[0].tobytes() and n_words.tobytes() == again[1].tobytes()
    # the plain definition on the small pages (the vectorised reference is compared with it on the CPU)
    small = slice(int(g["node_off"][5]), int(g["node_off"][6])), slice(int(g["block_off"][5]), int(g["block_off"][6]))
    s, c = ref.score_page(g["bbox"][small[0]], logits[small[0]], g["blocks"][small[1]], g["cats"][small[1]], masks)
    assert c == n_words[small[1]].tolist() and np.abs(np.asarray(s) - score[small[1]]).max() <= BOUND


def test_block_counts_around_a_scan_group():
    """tests/scan_group_cases.py: 9 pages of 1 .. 9 blocks, without and with a NaN corner in every page's last block; 9 classes,
    seeded normal logits.  The bound 2^-18 is the derived one of this module's docstring; the measured maximum is printed."""
    rng = np.random.default_rng(31)
    masks = PP.category_class_masks()
    for nan_last in (False, True):
        pages = cases.scan_group_pages(nan_last)
        bbox, blocks = np.concatenate([w for w, _, _ in pages]), np.concatenate([b for _, _, b in pages])
        node_off = np.concatenate([[0], np.cumsum([len(w) for w, _, _ in pages])])
        block_off = np.concatenate([[0], np.cumsum([len(b) for _, _, b in pages])])
        cats = (np.arange(len(blocks)) % 13).astype(np.int32)
        logits = rng.standard_normal((len(bbox), 9)).astype(np.float32)
        args = (bbox, node_off, logits, blocks, block_off, cats, masks)
        score, n_words = _abi(*args)
        want, want_words = ref.block_scores_fast(*args)
        np.testing.assert_array_equal(n_words, want_words)
        err = float(np.abs(score.astype(np.float64) - want).max())
        print(f"nan_last={nan_last}: max |score - ref| = {err:.3e} = {err * 2 ** 19:.3f} units of 2^-19")
        assert err <= BOUND
        last = block_off[1:] - 1
        assert (np.delete(n_words, last) >= 7).all() and ((n_words[last] == 0).all() if nan_last else (n_words[last] >= 7).all())


def test_a_full_page_in_one_block_of_every_class_scores_exactly_one():
    """4096 words that all meet one block whose mask holds every class: p = 1 for every word, the fixed-point sum is 2^31 -- the
    case that needs all 32 bits of the accumulator."""
    n = _lib.load().gte_block_scores_max_page_words()
    assert n == 4096
    rng = np.random.default_rng(2)
    bbox = _words(rng, n)
    for n_classes in (1, 9):
        logits = (5.0 * rng.standard_normal((n, n_classes))).astype(np.float32)
        score, n_words = _abi(bbox, [0, n], logits, [[0.0, 0.0, 3000.0, 3000.0], [-50.0, -50.0, -10.0, -10.0]], [0, 2], [3, 3],
                              [0, 0, 0, (1 << n_classes) - 1])
        assert n_words.tolist() == [n, 0] and score[0] == np.float32(1.0) and score[1] == np.float32(1.0)


def test_a_page_above_the_limits_is_refused_before_any_launch():
    lib = _lib.load()
    rng = np.random.default_rng(4)
    n = lib.gte_block_scores_max_page_words() + 1
    score, n_words = _abi(_words(rng, n), [0, n], np.zeros((n, 2)), _blocks(rng, 3), [0, 3], [0, 0, 0], [3], expect=-4)
    assert b"4097 words exceeds" in lib.gte_last_error()
    assert (score == SCORE_SENTINEL).all() and (n_words == SENTINEL).all()
    nb = lib.gte_block_scores_max_page_blocks() + 1
    score, n_words = _abi(_words(rng, 10), [0, 10], np.zeros((10, 2)), _blocks(rng, nb), [0, nb], [0] * nb, [3], expect=-4)
    assert b"513 blocks exceeds" in lib.gte_last_error()
    assert (score == SCORE_SENTINEL).all() and (n_words == SENTINEL).all()
    t = lambda a, d: torch.from_numpy(np.asarray(a, dtype=d)).to(DEV)
    with pytest.raises(_lib.GteError, match="exceeds"):
        PP.block_scores(t(_words(rng, 10), np.int32), [0, 10], t(np.zeros((10, 2)), np.float32), t(_blocks(rng, nb), np.float64), [0, nb],
                        t([0] * nb, np.int32), [3])


def test_the_hand_page_a_word_in_three_blocks_a_word_in_none_a_nan_corner_and_a_non_finite_row():
    blocks = [[0.0, 0.0, 100.0, 100.0], [50.0, 50.0, 200.0, 200.0], [40.0, 40.0, 70.0, 70.0], [500.0, 500.0, 600.0, 600.0],
              [0.0, float("nan"), 300.0, 300.0]]
    cats = [4, 1, 2, 5, 1]
    words = [[10, 10, 20, 20], [60, 60, 65, 65], [100, 10, 120, 20], [150, 150, 160, 160], [55, 55, 65, 65], [300, 300, 310, 310]]
    row = lambda p: np.log(np.asarray(p, dtype=np.float64))
    logits = np.stack([row([.1, .1, .025, .025, .025, .025, .4, .1, .2]), row([.1, .5, .125, .025, .025, .025, .05, .05, .1]),
                       row([.2, .2, .025, .025, .025, .025, .3, .1, .1]), row([.1, .8, .0125, .0125, .0125, .0125, .0125, .0125, .025]),
                       row([.1, .1, .025, .025, .025, .025, .4, .1, .2]), row([1 / 9] * 9)])
    logits[4, 3] = np.nan
    score, n_words = _abi(words, [0, 6], logits, blocks, [0, 5], cats, PP.category_class_masks())
    assert n_words.tolist() == [4, 3, 2, 0, 0]                                            # word 1 in three blocks, word 5 in none
    want = [(.7 + .2 + .5 + 0.0) / 4, (.5 + .8 + 0.0) / 3, (.125 + 0.0) / 2, 1.0, 1.0]
    assert np.abs(score.astype(np.float64) - np.asarray(want)).max() <= BOUND
    assert score[3] == 1.0 and score[4] == 1.0
    ref_score, ref_words = ref.score_page(words, logits, blocks, cats, PP.category_class_masks())
    assert ref_words == n_words.tolist() and np.abs(score - np.asarray(ref_score)).max() <= BOUND


def test_a_page_above_the_stated_maxima_takes_no_score_and_bad_offsets_write_nothing():
    rng = np.random.default_rng(6)
    bbox, logits = _words(rng, 60, extent=300), rng.standard_normal((60, 3))
    blocks, cats = _blocks(rng, 12, extent=300, size=(50, 200)), [0] * 12
    node_off, block_off = [0, 20, 30, 60], [0, 3, 9, 12]
    full = _abi(bbox, node_off, logits, blocks, block_off, cats, [7, 1])
    score, n_words = _abi(bbox, node_off, logits, blocks, block_off, cats, [7, 1], max_blocks=4)       # page 1 has 6 blocks
    assert n_words[3:9].tolist() == [-1] * 6 and not score[3:9].any()
    assert np.array_equal(n_words[:3], full[1][:3]) and np.array_equal(score[9:], full[0][9:]) and full[1].max() > 3
    score, n_words = _abi(bbox, node_off, logits, blocks, block_off, cats, [7, 1], max_words=25)        # page 2 has 30 words
    assert n_words[9:].tolist() == [-1] * 3 and not score[9:].any() and np.array_equal(n_words[:9], full[1][:9])
    score, n_words = _abi(bbox, [0, 20, 70, 60], logits, blocks, block_off, cats, [7, 1], max_words=50)  # page 1 names words past the end
    assert (n_words[3:9] == SENTINEL).all() and (score[3:9] == SCORE_SENTINEL).all() and np.array_equal(n_words[:3], full[1][:3])


def test_the_wrapper_equals_the_reference_takes_a_row_stride_and_checks_its_arguments():
    rng = np.random.default_rng(9)
    sizes, counts = [40, 0, 200], [6, 2, 30]
    node_off, block_off = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(counts)])
    bbox, blocks = _words(rng, 240, extent=600), _blocks(rng, 38, extent=600, size=(100, 400))
    cats = rng.integers(0, 13, 38).astype(np.int32)
    wide = (3.0 * rng.standard_normal((240, 12))).astype(np.float32)
    masks = PP.category_class_masks()
    t = lambda a: torch.from_numpy(a).to(DEV)
    got = PP.block_scores(t(bbox), node_off, t(wide)[:, :9], t(blocks), block_off, t(cats), masks)          # a view: row stride 12
    assert isinstance(got, PP.BlockScores) and got.score.dtype == torch.float32 and got.n_words.dtype == torch.int32 and got.score.is_cuda
    want, want_words = ref.block_scores_fast(bbox, node_off, wide[:, :9], blocks, block_off, cats, masks)
    np.testing.assert_array_equal(got.n_words.cpu().numpy(), want_words)
    assert np.abs(got.score.cpu().numpy() - want).max() <= BOUND and want_words.max() > 10
    packed = PP.block_scores(t(bbox), node_off, t(np.ascontiguousarray(wide[:, :9])), t(blocks), block_off, t(cats), masks)
    assert torch.equal(packed.score, got.score) and torch.equal(packed.n_words, got.n_words)
    with pytest.raises(ValueError, match="float64"):
        PP.block_scores(t(bbox), node_off, t(wide), t(blocks.astype(np.float32)), block_off, t(cats), masks)
    with pytest.raises(ValueError, match="int32"):
        PP.block_scores(t(bbox.astype(np.int64)), node_off, t(wide), t(blocks), block_off, t(cats), masks)
    with pytest.raises(ValueError, match="logits"):
        PP.block_scores(t(bbox), node_off, t(wide[:-1]), t(blocks), block_off, t(cats), masks)
    with pytest.raises(ValueError, match="do not partition"):
        PP.block_scores(t(bbox), node_off[:-1], t(wide), t(blocks), block_off[:-1], t(cats), masks)
    with pytest.raises(ValueError, match="classes outside"):
        PP.block_scores(t(bbox), node_off, t(np.zeros((240, 17), dtype=np.float32)), t(blocks), block_off, t(cats), masks)
    with pytest.raises(ValueError, match="class masks outside"):
        PP.block_scores(t(bbox), node_off, t(wide), t(blocks), block_off, t(cats), [1] * 17)
