"""CPU-only: tests/blockscore_ref.py on a hand case whose answer is worked out below, the mutants of its rules that the hand case
must catch, and the vectorised form against the plain one."""
import numpy as np
import pytest

from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from tests import blockscore_ref as ref

LN = np.log
# classes: 0 other, 1 text, 2 title, ... 6 column header, 7 spanning cell, 8 table cell (DEFAULT_CLASS_CATEGORY)
MASKS = PP.category_class_masks()
# blocks (word coordinates): a TABLE, a TEXT block that overlaps it, a FIGURE nothing meets, a block with a NaN corner
BLOCKS = [[0.0, 0.0, 100.0, 100.0], [50.0, 50.0, 200.0, 200.0], [500.0, 500.0, 600.0, 600.0], [0.0, float("nan"), 300.0, 300.0]]
CATS = [4, 1, 5, 1]
WORDS = [[10, 10, 20, 20],          # in the table only
         [60, 60, 70, 70],          # in the table AND the text block
         [100, 10, 120, 20],        # touches the table's right edge
         [150, 150, 160, 160],      # in the text block only
         [55, 55, 65, 65],          # in both, a NaN logit
         [300, 300, 310, 310]]      # in none


def _row(probs):
    """a logit row whose softmax is ``probs``"""
    return LN(np.asarray(probs, dtype=np.float64))


LOGITS = np.stack([_row([.1, .1, .025, .025, .025, .025, .4, .1, .2]),                   # table mass .7
                   _row([.1, .5, .025, .025, .025, .025, .1, .1, .1]),                   # table mass .3, text mass .5
                   _row([.2, .2, .025, .025, .025, .025, .3, .1, .1]),                   # table mass .5
                   _row([.1, .8, .0125, .0125, .0125, .0125, .0125, .0125, .025]),       # text mass .8
                   _row([.1, .1, .025, .025, .025, .025, .4, .1, .2]),
                   _row([1 / 9] * 9)])
LOGITS[4, 3] = np.nan
WANT_SCORE = [(.7 + .3 + .5 + 0.0) / 4, (.5 + .8 + 0.0) / 3, 1.0, 1.0]
WANT_WORDS = [4, 3, 0, 0]


def _hand(rule=ref.Rule(), masks=MASKS):
    return ref.score_page(WORDS, LOGITS, BLOCKS, CATS, masks, rule)


def test_the_hand_case():
    score, n_words = _hand()
    assert n_words == WANT_WORDS
    np.testing.assert_allclose(score, WANT_SCORE, rtol=0, atol=1e-12)
    batch = ref.block_scores_ref(WORDS, [0, len(WORDS)], LOGITS, BLOCKS, [0, len(BLOCKS)], CATS, MASKS)
    assert batch[1].tolist() == WANT_WORDS and batch[0].tolist() == score


def test_the_class_masks():
    assert MASKS.dtype == np.uint32 and MASKS.shape == (13,)
    want = {0: 1 << 0, 1: 1 << 1, 2: 1 << 2, 3: 1 << 3, 5: 1 << 4, 6: 1 << 5, 7: 1 << 6, 8: 1 << 7, 10: 1 << 8,
            4: (1 << 6) | (1 << 7) | (1 << 8)}
    assert {k: int(m) for k, m in enumerate(MASKS) if m} == want
    assert PP.category_class_masks([1, 1, 4, 10], n_cat=16).tolist() == [0, 3, 0, 0, 12, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0]
    assert ref.word_mass([0.0, 0.0], 0) == 0.0 and ref.word_mass([0.0, 0.0], 3) == 1.0 and ref.word_mass([0.0, np.inf], 3) == 0.0


MUTANTS = {
    "first_block_only": dict(rule=ref.Rule(every_block=False)),
    "open_rectangle_test": dict(rule=ref.Rule(closed=False)),
    "non_finite_rows_left_out": dict(rule=ref.Rule(count_non_finite=False)),
    "table_mask_without_the_header_classes": dict(masks=np.where(np.arange(13) == 4, np.uint32(1 << 8), MASKS)),
    "zero_for_a_block_without_words": dict(rule=ref.Rule(empty_score=0.0)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_fails_the_hand_case(name):
    score, n_words = _hand(**MUTANTS[name])
    assert n_words != WANT_WORDS or float(np.abs(np.asarray(score) - np.asarray(WANT_SCORE)).max()) > 2.0 ** -18, name


def test_the_vectorised_form_equals_the_plain_one():
    rng = np.random.default_rng(3)
    sizes, n_blocks = [0, 1, 40, 25], [3, 0, 6, 5]
    node_off, block_off = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(n_blocks)])
    n, nb = int(node_off[-1]), int(block_off[-1])
    x0, y0 = rng.integers(0, 300, n), rng.integers(0, 300, n)
    bbox = np.stack([x0, y0, x0 + rng.integers(0, 40, n), y0 + rng.integers(0, 15, n)], axis=1)
    bbox[5] = bbox[5][[2, 3, 0, 1]]                                                       # corners the other way round
    bx, by = rng.integers(0, 250, nb).astype(np.float64), rng.integers(0, 250, nb).astype(np.float64)
    blocks = np.stack([bx, by, bx + rng.integers(20, 150, nb), by + rng.integers(20, 150, nb)], axis=1) / 0.36 * 0.36
    blocks[4] = blocks[4][[2, 1, 0, 3]]
    blocks[7, 2] = np.nan
    cats = rng.integers(-1, 15, nb)
    logits = 3.0 * rng.standard_normal((n, 9))
    logits[3, 2], logits[50, 0] = np.inf, np.nan
    a = ref.block_scores_ref(bbox, node_off, logits, blocks, block_off, cats, MASKS)
    b = ref.block_scores_fast(bbox, node_off, logits, blocks, block_off, cats, MASKS)
    assert a[1].tolist() == b[1].tolist() and a[1].max() >= 4 and (a[1] == 0).any()
    np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-14)
