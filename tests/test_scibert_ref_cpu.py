"""tests/scibert_ref.py (the numpy oracle of gte_token_pool_f32 and of the host mask rule) against the reference's recorded batches
and outputs (tests/golden/scibert_cases.json, written by tools/make_scibert_golden.py): ids and masks equal, the max output equal by
value, the mean output within the gap that two float32 summation orders of c terms plus the final rounding can open -- torch's
reduction order is not defined."""
import numpy as np
import pytest

from tests import scibert_ref as ref

DATA = ref.golden()
PAGES = DATA["pages"]
IDS = {t: i for i, t in enumerate(DATA["vocab"])}
CLS, SEP, PAD = IDS["[CLS]"], IDS["[SEP]"], IDS["[PAD]"]
WIDTH = DATA["max_length"] - 1


def page_tok(page):
    return ref.page_ids(page["pieces"], CLS, SEP, PAD, WIDTH)


def test_the_fixture_holds_the_kinds_of_page_the_rule_depends_on():
    names = {p["name"] for p in PAGES}
    assert {"mixed_lengths", "equal_lengths", "only_empty", "one_word", "special_tokens", "over_14_pieces", "over_100_characters"} <= names
    assert len(DATA["vocab"]) == DATA["embeddings"].shape[0] == DATA["normalized"].shape[0]
    norms = np.sqrt((DATA["normalized"].astype(np.float64) ** 2).sum(axis=1))
    assert np.all(np.abs(norms - 1) < 1e-6)
    unk = sum(p == [IDS["[UNK]"]] for page in PAGES for p in page["pieces"])
    assert unk < sum(len(page["words"]) for page in PAGES) / 2           # the recorded tokenizer did tokenise


@pytest.mark.parametrize("page", PAGES, ids=[p["name"] for p in PAGES])
def test_rows_and_masks_equal_the_recorded_batch(page):
    ids, mask = ref.page_rows(page["pieces"], CLS, SEP, PAD)
    np.testing.assert_array_equal(ids, np.asarray(page["input_ids"]))
    np.testing.assert_array_equal(mask, np.asarray(page["mask"]))
    assert all(len(p) <= DATA["max_length"] - 2 for p in page["pieces"])
    tok = page_tok(page)
    want = np.where(np.asarray(page["mask"]) == 1, np.asarray(page["input_ids"]), -1)[:, 1:]
    np.testing.assert_array_equal(tok[:, :want.shape[1]], want)
    assert (tok[:, want.shape[1]:] == -1).all() and tok.shape == (len(page["words"]), WIDTH)


@pytest.mark.parametrize("page", PAGES, ids=[p["name"] for p in PAGES])
def test_pooled_outputs_against_the_recorded_ones(page):
    tok = page_tok(page)
    np.testing.assert_array_equal(ref.pool(tok, DATA["normalized"], "max"), page["max"])
    mean = ref.pool(tok, DATA["normalized"], "mean")
    bound = ref.mean_bound(tok, DATA["normalized"], page["mean"])
    err = np.abs(mean.astype(np.float64) - page["mean"])
    assert np.all(err <= bound), (float(err.max()), float((err - bound).max()))
    none = ~((tok >= 0).any(axis=1))
    assert not mean[none].any() and not page["mean"][none].any()         # 0 / 1e-9 there, 0 here


def test_the_page_dependent_sep_rule_on_the_recorded_pages():
    by_name = {p["name"]: p for p in PAGES}
    equal = page_tok(by_name["equal_lengths"])
    assert ((equal >= 0).sum(axis=1) == 1).all() and SEP not in equal   # no [SEP] is pooled
    mixed = page_tok(by_name["mixed_lengths"])
    counts = (mixed >= 0).sum(axis=1)
    longest = max(len(p) for p in by_name["mixed_lengths"]["pieces"])
    for row, c, p in zip(mixed, counts, by_name["mixed_lengths"]["pieces"]):
        assert c == (len(p) if len(p) == longest else len(p) + 1) and (row[len(p)] == SEP) == (len(p) < longest)
    assert (page_tok(by_name["only_empty"]) == -1).all()
    assert not by_name["only_empty"]["mean"].any() and not by_name["only_empty"]["max"].any()
    beside = page_tok(by_name["empty_beside_longer"])
    assert beside[0].tolist() == [SEP] + [-1] * (WIDTH - 1)             # an empty word beside longer ones pools [SEP] alone
    assert (page_tok(by_name["all_truncated"]) >= 0).sum(axis=1).tolist() == [14, 14]


def test_pool_skips_what_names_no_row_and_keeps_position_order():
    table = np.array([[1e8, -1.0], [1.0, -2.0], [-1e8, 0.5]], dtype=np.float32)
    tok = np.array([[0, 1, 2], [2, 0, 1], [-1, 3, 7], [1, -1, 1]])
    mean = ref.pool(tok, table, "mean")
    # (1e8 + 1) - 1e8 = 0 in float32, (-1e8 + 1e8) + 1 = 1: the order of the positions is the order of the adds
    assert mean[0, 0] == 0 and mean[1, 0] == np.float32(1) / np.float32(3)
    assert not mean[2].any() and mean[3].tolist() == [1.0, -2.0]
    assert ref.pool(tok, table, "max").tolist() == [[1e8, 0.5], [1e8, 0.5], [0, 0], [1, 0]]
