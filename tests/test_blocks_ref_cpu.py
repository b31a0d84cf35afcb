"""tests/blocks_ref.py (the CPU reference of the block vote) against the reference's own vote statements: every case of
tests/golden/blocks_cases.json (tools/make_blocks_golden.py), exactly -- counters, labels and the word assignment."""
import json
import os

import numpy as np

from tests import blocks_ref as ref
from tests import scan_group_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blocks_cases.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_vote_page_equals_every_golden_vote_case():
    g = _golden()
    assert len(g["votes"]) >= 40 and g["scale"] == 0.36 and g["n_cat"] == 13 and g["double_cat"] == 2
    for c in g["votes"]:
        scaled = np.asarray(c["blocks"], dtype=np.float64).reshape(-1, 4) / g["scale"]
        word_block, votes, labels = ref.vote_page(c["bboxs"], c["cats"], scaled, g["n_cat"], g["double_cat"])
        assert votes == c["ref"]["counters"], c["name"]
        assert labels == c["ref"]["labels"], c["name"]
        assert word_block == c["ref"]["word_block"], c["name"]


def test_the_golden_cases_hold_what_the_rule_turns_on():
    by_name = {c["name"]: c for c in _golden()["votes"]}
    assert by_name["corner_point"]["ref"]["word_block"] == [0]                          # touching at one point counts
    assert by_name["two_blocks_lower_index"]["ref"]["word_block"] == [0, 1]        # inside blocks 0 + 1 and 1 + 2
    assert by_name["inverted_block"]["ref"]["word_block"] == [0, -1]
    assert by_name["empty_blocks"]["ref"]["labels"] == [0, 0]
    assert by_name["title_one_against_two_text"]["ref"]["labels"] == [1]                # 2 : 2, the lower category
    assert by_name["title_one_against_one_text"]["ref"]["labels"] == [2]
    assert by_name["title_one_against_two_list"]["ref"]["labels"] == [2]
    assert by_name["title_one_against_three_list"]["ref"]["labels"] == [3]
    assert by_name["tie_high_categories"]["ref"]["labels"] == [7]
    edge = by_name["edge_after_division"]
    assert edge["ref"]["word_block"][2] == -1 and edge["ref"]["word_block"][1] == 0     # one pixel short / at or past the edge


def test_vote_batch_is_vote_page_per_page_with_global_indices():
    g = _golden()
    cases = g["votes"][:12]
    bbox = np.concatenate([np.asarray(c["bboxs"], dtype=np.int32).reshape(-1, 4) for c in cases])
    cats = np.concatenate([np.asarray(c["cats"], dtype=np.int32).reshape(-1) for c in cases])
    blocks = np.concatenate([np.asarray(c["blocks"], dtype=np.float64).reshape(-1, 4) for c in cases]) / g["scale"]
    node_off = np.concatenate([[0], np.cumsum([len(c["bboxs"]) for c in cases])])
    block_off = np.concatenate([[0], np.cumsum([len(c["blocks"]) for c in cases])])
    word_block, votes, label = ref.vote_batch(bbox, node_off, cats, blocks, block_off, g["n_cat"], g["double_cat"])
    for k, c in enumerate(cases):
        want = [block_off[k] + j if j >= 0 else -1 for j in c["ref"]["word_block"]]
        assert word_block[node_off[k]:node_off[k + 1]].tolist() == want
        assert votes[block_off[k]:block_off[k + 1]].tolist() == c["ref"]["counters"]
        assert label[block_off[k]:block_off[k + 1]].tolist() == c["ref"]["labels"]


def test_nan_blocks_meet_nothing_and_out_of_range_categories_cast_no_vote():
    blocks = [[float("nan"), 0.0, 100.0, 100.0], [0.0, 0.0, 100.0, float("nan")], [0.0, 0.0, 100.0, 100.0]]
    word_block, votes, labels = ref.vote_page([[10, 10, 20, 20], [30, 30, 40, 40], [50, 50, 60, 60]], [3, -1, 13], blocks)
    assert word_block == [2, 2, 2] and votes[2] == [0, 0, 0, 1] + [0] * 9 and labels == [0, 0, 3]
    assert ref.vote_page([[10, 10, 20, 20]], [2], blocks, double_cat=-1)[1][2][2] == 1


def test_the_scan_group_pages_fill_every_block_and_leave_words_outside():
    """what the device tests on tests/scan_group_cases.py compare against is not empty: every block takes words, every page
    leaves words in no block, and with the NaN corner the last block takes none"""
    for nan_last in (False, True):
        for k, (words, cats, blocks) in enumerate(cases.scan_group_pages(nan_last)):
            n_blocks = k + 1
            assert len(blocks) == n_blocks and len(words) == cases.WORDS > 64
            word_block, votes, _ = ref.vote_page(words, cats, blocks)
            live = n_blocks - 1 if nan_last else n_blocks
            cell = cases.word_cells(k)
            assert word_block == np.where(cell < live, cell, -1).tolist()
            assert all(word_block.count(j) >= 1 and sum(votes[j]) >= 1 for j in range(live))
            assert word_block.count(-1) >= 1
            if nan_last:
                assert np.isnan(blocks[-1]).sum() == 1 and word_block.count(n_blocks - 1) == 0 and not any(votes[-1])


def test_synthetic_blocks_cover_most_words_and_leave_some_outside():
    rng = np.random.default_rng(5)
    x0, y0 = rng.integers(0, 1500, 400), rng.integers(0, 2100, 400)
    bboxs = np.stack([x0, y0, x0 + rng.integers(5, 120, 400), y0 + rng.integers(8, 30, 400)], axis=1)
    blocks = ref.synthetic_blocks(bboxs, rng)
    assert 10 < len(blocks) < 200 and all(b[0] <= b[2] and b[1] <= b[3] for b in blocks)
    word_block, _, _ = ref.vote_page(bboxs, [1] * 400, np.asarray(blocks) / 0.36)
    inside = sum(j >= 0 for j in word_block)
    assert 300 < inside < 400
    assert ref.synthetic_blocks(np.zeros((0, 4)), rng) == []
