"""tests/table_grid_ref.py pinned on literals of the rule in include/gte.h (gte_table_grid), and the host stages behind the launch
-- tables_from_grids, table_csv, tables_json, table_structure_json -- on the reference's outputs.  No device."""
import csv
import io
import json
from types import SimpleNamespace

import numpy as np
import pytest

from gnn_tableextraction_amd.components.graphs import postprocessing as PP
from tests import table_grid_ref as ref

FIVE = ([0, 31, 32, 40, 64], [31, 32, 33, 63, 96])


def _axis(lo, hi, gap=0, profile=None):
    got = ref.axis_ref(lo, hi, [True] * len(lo) if profile is None else profile, gap)
    return None if got is None else (got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4])


@pytest.mark.parametrize("gap, bands, extents", [
    (0, [0, 0, 0, 1, 2], [(0, 33), (40, 63), (64, 96)]),
    (6, [0, 0, 0, 1, 1], [(0, 33), (40, 96)]),
    (7, [0, 0, 0, 0, 0], [(0, 96)]),
])
def test_five_words_under_three_gaps(gap, bands, extents):
    b0, b1, start, end, got = _axis(*FIVE, gap=gap)
    assert b0 == bands and b1 == bands and got == extents
    assert start == [extents[b][0] for b in bands] and end == [extents[b][1] for b in bands]


def test_a_zero_width_word_occupies_one_pixel():
    b0, b1, start, end, extents = _axis([5, 5, 20], [5, 9, 20])
    assert b0 == b1 == [0, 0, 1] and extents == [(5, 9), (20, 21)] and start == [5, 5, 20] and end == [9, 9, 21]


def test_a_word_that_is_no_profile_word_spans_the_bands_it_meets():
    b0, b1, start, end, extents = _axis([0, 10, 0], [4, 14, 14], profile=[True, True, False])
    assert extents == [(0, 4), (10, 14)] and (b0[2], b1[2]) == (0, 1) and (start[2], end[2]) == (0, 14)
    # between the bands: no pixel inside is occupied; within gap pixels behind a band's last word: that band
    b0, b1, start, end, _ = _axis([0, 10, 5, 5], [4, 14, 9, 9], profile=[True, True, False, False])
    assert (b0[2], b1[2], start[2], end[2]) == (-1, -1, 0, 0)
    b0, b1, start, end, extents = _axis([0, 10, 5], [4, 14, 7], gap=2, profile=[True, True, False])
    assert extents == [(0, 4), (10, 14)] and (b0[2], b1[2], start[2], end[2]) == (0, 0, 0, 4)


def test_the_extent_limit_and_the_gap_limit():
    assert _axis([0, 8191], [1, 8192]) is not None
    assert _axis([0, 8192], [1, 8193]) is None
    assert _axis([0, 8191], [1, 8192], gap=1024)[4] == [(0, 1), (8191, 8192)]
    assert _axis([0], [1], gap=1025) is None and _axis([0], [1], gap=-1) is None
    assert _axis([-(1 << 30) - 1], [0]) is None and _axis([(1 << 30) - 1], [1 << 30]) is not None


def test_swapped_corners_equal_the_ordered_ones():
    assert _axis(FIVE[1], FIVE[0], gap=6) == _axis(*FIVE, gap=6)
    rng = np.random.default_rng(2)
    bbox = rng.integers(0, 500, (40, 4))
    swapped = bbox[:, [2, 3, 0, 1]]
    args = ([0, 40], np.zeros(40), rng.choice([7, 8, 10], 40), [0], [0], [[3, 0]], (7, 10), (7, 8, 10))
    for a, b in zip(ref.table_grid_ref(bbox, *args), ref.table_grid_ref(swapped, *args)):
        np.testing.assert_array_equal(a, b)


def test_statuses_and_untouched_rows_of_the_batch_reference():
    bbox = [[0, 0, 10, 10], [20, 0, 30, 10], [0, 0, 9000, 10], [5, 5, 6, 6], [0, 20, 10, 30]]
    table = [0, 0, 2, -1, 0]
    prefill = np.full((5, 4), 77)
    cell, cell_box, shape, box, words, status = ref.table_grid_ref(
        bbox, [0, 2, 5], table, [10, 10, 10, 10, 10], [0, 2, 0, 5, 0, -1], [0, 1, 1, 1, 2, 0], [[0, 0]] * 6, (10,), (10,), prefill, prefill)
    assert status.tolist() == [0, 2, 0, 1, 3, 1] and words.tolist() == [2, 1, 1, 0, 0, 0]
    assert shape.tolist() == [[1, 2], [0, 0], [1, 1], [0, 0], [0, 0], [0, 0]]
    assert box.tolist() == [[0, 0, 30, 10], [0, 0, 9000, 10], [0, 20, 10, 30], [0] * 4, [0] * 4, [0] * 4]
    assert cell.tolist() == [[0, 0, 0, 0], [0, 0, 1, 1], [-1] * 4, [77] * 4, [0, 0, 0, 0]]       # word 3: in no listed table
    assert cell_box.tolist() == [[0, 0, 10, 10], [20, 0, 30, 10], [0] * 4, [77] * 4, [0, 20, 10, 30]]


def test_the_reference_recovers_300_synthetic_tables():
    rng = np.random.default_rng(12)
    for k in range(300):
        tab = ref.synthetic_table(rng, int(rng.integers(1, 8)), int(rng.integers(1, 7)), header=bool(k % 3))
        n = len(tab["text"])
        cell, cell_box, shape, _, _, status = ref.table_grid_ref(tab["bbox"], [0, n], np.zeros(n), tab["role"], [0], [0],
                                                                 [[ref.auto_gap(tab["bbox"]), 0]], (7, 10), (7, 8, 10))
        assert status.tolist() == [0] and shape.tolist() == [[len(tab["rows"]), len(tab["cols"])]]
        np.testing.assert_array_equal(cell, np.stack([tab["row"], tab["row"], tab["col"], tab["col"]], axis=1))
        want = [[tab["cols"][c][0], tab["rows"][r][0], tab["cols"][c][1], tab["rows"][r][1]] for r, c in zip(tab["row"], tab["col"])]
        np.testing.assert_array_equal(cell_box, want)


# ---- the host stages on the reference's outputs: a 3 x 4 table with a spanning header cell and a two-word cell ---------------------
WORDS = [  # text, box, category
    ("Name", [10, 10, 50, 30], 7), ("Scores", [80, 10, 190, 30], 8), ("Total", [220, 10, 260, 30], 7),
    ("Ann", [10, 40, 50, 60], 10), ("1", [80, 40, 120, 60], 10), ("2", [150, 40, 190, 60], 10), ("3", [220, 40, 260, 60], 10),
    ("Bob", [10, 70, 50, 90], 10), ("4", [80, 70, 95, 90], 10), ("5", [100, 70, 120, 90], 10), ("6", [150, 70, 190, 90], 10),
    ("7", [220, 70, 260, 90], 10),
    ("outside", [400, 400, 460, 420], 1), ("caption", [10, 120, 90, 140], 6),
]
GRID = [["Name", "Scores", "", "Total"], ["Ann", "1", "2", "3"], ["Bob", "4 5", "6", "7"]]


def _page(col_roles=PP.DEFAULT_COL_ROLES):
    order = np.random.default_rng(4).permutation(len(WORDS))
    texts = [WORDS[i][0] for i in order]
    bbox = np.asarray([WORDS[i][1] for i in order], dtype=np.int32)
    role = np.asarray([WORDS[i][2] for i in order], dtype=np.int32)
    member = np.isin(role, (7, 8, 10))
    root = int(np.nonzero(member)[0][0])
    table = np.where(member, root, -1)
    gap = [[ref.auto_gap(bbox[member]), 0]]
    assert gap == [[10, 0]]
    args = (table, bbox, role, [0, len(WORDS)], [root], [0])
    grids = ref.table_grid_ref(bbox, [0, len(WORDS)], table, role, [root], [0], gap, col_roles, PP.DEFAULT_ROW_ROLES)
    pages = PP.tables_from_grids(*args, grids, [texts], col_roles, PP.DEFAULT_ROW_ROLES)
    return pages, texts, bbox


def test_tables_from_grids_gives_the_literal_grid():
    pages, texts, bbox = _page()
    assert len(pages) == 1 and len(pages[0]) == 1
    tab = pages[0][0]
    assert (tab["n_rows"], tab["n_cols"], tab["status"], tab["n_words"]) == (3, 4, 0, 12) and "score" not in tab
    assert tab["grid"] == GRID and tab["box"] == [10, 10, 260, 90] and tab["loose"] == [] and tab["header_rows"] == [0]
    assert tab["rows"] == [[10, 30], [40, 60], [70, 90]] and tab["cols"] == [[10, 50], [80, 120], [150, 190], [220, 260]]
    assert [(c["row"], c["col"]) for c in tab["cells"]] == [([0, 0], [0, 0]), ([0, 0], [1, 2]), ([0, 0], [3, 3])] + \
        [([r, r], [c, c]) for r in (1, 2) for c in range(4)]
    span = tab["cells"][1]
    assert span["text"] == "Scores" and span["role"] == 8 and span["box"] == [80, 10, 190, 30] and span["col"] == [1, 2]
    two = next(c for c in tab["cells"] if c["text"] == "4 5")
    assert [texts[i] for i in two["words"]] == ["4", "5"] and two["box"] == [80, 70, 120, 90] and two["role"] == 10
    assert all(c["role"] == 7 for c in tab["cells"] if c["text"] in ("Name", "Total"))
    assert sorted(i for c in tab["cells"] for i in c["words"]) == sorted(i for i, t in enumerate(texts) if t not in ("outside", "caption"))
    json.dumps(tab)                                       # ints, floats, strings and lists only


def test_a_spanning_cell_in_the_column_profile_merges_its_columns():
    tab = _page(col_roles=(7, 8, 10))[0][0][0]
    assert (tab["n_rows"], tab["n_cols"]) == (3, 3) and tab["cols"] == [[10, 50], [80, 190], [220, 260]]
    assert tab["grid"] == [["Name", "Scores", "Total"], ["Ann", "1 2", "3"], ["Bob", "4 5 6", "7"]]


def test_writers_and_documents():
    pages, _, _ = _page()
    tab = pages[0][0]
    text = PP.table_csv(tab)
    assert text == "Name,Scores,,Total\r\nAnn,1,2,3\r\nBob,4 5,6,7\r\n" and list(csv.reader(io.StringIO(text))) == GRID
    assert PP.table_csv(dict(tab, grid=[['a,b', 'say "hi"']])) == '"a,b","say ""hi"""\r\n'
    data = SimpleNamespace(pages=[{"page": "p7"}])
    assert PP.tables_json(data, pages) == {"p7": [tab]} and json.loads(json.dumps(PP.tables_json(data, pages))) == {"p7": [tab]}
    doc = PP.table_structure_json(data, pages)
    assert list(doc) == ["table", "table-row", "table-col"]
    assert doc["table"] == {"p7": {"bboxes": [[10, 10, 260, 90]], "scores": [1.0]}}
    assert doc["table-row"] == {"p7": {"bboxes": [[10, 10, 260, 30], [10, 40, 260, 60], [10, 70, 260, 90]], "scores": [1.0] * 3}}
    assert doc["table-col"]["p7"]["bboxes"] == [[10, 10, 50, 90], [80, 10, 120, 90], [150, 10, 190, 90], [220, 10, 260, 90]]
    scored = PP.table_structure_json(data, [[dict(tab, score=0.25)]])
    assert scored["table-col"]["p7"]["scores"] == [0.25] * 4 and scored["table"]["p7"]["scores"] == [0.25]
    assert PP.table_structure_json(data, [[]]) == {"table": {}, "table-row": {}, "table-col": {}}


def test_a_table_without_a_grid_keeps_its_words_loose_and_scores_travel():
    bbox = [[0, 0, 9000, 10], [0, 20, 10, 30]]
    args = ([0, 0], bbox, [10, 10], [0, 2], [0], [0])
    grids = ref.table_grid_ref(bbox, [0, 2], [0, 0], [10, 10], [0], [0], [[0, 0]], (10,), (10,))
    tab = PP.tables_from_grids(*args, grids, None, (10,), (10,), score=[0.5])[0][0]
    assert tab["status"] == 2 and tab["loose"] == [0, 1] and tab["cells"] == [] and tab["grid"] == [] and tab["rows"] == []
    assert tab["score"] == 0.5 and PP.table_csv(tab) == ""
    assert PP.role_mask((7, 10)) == (1 << 7) | (1 << 10) and PP.role_mask(5) == 5
    with pytest.raises(ValueError, match="0 .. 31"):
        PP.role_mask((7, 32))


def test_table_batch_is_torch_plumbing_that_runs_on_host_tensors():
    import torch
    rng = np.random.default_rng(8)
    pages = [ref.synthetic_page(rng, 3, 2), ref.synthetic_page(rng, 1, 1), ref.synthetic_page(rng, 2, 4)]
    off = np.concatenate([[0], np.cumsum([len(p["text"]) for p in pages])])
    member = np.concatenate([p["member"] for p in pages])
    first = np.asarray([off[k] + np.nonzero(p["member"])[0][0] for k, p in enumerate(pages)])
    text_root = np.asarray([off[k] + np.nonzero(~p["member"])[0][0] for k, p in enumerate(pages)])
    comp = np.where(member, np.repeat(first, np.diff(off)), np.repeat(text_root, np.diff(off)))
    root = np.sort(np.concatenate([first, text_root]))
    is_table = np.isin(root, first)
    n_words = np.asarray([(comp == r).sum() for r in root])
    t = torch.from_numpy
    reg = PP.PageRegions(t(comp.astype(np.int32)), t(root), t(np.searchsorted(off[1:], root, side="right")),
                         t(np.where(is_table, 4, 1).astype(np.int32)), torch.zeros((6, 4), dtype=torch.int32), t(n_words.astype(np.int32)),
                         t(np.linspace(0.1, 0.6, 6).astype(np.float32)))
    bbox, role = t(np.concatenate([p["bbox"] for p in pages])), t(np.concatenate([p["role"] for p in pages]))
    tb = PP.table_batch(reg, bbox, role, off)
    assert tb.root.tolist() == first.tolist() and tb.page.tolist() == [0, 1, 2] and tb.root.dtype == tb.page.dtype == tb.gap.dtype == torch.int32
    np.testing.assert_array_equal(tb.table.numpy(), np.where(member, comp, -1))
    assert tb.gap.tolist() == [[ref.auto_gap(p["bbox"][p["member"]]), 0] for p in pages]
    np.testing.assert_array_equal(tb.score.numpy(), reg.score.numpy()[is_table])
    small = PP.table_batch(reg, bbox, role, off, col_gap=4, row_gap=2, min_words=5)     # the 1 x 1 table has at most 3 words
    assert small.root.tolist() == first[[0, 2]].tolist() and small.gap.tolist() == [[4, 2], [4, 2]]
    assert (small.table.numpy()[off[1]:off[2]] == -1).all()
    with pytest.raises(ValueError, match="table_batch"):
        PP.table_batch(reg, bbox, role, off[:-1])
