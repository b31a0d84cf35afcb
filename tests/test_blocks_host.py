"""The host side of the block route (postprocessing.assemble_tables, blocks_json, extract_blocks' argument checks) against the
reference's own get_tables_bbox on the pages of tests/golden/blocks_cases.json (tools/make_blocks_golden.py).  No GPU."""
import copy
import json
import os
from types import SimpleNamespace

import pytest

from gnn_tableextraction_amd.components.graphs import postprocessing as PP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blocks_cases.json")
TABLE, COLH, SP, TCELL = 4, 7, 8, 10


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_assemble_tables_equals_the_reference_on_every_golden_page_and_leaves_its_inputs_alone(golden):
    assert len(golden["assembly"]) >= 60
    tables = headers = 0
    for i, c in enumerate(golden["assembly"]):
        blocks, labels = copy.deepcopy(c["blocks"]), list(c["labels"])
        got_blocks, got_labels, got_headers = PP.assemble_tables(blocks, labels)
        assert got_blocks == c["ref"]["blocks"], i
        assert got_labels == c["ref"]["labels"], i
        assert got_headers == c["ref"]["headers"], i
        assert blocks == c["blocks"] and labels == c["labels"], i
        assert TCELL not in got_labels and all(b in got_headers for b, l in zip(got_blocks, got_labels) if l in (COLH, SP))
        tables += got_labels.count(TABLE)
        headers += len(got_headers)
    assert tables > 60 and headers > 60


def test_assemble_tables_takes_tuples_and_pages_without_table_blocks():
    blocks = ((10.0, 10.0, 200.0, 40.0), (10.0, 50.0, 200.0, 90.0))
    assert PP.assemble_tables(blocks, (1, 2)) == ([blocks[0], blocks[1]], [1, 2], [])
    assert PP.assemble_tables([], []) == ([], [], [])
    # one header above one cell block in one column: a table, the hull of the two; the paragraph it overlaps is absorbed
    page = [[10.0, 10.0, 100.0, 20.0], [12.0, 24.0, 98.0, 34.0], [50.0, 30.0, 300.0, 60.0], [10.0, 200.0, 300.0, 260.0]]
    got = PP.assemble_tables(page, [COLH, TCELL, 1, 1])
    assert got == ([[10.0, 200.0, 300.0, 260.0], [10.0, 10.0, 300.0, 60.0]], [1, TABLE], [[10.0, 10.0, 100.0, 20.0]])


def test_default_class_category_is_the_references_revert_map(golden):
    assert golden["label_revert"]["to_remove"] == [4, 9, 11, 12]
    assert list(PP.DEFAULT_CLASS_CATEGORY) == golden["label_revert"]["revert"]
    assert len(PP.CATEGORY_NAMES) == golden["n_cat"] == 13 and len(set(PP.CATEGORY_NAMES)) == 13
    assert [PP.CATEGORY_NAMES[k] for k in PP.GROUP_NAMES] == list(PP.GROUP_NAMES.values())
    assert PP.CATEGORY_NAMES[0] == "other" and PP.CATEGORY_NAMES[TCELL] == "table-tcell" and PP.CATEGORY_NAMES[12] == "table-row"


def _data(n, blocks=True):
    pages = [{"page": f"doc_{i}.pdf", "bboxs": [[10 * i, 10, 10 * i + 5, 20]]} for i in range(n)]
    if blocks:
        for p in pages:
            p["blocks"] = [[0.0, 0.0, 50.0, 50.0]]
    return SimpleNamespace(graphs=[None] * n, pages=pages)


def test_blocks_json_has_the_thirteen_kinds_float_coordinates_and_unit_scores():
    data = _data(3)
    result = [{"blocks": [[1, 2, 3, 4], [5.5, 6.0, 7.25, 8.0], [9.0, 9.0, 10.0, 10.0]], "labels": [1, 4, 1]},
              {"blocks": [], "labels": []},
              {"blocks": [[0.0, 0.0, 2.0, 2.0]], "labels": [5]}]
    doc = PP.blocks_json(data, result)
    assert list(doc) == list(PP.CATEGORY_NAMES) and len(doc) == 13
    assert doc["text"] == {"doc_0.pdf": {"bboxes": [[1.0, 2.0, 3.0, 4.0], [9.0, 9.0, 10.0, 10.0]], "scores": [1.0, 1.0]}}
    assert doc["table"] == {"doc_0.pdf": {"bboxes": [[5.5, 6.0, 7.25, 8.0]], "scores": [1.0]}}
    assert doc["figure"] == {"doc_2.pdf": {"bboxes": [[0.0, 0.0, 2.0, 2.0]], "scores": [1.0]}}
    assert all(isinstance(v, float) for e in doc["text"].values() for b in e["bboxes"] for v in b)
    assert all(doc[k] == {} for k in doc if k not in ("text", "table", "figure"))
    assert json.loads(json.dumps(doc)) == doc


def test_extract_blocks_refuses_arguments_that_do_not_fit():
    data = _data(2)
    pred = [[1], [1]]
    with pytest.raises(ValueError, match="1 prediction lists for 2 pages"):
        PP.extract_blocks(data, pred[:1])
    with pytest.raises(ValueError, match="3 block lists for 2 pages"):
        PP.extract_blocks(data, pred, blocks=[[], [], []])
    with pytest.raises(ValueError, match="1 image lists for 2 pages"):
        PP.extract_blocks(data, pred, images=[[]])
    with pytest.raises(ValueError, match="scale"):
        PP.extract_blocks(data, pred, scale=0.0)
    with pytest.raises(ValueError, match=r"page 1 .*shape \(1, 3\)"):
        PP.extract_blocks(data, pred, blocks=[[], [[1.0, 2.0, 3.0]]])
    missing = _data(2)
    del missing.pages[1]["blocks"]
    with pytest.raises(ValueError, match=r"page 1 \(doc_1.pdf\) carries no 'blocks'"):
        PP.extract_blocks(missing, pred)
    with pytest.raises(ValueError, match="page 0 has 2 predictions and 1 boxes"):
        PP.extract_blocks(data, [[1, 1], [1]], device="cpu")
    with pytest.raises(ValueError, match="page 1 holds a class outside"):
        PP.extract_blocks(data, [[1], [9]], device="cpu")
