"""Golden cases of the block route  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the reference tree).

Runs the REFERENCE's own code, cut out of its files with ``ast`` at run time (the modules import PyMuPDF, pdf2image and a font
at their top and cannot be imported here); none of its text is held in this repository:
  * ``Categories_names`` (src/utils/const.py), ``intersect`` (src/components/graphs/utils.py) and ``get_tables_bbox``
    (src/components/graphs/postprocessing_2.py), compiled as they stand;
  * the two vote statements inside ``get_objects_bboxs``: the ``for bid, bbox in enumerate(bboxs)`` loop and the
    ``for l in labels_inside_blocks_counter`` loop, executed in a namespace that supplies ``bboxs``, ``blocks``, ``sf``,
    ``graph_node_preds``, ``cm``, ``labels_inside_blocks_counter`` and ``block_labels``;
  * ``LableModification`` (src/components/graphs/labels.py) for the revert map of the shipped ``to_remove``.
It writes tests/golden/blocks_cases.json: the inputs and the reference's outputs only.  The word assignment of a vote case is
the reference's too: the vote loop run on one word at a time names the block that the word's vote went to.

A generated assembly page on which the reference raises is dropped and counted; the tool fails above 2 % dropped pages.

    python tools/make_blocks_golden.py [reference/src]        # writes tests/golden/blocks_cases.json
"""
import ast
import copy
import json
import os
import sys
from enum import Enum

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import blocks_ref as ref                                    # noqa: E402

SF = 0.36
N_CAT = 13
OTHER, TEXT, TITLE, LIST, TABLE, FIGURE, CAPTION, COLH, SP, TCELL = 0, 1, 2, 3, 4, 5, 6, 7, 8, 10


def _top_level(path, name, kinds):
    text = open(path).read()
    for node in ast.parse(text).body:
        if isinstance(node, kinds) and node.name == name:
            return node
    raise KeyError(f"{name} not found in {path}")


def _run(node, path, ns):
    exec(compile(ast.Module(body=[node], type_ignores=[]), f"{path}:{getattr(node, 'name', 'statement')}", "exec"), ns)


def reference_code(src_root):
    """-> (get_tables_bbox, vote(bboxs, preds, blocks) -> (counters, labels), revert map of the shipped configuration)."""
    const = os.path.join(src_root, "utils", "const.py")
    ns = {"Enum": Enum}
    _run(_top_level(const, "Categories_names", ast.ClassDef), const, ns)
    cm = ns["Categories_names"]
    utils = os.path.join(src_root, "components", "graphs", "utils.py")
    _run(_top_level(utils, "intersect", ast.FunctionDef), utils, ns)
    post = os.path.join(src_root, "components", "graphs", "postprocessing_2.py")
    ns["cm"] = cm
    _run(_top_level(post, "get_tables_bbox", ast.FunctionDef), post, ns)

    outer = _top_level(post, "get_objects_bboxs", ast.FunctionDef)
    loops = [n for n in ast.walk(outer) if isinstance(n, ast.For)]
    word_loop = [n for n in loops if isinstance(n.target, ast.Tuple) and [getattr(e, "id", None) for e in n.target.elts] == ["bid", "bbox"]]
    label_loop = [n for n in loops if isinstance(n.target, ast.Name) and n.target.id == "l"
                  and getattr(n.iter, "id", None) == "labels_inside_blocks_counter"]
    assert len(word_loop) == 1 and len(label_loop) == 1, (len(word_loop), len(label_loop))

    def vote(bboxs, preds, blocks):
        env = {"bboxs": bboxs, "blocks": blocks, "sf": SF, "graph_node_preds": preds, "cm": cm,
               "labels_inside_blocks_counter": [[0 for _ in range(N_CAT)] for _ in blocks], "block_labels": list()}
        _run(word_loop[0], post, env)
        _run(label_loop[0], post, env)
        return env["labels_inside_blocks_counter"], env["block_labels"]

    labels = os.path.join(src_root, "components", "graphs", "labels.py")
    lns = {"np": np, "Categories_names": cm, "MAX_CLASS_COUNT": len(cm)}
    _run(_top_level(labels, "LableModification", ast.ClassDef), labels, lns)
    import yaml
    to_remove = yaml.safe_load(open(os.path.join(os.path.dirname(src_root), "configs", "graph", "graphs.yaml")))["LABELS"]["to_remove"]
    lt = lns["LableModification"](config={"LABELS": {"to_remove": to_remove}})
    n_classes = len(cm) - len(to_remove)
    revert = [int(v) for v in lt.revert(list(range(n_classes)))]
    return ns["get_tables_bbox"], vote, {"to_remove": [int(v) for v in to_remove], "revert": revert}


# ---- vote cases ---------------------------------------------------------------------------------------------------------
def hand_vote_cases():
    """Small pages, each made for one point of the rule (name, word boxes, categories, blocks in PDF points)."""
    e = 36.0                                                             # a block edge; where e / sf lands decides 'touching'
    edge = e / SF
    lo, hi = int(np.floor(edge)), int(np.ceil(edge))
    return [
        ("corner_point", [[200, 200, 300, 300]], [TEXT], [[108.0, 108.0, 144.0, 144.0]]),           # 108 / sf vs 300
        ("corner_point_word_first", [[0, 0, 100, 100]], [TEXT], [[36.0, 36.0, 72.0, 72.0]]),
        ("edge_after_division", [[10, 10, lo, 50], [10, 60, hi, 90], [10, 100, lo - 1, 120]], [TEXT, TEXT, LIST],
         [[e, 0.0, 72.0, 72.0]]),
        ("two_blocks_lower_index", [[100, 100, 200, 120], [400, 100, 420, 120]], [TEXT, LIST],
         [[18.0, 18.0, 90.0, 72.0], [30.0, 30.0, 180.0, 90.0], [140.0, 30.0, 160.0, 50.0]]),
        ("inverted_block", [[100, 100, 150, 120], [260, 100, 320, 120]], [CAPTION, CAPTION], [[90.0, 54.0, 30.0, 18.0]]),
        ("inverted_word", [[150, 120, 100, 100]], [LIST], [[30.0, 18.0, 90.0, 54.0]]),
        ("empty_blocks", [[1000, 1000, 1100, 1020]], [TEXT], [[0.0, 0.0, 10.0, 10.0], [20.0, 20.0, 30.0, 30.0]]),
        ("no_words", [], [], [[0.0, 0.0, 10.0, 10.0]]),
        ("no_blocks", [[1, 2, 3, 4], [5, 6, 7, 8]], [TEXT, TITLE], []),
        ("tie_lowest_category", [[10, 10, 20, 20], [30, 10, 40, 20], [50, 10, 60, 20], [70, 10, 80, 20]], [LIST, TEXT, LIST, TEXT],
         [[0.0, 0.0, 72.0, 72.0]]),
        ("tie_high_categories", [[10, 10, 20, 20], [30, 10, 40, 20]], [TCELL, COLH], [[0.0, 0.0, 72.0, 72.0]]),
        ("title_one_against_two_text", [[10, 10, 20, 20], [30, 10, 40, 20], [50, 10, 60, 20]], [TITLE, TEXT, TEXT],
         [[0.0, 0.0, 72.0, 72.0]]),                                                                  # 2 : 2 -> TEXT (lower)
        ("title_one_against_one_text", [[10, 10, 20, 20], [30, 10, 40, 20]], [TITLE, TEXT], [[0.0, 0.0, 72.0, 72.0]]),
        ("title_one_against_two_list", [[10, 10, 20, 20], [30, 10, 40, 20], [50, 10, 60, 20]], [TITLE, LIST, LIST],
         [[0.0, 0.0, 72.0, 72.0]]),                                                                  # 2 : 2 -> TITLE (lower)
        ("title_one_against_three_list", [[10, 10, 20, 20], [30, 10, 40, 20], [50, 10, 60, 20], [70, 10, 80, 20]],
         [TITLE, LIST, LIST, LIST], [[0.0, 0.0, 72.0, 72.0]]),
        ("zero_size_word_on_an_edge", [[200, 50, 200, 50]], [OTHER], [[36.0, 0.0, 72.0, 72.0]]),
    ]


def random_vote_case(rng):
    """A page of word boxes on text lines and blocks around groups of lines: some blocks overlap or touch their neighbours,
    some are inverted, some hold no word; few categories per page, so equal counts are common."""
    n_blocks = int(rng.integers(1, 9))
    blocks, words, cats = [], [], []
    for _ in range(n_blocks):
        x0, y0 = int(rng.integers(20, 1200)), int(rng.integers(20, 1900))
        w, h = int(rng.integers(80, 500)), int(rng.integers(20, 300))
        main = int(rng.choice([TEXT, TITLE, LIST, CAPTION, COLH, SP, TCELL]))
        other = int(rng.choice([TEXT, TITLE, LIST]))
        n_words = int(rng.integers(0, 7))
        for k in range(n_words):
            wx, wy = x0 + int(rng.integers(0, w)), y0 + int(rng.integers(0, h))
            words.append([wx, wy, min(wx + int(rng.integers(0, 90)), x0 + w), min(wy + int(rng.integers(0, 25)), y0 + h)])
            cats.append(main if rng.random() < 0.5 else other)
        # the block in PDF points as a text extractor gives them: the pixel box times sf, rounded to 3 decimals
        b = [round(x0 * SF, 3), round(y0 * SF, 3), round((x0 + w) * SF, 3), round((y0 + h) * SF, 3)]
        if rng.random() < 0.15:
            b = [b[2], b[3], b[0], b[1]]                                 # inverted corners
        blocks.append(b)
    for _ in range(int(rng.integers(0, 4))):                             # strays: often outside every block
        wx, wy = int(rng.integers(0, 1700)), int(rng.integers(0, 2200))
        words.append([wx, wy, wx + int(rng.integers(0, 90)), wy + int(rng.integers(0, 25))])
        cats.append(int(rng.choice([OTHER, TEXT, FIGURE])))
    order = rng.permutation(len(words)).tolist()
    return [words[i] for i in order], [cats[i] for i in order], blocks


def vote_case(name, words, cats, blocks, vote, get_tables_bbox):
    """The reference's vote on one page, and -- where its table assembly gives an answer for the voted labels -- the page's
    objects as get_objects_bboxs hands them on: the assembled blocks divided by sf (postprocessing_2.py:261,306), their labels."""
    counters, labels = vote(copy.deepcopy(words), list(cats), copy.deepcopy(blocks))
    try:
        new_blocks, new_labels, _ = get_tables_bbox(copy.deepcopy(blocks), list(labels))
        objects = {"blocks": [[n / SF for n in block] for block in new_blocks], "labels": [int(l) for l in new_labels]}
    except Exception:
        objects = None
    word_block = []
    for w, c in zip(words, cats):                                        # the reference's loop on one word: where did its vote go?
        one, _ = vote([list(w)], [c], copy.deepcopy(blocks))
        hit = [j for j, row in enumerate(one) if any(row)]
        assert len(hit) <= 1
        word_block.append(hit[0] if hit else -1)
    mine = ref.vote_page(words, cats, (np.asarray(blocks, dtype=np.float64).reshape(-1, 4) / SF), N_CAT, TITLE)
    assert mine == (word_block, counters, labels), name                  # tests/blocks_ref.py, re-verified on every case written
    return {"name": name, "bboxs": words, "cats": cats, "blocks": blocks,
            "ref": {"counters": counters, "labels": labels, "word_block": word_block, "objects": objects}}


# ---- assembly cases -------------------------------------------------------------------------------------------------------
def assembly_page(rng):
    """One page of one or two columns: paragraphs, titles and tables of 1 - 4 cell columns (optional header row, optional
    spanning row under it, missing cells, cells over two columns, stray TEXT blocks between rows, slivers of text centred
    exactly on a cell's edge).  PDF points, one decimal."""
    n_cols = int(rng.integers(1, 3))
    col_w = 520.0 / n_cols
    blocks, labels, stats = [], [], dict(missing=0, header=0, spanning=0, stray=0, wide=0, on_edge=0, two_columns=n_cols == 2)
    r1 = lambda v: round(float(v), 1)
    for c in range(n_cols):
        left = 40.0 + c * (col_w + 15.0)
        y = 50.0 + float(rng.integers(0, 30))
        while y < 380.0:
            if rng.random() < 0.45:                                      # a table
                k = int(rng.integers(1, 5))
                cw = (col_w - 10.0) / k
                if rng.random() < 0.6:
                    stats["header"] += 1
                    for j in range(k):
                        blocks.append([r1(left + j * cw + rng.uniform(0, 4)), r1(y), r1(left + (j + 1) * cw - rng.uniform(2, 8)), r1(y + 10)])
                        labels.append(COLH)
                    y += 13.0
                    if rng.random() < 0.35:
                        stats["spanning"] += 1
                        blocks.append([r1(left + rng.uniform(0, 4)), r1(y), r1(left + k * cw - rng.uniform(2, 8)), r1(y + 9)])
                        labels.append(SP)
                        y += 12.0
                headed = bool(labels) and labels[-1] in (COLH, SP)
                for row in range(int(rng.integers(1, 7))):               # rows
                    j, cells = 0, []
                    while j < k:
                        if rng.random() < 0.15:
                            stats["missing"] += 1
                            j += 1
                            continue
                        span = 2 if j + 1 < k and rng.random() < 0.1 else 1          # a cell over two columns
                        stats["wide"] += span == 2
                        dy = 0.5 * int(rng.integers(0, 4))               # few values: equal y-centres inside a group happen
                        cells.append([r1(left + j * cw + rng.uniform(0, 6)), r1(y + dy), r1(left + (j + span) * cw - rng.uniform(2, 12)),
                                      r1(y + 9 + dy)])
                        j += span
                    blocks.extend(cells)
                    labels.extend([TCELL] * len(cells))
                    if row == 0 and headed and cells and rng.random() < 0.3:
                        # a sliver of text in the gap under the header whose x-centre is EXACTLY an edge of a first-row cell
                        cell = cells[int(rng.integers(0, len(cells)))]
                        edge = cell[int(rng.choice([0, 2]))]
                        for d in (3.0, 4.5, 6.0, 2.5):
                            x0, x1 = r1(edge - d), r1(edge + d)
                            if (x1 + x0) / 2 == edge:
                                stats["on_edge"] += 1
                                blocks.append([x0, r1(y - 2.5), x1, r1(y - 0.5)])
                                labels.append(TEXT)
                                break
                    y += 13.0
                    if rng.random() < 0.12:                              # a stray text block inside the table
                        stats["stray"] += 1
                        sx = left + rng.uniform(0, col_w / 2)
                        blocks.append([r1(sx), r1(y), r1(sx + rng.uniform(20, col_w / 2)), r1(y + 8)])
                        labels.append(TEXT)
                        y += 10.0
                y += float(rng.integers(8, 30))
            else:                                                        # a paragraph, a title or a list
                h = float(rng.integers(10, 90))
                blocks.append([r1(left + rng.uniform(0, 3)), r1(y), r1(left + col_w - rng.uniform(0, 30)), r1(y + h)])
                labels.append(int(rng.choice([TEXT, TEXT, TEXT, TITLE, LIST, CAPTION])))
                y += h + float(rng.integers(6, 20))
    return blocks, labels, stats


def main(src_root):
    get_tables_bbox, vote, revert = reference_code(src_root)
    rng = np.random.default_rng(20261)

    votes = [vote_case(name, w, c, b, vote, get_tables_bbox) for name, w, c, b in hand_vote_cases()]
    while len(votes) < 40:
        w, c, b = random_vote_case(rng)
        votes.append(vote_case(f"random_{len(votes)}", w, c, b, vote, get_tables_bbox))
    seen_v = dict(
        tables=sum(bool(v["ref"]["objects"]) and TABLE in v["ref"]["objects"]["labels"] for v in votes),
        outside=sum(any(x == -1 for x in v["ref"]["word_block"]) for v in votes),
        tie=sum(any(sorted(row)[-1] == sorted(row)[-2] > 0 for row in v["ref"]["counters"]) for v in votes),
        empty_block=sum(any(not any(row) for row in v["ref"]["counters"]) for v in votes),
        inverted=sum(any(b[0] > b[2] for b in v["blocks"]) for v in votes),
        title=sum(any(row[TITLE] for row in v["ref"]["counters"]) for v in votes))
    assert all(n >= 3 for n in seen_v.values()), seen_v
    assert sum(v["ref"]["objects"] is not None for v in votes) >= 30     # (an inverted table block may leave the assembly no answer)

    pages, dropped, tried = [], 0, 0
    seen_a = dict(missing=0, header=0, spanning=0, stray=0, wide=0, on_edge=0, shuffled=0, two_columns=0, absorbed=0)
    while len(pages) < 60:
        tried += 1
        blocks, labels, stats = assembly_page(rng)
        shuffled = len(pages) % 3 == 2
        if shuffled:
            order = rng.permutation(len(blocks)).tolist()
            blocks, labels = [blocks[i] for i in order], [labels[i] for i in order]
        try:
            out_blocks, out_labels, headers = get_tables_bbox(copy.deepcopy(blocks), list(labels))
        except Exception:                                                # the reference gives no answer for this page
            dropped += 1
            continue
        for k in ("missing", "header", "spanning", "stray", "wide", "on_edge", "two_columns"):
            seen_a[k] += bool(stats[k])
        seen_a["shuffled"] += shuffled
        seen_a["absorbed"] += len(out_blocks) < len([l for l in labels if l not in (COLH, SP, TCELL)]) + out_labels.count(TABLE)
        pages.append({"blocks": blocks, "labels": labels,
                      "ref": {"blocks": out_blocks, "labels": [int(l) for l in out_labels], "headers": headers}})
    assert dropped <= 0.02 * tried, f"the reference raised on {dropped} of {tried} generated pages"
    assert all(n >= 10 for n in seen_a.values()), seen_a

    out = os.path.join(ROOT, "tests", "golden", "blocks_cases.json")
    with open(out, "w") as f:
        json.dump({"scale": SF, "n_cat": N_CAT, "double_cat": TITLE, "label_revert": revert, "votes": votes, "assembly": pages}, f,
                  separators=(",", ":"))
    assert json.load(open(out))["assembly"] == pages                     # JSON floats round-trip exactly
    print(f"{out}: {len(votes)} vote cases {seen_v}, {len(pages)} assembly pages {seen_a} ({dropped} of {tried} dropped), "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        from oracle.make_aux_golden import REF                          # where the other golden tools read the reference
        main(REF)
