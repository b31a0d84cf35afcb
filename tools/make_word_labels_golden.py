"""Golden cases of the word labels  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the reference tree).

Runs the REFERENCE's own code, cut out of its files with ``ast`` at run time (builder.py imports PyMuPDF and DGL at its top and
cannot be imported here); none of its text is held in this repository:
  * ``center`` (src/components/graphs/utils.py) and the nested ``get_label`` (src/components/graphs/builder.py), compiled as they
    stand, with ``annotations`` and ``center`` supplied as the globals their bodies use;
  * the two statements of ``get_nodes`` that build the node list: the ``if set_labels:`` block that turns FIGURE annotations
    into nodes and the ``for token in tokens`` loop, executed in a namespace that supplies ``annotations``, ``tokens``,
    ``set_labels``, ``SCALE_FACTOR`` = 1 (the words are given in page pixels already) and the three result lists;
  * ``Categories_names`` (src/utils/const.py) for the names an annotation carries next to its id.
An annotation of the reference is ``[rectangle, category id, category name]``.  The winning annotation of a word is the
reference's too: ``get_label`` run on the same rectangles with every name 'FIGURE' exchanged for 'TEXT' and the ids replaced by
1 + the annotation's index returns exactly that.

It writes tests/golden/word_labels_cases.json: the inputs and the reference's outputs only (a NaN coordinate is written as null).

    python tools/make_word_labels_golden.py        # writes tests/golden/word_labels_cases.json
"""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_aux_golden as aux                              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "word_labels_cases.json")
OTHER, TEXT, TITLE, LIST, TABLE, FIGURE, CAPTION, COLH, SP, GCELL, TCELL, COL, ROW = range(13)


def reference_code():
    """-> (names [13], labels(words, ann) -> get_label per word, nodes(words, texts, ann) -> (bboxs, texts, labels))."""
    const_src = open(os.path.join(aux.REF, "utils/const.py")).read()
    enum = next(n for n in ast.walk(ast.parse(const_src)) if isinstance(n, ast.ClassDef) and n.name == "Categories_names")
    names = {t.value.value: t.targets[0].id for t in enum.body if isinstance(t, ast.Assign)}
    names = [names[i] for i in range(len(names))]
    center = aux.extract("components/graphs/utils.py", "center")
    path = os.path.join(aux.REF, "components/graphs/builder.py")
    tree = ast.parse(open(path).read())
    get_nodes = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "get_nodes")
    figure_block = [n for n in get_nodes.body if isinstance(n, ast.If) and getattr(n.test, "id", None) == "set_labels"]
    token_loop = [n for n in get_nodes.body if isinstance(n, ast.For) and getattr(n.target, "id", None) == "token"]
    assert len(figure_block) == 1 and len(token_loop) == 1, (len(figure_block), len(token_loop))

    def as_reference(ann, ids=None, rename=False):
        return [[list(r[:4]), int(r[4]) if ids is None else ids[j], "TEXT" if rename and names[int(r[4])] == "FIGURE" else names[int(r[4])]]
                for j, r in enumerate(ann)]

    def get_label_of(annotations):
        return aux.extract("components/graphs/builder.py", "get_label", glb={"annotations": annotations, "center": center})

    def labels(words, ann):
        f = get_label_of(as_reference(ann))
        g = get_label_of(as_reference(ann, ids=[j + 1 for j in range(len(ann))], rename=True))
        return [f(list(w)) for w in words], [g(list(w)) - 1 for w in words]

    def nodes(words, texts, ann):
        annotations = as_reference(ann)
        env = {"annotations": annotations, "tokens": [list(w) + [t] for w, t in zip(words, texts)], "set_labels": True,
               "SCALE_FACTOR": 1, "get_label": get_label_of(annotations), "bboxs": [], "texts": [], "labels": []}
        for stmt in (figure_block[0], token_loop[0]):
            exec(compile(ast.Module(body=[stmt], type_ignores=[]), f"{path}:get_nodes", "exec"), env)
        return env["bboxs"], env["texts"], env["labels"]

    return names, labels, nodes


def hand_made():
    """(name, words, annotations [r0, r1, r2, r3, category]) -- the edges of the rule, one at a time."""
    big = 2 ** 31 - 1
    cases = [
        ("odd_and_even_sums", [[0, 0, 10, 10], [0, 0, 11, 11], [1, 1, 10, 10], [3, 3, 4, 4]], [[4, 4, 6, 6, TEXT], [3, 3, 5, 5, TITLE]]),
        ("negative_truncates_towards_zero", [[-11, -11, 0, 0], [-11, -11, 2, 2], [-3, -3, 0, 0], [-1, -1, 0, 0]],
         [[-5.5, -5.5, -4.5, -4.5, TEXT], [-6.5, -6.5, -5.5, -5.5, TITLE], [-1.5, -1.5, -0.5, -0.5, LIST], [-0.5, -0.5, 0.5, 0.5, CAPTION]]),
        ("zero_size_word", [[7, 7, 7, 7], [0, 0, 0, 0]], [[6, 6, 8, 8, LIST], [-1, -1, 1, 1, SP]]),
        ("near_int32_limits", [[big - 2, big - 2, big, big], [-big - 1, -big - 1, -big + 1, -big + 1], [-big - 1, -big - 1, big, big]],
         [[big - 2, big - 2, big, big, TEXT], [-big - 1.5, -big - 1.5, -big + 0.5, -big + 0.5, TITLE], [-1, -1, 1, 1, LIST]]),
        ("on_each_edge_and_one_inside", [[10, 20, 10, 20], [30, 20, 30, 20], [20, 10, 20, 10], [20, 30, 20, 30], [11, 11, 11, 11],
                                         [29, 29, 29, 29], [20, 20, 20, 20]], [[10, 10, 30, 30, TEXT]]),
        ("half_integer_edges", [[10, 10, 10, 10], [11, 11, 11, 11], [12, 12, 12, 12], [10, 10, 11, 11]],
         [[10.5, 10.5, 11.5, 11.5, TITLE], [9.5, 9.5, 10.5, 10.5, LIST]]),
        ("overlap_a_then_b", [[5, 5, 15, 15]], [[0, 0, 20, 20, TEXT], [5, 5, 15, 15, TITLE]]),
        ("overlap_b_then_a", [[5, 5, 15, 15]], [[5, 5, 15, 15, TITLE], [0, 0, 20, 20, TEXT]]),
        ("table_first_is_skipped", [[12, 12, 18, 18], [40, 40, 44, 44]],
         [[0, 0, 100, 100, TABLE], [0, 0, 100, 50, ROW], [0, 0, 50, 100, COL], [0, 0, 100, 100, GCELL], [10, 10, 20, 20, TCELL]]),
        ("figure_first_drops", [[5, 5, 15, 15], [50, 50, 60, 60]], [[0, 0, 20, 20, FIGURE], [0, 0, 20, 20, TEXT]]),
        ("text_then_figure_keeps", [[5, 5, 15, 15], [50, 50, 60, 60]], [[0, 0, 20, 20, TEXT], [0, 0, 20, 20, FIGURE], [45, 45, 70, 70, FIGURE]]),
        ("nan_and_inverted", [[5, 5, 15, 15]], [[float("nan"), 0, 20, 20, TEXT], [0, 0, float("nan"), 20, TITLE], [20, 20, 0, 0, LIST],
                                               [20, 0, 0, 20, CAPTION], [0, 0, 20, 20, SP]]),
        ("no_annotations", [[1, 2, 3, 4], [5, 6, 7, 8]], []),
        ("no_words", [], [[0, 0, 9, 9, FIGURE], [0, 0, 9, 9, TEXT]]),
        ("only_figures", [[1, 1, 3, 3]], [[0, 0, 4, 4, FIGURE], [10, 10, 20, 20, FIGURE]]),
        ("every_word_dropped", [[1, 1, 3, 3], [2, 2, 4, 4]], [[0, 0, 10, 10, FIGURE]]),
    ]
    return cases


def random_page(rng, k):
    """A page in the spirit of the dataset: regions of every category, some nested (cells in a table), a few degenerate."""
    n_words, n_ann = int(rng.integers(1, 60)), int(rng.integers(0, 30))
    x0, y0 = rng.integers(-40, 600, n_words), rng.integers(-40, 800, n_words)
    words = np.stack([x0, y0, x0 + rng.integers(0, 60, n_words), y0 + rng.integers(0, 20, n_words)], 1).tolist()
    ann = []
    for _ in range(n_ann):
        ax, ay = float(rng.integers(-60, 560)), float(rng.integers(-60, 760))
        w, h = float(rng.integers(1, 400)), float(rng.integers(1, 400))
        if rng.random() < 0.3:
            ax, ay, w, h = ax + 0.5, ay + 0.5, w + 0.5 * int(rng.integers(0, 2)), h
        cat = int(rng.integers(0, 13)) if k % 3 else int(rng.choice([TEXT, TABLE, FIGURE, TCELL, COLH, ROW]))
        r = [ax, ay, ax + w, ay + h]
        if cat == FIGURE:                                    # a figure becomes a node: whole pixels, as in the dataset
            r = [float(int(v)) for v in r]
        elif rng.random() < 0.05:
            r = [r[2], r[3], r[0], r[1]]                    # inverted
        ann.append(r + [cat])
    return words, ann


def main(out=OUT):
    names, labels, nodes = reference_code()
    rng = np.random.default_rng(20240607)
    cases = hand_made() + [(f"random_{k}", *random_page(rng, k)) for k in range(48)]
    doc = {"categories": names, "cases": []}
    n_labelled = n_dropped = 0
    for name, words, ann in cases:
        texts = [f"w{i}" for i in range(len(words))]
        word_label, word_ann = labels(words, ann)
        bboxs, node_texts, node_labels = nodes(words, texts, ann)
        n_fig = sum(1 for r in ann if r[4] == FIGURE)
        assert node_texts[:n_fig] == ["IMAGE!"] * n_fig
        n_labelled += sum(1 for v in word_label if v > 0)
        n_dropped += sum(1 for v in word_label if v == -1)
        doc["cases"].append({
            "name": name, "words": words, "annotations": [[None if v != v else v for v in r[:4]] + [r[4]] for r in ann],
            "word_label": word_label, "word_ann": word_ann, "kept": [int(v != -1) for v in word_label],
            "figures": [j for j, r in enumerate(ann) if r[4] == FIGURE],
            "node_boxes": [[None if v != v else v for v in b] for b in bboxs], "node_labels": node_labels,
            "node_words": [int(t[1:]) if t != "IMAGE!" else -1 for t in node_texts]})
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"wrote {out}: {len(doc['cases'])} cases, {n_labelled} words labelled, {n_dropped} dropped for a figure, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
