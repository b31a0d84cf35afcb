"""Golden cases of the REPR embedder  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the reference tree and the
``tokenizers`` library).

Runs the REFERENCE's own code, cut out of src/components/nlp/repr.py with ``ast`` at run time (the module imports ``attrdict`` and
the project's paths at its top and cannot be imported here); none of its text is held in this repository:
  * ``CustomNormalizer``, compiled as it stands;
  * ``Repr``, compiled as it stands on a stub base class; an instance is made without its constructor and given the attributes
    that ``inizialize`` would have set -- the arrays from the case, and the tokenizer from the statements of ``inizialize`` that
    build it (the ones that assign to ``tok`` or hand it to ``self``), executed in a namespace that supplies ``self``.
It writes tests/golden/repr_cases.json: inputs and the reference's outputs only.
  (a) ``tokeniser``: a corpus of pages of words with the ids and tokens that the reference's ``encode`` gives for the page string
      of repr.py:103-104.  ``Repr.token_ids`` (the pure-Python normaliser) is re-verified on every page written.
  (b) ``sets``: artefact sets with pages and the reference's ``__call__`` outputs, hard and combined, the first n_p rows of every
      page.  The tool asserts that every vocabulary row of every set has its two best clamped distances bit-equal or more than
      1e-9 apart (tests/repr_ref.py: separated_or_tied), and that tests/repr_ref.py reproduces the hard outputs exactly.

    python tools/make_repr_golden.py [reference/src]        # writes tests/golden/repr_cases.json
"""
import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import repr_ref as ref                                      # noqa: E402

u = chr                                                                  # code points below are written as numbers: no invisible text


def reference_code(src_root):
    """-> make(repr2idx, embeddings, prototypes, i_embedding): an instance of the reference's Repr on the CPU."""
    import torch
    import tokenizers
    from tokenizers import NormalizedString, Regex, Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.normalizers import Normalizer
    from tokenizers.pre_tokenizers import WhitespaceSplit
    path = os.path.join(src_root, "components", "nlp", "repr.py")
    body = ast.parse(open(path).read()).body
    classes = {n.name: n for n in body if isinstance(n, ast.ClassDef)}
    ns = {"t": torch, "Tokenizer": Tokenizer, "Regex": Regex, "NormalizedString": NormalizedString, "Normalizer": Normalizer,
          "WhitespaceSplit": WhitespaceSplit, "WordLevel": WordLevel, "Embedder": type("Embedder", (), {})}
    for name in ("CustomNormalizer", "Repr"):
        exec(compile(ast.Module(body=[classes[name]], type_ignores=[]), f"{path}:{name}", "exec"), ns)
    init = [n for n in classes["Repr"].body if isinstance(n, ast.FunctionDef) and n.name == "inizialize"][0]

    def about_tok(stmt):
        if not isinstance(stmt, ast.Assign):
            return False
        target = stmt.targets[0]
        on_tok = isinstance(target, ast.Name) and target.id == "tok" or \
            isinstance(target, ast.Attribute) and isinstance(target.value, ast.Name) and target.value.id == "tok"
        return on_tok or isinstance(stmt.value, ast.Name) and stmt.value.id == "tok"
    tok_statements = [s for s in init.body if about_tok(s)]
    assert len(tok_statements) >= 4, len(tok_statements)

    def make(repr2idx, embeddings, prototypes, i_embedding):
        obj = ns["Repr"].__new__(ns["Repr"])
        obj.specifics = types.SimpleNamespace(is_cuda=False, return_tensor=True, use_words=False)
        obj.centers = torch.from_numpy(np.asarray(prototypes)).double()
        obj.i_prototypes = torch.from_numpy(np.asarray(i_embedding)).double()
        obj.embeddings = torch.from_numpy(np.asarray(embeddings)).double()
        obj.repr2idx = dict(repr2idx)
        env = dict(ns, self=obj)
        exec(compile(ast.Module(body=tok_statements, type_ignores=[]), f"{path}:inizialize", "exec"), env)
        return obj
    return make, tokenizers.__version__


def page_string(words):
    """The string that the reference encodes for a page (the two comprehensions in front of ``encode``, restated: the tool's
    own assertion below compares the whole ``__call__`` on the same pages)."""
    return " ".join("".join(w.split(" ")) for w in words)


# ---- (a) the tokeniser corpus -------------------------------------------------------------------------------------------
TOKENS = ["<UNK_W>", "w", "x", "wx", "xw", "w-w", "-x", "+x", "x-x", "w-x", "x.x", "(x.x,", "x,x", "w.", "(w)", "x%", "wxw", "w:"]


def corpus():
    fw = lambda s, base: "".join(u(base + ord(c)) for c in s)            # full-width forms: U+FF01 .. = '!' ..
    return [
        ("ascii", ["banana33", "p-value", "33", "1.1", "(1.1,", "Table", "2:", "results", "(n)", "45%", "1,5", "a1b", "7th"]),
        ("signs", ["-5", "+5", "3-5", "x-ray", "e-3", "--", "-", "5-", "a-5", "A-B-C"]),
        ("latin1_greek", ["na" + u(0xEF) + "ve", u(0xC5) + "ngstr" + u(0xF6) + "m", u(0x3A9) + "-7", u(0x3B1) + u(0x3B2), u(0xB5) + "m",
                          u(0xDF), u(0x3C0) + "2"]),
        ("full_width", [fw("123", 0xFEE0), fw("ABC", 0xFEE0), fw("a1", 0xFEE0), fw("-5", 0xFEE0), fw("(1.1,", 0xFEE0)]),
        ("compat", [u(0xFB01) + "nd", "e" + u(0xFB03) + "ct", "x" + u(0xB2), "10" + u(0x207B) + u(0xB3), u(0xBD), "1" + u(0xBC), u(0x2460),
                    u(0x2167), u(0x2122), "n" + u(0x2080)]),
        ("inner_space", ["New York", " lead", "trail ", "a b c", "1 000", "p - value"]),
        ("odd_spaces", ["a\tb", "c" + u(0xA0) + "d", "e" + u(0x2009) + "f", "g" + u(0x1F) + "h", "i" + u(0x1C) + "j", "k\nl", "m" + u(0x3000) + "n",
                        "o" + u(0x200B) + "p", "q" + u(0x85) + "r", "s" + u(0x202F) + "t"]),
        ("empty_middle_and_end", ["alpha", "", "12", "beta-2", "", "9", ""]),
        ("only_empty", ["", "", ""]),
        ("spaces_only_words", [" ", "word", "  ", "7"]),
        ("unknown_symbols", [u(0x2211), u(0x2192) + "x", "@", "#1", u(0x20AC) + "5", "a_b", "~", u(0x4E2D) + u(0x6587), u(0x0663)]),
        ("no_words", []),
    ]


def tokeniser_section(make):
    repr2idx = {t: i for i, t in enumerate(TOKENS)}
    tok = make(repr2idx, np.zeros((len(TOKENS), 1)), np.zeros((1, 1)), np.zeros((1, 1))).tokenizer
    from gnn_tableextraction_amd.components.nlp.repr import Repr
    mine = Repr.__new__(Repr)
    mine.repr2idx, mine.unk, mine.n_vocab = repr2idx, 0, len(TOKENS)
    pages = []
    for name, words in corpus():
        enc = tok.encode(page_string(words))
        pages.append({"name": name, "words": words, "ids": [int(i) for i in enc.ids], "tokens": list(enc.tokens)})
        got = mine.token_ids([words])
        assert got.tolist() == ref.align([enc.ids], [len(words)]).tolist(), (name, got.tolist(), enc.ids, enc.tokens)
    return {"repr2idx": repr2idx, "pages": pages}


# ---- (b) artefact sets ----------------------------------------------------------------------------------------------------
SET_TOKENS = ["<UNK_W>", "w", "x", "wx", "w-w", "-x", "x.x", "(x.x,", "w.", "x%", "x-x", "w:"]
SET_PAGES = [
    ["banana33", "p-value", "33", "1.1", "(1.1,", "Table", "2:", "end.", "45%", "3-5", "-5", "results"],
    ["alpha", "", "12", "beta-gamma", u(0x2211), "9", "x"],                # an empty word: later words shift, the last node has no token
    ["7", "New York", "caption:", "", ""],
    ["a b", "c\td", "4"],                                                  # a tab inside a word: one token more than words
]


def f32_json(a):
    vals = [[float(str(np.float32(v))) for v in row] for row in np.asarray(a, dtype=np.float32)]
    assert np.array_equal(np.asarray(vals, dtype=np.float64).astype(np.float32), np.asarray(a, dtype=np.float32))
    return vals


def artefact_set(make, name, embeddings, prototypes, i_embedding):
    import torch
    repr2idx = {t: i for i, t in enumerate(SET_TOKENS)}
    assert embeddings.shape[0] == len(SET_TOKENS)
    assert ref.separated_or_tied(embeddings, prototypes), name
    obj = make(repr2idx, embeddings, prototypes, i_embedding)
    sizes = [len(p) for p in SET_PAGES]
    out = {"name": name, "repr2idx": repr2idx, "embeddings": embeddings.tolist(), "prototypes": prototypes.tolist(),
           "i_embedding": i_embedding.tolist(), "pages": SET_PAGES}
    ids = [obj.tokenizer.encode(page_string(p)).ids for p in SET_PAGES]
    tok = ref.align(ids, sizes)
    for mode, combined in (("hard", False), ("combined", True)):
        with torch.no_grad():
            res = obj(None, [list(p) for p in SET_PAGES], None, combined=combined).numpy()
        assert res.dtype == np.float32 and res.shape[0] == len(SET_PAGES)
        rows = [res[i, :min(n, res.shape[1])] for i, n in enumerate(sizes)]          # the first n_p rows (fewer: the tensor is shorter)
        out[mode] = [f32_json(r) for r in rows]
        want, bound = ref.features(tok, embeddings, prototypes, i_embedding, 1.0, combined)
        o = 0
        for r, n in zip(rows, sizes):
            w, b = want[o:o + len(r)], bound[o:o + len(r)]
            assert np.all(np.abs(r.astype(np.float64) - w) <= b), (name, mode, float(np.abs(r - w).max()))
            assert np.all(want[o + len(r):o + n] == 0)
            o += n
    return out


def sets_section(make):
    rng = np.random.default_rng(20267)
    v, c = len(SET_TOKENS), 47
    r4 = lambda shape: np.round(rng.normal(size=shape), 4)              # short decimal literals; the doubles they name are the data
    out = [artefact_set(make, "normal_c47_d3_p50", r4((v, 3)), r4((c, 3)), r4((c, 50))),
           artefact_set(make, "normal_c47_d50_p50", r4((v, 50)), r4((c, 50)), r4((c, 50)))]
    # small integers with real ties.  Row 1 ('w'): the centres 2, 5 and 7 lie within 1e-4 of it -- 2 at distance 1e-5, 5 at distance 0,
    # 7 at 2e-5: all clamp to 1e-4 and centre 2 wins.  Row 2 ('x'): the centres 3 and 9 are duplicates.  Row 3 ('wx'): the centres 0
    # and 4 are different points at the same distance.  Every other distance is the root of a different small integer.
    emb = rng.integers(-4, 5, size=(v, 3)).astype(np.float64)
    cen = rng.integers(-4, 5, size=(12, 3)).astype(np.float64) + np.array([20.0, 0.0, 0.0])     # far from every row by default
    emb[1] = [1.0, 2.0, 3.0]
    cen[2], cen[5], cen[7] = [1.0, 2.0, 3.0 + 1e-5], [1.0, 2.0, 3.0], [1.0 + 2e-5, 2.0, 3.0]
    emb[2] = [-3.0, 0.0, 2.0]
    cen[3] = cen[9] = [-3.0, 1.0, 2.0]
    emb[3] = [0.0, -4.0, 0.0]
    cen[0], cen[4] = [2.0, -4.0, 0.0], [0.0, -4.0, -2.0]
    ipr = (np.arange(12)[:, None] * 4 + np.arange(4)[None, :]).astype(np.float64)                # row c = c * P + j: names its centre
    ties = artefact_set(make, "integer_ties_c12_d3_p4", emb, cen, ipr)
    chosen = ref.chosen_centre([1, 2, 3], emb, cen)
    assert chosen.tolist() == [2, 3, 0], chosen
    out.append(ties)
    return out


def main(src_root):
    make, version = reference_code(src_root)
    data = {"tokenizers_version": version, "tokeniser": tokeniser_section(make), "sets": sets_section(make)}
    out = os.path.join(ROOT, "tests", "golden", "repr_cases.json")
    with open(out, "w") as f:
        json.dump(data, f, separators=(",", ":"), ensure_ascii=True)
    back = json.load(open(out))
    assert back["sets"] == data["sets"] and back["tokeniser"] == data["tokeniser"]          # JSON floats and strings round-trip exactly
    n_words = sum(len(p["words"]) for p in data["tokeniser"]["pages"]) + sum(len(p) for p in SET_PAGES)
    print(f"{out}: tokenizers {version}, {len(data['tokeniser']['pages'])} corpus pages, {len(data['sets'])} artefact sets, "
          f"{n_words} words, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        from oracle.make_aux_golden import REF                          # where the other golden tools read the reference
        main(REF)
