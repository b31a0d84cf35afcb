"""Golden cases of the SCIBERT embedder  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the reference tree and the
``transformers`` library).

Runs the REFERENCE's own code, cut out of src/components/nlp/scibert.py with ``ast`` at run time (the module imports ``dgl`` and the
project's paths at its top and cannot be imported here); none of its text is held in this repository: ``list_of_sentence``,
``mean_pooling`` and ``max_pooling``, compiled as they stand into a stub class.  An instance is given what ``inizialize`` would
have set: the library's BERT tokenizer on a MADE-UP vocabulary of a few hundred entries (``BertTokenizer(vocab=<dict>,
do_lower_case=True)``: with ``vocab_file=`` transformers 5.15.0 maps every word to ``[UNK]``), and an ``Embedding`` of the
row-normalised seeded table, D = 12.  The tokenizer is wrapped so that the batch it returns -- whose mask ``list_of_sentence``
then modifies in place -- can be read afterwards.

It writes tests/golden/scibert_cases.json: inputs and the reference's outputs only.  Per page: the words, ``input_ids``, the
modified mask, and the mean and max outputs.  Before it writes, it asserts on every page that
  * tests/scibert_ref.py reproduces ``input_ids`` and the mask from the pieces, the max output by value and the mean output within
    ``scibert_ref.mean_bound``;
  * ``SciBERT.token_ids`` (the pure-Python tokeniser) gives the recorded ids with -1 where the mask is 0;
and that not every recorded word is ``[UNK]``.

    python tools/make_scibert_golden.py [reference/src]      # writes tests/golden/scibert_cases.json
"""
import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import scibert_ref as ref                                   # noqa: E402

u = chr                                                                  # code points below are written as numbers: no invisible text
DIM = 12
MAX_LENGTH = 16


def vocabulary():
    letters = "abcdefghijklmnopqrstuvwxyz"
    digits = "0123456789"
    some = "aeiourstn"
    tokens = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    tokens += list(letters) + list(digits) + ["##" + c for c in letters + digits]
    tokens += list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~") + [u(0x2013), u(0xAB), u(0xBB), u(0x3002)]
    tokens += [a + b for a in some for b in some] + ["##" + a + b for a in some for b in some]
    tokens += ["cafe", "table", "value", "image", "results", "caption", "figure", "york", "new", "##ble", "##lue", "naive", "angstrom",
               "sep", "cls", "mask", u(0x3BC), u(0x3BC) + "m", u(0x3C3), "##" + u(0x3C3), u(0x3C2), "##" + u(0x3C2), u(0x3B1), "##" + u(0x3B2),
               u(0x4E2D), u(0x6587), u(0x3042), "##" + u(0x3042), u(0xDF), "i" + u(0x307)]
    assert len(set(tokens)) == len(tokens), [t for t in tokens if tokens.count(t) > 1]
    return tokens


def corpus():
    long_word = "b1c2d3f4g5h6j7k8l9"                                   # 18 pieces: cut to 14
    return [
        ("mixed_lengths", ["banana33", "p-value", "33", "1.1", "(1.1,", "Table", "2:", "results", "Caf" + u(0xE9), "IMAGE!", "a"]),
        ("equal_lengths", ["a", "b", "table", "7", "!"]),                # one piece each: no [SEP] is pooled
        ("equal_lengths_three", ["1.1", "a-b", "(a)"]),
        ("only_empty", ["", "", ""]),
        ("one_word", ["p-value"]),
        ("one_empty_word", [""]),
        ("one_long_word", [long_word]),
        ("empty_beside_longer", ["", "table", "", "a1", " ", "   "]),   # [SEP] alone; words of spaces only
        ("accents_capitals", ["Caf" + u(0xE9), "CAFE", "na" + u(0xEF) + "ve", u(0xC5) + "ngstr" + u(0xF6) + "m", u(0x130), "a" + u(0x301), u(0xC9) + "a",
                              "A" + u(0x3A3), u(0x3A3) + "a", u(0xDF), "STRASSE"]),
        ("punctuation", ["(1.1,", "--", "a.b.c", "[1]", "x^2", "a_b", "$5", "50%", u(0xAB) + "a" + u(0xBB), "a" + u(0x2013) + "b", "a" + u(0x3002),
                         "...", "~", "'s"]),
        ("hyphens", ["p-value", "x-ray", "-5", "3-5", "a-b-c", "-"]),
        ("cjk", ["a" + u(0x4E2D) + "b", u(0x4E2D) + u(0x6587), "table" + u(0x6587), u(0x3042) + u(0x3042), "a" + u(0x3042), u(0x4E2D)]),
        ("control_zero_width", ["a" + u(0x200B) + "b", "a" + u(0) + "b", "a" + u(0xFFFD) + "b", "a" + u(0xAD) + "b", "a" + u(0x1C) + "b", "a" + u(0x85) + "b",
                                "a" + u(0xE000) + "b", "a" + u(0x180E) + "b", u(0x200B), "a" + u(0x7F) + "b", "a" + u(0xFEFF) + "b"]),
        ("inner_whitespace", ["a\tb", "a" + u(0xA0) + "b", "a\nb", "a" + u(0x2028) + "b", "a" + u(0x3000) + "b", "New York", " lead", "a" + u(0x2009) + "b",
                              "a\rb", "a" + u(0x202F) + "b", "\t"]),
        ("micro", [u(0xB5) + "m", u(0x3BC) + "m", u(0x3BC), "5" + u(0xB5) + "m", u(0x3B1) + u(0x3B2)]),
        ("over_100_characters", ["a" * 101, "a" * 100, "ab" * 51, "a" * 101 + "-b", "b"]),
        ("over_14_pieces", [long_word, "a1b2c3d4e5f6g7", "a1b2c3d4e5f6g7h", "a1b2c3d4e5f6g", "ab"]),
        ("all_truncated", [long_word, long_word + "x"]),                 # every row is 16 long: no [SEP] is pooled
        ("special_tokens", ["[SEP]", "[CLS]", "[PAD]", "[UNK]", "[MASK]", "x[SEP]y", "[sep]", "[SEP][SEP]", "a[CLS]", "[ SEP ]", "[SEP"]),
        ("image", ["IMAGE!", "IMAGE!", "table"]),
        ("unknown", ["zzzz" + u(0x394), "a" + u(0x394), u(0x394), "q", "caf" + u(0x394)]),
    ]


def reference_code(src_root):
    """-> make(tokenizer, weight): an object with the reference's list_of_sentence and poolings, on the CPU."""
    import torch
    path = os.path.join(src_root, "components", "nlp", "scibert.py")
    with open(path) as f:
        body = ast.parse(f.read()).body
    cls = [n for n in body if isinstance(n, ast.ClassDef) and n.name == "SciBERT"][0]
    wanted = ("list_of_sentence", "mean_pooling", "max_pooling")
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(m.name for m in methods) == sorted(wanted)
    stub = ast.ClassDef(name="Cut", bases=[], keywords=[], body=methods, decorator_list=[])
    if "type_params" in ast.ClassDef._fields:
        stub.type_params = []
    ns = {"torch": torch}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[stub], type_ignores=[])), f"{path}:SciBERT", "exec"), ns)

    def make(tokenizer, weight, pooling):
        obj = ns["Cut"]()
        obj.specifics = types.SimpleNamespace(is_cuda=False, return_tensor=True)
        obj.seen = []

        def recording(texts, **kw):
            enc = tokenizer(texts, **kw)
            obj.seen.append(enc)
            return enc
        obj.tokenizer = recording
        obj.embeddings = torch.nn.Embedding.from_pretrained(weight)
        obj.pooling = getattr(obj, pooling + "_pooling")
        return obj
    return make


def f32_list(a):
    vals = [float(str(np.float32(v))) for v in np.asarray(a, dtype=np.float32).ravel()]
    assert np.array_equal(np.asarray(vals, dtype=np.float64).astype(np.float32), np.asarray(a, dtype=np.float32).ravel())
    return vals


def main(src_root):
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")
    import torch
    import tokenizers
    import transformers
    from transformers import BertTokenizer
    from gnn_tableextraction_amd.components.nlp.scibert import SciBERT

    tokens = vocabulary()
    vocab = {t: i for i, t in enumerate(tokens)}
    tokenizer = BertTokenizer(vocab=vocab, do_lower_case=True)
    assert len(tokenizer) == len(tokens)
    rng = np.random.default_rng(20268)
    table = np.round(rng.normal(size=(len(tokens), DIM)), 4).astype(np.float32)
    with torch.no_grad():
        weight = torch.nn.functional.normalize(torch.FloatTensor(torch.from_numpy(table)))           # scibert.py:45-46
    normalized = weight.numpy()
    make = reference_code(src_root)
    objs = {mode: make(tokenizer, weight, mode) for mode in ("mean", "max")}
    mine = SciBERT(vocab, table, device="cpu", max_length=MAX_LENGTH)
    cls, sep, pad, unk = (vocab[t] for t in ("[CLS]", "[SEP]", "[PAD]", "[UNK]"))

    pages, n_words, n_unk = [], 0, 0
    for name, words in corpus():
        texts = ["".join(w.split(" ")) for w in words]                  # what _online_batch_ hands to list_of_sentence
        out = {}
        for mode, obj in objs.items():
            with torch.no_grad():
                out[mode] = obj.list_of_sentence(list(texts), max_length=MAX_LENGTH).numpy()
            assert out[mode].dtype == np.float32 and out[mode].shape == (len(words), DIM)
        enc = objs["mean"].seen[-1]
        ids, mask = enc["input_ids"].numpy(), enc["attention_mask"].numpy()
        assert np.array_equal(ids, objs["max"].seen[-1]["input_ids"].numpy())
        assert not mask[:, 0].any() and not mask[:, -1].any() and ids.shape[1] <= MAX_LENGTH
        # the pieces of every word: between [CLS] and the [SEP] that ends the row, by the library's own UNMODIFIED mask (a second
        # call: the first call's mask has been changed in place; a word may itself hold [SEP] or [PAD])
        lengths = tokenizer(list(texts), padding=True, truncation=True, max_length=MAX_LENGTH, return_tensors="pt")["attention_mask"].sum(1)
        pieces = [row[1:int(n) - 1] for row, n in zip(ids.tolist(), lengths)]
        want_ids, want_mask = ref.page_rows(pieces, cls, sep, pad)
        tok = ref.page_ids(pieces, cls, sep, pad, MAX_LENGTH - 1)
        assert np.array_equal(want_ids, ids) and np.array_equal(want_mask, mask), (name, ids, want_ids, mask, want_mask)
        got = mine.token_ids([words])
        assert np.array_equal(got, tok), (name, got.tolist(), tok.tolist())
        assert np.array_equal(ref.pool(tok, normalized, "max"), out["max"]), name
        mean = ref.pool(tok, normalized, "mean")
        bound = ref.mean_bound(tok, normalized, out["mean"])
        assert np.all(np.abs(mean.astype(np.float64) - out["mean"]) <= bound), (name, float(np.abs(mean - out["mean"]).max()))
        n_words += len(words)
        n_unk += sum(p == [unk] for p in pieces)
        pages.append({"name": name, "words": words, "input_ids": ids.tolist(), "mask": mask.tolist(), "pieces": pieces,
                      "mean": f32_list(out["mean"]), "max": f32_list(out["max"])})
    assert n_unk < n_words / 2, (n_unk, n_words)                        # the tokenizer really tokenises (see the module docstring)

    data = {"transformers_version": transformers.__version__, "tokenizers_version": tokenizers.__version__, "max_length": MAX_LENGTH,
            "do_lower_case": True, "vocab": tokens, "embeddings": [f32_list(r) for r in table],
            "normalized": [f32_list(r) for r in normalized], "pages": pages}
    path = os.path.join(ROOT, "tests", "golden", "scibert_cases.json")
    with open(path, "w") as f:
        json.dump(data, f, separators=(",", ":"), ensure_ascii=True)
    with open(path) as f:
        assert json.load(f) == data                                     # JSON floats and strings round-trip exactly
    print(f"{path}: transformers {transformers.__version__}, {len(pages)} pages, {n_words} words ({n_unk} of them [UNK]), "
          f"{len(tokens)} vocabulary entries, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        from oracle.make_aux_golden import REF                          # where the other golden tools read the reference
        main(REF)
