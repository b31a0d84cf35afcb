"""The host half of the SCIBERT embedder (components/nlp/scibert.py), without a device: the pure-Python BERT tokeniser against every
word recorded from the library (tests/golden/scibert_cases.json), the layout of ``token_ids`` with the page-dependent ``[SEP]``
rule, ``from_model_dir`` on a tiny directory, every ``ValueError``, and the memo."""
import json
import os

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.components.nlp.scibert import SciBERT, normalise, split_pieces
from tests import scibert_ref as ref

DATA = ref.golden()
PAGES = DATA["pages"]
VOCAB = DATA["vocab"]
IDS = {t: i for i, t in enumerate(VOCAB)}
CLS, SEP, PAD, UNK = (IDS[t] for t in ("[CLS]", "[SEP]", "[PAD]", "[UNK]"))
u = chr


def embedder(**kw):
    return SciBERT(VOCAB, DATA["embeddings"], device="cpu", **kw)


@pytest.fixture(scope="module")
def emb():
    return embedder()


@pytest.mark.parametrize("page", PAGES, ids=[p["name"] for p in PAGES])
def test_tokeniser_gives_the_recorded_pieces_of_every_word(emb, page):
    for word, pieces in zip(page["words"], page["pieces"]):
        assert list(emb.word_ids(word)) == pieces, (word, [VOCAB[i] for i in emb.word_ids(word)], [VOCAB[i] for i in pieces])


@pytest.mark.parametrize("page", PAGES, ids=[p["name"] for p in PAGES])
def test_token_ids_are_the_recorded_rows_under_the_recorded_mask(emb, page):
    got = emb.token_ids([page["words"]])
    assert got.dtype == np.int32 and got.shape == (len(page["words"]), 15)
    want = np.where(np.asarray(page["mask"]) == 1, np.asarray(page["input_ids"]), -1)[:, 1:]
    np.testing.assert_array_equal(got[:, :want.shape[1]], want)
    assert (got[:, want.shape[1]:] == -1).all()
    np.testing.assert_array_equal(got, ref.page_ids(page["pieces"], CLS, SEP, PAD, 15))


def test_the_steps_of_the_tokeniser_one_by_one():
    assert normalise("Caf" + u(0xE9)) == "cafe" and normalise("Caf" + u(0xE9), do_lower_case=False) == "Caf" + u(0xE9)
    assert normalise("a" + u(0x200B) + "b" + u(0) + "c" + u(0xFFFD) + u(0x85) + u(0x1C) + "d") == "abcd"       # dropped, not spaces
    assert normalise("a\tb" + u(0xA0) + "c" + u(0x3000) + "d" + u(0x2028)) == "a b c d "
    assert normalise("a" + u(0x4E2D) + "b") == "a " + u(0x4E2D) + " b"
    assert normalise("A" + u(0x3A3)) == "a" + u(0x3C3)                   # not the final sigma
    assert normalise(u(0x130)) == "i" and normalise(u(0xB5) + "m") == u(0xB5) + "m"       # no compatibility folding
    assert split_pieces("(1.1, p-value  x") == ["(", "1", ".", "1", ",", "p", "-", "value", "x"]
    assert split_pieces("a" + u(0x2013) + "b" + u(0x3002)) == ["a", u(0x2013), "b", u(0x3002)]
    assert split_pieces("") == [] and split_pieces("  ") == []


def test_wordpiece_rules(emb):
    assert emb.wordpiece("a" * 101) == [UNK] and len(emb.wordpiece("a" * 100)) > 1
    assert emb.wordpiece("table") == [IDS["table"]] and emb.wordpiece("tables") == [IDS["table"], IDS["##s"]]
    assert emb.wordpiece("ta" + u(0x394)) == [UNK]                       # an unmatched stretch: the whole piece
    assert emb.tokenize("x[SEP]y") == [IDS["x"], SEP, IDS["y"]] and emb.tokenize("[sep]") == [IDS["["], IDS["sep"], IDS["]"]]
    assert len(emb.word_ids("b1c2d3f4g5h6j7k8l9")) == 14 and len(emb.tokenize("b1c2d3f4g5h6j7k8l9")) == 18
    assert emb.word_ids("New York") == emb.word_ids("NewYork") == (IDS["new"], IDS["##y"], IDS["##or"], IDS["##k"])
    cased = embedder(do_lower_case=False)
    assert cased.word_ids("Table") == (UNK,) and cased.word_ids("table") == (IDS["table"],)
    no_mask = SciBERT([t for t in VOCAB if t != "[MASK]"], DATA["embeddings"][1:], device="cpu")
    assert len(no_mask.word_ids("[MASK]")) == 3 and no_mask.word_ids("[SEP]") == (no_mask.sep,)


def test_token_ids_layout_and_the_page_dependent_sep_rule(emb):
    a, t = IDS["a"], IDS["table"]
    pages = [["a", "table"], ["a", "a-a"], [], ["", ""], ["", "a"], ["a"]]
    got = emb.token_ids(pages)
    assert got.shape == (9, 15) and (got[:, 3:] == -1).all()
    dash = IDS["-"]
    want = [[a, -1, -1], [t, -1, -1],                # equal lengths: no [SEP]
            [a, SEP, -1], [a, dash, a],              # the same word beside a longer one: its [SEP] takes part, the longest word's not
            [-1, -1, -1], [-1, -1, -1],              # only empty words: nothing
            [SEP, -1, -1], [a, -1, -1],              # an empty word beside a longer one: [SEP] alone
            [a, -1, -1]]                             # a page of one word
    assert got[:, :3].tolist() == want
    assert emb.token_ids([]).shape == (0, 15) and emb.token_ids([[], []]).shape == (0, 15)
    short = embedder(max_length=4)
    assert short.token_ids([["a-a-a", "a"]]).tolist() == [[a, dash, -1], [a, SEP, -1]]


def test_memo_does_not_change_results():
    pages = [p["words"] for p in PAGES]
    cold, warm = embedder(), embedder()
    first = warm.token_ids(pages)
    assert warm._memo and np.array_equal(first, warm.token_ids(pages))       # from the memo
    np.testing.assert_array_equal(first, np.concatenate([cold.token_ids([p]) for p in reversed(pages)][::-1]))
    for p in pages:                                                          # and against no memo at all
        for w in p:
            stripped = "".join(w.split(" "))
            assert warm.word_ids(w) == tuple(cold.tokenize(stripped)[:14])
    assert len(warm._memo) <= len({"".join(w.split(" ")) for p in pages for w in p})


def test_from_model_dir(tmp_path):
    vocab = VOCAB[:40]
    weight = torch.arange(40 * 6, dtype=torch.float32).reshape(40, 6) + 1
    (tmp_path / "vocab.txt").write_text("".join(t + "\n" for t in vocab), encoding="utf-8")
    torch.save({"bert.embeddings.word_embeddings.weight": weight, "bert.embeddings.position_embeddings.weight": torch.zeros(4, 6)},
               tmp_path / "pytorch_model.bin")
    emb = SciBERT.from_model_dir(tmp_path, device="cpu", pooling="max")
    assert emb.do_lower_case and emb.pooling == "max" and (emb.n_vocab, emb.n_out) == (40, 6)
    assert torch.equal(emb.table, torch.nn.functional.normalize(weight))
    assert emb.word_ids("A") == (vocab.index("a"),)
    (tmp_path / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": False}))
    assert SciBERT.from_model_dir(os.fspath(tmp_path), device="cpu").word_ids("A") == (1,)
    os.remove(tmp_path / "pytorch_model.bin")
    with pytest.raises(ValueError, match="path"):
        SciBERT.from_model_dir(tmp_path, device="cpu")
    try:
        import safetensors.torch
    except ImportError:                                                      # read only where the library imports
        with pytest.raises(ValueError, match="path"):
            SciBERT.from_model_dir(tmp_path, device="cpu")
        return
    safetensors.torch.save_file({"embeddings.word_embeddings.weight": weight}, os.fspath(tmp_path / "model.safetensors"))
    assert torch.equal(SciBERT.from_model_dir(tmp_path, device="cpu").table, torch.nn.functional.normalize(weight))


def test_normalized_takes_the_table_as_it_is():
    table = torch.from_numpy(DATA["normalized"])
    assert torch.equal(embedder().table, torch.nn.functional.normalize(torch.from_numpy(DATA["embeddings"])))
    assert torch.equal(SciBERT(VOCAB, table, device="cpu", normalized=True).table, table)


@pytest.mark.parametrize("kw,word", [
    (dict(vocab=[t for t in VOCAB if t != "[UNK]"]), "vocab"), (dict(vocab=[t for t in VOCAB if t != "[CLS]"]), "vocab"),
    (dict(vocab=[t for t in VOCAB if t != "[SEP]"]), "vocab"), (dict(vocab={t: i for t, i in IDS.items() if t != "[PAD]"}), "vocab"),
    (dict(embeddings=DATA["embeddings"][:-1]), "embeddings"), (dict(embeddings=DATA["embeddings"][0]), "embeddings"),
    (dict(embeddings=np.zeros((len(VOCAB), 4), dtype=np.int64)), "embeddings"),
    (dict(pooling="sum"), "pooling"), (dict(max_length=2), "max_length"), (dict(max_length=34), "max_length"),
    (dict(max_length=16.0), "max_length")])
def test_value_errors_name_the_argument(kw, word):
    args = dict(vocab=VOCAB, embeddings=DATA["embeddings"], device="cpu")
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        SciBERT(**args)


def test_the_launcher_picks_the_access_form_and_refuses_bad_arguments_on_the_host():
    """Host arithmetic only: the pointers are numbers that nothing dereferences -- every call below returns before a launch."""
    lib = _lib.load()
    assert (lib.gte_token_pool_max_width(), lib.gte_token_pool_max_dim()) == (32, 4096)
    form = lib.gte_token_pool_access_bytes
    assert form(4096, 768, 8192, 768) == 16 and form(4096, 768, 8192 + 64 * 4, 832) == 16       # column 64 of an 832-float row
    assert form(4096, 768, 8192 + 63 * 4, 831) == 4 and form(4096, 768, 8192, 831) == 4         # column 63 of an 831-float row
    assert form(4096 + 4, 768, 8192, 768) == 4 and form(4096, 5, 8192, 8) == 4 and form(4096, 12, 8192, 12) == 16

    def call(tok=4096, n=7, width=15, table=8192, v=50, dim=12, mode=0, row_map=None, out=16384, ldo=12):
        return lib.gte_token_pool_f32(tok, n, width, table, v, dim, mode, row_map, out, ldo, None)
    for kw, code in [(dict(n=-1), -1), (dict(v=-1), -1), (dict(width=0), -1), (dict(dim=0), -1), (dict(v=2 ** 31), -1),
                     (dict(ldo=11), -1), (dict(mode=2), -1), (dict(width=33), -4), (dict(dim=4097, ldo=4097), -4),
                     (dict(tok=None), -1), (dict(out=None), -1), (dict(table=None), -1), (dict(tok=4098), -1),
                     (dict(table=8193), -1), (dict(out=16386), -1), (dict(row_map=4100), -1)]:
        assert call(**kw) == code, kw
        assert lib.gte_last_error()
    assert call(n=0) == 0 and call(n=0, tok=None, table=None, out=None) == 0


def test_no_cpu_fallback(emb):
    with pytest.raises(_lib.GteError):
        emb.features([["a"]])
