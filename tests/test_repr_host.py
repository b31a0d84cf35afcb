"""Host side of the REPR embedder (components/nlp/repr.py): the pure-Python normaliser and the page alignment against the ids that
the reference's tokenizer recorded (tests/golden/repr_cases.json), the constructor's checks, the reference's file layout, and the
argument checks of gte_repr_features that return before any launch.  Nothing here needs a GPU."""
import pickle
import random

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.components.nlp import repr as R
from gnn_tableextraction_amd.components.nlp.repr import Repr
from tests import repr_ref as ref

DATA = ref.golden()
CORPUS = DATA["tokeniser"]


def embedder(repr2idx, n_vocab=None):
    n = max(repr2idx.values()) + 1 if n_vocab is None else n_vocab
    return Repr(repr2idx, np.zeros((n, 2)), np.zeros((3, 2)), np.zeros((3, 5)), device="cpu")


@pytest.mark.parametrize("page", CORPUS["pages"], ids=[p["name"] for p in CORPUS["pages"]])
def test_token_ids_reproduce_the_recorded_ids_and_the_alignment(page):
    emb = embedder(CORPUS["repr2idx"])
    known = CORPUS["repr2idx"]                                             # (the recorded tokens name an unknown one "<UNK_W>")
    assert [t if t in known else "<UNK_W>" for t in R.page_tokens(page["words"])] == page["tokens"]
    got = emb.token_ids([page["words"]])
    assert got.dtype == np.int32 and got.shape == (len(page["words"]),)
    np.testing.assert_array_equal(got, ref.align([page["ids"]], [len(page["words"])]))


def test_the_corpus_covers_what_it_should():
    pages = {p["name"]: p for p in CORPUS["pages"]}
    n_words = sum(len(p["words"]) for p in CORPUS["pages"])
    assert 60 <= n_words <= 400
    assert any(len(p["ids"]) > len(p["words"]) for p in CORPUS["pages"])          # surplus tokens (a tab inside a word)
    assert any(0 < len(p["ids"]) < len(p["words"]) for p in CORPUS["pages"])      # empty words: nodes without a token
    assert pages["only_empty"]["ids"] == [] and len(pages["only_empty"]["words"]) == 3
    signs = dict(zip(pages["signs"]["words"], pages["signs"]["tokens"]))
    assert signs["-5"] == "-x" and signs["+5"] == "+x" and signs["3-5"] == "x-x"  # the fifth step has no effect
    assert "w-x" in pages["latin1_greek"]["tokens"] and all(t == t.lower() or t == "<UNK_W>" for p in CORPUS["pages"] for t in p["tokens"])
    odd = pages["odd_spaces"]
    assert any("\x1f" in w for w in odd["words"]) and len(odd["ids"]) > len(odd["words"])


def test_all_pages_at_once_padding_and_truncation():
    emb = embedder(CORPUS["repr2idx"])
    pages = [p["words"] for p in CORPUS["pages"]]
    got = emb.token_ids(pages)
    np.testing.assert_array_equal(got, ref.align([p["ids"] for p in CORPUS["pages"]], [len(w) for w in pages]))
    ids = CORPUS["repr2idx"]
    w, x = ids["w"], ids["x"]
    # an empty word yields no token: the later words of its page take their successor's, the last node is left without one
    np.testing.assert_array_equal(emb.token_ids([["alpha", "", "12", "beta"]]), [w, x, w, -1])
    np.testing.assert_array_equal(emb.token_ids([["", ""], ["7"]]), [-1, -1, x])
    # a tab inside a word makes two tokens of it: the surplus token at the end of the page is dropped
    np.testing.assert_array_equal(emb.token_ids([["a\tb", "4"]]), [w, w])
    np.testing.assert_array_equal(emb.token_ids([["a b", "4"]]), [w, x])           # an ASCII space inside a word is removed
    np.testing.assert_array_equal(emb.token_ids([["g\x1fh"]]), [ids["<UNK_W>"]])   # U+001F is no white space: one unknown token
    assert emb.token_ids([]).shape == (0,) and emb.token_ids([[]]).shape == (0,)


def test_a_page_with_an_id_outside_the_table_falls_back_to_row_zero():
    repr2idx = {"<UNK_W>": 2, "w": 1, "x": 7}                                      # 'x' names no row of a 3-row table
    emb = embedder(repr2idx, n_vocab=3)
    got = emb.token_ids([["abc", "12", "def", ""], ["abc", "?"], ["9"]])
    np.testing.assert_array_equal(got, [0, 0, 0, -1, 1, 2, 0])
    neg = embedder({"<UNK_W>": 0, "w": -1}, n_vocab=3)
    np.testing.assert_array_equal(neg.token_ids([["abc", "1"]]), [0, 0])


def test_constructor_checks():
    with pytest.raises(ValueError, match="<UNK_W>"):
        Repr({"w": 0}, np.zeros((1, 2)), np.zeros((3, 2)), np.zeros((3, 5)), device="cpu")
    with pytest.raises(ValueError, match="do not fit together"):
        Repr({"<UNK_W>": 0}, np.zeros((1, 2)), np.zeros((3, 4)), np.zeros((3, 5)), device="cpu")
    with pytest.raises(ValueError, match="do not fit together"):
        Repr({"<UNK_W>": 0}, np.zeros((1, 2)), np.zeros((3, 2)), np.zeros((4, 5)), device="cpu")
    emb = Repr({"<UNK_W>": 0}, np.zeros((1, 2), dtype=np.float32), [[0, 1]], [[1, 2, 3]], device="cpu", alpha=2)
    assert emb.embeddings.dtype == emb.centers.dtype == emb.i_prototypes.dtype == torch.float64
    assert (emb.n_vocab, emb.n_out, emb.alpha) == (1, 3, 2.0)


def test_no_cpu_fallback():
    emb = embedder(CORPUS["repr2idx"])
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        emb.features([["abc"]])
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        emb(None, [["abc"]], None)
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        G.repr_features(torch.zeros(1, dtype=torch.int32), emb.embeddings, emb.centers, emb.i_prototypes)


def test_from_reference_files_round_trip(tmp_path):
    case = DATA["sets"][0]
    tables, pts = tmp_path / "tables_preprocess", tmp_path / "repr_pts"
    (pts / "run7").mkdir(parents=True)
    tables.mkdir()
    with open(pts / "run7" / "trained_prototypes_epoch12_47_0.5.dat", "wb") as f:
        pickle.dump({"prototypes": case["prototypes"], "i_embedding": case["i_embedding"], "unused": 1}, f)
    with open(tables / "embed-repr-47-3-5000.dat", "wb") as f:
        pickle.dump({"embeddings": case["embeddings"]}, f)
    with open(tables / "repr2idx.dat", "wb") as f:
        pickle.dump(case["repr2idx"], f)
    emb = Repr.from_reference_files(tables, pts, "run7", 12, 47, 0.5, 3, 5000, device="cpu")
    assert emb.repr2idx == case["repr2idx"] and emb.alpha == 1.0
    np.testing.assert_array_equal(emb.embeddings.numpy(), case["embeddings"])
    np.testing.assert_array_equal(emb.centers.numpy(), case["prototypes"])
    np.testing.assert_array_equal(emb.i_prototypes.numpy(), case["i_embedding"])
    with pytest.raises(FileNotFoundError):
        Repr.from_reference_files(tables, pts, "run8", 12, 47, 0.5, 3, 5000, device="cpu")


def chars(*points):
    return "".join(chr(c) for c in points)


# code points as numbers: no invisible text in this file
ALPHABETS = ["abcXYZ", "0123456789", "-+.,()%:/'",
             chars(0xE9, 0xEF, 0xF6, 0xC5, 0xDF, 0xB5),                                         # Latin-1 letters
             chars(0x3A9, 0x3B1, 0x3B2, 0x3C0, 0x3A3),                                          # Greek
             chars(0xFF11, 0xFF12, 0xFF19, 0xFF21, 0xFF42, 0xFF0D, 0xFF08),                     # full-width digits, letters, signs
             chars(0xFB01, 0xFB03, 0xB2, 0xB3, 0x207B, 0x2080, 0xBD, 0xBC, 0x2460, 0x2167, 0x2122),   # ligatures, superscripts, fractions
             chars(0x09, 0xA0, 0x2009, 0x1F, 0x1C, 0x3000, 0x200B, 0x85, 0x202F, 0x0A),         # spaces and what is none
             chars(0x2211, 0x2192, 0x40, 0x23, 0x7E, 0x5F, 0x20AC, 0x4E2D, 0x663)]              # symbols, CJK, an Arabic-Indic digit


def test_the_normaliser_agrees_with_the_tokenizers_library():
    """The effective steps (NFKC, the character map, the two collapses) and the whitespace split, built from the library's own
    operations, on a generated corpus over the alphabets of the fixture.  That the reference's fifth and sixth steps have no
    effect is not asserted here but recorded in the fixture."""
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers import Regex, Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.normalizers import Normalizer
    from tokenizers.pre_tokenizers import WhitespaceSplit

    class Steps:
        def normalize(self, text):
            text.nfkc()
            text.map(lambda ch: "x" if ch.isdigit() else "w" if ch.isalpha() else ch)
            text.replace(Regex("x+"), "x")
            text.replace(Regex("w+"), "w")

    repr2idx = CORPUS["repr2idx"]
    tok = Tokenizer(WordLevel(repr2idx, unk_token="<UNK_W>"))
    tok.normalizer = Normalizer.custom(Steps())
    tok.pre_tokenizer = WhitespaceSplit()
    rnd = random.Random(5)
    pages = []
    for _ in range(30):
        words = []
        for _ in range(rnd.randint(0, 14)):
            kinds = rnd.sample(ALPHABETS, rnd.randint(1, 3))
            words.append("".join(rnd.choice(rnd.choice(kinds)) for _ in range(rnd.randint(0, 6))))
        pages.append(words)
    assert 150 <= sum(len(p) for p in pages) <= 400
    emb = embedder(repr2idx)
    for words in pages:
        enc = tok.encode(" ".join("".join(w.split(" ")) for w in words))
        assert [repr2idx.get(t, 0) for t in R.page_tokens(words)] == enc.ids, words
        np.testing.assert_array_equal(emb.token_ids([words]), ref.align([enc.ids], [len(words)]))


# ---- gte_repr_features: what returns before a launch -------------------------------------------------------------------------
def call(lib, tok=0x1000, n=4, emb=0x2000, v=10, d=3, cen=0x3000, ipr=0x4000, c=47, p=50, alpha=1.0, combined=0, out=0x5000, ldo=None):
    return lib.gte_repr_features(tok, n, emb, v, d, cen, ipr, c, p, alpha, combined, out, p if ldo is None else ldo, None)


def test_limits_and_argument_checks_return_before_any_launch():
    lib = _lib.load()
    assert (lib.gte_repr_max_centroids(), lib.gte_repr_max_dim(), lib.gte_repr_max_out()) == (64, 1024, 1024)
    bad = [dict(tok=0), dict(emb=0), dict(cen=0), dict(ipr=0), dict(out=0), dict(n=-1), dict(v=-1), dict(d=0), dict(c=0), dict(p=0),
           dict(d=-3), dict(ldo=49), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(combined=2),
           dict(emb=0x2004), dict(cen=0x3004), dict(ipr=0x4004), dict(tok=0x1002), dict(out=0x5001)]
    for kw in bad:
        assert call(lib, **kw) == -1, kw
        assert b"repr_features" in lib.gte_last_error()
    for kw in (dict(c=65), dict(d=1025), dict(p=1025), dict(c=65, n=0), dict(c=65, tok=0)):       # the limits come before everything
        assert call(lib, **kw) == -4, kw                                                         # but the plain size checks
    assert call(lib, c=65, ldo=10) == -1
    # nothing to do: no launch, whatever the pointers
    assert call(lib, n=0) == 0 and call(lib, n=0, tok=0, emb=0, cen=0, ipr=0, out=0) == 0
    assert call(lib, n=0, c=64, d=1024, p=1024) == 0
