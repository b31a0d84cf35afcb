"""Host side of the REPR training stage (components/tables/): the alphabet compaction and the dense cost tables of
``LevenshteinSimilitudes``, its limits, the vocabulary builders, ``train_repr`` on a caller's similarity matrix (scikit-learn on
the host), the files it writes as ``Repr.from_reference_files`` reads them, and the argument checks of gte_lev_matrix_f64 that
return before any launch.  Nothing here needs a GPU."""
import pickle
import random

import numpy as np
import pytest

from gnn_tableextraction_amd import _lib
from gnn_tableextraction_amd.components.nlp.repr import Repr
from gnn_tableextraction_amd.components.tables import levenshtein as L, preprocessor as P, vocabulator as V
from tests import lev_ref as ref

BOM, ASTRAL = chr(0xFEFF), chr(0x1D7D9)               # code points as numbers: no invisible text in this file


# ---- LevenshteinSimilitudes: what happens before the device ------------------------------------------------------------------
def test_alphabet_compaction_with_an_astral_code_point_and_the_bom():
    words = ["x.x", BOM + "w" + ASTRAL, "", "%"]
    src, dst, alphabet = L.LevenshteinSimilitudes().prepare(words)
    assert dst == words and src == ["x.x", "w" + ASTRAL, "", "%"]         # only the first argument loses U+FEFF
    assert alphabet == sorted(ord(c) for c in "x.w%" + BOM + ASTRAL) and alphabet[-1] == 0x1D7D9 and 0xFEFF in alphabet
    chars, off = L.encode(dst, alphabet)
    assert chars.dtype == np.uint16 and off.dtype == np.int32
    np.testing.assert_array_equal(off, [0, 3, 6, 6, 7])
    assert [alphabet[k] for k in chars] == [ord(c) for c in "".join(dst)]
    chars_s, off_s = L.encode(src, alphabet)
    np.testing.assert_array_equal(off_s, [0, 3, 5, 5, 6])
    assert L.alphabet_of(["ba"], ["c", ""]) == [97, 98, 99] and L.alphabet_of([], [""]) == []
    # numpy strings, as train_repr hands them over
    assert L.LevenshteinSimilitudes().prepare(np.asarray(["w", "x-x"]))[1] == ["w", "x-x"]
    assert L.LevenshteinSimilitudes().prepare([""])[2] == [0]              # only empty words: a one-character alphabet


def test_dense_tables_hold_the_defaults_and_the_overrides():
    alphabet = sorted("wx.,%-" + BOM + ASTRAL)
    points = [ord(c) for c in alphabet]
    lev = L.LevenshteinSimilitudes()
    for got, want in zip(lev.tables(points), ref.uniform().dense(alphabet)):
        np.testing.assert_array_equal(got, want)
        assert got.dtype == np.float64 and (got == 1.0).all()
    assert lev.init_weights() is lev
    ins, dele, sub = lev.tables(points)
    for got, want in zip((ins, dele, sub), ref.reference().dense(alphabet)):
        np.testing.assert_array_equal(got, want)
    at = {c: k for k, c in enumerate(alphabet)}
    assert sub[at["x"], at["%"]] == 5.0 and sub[at["%"], at["x"]] == 1.0   # one direction only
    assert sub[at["."], at[","]] == sub[at[","], at["."]] == sub[at["w"], at["x"]] == sub[at["x"], at["w"]] == 1.9
    assert (ins[at["%"]], ins[at["."]], ins[at[","]], dele[at["%"]], dele[at["."]], dele[at[","]]) == (1.5, 2, 2, 1.5, 2, 2)
    # overrides by character or code point; characters outside the alphabet do not appear; uniform drops everything
    lev.set_insert(ASTRAL, 3.0).set_delete(0xFEFF, 0.5).set_substitute("-", ASTRAL, 7.0).set_insert("q", 9.0)
    ins, dele, sub = lev.tables(points)
    assert ins[at[ASTRAL]] == 3.0 and dele[at[BOM]] == 0.5 and sub[at["-"], at[ASTRAL]] == 7.0 and sub[at[ASTRAL], at["-"]] == 1.0
    assert 9.0 not in ins
    assert all((t == 1.0).all() for t in lev.init_weights_uniform().tables(points))
    with pytest.raises(ValueError, match="not one character"):
        lev.set_insert("ab", 1.0)


def test_limits_raise_before_any_device_call():
    lev = L.LevenshteinSimilitudes().init_weights()
    assert lev.prepare(["w" * 64])[1] == ["w" * 64]
    with pytest.raises(ValueError, match="65 characters"):
        lev.calculate_similarity(["w", "x" * 65], device="cuda:0")
    many = [chr(0x4E00 + i) for i in range(1025)]
    assert len(lev.prepare(many[:1024])[2]) == 1024
    with pytest.raises(ValueError, match="1025 distinct"):
        lev.calculate_similarity(many, device="cuda:0")


def test_the_empty_word_list_and_no_cpu_fallback():
    got = L.LevenshteinSimilitudes().calculate_similarity([], device="cuda:0")
    assert got.shape == (0, 0) and got.dtype == np.float64
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        L.LevenshteinSimilitudes().calculate_similarity(["w", "x"], device="cpu")


# ---- the vocabulary -------------------------------------------------------------------------------------------------------------
def test_build_repr_vocab_order_and_stable_ties():
    rc = {"w": 5, "<UNK_W>": 1, "x": 9, "x.x": 5, "w-w": 5, "(x)": 2, "%": 9}
    idx2repr, repr2idx, vocab = V.build_repr_vocab(rc, max_vocab=6)
    assert idx2repr == ["<UNK_W>", "x", "%", "w", "x.x", "w-w"]            # ties keep the order of rc; '(x)' falls off
    assert repr2idx == {t: i for i, t in enumerate(idx2repr)} and vocab == set(idx2repr)
    assert V.build_repr_vocab(rc)[0] == ["<UNK_W>", "x", "%", "w", "x.x", "w-w", "(x)"]
    assert V.build_repr_vocab(rc, max_vocab=1)[0] == ["<UNK_W>"]
    assert rc["<UNK_W>"] == 1 and len(rc) == 7                             # the caller's dictionary is left alone
    with pytest.raises(ValueError, match="<UNK_W>"):
        V.build_repr_vocab({"w": 1})
    # the unknown token counted high: still first, and only once
    assert V.build_repr_vocab({"w": 2, "<UNK_W>": 50, "x": 3})[0] == ["<UNK_W>", "x", "w"]


def test_count_representations_counts_the_tokens_the_embedder_looks_up():
    pages = [["Table", "12", "3.5", "a b", ""], ["-5", "x1", "12", "7,5%", "tab\there"]]
    rc = V.count_representations(pages)
    assert rc == {"<UNK_W>": 1, "w": 4, "x": 2, "x.x": 1, "-x": 1, "wx": 1, "x,x%": 1}
    assert list(rc)[0] == "<UNK_W>"
    assert V.count_representations([]) == {"<UNK_W>": 1} and V.count_representations([[], [""]]) == {"<UNK_W>": 1}
    emb = Repr(V.build_repr_vocab(rc)[1], np.zeros((len(rc), 2)), np.zeros((3, 2)), np.zeros((3, 5)), device="cpu")
    assert (emb.token_ids(pages) != emb.unk).all()                         # every token of the corpus is in its vocabulary


# ---- train_repr on the host ------------------------------------------------------------------------------------------------------
def small_rc(n=50, seed=3):
    rnd = random.Random(seed)
    rc = {}
    while len(rc) < n - 1:
        rc.setdefault("".join(rnd.choice("wx.,-%()/") for _ in range(rnd.randint(1, 6))), rnd.randint(1, 40))
    items = list(rc.items())
    items.insert(n // 2, ("<UNK_W>", 1))
    return dict(items)


def test_repr_words_orders():
    rc = small_rc()
    words = P.repr_words(rc, 20)
    assert len(words) == 20 and [rc[w] for w in words] == sorted(rc.values(), reverse=True)[:20]
    assert P.repr_words(rc, 5000) == sorted(rc, key=rc.get, reverse=True) and "<UNK_W>" in P.repr_words(rc, 5000)
    assert P.repr_words(rc, 20, align=True) == V.build_repr_vocab(rc, 20)[0]


def test_train_repr_on_a_given_similarity_and_the_files_it_leaves(tmp_path):
    pytest.importorskip("sklearn")
    rc = small_rc()
    n, limit = len(rc), 2000
    words = P.repr_words(rc, limit)
    sim = ref.similarity(words, ref.reference())
    result = P.train_repr(rc, limit=limit, similarity=sim, random_state=0, tsne_kwargs={"perplexity": 10})
    assert set(result) == {"centers", "labels", "words", "embeddings"}
    assert list(result["words"]) == words
    centers, labels = np.asarray(result["centers"]), np.asarray(result["labels"])
    assert 1 <= len(centers) <= n and ((0 <= centers) & (centers < n)).all()
    assert labels.shape == (n,) and set(labels) == set(range(len(centers)))
    np.testing.assert_array_equal(labels[centers], np.arange(len(centers)))           # every exemplar leads its own cluster
    assert result["embeddings"].shape == (n, 3) and np.isfinite(result["embeddings"]).all()
    with pytest.raises(ValueError, match="similarity matrix"):
        P.train_repr(rc, limit=limit, similarity=sim[:-1, :-1])

    # the files, read back as the embedder reads them
    tables, pts = tmp_path / "tables_preprocess", tmp_path / "repr_pts"
    idx2repr, repr2idx, vocab = V.build_repr_vocab(rc, max_vocab=limit)
    V.dump_repr_files(tables, rc, idx2repr, repr2idx, vocab)
    path = P.write_embed_repr(tables, result, 3, limit)
    assert path == str(tables / f"embed-repr-{len(centers)}-3-{n}.dat")                # the limit is lowered to the words taken
    for name, want in (("rc.dat", rc), ("idx2repr.dat", idx2repr), ("repr2idx.dat", repr2idx), ("repr_vocab.dat", vocab)):
        with open(tables / name, "rb") as f:
            assert pickle.load(f) == want
    (pts / "run1").mkdir(parents=True)
    rng = np.random.default_rng(0)
    proto = {"prototypes": result["embeddings"][centers], "i_embedding": rng.normal(size=(len(centers), 50))}
    with open(pts / "run1" / f"trained_prototypes_epoch3_{len(centers)}_1.0.dat", "wb") as f:
        pickle.dump(proto, f)
    emb = Repr.from_reference_files(tables, pts, "run1", 3, len(centers), 1.0, 3, n, device="cpu")
    assert emb.repr2idx == repr2idx and emb.n_vocab == n and emb.n_out == 50
    np.testing.assert_array_equal(emb.embeddings.numpy(), result["embeddings"])
    np.testing.assert_array_equal(emb.centers.numpy(), proto["prototypes"])


def test_align_puts_the_row_of_a_token_at_its_repr2idx():
    pytest.importorskip("sklearn")
    rc = small_rc(n=40, seed=4)
    idx2repr, repr2idx, _ = V.build_repr_vocab(rc, max_vocab=30)
    words = P.repr_words(rc, 30, align=True)
    sim = ref.similarity(words, ref.reference())
    result = P.train_repr(rc, limit=30, similarity=sim, random_state=0, tsne_kwargs={"perplexity": 8}, align=True)
    assert all(result["words"][repr2idx[t]] == t for t in idx2repr) and result["embeddings"].shape == (30, 3)
    assert ((0 <= np.asarray(result["centers"])) & (np.asarray(result["centers"]) < 30)).all()
    # the default order is another one: the unknown token is not first there
    assert P.repr_words(rc, 30)[0] != "<UNK_W>"


def test_train_repr_names_the_stages_that_need_scikit_learn(monkeypatch):
    import sys
    for name in [m for m in sys.modules if m == "sklearn" or m.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "sklearn", None)                      # import sklearn -> ImportError
    with pytest.raises(ImportError, match="AffinityPropagation.*TSNE"):
        P.train_repr({"<UNK_W>": 1, "w": 2}, similarity=np.zeros((2, 2)))


# ---- gte_lev_matrix_f64: what returns before a launch ----------------------------------------------------------------------------
def call(lib, sc=0x1000, so=0x2000, ns=3, dc=0x3000, do=0x4000, nd=5, max_len=64, ins=0x5000, dele=0x6000, sub=0x7000, na=12,
         out=0x8000, ldo=None):
    return lib.gte_lev_matrix_f64(sc, so, ns, dc, do, nd, max_len, ins, dele, sub, na, out, nd if ldo is None else ldo, None)


def test_limits_and_argument_checks_return_before_any_launch():
    lib = _lib.load()
    assert (lib.gte_lev_max_len(), lib.gte_lev_max_alphabet()) == (64, 1024)
    bad = [dict(ns=-1), dict(nd=-1), dict(max_len=-1), dict(ldo=4), dict(so=0), dict(do=0), dict(ins=0), dict(dele=0), dict(sub=0),
           dict(out=0), dict(sc=0x1001), dict(dc=0x3001), dict(so=0x2002), dict(do=0x4002), dict(ins=0x5004), dict(dele=0x6004),
           dict(sub=0x7004), dict(out=0x8004)]
    for kw in bad:
        assert call(lib, **kw) == -1, kw
        assert b"lev_matrix" in lib.gte_last_error()
    for kw in (dict(max_len=65), dict(na=1025), dict(na=0), dict(na=-3), dict(max_len=65, ns=0), dict(na=1025, out=0)):
        assert call(lib, **kw) == -4, kw                                   # the limits come before the empty call and the pointers
    assert call(lib, max_len=65, ldo=4) == -1                              # but after the plain size checks
    # nothing to do: no launch, whatever the pointers
    assert call(lib, ns=0) == 0 and call(lib, nd=0) == 0
    assert call(lib, ns=0, sc=0, so=0, dc=0, do=0, ins=0, dele=0, sub=0, out=0) == 0
    assert call(lib, nd=0, max_len=64, na=1024, out=0) == 0
