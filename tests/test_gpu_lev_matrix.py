"""gte_lev_matrix_f64 against tests/lev_ref.py (the recurrence of include/gte.h in numpy, pinned on hand cases by
tests/test_lev_ref_cpu.py).  Every comparison is exact: each cell is one of three correctly rounded float64 sums or a copy.

Shapes (n_src, n_dst): below, at and above one wave of words on either side -- the kernel puts one dst word on a lane, the issue's
shapes were chosen for one src word per lane, so both orientations are here -- and several words on the other side.  Word lengths
from {0, 1, 2, 5, 9} plus a word of 63 and one of 64 characters on each side, an empty word against an empty word included.  Costs:
uniform; the reference's; random in [0.1, 5] with ins != del and an asymmetric sub (swapped tables, swapped operands and the wrong
equal-characters rule all show there).  Alphabets of 1, 12 and 1024 characters."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.components.tables import levenshtein as L
from tests import lev_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (1, 3), (63, 2), (64, 1), (65, 5), (130, 67), (2, 63), (1, 64), (5, 65)]
LENGTHS = (0, 1, 2, 5, 9)


def make_words(n, n_alpha, rng, long_words):
    """n words as lists of compact ids; with ``long_words`` two of them (when n allows) have 63 and 64 characters."""
    lens = [int(rng.choice(LENGTHS)) for _ in range(n)]
    if long_words and n >= 3:
        lens[n // 2], lens[n - 1] = 63, 64
        lens[0] = 0                                                        # an empty word on both sides: '' against ''
    return [[int(c) for c in rng.integers(0, n_alpha, size=k)] for k in lens]


def pack(words):
    off = np.zeros(len(words) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(w) for w in words])
    return np.asarray([c for w in words for c in w], dtype=np.uint16), off


def random_costs(n_alpha, rng):
    ins, dele, sub = rng.uniform(0.1, 5.0, n_alpha), rng.uniform(0.1, 5.0, n_alpha), rng.uniform(0.1, 5.0, (n_alpha, n_alpha))
    assert n_alpha == 1 or ((ins != dele).any() and (sub != sub.T).any())
    return ins, dele, sub


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(src, dst, tables, **kw):
    (sc, so), (dc, do) = pack(src), pack(dst)
    return G.lev_matrix(dev(sc), dev(so), dev(dc), dev(do), *(dev(t) for t in tables), **kw)


@pytest.mark.parametrize("n_src,n_dst", SHAPES)
def test_random_costs_over_twelve_characters_are_exact(n_src, n_dst):
    rng = np.random.default_rng(n_src * 1000 + n_dst)
    tables = random_costs(12, rng)
    src, dst = make_words(n_src, 12, rng, True), make_words(n_dst, 12, rng, True)
    want = ref.matrix_ids(src, dst, *tables)
    got = run(src, dst, tables)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n_src, n_dst)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if n_src >= 3 and n_dst >= 3:
        assert want[0, 0] == 0.0 and want[n_src - 1, n_dst - 1] > 0.0       # '' -> '' and the 64 against the 64 are in the data


def test_the_data_tells_the_equal_character_rule_and_the_operand_order_apart():
    """What the random-cost cases can catch, asserted on the oracle: the other equal-characters rule, src and dst swapped, and
    ins / del swapped each change at least one entry of the (65, 5) case."""
    rng = np.random.default_rng(65 * 1000 + 5)
    ins, dele, sub = random_costs(12, rng)
    src, dst = make_words(65, 12, rng, True), make_words(5, 12, rng, True)
    want = ref.matrix_ids(src, dst, ins, dele, sub)
    costs = ref.Tables(ins, dele, sub)
    assert any(ref.lev_full_min(a, b, costs) != want[p, q] for p, a in enumerate(src) for q, b in enumerate(dst) if len(a) < 10)
    assert (ref.matrix_ids(dst, src, ins, dele, sub).T != want).any()
    assert (ref.matrix_ids(src, dst, dele, ins, sub) != want).any() and (ref.matrix_ids(src, dst, ins, dele, sub.T.copy()) != want).any()


@pytest.mark.parametrize("kind", ["uniform", "reference"])
def test_uniform_and_reference_costs_on_word_shapes(kind):
    costs = ref.uniform() if kind == "uniform" else ref.reference()
    rng = np.random.default_rng(7)
    signs = "wx.,%-()/"
    def words(n):
        out = ["".join(signs[i] for i in rng.integers(0, len(signs), size=int(rng.choice(LENGTHS)))) for _ in range(n)]
        return out + ["x.x%", "", "w" * 63, "x," * 32]
    src, dst = words(66), words(70)
    alphabet, tables, (src_ids, dst_ids) = ref.compact(costs, src, dst)
    want = ref.matrix(src, dst, costs)
    np.testing.assert_array_equal(run(src_ids, dst_ids, tables).cpu().numpy(), want)
    assert want[src.index("x.x%"), dst.index("")] == (4.0 if kind == "uniform" else 5.5)
    # the package's own tables over the same alphabet give the same distances
    lev = L.LevenshteinSimilitudes()
    own = (lev if kind == "uniform" else lev.init_weights()).tables([ord(c) for c in alphabet])
    np.testing.assert_array_equal(run(src_ids, dst_ids, own).cpu().numpy(), want)


def test_an_alphabet_of_one_character():
    rng = np.random.default_rng(11)
    tables = (np.array([0.7]), np.array([1.3]), np.array([[2.9]]))
    src, dst = make_words(9, 1, rng, True), make_words(70, 1, rng, True)
    want = ref.matrix_ids(src, dst, *tables)
    np.testing.assert_array_equal(run(src, dst, tables).cpu().numpy(), want)
    assert want[0, 0] == 0.0 and abs(want[0, 69] - 64 * 0.7) < 1e-9        # '' -> '' and '' -> 64 characters: inserts only


def test_an_alphabet_of_1024_characters_with_astral_code_points():
    """The cap of the tables: ids up to 1023, sub_cost 8 MB.  The ids come from the package's own compaction of code points
    that include astral ones."""
    rng = np.random.default_rng(13)
    points = [0x20 + i for i in range(500)] + [0x4E00 + i for i in range(400)] + [0xFEFF] + [0x1D400 + i for i in range(123)]
    assert len(points) == 1024
    def words(n):
        out = ["".join(chr(points[i]) for i in rng.integers(0, 1024, size=int(rng.choice(LENGTHS)))) for _ in range(n)]
        return out + ["".join(chr(p) for p in points[k:k + 64]) for k in (0, 960)]
    src, dst = words(20), words(66)
    everything = ["".join(chr(p) for p in points[k:k + 64]) for k in range(0, 1024, 64)]      # every id appears
    alphabet = L.alphabet_of(src, dst + everything)
    assert alphabet == sorted(points)
    tables = random_costs(1024, rng)
    (sc, so), (dc, do) = L.encode(src, alphabet), L.encode(dst + everything, alphabet)
    ids = lambda chars, off: [list(map(int, chars[off[i]:off[i + 1]])) for i in range(len(off) - 1)]      # noqa: E731
    want = ref.matrix_ids(ids(sc, so), ids(dc, do), *tables)
    got = G.lev_matrix(dev(sc), dev(so), dev(dc), dev(do), *(dev(t) for t in tables))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert int(sc.max()) >= 1000 and int(dc.max()) == 1023


def test_out_with_a_row_stride_leaves_the_padding_untouched():
    rng = np.random.default_rng(17)
    tables = random_costs(12, rng)
    src, dst = make_words(66, 12, rng, True), make_words(67, 12, rng, True)
    want = ref.matrix_ids(src, dst, *tables)
    wide = torch.full((66, 80), -7.0, dtype=torch.float64, device=DEV)
    got = run(src, dst, tables, out=wide[:, 5:72])
    assert got.data_ptr() == wide[:, 5:72].data_ptr()
    host = wide.cpu().numpy()
    np.testing.assert_array_equal(host[:, 5:72], want)
    np.testing.assert_array_equal(host[:, :5], -7.0)
    np.testing.assert_array_equal(host[:, 72:], -7.0)


def test_max_len_cuts_longer_words():
    rng = np.random.default_rng(19)
    tables = random_costs(12, rng)
    src, dst = make_words(5, 12, rng, False) + [[3] * 20], make_words(6, 12, rng, False) + [[4] * 30]
    want = ref.matrix_ids([w[:4] for w in src], [w[:4] for w in dst], *tables)
    np.testing.assert_array_equal(run(src, dst, tables, max_len=4).cpu().numpy(), want)


def test_limits_are_unsupported_and_empty_lists_give_empty_tensors():
    rng = np.random.default_rng(23)
    src, dst = make_words(3, 12, rng, False), make_words(4, 12, rng, False)
    tables = random_costs(12, rng)
    with pytest.raises(_lib.GteError, match=r"\(-4\)"):
        run(src, dst, tables, max_len=65)
    with pytest.raises(_lib.GteError, match=r"\(-4\)"):
        run(src, dst, random_costs(1025, rng))
    assert tuple(run([], dst, tables).shape) == (0, 4) and tuple(run(src, [], tables).shape) == (3, 0)
    assert run([[]], [[]], tables).cpu().tolist() == [[0.0]]


def test_wrapper_checks_raise_before_the_call():
    rng = np.random.default_rng(29)
    ins, dele, sub = (dev(t) for t in random_costs(12, rng))
    (sc, so), (dc, do) = pack(make_words(3, 12, rng, False) + [[1]]), pack(make_words(4, 12, rng, False) + [[2]])
    sc, so, dc, do = dev(sc), dev(so), dev(dc), dev(do)
    with pytest.raises(ValueError, match="uint16"):
        G.lev_matrix(sc.to(torch.int32), so, dc, do, ins, dele, sub)
    with pytest.raises(ValueError, match="int32"):
        G.lev_matrix(sc, so.to(torch.int64), dc, do, ins, dele, sub)
    with pytest.raises(ValueError, match="float64"):
        G.lev_matrix(sc, so, dc, do, ins.float(), dele, sub)
    with pytest.raises(ValueError, match="do not fit together"):
        G.lev_matrix(sc, so, dc, do, ins, dele[:11], sub)
    with pytest.raises(ValueError, match="do not fit together"):
        G.lev_matrix(sc, so, dc, do, ins, dele, sub[:, :11])
    with pytest.raises(ValueError, match="out must be"):
        G.lev_matrix(sc, so, dc, do, ins, dele, sub, out=torch.empty((4, 4), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="ends at"):
        G.lev_matrix(sc[:-1], so, dc, do, ins, dele, sub)                  # offsets that pass the end of the characters
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        G.lev_matrix(sc.cpu(), so, dc, do, ins, dele, sub)
