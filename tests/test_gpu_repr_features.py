"""gte_repr_features against tests/repr_ref.py (float64 numpy, pinned on the reference's recorded outputs by
tests/test_repr_ref_cpu.py).  Hard mode must match exactly -- the values, and the chosen centre recovered from a prototype table whose
row c is c * P + j; combined mode within (C + 3) * 2^-24 * sum_c |q_c * p_cj| per element, the rounding bound of a C-term float32
dot product of float32-rounded factors.

Shapes: one centre per lane up to 64 (C = 1, 2, 33, 47, 63, 64); D = 1, 3, 50, the staging chunk 64 and 65 / 130 above it (the centres
are then restaged for every word); P = 1, 50 and 70 / 130 above a wave; N = 1, 63, 65, 1000 and 8200, above the 2048 workgroups x 4
words of one pass of the grid-stride loop.  Every input satisfies, asserted before the device is touched, that the two best clamped
distances of every vocabulary row are bit-equal or more than 1e-9 apart."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from tests import repr_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = 40
#        C   D    P    N
SHAPES = [(1, 1, 1, 1), (2, 3, 50, 63), (33, 50, 50, 65), (47, 50, 50, 1000), (63, 3, 70, 65), (64, 1, 50, 63), (64, 64, 1, 65),
          (47, 65, 130, 1000), (64, 130, 50, 8200), (47, 50, 50, 8200)]


def make_case(c, d, p, n, seed):
    rng = np.random.default_rng(seed)
    emb, cen = rng.normal(size=(V, d)), rng.normal(size=(c, d))
    if c >= 4:
        cen[c - 1] = cen[1]                                              # a duplicate centre: bit-equal distances
        cen[2, 0] += 40.0                                                # far from every other row: never among their two best
        emb[0] = cen[2]                                                  # a row ON a centre ...
        cen[0] = cen[2] + 1e-5 / np.sqrt(d)                              # ... with an earlier centre inside the margin: it wins
    assert ref.separated_or_tied(emb, cen), (c, d)
    tok = rng.integers(0, V, size=n).astype(np.int32)
    tok[rng.random(n) < 0.1] = -1
    if n >= 8:
        tok[:4] = [0, 0, -1, 0]                                          # repeated ids
    return tok, emb, cen


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("c,d,p,n", SHAPES)
def test_hard_mode_is_exact(c, d, p, n):
    tok, emb, cen = make_case(c, d, p, n, seed=c * 1000 + d)
    names = (np.arange(c)[:, None] * p + np.arange(p)[None, :]).astype(np.float64)       # row c names its centre
    want_c = ref.chosen_centre(tok, emb, cen)
    got = G.repr_features(dev(tok), dev(emb), dev(cen), dev(names)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (n, p)
    has = tok >= 0
    np.testing.assert_array_equal(got[~has], 0)
    np.testing.assert_array_equal((got[has, 0] / p).astype(np.int64), want_c[has])
    if c >= 4 and (tok == 0).any():
        assert set(want_c[tok == 0]) == {0}                              # the margin case is in the data
    table = np.random.default_rng(3).normal(size=(c, p))                                 # and with values that float32 rounds
    want, bound = ref.features(tok, emb, cen, table)
    got = G.repr_features(dev(tok), dev(emb), dev(cen), dev(table), combined=False).cpu().numpy()
    assert not bound.any()
    np.testing.assert_array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("alpha", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("c,d,p,n", SHAPES)
def test_combined_mode_stays_within_the_rounding_bound(c, d, p, n, alpha):
    tok, emb, cen = make_case(c, d, p, n, seed=c * 1000 + d)
    table = np.random.default_rng(4).normal(size=(c, p))
    want, bound = ref.features(tok, emb, cen, table, alpha, combined=True)
    got = G.repr_features(dev(tok), dev(emb), dev(cen), dev(table), alpha=alpha, combined=True).cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(got[tok < 0], 0)
    err = np.abs(got - want)
    assert np.all(err <= bound), (float((err - bound).max()), float(err.max()))
    assert (tok < 0).all() or (bound[tok >= 0] > 0).all()


def test_the_tie_cases_of_the_fixture():
    case = [s for s in ref.golden()["sets"] if s["name"].startswith("integer_ties")][0]
    tok = np.array([1, 2, 3, 1, -1, 3], dtype=np.int32)
    got = G.repr_features(dev(tok), dev(case["embeddings"]), dev(case["prototypes"]), dev(case["i_embedding"])).cpu().numpy()
    p = case["i_embedding"].shape[1]
    # three centres inside the margin (the exact one is not the first), duplicate centres, two centres at one distance
    np.testing.assert_array_equal(got[:, 0], np.array([2, 3, 0, 2, 0, 0]) * p)
    np.testing.assert_array_equal(got, ref.features(tok, case["embeddings"], case["prototypes"], case["i_embedding"])[0])


def test_ids_that_name_no_row_write_zeros():
    tok, emb, cen = make_case(47, 50, 50, 65, seed=9)
    tok[5], tok[6], tok[64] = V, V + 1000, -7
    table = np.random.default_rng(5).normal(size=(47, 50))
    for combined in (False, True):
        got = G.repr_features(dev(tok), dev(emb), dev(cen), dev(table), combined=combined).cpu().numpy()
        valid = np.where((tok >= 0) & (tok < V), tok, -1)
        want, bound = ref.features(valid, emb, cen, table, combined=combined)
        np.testing.assert_array_equal(got[[5, 6, 64]], 0)
        assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("combined", [False, True])
def test_a_column_slice_of_a_wider_matrix_and_nothing_outside_it(combined):
    c, d, p, n = 47, 50, 50, 65
    tok, emb, cen = make_case(c, d, p, n, seed=11)
    table = np.random.default_rng(6).normal(size=(c, p))
    sentinel = -12345.5
    wide = torch.full((n, 13 + p + 3), sentinel, dtype=torch.float32, device=DEV)
    out = G.repr_features(dev(tok), dev(emb), dev(cen), dev(table), combined=combined, out=wide[:, 13:13 + p])
    assert out.data_ptr() == wide[:, 13:].data_ptr()
    got = wide.cpu().numpy()
    assert np.all(got[:, :13] == sentinel) and np.all(got[:, 13 + p:] == sentinel)
    want, bound = ref.features(tok, emb, cen, table, combined=combined)
    assert np.all(np.abs(got[:, 13:13 + p] - want) <= bound)
    with pytest.raises(ValueError, match="unit column stride"):
        G.repr_features(dev(tok), dev(emb), dev(cen), dev(table), out=wide[:, 0:2 * p:2])
    with pytest.raises(ValueError, match="float64 matrix"):
        G.repr_features(dev(tok), dev(emb).float(), dev(cen), dev(table))
    with pytest.raises(ValueError, match="do not fit together"):
        G.repr_features(dev(tok), dev(emb), dev(cen[:, :3]), dev(table))


def test_a_non_default_stream_and_an_empty_batch():
    tok, emb, cen = make_case(47, 50, 50, 1000, seed=12)
    table = np.random.default_rng(7).normal(size=(47, 50))
    args = [dev(a) for a in (tok, emb, cen, table)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = G.repr_features(*args)
    stream.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), ref.features(tok, emb, cen, table)[0])
    empty = G.repr_features(args[0][:0], *args[1:])
    assert tuple(empty.shape) == (0, 50)
    with pytest.raises(_lib.GteError, match="limits"):
        G.repr_features(args[0], args[1], torch.zeros((65, 50), dtype=torch.float64, device=DEV),
                        torch.zeros((65, 50), dtype=torch.float64, device=DEV))
