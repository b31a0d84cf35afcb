"""tests/repr_ref.py against the reference's recorded ``Repr.__call__`` outputs (tests/golden/repr_cases.json, written by
tools/make_repr_golden.py): hard mode equal, combined mode within the rounding bound of a C-term float32 dot product of
float32-rounded factors, (C + 3) * 2^-24 * sum_c |q_c * p_cj| per element -- derived, not measured."""
import numpy as np
import pytest

from gnn_tableextraction_amd.components.nlp.repr import Repr
from tests import repr_ref as ref

DATA = ref.golden()


def node_tokens(case):
    emb = Repr(case["repr2idx"], case["embeddings"], case["prototypes"], case["i_embedding"], device="cpu")
    return emb.token_ids(case["pages"])


@pytest.mark.parametrize("case", DATA["sets"], ids=[s["name"] for s in DATA["sets"]])
def test_every_set_is_separated_or_tied(case):
    assert ref.separated_or_tied(case["embeddings"], case["prototypes"])


def test_the_condition_itself():
    zero = np.zeros((1, 1))
    assert not ref.separated_or_tied(zero, np.array([[2e-4], [2e-4 * (1 + 1e-12)]]))     # neither tied nor apart
    assert ref.separated_or_tied(zero, np.array([[2e-4], [2e-4]]))                       # bit-equal
    assert ref.separated_or_tied(zero, np.array([[1e-5], [0.0], [3.0]]))                 # both clamp to the margin
    assert ref.separated_or_tied(zero, np.array([[2e-4], [2e-4 * (1 + 1e-8)]]))


@pytest.mark.parametrize("combined", [False, True], ids=["hard", "combined"])
@pytest.mark.parametrize("case", DATA["sets"], ids=[s["name"] for s in DATA["sets"]])
def test_restatement_equals_the_recorded_reference_outputs(case, combined):
    tok = node_tokens(case)
    want, bound = ref.features(tok, case["embeddings"], case["prototypes"], case["i_embedding"], 1.0, combined)
    recorded = case["combined" if combined else "hard"]
    sizes = [len(p) for p in case["pages"]]
    assert len(recorded) == len(sizes) and want.shape == (sum(sizes), case["i_embedding"].shape[1])
    o = 0
    for rows, n in zip(recorded, sizes):
        assert len(rows) <= n
        got = rows.astype(np.float64)
        if combined:
            assert np.all(np.abs(got - want[o:o + len(rows)]) <= bound[o:o + len(rows)])
            assert np.all(bound[o:o + len(rows)][tok[o:o + len(rows)] >= 0] > 0)
        else:
            np.testing.assert_array_equal(got, want[o:o + len(rows)])
        assert np.all(want[o + len(rows):o + n] == 0)                    # nodes beyond the reference's tensor: no token
        o += n


def test_the_tie_set_chooses_the_lowest_index():
    case = [s for s in DATA["sets"] if s["name"].startswith("integer_ties")][0]
    emb, cen = case["embeddings"], case["prototypes"]
    t = ref.clamped_distances(emb[1:4], cen)
    assert np.count_nonzero(t[0] == 1e-4) == 3 and t[0].min() == 1e-4    # three centres inside the margin, one of them exact
    assert np.flatnonzero(t[0] == 1e-4).tolist() == [2, 5, 7] and np.array_equal(cen[5], emb[1])
    assert np.array_equal(cen[3], cen[9]) and t[1, 3] == t[1].min()       # duplicates
    assert t[2, 0] == t[2, 4] == t[2].min() and not np.array_equal(cen[0], cen[4])
    assert ref.chosen_centre([1, 2, 3, -1], emb, cen).tolist() == [2, 3, 0, -1]
    # the recorded reference rows name the same centres: row c of this set's table is c * P + j
    tok = node_tokens(case)
    p = case["i_embedding"].shape[1]
    flat = np.concatenate(case["hard"])
    assert flat.shape[0] == tok.shape[0]
    for want_c, token in ((2, 1), (3, 2), (0, 3)):
        rows = flat[tok == token]
        assert len(rows) > 0 and np.all(rows[:, 0] == want_c * p)
