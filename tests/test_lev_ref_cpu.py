"""The weighted Levenshtein oracle (tests/lev_ref.py) on hand cases under the reference's costs (tests/golden/lev_cases.json), its
two evaluations against each other, and the proof that random costs tell the recurrence's equal-characters rule (a copy, no
minimum) from "substitution cost 0".  Nothing here needs a GPU or the library."""
import random

import numpy as np
import pytest

from tests import lev_ref as ref

DATA = ref.golden()


@pytest.mark.parametrize("case", DATA["pairs"], ids=[f"{i}" for i in range(len(DATA["pairs"]))])
def test_hand_cases_under_the_reference_costs(case):
    costs = ref.reference()
    assert ref.lev(case["src"], case["dst"], costs) == case["distance"], case
    assert ref.matrix([case["src"]], [case["dst"]], costs)[0, 0] == case["distance"], case


def test_the_hand_cases_cover_what_they_should():
    pairs = {(c["src"], c["dst"]): c["distance"] for c in DATA["pairs"]}
    assert len(pairs) == 11
    assert pairs[("x", "%")] == 2.5 and pairs[("%", "x")] == 1.0              # the one-way override, beaten by delete + insert
    assert pairs[("", "x.x%")] == pairs[("x.x%", "")] == 5.5                  # an empty word on either side
    assert pairs[("x", "\ufeffx")] == 1.0


@pytest.mark.parametrize("case", DATA["similarities"], ids=["one_way", "bom"])
def test_similarity_is_negated_transposed_and_strips_only_the_first_argument(case):
    got = ref.similarity(case["words"], ref.reference())
    np.testing.assert_array_equal(got, np.asarray(case["matrix"], dtype=np.float64))
    if "\ufeff" in case["words"][0]:
        assert got[0, 0] == -1.0                                             # a word with U+FEFF: non-zero on the diagonal


def random_tables(n_alpha, seed):
    rng = np.random.RandomState(seed)
    return rng.uniform(0.1, 5.0, n_alpha), rng.uniform(0.1, 5.0, n_alpha), rng.uniform(0.1, 5.0, (n_alpha, n_alpha))


def test_random_costs_tell_the_two_equal_character_rules_apart():
    ins, dele, sub = random_tables(4, 1)
    costs = ref.Tables(ins, dele, sub)
    rnd = random.Random(1)
    differ = 0
    for _ in range(3000):
        a = [rnd.randrange(4) for _ in range(rnd.randint(0, 6))]
        b = [rnd.randrange(4) for _ in range(rnd.randint(0, 6))]
        differ += ref.lev(a, b, costs) != ref.lev_full_min(a, b, costs)
    assert differ >= 1, "the data cannot tell 'copy the diagonal' from 'substitution cost 0'"
    # under uniform costs the two rules agree: it takes uneven costs to see the difference
    assert all(ref.lev(w, v, ref.uniform()) == ref.lev_full_min(w, v, ref.uniform()) for w in ("", "ab", "abca") for v in ("b", "cab", "aa"))


def test_both_evaluations_of_the_oracle_agree_bit_for_bit():
    ins, dele, sub = random_tables(5, 2)
    rnd = random.Random(2)
    src = [[rnd.randrange(5) for _ in range(rnd.choice((0, 1, 2, 5, 9)))] for _ in range(23)] + [[]]
    dst = [[rnd.randrange(5) for _ in range(rnd.choice((0, 1, 3, 7, 12)))] for _ in range(17)] + [[]]
    got = ref.matrix_ids(src, dst, ins, dele, sub)
    costs = ref.Tables(ins, dele, sub)
    want = np.array([[ref.lev(a, b, costs) for b in dst] for a in src])
    np.testing.assert_array_equal(got, want)
    assert (got != got.T[:got.shape[0], :got.shape[1]]).any() if got.shape[0] == got.shape[1] else True
    assert ref.matrix_ids([], dst, ins, dele, sub).shape == (0, 18) and ref.matrix_ids(src, [], ins, dele, sub).shape == (24, 0)
    assert ref.matrix([""], ["", ""], ref.reference()).tolist() == [[0.0, 0.0]]
