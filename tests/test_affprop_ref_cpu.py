"""tests/affprop_ref.py pinned on scikit-learn itself: for every case of the GPU test, ``cluster_centers_indices_``, ``labels_``
and ``n_iter_`` of ``AffinityPropagation(affinity='precomputed', ..., random_state=7).fit(S)`` equal what the reference computes
from the contract of include/gte.h.  No GPU."""
import warnings

import numpy as np
import pytest

from tests import affprop_ref as ref

pytest.importorskip("sklearn")


def sklearn_fit(case):
    from sklearn.cluster import AffinityPropagation
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = AffinityPropagation(affinity="precomputed", damping=case.damping, convergence_iter=case.ci, max_iter=case.max_iter,
                                  preference=case.pref(), random_state=ref.SEED).fit(case.S())
    return np.asarray(est.cluster_centers_indices_, dtype=np.intp), est.labels_, est.n_iter_


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.id)
def test_reference_equals_scikit_learn(case):
    want_centers, want_labels, want_n_iter = sklearn_fit(case)
    last = case.reference()[case.max_iter]
    centers, labels = ref.finish(case.noisy(), last["E"])
    print(case.id, "n_iter", last["state"][0], "converged", last["state"][2], "K", last["state"][3])
    assert last["state"][0] == want_n_iter
    np.testing.assert_array_equal(centers, want_centers)
    np.testing.assert_array_equal(labels, want_labels)
    assert last["state"][1] == 1                                           # stopped, one way or the other
    # the wrapper of the reference gives the same from the raw matrix
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c2, l2, n2 = ref.affinity_propagation(case.S(), case.pref(), case.ci, case.max_iter, case.damping, ref.SEED)
    np.testing.assert_array_equal(c2, want_centers)
    np.testing.assert_array_equal(l2, want_labels)
    assert n2 == want_n_iter


def test_the_case_list_holds_what_it_is_meant_to_hold():
    ends = {c.id: c.reference()[c.max_iter]["state"] for c in ref.CASES}
    # both endings occur in the grid, and converged runs of different lengths
    grid = [ends[c.id] for c in ref.GRID]
    assert any(s[2] == 1 for s in grid) and len({s[0] for s in grid if s[2] == 1}) > 5
    for case in ref.CUT_SHORT:                                             # cut short: the same problem needs more sweeps
        full = ref.Case(case.family, case.n, case.damping, case.ci).reference()[200]["state"]
        assert full[2] == 1 and full[0] > case.max_iter
        assert ends[case.id][:3] == [case.max_iter, 1, 0] and ends[case.id][3] > 0
    for case in ref.NO_EXEMPLAR:
        assert ends[case.id] == [case.max_iter, 1, 0, 0]
    for case in ref.TWO:
        assert ends[case.id][2] == 1


def test_degenerate_inputs_as_scikit_learn_answers_them():
    from sklearn.cluster import AffinityPropagation
    for S, pref in ((np.array([[-2.0]]), None), (np.full((4, 4), -1.0), -5.0), (np.full((4, 4), -1.0), 0.0),
                    (np.array([[0.0, -2.0], [-2.0, 0.0]]), -2.0)):
        with pytest.warns(UserWarning, match="mutually equal"):
            est = AffinityPropagation(affinity="precomputed", preference=pref, random_state=0).fit(S)
        with pytest.warns(UserWarning, match="mutually equal"):
            noisy, (centers, labels, n_iter) = ref.prepare(S, pref, 0)
        assert noisy is None and n_iter == est.n_iter_ == 0
        np.testing.assert_array_equal(centers, est.cluster_centers_indices_)
        np.testing.assert_array_equal(labels, est.labels_)
