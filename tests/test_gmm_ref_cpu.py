"""tests/gmm_ref.py -- the numpy oracle of the Gaussian-mixture kernels, written from the contract in include/gte.h -- pinned on
scikit-learn 1.7.2: the soft fit on ``GaussianMixture``, the hard fit on a small subclass that the contract's hard variant
describes (tests/gmm_ref.py: sklearn_estimator).  No GPU.

The tolerance is measured, not fixed: summation order alone moves scikit-learn's own result (the fit of ``x[::-1]`` against the fit
of ``x``) by d per case (tests/golden/gmm_sensitivity.json, tools/make_gmm_golden.py); ``1000 * max(d, eps)`` is allowed.  EM is
contractive near its fixed point, so the difference stays a small multiple of one step's rounding; a formula error shows at 1e-3."""
import warnings

import numpy as np
import pytest

from tests import gmm_ref as ref

sklearn = pytest.importorskip("sklearn")
TOL = 1e-3


@pytest.fixture(scope="module", params=sorted(ref.FIT_CASES))
def case(request):
    return (request.param,) + ref.fit_case(request.param)


@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_the_oracle_fits_as_scikit_learn_does(case, kind):
    name, x, w, mu, prec = case
    K = w.shape[0]
    hard = kind == "hard"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sk = ref.sklearn_estimator(hard, K, w, mu, prec, tol=TOL).fit(x.reshape(-1, 1))
    # the condition on every fit case: no stop can flip on rounding
    assert all(abs(abs(c) - TOL) > 1e-6 for c in sk.changes_), sk.changes_
    mine = ref.fit(x, w, mu, prec, hard=hard, tol=TOL)
    assert (mine["n_iter"], mine["converged"], mine["error"]) == (sk.n_iter_, sk.converged_, False)
    bound = ref.fit_tolerance(name, kind)
    got = {"weights": ref.rel_diff(mine["P"][0], sk.weights_), "means": ref.rel_diff(mine["P"][1], sk.means_),
           "covariances": ref.rel_diff(mine["P"][2], sk.covariances_), "pc": ref.rel_diff(mine["P"][3], sk.precisions_cholesky_),
           "lower_bound": ref.rel_diff([mine["lower_bound"]], [sk.lower_bound_])}
    print(name, kind, "bound", bound, got)
    assert max(got.values()) <= bound, (got, bound)


def test_the_measured_sensitivity_is_what_scikit_learn_shows_here(case):
    """The golden d is of the order this machine's scikit-learn shows (within a factor of 1000 either way: BLAS builds differ in
    their order, not in kind), and small: the bound stays many orders below a formula error."""
    name, x, w, mu, prec = case
    K = w.shape[0]
    a = ref.sklearn_estimator(False, K, w, mu, prec, tol=TOL).fit(x.reshape(-1, 1))
    b = ref.sklearn_estimator(False, K, w, mu, prec, tol=TOL).fit(x[::-1].copy().reshape(-1, 1))
    d = max(ref.rel_diff(b.weights_, a.weights_), ref.rel_diff(b.means_, a.means_), ref.rel_diff(b.covariances_, a.covariances_),
            ref.rel_diff([b.lower_bound_], [a.lower_bound_]))
    assert d <= 1000 * max(ref.sensitivity()[name]["soft"], ref.EPS)
    assert ref.fit_tolerance(name, "soft") < 1e-8 and ref.fit_tolerance(name, "hard") < 1e-8


def test_the_hard_subclass_does_not_raise_on_an_empty_component():
    """nk = 10 eps, mean 0, covariance reg_covar: scikit-learn 1.7.2 runs through, and so does the oracle."""
    x = np.array([1.0, 1.1, 0.9, 1.05, 5.0, 5.1, 4.9, 5.2])
    w, mu, prec = np.array([0.4, 0.4, 0.2]), np.array([1.0, 5.0, 100.0]), np.array([1.0, 1.0, 1.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = ref.sklearn_estimator(True, 3, w, mu, prec, max_iter=3).fit(x.reshape(-1, 1))
    mine = ref.fit(x, w, mu, prec, hard=True, max_iter=3)
    assert not mine["error"] and mine["n_iter"] == sk.n_iter_
    assert mine["P"][1][2] == 0.0 and sk.means_[2, 0] == 0.0
    assert mine["P"][2][2] == 1e-6 and sk.covariances_[2, 0, 0] == 1e-6
    assert mine["P"][0][2] == pytest.approx(10 * ref.EPS / 8, rel=1e-12) and sk.weights_[2] == pytest.approx(10 * ref.EPS / 8, rel=1e-12)
    np.testing.assert_allclose(mine["P"][1], sk.means_.reshape(-1), rtol=1e-13)


def test_step_exact_is_extended_precision_and_agrees():
    if not np.finfo(np.longdouble).eps < 2e-19:
        pytest.skip("np.longdouble is not the 80-bit format here")
    x, w, mu, prec = ref.fit_case("n257_k3")
    P0 = ref.initial_block(w, mu, prec)
    for hard in (False, True):
        P, lb, _ = ref.step(x, P0, hard)
        Pe, lbe, _ = ref.step_exact(x, P0, hard)
        assert Pe.dtype == np.longdouble
        assert ref.rel_diff(P, Pe.astype(np.float64)) < 1e-12 and abs(lb - float(lbe)) < 1e-12
