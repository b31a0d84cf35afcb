"""gte_gmm_iterate / gte_gmm_posterior and components/tables/gmm.py against tests/gmm_ref.py (the contract of include/gte.h in numpy
float64, pinned on scikit-learn by tests/test_gmm_ref_cpu.py) and its np.longdouble twin ``step_exact``.

Bounds.  One iteration: per case ``4 x`` the error that the numpy float64 oracle itself shows against ``step_exact`` on that case,
with a floor of ``(L(n) + 8) * eps`` relative, L(n) = 23 + ceil(ceil(n / gte_gmm_workgroup_samples()) / 64) the longest addition
chain of the kernels (csrc/gmm.hip).  The error of ``exp(wlp - lse)`` is ``eps * |wlp|``-conditioned and hits numpy and the device
alike; the factor covers the device's 1 - 2 ulp exp / log and its different chain.  Whole fits: ``1000 * max(d, eps)``, d the
measured sensitivity of scikit-learn's own fit to the sample order (tests/golden/gmm_sensitivity.json).

Sizes of the one-iteration cases: 2; below / at / above one wave (63, 64, 65) and one row of lanes (255, 256, 257); one, two and
three workgroups' worth of samples, each - 1, + 0, + 1 (the count is the library's: gte_gmm_workgroup_samples()).  The step cases
use positive samples, so no sum cancels and entrywise relative errors are meaningful; empty components (hard mode, K = 64) give an
exact 0 mean and ``reg_covar`` on both sides."""
import functools
import os
import pickle
import sys
import warnings

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.components.tables import gmm as M, preprocessor as P
from tests import gmm_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = ref.EPS
WG = _lib.load().gte_gmm_workgroup_samples()
STEP_N = [2, 63, 64, 65, 255, 256, 257] + [g * WG + o for g in (1, 2, 3) for o in (-1, 0, 1)]
STEP_K = [1, 2, 20, 64]
INIT_STATE = [0, 0, 0, 0, -np.inf, -np.inf, 0, 0]


def chain(n):
    return 23 + -(-(-(-n // WG)) // 64)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(DEV)   # (a copy: the shared inputs are read-only)


def device_iterations(x, P0, hard=False, tol=0.0, reg_covar=1e-6, max_iter=1, n_iters=None):
    """-> (P [4, K], state [8]) after ``n_iters`` (default: max_iter) enqueued iterations from ``P0``."""
    xd, Pd = dev(x), dev(P0)
    ws = G.gmm_workspace(x.shape[0], P0.shape[1], DEV)
    state = torch.tensor(INIT_STATE, dtype=torch.float64, device=DEV)
    G.gmm_iterate(xd, Pd, hard, tol, reg_covar, max_iter, max_iter if n_iters is None else n_iters, ws, state)
    return Pd.cpu().numpy(), state.cpu().numpy()


def device_labels(x, P0):
    return G.gmm_posterior(dev(x), dev(P0), resp=False, label=True)[2].cpu().numpy()


@functools.lru_cache(maxsize=None)
def step_case(n, K):
    """Positive samples around a few centres and a plausible parameter block with broad components (|wlp| stays in the tens)."""
    rng = np.random.RandomState(1000 * K + n % 997)
    centres = rng.uniform(2.0, 40.0, size=4)
    x = np.abs(centres[rng.randint(4, size=n)] + 1.5 * rng.standard_normal(n)) + 0.5
    w = rng.uniform(0.5, 1.5, size=K)
    w = w / w.sum()
    mu = np.sort(rng.uniform(1.0, 42.0, size=K))
    sigma = rng.uniform(3.0, 6.0, size=K)
    P0 = np.stack([w, mu, sigma ** 2, 1.0 / sigma])
    x.setflags(write=False)
    P0.setflags(write=False)
    return x, P0


# ---- one iteration at the edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", STEP_N)
def test_one_iteration_against_the_extended_precision_step(n):
    if not np.finfo(np.longdouble).eps < 2e-19:
        pytest.skip("np.longdouble is not the 80-bit format here")
    floor = (chain(n) + 8) * EPS
    for K in STEP_K:
        if n < K:
            continue
        x, P0 = step_case(n, K)
        for hard in (False, True):
            Pe, lbe, label_e = ref.step_exact(x, P0, hard)
            Pn, lbn, label_n = ref.step(x, P0, hard)
            assert (label_n == label_e).all()                              # no label of the case hangs on float64 rounding
            Pd, state = device_iterations(x, P0, hard)
            assert state[:4].tolist() == [1, 0, 0, 0] and state[5] == -np.inf and state[6] == np.inf
            if hard:
                assert (device_labels(x, P0) == label_n).all()
            Pe64, lbe64 = Pe.astype(np.float64), float(lbe)
            for q, name in enumerate(("weights", "means", "covariances")):
                e_np, e_dev = ref.rel_diff(Pn[q], Pe64[q]), ref.rel_diff(Pd[q], Pe64[q])
                bound = max(4 * e_np, floor)
                print(f"gmm step n={n} K={K} {'hard' if hard else 'soft'} {name}: device {e_dev / EPS:.1f} eps, numpy {e_np / EPS:.1f} eps, "
                      f"bound {bound / EPS:.1f} eps")
                assert e_dev <= bound, (n, K, hard, name, e_dev, bound)
            e_np, e_dev = ref.rel_diff([lbn], [lbe64]), ref.rel_diff([state[4]], [lbe64])
            bound = max(4 * e_np, floor)
            print(f"gmm step n={n} K={K} {'hard' if hard else 'soft'} lb: device {e_dev / EPS:.1f} eps, numpy {e_np / EPS:.1f} eps, "
                  f"bound {bound / EPS:.1f} eps")
            assert e_dev <= bound, (n, K, hard, "lb", e_dev, bound)
            assert Pd[3].tolist() == (1.0 / np.sqrt(Pd[2])).tolist()       # pc = 1 / sqrt(cov): correctly rounded operations on both sides


# ---- ill-conditioned data ----------------------------------------------------------------------------------------------------------------
def test_large_offsets_with_a_tiny_spread_need_the_two_pass_covariance():
    """Samples at 1e6 and 1e6 + 1 with spread 1e-2.  A one-pass ``sum r x^2 - nk mean^2`` loses everything (eps * 1e12 against 1e-4).
    Two passes: the mean carries at most delta = (L + 8) eps 1e6 of error, which enters the covariance as
    2 (delta / sigma) |sum r d| / (nk sigma) + (delta / sigma)^2 <= 2 (delta / sigma) + (delta / sigma)^2, next to the sum's own
    (L + 8) eps."""
    rng = np.random.RandomState(5)
    n, sigma = 3001, 1e-2
    x = 1e6 + rng.randint(2, size=n) + sigma * rng.standard_normal(n)
    P0 = np.array([[0.5, 0.5], [1e6, 1e6 + 1.0], [1e-3, 1e-3], [1e-3 ** -0.5, 1e-3 ** -0.5]])
    Pe, lbe, _ = ref.step_exact(x, P0, reg_covar=0.0)
    Pd, state = device_iterations(x, P0, reg_covar=0.0)
    assert state[3] == 0
    floor = (chain(n) + 8) * EPS
    ds = floor * 1e6 / sigma
    e_mean, e_cov = ref.rel_diff(Pd[1], Pe[1].astype(np.float64)), ref.rel_diff(Pd[2], Pe[2].astype(np.float64))
    print(f"gmm offsets: mean {e_mean / EPS:.1f} eps, covariance {e_cov:.3e} (bound {floor + 2 * ds + ds * ds:.3e})")
    assert e_mean <= floor and e_cov <= floor + 2 * ds + ds * ds
    assert np.all(np.abs(np.sqrt(Pd[2]) - sigma) < 0.1 * sigma)


@pytest.mark.parametrize("hard", [False, True])
def test_equal_samples_give_exactly_reg_covar(hard):
    x = np.full(500, 3.7)
    P0 = np.array([[0.3, 0.7], [3.0, 4.0], [1.0, 1.0], [1.0, 1.0]])
    Pd, state = device_iterations(x, P0, hard)
    assert state[3] == 0 and Pd[2].tolist() == [1e-6, 1e-6] and Pd[3].tolist() == [1.0 / np.sqrt(1e-6)] * 2


def test_an_empty_component_is_no_error():
    rng = np.random.RandomState(6)
    x = 5.0 + rng.standard_normal(2000)
    P0 = np.array([[0.5, 0.3, 0.2], [4.0, 6.0, 1e4], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]])      # exp(-5e7) is 0: component 2 owns nothing
    for hard in (False, True):
        Pd, state = device_iterations(x, P0, hard, max_iter=2)
        assert state[:4].tolist() == [2, 0, 0, 0] and np.isfinite(Pd).all()
        assert 0.9e-18 < Pd[0, 2] < 1.3e-18 and Pd[1, 2] == 0.0 and Pd[2, 2] == 1e-6             # 10 eps / n, 0 / nk, 0 / nk + reg_covar


def test_an_outlier_at_1e30_underflows_without_a_nan():
    rng = np.random.RandomState(7)
    x = np.concatenate([5.0 + rng.standard_normal(700), [1e30]])
    P0 = np.array([[0.5, 0.3, 0.2], [4.0, 6.0, 9.0], [1.0, 1.0, 4.0], [1.0, 1.0, 0.5]])
    resp, lse, _ = (t.cpu().numpy() for t in G.gmm_posterior(dev(x), dev(P0), resp=True, lse=True, label=True))
    assert np.isfinite(resp).all() and np.isfinite(lse).all() and lse[-1] < -1e58
    assert sorted(resp[-1].tolist()) == [0.0, 0.0, 1.0]                    # the broadest component takes it, the others underflow
    for hard in (False, True):
        Pd, state = device_iterations(x, P0, hard)
        assert state[3] == 0 and np.isfinite(Pd).all() and np.isfinite(state).sum() == 6       # (prev = -inf, change = +inf)
        assert abs(Pd[0].sum() - 1.0) <= 3 * EPS and Pd[1].max() > 1e26


def test_identical_components_tie_to_the_first_index():
    rng = np.random.RandomState(8)
    x = np.concatenate([2.0 + 0.5 * rng.standard_normal(300), 9.0 + rng.standard_normal(341)])
    P0 = np.array([[0.25, 0.25, 0.25, 0.25], [2.0, 2.0, 9.0, 9.0], [0.25, 0.25, 1.0, 1.0], [2.0, 2.0, 1.0, 1.0]])
    want = ref.e_step(x, P0, hard=True)[2]
    got = device_labels(x, P0)
    assert (got == want).all() and set(got.tolist()) == {0, 2}
    Pd, state = device_iterations(x, P0, hard=True)
    Pn, _, _ = ref.step(x, P0, hard=True)
    assert Pd[0, 1] == Pn[0, 1] == 10 * EPS / x.shape[0] and Pd[0, 3] == Pn[0, 3]
    assert Pd[0, 0] == np.count_nonzero(want == 0) / x.shape[0]             # counts are exact: nk / n is one division


# ---- the stop ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_fit(name, hard, max_iter=100):
    x, w, mu, prec = ref.fit_case(name)
    return ref.fit(x, w, mu, prec, hard=hard, max_iter=max_iter)


@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_the_fit_stops_where_the_oracle_stops(kind):
    x, w, mu, prec = ref.fit_case("n257_k3")
    want = reference_fit("n257_k3", kind == "hard")
    assert want["converged"] and 3 <= want["n_iter"] <= 7
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = M.gaussian_mixture(x, w, mu, prec, hard=kind == "hard", device=DEV)
    assert (got.n_iter_, got.converged_) == (want["n_iter"], True)
    assert got.means_.shape == (3, 1) and got.covariances_.shape == (3, 1, 1) and got.precisions_cholesky_.shape == (3, 1, 1)
    # out of iterations: the warning, scikit-learn's text
    short = reference_fit("n257_k3", kind == "hard", max_iter=2)
    with pytest.warns(M.GmmConvergenceWarning, match="Best performing initialization did not converge"):
        got = M.gaussian_mixture(x, w, mu, prec, hard=kind == "hard", max_iter=2, device=DEV)
    assert (got.n_iter_, got.converged_) == (2, False) == (short["n_iter"], short["converged"])
    with pytest.warns(M.GmmConvergenceWarning):
        got = M.gaussian_mixture(x, w, mu, prec, hard=kind == "hard", max_iter=1, device=DEV)
    assert (got.n_iter_, got.converged_) == (1, False)
    one = ref.step(x, ref.initial_block(w, mu, prec), kind == "hard")
    assert ref.rel_diff(got.means_, one[0][1]) <= ref.fit_tolerance("n257_k3", kind)
    assert abs(got.lower_bound_ - one[1]) <= ref.fit_tolerance("n257_k3", kind) * abs(one[1])


def test_a_zero_covariance_raises_scikit_learns_error():
    """One component, 64 samples of 3.75, reg_covar = 0: resp = exp(0) = 1, nk = 64, the sums and the mean are exact, cov = 0."""
    x = np.full(64, 3.75)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        M.gaussian_mixture(x, [1.0], [3.0], [1.0], reg_covar=0.0, device=DEV)
    Pd, state = device_iterations(x, np.array([[1.0], [3.0], [1.0], [1.0]]), reg_covar=0.0, max_iter=5)
    assert state[:4].tolist() == [1, 1, 0, 1] and Pd[1, 0] == 3.75 and Pd[2, 0] == 0.0        # stopped at once; iterations behind it did nothing


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_chunks_and_repeats_change_no_bit(kind):
    x, w, mu, prec = ref.fit_case("n4099_k5")
    prepared = M.prepare(x, w, mu, prec, hard=kind == "hard")
    runs = [M.run(prepared, DEV, chunk=c) for c in (1, 8, 100, 8)]
    for r in runs[1:]:
        assert r.n_iter_ == runs[0].n_iter_ and r.converged_ == runs[0].converged_ and r.lower_bound_ == runs[0].lower_bound_
        for a, b in zip(r[:4], runs[0][:4]):
            assert a.tobytes() == b.tobytes()


# ---- whole fits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("name", sorted(ref.FIT_CASES))
def test_whole_fits_against_the_oracle(name, kind):
    x, w, mu, prec = ref.fit_case(name)
    K = w.shape[0]
    want = reference_fit(name, kind == "hard")
    got = M.gaussian_mixture(x, w, mu, prec, hard=kind == "hard", device=DEV)
    assert (got.n_iter_, got.converged_) == (want["n_iter"], want["converged"])
    bound = ref.fit_tolerance(name, kind)
    diffs = {"weights": ref.rel_diff(got.weights_, want["P"][0]), "means": ref.rel_diff(got.means_, want["P"][1]),
             "covariances": ref.rel_diff(got.covariances_, want["P"][2]), "pc": ref.rel_diff(got.precisions_cholesky_, want["P"][3]),
             "lower_bound": ref.rel_diff([got.lower_bound_], [want["lower_bound"]])}
    print(f"gmm fit {name} {kind}: bound {bound:.3e}", {k: f"{v:.3e}" for k, v in diffs.items()})
    assert max(diffs.values()) <= bound, (diffs, bound)
    points = x[:5000]
    proba = M.predict_proba(got, points, DEV)
    assert proba.shape == (points.shape[0], K) and proba.dtype == np.float64
    off = np.abs(proba.sum(axis=1) - 1.0).max()
    print(f"gmm fit {name} {kind}: predict_proba rows sum to 1 within {off / EPS:.2f} eps (K = {K})")
    assert off <= K * EPS
    labels = M.predict(got, points.reshape(-1, 1), DEV)
    assert (labels == np.argmax(proba, axis=1)).all()
    lse = M.score_samples(got, points, DEV)
    want_lse = ref.e_step(points, got.parameter_block())[0]
    assert np.abs(lse - want_lse).max() <= 8 * EPS * np.abs(want_lse).max() + 8 * EPS


# ---- train_gmm end to end ------------------------------------------------------------------------------------------------------------------
def numeral_counts():
    rng = np.random.RandomState(9)
    values = np.round(rng.lognormal(2.0, 1.5, size=300) * rng.choice([-1.0, 1.0, 1.0, 1.0], size=300), 3)
    nc = {repr(float(v)): int(c) for v, c in zip(values, rng.randint(1, 20, size=300))}
    nc["n/a"] = 7                                                          # an invalid numeral among them
    assert len(nc) == 301
    return nc


@pytest.mark.parametrize("log_space", [False, True])
@pytest.mark.parametrize("mode", ["rd", "fp"])
def test_train_gmm_end_to_end_without_scikit_learn(mode, log_space, tmp_path, monkeypatch):
    for name in [m for m in sys.modules if m == "sklearn" or m.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "sklearn", None)                      # `import sklearn` raises ImportError
    nc = numeral_counts()
    K = 6
    prototypes = P.train_som(nc, prototypes=K, iters=500, log_space=log_space) if mode == "fp" else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", M.GmmConvergenceWarning)
        out = P.train_gmm(nc, components=K, iters=30, gmm_init_mode=mode, gmm_type="soft", prototypes=prototypes, log_space=log_space,
                          device=DEV)
    assert out["numerals"] == [k for k in nc if k != "n/a"]
    post = out["posterior"]
    assert post.shape == (300, K) and post.dtype == np.float64 and np.isfinite(post).all()
    assert np.abs(post.sum(axis=1) - 1.0).max() <= K * EPS
    g = out["gmm"]
    assert 1 <= g.n_iter_ <= 30 and np.isfinite(g.lower_bound_) and abs(g.weights_.sum() - 1.0) <= K * EPS and (g.covariances_ > 0).all()
    paths = P.write_gmm_files(tmp_path, out, K, mode, "soft", log_space)
    folder = tmp_path / ("gmm_log" if log_space else "gmm")
    assert paths == (str(folder / f"gmm-{K}-{mode}-soft.dat"), str(folder / f"gmm_posterior-{K}-{mode}-soft.dat"))
    assert np.array_equal(pickle.load(open(paths[1], "rb")), post)
    assert np.array_equal(pickle.load(open(paths[0], "rb"))["means_"], g.means_)
    if mode == "fp":
        som_path = P.write_som_prototypes(tmp_path, prototypes, K, 0.03, 0.3, log_space)
        assert os.path.basename(som_path) == f"prototypes-{K}-0.03-0.3.dat" and np.array_equal(pickle.load(open(som_path, "rb")), prototypes)
    assert "sklearn" not in sys.modules or sys.modules["sklearn"] is None
