"""tests/tsne_ref.py -- the numpy restatement of the t-SNE contract in include/gte.h that the GPU tests use as their oracle --
against scikit-learn's own functions: ``_binary_search_perplexity``, ``_joint_probabilities``, ``_kl_divergence`` and
``_gradient_descent``.  Nothing here needs a GPU or the package.

Bounds, u = 2^-53.  A conditional row: an exp and a division cost <= 1 ulp each and a sum of n positive terms has relative
error <= n u, so two correct evaluations of a row differ by at most (n + 8) u relative -- PROVIDED they take the same beta path,
which holds while the decision margin of the search (``cond_p``'s third result) is far above the rounding of H (~ n u).  A beta
path that differed anywhere would change the row by many orders more than the bound, so the row comparison is also the
comparison of the path (scikit-learn does not return beta).  Joint P: one more sum and one more division, + 2 u.  Gradient, per
component: every term carries a bounded number of roundings (8 n u covers them together with the row sum of n terms), and Q
carries Z's, a sum of chains no longer than L <= n: |grad - grad'| <= c (8 n u (A + R) + 4 L u R), c = 2 (alpha + 1) / alpha,
with A and R the absolute-term sums of the reference."""
import numpy as np
import pytest

from tests import tsne_ref as ref

pytest.importorskip("sklearn")
from scipy.spatial.distance import squareform  # noqa: E402
from sklearn.manifold import _t_sne, _utils  # noqa: E402

U = ref.U


CASES = [(2, 1.5, 1), (33, 5.0, 2), (200, 30.0, 3)]


@pytest.mark.parametrize("n,perplexity,seed", CASES)
def test_cond_p_and_joint_p_equal_scikit_learn(n, perplexity, seed):
    d32 = ref.gaussian_sq_dist(n, seed)
    C, beta, margin = ref.cond_p(d32, perplexity)
    assert margin > 1e-9, margin
    want = _utils._binary_search_perplexity(d32, perplexity, 0)
    rel = np.abs(C - want) / np.where(want > 0, want, 1.0)
    print(f"n={n}: cond_p max rel {rel.max():.3e} (bound {(n + 8) * U:.3e}), margin {margin:.3e}")
    assert rel.max() <= (n + 8) * U
    assert (C[want == 0] == 0).all() and (np.diag(C) == 0).all()
    assert np.isfinite(beta).all() and (beta > 0).all()
    if n == 2:
        assert (beta == 2.0 ** -100).all()                                 # H = 0 < log(1.5) at every step: 100 halvings
    P = ref.joint_p(C)
    want_p = _t_sne._joint_probabilities(d32, perplexity, 0)
    got_p = squareform(P, checks=False)
    rel = np.abs(got_p - want_p) / want_p
    print(f"n={n}: joint_p max rel {rel.max():.3e} (bound {(n + 10) * U:.3e})")
    assert rel.max() <= (n + 10) * U
    assert (P == P.T).all() and (np.diag(P) == 0).all() and (P[~np.eye(n, dtype=bool)] >= ref.EPS).all()


def test_cond_p_summed_in_another_order_takes_the_same_path():
    d32 = ref.gaussian_sq_dist(65, 4)
    a, b = ref.cond_p(d32, 5.0), ref.cond_p(d32, 5.0, reverse=True)
    np.testing.assert_array_equal(a[1], b[1])
    assert np.abs(a[0] - b[0]).max() <= (65 + 8) * U * a[0].max()


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["init", "spread"])
def test_kl_grad_equals_scikit_learn(d, kind):
    n = 65
    P = ref.joint_p(ref.cond_p(ref.gaussian_sq_dist(n, 5), 10.0)[0])
    Y = ref.init_embedding(n, d, 0) if kind == "init" else 50.0 * np.random.default_rng(1).uniform(-1, 1, (n, d))
    for e in (12.0, 1.0):
        k = ref.kl_grad(Y, P, e)
        kl, grad = _t_sne._kl_divergence(Y.ravel().copy(), squareform(P, checks=False) * e, max(d - 1, 1), n, d)
        excess = np.abs(k["grad"] - grad.reshape(n, d)) / ref.grad_bound(k, n, n)
        print(f"d={d} {kind} e={e}: gradient error / bound {excess.max():.3f}, KL {k['KL']:.6f} vs {kl:.6f}")
        assert excess.max() <= 1.0
        assert abs(k["KL"] - kl) <= ref.kl_bound(k, n, n)


def test_run_equals_three_iterations_of_gradient_descent():
    n, d, lr, e = 65, 3, 200.0, 12.0
    P = ref.joint_p(ref.cond_p(ref.gaussian_sq_dist(n, 5), 10.0)[0])
    y0 = ref.init_embedding(n, d, 0)
    p, error, it = _t_sne._gradient_descent(_t_sne._kl_divergence, y0.ravel().copy(), it=0, max_iter=3, n_iter_check=50, momentum=0.5,
                                            learning_rate=lr, min_gain=0.01, min_grad_norm=1e-7,
                                            args=[squareform(P, checks=False) * e, max(d - 1, 1), n, d])
    Y, update, gains, state = ref.run(P, y0, 0, 3, lr, 0.5, e, 250, 1e-7)
    Yr = ref.run(P, y0, 0, 3, lr, 0.5, e, 250, 1e-7, reverse=True)[0]
    margin = 16 * np.abs(Y - Yr).max()                                     # the reference against itself in another order
    print(f"3 iterations: max |Y - sklearn| {np.abs(Y - p.reshape(n, d)).max():.3e}, margin {margin:.3e}")
    assert margin > 0 and np.abs(Y - p.reshape(n, d)).max() <= margin
    assert it == 2 and state["it"] == 3 and not state["stopped"]
    # the error is the KL at the embedding the last iteration started from: its own rounding, plus what the trajectories' distance
    # (at most `margin`) can move it, |dKL| <= sum |grad| * |dY|
    k = ref.kl_grad(ref.run(P, y0, 0, 2, lr, 0.5, e, 250, 1e-7)[0], P, e)
    assert state["error"] == k["KL"]
    assert abs(state["error"] - error) <= ref.kl_bound(k, n, n) + margin * np.abs(k["grad"]).sum()
    assert state["best_error"] == ref.BIG and state["best_iter"] == 0      # no check iteration among 0 .. 2


def test_decide_is_the_stop_rule_of_gradient_descent():
    s = ref.new_state(0)
    s = ref.decide(s, 48, 5.0, 1.0, 10, 1e-7, 1000)
    assert s["error"] == ref.BIG and s["it"] == 49 and not s["stopped"]    # not a check iteration: nothing but the count
    s = ref.decide(s, 49, 5.0, 1.0, 10, 1e-7, 1000)
    assert (s["best_error"], s["best_iter"], s["stopped"], s["error"], s["grad_norm"]) == (5.0, 49, 0, 5.0, 1.0)
    s = ref.decide(s, 99, 5.0, 1.0, 10, 1e-7, 1000)                        # no progress, 99 - 49 > 10
    assert (s["stopped"], s["reason"], s["it"]) == (1, 1, 100)
    s = ref.decide(ref.new_state(0), 49, 5.0, 1e-8, 10, 1e-7, 1000)        # progress, but the gradient is small
    assert (s["stopped"], s["reason"], s["best_iter"]) == (1, 2, 49)
    s = ref.decide(ref.new_state(0), 119, 3.0, 1.0, 10, 1e-7, 120)         # the last iteration: the error without a check
    assert (s["error"], s["best_error"], s["stopped"], s["it"]) == (3.0, ref.BIG, 0, 120)
