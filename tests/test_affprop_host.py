"""Host side of affinity propagation (components/tables/affinity.py, utils/matrixes.py, train_repr's ``affinity`` switch):
``prepare`` and ``finish`` around the reference sweep of tests/affprop_ref.py against scikit-learn, the degenerate inputs that
never reach a device, what raises before any device call, and the argument checks of gte_affprop_iterate that return before any
launch.  Nothing here needs a GPU."""
import warnings

import numpy as np
import pytest

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.components.tables import affinity as AP, preprocessor as P
from gnn_tableextraction_amd.utils import matrixes as M
from tests import affprop_ref as ref, lev_ref


def sklearn_fit(S, **kw):
    from sklearn.cluster import AffinityPropagation
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = AffinityPropagation(affinity="precomputed", **kw).fit(S)
    return np.asarray(est.cluster_centers_indices_, dtype=np.intp), est.labels_, est.n_iter_


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device stage fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device function was called")
    monkeypatch.setattr(G, "affprop_iterate", boom)
    monkeypatch.setattr(G, "affprop_workspace", boom)
    monkeypatch.setattr(AP, "run", boom)


# ---- prepare / finish --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ref.GRID[37], ref.GRID[16], ref.GRID[6]] + ref.CUT_SHORT[:1] + ref.NO_EXEMPLAR[:1] + ref.RAMP,
                         ids=lambda c: c.id)
def test_prepare_reference_sweep_finish_equals_scikit_learn(case, no_device):
    pytest.importorskip("sklearn")
    want = sklearn_fit(case.S(), damping=case.damping, convergence_iter=case.ci, max_iter=case.max_iter, preference=case.pref(),
                       random_state=ref.SEED)
    S = case.S().copy()
    prepared = AP.prepare(S, preference=case.pref(), random_state=ref.SEED)
    np.testing.assert_array_equal(S, case.S())                            # the caller's matrix is left alone
    assert prepared.result is None
    np.testing.assert_array_equal(prepared.S, case.noisy())               # the noise bits are numpy's
    run = ref.Run(prepared.S, case.damping, case.ci, case.max_iter).advance(case.max_iter)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        centers, labels = AP.finish(prepared.S, run.E, bool(run.converged))
    np.testing.assert_array_equal(centers, want[0])
    np.testing.assert_array_equal(labels, want[1])
    assert run.done == want[2]
    texts = [str(w.message) for w in seen if issubclass(w.category, AP.AffinityConvergenceWarning)]
    if run.K == 0:
        assert texts == [AP.NO_CENTERS_TEXT]
    elif not run.converged:
        assert texts == [AP.NOT_CONVERGED_TEXT]
    else:
        assert texts == []


def test_the_noise_comes_from_the_generator_scikit_learn_would_use():
    S = ref.blobs(63)
    want = ref.prepare(S, None, 5)[0]
    np.testing.assert_array_equal(AP.prepare(S, random_state=5).S, want)
    np.testing.assert_array_equal(AP.prepare(S, random_state=np.int64(5)).S, want)
    np.testing.assert_array_equal(AP.prepare(S, random_state=np.random.RandomState(5)).S, want)
    saved = np.random.get_state()
    try:
        np.random.seed(5)
        np.testing.assert_array_equal(AP.prepare(S, random_state=None).S, want)       # None: numpy's global generator
    finally:
        np.random.set_state(saved)
    rs = np.random.RandomState(5)
    AP.prepare(S, random_state=rs)
    assert rs.standard_normal() == np.random.RandomState(5).standard_normal(63 * 63 + 1)[-1]      # an instance is advanced
    with pytest.raises(ValueError, match="seed"):
        AP.prepare(S, random_state="seven")
    # integers and float32 are taken as float64
    np.testing.assert_array_equal(AP.prepare(np.round(S).astype(np.int64), random_state=5).S, ref.prepare(np.round(S), None, 5)[0])


def test_finish_without_an_exemplar():
    S = ref.Case("blobs", 63, 0.5, 3).noisy()
    for converged in (False, True):
        with pytest.warns(AP.AffinityConvergenceWarning, match="will not have any cluster centers"):
            centers, labels = AP.finish(S, np.zeros(63, dtype=bool), converged)
        assert len(centers) == 0 and centers.dtype.kind == "i"
        np.testing.assert_array_equal(labels, np.full(63, -1))
    assert issubclass(AP.AffinityConvergenceWarning, UserWarning)


@pytest.mark.parametrize("S,preference", [(np.array([[-2.0]]), None), (np.full((4, 4), -1.0), -5.0), (np.full((4, 4), -1.0), 0.0),
                                          (np.array([[0.0, -2.0], [-2.0, 0.0]]), None), (np.array([[0.0, -2.0], [-2.0, 0.0]]), -2.0)],
                         ids=["one", "equal-low-preference", "equal-high-preference", "symmetric-2x2", "symmetric-2x2-preference"])
def test_degenerate_inputs_never_reach_the_device(S, preference, no_device):
    pytest.importorskip("sklearn")
    from sklearn.cluster import AffinityPropagation
    with pytest.warns(UserWarning, match="mutually equal"):
        est = AffinityPropagation(affinity="precomputed", preference=preference, random_state=0).fit(S)
    rs = np.random.RandomState(3)
    with pytest.warns(UserWarning, match="^All samples have mutually equal similarities. Returning arbitrary cluster center"):
        centers, labels, n_iter = AP.affinity_propagation(S, preference=preference, random_state=rs, return_n_iter=True, device="cuda:0")
    np.testing.assert_array_equal(centers, est.cluster_centers_indices_)
    np.testing.assert_array_equal(labels, est.labels_)
    assert n_iter == est.n_iter_ == 0
    assert rs.standard_normal() == np.random.RandomState(3).standard_normal()          # the generator was not touched
    with pytest.warns(UserWarning, match="mutually equal"):
        pair = M.affinity(S, device="cuda:0") if preference is None else AP.affinity_propagation(S, preference=preference)
    assert len(pair) == 2


# ---- what raises before any device call ------------------------------------------------------------------------------------------
def test_value_errors_come_before_any_device_call(no_device):
    S = ref.blobs(63)
    bad_inputs = [S[:, :-1], S[0], np.zeros((0, 0)), np.zeros((2, 2, 2))]
    for bad in bad_inputs:
        with pytest.raises(ValueError, match="square|at least one"):
            AP.affinity_propagation(bad)
    for value in (np.nan, np.inf, -np.inf):
        bad = S.copy()
        bad[5, 7] = value
        with pytest.raises(ValueError, match="NaN or infinity"):
            AP.affinity_propagation(bad)
        with pytest.raises(ValueError, match="NaN or infinity"):
            AP.prepare(bad)
    for damping in (0.49, 1.0, 1.5, -0.1, float("nan"), "0.9"):
        with pytest.raises(ValueError, match="damping"):
            AP.affinity_propagation(S, damping=damping)
    for ci in (0, -1, 2.5):
        with pytest.raises(ValueError, match="convergence_iter"):
            AP.affinity_propagation(S, convergence_iter=ci)
    with pytest.raises(ValueError, match="max_iter"):
        AP.affinity_propagation(S, max_iter=0)
    for pref in (np.zeros(5), np.zeros((63, 63)), np.nan):
        with pytest.raises(ValueError, match="preference"):
            AP.affinity_propagation(S, preference=pref)
    lib = _lib.load()
    max_n, max_ci = lib.gte_affprop_max_n(), lib.gte_affprop_max_convergence_iter()
    assert max_n >= 8192 and max_ci >= 64
    huge = np.broadcast_to(np.float64(-1.0), (max_n + 1, max_n + 1))       # a view of one number: nothing that size is allocated
    with pytest.raises(ValueError, match=f"{max_n + 1} samples"):
        AP.affinity_propagation(huge)
    with pytest.raises(ValueError, match="ring"):
        AP.affinity_propagation(S, convergence_iter=max_ci + 1)


def test_no_cpu_fallback():
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        AP.run(ref.Case("blobs", 3, 0.5, 3).noisy(), 0.5, 3, 10, device="cpu")


# ---- gte_affprop_iterate: what returns before a launch ---------------------------------------------------------------------------
def call(lib, S=0x10000, A=0x20000, R=0x30000, n=5, d=0.9, omd=None, ci=15, max_iter=200, sweeps=3, ex=0x40001, ws=0x50000,
         ws_bytes=None, state=0x60004):
    ws_bytes = lib.gte_affprop_workspace_bytes(max(n, 0), max(ci, 1)) if ws_bytes is None else ws_bytes
    return lib.gte_affprop_iterate(S, A, R, n, d, 1.0 - d if omd is None else omd, ci, max_iter, sweeps, ex, ws, ws_bytes, state, None)


def test_limits_and_argument_checks_return_before_any_launch():
    lib = _lib.load()
    max_n, max_ci = lib.gte_affprop_max_n(), lib.gte_affprop_max_convergence_iter()
    bad = [dict(n=-1), dict(ci=0), dict(max_iter=0), dict(sweeps=-1), dict(d=1.5), dict(d=-0.5), dict(d=float("nan")), dict(omd=2.0),
           dict(S=0), dict(A=0), dict(R=0), dict(ex=0), dict(ws=0), dict(state=0),
           dict(S=0x10004), dict(A=0x20004), dict(R=0x30004), dict(ws=0x50004), dict(state=0x60002)]
    for kw in bad:
        assert call(lib, **kw) == -1, kw
        assert b"affprop" in lib.gte_last_error()
    for kw in (dict(n=max_n + 1), dict(ci=max_ci + 1), dict(n=max_n + 1, S=0), dict(ci=max_ci + 1, sweeps=0), dict(n=max_n + 1, ws_bytes=0)):
        assert call(lib, **kw) == -4, kw                                   # the limits come before the empty call and the pointers
    assert call(lib, n=max_n + 1, sweeps=-1) == -1                         # but after the plain size checks
    need = lib.gte_affprop_workspace_bytes(5, 15)
    assert need >= 5 * 8 + 5 * 15 and lib.gte_affprop_workspace_bytes(max_n, max_ci) >= max_n * (8 + max_ci)
    assert lib.gte_affprop_workspace_bytes(2, 3) < lib.gte_affprop_workspace_bytes(2000, 3) < lib.gte_affprop_workspace_bytes(2000, 200)
    for short in (0, need - 1):
        assert call(lib, ws_bytes=short) == -3
        assert b"workspace" in lib.gte_last_error()
    assert call(lib, ws_bytes=need - 1, S=0) == -1                         # pointers before the workspace size
    # nothing to do: no launch, whatever the pointers
    assert call(lib, sweeps=0) == 0 and call(lib, n=0) == 0
    assert call(lib, sweeps=0, S=0, A=0, R=0, ex=0, ws=0, state=0, ws_bytes=0) == 0


# ---- train_repr -------------------------------------------------------------------------------------------------------------------
def test_train_repr_rejects_an_unknown_affinity_before_anything_else(no_device):
    with pytest.raises(ValueError, match="affinity must be 'host' or 'device'"):
        P.train_repr({"<UNK_W>": 1, "w": 2}, similarity=np.zeros((2, 2)), affinity="bogus")
    with pytest.raises(ValueError, match="bogus"):
        P.train_repr({"<UNK_W>": 1, "w": 2}, affinity="bogus")             # before the similarity matrix is asked of a device


def test_train_repr_default_still_clusters_with_scikit_learn(no_device):
    pytest.importorskip("sklearn")
    rc = ref.small_rc()
    words = P.repr_words(rc, 2000)
    sim = lev_ref.similarity(words, lev_ref.reference())
    want = sklearn_fit(sim, damping=0.9, random_state=0)
    for kw in ({}, {"affinity": "host"}):
        result = P.train_repr(rc, similarity=sim, random_state=0, tsne_kwargs={"perplexity": 10}, **kw)
        np.testing.assert_array_equal(result["centers"], want[0])
        np.testing.assert_array_equal(result["labels"], want[1])
    # and the reference sweep on the same matrix gives what 'device' has to give
    centers, labels, n_iter = ref.affinity_propagation(sim, damping=0.9, random_state=0)
    np.testing.assert_array_equal(centers, want[0])
    np.testing.assert_array_equal(labels, want[1])
    assert n_iter == want[2]
