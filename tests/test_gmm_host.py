"""Host side of the device Gaussian mixture (components/tables/gmm.py, numerals.py, som.py, preprocessor.train_gmm / train_som):
what is raised before any device call, the reference's initialisation from prototypes with its quirks, the numeral samples, the
self-organising map against recorded weights of the reference's, the module without scikit-learn, and the argument checks of the
gte_gmm_* entry points that return before any launch.  Nothing here needs a GPU."""
import importlib
import json
import os
import pickle
import random
import sys

import numpy as np
import pytest

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.components.tables import gmm as M, numerals as N, preprocessor as P, som as S

_real_workspace = G.gmm_workspace                                         # (the no_device fixture replaces the attribute)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device stage fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device function was called")
    for name in ("gmm_workspace", "gmm_iterate", "gmm_posterior"):
        monkeypatch.setattr(G, name, boom)
    monkeypatch.setattr(M, "run", boom)


X = np.array([1.0, 1.2, 0.8, 5.0, 5.3, 4.7, 9.0])
W, MU, PREC = np.array([0.5, 0.5]), np.array([[1.0], [5.0]]), np.array([[[1.0]], [[2.0]]])


def test_value_errors_of_prepare_come_before_any_device_call(no_device):
    fit = M.gaussian_mixture
    for value in (np.nan, np.inf):
        bad = X.copy()
        bad[2] = value
        with pytest.raises(ValueError, match="NaN or infinity"):
            fit(bad, W, MU, PREC)
    with pytest.raises(ValueError, match="one feature"):
        fit(np.zeros((4, 2)), W, MU, PREC)
    with pytest.raises(ValueError, match="one feature"):
        fit(np.zeros((2, 2, 1)), W, MU, PREC)
    with pytest.raises(ValueError, match=r"Found array with 1 sample\(s\) .* while a minimum of 2 is required"):
        fit(X[:1], [1.0], [1.0], [1.0])
    with pytest.raises(ValueError, match="Expected n_samples >= n_components but got n_components = 3, n_samples = 2"):
        fit(X[:2], [0.2, 0.3, 0.5], [1.0, 2.0, 3.0], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match=r"The parameter 'weights' should be in the range \[0, 1\]"):
        fit(X, [1.5, -0.5], MU, PREC)
    with pytest.raises(ValueError, match=r"The parameter 'weights' should be normalized, but got sum\(weights\) = 0.90000"):
        fit(X, [0.5, 0.4], MU, PREC)
    fit_ok = M.prepare(X, [0.5, 0.5 + 5e-9], MU, PREC)                     # inside scikit-learn's 1e-8
    assert fit_ok.P.shape == (4, 2)
    with pytest.raises(ValueError, match=r"The parameter 'weights' should have the shape of \(2,\), but got \(3,\)"):
        fit(X, [0.2, 0.3, 0.5], MU, PREC)
    with pytest.raises(ValueError, match=r"The parameter 'means' should have the shape of \(2, 1\), but got \(2, 2\)"):
        fit(X, W, np.zeros((2, 2)), PREC)
    with pytest.raises(ValueError, match=r"The parameter 'full precision' should have the shape of \(2, 1, 1\)"):
        fit(X, W, MU, np.ones((3, 1, 1)))
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="'full precision' should be symmetric, positive-definite"):
            fit(X, W, MU, [1.0, bad])
    with pytest.raises(ValueError, match="all required"):
        fit(X, None, MU, PREC)
    for kw in (dict(tol=-1.0), dict(tol=np.nan), dict(reg_covar=-1e-6), dict(reg_covar=np.inf), dict(max_iter=0), dict(max_iter=2.5),
               dict(max_iter=True)):
        with pytest.raises(ValueError):
            fit(X, W, MU, PREC, **kw)
    max_k = _lib.load().gte_gmm_max_components()
    assert max_k == 64
    many = np.arange(max_k + 1, dtype=np.float64)
    with pytest.raises(ValueError, match=f"{max_k + 1} components"):
        fit(np.arange(200.0), np.full(max_k + 1, 1.0 / (max_k + 1)), many, np.ones(max_k + 1))
    # the sample limit: prepare copies and scans its samples ahead of it, which at 2^31 samples is 16 GB, so the limit is asserted on
    # what refuses such a fit ahead of any launch at no cost: the size query and the workspace wrapper
    lib = _lib.load()
    assert lib.gte_gmm_workspace_bytes(2 ** 31, 2) == 0 and lib.gte_gmm_workspace_bytes(2 ** 31 - 1, 2) > (2 ** 31 - 1) * 12
    with pytest.raises(ValueError, match="samples"):
        _real_workspace(2 ** 31, 2, "cpu")


def test_what_prepare_hands_on(no_device):
    p = M.prepare(X.reshape(-1, 1), W, MU, PREC, hard=True, tol=0, max_iter=7)
    assert p.x.dtype == np.float64 and p.x.shape == (7,) and p.P.dtype == np.float64 and p.P.flags.c_contiguous
    assert p.P.tolist() == [[0.5, 0.5], [1.0, 5.0], [1.0, 0.5], [1.0, np.sqrt(2.0)]]          # pc = sqrt(precision)
    assert (p.hard, p.tol, p.reg_covar, p.max_iter) == (True, 0.0, 1e-6, 7)
    q = M.prepare(X.astype(np.float32), W, MU.reshape(-1), PREC.reshape(-1))                 # flat inits, float32 samples widened
    assert q.P.tolist() == p.P.tolist() and q.x.dtype == np.float64


def test_train_gmm_rejects_modes_and_types_before_anything_else(no_device, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("work was done ahead of the argument check")
    monkeypatch.setattr(N, "numeral_samples", boom)
    nc = {"1": 3, "2": 2}
    with pytest.raises(ValueError, match="gmm_init_mode"):
        P.train_gmm(nc, 2, gmm_init_mode="xx")
    with pytest.raises(ValueError, match="gmm_type"):
        P.train_gmm(nc, 2, gmm_type="medium")
    with pytest.raises(NotImplementedError, match="km"):
        P.train_gmm(nc, 2, gmm_init_mode="km")
    with pytest.raises(ValueError, match="needs prototypes"):
        P.train_gmm(nc, 2, gmm_init_mode="fp")
    with pytest.raises(ValueError, match="3 prototypes for 2 components"):
        P.train_gmm(nc, 2, gmm_init_mode="fp", prototypes=[1.0, 2.0, 3.0])


def test_train_gmm_host_errors_come_before_any_device_call(no_device):
    with pytest.raises(ValueError, match="no valid numeral"):
        P.train_gmm({"abc": 3, "nan": 1}, 2)
    with pytest.raises(ValueError, match="zero standard deviation"):      # every sample is 0: every list is zeros
        P.train_gmm({"0": 5}, 1)
    with pytest.raises(ValueError, match="Expected n_samples >= n_components"):
        P.train_gmm({"1": 1, "5": 1}, 3, gmm_init_mode="fp", prototypes=[1.0, 5.0, 9.0])


def test_init_from_prototypes_on_hand_cases(no_device):
    data = np.array([1.0, 3.0, 10.0, 12.0, 2.0])
    w, mu, prec = M.init_from_prototypes(data, [2.0, 11.0])
    # clusters [0, 1, 3, 2] and [0, 10, 12]: the leading 0 is in the mean, the standard deviation and the count
    assert w.tolist() == [4 / 7, 3 / 7]
    assert mu.shape == (2, 1) and mu.reshape(-1).tolist() == [np.mean([0, 1.0, 3.0, 2.0]), np.mean([0, 10.0, 12.0])]
    assert prec.shape == (2, 1, 1)
    assert prec.reshape(-1).tolist() == [1 / np.std([0, 1.0, 3.0, 2.0]), 1 / np.std([0, 10.0, 12.0])]    # 1 / std: not 1 / variance
    # a tie goes to the first prototype
    w, mu, prec = M.init_from_prototypes(np.array([2.0, 4.0]), [1.0, 3.0])
    assert w.tolist() == [2 / 4, 2 / 4] and mu.reshape(-1).tolist() == [1.0, 2.0]
    # a prototype that wins nothing (a repeated draw's second copy, for one) keeps the lone 0: mean 0, min_sigma for its deviation
    for protos in ([1.0, 50.0], [1.0, 1.0]):
        w, mu, prec = M.init_from_prototypes(np.array([1.0, 2.0]), protos)
        assert w.tolist() == [3 / 4, 1 / 4] and mu.reshape(-1).tolist() == [1.0, 0.0] and prec.reshape(-1)[1] == 1 / 1e-6
    assert M.init_from_prototypes(np.array([1.0, 2.0]), [1.0, 50.0], min_sigma=0.5)[2].reshape(-1)[1] == 2.0
    with pytest.raises(ValueError, match=r"clusters \[0\] have zero standard deviation"):
        M.init_from_prototypes(np.array([0.0, 0.0, 7.0]), [1.0, 6.0])      # a list of zeros only
    with pytest.raises(ValueError):
        M.init_from_prototypes(data, [])
    # chunks change nothing
    rng = np.random.RandomState(0)
    big, protos = rng.uniform(0, 100, 1000), rng.uniform(0, 100, 7)
    a, b = M.init_from_prototypes(big, protos, chunk=64), M.init_from_prototypes(big, protos)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_numerals_and_samples(no_device):
    assert N.to_numeral("1.5") == np.float32(1.5) and isinstance(N.to_numeral("1.5"), np.float32)
    assert N.to_numeral("16777217") == np.float32(16777216)
    for bad in ("abc", "", "nan", "inf", "-inf", "1e39", "1,5"):
        assert N.to_numeral(bad) is None, bad
    f = np.float32
    assert N.weighted_log(f(1)) == 1 and N.weighted_log(f(-1)) == -1 and N.weighted_log(f(0)) == 0 and N.weighted_log(f(0.5)) == f(0.5)
    assert N.weighted_log(f(100)) == np.log(f(100)) + 1 and N.weighted_log(f(100)).dtype == np.float32
    assert N.weighted_log(f(-100)) == -(np.log(f(100)) + 1)
    nc = {"3": 2, "x": 4, "-250.5": 3, "nan": 1, "0.25": 1, "1e3": 2}
    keys, values = N.valid_numerals(nc)
    assert keys == ["3", "-250.5", "0.25", "1e3"] and values == [f(3), f(-250.5), f(0.25), f(1000)]
    unfolded = [3.0, 3.0, -250.5, -250.5, -250.5, 0.25, 1000.0, 1000.0]
    want = list(unfolded)
    random.Random(42).shuffle(want)
    got = N.numeral_samples(nc)
    assert got.dtype == np.float64 and got.tolist() == want and want != unfolded
    random.seed(42)                                                        # the stream random.shuffle has after set_seeds(42)
    again = list(unfolded)
    random.shuffle(again)
    assert again == want
    assert N.numeral_samples(nc, cap=3).tolist() == want[:3]
    assert N.numeral_samples(nc, random_state=7).tolist() != want
    logged = N.numeral_samples(nc, log_space=True)
    assert logged.tolist() == [float(N.weighted_log(f(v))) for v in want]
    assert N.numeral_samples({"x": 2}).shape == (0,)


def test_the_som_equals_the_reference_minisom(no_device):
    cases = json.load(open(os.path.join(GOLDEN, "som_cases.json")))
    assert len(cases) >= 4
    for c in cases:
        data = np.array([float.fromhex(v) for v in c["data"]])
        got = S.train_som_1d(data, c["units"], sigma=c["sigma"], learning_rate=c["learning_rate"], num_iteration=c["iterations"],
                             random_seed=c["seed"])
        assert [float(v).hex() for v in got] == c["weights"], c["name"]
    with pytest.raises(ValueError):
        S.train_som_1d([1.0, 2.0], 3, num_iteration=0)


def test_train_som_and_the_writers(no_device, tmp_path):
    nc = {"3": 20, "x": 4, "-250.5": 3, "0.25": 10, "1e3": 12, "7": 5}
    w = P.train_som(nc, prototypes=4, iters=50)
    assert w.shape == (4,) and w.dtype == np.float64
    data = N.numeral_samples(nc, random_state=42, cap=None)
    assert np.array_equal(w, S.train_som_1d(data, 4, sigma=0.03, learning_rate=0.3, num_iteration=50, random_seed=42))
    assert not np.array_equal(w, P.train_som(nc, prototypes=4, iters=50, log_space=True))
    path = P.write_som_prototypes(tmp_path, w, 4, 0.03, 0.3, log_space=True)
    assert path == str(tmp_path / "som_log" / "prototypes-4-0.03-0.3.dat") and np.array_equal(pickle.load(open(path, "rb")), w)
    result = M.GmmResult(np.array([1.0]), np.zeros((1, 1)), np.ones((1, 1, 1)), np.ones((1, 1, 1)), True, 3, -1.5, False)
    paths = P.write_gmm_files(tmp_path, {"gmm": result, "posterior": np.ones((2, 1)), "numerals": ["1", "2"]}, 1, "rd", "soft")
    assert paths == (str(tmp_path / "gmm" / "gmm-1-rd-soft.dat"), str(tmp_path / "gmm" / "gmm_posterior-1-rd-soft.dat"))
    assert pickle.load(open(paths[0], "rb"))["n_iter_"] == 3 and pickle.load(open(paths[1], "rb")).shape == (2, 1)


def test_the_modules_import_without_scikit_learn(monkeypatch):
    for name in [m for m in sys.modules if m == "sklearn" or m.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "sklearn", None)                      # `import sklearn` raises ImportError
    for mod in (M, N, S, P):
        importlib.reload(mod)
    try:
        p = M.prepare(X, W, MU, PREC)
        assert p.P.shape == (4, 2) and "sklearn" not in M.__dict__
    finally:
        monkeypatch.undo()
        for mod in (M, N, S, P):
            importlib.reload(mod)


def test_entry_points_return_their_codes_without_a_launch():
    lib = _lib.load()
    assert lib.gte_gmm_max_components() == 64 and lib.gte_gmm_workgroup_samples() >= 256
    S_ = lib.gte_gmm_workgroup_samples()
    a = 0x10000                                                            # a dummy aligned address: every call below returns before a launch
    need = lib.gte_gmm_workspace_bytes(1000, 20)
    assert need >= 1000 * 12 and lib.gte_gmm_workspace_bytes(S_ + 1, 20) > lib.gte_gmm_workspace_bytes(S_, 20)
    for n, K in ((0, 2), (-1, 2), (10, 0), (10, 65), (2 ** 31, 2)):
        assert lib.gte_gmm_workspace_bytes(n, K) == 0

    def iterate(x=a, n=1000, K=20, P=a, hard=0, tol=1e-3, reg=1e-6, max_iter=100, n_iters=8, ws=a, ws_bytes=need, state=a):
        return lib.gte_gmm_iterate(x, n, K, P, hard, tol, reg, max_iter, n_iters, ws, ws_bytes, state, None)
    INVALID, UNSUPPORTED, TOO_SMALL = -1, -4, -3                           # GTE_ERR_INVALID_ARGUMENT, _UNSUPPORTED, _WORKSPACE_TOO_SMALL
    for kw in (dict(n=0), dict(n=-5), dict(K=0), dict(K=65), dict(max_iter=0), dict(n_iters=-1), dict(tol=-1.0), dict(tol=float("nan")),
               dict(reg=-1.0), dict(x=0), dict(P=0), dict(ws=0), dict(state=0), dict(x=a + 4), dict(state=a + 4)):
        assert iterate(**kw) == INVALID, kw
    assert iterate(n=2 ** 31) == UNSUPPORTED
    assert iterate(ws_bytes=need - 1) == TOO_SMALL and b"needed" in lib.gte_last_error()
    assert iterate(n_iters=0) == 0                                         # nothing to enqueue: GTE_OK, nothing launched

    def posterior(x=a, m=10, K=3, P=a, resp=a, lse=a, label=a):
        return lib.gte_gmm_posterior(x, m, K, P, resp, lse, label, None)
    for kw in (dict(m=0), dict(K=0), dict(K=65), dict(x=0), dict(P=0), dict(resp=0, lse=0, label=0), dict(resp=a + 4), dict(label=a + 2)):
        assert posterior(**kw) == INVALID, kw
    assert posterior(m=2 ** 31) == UNSUPPORTED


def test_graph_wrappers_check_sizes_and_tensors_on_the_host():
    import torch
    for n, K in ((0, 2), (10, 0), (10, 65), (2 ** 31, 2)):
        with pytest.raises(ValueError):
            G.gmm_workspace(n, K, "cpu")
    x, Pm = torch.zeros(8, dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64)
    with pytest.raises(_lib.GteError):                                     # host tensors: there is no CPU fallback
        G.gmm_iterate(x, Pm, False, 1e-3, 1e-6, 10, 1, torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.float64))
    with pytest.raises(_lib.GteError):
        G.gmm_posterior(x, Pm)
