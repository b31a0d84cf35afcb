"""gte_tsne_cond_p / gte_tsne_joint_p / gte_tsne_iterate and components/tables/tsne.py against tests/tsne_ref.py (the contract of
include/gte.h in numpy float64, pinned on scikit-learn's own functions by tests/test_tsne_ref_cpu.py).  t-SNE's descent is
chaotic, so nothing compares embeddings of a long run: parity is per stage and per step, and end to end it is the quality reached.

Bounds, u = 2^-53 (tests/tsne_ref.py: grad_bound, kl_bound, chain_length; derived in tests/test_tsne_ref_cpu.py).  The kernels
evaluate num = x^(-(alpha + 1) / 2) with at most two products, a sqrt and a division for d <= 4 -- at most 4 roundings against
pow's one -- which the per-term allowance of 8 n u >= 16 u covers; the sums are chains of at most L(n) additions (stated in
csrc/tsne.hip; an addition of an exact zero rounds nothing, so L is capped by the number of non-zero addends).

How one iteration is observed.  With update = 0, gains = 1.25, momentum = 0 and learning_rate = 1 the contract gives
gains' = fl(1.25 * 0.8) = 1 exactly, g = grad and update' = 0 - g: the gradient is read off ``update`` bit for bit.  KL is the
state's error when the iteration is the last one (max_iter = 1), and Z is recorded behind the Z partials of the workspace.

Sizes: n = 2, 3; below / at / above one wave (63, 64, 65); 257 and 300 -- more than the 256 columns of one tile and, with 4 and 16
rows per workgroup, last workgroups with one and twelve live rows."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import graph as G
from gnn_tableextraction_amd.components.tables import preprocessor as P, tsne as T
from tests import affprop_ref, lev_ref, tsne_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = ref.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_quality.json")


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to(DEV)     # (a copy: the shared inputs are read-only)


# ---- (a) conditional and joint probabilities -------------------------------------------------------------------------------------
# (n, perplexity, kind, seed): every size at every perplexity it admits, on Gaussian points; zero distances and an outlier whose
# row sum underflows to 0 at beta = 1 at one small and one large size each.  The seeds are those at which the reference's
# decision margin exceeds 1e-9 (asserted below).
P_CASES = [(2, 1.5, "gauss", 0), (3, 1.5, "gauss", 0)] \
    + [(n, p, "gauss", 0) for n in (63, 64, 65, 257) for p in (1.5, 5.0, 30.0)] \
    + [(65, 5.0, "dup", 1), (257, 30.0, "dup", 1), (64, 5.0, "outlier", 2), (257, 1.5, "outlier", 2), (65, 30.0, "outlier", 2)]


def p_input(n, kind, seed):
    return ref.gaussian_sq_dist(n, seed, duplicates=n // 4 if kind == "dup" else 0, outlier=kind == "outlier")


@pytest.mark.parametrize("n,perplexity,kind,seed", P_CASES, ids=lambda v: str(v))
def test_conditional_and_joint_probabilities(n, perplexity, kind, seed):
    d32 = p_input(n, kind, seed)
    C_ref, beta_ref, margin = ref.cond_p(d32, perplexity)
    assert margin > 1e-9, margin                                           # every decision of the search is far from flipping
    if kind == "outlier":
        assert np.exp(-d32[0].astype(np.float64))[1:].sum() == 0.0         # row 0 takes the 1e-8f branch at beta = 1
    if kind == "dup":
        assert (d32[~np.eye(n, dtype=bool)] == 0).any()
    C, beta = G.tsne_cond_p(dev(d32, torch.float32), perplexity)
    C, beta = C.cpu().numpy(), beta.cpu().numpy()
    np.testing.assert_array_equal(beta, beta_ref)
    if n == 2:
        assert (beta == 2.0 ** -100).all()                                 # all 100 steps ran
    scale = np.where(C_ref > 0, C_ref, 1.0)
    rel = np.abs(C - C_ref) / scale
    print(f"cond_p n={n} perplexity={perplexity} {kind}: max rel {rel.max():.3e}, bound {(n + 8) * U:.3e}, margin {margin:.3e}")
    assert rel.max() <= (n + 8) * U
    assert (np.diag(C) == 0).all()

    Pd = G.tsne_joint_p(dev(C)).cpu().numpy()
    P_ref = ref.joint_p(C)                                                 # from the device's C: this stage alone
    off = ~np.eye(n, dtype=bool)
    rel = np.abs(Pd - P_ref)[off] / P_ref[off]
    print(f"joint_p n={n}: max rel {rel.max():.3e}, bound {(n + 10) * U:.3e}")
    assert rel.max() <= (n + 10) * U
    np.testing.assert_array_equal(Pd, Pd.T)
    assert (np.diag(Pd) == 0).all() and (Pd[off] >= ref.EPS).all()


# ---- one iteration ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def joint(n):
    perplexity = {2: 1.5, 40: 8.0, 65: 10.0, 300: 30.0}[n]
    Pm = ref.joint_p(ref.cond_p(ref.gaussian_sq_dist(n, 5), perplexity)[0])
    Pm.setflags(write=False)
    return Pm


def embedding(n, d, kind, seed=0):
    if kind == "init":
        return ref.init_embedding(n, d, seed)
    rng = np.random.default_rng(100 + seed)
    Y = 50.0 * rng.uniform(-1.0, 1.0, (n, d)) if kind in ("spread", "coincident") else rng.standard_normal((n, d))
    if kind == "coincident":
        Y[n // 2:] = Y[:n - n // 2]                                        # every point of the second half on one of the first
    return Y


class Phase:
    """The buffers of one phase on the device.  The buffer that is not current is filled with NaN."""

    def __init__(self, Pm, Y, first=0, update=None, gains=None, cur=0):
        n, d = Y.shape
        self.P = dev(Pm)
        self.Y = torch.full((2, n, d), float("nan"), dtype=torch.float64, device=DEV)
        self.Y[cur] = dev(Y)
        self.update = dev(np.zeros((n, d)) if update is None else update)
        self.gains = dev(np.ones((n, d)) if gains is None else gains)
        self.ws = G.tsne_workspace(n, DEV)
        self.state = torch.tensor([first, 0, 0, first, cur, ref.BIG, ref.BIG, 0], dtype=torch.float64, device=DEV)
        self.n = n

    def advance(self, iters, lr, momentum, e, patience, min_grad_norm, max_iter):
        G.tsne_iterate(self.P, self.Y, self.update, self.gains, lr, momentum, e, patience, min_grad_norm, max_iter, iters, self.ws,
                       self.state)
        return self

    def snapshot(self):
        it, stopped, reason, best_iter, cur, error, best_error, grad_norm = self.state.tolist()
        Y = self.Y.cpu().numpy()
        return {"Y": Y[int(cur)], "other": Y[1 - int(cur)], "update": self.update.cpu().numpy(), "gains": self.gains.cpu().numpy(),
                "Z": float(self.ws.view(torch.float64)[-(-self.n // 16)]), "cur": int(cur),
                "state": {"it": int(it), "stopped": int(stopped), "reason": int(reason), "best_iter": int(best_iter), "error": error,
                          "best_error": best_error, "grad_norm": grad_norm}}


@pytest.mark.parametrize("kind", ["init", "spread", "coincident"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [2, 65, 300])
def test_z_gradient_and_kl(n, d, kind):
    Pm, Y = joint(n), embedding(n, d, kind)
    L = ref.chain_length(n)
    for e in (12.0, 1.0):
        k = ref.kl_grad(Y, Pm, e)
        got = Phase(Pm, Y, gains=np.full((n, d), 1.25)).advance(1, 1.0, 0.0, e, 250, 0.0, 1).snapshot()
        assert (got["gains"] == 1.0).all()                                 # so update' = -grad exactly (see the module docstring)
        grad = -got["update"]
        z_err, z_bound = abs(got["Z"] - k["Z"]), 4 * L * U * k["Z"]
        g_err, g_bound = np.abs(grad - k["grad"]), ref.grad_bound(k, n, L)    # (a bound of 0: coincident points only, grad = 0)
        g_excess = np.divide(g_err, g_bound, out=np.zeros_like(g_err), where=g_bound > 0).max()
        kl_err, kl_bound = abs(got["state"]["error"] - k["KL"]), ref.kl_bound(k, n, L)
        print(f"n={n} d={d} {kind} e={e}: Z error {z_err:.3e} / {z_bound:.3e}, gradient error / bound {g_excess:.3f}, "
              f"KL error {kl_err:.3e} / {kl_bound:.3e}")
        assert z_err <= z_bound
        assert (g_err <= g_bound).all()
        assert kl_err <= kl_bound
        assert got["state"]["it"] == 1 and got["state"]["stopped"] == 0 and got["cur"] == 1


@pytest.mark.parametrize("n,d,seed", [(65, 2, 0), (65, 3, 1), (300, 3, 2), (300, 4, 3), (2, 2, 4)])
def test_the_update_of_one_iteration(n, d, seed):
    rng = np.random.default_rng(seed)
    Pm, Y = joint(n), embedding(n, d, "normal", seed)
    update = rng.choice([-1.0, 1.0], (n, d)) * rng.uniform(1e-4, 1e-2, (n, d))
    gains = rng.uniform(0.01, 3.0, (n, d))
    gains[0, 0] = 0.01                                                     # 0.01 * 0.8 is clamped back to 0.01 where the signs agree
    lr, momentum, e = 200.0, 0.8, 12.0
    k = ref.kl_grad(Y, Pm, e)
    bound = ref.grad_bound(k, n, ref.chain_length(n))
    sure = np.abs(k["grad"]) > bound                                       # elsewhere the sign of the gradient is not pinned
    assert (~sure).sum() == 0                                              # these seeds leave no component out (at most 1 % may be)
    Y_ref, update_ref, gains_ref, _ = ref.step(Y, update, gains, k["grad"], lr, momentum)
    got = Phase(Pm, Y, first=7, update=update, gains=gains, cur=1).advance(1, lr, momentum, e, 250, 0.0, 1000).snapshot()
    np.testing.assert_array_equal(got["gains"][sure], gains_ref[sure])     # the same two float64 operations
    assert (got["gains"] >= 0.01).all() and got["gains"][0, 0] in (0.01, 0.01 + 0.2)
    # update = momentum * update - lr * g: the gradient bound through lr * gains, and 4 u relative to its two operands
    u_bound = lr * gains_ref * bound + 4 * U * (np.abs(momentum * update) + np.abs(lr * k["grad"] * gains_ref))
    y_bound = u_bound + 4 * U * (np.abs(Y) + np.abs(update_ref))
    print(f"n={n} d={d}: update error / bound {(np.abs(got['update'] - update_ref) / u_bound).max():.3f}, "
          f"Y error / bound {(np.abs(got['Y'] - Y_ref) / y_bound).max():.3f}")
    assert (np.abs(got["update"] - update_ref) <= u_bound).all()
    assert (np.abs(got["Y"] - Y_ref) <= y_bound).all()                     # no NaN of the other buffer leaked in
    assert got["cur"] == 0 and got["state"]["it"] == 8
    np.testing.assert_array_equal(got["other"], Y)                         # the buffer that was read is left as it was
    assert got["state"]["error"] == ref.BIG                                # iteration 7 is neither a check nor the last one


# ---- (d) the stop rule ------------------------------------------------------------------------------------------------------------
# (learning rate 5: the points move -- to |y| ~ 0.1 from the 1e-4 init -- but 120 iterations are not yet chaotic: the reference
# summed in another order reports the same errors to the last bit or two)
STOPS = {"grad-norm": dict(lr=5.0, patience=250, min_grad_norm=1e30, ends=50, stopped=1, reason=2),
         "no-progress": dict(lr=0.0, patience=10, min_grad_norm=0.0, ends=100, stopped=1, reason=1),
         "runs-out": dict(lr=5.0, patience=250, min_grad_norm=0.0, ends=120, stopped=0, reason=0)}


@pytest.mark.parametrize("name", list(STOPS))
def test_the_stop_rule(name):
    c = STOPS[name]
    n, d, max_iter, e, momentum = 40, 2, 120, 12.0, 0.5
    Pm, Y0 = joint(n), ref.init_embedding(n, d, 3)
    args = (c["lr"], momentum, e, c["patience"], c["min_grad_norm"], max_iter)
    Y_ref, _, gains_ref, want = ref.run(Pm, Y0, 0, max_iter, c["lr"], momentum, e, c["patience"], c["min_grad_norm"])
    _, _, _, other = ref.run(Pm, Y0, 0, max_iter, c["lr"], momentum, e, c["patience"], c["min_grad_norm"], reverse=True)
    assert (want["it"], want["stopped"], want["reason"]) == (c["ends"], c["stopped"], c["reason"])
    run = Phase(Pm, Y0)
    run.advance(30, *args).advance(60, *args).advance(40, *args)           # 130 enqueued: past every ending
    got = run.snapshot()
    for key in ("it", "stopped", "reason", "best_iter"):
        assert got["state"][key] == want[key], key
    # the numbers of the state.  What may differ: the rounding of one evaluation (the (b) bounds, taken at the reference's last
    # embedding) and the distance of two trajectories, whose scale the reference summed in another order gives (16 times it)
    k = ref.kl_grad(Y_ref, Pm, e)
    L = ref.chain_length(n)
    rounding = {"error": ref.kl_bound(k, n, L), "best_error": ref.kl_bound(k, n, L),
                "grad_norm": float(np.linalg.norm(gains_ref * ref.grad_bound(k, n, L))) + 4 * U * want["grad_norm"]}
    for key in ("error", "best_error", "grad_norm"):
        margin = 16 * abs(want[key] - other[key]) + rounding[key]
        print(f"{name}: {key} {got['state'][key]!r} vs {want[key]!r}, margin {margin:.3e}")
        assert abs(got["state"][key] - want[key]) <= margin, key
    if name == "runs-out":
        assert want["best_iter"] == 99 and want["error"] != want["best_error"]            # iteration 119: an error without a check
    after = run.advance(25, *args).snapshot()
    for key in ("Y", "other", "update", "gains"):
        np.testing.assert_array_equal(after[key].view(np.uint64), got[key].view(np.uint64), err_msg=key)
    assert after["state"] == got["state"] and after["cur"] == got["cur"]


# ---- (e) a short trajectory -------------------------------------------------------------------------------------------------------
def test_ten_iterations_follow_the_reference():
    n, d, iters, lr, e = 65, 3, 10, 50.0, 12.0
    Pm, Y0 = joint(n), ref.init_embedding(n, d, 0)
    Y_ref, update_ref, gains_ref, _ = ref.run(Pm, Y0, 0, iters, lr, 0.5, e, 250, 0.0)
    Y_rev = ref.run(Pm, Y0, 0, iters, lr, 0.5, e, 250, 0.0, reverse=True)[0]
    margin = 16 * np.abs(Y_ref - Y_rev).max()                              # from the reference alone
    assert margin > 0
    got = Phase(Pm, Y0).advance(iters, lr, 0.5, e, 250, 0.0, 250).snapshot()
    err = np.abs(got["Y"] - Y_ref).max()
    print(f"10 iterations: max |Y - Y_ref| {err:.3e}, margin {margin:.3e}, max |Y| {np.abs(Y_ref).max():.3e}")
    assert err <= margin
    np.testing.assert_array_equal(got["gains"], gains_ref)
    assert got["state"]["it"] == iters and got["cur"] == 0


# ---- (f) quality, end to end ------------------------------------------------------------------------------------------------------
def test_the_quality_reached_is_scikit_learns():
    with open(GOLDEN) as f:
        golden = json.load(f)
    kls = [r["kl_divergence"] for r in golden["runs"]]
    assert [r["random_state"] for r in golden["runs"]] == [0, 1, 2, 3]
    limit = max(kls) + (max(kls) - min(kls))
    D = ref.cluster_distances()
    assert D.shape == (200, 200)
    Pm = ref.joint_p(ref.cond_p((D ** 2).astype(np.float32), 30.0)[0])
    L = ref.chain_length(200)
    for seed in range(4):
        Y, info = T.tsne(D, 3, random_state=seed, device=DEV, return_info=True)
        assert Y.shape == (200, 3) and Y.dtype == np.float64 and np.isfinite(Y).all()
        assert set(info) == {"kl_divergence", "n_iter", "learning_rate"} and info["learning_rate"] == 50.0
        k = ref.kl_grad(Y, Pm, 1.0)
        print(f"seed {seed}: KL {k['KL']:.6f} (device reports {info['kl_divergence']:.6f}, n_iter {info['n_iter']}); scikit-learn "
              f"{kls[seed]:.6f}, limit {limit:.6f}")
        assert k["KL"] <= limit
        assert 250 <= info["n_iter"] <= 999 and info["kl_divergence"] <= limit
        if seed == 0:
            again, info2 = T.tsne(D, 3, random_state=seed, device=DEV, return_info=True)
            np.testing.assert_array_equal(Y.view(np.uint64), again.view(np.uint64))        # two runs, the same bits
            assert info2 == info


def test_the_reported_kl_is_the_kl_of_the_embedding_it_was_computed_at():
    """The error of the last iteration is, as in scikit-learn, the KL at the embedding that iteration STARTED from; the embedding
    returned is one update further, so the two can be compared to rounding only where the former is read back.  Through
    ``graph.tsne_iterate``: phase 1, 49 iterations of phase 2, a read-back of Y, then iteration 299 as the last one of max_iter =
    300."""
    D = ref.cluster_distances()
    prepared = T.prepare(D, 3, random_state=0)
    Pm = ref.joint_p(ref.cond_p(prepared.sq_dist, 30.0)[0])
    run = Phase(Pm, prepared.init)
    run.advance(250, 50.0, 0.5, 12.0, 250, 1e-7, 250)
    mid = run.snapshot()
    assert mid["state"]["it"] == 250 and not mid["state"]["stopped"]
    second = Phase(Pm, mid["Y"], first=250)
    second.advance(49, 50.0, 0.8, 1.0, 300, 1e-7, 300)
    at = second.snapshot()
    assert at["state"]["it"] == 299
    last = second.advance(1, 50.0, 0.8, 1.0, 300, 1e-7, 300).snapshot()
    k = ref.kl_grad(at["Y"], Pm, 1.0)
    err, bound = abs(last["state"]["error"] - k["KL"]), ref.kl_bound(k, 200, ref.chain_length(200))
    print(f"KL reported {last['state']['error']!r}, recomputed {k['KL']!r}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound and last["state"]["it"] == 300


# ---- (g) train_repr ---------------------------------------------------------------------------------------------------------------
def test_train_repr_without_scikit_learn(tmp_path, monkeypatch):
    import pickle
    from gnn_tableextraction_amd.components.nlp.repr import Repr
    from gnn_tableextraction_amd.components.tables import vocabulator as V
    rc = affprop_ref.small_rc(60)
    words = P.repr_words(rc, 2000)
    assert len(words) == 60
    sim = lev_ref.similarity(words, lev_ref.reference())
    kw = dict(similarity=sim, affinity="device", random_state=0, device=DEV, tsne_kwargs={"perplexity": 10})
    host = P.train_repr(rc, tsne="host", **{**kw, "tsne_kwargs": {"perplexity": 10, "max_iter": 250}})
    monkeypatch.setitem(sys.modules, "sklearn", None)
    for name in [m for m in sys.modules if m.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, name)
    with pytest.raises(ImportError):
        P.train_repr(rc, tsne="host", **kw)
    result = P.train_repr(rc, tsne="device", **kw)
    assert result["embeddings"].shape == (60, 3) and np.isfinite(result["embeddings"]).all()
    np.testing.assert_array_equal(result["centers"], host["centers"])
    np.testing.assert_array_equal(result["labels"], host["labels"])
    assert list(result["words"]) == list(host["words"])
    four = P.train_repr(rc, n_components=4, tsne="device", **kw)          # the reference's own configuration
    assert four["embeddings"].shape == (60, 4) and np.isfinite(four["embeddings"]).all()
    assert np.ptp(four["embeddings"], axis=0).min() > 1e-3                 # the points moved apart from the 1e-4 init

    idx2repr, repr2idx, vocab = V.build_repr_vocab(rc, max_vocab=2000)
    tables, pts = tmp_path / "tables_preprocess", tmp_path / "repr_pts"
    V.dump_repr_files(tables, rc, idx2repr, repr2idx, vocab)
    path = P.write_embed_repr(tables, result, 3, 2000)
    centers = np.asarray(result["centers"])
    assert os.path.basename(path) == f"embed-repr-{len(centers)}-3-60.dat"
    (pts / "run1").mkdir(parents=True)
    with open(pts / "run1" / f"trained_prototypes_epoch1_{len(centers)}_1.0.dat", "wb") as f:
        pickle.dump({"prototypes": result["embeddings"][centers], "i_embedding": np.zeros((len(centers), 8))}, f)
    emb = Repr.from_reference_files(tables, pts, "run1", 1, len(centers), 1.0, 3, 60, device=DEV)
    with open(path, "rb") as f:
        np.testing.assert_array_equal(pickle.load(f)["embeddings"], result["embeddings"])
    assert emb is not None
