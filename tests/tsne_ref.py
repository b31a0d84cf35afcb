"""Exact t-SNE in numpy float64, written from the contract of gte_tsne_cond_p / gte_tsne_joint_p / gte_tsne_iterate in
include/gte.h; it never imports the package.  tests/test_tsne_ref_cpu.py pins it on scikit-learn's own functions, the GPU
tests pin the kernels on it.  Sums are numpy's (pairwise) or plain loops: the contract leaves their order free."""
import numpy as np

EPS = float(np.finfo(np.double).eps)
U = 2.0 ** -53
BIG = float(np.finfo(float).max)
CHECK_EVERY = 50
SEARCH_STEPS = 100


# ---- probabilities ----------------------------------------------------------------------------------------------------------------
def cond_p(sq_dist, perplexity, reverse=False):
    """``(C float64 [n, n], beta [n], margin)``: the perplexity search on float32 squared distances.  ``margin``: the smallest
    distance of any step's |H - target| from 0 and from the tolerance -- how far every decision of the search (hit / too high /
    too low) is from flipping.  ``reverse``: sum from the last column to the first (another valid order)."""
    d32 = np.asarray(sq_dist, dtype=np.float32)
    n = d32.shape[0]
    d = d32.astype(np.float64)
    target = float(np.log(np.float64(np.float32(perplexity))))
    tol = float(np.float32(1e-5))
    tiny = float(np.float32(1e-8))
    C = np.zeros((n, n))
    betas = np.zeros(n)
    margin = np.inf
    order = slice(None, None, -1) if reverse else slice(None)
    for i in range(n):
        beta, lo, hi = 1.0, -np.inf, np.inf
        other = np.arange(n) != i
        for _ in range(SEARCH_STEPS):
            p = np.where(other, np.exp(-d[i] * beta), 0.0)
            s = float(np.sum(p[order]))
            if s == 0.0:
                s = tiny
            p = p / s
            diff = (float(np.log(s)) + beta * float(np.sum((d[i] * p)[order]))) - target
            margin = min(margin, abs(diff), abs(abs(diff) - tol))
            if abs(diff) <= tol:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        C[i] = p
        betas[i] = beta
    return C, betas, margin


def joint_p(C):
    """P float64 [n, n]: symmetric, zero diagonal, every other entry at least eps."""
    S = C + C.T
    P = np.maximum(S / max(float(np.sum(S)), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


# ---- one iteration ----------------------------------------------------------------------------------------------------------------
def kl_grad(Y, P, exaggeration=1.0, reverse=False):
    """``dict(grad [n, d], Z, KL, A [n, d], R [n, d], KL_abs)`` at the embedding ``Y``.  ``A`` and ``R``: the sums of the absolute
    values of the attractive and the repulsive terms of every gradient component (without the factor 2 (alpha + 1) / alpha),
    ``KL_abs`` the same for KL: what a rounding bound of the sums scales with.  ``reverse``: row sums from the last column to the
    first."""
    Y = np.asarray(Y, dtype=np.float64)
    n, d = Y.shape
    alpha = float(max(d - 1, 1))
    diff = Y[:, None, :] - Y[None, :, :]
    dist = np.zeros((n, n))
    for c in range(d):                                                     # in component order
        dist = dist + diff[:, :, c] * diff[:, :, c]
    num = (1.0 + dist / alpha) ** (-(alpha + 1.0) / 2.0)
    np.fill_diagonal(num, 0.0)
    Z = float(np.sum(num))
    Q = np.maximum(num / Z, EPS)
    eP = exaggeration * P
    order = slice(None, None, -1) if reverse else slice(None)
    w = (eP - Q) * num
    np.fill_diagonal(w, 0.0)
    terms = w[:, :, None] * diff
    grad = np.sum(terms[:, order, :], axis=1) * (2.0 * (alpha + 1.0) / alpha)
    off = ~np.eye(n, dtype=bool)
    A = np.sum(np.abs((eP * num)[:, :, None] * diff) * off[:, :, None], axis=1)
    R = np.sum(np.abs((Q * num)[:, :, None] * diff) * off[:, :, None], axis=1)
    kl_terms = np.where(off, eP * np.log(np.maximum(eP, EPS) / np.where(off, Q, 1.0)), 0.0)
    return {"grad": grad, "Z": Z, "KL": float(np.sum(kl_terms)), "A": A, "R": R, "KL_abs": float(np.sum(np.abs(kl_terms))),
            "eP_sum": float(np.sum(eP)), "alpha": alpha}


def grad_bound(k, n, L):
    """|grad - grad'| per component for two correct evaluations: c (8 n u (A + R) + 4 L u R), c = 2 (alpha + 1) / alpha.  8 n u: the
    roundings of one term and of a row sum of n terms; 4 L u: Z, chains of at most L additions, enters the repulsive terms."""
    c = 2.0 * (k["alpha"] + 1.0) / k["alpha"]
    return c * (8 * n * U * (k["A"] + k["R"]) + 4 * L * U * k["R"])


def kl_bound(k, n, L):
    """The analogue for KL: 8 n u on the absolute-term sum; the relative error of Z (4 L u) and of the quotient under the logarithm
    (8 u) shift every logarithm by that much, which the sum of e P weighs."""
    return 8 * n * U * k["KL_abs"] + (4 * L + 8) * U * k["eP_sum"]


def step(Y, update, gains, grad, lr, momentum):
    """The update of one iteration: ``(Y, update, gains, grad_norm)``, all new arrays."""
    inc = update * grad < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    g = grad * gains
    update = momentum * update - lr * g
    return Y + update, update, gains, float(np.sqrt(np.sum(g * g)))


def new_state(first):
    return {"it": first, "stopped": 0, "reason": 0, "best_iter": first, "error": BIG, "best_error": BIG, "grad_norm": 0.0}


def decide(state, it, error, grad_norm, n_iter_without_progress, min_grad_norm, max_iter):
    """The end of iteration ``it``: the state block after it (a new dict).  ``error`` is used only where the contract computes
    it -- on check iterations and on the last one."""
    s = dict(state)
    check = (it + 1) % CHECK_EVERY == 0
    if check or it == max_iter - 1:
        s["error"] = error
    if check:
        s["grad_norm"] = grad_norm
        if error < s["best_error"]:
            s["best_error"], s["best_iter"] = error, it
        elif it - s["best_iter"] > n_iter_without_progress:
            s["stopped"], s["reason"] = 1, 1
        if not s["stopped"] and grad_norm <= min_grad_norm:
            s["stopped"], s["reason"] = 1, 2
    s["it"] = it + 1
    return s


def run(P, Y, first, max_iter, lr, momentum, exaggeration, n_iter_without_progress, min_grad_norm, update=None, gains=None,
        reverse=False):
    """One phase from iteration ``first``: ``(Y, update, gains, state)``."""
    Y = np.array(Y, dtype=np.float64)
    update = np.zeros_like(Y) if update is None else np.array(update, dtype=np.float64)
    gains = np.ones_like(Y) if gains is None else np.array(gains, dtype=np.float64)
    state = new_state(first)
    for it in range(first, max_iter):
        k = kl_grad(Y, P, exaggeration, reverse=reverse)
        Y, update, gains, grad_norm = step(Y, update, gains, k["grad"], lr, momentum)
        state = decide(state, it, k["KL"], grad_norm, n_iter_without_progress, min_grad_norm, max_iter)
        if state["stopped"]:
            break
    return Y, update, gains, state


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def gaussian_sq_dist(n, seed, dims=3, scale=1.0, duplicates=0, outlier=False):
    """float32 squared distances of ``n`` seeded Gaussian points; the last ``duplicates`` points repeat the first ones (zero
    distances); ``outlier`` moves point 0 so far that every exp(-d) of its row is 0."""
    rng = np.random.default_rng(seed)
    X = scale * rng.standard_normal((n, dims))
    if duplicates:
        X[n - duplicates:] = X[:duplicates]
    if outlier:
        X[0] += 40.0
    diff = X[:, None, :] - X[None, :, :]
    return (diff ** 2).sum(-1).astype(np.float32)


def cluster_distances(seed=0, clusters=4, per=50, dims=5, scale=6.0):
    """The [200, 200] distance matrix (NOT squared) of four seeded Gaussian clusters: the matrix of the quality test and of
    tools/make_tsne_golden.py."""
    rng = np.random.default_rng(seed)
    centres = scale * rng.standard_normal((clusters, dims))
    X = np.concatenate([c + rng.standard_normal((per, dims)) for c in centres])
    diff = X[:, None, :] - X[None, :, :]
    return np.sqrt((diff ** 2).sum(-1))


def init_embedding(n, d, seed):
    """scikit-learn's random init, as float64."""
    return (1e-4 * np.random.RandomState(seed).standard_normal(size=(n, d)).astype(np.float32)).astype(np.float64)


def chain_length(n):
    """L(n) of csrc/tsne.hip: the additions of the longest chain into Z, capped by the number of non-zero addends."""
    L = 16 * -(-n // 256) + -(-(-(-n // 16)) // 256) + 18
    return min(L, n * (n - 1))
