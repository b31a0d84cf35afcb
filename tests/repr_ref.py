"""REPR features in float64 numpy, written from the contract of gte_repr_features in include/gte.h, and the page alignment rule of
``Repr.token_ids``.  Pinned against the reference's recorded outputs by tests/test_repr_ref_cpu.py; the oracle of the GPU tests.

Every operation is an elementwise numpy operation, rounded once, in the order the contract states: the squares are summed over
k = 0 .. D-1 one at a time and the weights over c = 0 .. C-1 one at a time, so nothing depends on numpy's reduction order."""
import numpy as np

MIN_MARGIN = 1e-4


def clamped_distances(rows, centers):
    """t [n, C] = max(sqrt(sum_k (e_k - c_k)^2), 1e-4) for the embedding rows ``rows`` [n, D]."""
    rows, centers = np.asarray(rows, dtype=np.float64), np.asarray(centers, dtype=np.float64)
    acc = np.zeros((rows.shape[0], centers.shape[0]), dtype=np.float64)
    for k in range(rows.shape[1]):
        diff = rows[:, k, None] - centers[None, :, k]
        acc = acc + diff * diff
    return np.maximum(np.sqrt(acc), MIN_MARGIN)


def similarity(rows, centers, alpha=1.0):
    """q [n, C]: the weights (1 / t)^alpha divided by their sum taken in the order c = 0 .. C-1."""
    inv = 1.0 / clamped_distances(rows, centers)
    w = inv if alpha == 1.0 else np.power(inv, np.float64(alpha))
    s = np.zeros(w.shape[0], dtype=np.float64)
    for c in range(w.shape[1]):
        s = s + w[:, c]
    return w / s[:, None]


def chosen_centre(tok, embeddings, centers, alpha=1.0):
    """int [n]: the first index at which q is largest; -1 for a node without a token."""
    tok = np.asarray(tok, dtype=np.int64)
    out = np.full(tok.shape[0], -1, dtype=np.int64)
    has = tok >= 0
    if has.any():
        out[has] = np.argmax(similarity(np.asarray(embeddings)[tok[has]], centers, alpha), axis=1)      # the FIRST maximum
    return out


def features(tok, embeddings, centers, i_proto, alpha=1.0, combined=False):
    """-> (out float64 [n, P], bound float64 [n, P]).  Hard mode: out is exactly representable in float32 ((float)i_proto of the
    chosen row) and bound is 0.  Combined mode: out = sum_c (float)q_c * (float)i_proto[c, j] in float64 and bound =
    (C + 3) * 2^-24 * sum_c |q_c * p_cj|, the rounding bound of a C-term float32 dot product of float32-rounded factors
    whatever its order.  Rows of a node without a token (-1) are zero."""
    tok = np.asarray(tok, dtype=np.int64)
    i_proto = np.asarray(i_proto, dtype=np.float64)
    n, (n_c, p) = tok.shape[0], i_proto.shape
    out, bound = np.zeros((n, p)), np.zeros((n, p))
    has = tok >= 0
    if not has.any():
        return out, bound
    pf = i_proto.astype(np.float32).astype(np.float64)
    if not combined:
        out[has] = pf[chosen_centre(tok[has], embeddings, centers, alpha)]
        return out, bound
    q = similarity(np.asarray(embeddings)[tok[has]], centers, alpha)
    qf = q.astype(np.float32).astype(np.float64)
    acc, mag = np.zeros((q.shape[0], p)), np.zeros((q.shape[0], p))
    for c in range(n_c):
        acc = acc + qf[:, c, None] * pf[None, c, :]
        mag = mag + np.abs(q[:, c, None] * i_proto[None, c, :])
    out[has], bound[has] = acc, (n_c + 3) * 2.0 ** -24 * mag
    return out, bound


def separated_or_tied(embeddings, centers, rel=1e-9):
    """True where every vocabulary row has its two best clamped distances either bit-equal or more than ``rel`` apart, relative:
    the condition under which the choice of a centre does not depend on a summation order."""
    t = np.sort(clamped_distances(embeddings, centers), axis=1)
    if t.shape[1] < 2:
        return True
    a, b = t[:, 0], t[:, 1]
    return bool(np.all((a == b) | (b - a > rel * b)))


def golden():
    """tests/golden/repr_cases.json (tools/make_repr_golden.py) with the arrays of every artefact set as float64 / float32."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repr_cases.json")) as f:
        data = json.load(f)
    for s in data["sets"]:
        for key in ("embeddings", "prototypes", "i_embedding"):
            s[key] = np.asarray(s[key], dtype=np.float64)
        for key in ("hard", "combined"):
            s[key] = [np.asarray(rows, dtype=np.float64).astype(np.float32).reshape(len(rows), s["i_embedding"].shape[1])
                      for rows in s[key]]
    return data


def align(page_token_ids, page_sizes):
    """The node ids of ``Repr.token_ids`` from every page's token ids: token j of a page belongs to node j, surplus tokens are
    dropped, nodes beyond the last token get -1."""
    out = []
    for ids, n in zip(page_token_ids, page_sizes):
        ids = list(ids)[:n]
        out.extend(ids + [-1] * (n - len(ids)))
    return np.asarray(out, dtype=np.int32)
