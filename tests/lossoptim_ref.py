"""float64 oracle of the loss and optimiser kernels (csrc/loss_optim.hip, the fused head of csrc/narrow_layer.hip).

numpy only: no torch, no device.  Every function takes the float32 arrays the device gets, converts them to float64 and does
everything else in float64, so a difference between a kernel and this file is the kernel's float32 rounding (or a bug).
tests/test_lossoptim_ref_cpu.py checks this file against torch in float64; tests/test_gpu_loss_optim.py checks the kernels
against it.
"""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def labels_of(labels, n_classes):
    """(y, valid): y = int(label), truncation toward zero like ``.long()``; valid = label inside [0, C)."""
    y = np.trunc(_f64(labels)).astype(np.int64)
    return y, (y >= 0) & (y < n_classes)


def ce_rows(logits, labels, class_weight=None):
    """Per-node pieces of the weighted cross-entropy: dict of max logit ``m``, log-sum-exp ``lse``, the label's logit ``zy``,
    ``nll`` = lse - zy, weight ``w`` (0 for an ignored node), ``softmax`` [n, C], ``onehot`` [n, C], ``arg`` (first maximum),
    ``y``, ``valid``.  Ignored nodes have zy = nll = 0."""
    z = _f64(logits)
    n, c = z.shape
    y, valid = labels_of(labels, c)
    m = z.max(axis=1)
    e = np.exp(z - m[:, None])
    s = e.sum(axis=1)
    lse = m + np.log(s)
    ys = np.where(valid, y, 0)
    zy = np.where(valid, z[np.arange(n), ys], 0.0)
    w = np.ones(n) if class_weight is None else _f64(class_weight)[ys]
    w = np.where(valid, w, 0.0)
    onehot = np.zeros((n, c))
    onehot[np.arange(n)[valid], y[valid]] = 1.0
    return {"m": m, "lse": lse, "zy": zy, "nll": np.where(valid, lse - zy, 0.0), "w": w, "softmax": e / s[:, None],
            "onehot": onehot, "arg": z.argmax(axis=1), "y": y, "valid": valid}          # np.argmax: the first maximum


def ce(logits, labels, class_weight=None, grad_scale=1.0):
    """Weighted cross-entropy as include/gte.h A10 defines it -> (loss, sum_w, n_correct, dlogits).

    loss = sum_i w[y_i] nll_i / sum_w, sum_w = sum_i w[y_i], dlogits = grad_scale * d loss / d logits.
    A node whose label is outside [0, C) is ignored: nothing to loss, sum_w or n_correct, a zero dlogits row.
    sum_w == 0: the loss is 0 and every dlogits row is 0.  n_correct counts the nodes whose FIRST maximum is their label."""
    r = ce_rows(logits, labels, class_weight)
    sum_w = float(r["w"].sum())
    n_correct = int((r["valid"] & (r["arg"] == r["y"])).sum())
    if not sum_w > 0.0:
        return 0.0, sum_w, n_correct, np.zeros_like(r["softmax"])
    loss = float((r["w"] * r["nll"]).sum() / sum_w)
    dl = (float(np.float64(np.float32(grad_scale))) * r["w"] / sum_w)[:, None] * (r["softmax"] - r["onehot"])
    dl[~r["valid"]] = 0.0
    return loss, sum_w, n_correct, dl


def colsum(x):
    """out[c] = sum_r x[r][c]"""
    return _f64(x).sum(axis=0)


def aggregate(indptr, indices, eweight, t_self, t_neigh, mean=True):
    """logits of gte_head_agg_ce: t_self[v] + scale_v * sum_{e in row v} w[e] t_neigh[indices[e]], scale_v = 1 / in-degree for the
    mean (0 for a node without in-edges), 1 for the sum.  Also returns the same sum over magnitudes (a rounding-error scale)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    idx = np.asarray(indices, dtype=np.int64)
    deg = np.diff(indptr)
    n = len(deg)
    w = np.ones(len(idx)) if eweight is None else _f64(eweight)
    tn = _f64(t_neigh)
    rows = np.repeat(np.arange(n), deg)
    acc, mag = np.zeros((n, tn.shape[1])), np.zeros((n, tn.shape[1]))
    np.add.at(acc, rows, w[:, None] * tn[idx])
    np.add.at(mag, rows, np.abs(w[:, None] * tn[idx]))
    scale = (np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0) if mean else np.ones(n))[:, None]
    return _f64(t_self) + scale * acc, np.abs(_f64(t_self)) + scale * mag


def head(indptr, indices, eweight, t_self, t_neigh, labels, class_weight, grad_scale, rindptr, rindices, w_out, mean=True):
    """The fused head (gte_head_agg_ce + gte_head_dlq_finish) as include/gte.h and the comment above head_dlq_finish_kernel
    define it.  (indptr, indices, eweight): in-edge CSR with the edge weights; (rindptr, rindices, w_out): out-edge CSR whose
    weights already hold the 1 / in-degree(dst) of the mean ("norm").  Returns a dict:

    logits     t_self + aggregate(t_neigh)                                  [n, C]
    loss, sum_w, n_correct   the weighted cross-entropy of those logits (:func:`ce`)
    alpha      grad_scale / sum_w, 0 when sum_w == 0
    dl         alpha * w_y (softmax - onehot)                               [n, C]
    q          alpha * A_w^T (norm dl'): q[u] = alpha sum_{e out of u} w_out[e] dl'[rindices[e]]   [n, C]
    gbias      colsum(alpha dl')                                            [C]
    plus the magnitude sums ``logits_mag``, ``q_mag`` (sum of |terms|) that the rounding-error bounds are written in."""
    logits, logits_mag = aggregate(indptr, indices, eweight, t_self, t_neigh, mean)
    r = ce_rows(logits, labels, class_weight)
    loss, sum_w, n_correct, _ = ce(logits, labels, class_weight, 1.0)
    gs = float(np.float64(np.float32(grad_scale)))
    alpha = gs / sum_w if sum_w > 0.0 else 0.0
    dl_un = r["w"][:, None] * (r["softmax"] - r["onehot"])           # dl' of gte_head_agg_ce: without 1 / sum_w
    n, c = dl_un.shape
    rindptr = np.asarray(rindptr, dtype=np.int64)
    ridx = np.asarray(rindices, dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(rindptr))
    wo = np.ones(len(ridx)) if w_out is None else _f64(w_out)
    q, q_mag = np.zeros((n, c)), np.zeros((n, c))
    np.add.at(q, rows, wo[:, None] * dl_un[ridx])
    np.add.at(q_mag, rows, np.abs(wo[:, None] * dl_un[ridx]))
    return {"logits": logits, "logits_mag": logits_mag, "loss": loss, "sum_w": sum_w, "n_correct": n_correct, "alpha": alpha,
            "dl": alpha * dl_un, "q": alpha * q, "q_mag": alpha * q_mag, "gbias": (alpha * dl_un).sum(axis=0), "rows": r}


def _hyper(x):
    return float(np.float64(np.float32(x)))


def bias_corrections(b1, b2, t):
    """(1 - b1^t, sqrt(1 - b2^t)) in float64 from the float32-rounded betas (see :func:`adam`)."""
    b1, b2, t = _hyper(b1), _hyper(b2), float(t)
    return 1.0 - b1 ** t, float(np.sqrt(1.0 - b2 ** t))


def adam(p, g, m, v, t, lr, b1, b2, eps, wd, grad_scale):
    """One torch.optim.Adam step (L2-coupled weight decay, not AdamW) at step ``t`` (1-based) -> the new (p, m, v) in float64:

        g' = grad_scale g + wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
        p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

    The hyper-parameters enter as their FLOAT32-ROUNDED values (``np.float32(0.999)`` converted to float64): that is what the C
    ABI (float arguments of gte_adam_step) and the device ``state`` of gte_adam_step_dev hold.  With the double 0.999 the bias
    correction 1 - b2^t differs by about 1.3e-5 relative at t = 1; that difference is the ABI's, not a kernel bug, and it must
    neither be "fixed" in a kernel nor hidden by a wider tolerance."""
    lr, b1, b2, eps, wd, gs = (_hyper(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    bc1, bc2s = bias_corrections(b1, b2, t)
    gi = gs * g + wd * p
    m1 = b1 * m + (1.0 - b1) * gi
    v1 = b2 * v + (1.0 - b2) * gi * gi
    denom = np.sqrt(v1) / bc2s + eps
    return p - (lr / bc1) * (m1 / denom), m1, v1
