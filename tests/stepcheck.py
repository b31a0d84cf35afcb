"""Whole-step comparison against a float64 oracle that takes the DEVICE's ReLU masks -- shared by the step tests (not a conftest).

Why the masks: a LayerNorm output within rounding of zero can get a different ReLU decision on the device than in any host
re-computation, and then one (node, feature) of the backward differs by a whole contribution.  The device's backward decides
the mask at exactly one formula, ``fmaf((z - mean) * rstd, gamma, beta) <= 0.f`` with contraction off (csrc/layernorm.h
gte_ln_bwd_pre4 / _pre4m -- ln_relu_bwd_vec_kernel, the planes NT GEMM's LayerNorm-backward epilogue and the narrow layer's fused
backward share it --, the scalar ln_relu_bwd kernels of csrc/layernorm.hip, csrc/smallk_step.h), from the step's pre-LayerNorm ``z`` and its row statistics
``stats`` = [mean[0:n] | rstd[0:n]].  Both stay in the step's buffers after the step (dz is formed in ``dy``), so the host
reproduces the decision bit for bit: xh = fp32(fp32(z - mean) * rstd), and the sign of xh * gamma + beta taken in float64 is the
sign of the fma (the product of two fp32 values is exact in float64; rounding keeps the sign).  A float64 oracle run with those
masks has no branch left to disagree on: every remaining difference is device rounding, so every case is checked tightly.

Where ``z`` lives (``device_relu_masks``):
  * one-call plan (models/step_plan.py, OneCallPlan._alloc, found through engine.plan_buffers): ``t[i]``, columns [0, fout) -- a planes layer's
    [z | t_neigh] (z accumulated into the left half), or the aggregate-first / cached input layer's z;
  * the call-by-call schedule (models/call_schedule.py, CallSchedule._alloc, found through engine._calls.buffer_set): ``t[i]``
    (left half) where the layer has one (transform-first or planes layer), else ``z[i]``;
  * the one-pass short-input layer (BBOX features, gte_sage_smallk_bwd / gte_gemm_p3_nt_smallk_bwd) does NOT save z: its
    backward recomputes z with the forward kernel's instruction sequence (csrc/smallk_step.h: bit-identical z) and reads the
    forward's stats.  The forward wrote y = fmaxf(fmaf(xh, gamma, beta), 0) from that same z, so there the mask is ``y > 0``
    exactly; y is read from the fp32 rows, or from the next layer's input image (an exact fp32 split) when only that was written.
The masks must be read right after the step: a later forward (forward_logits) reuses the buffers.  gamma / beta are the
PRE-step values (the step's Adam updates the module's parameters in place), passed in as ``state``.
"""
import numpy as np
import torch

from oracle import gcnsage_cpu as oc
from tests import poststep

GRAD_REL = 1e-4          # every gradient: max |device - oracle| <= GRAD_REL x max |oracle| of the tensor
LOSS_ATOL = 1e-5


# ---------------------------------------------------------------------------------------------------------------- the masks
def host_relu_mask(z, mean, rstd, gamma, beta) -> np.ndarray:
    """The backward's ReLU decision (keep = True) for fp32 z [n, f], mean / rstd [n], gamma / beta [f]: bit for bit the device's
    ``!(fmaf((z - mean) * rstd, gamma, beta) <= 0.f)``."""
    z = np.asarray(z, dtype=np.float32)
    xh = (z - np.asarray(mean, dtype=np.float32)[:, None]) * np.asarray(rstd, dtype=np.float32)[:, None]   # fp32, two roundings
    s = xh.astype(np.float64) * np.asarray(gamma, dtype=np.float64)[None, :] + np.asarray(beta, dtype=np.float64)[None, :]
    return s > 0


def _layer_buffers(engine, batch):
    """(buffer set, plan kinds or None for the call-by-call schedule, out_gemm) of the step the engine just ran on ``batch``."""
    xp = getattr(batch, "feat_p3", None)
    n, f0 = (xp.rows, xp.cols) if xp is not None else tuple(batch.ndata["feat"].shape)
    on_plan = engine.plan_buffers(batch)
    if on_plan is not None:
        return on_plan + (n, f0)
    return engine._calls.buffer_set(batch), None, False, n, f0


def device_relu_masks(engine, batch, state) -> list:
    """Per hidden layer: the ReLU mask (bool [n, fout]) the device's backward used in the step just run on ``batch`` (see the
    module docstring for where each path keeps z).  ``state``: the parameters BEFORE the step (name -> tensor)."""
    from gnn_tableextraction_amd import ops
    from gnn_tableextraction_amd._lib import LAYER_PLANES, LAYER_SMALLK
    b, kinds, out_gemm, n, f0 = _layer_buffers(engine, batch)
    lib = engine.lib
    layers = list(engine.model.layers)
    dims = [f0] + [l.out_feats for l in layers]
    nh = len(layers) - 1
    masks = []
    for i in range(nh):
        L, fin, fout = layers[i], dims[i], dims[i + 1]
        assert L.activation is not None and isinstance(L.lynorm, torch.nn.LayerNorm), "hidden layers: LayerNorm + ReLU"
        st = b["stats"][i][:2 * n].cpu().numpy()
        if kinds is not None:
            smallk = kinds[i] == LAYER_SMALLK and bool(lib.gte_sage_smallk_bwd_supported(2 * fin, fout))
        else:
            smallk = (b["t"][i] is None and bool(lib.gte_sage_linear_fwd_fuses_ln(2 * fin, fout)) and engine._smallk_bwd(i, L, fin))
        if smallk:
            # z is recomputed in the backward, bit-identical to the forward's: the forward's y carries the decision
            if kinds is not None:
                img = (b["hp_out"] if i == nh - 1 else b["hp"][i + 1]) if ((i < nh - 1 and kinds[i + 1] == LAYER_PLANES) or (i == nh - 1 and out_gemm)) else None
            else:
                img = b["hp"][i + 1] if (b["pl"][i + 1] and fout % 16 == 0) else None
            y = (ops.p3_to_f32(img.view_rows(n)) if img is not None else b["y"][i][:n])[:, :fout].cpu().numpy()
            masks.append(y > 0)
            continue
        zbuf = b["t"][i] if b["t"][i] is not None else b["z"][i]
        z = zbuf[:n, :fout].cpu().numpy()
        masks.append(host_relu_mask(z, st[:n], st[n:2 * n], state[f"layers.{i}.lynorm.weight"].cpu().numpy(),
                                    state[f"layers.{i}.lynorm.bias"].cpu().numpy()))
    return masks


# ---------------------------------------------------------------------------------------------------------- the fp64 oracle
def reference_step(state0, graph, x, labels, masks, class_weights=None, lr=0.01, weight_decay=5e-4, dtype=torch.float64,
                   layer_norm=None) -> dict:
    """One oracle step in ``dtype`` (float64 by default) with the given ReLU masks: loss, logits, gradients and post-step
    parameters as float64 ndarrays.  ``layer_norm``: test hook of gcnsage_forward (the power checks' corruptions)."""
    st = {k: torch.as_tensor(v).detach().cpu().to(dtype) for k, v in state0.items()}
    tr = oc.OracleTrainer(st, lr=lr, weight_decay=weight_decay, class_weights=class_weights)
    loss, logits = tr.step(graph, torch.as_tensor(np.asarray(x)).to(dtype), torch.as_tensor(np.asarray(labels)),
                           masks=None if masks is None else [torch.from_numpy(np.asarray(m)) for m in masks], layer_norm=layer_norm)
    f64 = lambda t: t.detach().to(torch.float64).numpy()
    return {"loss": float(loss), "logits": f64(logits), "grads": {k: f64(v) for k, v in tr.grads().items()},
            "state": {k: f64(v) for k, v in tr.state.items()}}


# ------------------------------------------------------------------------------------------------------- the comparisons
def grad_errors(got: dict, ref: dict, rel: float = GRAD_REL) -> dict:
    """name -> max |got - ref| in units of the tolerance rel x max |ref| (<= 1 passes)."""
    out = {}
    for k, r in ref.items():
        g = np.asarray(got[k], dtype=np.float64)
        r = np.asarray(r, dtype=np.float64)
        tol = rel * float(np.abs(r).max()) + 1e-30
        out[k] = float(np.abs(g - r).max()) / tol
    return out


def assert_grads(got: dict, ref: dict, rel: float = GRAD_REL, what: str = "") -> dict:
    """Every gradient within rel x its tensor's largest entry, no row exceptions.  Returns grad_errors."""
    errs = grad_errors(got, ref, rel)
    bad = {k: round(v, 3) for k, v in errs.items() if not v <= 1.0}
    assert not bad, f"{what}gradients beyond {rel:g} x max (in units of the tolerance): {bad}"
    return errs


def loss_error(got: float, ref: float, atol: float = LOSS_ATOL) -> float:
    """|got - ref| in units of atol."""
    return abs(float(got) - float(ref)) / atol


def check_poststep(ref: dict, params: dict, state0: dict, graph, x, logits_after, weight_decay=5e-4, lr=0.01, atol=1e-4) -> float:
    """Post-step parameters through poststep.hybrid_state (against the oracle's fp64 Adam step), and the logits after the step
    (``logits_after``: the device's forward on its post-step state) at ``atol`` against the fp64 forward of the hybrid state.
    Returns the logits error."""
    g_eff = {k: np.abs(ref["grads"].get(k, np.zeros_like(v)) + weight_decay * np.asarray(state0[k], dtype=np.float64))
             for k, v in ref["state"].items()}
    hyb = poststep.hybrid_state(ref["state"], params, g_eff, lr)
    want = oc.gcnsage_forward(hyb, graph, torch.as_tensor(np.asarray(x)).to(torch.float64)).numpy()
    err = float(np.abs(np.asarray(logits_after, dtype=np.float64) - want).max())
    assert err < atol, f"post-step logits differ by {err:.3e} (> {atol:g})"
    return err


# --------------------------------------------------------------------------------------------- row-localised probe batches
N_CLASSES = 9


def one_round_tile(m: int, cus: int) -> int:
    """The row tile csrc/gemm_p3.hip (one_round_row_tile) picks for m rows on cus CUs: the smallest of 32 / 64 / 96 that covers m
    in one round, else 128."""
    for t in (32, 64, 96):
        if -(-m // t) <= cus:
            return t
    return 128


def probe_pages(f0: int, m: int, tile: int, seed: int = 0, hub_deg: int = 300):
    """Pages with exactly ``m`` nodes in all (data/synthetic.make_page with chosen word counts) and the probe rows of the batch
    they make in page order.  Probes: row 0 and the last row; the last row of the first full ``tile`` and the first of the next;
    a row of the final (partial) tile; both sides of a page boundary; a node whose in-edges are removed (in-degree 0); a hub
    node given ``hub_deg`` extra in-edges from its page.  Labels: 0 on the probes, 1 ... 8 everywhere else -- with class
    weights [1, 0, ..., 0] (``probe_class_weights``) the loss and every dz live in the probes' receptive field only.
    Returns (pages, probes, page offsets)."""
    from gnn_tableextraction_amd.data import synthetic as S
    rng = np.random.default_rng(seed)
    sizes = []
    left = m
    while left > 0:
        k = int(rng.integers(150, 700)) if not sizes else int(rng.integers(40, 700))
        if sizes == [] and m >= hub_deg + 60:
            k = max(k, hub_deg + 60)
        if left - k < 40:
            k = left
        sizes.append(k)
        left -= k
    pages = [S.make_page(3 + j, in_feats=f0, n_words=k) for j, k in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    # the hub: node 1 of page 0 (>= hub_deg + 60 nodes) takes hub_deg more in-edges from its own page
    p = pages[0]
    hub_local = 1
    srcs = rng.choice(np.setdiff1d(np.arange(p.num_nodes), [hub_local]), size=min(hub_deg, p.num_nodes - 1), replace=False)
    p.src = np.concatenate([p.src, srcs.astype(np.int32)])
    p.dst = np.concatenate([p.dst, np.full(len(srcs), hub_local, dtype=np.int32)])
    p.weight = np.concatenate([p.weight, rng.uniform(0.05, 1.0, len(srcs)).astype(np.float32)])
    hub = int(off[0] + hub_local)
    # the in-degree-0 node: node 2 of the middle page loses its in-edges (it keeps its out-edges)
    pm = len(pages) // 2
    q = pages[pm]
    keep = q.dst != 2
    q.src, q.dst, q.weight = q.src[keep], q.dst[keep], q.weight[keep]
    zero_in = int(off[pm] + 2)
    last_full = (m // tile) * tile
    partial = last_full + (m - last_full) // 2 if last_full < m else m - tile // 2
    bnd = int(off[max(1, len(pages) // 3)])
    probes = sorted({0, m - 1, tile - 1, tile, partial, bnd - 1, bnd, zero_in, hub})
    probes = [r for r in probes if 0 <= r < m]
    for j, pg in enumerate(pages):
        lab = rng.integers(1, N_CLASSES, pg.num_nodes)
        loc = [r - off[j] for r in probes if off[j] <= r < off[j + 1]]
        lab[np.asarray(loc, dtype=np.int64)] = 0
        pg.label = lab.astype(np.int64)
    return pages, probes, off


def probe_class_weights(dtype=torch.float32):
    w = torch.zeros(N_CLASSES, dtype=dtype)
    w[0] = 1.0
    return w


def corrupted_layer_norm(kind: str, layer: int, row: int, factor: float = 1 + 1e-2):
    """A layer_norm hook for gcnsage_forward / reference_step that corrupts ONE row of ONE hidden layer the way a wrong kernel
    would: ``dz_scale`` (that row's dz times ``factor``), ``dz_zero`` (that row's dz zeroed), ``stats_swap`` (that row and the next
    one normalised with each other's mean / variance)."""
    import torch.nn.functional as F

    def ln(i, z, shape, weight, bias, eps):
        if i != layer:
            return F.layer_norm(z, shape, weight, bias, eps)
        if kind in ("dz_scale", "dz_zero"):
            if z.requires_grad:
                def hook(g):
                    g = g.clone()
                    g[row] = g[row] * (factor if kind == "dz_scale" else 0.0)
                    return g
                z.register_hook(hook)
            return F.layer_norm(z, shape, weight, bias, eps)
        assert kind == "stats_swap"
        mean = z.mean(1, keepdim=True)
        var = z.var(1, unbiased=False, keepdim=True)
        perm = torch.arange(z.shape[0])
        perm[row], perm[row + 1] = row + 1, row
        return (z - mean[perm]) / torch.sqrt(var[perm] + eps) * weight + bias
    return ln
