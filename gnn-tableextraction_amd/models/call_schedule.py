"""The call-by-call schedule of :class:`~.engine.FusedGcnSageStep`: forward, loss and backward as ~19 C-ABI calls issued from
Python.  The step of every configuration no one-call plan covers (GTE_GEMM_MODE=f32, one layer or more than 8, layers without
LayerNorm), of GTE_C_STEP=0, of the kernel timers, and of the split data-parallel step (forward_backward(upto_layer=k) +
backward_rest)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib, ops


def batch_shape(g):
    """(feature image or None, node count, input width) of a graph or batch: resident batches in image mode bring ``feat_p3``."""
    xp = getattr(g, "feat_p3", None)
    n, f0 = (xp.rows, xp.cols) if xp is not None else g.ndata['feat'].shape
    return xp, n, f0


def f32_rows(g) -> torch.Tensor:
    """The fp32 feature rows of a graph or batch; one that brings the image only gets them back from it (exactly the fp32
    values; kept in ``g.ndata['feat']``)."""
    if 'feat' not in g.ndata:
        g.ndata['feat'] = ops.p3_to_f32(g.feat_p3)
    return ops._row_major(g.ndata['feat'])


def row_capacity(n: int, slack: bool = False) -> int:
    """Rows a shared buffer set is allocated for: ``n`` -- with ``slack`` an eighth more, so that the set of the largest batch seen
    so far also holds the slightly larger ones that follow -- rounded up to 4096."""
    return -(-int(n * 1.125 if slack else n) // 4096) * 4096


def weight_pair(W: torch.Tensor, transpose: int, img, row: int = 0, block: int = 0):
    """The two conversion descriptors (gte_p3_desc) of a layer's weight W = [W_s | W_n] ([fout][2 fin], or transposed: [fin] x
    [fout] each) into ONE image: the W_s half at the image's origin, then the W_n half at row ``row``, 16-column block ``block``."""
    fout, fin = W.shape[0], W.shape[1] // 2
    wp, ld = W.data_ptr(), W.stride(0)
    rows, cols = (fin, fout) if transpose else (fout, fin)
    return [_lib.P3Desc(wp, ld, rows, cols, transpose, img.at(0, 0), img.ldp),
            _lib.P3Desc(wp + 4 * fin, ld, rows, cols, transpose, img.at(row, block), img.ldp)]


@dataclass
class Pass:
    """One pass of the schedule over one batch: what the batch brings, the row views of the buffer set it runs on, and what the
    forward and the upper layers' backward tell the layers below.  Kept with that buffer set until layer 0's backward has run:
    backward_rest() of the data-parallel overlap continues the pass an earlier call began."""
    g: object
    x: Optional[torch.Tensor]       # fp32 rows of the input (None: layer 0 reads the image)
    xp: Optional[ops.P3]            # the batch's feature image when layer 0 reads it
    n: int
    f0: int
    b: dict                         # row views [0:n] of the buffer set
    layers: list
    csr: object
    rcsr: object
    w_in: torch.Tensor
    w_out: torch.Tensor
    hp_used: list                   # per layer: the input image its forward GEMM read (its dW GEMM reads the same)
    t_in: object = None             # tiles of both CSRs (large batches only)
    t_out: object = None
    st: int = 0                     # the stream of the current call
    head_scale: Optional[float] = None      # the fused head left 1 / sum(w) and the loss to the output layer's backward
    ln_p3_done: Optional[int] = None        # layer whose LayerNorm backward already ran as the epilogue of the launch above
    smallk_done: bool = False               # layer 0's whole backward already ran as the epilogue of layer 1's dX


class CallSchedule:
    """Owns the schedule's capacity-sized buffer sets (``bufs``: (input width, planes on) -> set; a captured batch's private sets go
    through the engine's _private_set) and its weight images (``wimg``: layer index -> (forward image, backward image or None)).
    Everything else -- library, model, flat tensors, switches, layer predicates, hooks -- is read from the engine at call time."""

    def __init__(self, engine):
        self.eng = engine
        self.bufs = {}
        self.wimg = {}

    # -- buffers -------------------------------------------------------------------------------------
    def _alloc(self, cap: int, f0: int):
        """Buffer set of the call-by-call schedule only; a one-call plan has its own (step_plan.OneCallPlan._alloc)."""
        eng = self.eng
        dev = eng.flat_param.device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        layers = eng.model.layers
        dims = [f0] + [l.out_feats for l in layers]
        tf = [eng._transform_first(l, dims[i]) for i, l in enumerate(layers)]
        qf = [self._qform(i, l, dims[i]) for i, l in enumerate(layers)]
        b = {"cap": cap,
             # aggregated input [cap, fin] of an aggregate-first layer; a q-form layer reuses it for q in the backward
             "ahn": [None if tf[i] else new(cap, dims[i]) for i in range(len(layers))],
             # transform-first layer: t = [x W_s^T + b | x W_n^T]; z is accumulated into the left half, q reuses the right
             "t": [new(cap, 2 * dims[i + 1]) if tf[i] else None for i in range(len(layers))],
             "z": [new(cap, dims[i + 1]) if (isinstance(l.lynorm, nn.LayerNorm) and not tf[i]) else None
                   for i, l in enumerate(layers)],
             "stats": [new(2 * cap) if isinstance(l.lynorm, nn.LayerNorm) else None for l in layers],
             "y": [new(cap, dims[i + 1]) for i in range(len(layers))],
             "dy": [new(cap, dims[i + 1]) for i in range(len(layers))],      # grad w.r.t. layer output (dz in place)
             "dahn": new(cap, max([dims[i] for i in range(1, len(layers)) if not qf[i] and not eng._narrow(layers[i], dims[i])]
                                  + [1])),
             "tn": new(cap, dims[-1]), "q": new(cap, dims[-1]),       # narrow (class-count-wide) output layer
             "out3": new(3)}
        lib = eng.lib
        # planes layers: P3 images of the layer input (layer 0: only when the batch does not bring one), of dz and of q, and
        # the split-K workspace of the dW planes GEMM
        pl = [eng._planes_layer(i, l, dims[i]) for i, l in enumerate(layers)]
        b["pl"] = pl
        b["hp"] = [ops.P3.empty(cap, dims[i], dev) if pl[i] else None for i in range(len(layers))]
        b["dzp"] = [ops.P3.empty(cap, dims[i + 1], dev) if pl[i] else None for i in range(len(layers))]
        b["qp"] = [ops.P3.empty(cap, dims[i + 1], dev) if pl[i] else None for i in range(len(layers))]
        b["ws_p3"] = [torch.empty(int(lib.gte_gemm_p3_tn_workspace_bytes(dims[i + 1], 2 * dims[i], dims[i], cap)), dtype=torch.uint8,
                                  device=dev) if pl[i] else None for i in range(len(layers))]
        for i in range(len(layers)):
            if pl[i] and b["t"][i] is None:
                b["t"][i] = new(cap, 2 * dims[i + 1])
        # every workspace requirement grows with the node count, so the capacity's requirement covers any n <= cap
        ws = max([lib.gte_weighted_ce_workspace_bytes(cap)] +
                 [lib.gte_ln_relu_bwd_workspace_bytes(cap, d) for d in dims[1:]] +
                 [lib.gte_gemm_workspace_bytes(dims[i + 1], dims[i], cap) for i in range(len(layers))] +
                 [lib.gte_sage_narrow_bwd_workspace_bytes(cap, min(dims[-2], 256), min(dims[-1], 16))])
        b["ws"] = torch.empty(int(ws), dtype=torch.uint8, device=dev)
        # the backward defers its partial-sum folds to one launch (gte_fold_defer_*): every producer keeps its partials
        # in a workspace of its own until the flush
        b["ws_ln"] = [torch.empty(int(max(lib.gte_ln_relu_bwd_workspace_bytes(cap, dims[i + 1]),
                                          lib.gte_gemm_p3_nt_ln_bwd_workspace_bytes(cap, dims[i + 1]),
                                          lib.gte_sage_narrow_bwd_ln_workspace_bytes(cap, min(dims[i + 1], 256)))),
                                  dtype=torch.uint8, device=dev) for i in range(len(layers))]
        b["ce_part"] = torch.empty(int(lib.gte_head_agg_ce_workspace_bytes(cap)), dtype=torch.uint8, device=dev)
        b["ws_nar"] = torch.empty(int(lib.gte_sage_narrow_bwd_workspace_bytes(cap, min(dims[-2], 256), min(dims[-1], 16))),
                                  dtype=torch.uint8, device=dev)
        # one private workspace per layer for the dW GEMMs: they run on the side stream, several at once
        b["ws_dw"] = [torch.empty(int(eng._ws_dw_bytes(i, dims, cap)), dtype=torch.uint8, device=dev) for i in range(len(layers))]
        return b

    def _full_set(self, n: int, f0: int):
        """The buffer set a pass over n nodes runs on, allocated for a CAPACITY, not for n: in the real loop every batch has a
        different node count, and per-count buffers would grow without bound (~300 MB per new count at F0=831).  The shared set
        grows geometrically to the largest batch seen.  A captured HIP graph bakes pointers in, so each captured batch owns a
        private exact-size set that is never reallocated."""
        eng = self.eng
        key = (f0, eng._planes_on())                  # the layer plan (which layers take P3 operands) depends on the GEMM mode
        if eng._private_key is not None:
            return eng._private_set(key, n, lambda m: self._alloc(m, f0))
        full = self.bufs.get(key)
        if full is None or full["cap"] < n:
            # (at least the reserved capacity: a shape whose steps usually run on a plan is not sized by reserve())
            full = self._grow(key, max(row_capacity(n, slack=True), eng._reserved.get(f0, 0)))
        return full

    def _grow(self, key, cap: int):
        self.bufs = {k: v for k, v in self.bufs.items() if k[0] != key[0]}     # one set per input width alive: the old one goes first
        full = self.bufs[key] = self._alloc(cap, key[0])
        return full

    def reserve(self, n_nodes: int, f0: int) -> None:
        """engine.reserve() where no one-call plan covers the configuration: the shared set for batches of up to n_nodes, now."""
        key = (f0, self.eng._planes_on())
        full = self.bufs.get(key)
        if n_nodes > 0 and (full is None or full["cap"] < n_nodes):
            self._grow(key, row_capacity(n_nodes))

    def buffer_set(self, batch, private_key=None):
        """The buffer set a step of this schedule on ``batch`` ran on -- the shared set, or the private set of the batch captured
        under ``private_key`` (see engine.plan_buffers) -- for tests and tools; None when no such step has run yet."""
        key = (batch_shape(batch)[2], self.eng._planes_on())
        return self.bufs.get(key) if private_key is None else self.eng._graph_bufs.get((private_key, key))

    @staticmethod
    def _views(full, n: int):
        """Row views [0:n] of a buffer set."""
        v = lambda t: None if t is None else t[:n]
        return {"ahn": [v(t) for t in full["ahn"]], "t": [v(t) for t in full["t"]], "z": [v(t) for t in full["z"]],
                "stats": [None if t is None else t[:2 * n] for t in full["stats"]], "y": [v(t) for t in full["y"]],
                "dy": [v(t) for t in full["dy"]], "dahn": v(full["dahn"]), "tn": v(full["tn"]), "q": v(full["q"]),
                "out3": full["out3"], "ws": full["ws"], "ws_ln": full["ws_ln"], "ws_nar": full["ws_nar"],
                "ce_part": full["ce_part"],
                "ws_dw": full["ws_dw"], "pl": full["pl"], "ws_p3": full["ws_p3"],
                "hp": [None if t is None else t.view_rows(n) for t in full["hp"]],
                "dzp": [None if t is None else t.view_rows(n) for t in full["dzp"]],
                "qp": [None if t is None else t.view_rows(n) for t in full["qp"]]}

    def _ln_rows_below(self, i: int, layers, fin: int, b) -> bool:
        """The output layer's backward runs the LayerNorm(+ReLU) backward of the PLANES layer below in the row form
        (gte_sage_narrow_bwd_ln_p3: dz as fp32 + image)."""
        eng = self.eng
        return (eng.fuse_ln_narrow and i > 0 and i == len(layers) - 1 and bool(b["pl"][i - 1])
                and eng._narrow(layers[i], fin) and fin % 16 == 0 and bool(eng.lib.gte_head_supported(fin, layers[i].out_feats)))

    def _qform(self, i: int, layer, fin: int) -> bool:
        """Backward through q = A_w^T(norm * dz): dW = [dz^T h | q^T h], dh = dz W_s + q W_n.  Always for a transform-first
        layer (nothing else was saved); for an inner layer when q is not wider than the classic dahn."""
        eng = self.eng
        if eng._narrow(layer, fin):
            return False
        return eng._transform_first(layer, fin) or (eng.transform_first and i > 0 and layer.out_feats <= fin)

    def _weight_images(self, dims):
        """The schedule's conversion launch: P3 images of the planes layers' weights, forward [W_s rows ; W_n rows]
        x fin, backward (dX) [fin rows] x [W_s^T | W_n^T].  ONE launch in front of every forward (the parameters change every step;
        the launch is part of a captured step).  A one-call plan has its own images and descriptors (OneCallPlan.weight_images)."""
        eng = self.eng
        layers = eng.model.layers
        descs = []
        for i, L in enumerate(layers):
            fin, fout = dims[i], L.out_feats
            if not eng._planes_layer(i, L, fin):
                continue
            img = self.wimg.get(i)
            if img is None:
                # (weight images are BLOCK-MAJOR: the B operand of every NT planes GEMM -- ops.P3)
                zeros = lambda rows, cols: ops.P3.zeros(rows, cols, eng.flat_param.device, block_major=eng.block_major_weights)
                img = self.wimg[i] = (zeros(2 * fout, fin), zeros(fin, 2 * fout) if i > 0 else None)
            fwd, bwd = img
            descs += weight_pair(L.linear.weight, 0, fwd, row=fout)
            if bwd is not None:
                descs += weight_pair(L.linear.weight, 1, bwd, block=fout // 16)
        st = _lib.current_stream()
        for k in range(0, len(descs), 16):
            chunk = descs[k:k + 16]
            arr = (_lib.P3Desc * len(chunk))(*chunk)
            _lib.check(eng.lib.gte_p3_from_f32_batch(ctypes.addressof(arr), len(chunk), st), "gte_p3_from_f32_batch")

    # -- the schedule ----------------------------------------------------------------------------------
    def _recorded(self, g):
        """The buffer set that holds the pass an earlier forward began on this very graph object."""
        pk = self.eng._private_key
        sets = self.bufs.values() if pk is None else [v for k, v in self.eng._graph_bufs.items() if k[0] == pk]
        for full in sets:
            ps = full.get("_pass")
            if ps is not None and ps.g is g:
                return full
        raise RuntimeError("backward_rest: no forward of this batch is recorded with the call-by-call schedule's buffers -- "
                           "forward_backward(g, labels, upto_layer=k) has to run on this very graph object first, with no other "
                           "batch on the same buffers in between")

    def _begin(self, g):
        """A new pass over ``g``, recorded with the buffer set it runs on (returned); converts the weight images."""
        eng = self.eng
        xp, n, f0 = batch_shape(g)                # resident batches in image mode bring the features as a P3 image only
        if xp is None:
            x = f32_rows(g)
            _lib.require_device(x, "FusedGcnSageStep")
        elif eng._planes_layer(0, eng.model.layers[0], f0, n):
            x = None
        else:
            # an image batch on a layer that reads fp32 rows (this schedule runs layer 0 on planes for fewer shapes than the
            # one-call plans, and does not know the cached-aggregate form; or the GEMM mode changed after the resident pages
            # were converted): the rows back from the image -- exactly the fp32 values
            x, xp = f32_rows(g), None
        full = self._full_set(n, f0)
        layers = list(eng.model.layers)
        ew = g.edata.get("feat")
        ps = full["_pass"] = Pass(g, x, xp, n, f0, self._views(full, n), layers, g.in_csr(), g.out_csr(), g.in_weights(ew),
                                  g.out_weights(ew, True), hp_used=[None] * len(layers))
        if any(ps.b["pl"]):
            self._weight_images([f0] + [l.out_feats for l in layers])
        if n * max(f0, max(l.out_feats for l in layers)) * 4 >= min(ops.TILED_FULL_MIN_BYTES, ops.TILED_MIN_BYTES):
            ps.t_in, ps.t_out = g.in_tiles(), g.out_tiles()
        return full

    def run(self, g, labels, grad_scale, hi: int, lo: int, forward: bool = True, with_adam: bool = False):
        """Forward and loss (``forward``), then the backward of layers hi .. lo with their folds flushed; lo > 0 leaves the pass
        with its buffer set, where a later call with ``forward`` False finds it.  ``with_adam``: the optimiser step rides in the
        fold launch of layer 0 when the folds allow.  Returns (out3, Adam ran in the fold launch)."""
        eng = self.eng
        lib, P, check = eng.lib, _lib.ptr, _lib.check
        full = self._begin(g) if forward else self._recorded(g)
        ps = full["_pass"]
        ps.st = _lib.current_stream()
        # (this schedule converts its own weight images in front of every forward: the one-call plans' no longer follow the
        # parameters, and no later optimiser launch may rewrite them)
        eng._plan.images.stale()
        # scratch for the GEMM tail split (see gte_gemm_set_tail_workspace): registered for this launch sequence only
        tail = eng._tail_workspace()
        check(lib.gte_gemm_set_tail_workspace(P(tail) if eng.tail_split else None, tail.numel() if eng.tail_split else 0),
              "gte_gemm_set_tail_workspace")
        fused = ctypes.c_int(0)
        try:
            if forward:
                self._forward_loss(ps, labels, grad_scale)
            # ---------------- backward of layers hi .. lo ----------------
            check(lib.gte_fold_defer_begin(ps.st), "gte_fold_defer_begin")
            try:
                self._backward(ps, hi, lo)
            finally:
                if with_adam and lo == 0:
                    # the folds produce every gradient element: the optimiser step rides in the same launch (falls back to a
                    # plain flush, fused = 0, when some gradient was written directly)
                    check(lib.gte_fold_defer_flush_adam(P(eng.flat_param), P(eng.flat_grad), P(eng.exp_avg), P(eng.exp_avg_sq),
                                                        eng.flat_param.numel(), P(eng._hyper), P(eng._step_dev),
                                                        P(eng._ticket), ctypes.byref(fused)), "gte_fold_defer_flush_adam")
                else:
                    check(lib.gte_fold_defer_flush(), "gte_fold_defer_flush")
            if lo == 0:
                full["_pass"] = None                  # (the pass is over: nothing of the batch is kept)
            return ps.b["out3"], bool(fused.value)
        finally:
            lib.gte_gemm_set_tail_workspace(None, 0)

    def _aggregate(self, ps, csr_, w_, tiles_, src, ldsrc, dst, lddst, f, reduce, accumulate):
        lib, P, check, timed, n = self.eng.lib, _lib.ptr, _lib.check, ops._timed, ps.n
        PP = lambda a: a if isinstance(a, int) else P(a)           # tensor or raw device address (a column offset into one)
        nbytes = 2.0 * n * f * 4 + 8.0 * csr_.indices.numel() + 4.0 * (n + 1)
        if tiles_ is not None and ops.use_tiled(n, f, csr_.indices.numel()):
            with timed("spmm_tiled", nbytes):
                check(lib.gte_spmm_csr_tiled(P(csr_.indptr), P(csr_.indices), P(tiles_.local_index), P(w_),
                                             P(tiles_.tile_ptr), P(tiles_.tile_src), PP(src), ldsrc, PP(dst), lddst,
                                             n, f, reduce, int(accumulate), ps.st), "gte_spmm_csr_tiled")
        else:
            fn = lib.gte_spmm_csr_accumulate if accumulate else lib.gte_spmm_csr
            with timed("spmm_csr", nbytes):
                check(fn(P(csr_.indptr), P(csr_.indices), P(w_), PP(src), ldsrc, PP(dst), lddst, n, f, _lib.GTE_F32,
                         reduce, ps.st), "gte_spmm_csr")

    def _forward_loss(self, ps, labels, grad_scale):
        eng = self.eng
        lib, P, check = eng.lib, _lib.ptr, _lib.check
        timed, ld = ops._timed, ops._ld
        x, n, f0, b, layers, csr, w_in, t_in, st = ps.x, ps.n, ps.f0, ps.b, ps.layers, ps.csr, ps.w_in, ps.t_in, ps.st
        ws, wsn = P(b["ws"]), b["ws"].numel()
        # ---------------- forward ----------------
        h = x
        fused_head = False
        pending_ln = None            # (layer, z, y, stats) of a LayerNorm left to the output layer's forward kernel
        hp_in = None                 # P3 image of the current layer's input (set by the producer of h)
        for i, L in enumerate(layers):
            fin, fout = (f0 if i == 0 else layers[i - 1].out_feats), L.out_feats
            W, bias = L.linear.weight, L.linear.bias
            ln = isinstance(L.lynorm, nn.LayerNorm)
            relu = L.activation is not None
            ahn, y = b["ahn"][i], b["y"][i]
            if b["pl"][i]:
                # ---- planes layer: t = h [W_s ; W_n]^T + [b | 0] (planes GEMM), then z = t_self + mean-self._aggregate(ps, t_neigh),
                # LayerNorm, ReLU in ONE pass that writes y as the next planes layer's input image (and / or fp32)
                if hp_in is None:
                    hp_in = ps.xp if (i == 0 and ps.xp is not None) else b["hp"][i]
                    if not (i == 0 and ps.xp is not None):
                        check(lib.gte_p3_from_f32(P(h), ld(h), n, fin, 0, P(hp_in.data), hp_in.ldp, st), "gte_p3_from_f32")
                ps.hp_used[i] = hp_in
                wf = self.wimg[i][0]
                t = b["t"][i]
                with timed("gemm_nt", 4.0 * n * fin * fout) as tm:
                    for _ in tm.repeat():
                        if hp_in.row_map is not None:      # the RESIDENT image through the batch's row map
                            check(lib.gte_gemm_p3_nt_rows(P(hp_in.data), hp_in.ldp, fin, P(hp_in.row_map), hp_in.res_rows, P(wf.data),
                                                          wf.ldp, P(bias), fout, P(t), 2 * fout, n, 2 * fout, 0, 0, st),
                                  "gte_gemm_p3_nt_rows")
                        else:
                            check(lib.gte_gemm_p3_nt(P(hp_in.data), hp_in.ldp, fin, None, 0, 0, P(wf.data), wf.ldp, P(bias), fout, P(t),
                                                     2 * fout, n, 2 * fout, 0, 0, st), "gte_gemm_p3_nt")
                nxt_planes = i + 1 < len(layers) and b["pl"][i + 1]
                yp = b["hp"][i + 1] if nxt_planes else None
                with timed("spmm_csr", 3.0 * n * fout * 4 + 8.0 * csr.indices.numel() + 4.0 * (n + 1)):
                    check(lib.gte_spmm_csr_accumulate_ln_p3(P(csr.indptr), P(csr.indices), P(w_in), P(t) + 4 * fout, 2 * fout, P(t),
                                                            2 * fout, n, fout, _lib.REDUCE_MEAN, P(L.lynorm.weight),
                                                            P(L.lynorm.bias), float(L.lynorm.eps), int(relu),
                                                            None if nxt_planes else P(y), fout,
                                                            P(yp.data) if yp is not None else None, yp.ldp if yp is not None else 0,
                                                            P(b["stats"][i]), st), "gte_spmm_csr_accumulate_ln_p3")
                h, hp_in = y, yp
                continue
            hp_in = None
            if eng._narrow(L, fin):
                # class-count-wide layer: logits = h W_s^T + b + mean-self._aggregate(ps, h W_n^T)  (aggregation on C columns)
                with timed("narrow_fwd", 2.0 * n * fin * 4):
                    if pending_ln is not None:
                        # the layer below left its pre-LayerNorm z: normalise, write y / stats and multiply in one pass
                        Lb, zb, yb, sb = pending_ln
                        check(lib.gte_sage_narrow_fwd_ln(P(zb), ld(zb), fin, P(Lb.lynorm.weight), P(Lb.lynorm.bias),
                                                         float(Lb.lynorm.eps), int(Lb.activation is not None), P(yb), fin, P(sb),
                                                         P(W), 2 * fin, P(bias), fout, P(y), fout, P(b["tn"]), fout, n, st),
                              "gte_sage_narrow_fwd_ln")
                        pending_ln = None
                    else:
                        check(lib.gte_sage_narrow_fwd(P(h), ld(h), fin, P(W), 2 * fin, P(bias), fout, P(y), fout, P(b["tn"]),
                                                      fout, n, st), "gte_sage_narrow_fwd")
                fused_head = eng._fused_head(i, L, fin)
                if not fused_head:
                    self._aggregate(ps, csr, w_in, None, b["tn"], fout, y, fout, fout, _lib.REDUCE_MEAN, True)
                h = y
                continue
            if eng._transform_first(L, fin):
                t = b["t"][i]
                with timed("gemm_nt", 4.0 * n * fin * fout) as tm:
                    for _ in tm.repeat():
                        check(lib.gte_sage_transform_fwd(P(h), ld(h), fin, P(W), 2 * fin, P(bias), fout, P(t), 2 * fout, n,
                                                         st), "gte_sage_transform_fwd")
                if (fout % 4 == 0 and lib.gte_spmm_csr_accumulate_ln_supported(fout)
                        and not (t_in is not None and ops.use_tiled(n, fout, csr.indices.numel(), fused_ln=True))):
                    # z = t_self + mean-self._aggregate(ps, t_neigh) and y = relu(LayerNorm(z)) in one pass over the rows
                    with timed("spmm_csr", 3.0 * n * fout * 4 + 8.0 * csr.indices.numel() + 4.0 * (n + 1)):
                        check(lib.gte_spmm_csr_accumulate_ln(P(csr.indptr), P(csr.indices), P(w_in), P(t) + 4 * fout, 2 * fout,
                                                             P(t), 2 * fout, n, fout, _lib.REDUCE_MEAN, P(L.lynorm.weight),
                                                             P(L.lynorm.bias), float(L.lynorm.eps), int(relu), P(y), fout,
                                                             P(b["stats"][i]), st), "gte_spmm_csr_accumulate_ln")
                else:
                    self._aggregate(ps, csr, w_in, t_in, P(t) + 4 * fout, 2 * fout, t, 2 * fout, fout, _lib.REDUCE_MEAN, True)
                    check(lib.gte_ln_relu_fwd(P(t), 2 * fout, P(L.lynorm.weight), P(L.lynorm.bias), float(L.lynorm.eps),
                                              int(relu), P(y), fout, P(b["stats"][i]), n, fout, st), "gte_ln_relu_fwd")
                h = y
                continue
            self._aggregate(ps, csr, w_in, t_in, h, ld(h), ahn, fin, fin, _lib.REDUCE_MEAN, False)
            if ln and lib.gte_sage_linear_fwd_fuses_ln(2 * fin, fout):
                # short K (BBOX features, 13 + 13 inputs): linear + LayerNorm + ReLU in one pass over the rows; when the next
                # layer is a planes layer its input image is written by the same pass (and y itself is not needed)
                zs = None if eng._smallk_bwd(i, L, fin) else P(b["z"][i])   # (the one-pass backward recomputes z)
                if i + 1 < len(layers) and b["pl"][i + 1] and fout % 16 == 0:
                    yp = b["hp"][i + 1]
                    check(lib.gte_sage_linear_fwd_p3(P(h), ld(h), fin, P(ahn), fin, fin, P(W), 2 * fin, P(bias), P(L.lynorm.weight),
                                                     P(L.lynorm.bias), float(L.lynorm.eps), int(relu), zs, fout,
                                                     P(b["stats"][i]), None, fout, P(yp.data), yp.ldp, n, fout, st),
                          "gte_sage_linear_fwd_p3")
                    h, hp_in = y, yp
                    continue
                check(lib.gte_sage_linear_fwd(P(h), ld(h), fin, P(ahn), fin, fin, P(W), 2 * fin, P(bias), P(L.lynorm.weight),
                                              P(L.lynorm.bias), float(L.lynorm.eps), int(relu), zs, fout,
                                              P(b["stats"][i]), P(y), fout, n, fout, st), "gte_sage_linear_fwd")
                h = y
                continue
            lin_out = b["z"][i] if ln else y
            with timed("gemm_nt", 4.0 * n * fin * fout) as tm:
                for _ in tm.repeat():
                    check(lib.gte_sage_linear_fwd(P(h), ld(h), fin, P(ahn), fin, fin, P(W), 2 * fin, P(bias), None, None,
                                                  1e-5, int(relu and not ln), None, 0, None, P(lin_out), fout, n, fout, st),
                          "gte_sage_linear_fwd")
            if ln:
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                if (eng.fuse_ln_fwd and nxt is not None and i + 1 == len(layers) - 1 and eng._narrow(nxt, fout)
                        and lib.gte_sage_narrow_fwd_ln_supported(fout, nxt.out_feats)):
                    pending_ln = (L, lin_out, y, b["stats"][i])
                else:
                    check(lib.gte_ln_relu_fwd(P(lin_out), fout, P(L.lynorm.weight), P(L.lynorm.bias), float(L.lynorm.eps),
                                              int(relu), P(y), fout, P(b["stats"][i]), n, fout, st), "gte_ln_relu_fwd")
            h = y
        logits = h

        # ---------------- loss ----------------
        lab = labels if labels.dtype in (torch.float32, torch.int64) else labels.to(torch.int64)
        dl = b["dy"][-1]
        if fused_head:
            # one launch: logits += mean-self._aggregate(ps, t_neigh), CE terms, UNNORMALISED gradient; 1 / sum(w) is applied (and
            # the loss published) by the output layer's backward kernel -- see gte_head_agg_ce in include/gte.h
            with timed("spmm_csr", 2.0 * n * logits.shape[1] * 4 + 8.0 * csr.indices.numel() + 4.0 * (n + 1)):
                check(lib.gte_head_agg_ce(P(csr.indptr), P(csr.indices), P(w_in), P(b["tn"]), logits.shape[1], P(logits),
                                          logits.shape[1], P(lab), int(lab.dtype == torch.float32), P(eng.class_weights), n,
                                          logits.shape[1], _lib.REDUCE_MEAN, P(dl), dl.shape[1], P(b["ce_part"]),
                                          b["ce_part"].numel(), st), "gte_head_agg_ce")
            ps.head_scale = float(grad_scale)
        else:
            check(lib.gte_weighted_ce(P(logits), logits.shape[1], P(lab), int(lab.dtype == torch.float32),
                                      P(eng.class_weights), n, logits.shape[1], float(grad_scale), P(dl), dl.shape[1],
                                      P(b["out3"]), ws, wsn, st), "gte_weighted_ce")

    def _backward(self, ps, hi: int, lo: int) -> None:
        eng = self.eng
        lib, P, check = eng.lib, _lib.ptr, _lib.check
        timed, ld = ops._timed, ops._ld
        x, n, b, layers, rcsr, w_out, t_out, st = ps.x, ps.n, ps.b, ps.layers, ps.rcsr, ps.w_out, ps.t_out, ps.st
        ws, wsn = P(b["ws"]), b["ws"].numel()
        for i in range(hi, lo - 1, -1):
            L = layers[i]
            hin = x if i == 0 else b["y"][i - 1]
            fin, fout = (L.linear.weight.shape[1] // 2), L.out_feats
            W = L.linear.weight
            ln = isinstance(L.lynorm, nn.LayerNorm)
            relu = L.activation is not None
            dy = b["dy"][i]
            gW = eng._gslice[id(W)]
            gb = eng._gslice[id(L.linear.bias)] if L.linear.bias is not None else None
            gg = eng._gslice[id(L.lynorm.weight)] if ln else None
            gbe = eng._gslice[id(L.lynorm.bias)] if ln else None
            if eng._narrow(L, fin):
                # q = A_w^T (norm * dlogits) on C columns; dW = [dl^T h | q^T h], dh = dl W_s + q W_n, dbias = colsum(dl)
                self._aggregate(ps, rcsr, w_out, None, dy, fout, b["q"], fout, fout, _lib.REDUCE_SUM, False)
                dh = b["dy"][i - 1] if i > 0 else None
                with timed("narrow_bwd", 3.0 * n * fin * 4):
                    if self._ln_rows_below(i, layers, fin, b):
                        # the LayerNorm(+ReLU) backward of the planes layer below on the dh tile of every row block (row form):
                        # d(loss)/d(y) of that layer is never stored, its dz comes out as fp32 + image
                        Lb, gsl, dzb, wsl = layers[i - 1], eng._gslice, b["dzp"][i - 1], b["ws_ln"][i - 1]
                        hs = ps.head_scale
                        check(lib.gte_sage_narrow_bwd_ln_p3(
                            P(dy), fout, P(b["q"]), fout, P(hin), ld(hin), fin, P(W), 2 * fin, fout, P(dh), fin,
                            P(dzb.data), dzb.ldp,
                            P(gW), 2 * fin, P(gb), n, P(b["ws_nar"]), b["ws_nar"].numel(), P(b["ce_part"]) if hs is not None else None,
                            hs if hs is not None else 1.0, P(b["out3"]) if hs is not None else None, P(b["t"][i - 1]), 2 * fin,
                            P(b["stats"][i - 1]), P(Lb.lynorm.weight), P(Lb.lynorm.bias), int(Lb.activation is not None),
                            P(gsl[id(Lb.lynorm.weight)]), P(gsl[id(Lb.lynorm.bias)]), P(gsl[id(Lb.linear.bias)]), P(wsl), wsl.numel(),
                            st), "gte_sage_narrow_bwd_ln_p3")
                        ps.ln_p3_done = i - 1
                    elif ps.head_scale is not None and i == len(layers) - 1:
                        check(lib.gte_sage_narrow_bwd_ce(P(dy), fout, P(b["q"]), fout, P(hin), ld(hin), fin, P(W), 2 * fin, fout,
                                                         P(dh), fin, P(gW), 2 * fin, P(gb), n, P(b["ws_nar"]),
                                                         b["ws_nar"].numel(), P(b["ce_part"]), ps.head_scale, P(b["out3"]),
                                                         st), "gte_sage_narrow_bwd_ce")
                    else:
                        check(lib.gte_sage_narrow_bwd(P(dy), fout, P(b["q"]), fout, P(hin), ld(hin), fin, P(W), 2 * fin, fout,
                                                      P(dh), fin, P(gW), 2 * fin, P(gb), n, P(b["ws_nar"]),
                                                      b["ws_nar"].numel(), st), "gte_sage_narrow_bwd")
                continue
            if b["pl"][i]:
                # ---- planes layer: dz (fp32 for the transpose aggregation + image), q = A_w^T (norm dz) as an image,
                # dW = [dz^T h | q^T h] and dh = dz W_s + q W_n on the planes GEMMs
                t, dzp, qp, hp = b["t"][i], b["dzp"][i], b["qp"][i], ps.hp_used[i]
                if ps.ln_p3_done != i:         # (else: the launch above ran this layer's LayerNorm backward as its epilogue)
                    check(lib.gte_ln_relu_bwd_p3(P(dy), fout, P(t), 2 * fout, P(b["stats"][i]), P(L.lynorm.weight),
                                                 P(L.lynorm.bias), int(relu), P(dy), fout, P(dzp.data), dzp.ldp, P(gg), P(gbe), P(gb),
                                                 n, fout, P(b["ws_ln"][i]), b["ws_ln"][i].numel(), st), "gte_ln_relu_bwd_p3")
                with timed("spmm_csr", 2.0 * n * fout * 4 + 8.0 * rcsr.indices.numel() + 4.0 * (n + 1)):
                    check(lib.gte_spmm_csr_p3(P(rcsr.indptr), P(rcsr.indices), P(w_out), P(dy), fout, P(qp.data), qp.ldp, n, fout,
                                              _lib.REDUCE_SUM, st), "gte_spmm_csr_p3")
                if i == 0 and eng.before_last_gemm is not None:
                    eng.before_last_gemm()
                wsp = b["ws_p3"][i]

                def dw_planes(stream):
                    if hp.row_map is not None:
                        check(lib.gte_gemm_p3_tn_rows(P(dzp.data), dzp.ldp, P(qp.data), qp.ldp, P(hp.data), hp.ldp, P(hp.row_map),
                                                      hp.res_rows, fin, P(gW), 2 * fin, fout, 2 * fin, n, P(wsp), wsp.numel(), stream),
                              "gte_gemm_p3_tn_rows")
                    else:
                        check(lib.gte_gemm_p3_tn(P(dzp.data), dzp.ldp, P(qp.data), qp.ldp, P(hp.data), hp.ldp, None, 0, fin, P(gW),
                                                 2 * fin, fout, 2 * fin, n, P(wsp), wsp.numel(), stream), "gte_gemm_p3_tn")
                with timed("gemm_tn", 4.0 * n * fin * fout) as tm:
                    for _ in tm.repeat():
                        dw_planes(st)
                if i > 0:
                    wb = self.wimg[i][1]
                    Lb = layers[i - 1]
                    fin_b = Lb.linear.weight.shape[1] // 2
                    if (eng.fuse_smallk_dx and i == 1 and eng._smallk_bwd(0, Lb, fin_b)
                            and lib.gte_gemm_p3_nt_smallk_bwd_supported(2 * fin_b, fin)):
                        # dX with the WHOLE backward of the short-input layer below as its epilogue: nothing of layer 0 is left
                        gsl, wsd = eng._gslice, b["ws_dw"][0]
                        check(lib.gte_gemm_p3_nt_smallk_bwd(P(dzp.data), dzp.ldp, fout, P(qp.data), qp.ldp, fout, P(wb.data), wb.ldp,
                                                            P(x), ld(x), fin_b, P(b["ahn"][0]), fin_b, fin_b, P(Lb.linear.weight),
                                                            2 * fin_b, P(Lb.linear.bias), P(Lb.lynorm.weight), P(Lb.lynorm.bias),
                                                            P(b["stats"][0]), int(Lb.activation is not None), P(gsl[id(Lb.linear.weight)]),
                                                            2 * fin_b, P(gsl[id(Lb.linear.bias)]), P(gsl[id(Lb.lynorm.weight)]),
                                                            P(gsl[id(Lb.lynorm.bias)]), n, fin, P(wsd), wsd.numel(), st),
                              "gte_gemm_p3_nt_smallk_bwd")
                        ps.smallk_done = True
                    elif eng.fuse_ln_dx and b["pl"][i - 1] and lib.gte_gemm_p3_nt_ln_bwd_supported(fin):
                        # dX with the LayerNorm(+ReLU) backward of the layer below as its epilogue: d(loss)/d(y) of that layer
                        # is never stored, its dz comes out as fp32 + image
                        gsl, dzb, wsl = eng._gslice, b["dzp"][i - 1], b["ws_ln"][i - 1]
                        check(lib.gte_gemm_p3_nt_ln_bwd(P(dzp.data), dzp.ldp, fout, P(qp.data), qp.ldp, fout, P(wb.data), wb.ldp,
                                                        P(b["t"][i - 1]), 2 * fin, P(b["stats"][i - 1]), P(Lb.lynorm.weight),
                                                        P(Lb.lynorm.bias), int(Lb.activation is not None), P(b["dy"][i - 1]), fin,
                                                        P(dzb.data), dzb.ldp, P(gsl[id(Lb.lynorm.weight)]), P(gsl[id(Lb.lynorm.bias)]),
                                                        P(gsl[id(Lb.linear.bias)]), n, fin, P(wsl), wsl.numel(), st),
                              "gte_gemm_p3_nt_ln_bwd")
                        ps.ln_p3_done = i - 1
                    else:
                        with timed("gemm_nn", 4.0 * n * fin * fout) as tm:
                            for _ in tm.repeat():
                                check(lib.gte_gemm_p3_nt(P(dzp.data), dzp.ldp, fout, P(qp.data), qp.ldp, fout, P(wb.data), wb.ldp, None,
                                                         0, P(b["dy"][i - 1]), fin, n, fin, 0, 0, st), "gte_gemm_p3_nt dX")
                continue
            if eng._smallk_bwd(i, L, fin) and ps.smallk_done:
                if eng.before_last_gemm is not None:                  # (its backward ran as the epilogue of the layer above's dX)
                    eng.before_last_gemm()
                continue
            if eng._smallk_bwd(i, L, fin):
                # short-input layer 0: LayerNorm(+ReLU) backward and dW in ONE pass over dy (z recomputed, dz never stored)
                if eng.before_last_gemm is not None:
                    eng.before_last_gemm()
                wdw = b["ws_dw"][i]
                check(lib.gte_sage_smallk_bwd(P(dy), fout, P(hin), ld(hin), fin, P(b["ahn"][i]), fin, fin, P(W), 2 * fin,
                                              P(L.linear.bias), P(L.lynorm.weight), P(L.lynorm.bias), P(b["stats"][i]), int(relu),
                                              P(gW), 2 * fin, P(gb), P(gg), P(gbe), n, fout, P(wdw), wdw.numel(), st),
                      "gte_sage_smallk_bwd")
                continue
            tfirst, qform = eng._transform_first(L, fin), self._qform(i, L, fin)
            zsrc = b["t"][i] if tfirst else (b["z"][i] if ln else b["y"][i])
            # dz in place of dy; column sums straight into the flat gradient
            check(lib.gte_ln_relu_bwd(P(dy), fout, P(zsrc), 2 * fout if tfirst else fout, P(b["stats"][i]) if ln else None,
                                      P(L.lynorm.weight) if ln else None, P(L.lynorm.bias) if ln else None, int(relu),
                                      P(dy), fout, P(gg), P(gbe), P(gb), n, fout, P(b["ws_ln"][i]), b["ws_ln"][i].numel(),
                                      st), "gte_ln_relu_bwd")
            dz, ahn = dy, b["ahn"][i]
            if qform:
                # q = A_w^T (norm * dz) into the dead right half of t (transform-first) or the dead ahn buffer
                qp, ldq = (P(b["t"][i]) + 4 * fout, 2 * fout) if tfirst else (P(ahn), fin)
                self._aggregate(ps, rcsr, w_out, t_out, dz, fout, qp, ldq, fout, _lib.REDUCE_SUM, False)
            # dW is MFMA-bound and nothing downstream needs it before Adam; the rest of the backward chain (dX, the
            # transpose aggregation, the next LayerNorm backward) is mostly HBM-bound: run dW on the side stream so
            # the two kinds of work share the chip.  dz (= dy_i, final for this step) and ahn/h are read-only here.
            wdw = b["ws_dw"][i]
            if i == 0 and eng.before_last_gemm is not None:
                eng.before_last_gemm()

            def dw_launch(stream):
                if qform:
                    check(lib.gte_sage_qform_dw(P(dz), fout, qp, ldq, P(hin), ld(hin), fin, P(gW), 2 * fin, fout, n, P(wdw),
                                                wdw.numel(), stream), "gte_sage_qform_dw")
                else:
                    check(lib.gte_sage_linear_dw(P(dz), fout, P(hin), ld(hin), fin, P(ahn), fin, fin, P(gW), 2 * fin, fout,
                                                 n, P(wdw), wdw.numel(), stream), "gte_sage_linear_dw")
            with timed("gemm_tn", 4.0 * n * fin * fout) as tm:
                for _ in tm.repeat():
                    dw_launch(st)
            if i > 0 and qform:
                with timed("gemm_nn", 4.0 * n * fin * fout) as tm:
                    for _ in tm.repeat():
                        check(lib.gte_sage_qform_dx(P(dz), fout, qp, ldq, P(W), 2 * fin, fin, fout, P(b["dy"][i - 1]), fin, n,
                                                    st), "gte_sage_qform_dx")
            elif i > 0:
                dh, dahn = b["dy"][i - 1], b["dahn"]
                with timed("gemm_nn", 4.0 * n * fin * fout):
                    check(lib.gte_gemm_f32(0, 0, n, fin, fout, P(dz), fout, P(W), 2 * fin, P(dh), fin, 0, ws, wsn, st),
                          "gte_gemm_f32 dh_self")
                    check(lib.gte_gemm_f32(0, 0, n, fin, fout, P(dz), fout, P(W) + 4 * fin, 2 * fin, P(dahn), fin, 0, ws,
                                           wsn, st), "gte_gemm_f32 dh_neigh")
                self._aggregate(ps, rcsr, w_out, t_out, dahn, fin, dh, fin, fin, _lib.REDUCE_SUM, True)
