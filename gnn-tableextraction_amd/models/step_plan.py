"""The one-call plan of :class:`~.engine.FusedGcnSageStep`: the whole step (gte_gcnsage_step) or the evaluation forward
(gte_gcnsage_forward) as ONE host call on a gte_step_plan -- its buffer sets, its weight images, the binder and the two drivers --
and the one owner of the question whether those weight images still follow the parameters (:class:`ImageFreshness`)."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib, ops
from .._lib import LAYER_PLANES, LAYER_SMALLK, LAYER_AGGFIRST, LAYER_CACHED, LAYER_DROPOUT
from .call_schedule import batch_shape, f32_rows, row_capacity, weight_pair


def _c16(x: int) -> int:
    return -(-int(x) // 16) * 16


class ImageFreshness:
    """Whether the weight images of the one-call plans follow the parameters.  The fold + Adam launch of a one-call step also
    writes the weight images of the updated parameters (gte_fold_defer_flush_adam_images) and the next forward skips their
    conversion launch -- a mistake here faults nothing: the next forward multiplies by last step's weights.  The invariant, which
    these methods alone maintain (nothing else assigns the two fields):

    * the images of plan key K are current when they were written from parameters whose version counters (engine._param_sig) are
      S: ``sig`` = (S, K), None = stale.  In-place writes through torch (load_state_dict, p.copy_, flat_param.copy_) move the
      counters; raw writes through ``p.data`` do not: engine.invalidate_weight_images() then;
    * nothing is ever current during capture (a captured launch has not run; the graph's own forward converts);
    * an unfused optimiser launch may rewrite the images of the step that just ran, and of that step only.
    """

    def __init__(self, engine):
        self._eng = engine
        self.sig = None                               # read by engine._wimg_sig
        self._left = None
        self._seen = None                             # what fresh() read, for the wrote() of the same plan call

    def fresh(self, key, capturing: bool) -> bool:
        """The images of plan ``key`` were written from the parameters as they are now."""
        eng = self._eng
        self._seen = (eng._param_sig(), key)          # (reading the version counters is ~20 us of host time: once per plan call)
        return bool(eng.wimg_in_fold and not capturing and self.sig == self._seen)

    def stale(self) -> None:
        """The parameters change, or changed, behind the images: invalidate_weight_images(), a call-by-call pass, a replay."""
        self.sig = self._left = self._seen = None

    def begin(self) -> None:
        """A plan call starts: stale until it says :meth:`wrote` (a call that raises leaves them stale), and what an earlier step
        left for the optimiser is dropped."""
        self.sig = self._left = None

    def wrote(self, key, capturing: bool) -> None:
        """The fold launch, the forward's conversion or gte_adam_step_dev_images wrote the images of plan ``key`` from the
        parameters as they are now -- for a plan call, as its own :meth:`fresh` saw them: the call's kernels write the parameters
        raw and move no version counter (an older signature can only read as stale later, never as fresh)."""
        seen, self._seen = self._seen, None
        if not capturing:
            self.sig = seen if seen is not None and seen[1] == key else (self._eng._param_sig(), key)

    def leave_for_optimiser(self, descs, n_descs: int, key, keep) -> None:
        """The step that just ran left Adam to a launch of its own, which may rewrite that step's images through ``descs``
        (``keep``: what holds the descriptor array and the image tensors it points into alive until then)."""
        self._left = (descs, n_descs, key, keep)

    def take_for_optimiser(self):
        """An optimiser launch begins: the images are stale (it says :meth:`wrote` if it rewrites them); returns what the last
        step left for it -- (descs, n_descs, key, keep) or None -- once."""
        left = self._left
        self.stale()
        return left


class OneCallPlan:
    """Owns the plans' capacity-sized buffer sets (``bufs``: :meth:`key` -> set, with the bound gte_step_plan structures of the
    set under ``"_plans"``; a captured batch's private sets go through the engine's _private_set), their weight-image sets
    (``wimg``: key -> (images, descriptor array, count)) and the images' freshness (``images``).  Everything else -- library,
    model, flat tensors, gradient slices, switches, layer predicates, hooks, the Adam state -- is read from the engine at call time."""

    def __init__(self, engine):
        self.eng = engine
        self.bufs = {}
        self.wimg = {}
        self.images = ImageFreshness(engine)
        self._keep = ()                               # what the last call's plan points at: alive until the next call
        self._fwd_ev_arr = None

    # -- buffers (padded rows) -------------------------------------------------------------------------
    def _alloc(self, cap: int, f0: int, kinds, out_gemm: bool):
        """Buffer set of a one-call plan: the fp32 row buffers of a hidden layer are PADDED to ld = hidden rounded up to 16 floats
        (include/gte.h, gte_step_layer.ldf; no padding at a 16-aligned width), zero-initialised once (the kernels keep the padding
        zero); images are padded to 16-column blocks by construction."""
        eng = self.eng
        dev, lib = eng.flat_param.device, eng.lib
        layers = list(eng.model.layers)
        dims = [f0] + [l.out_feats for l in layers]
        nh = len(layers) - 1
        ld = [_c16(d) for d in dims[1:nh + 1]]
        z32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        u8 = lambda nbytes: torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        img = lambda rows, cols: ops.P3.zeros(rows, cols, dev)
        b = {"cap": cap, "ld": ld}
        b["t"] = [z32(cap, 2 * ld[i]) if kinds[i] == LAYER_PLANES else z32(cap, ld[i]) for i in range(nh)]     # [t_self | t_neigh], or z
        b["y"] = [z32(cap, ld[i]) for i in range(nh)]
        b["dy"] = [z32(cap, ld[i]) for i in range(nh)]
        b["stats"] = [z32(2 * cap) for _ in range(nh)]
        b["ahn"] = [z32(cap, dims[0]) if kinds[i] == LAYER_SMALLK else None for i in range(nh)]
        b["ahnp"] = [img(cap, dims[i]) if kinds[i] in (LAYER_AGGFIRST, LAYER_DROPOUT) else None for i in range(nh)]
        # a dropout layer above layer 0: G = dz W [n][2 ceil16(fin)] (self half, then the aggregate half from column ceil16(fin))
        b["g"] = [z32(cap, 2 * _c16(dims[i])) if (kinds[i] == LAYER_DROPOUT and i > 0) else None for i in range(nh)]
        # (a cached layer reads both operands from resident images)
        b["hp"] = [img(cap, dims[i]) if kinds[i] not in (LAYER_SMALLK, LAYER_CACHED) else None for i in range(nh)]
        b["dzp"] = [img(cap, dims[i + 1]) if kinds[i] != LAYER_SMALLK else None for i in range(nh)]
        b["qp"] = [img(cap, dims[i + 1]) if kinds[i] == LAYER_PLANES else None for i in range(nh)]
        b["ws_dw"] = [u8(lib.gte_gemm_p3_tn_workspace_bytes(dims[i + 1], 2 * dims[i], dims[i], cap) if kinds[i] != LAYER_SMALLK
                         else eng._ws_dw_bytes(i, dims, cap)) for i in range(nh)]
        b["ws_ln"] = [u8(max(lib.gte_ln_relu_bwd_workspace_bytes(cap, dims[i + 1]),
                             lib.gte_gemm_p3_nt_ln_bwd_workspace_bytes(cap, dims[i + 1]) if dims[i + 1] <= 256 else 0,
                             lib.gte_sage_narrow_bwd_ln_workspace_bytes(cap, min(_c16(dims[i + 1]), 256)))) for i in range(nh)]
        C = dims[-1]
        b["out3"] = z32(3)
        if out_gemm:
            b["hp_out"] = img(cap, dims[-2])                       # image of the last hidden layer's output
            b["t_out"], b["dlq"] = z32(cap, 32), z32(cap, 32)      # [logits .. | t_neigh ..], [dl .. | q ..]
            b["dlqp"] = img(cap + 8, 32)
            b["ws_out"] = u8(lib.gte_gemm_p3_tn_workspace_bytes(C, 2 * dims[-2], dims[-2], cap))
            b["ws_ce"] = u8(max(lib.gte_weighted_ce_workspace_bytes(cap), lib.gte_head_agg_ce_workspace_bytes(cap)))
            b["ws_cs"] = u8(max(lib.gte_colsum_workspace_bytes(cap, C), lib.gte_head_dlq_finish_workspace_bytes(cap)))
        else:
            b["logits"], b["tn"], b["q"], b["dl"] = z32(cap, C), z32(cap, C), z32(cap, C), z32(cap, C)
            b["ce_part"] = u8(lib.gte_head_agg_ce_workspace_bytes(cap))
            b["ws_nar"] = u8(lib.gte_sage_narrow_bwd_workspace_bytes(cap, min(_c16(dims[-2]), 256), min(C, 16)))
        return b

    @staticmethod
    def key(f0: int, kinds, out_gemm: bool):
        """What names a one-call plan's layout: the key of its buffer set and of its weight-image set."""
        return ("gen", f0, tuple(kinds), bool(out_gemm))

    def _buffers(self, key, n: int):
        """The (capacity-sized, shared or captured-batch-private) buffer set of the plan ``key``; see CallSchedule._full_set."""
        eng = self.eng
        _gen, f0, kinds, out_gemm = key
        if eng._private_key is not None:
            return eng._private_set(key, n, lambda m: self._alloc(m, f0, kinds, out_gemm))
        full = self.bufs.get(key)
        if full is None or full["cap"] < n:
            self.bufs.pop(key, None)
            full = self.bufs[key] = self._alloc(max(row_capacity(n, slack=True), eng._reserved.get(f0, 0)), f0, kinds, out_gemm)
        return full

    def buffers(self, batch, private_key=None):
        """engine.plan_buffers()."""
        eng = self.eng
        _xp, n, f0 = batch_shape(batch)
        kinds = eng._plan_kinds(f0, n, eng._batch_cached(batch))
        if kinds is None:
            return None
        out_gemm = eng._plan_mode(kinds, f0)[1]
        key = self.key(f0, kinds, out_gemm)
        full = self.bufs.get(key) if private_key is None else eng._graph_bufs.get((private_key, key))
        return None if full is None else (full, kinds, out_gemm)

    # -- weight images ---------------------------------------------------------------------------------
    def weight_images(self, dims, kinds, out_gemm: bool):
        """Weight images of a one-call plan (kept per :meth:`key`) and their conversion descriptors.  A planes layer's forward
        image holds [W_s rows ; zero rows up to ld ; W_n rows ; zero rows] (ld = fout rounded up to 16: the two halves of t start on
        16-column boundaries), its backward image [fin] x [W_s^T | W_n^T] with the second segment at column block ld / 16; an
        aggregate-first layer's image is [fout] x [W_s | W_n] with the second K segment at block ceil(fin / 16); the output
        layer's images are [32] x [H] (rows 0.. = W_s, 16.. = W_n) and [H] x [32].  Allocated zeroed: the padding is never written."""
        key = self.key(dims[0], kinds, out_gemm)
        hit = self.wimg.get(key)
        if hit is not None:
            return hit
        eng = self.eng
        layers = list(eng.model.layers)
        # (weight images are BLOCK-MAJOR: the B operand of every NT planes GEMM -- ops.P3)
        img = lambda rows, cols: ops.P3.zeros(rows, cols, eng.flat_param.device, block_major=eng.block_major_weights)
        imgs, descs = {}, []
        for i, k in enumerate(kinds):
            fin, fout = dims[i], layers[i].out_feats
            W = layers[i].linear.weight
            bwd = None
            if k == LAYER_PLANES:
                ld = _c16(fout)
                fwd = img(2 * ld, fin)
                descs += weight_pair(W, 0, fwd, row=ld)
                if i > 0:
                    bwd = img(fin, 2 * ld)
                    descs += weight_pair(W, 1, bwd, block=ld // 16)
            elif k in (LAYER_AGGFIRST, LAYER_CACHED, LAYER_DROPOUT):
                kp = _c16(fin)
                fwd = img(fout, 2 * kp)
                descs += weight_pair(W, 0, fwd, block=kp // 16)
                if k == LAYER_DROPOUT and i > 0:
                    # G = dz W: the image [2 kp][fout] = [W_s^T ; zero rows ; W_n^T from row kp ; zero rows] (B operand of an NT GEMM)
                    bwd = img(2 * kp, fout)
                    descs += weight_pair(W, 1, bwd, row=kp)
            else:
                continue
            imgs[i] = (fwd, bwd)
        if out_gemm:
            W = layers[-1].linear.weight
            fwd, bwd = img(32, dims[-2]), img(dims[-2], 32)
            descs += weight_pair(W, 0, fwd, row=16) + weight_pair(W, 1, bwd, block=1)
            imgs["out"] = (fwd, bwd)
        if len(descs) > 32:
            raise _lib.GteError("gte_gcnsage_step: more than 32 weight images")
        arr = (_lib.P3Desc * max(len(descs), 1))(*descs)
        hit = self.wimg[key] = (imgs, arr, len(descs))
        return hit

    # -- the binder ------------------------------------------------------------------------------------
    def _build(self, b, key, with_adam: bool):
        """What is bound ONCE per buffer set ``b`` (and cached with it, whose addresses it holds): the gte_step_plan with every
        field that does not depend on the batch -- layers, parameters and their gradient slices, buffers, weight images, the
        Adam state.  Returns (plan, fused flag, key, the weight-image set the plan points into)."""
        eng, P = self.eng, _lib.ptr
        _gen, f0, kinds, out_gemm = key
        layers = list(eng.model.layers)
        dims = [f0] + [l.out_feats for l in layers]
        nh = len(layers) - 1
        wset = self.weight_images(dims, kinds, out_gemm)
        imgs, arr, n_desc = wset
        plan = _lib.StepPlan()
        plan.n_hidden = nh
        gs = eng._gslice
        for i, L in enumerate(layers[:-1]):
            sl = plan.layer[i]
            fin, fout = dims[i], L.out_feats
            sl.kind, sl.fin, sl.fout, sl.ldf = kinds[i], fin, fout, b["ld"][i]
            sl.W, sl.bias, sl.gamma, sl.beta = P(L.linear.weight), P(L.linear.bias), P(L.lynorm.weight), P(L.lynorm.bias)
            sl.eps, sl.relu = float(L.lynorm.eps), int(L.activation is not None)
            sl.gW, sl.gbias = P(gs[id(L.linear.weight)]), P(gs[id(L.linear.bias)])
            sl.ggamma, sl.gbeta = P(gs[id(L.lynorm.weight)]), P(gs[id(L.lynorm.bias)])
            last_hidden = i == nh - 1
            nxt_img = (not last_hidden and kinds[i + 1] == LAYER_PLANES) or (last_hidden and out_gemm)
            # the layer's output: as an image for a planes consumer, as fp32 rows for the narrow output kernels
            if nxt_img:
                yp = b["hp_out"] if last_hidden else b["hp"][i + 1]
                sl.yp, sl.ldp_y = P(yp.data), yp.ldp
            sl.y = P(b["y"][i]) if (last_hidden and not out_gemm) or not nxt_img else None
            sl.t, sl.stats, sl.dy = P(b["t"][i]), P(b["stats"][i]), P(b["dy"][i])
            sl.ws_ln, sl.ws_ln_bytes = P(b["ws_ln"][i]), b["ws_ln"][i].numel()
            sl.ws_dw, sl.ws_dw_bytes = P(b["ws_dw"][i]), b["ws_dw"][i].numel()
            if kinds[i] == LAYER_SMALLK:
                sl.ahn = P(b["ahn"][i])
                continue
            wf, wb = imgs[i]
            sl.wimg_fwd, sl.ldp_wfwd = P(wf.data), wf.ldp
            if wb is not None:
                sl.wimg_bwd, sl.ldp_wbwd = P(wb.data), wb.ldp
            sl.dzp, sl.ldp_o = P(b["dzp"][i].data), b["dzp"][i].ldp
            if kinds[i] == LAYER_CACHED:
                continue                                      # (both operand images are the batch's: bound per call)
            sl.hp, sl.ldp_h = P(b["hp"][i].data), b["hp"][i].ldp
            if kinds[i] == LAYER_DROPOUT:
                # the masked operand images [D(x') | D(ahn')]; above layer 0 the input is y of the layer below, and G
                sl.ahnp, sl.ldp_ahn = P(b["ahnp"][i].data), b["ahnp"][i].ldp
                if i > 0:
                    sl.x, sl.ldx = P(b["y"][i - 1]), b["ld"][i - 1]
                    sl.g, sl.ldg = P(b["g"][i]), b["g"][i].shape[1]
                continue
            if kinds[i] == LAYER_PLANES:
                sl.qp = P(b["qp"][i].data)
            else:
                sl.ahnp, sl.ldp_ahn = P(b["ahnp"][i].data), b["ahnp"][i].ldp
        Lo = layers[-1]
        plan.out_fin, plan.n_classes = dims[-2], Lo.out_feats
        plan.W_out, plan.b_out = P(Lo.linear.weight), P(Lo.linear.bias)
        plan.gW_out, plan.gb_out = P(gs[id(Lo.linear.weight)]), P(gs[id(Lo.linear.bias)])
        plan.ld_h_out = b["ld"][-1]
        plan.dh_out = P(b["dy"][-1])
        if out_gemm:
            wf, wb = imgs["out"]
            plan.out_gemm, plan.ld_lg = 1, 32
            plan.hp_out, plan.ldp_hout = P(b["hp_out"].data), b["hp_out"].ldp
            plan.wimg_out_fwd, plan.ldp_wout_fwd = P(wf.data), wf.ldp
            plan.wimg_out_bwd, plan.ldp_wout_bwd = P(wb.data), wb.ldp
            plan.logits, plan.tn = P(b["t_out"]), P(b["t_out"]) + 64
            plan.dl, plan.q_out = P(b["dlq"]), P(b["dlq"]) + 64
            plan.dlqp, plan.ldp_dlq = P(b["dlqp"].data), b["dlqp"].ldp
            plan.ws_out, plan.ws_out_bytes = P(b["ws_out"]), b["ws_out"].numel()
            plan.ws_ce, plan.ws_ce_bytes = P(b["ws_ce"]), b["ws_ce"].numel()
            plan.ws_cs, plan.ws_cs_bytes = P(b["ws_cs"]), b["ws_cs"].numel()
        else:
            plan.h_out = P(b["y"][-1])
            plan.logits, plan.tn, plan.q_out, plan.dl = P(b["logits"]), P(b["tn"]), P(b["q"]), P(b["dl"])
            plan.ce_part, plan.ce_part_bytes = P(b["ce_part"]), b["ce_part"].numel()
            plan.ws_nar, plan.ws_nar_bytes = P(b["ws_nar"]), b["ws_nar"].numel()
        plan.out3 = P(b["out3"])
        plan.wimg_descs, plan.n_wimg_descs = ctypes.addressof(arr), n_desc
        if with_adam:
            plan.param, plan.grad, plan.exp_avg, plan.exp_avg_sq = (P(eng.flat_param), P(eng.flat_grad), P(eng.exp_avg),
                                                                    P(eng.exp_avg_sq))
            plan.n_param = eng.flat_param.numel()
            plan.hyper, plan.step_counter, plan.ticket = P(eng._hyper), P(eng._step_dev), P(eng._ticket)
        tail = eng._tail_workspace()
        if eng.tail_split:
            plan.tail_ws, plan.tail_ws_bytes = P(tail), tail.numel()
        return plan, ctypes.c_int(0), key, wset

    def _bind_input(self, L0, kind, b, g, xp, x) -> None:
        """Layer 0's input, per call, once per kind: LAYER_SMALLK and LAYER_AGGFIRST read fp32 rows (``x``); LAYER_PLANES and
        LAYER_CACHED read an image (``hp``) and LAYER_DROPOUT an image (``xp``) or fp32 rows.  The image is the batch's own --
        resident rows behind its row map when it brings one -- and a planes layer whose batch brings fp32 rows makes its image
        from them (``make_hp``); a cached layer reads the batch's aggregate image beside it."""
        P = _lib.ptr
        if kind in (LAYER_SMALLK, LAYER_AGGFIRST):
            # (an image-only batch on a layer that reads fp32 rows -- copied image rows without the aggregate image, GTE_P3_ROWS=0 --
            # gets the rows back from the image: slow, a measurement configuration)
            x = f32_rows(g) if x is None else x
            L0.x, L0.ldx = P(x), ops._ld(x)
            return
        ap = getattr(g, "agg_p3", None) if kind == LAYER_CACHED else None
        if kind == LAYER_CACHED and (xp is None or ap is None):
            raise _lib.GteError("a cached-aggregate input layer needs feat_p3 and agg_p3 (resident images behind a row map, or the graph's own)")
        src = xp if xp is not None else (b["hp"][0] if kind == LAYER_PLANES else None)
        image = (None, 0) if src is None else (P(src.data), src.ldp)
        if kind == LAYER_DROPOUT:
            L0.xp, L0.ldp_x = image
        else:
            L0.hp, L0.ldp_h = image
            L0.make_hp = int(xp is None)
        L0.x, L0.ldx = (P(x), ops._ld(x)) if xp is None else (None, 0)
        L0.h_rows, L0.n_res_rows = (P(xp.row_map), xp.res_rows) if xp is not None and xp.row_map is not None else (None, 0)
        if ap is not None:
            L0.ahnp, L0.ldp_ahn = P(ap.data), ap.ldp

    def _bind(self, g, kinds, with_adam: bool):
        """The gte_step_plan of this layer plan (:meth:`_build`, cached under ``"_plans"`` of the buffer set) with what is set per
        call -- switches, class weights, layer 0's input, the graph, the node count -- set for ``g``.  Returns (what _build
        returned, buffer set, node count, tensors the plan points at)."""
        eng, P = self.eng, _lib.ptr
        xp, n, f0 = batch_shape(g)
        x = None
        if xp is None:
            x = f32_rows(g)
            _lib.require_device(x, "FusedGcnSageStep")
        key = self.key(f0, kinds, eng._plan_mode(kinds, f0)[1])
        b = self._buffers(key, n)
        ew = g.edata.get("feat")
        csr, rcsr = g.in_csr(), g.out_csr()
        w_in, w_out = g.in_weights(ew), g.out_weights(ew, True)
        plans = b.setdefault("_plans", {})
        bound = plans.get(with_adam)
        if bound is None:
            bound = plans[with_adam] = self._build(b, key, with_adam)
        plan = bound[0]
        plan.class_weights = P(eng.class_weights)
        plan.fuse_ln_dx = (int(eng.fuse_ln_dx) | (2 if eng.fuse_ln_narrow else 0) | (8 if eng.fuse_smallk_dx else 0)
                           | (4 if eng.fuse_head_gemm else 0) | (16 if eng.fuse_ln_fwd else 0))
        self._bind_input(plan.layer[0], kinds[0], b, g, xp, x)
        if kinds[0] == LAYER_DROPOUT:
            # the masks of this seed / rank at the device step counter
            eng._adam_state()
            plan.dropout_p, plan.dropout_seed, plan.rank = float(eng.dropout_p), eng.dropout_seed, eng.rank
            plan.step_counter = P(eng._step_dev)
        plan.indptr, plan.indices, plan.w_in = P(csr.indptr), P(csr.indices), P(w_in)
        plan.rindptr, plan.rindices, plan.w_out = P(rcsr.indptr), P(rcsr.indices), P(w_out)
        plan.n_nodes = n
        return bound, b, n, (csr, rcsr, w_in, w_out, eng.class_weights)

    # -- the drivers -----------------------------------------------------------------------------------
    def step(self, g, labels, grad_scale, kinds, with_adam: bool):
        """forward + loss + backward (+ Adam inside the fold launch) through gte_gcnsage_step: two host calls (the next batch's
        assembly is queued between them) instead of ~19.  Returns out3."""
        eng, P = self.eng, _lib.ptr
        lib = eng.lib
        st = _lib.current_stream()
        (plan, fused, key, wset), b, _n, keep = self._bind(g, kinds, with_adam)
        lab = labels if labels.dtype in (torch.float32, torch.int64) else labels.to(torch.int64)
        plan.labels, plan.labels_f32 = P(lab), int(lab.dtype == torch.float32)
        plan.grad_scale = float(grad_scale)
        if eng.fwd_events:
            for e in eng.fwd_events:
                if not e.cuda_event:                  # (created lazily by the first record)
                    e.record()
            self._fwd_ev_arr = (ctypes.c_void_p * len(eng.fwd_events))(*[e.cuda_event for e in eng.fwd_events])
            plan.fwd_events = ctypes.addressof(self._fwd_ev_arr)
        else:
            plan.fwd_events = None
        capturing = torch.cuda.is_current_stream_capturing()
        plan.wimg_fresh = int(self.images.fresh(key, capturing))
        plan.wimg_in_fold = int(eng.wimg_in_fold and with_adam and not capturing)
        self.images.begin()
        addr = ctypes.addressof(plan)
        if eng.before_last_gemm is not None:
            _lib.check(lib.gte_gcnsage_step(addr, 1, ctypes.byref(fused), st), "gte_gcnsage_step")
            # phase 1 returned with this thread's fold deferral OPEN and the tail workspace registered: whatever the callback (the
            # next batch's assembly) or phase 2 raises, both are closed again -- a step that died here must not poison the next
            # one ("a deferral is already open") or let later standalone calls queue folds nobody flushes
            try:
                eng.before_last_gemm()
                _lib.check(lib.gte_gcnsage_step(addr, 2, ctypes.byref(fused), st), "gte_gcnsage_step")
            except BaseException:
                lib.gte_fold_defer_flush()                      # (an error if phase 2 already closed it: ignored)
                lib.gte_gemm_set_tail_workspace(None, 0)
                raise
        else:
            _lib.check(lib.gte_gcnsage_step(addr, 0, ctypes.byref(fused), st), "gte_gcnsage_step")
        eng._adam_fused = bool(fused.value & 1)
        # the images now hold: the updated parameters (written by the fold launch), or -- no optimiser step in this call -- the
        # unchanged ones the forward converted; otherwise Adam follows as its own launch and they are stale
        if (fused.value & 2) or not with_adam:
            self.images.wrote(key, capturing)
        self._keep = (lab,) + keep
        # (the data-parallel step's own Adam launch writes the same images, gte_adam_step_dev_images: left only while an UNFUSED
        # optimiser launch may still follow this very step -- a step whose fold launch already ran Adam must not leave descriptors
        # behind for a later launch of another plan)
        if not capturing and not (fused.value & 1):
            self.images.leave_for_optimiser(plan.wimg_descs, int(plan.n_wimg_descs), key, wset)
        return b["out3"]

    def forward(self, g, kinds) -> torch.Tensor:
        """The plan half of engine.forward_logits(): logits [n, n_classes] through ONE host call (gte_gcnsage_forward), a view of
        the plan's own buffers."""
        (plan, _fused, key, _wset), b, n, keep = self._bind(g, kinds, with_adam=False)
        capturing = torch.cuda.is_current_stream_capturing()
        plan.wimg_fresh = int(self.images.fresh(key, capturing))
        self.images.begin()
        _lib.check(self.eng.lib.gte_gcnsage_forward(ctypes.addressof(plan), _lib.current_stream()), "gte_gcnsage_forward")
        self.images.wrote(key, capturing)             # (the forward converted them, or they were fresh)
        self._keep = keep
        return b["t_out"][:n, :plan.n_classes] if plan.out_gemm else b["logits"][:n]

    def wide_layers(self, g) -> int:
        """engine.wide_layers()."""
        eng = self.eng
        _xp, n, f0 = batch_shape(g)
        kinds = eng._plan_kinds(f0, n, eng._batch_cached(g))
        if kinds is None or eng.dropout_p == 0:
            return 0
        plan = self._bind(g, kinds, with_adam=bool(eng._fuse_adam_req))[0][0]
        rc = int(eng.lib.gte_gcnsage_step_wide_layers(ctypes.addressof(plan)))
        if rc < 0:
            _lib.check(rc, "gte_gcnsage_step_wide_layers")
        return rc
