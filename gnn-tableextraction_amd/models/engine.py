"""One optimisation step of the node classifier on the HIP path, single- or multi-GPU.

Restates the reference's batch loop body (src/models/model_train.py:320-332:
``logits = model(g); loss = CE(logits, labels.long()); zero_grad; backward; optimizer.step()``)
over ONE flat fp32 parameter buffer and ONE flat gradient buffer:
  * the model's parameters are views into ``flat_param``; their ``.grad`` are views into
    ``flat_grad`` (autograd accumulates in place), so the optimiser is one fused Adam launch
    (gte_adam_step: torch.optim.Adam semantics, L2-coupled weight decay) and
  * data parallelism is ONE RCCL all-reduce of ``flat_grad`` per step (page graphs never share
    edges, so there is no other exchange).  Each rank's loss is a mean over ITS nodes; scaling it
    by n_local / n_global before backward makes the summed gradient equal to the single-GPU
    gradient of the mean over all nodes.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops
from .._lib import LAYER_PLANES, LAYER_SMALLK, LAYER_AGGFIRST, LAYER_CACHED, LAYER_DROPOUT
from ..components.graphs.models import GcnSAGE, _is_relu
from .call_schedule import CallSchedule, batch_shape, f32_rows, row_capacity
from .step_plan import OneCallPlan, _c16


class TrainStep:
    def __init__(self, model: torch.nn.Module, lr: float = 0.01, weight_decay: float = 5e-4,
                 class_weights: Optional[torch.Tensor] = None, betas=(0.9, 0.999), eps: float = 1e-8,
                 process_group=None, distributed: bool = False):
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = lr, weight_decay, betas, eps
        self.class_weights = class_weights
        self.distributed = distributed
        self.group = process_group
        params = [p for p in model.parameters() if p.requires_grad]
        dev = params[0].device
        total = sum(p.numel() for p in params)
        self.flat_param = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        for p in params:
            n = p.numel()
            self.flat_param[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_param[off:off + n].view_as(p)
            p.grad = self.flat_grad[off:off + n].view_as(p)
            off += n
        self.t = 0
        if distributed:
            import torch.distributed as dist
            dist.broadcast(self.flat_param, src=0, group=process_group)   # same initial weights everywhere

    def _dp_scale(self, n_local: int, n_global: Optional[int], loss_scale: Optional[float]) -> float:
        """Factor on the local loss so that the SUM of the ranks' gradients is the single-GPU gradient.
        Unweighted CE is a mean over nodes: n_local / n_global.  With class weights the local loss is
        sum(w nll) / sum_local(w) (nn.CrossEntropyLoss(weight), model_train.py:171) and the factor is
        sum_local(w) / sum_global(w): the caller, who knows every rank's labels from the shared plan, passes it as
        ``loss_scale`` -- a node-count ratio would silently optimise a different objective."""
        if loss_scale is not None:
            return float(loss_scale)
        if not (self.distributed and n_global):
            return 1.0
        if self.class_weights is not None:
            raise ValueError("data-parallel step with class weights needs loss_scale = sum_local(w) / sum_global(w) "
                             "(distributed.step_weight_sums); n_local / n_global is only right for unweighted CE")
        return float(n_local) / float(n_global)

    def step(self, g, labels: torch.Tensor, n_global: Optional[int] = None,
             loss_scale: Optional[float] = None) -> torch.Tensor:
        """Forward, loss, backward, (all-reduce), Adam.  Returns the device vector
        [loss (local mean), sum of class weights, #correct] without synchronising."""
        self.model.train()
        self.flat_grad.zero_()
        logits = self.model(g)
        loss, out3 = self._loss(logits, labels)
        scale = self._dp_scale(labels.shape[0], n_global, loss_scale)
        if scale != 1.0:
            loss = loss * scale
        loss.backward()
        if self.distributed:
            import torch.distributed as dist
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=self.group)
        self.t += 1
        self._optimizer_step()
        return out3

    # the two arithmetic pieces of the step; HIP here (tests of the DP logic override them on CPU)
    def _loss(self, logits, labels):
        return ops.cross_entropy(logits, labels, self.class_weights)

    def _optimizer_step(self) -> None:
        ops.adam_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.t, self.lr,
                      self.betas[0], self.betas[1], self.eps, self.weight_decay)

    # checkpoint-compatible with torch.optim.Adam's state_dict layout is handled by model_train.py
    def lr_scale(self, factor: float) -> None:
        self.lr *= factor


# ======================================================================================================
# Hand-scheduled step for GcnSAGE: no autograd, no per-step allocation, HIP-graph capturable
# ======================================================================================================
DROPOUT_MAX_ROWS = 1 << 30          # GTE_DROPOUT_MAX_ROWS of include/gte.h: nodes of a dropout plan


def _switch(name: str, default: str = "1") -> bool:
    """An on / off switch of the engine, from the environment."""
    return os.environ.get(name, default) == "1"


class FusedGcnSageStep(TrainStep):
    """The same optimisation step as :class:`TrainStep` for a :class:`GcnSAGE` model, scheduled by hand:

    * forward and backward are explicit sequences of C-ABI calls (aggregation, split-weight GEMM,
      LayerNorm/ReLU, CE, LayerNorm backward, dW / dX GEMMs, transpose aggregation) -- no autograd
      graph, no Python allocation per step (buffers are cached per node count);
    * parameter gradients are written by the kernels DIRECTLY into their slices of ``flat_grad`` (every
      producer overwrites, so the buffer is never zeroed and never accumulated into);
    * nothing in a step synchronises or allocates, so a step on a resident batch can be captured
      into a HIP graph (:meth:`capture`) and replayed with one launch -- the page-batch regime is a few
      dozen 10-300 us kernels, where per-launch host time would otherwise bound the step.
    Requires ReLU (or no) activations and use_pp False; anything else goes through the autograd path (:class:`TrainStep`).
    Dropout 0 < p < 1 (``GcnSAGE(..., dropout=p)``, the reference's ``--dropout``) runs on the one-call plan with every hidden
    layer as GTE_LAYER_DROPOUT: counter-based masks (csrc/dropout.h) of ``dropout_seed`` (default: torch.initial_seed()), the
    data-parallel rank and the device step counter, regenerated by the kernels that need them -- captured replays draw fresh masks.
    Evaluation (forward_logits) applies no dropout.
    """

    def __init__(self, model: GcnSAGE, dropout_seed: Optional[int] = None, **kw):
        if not isinstance(model, GcnSAGE):
            raise TypeError("FusedGcnSageStep needs a GcnSAGE model")
        for layer in model.layers:
            if layer.use_pp or not (layer.activation is None or _is_relu(layer.activation)):
                raise ValueError("FusedGcnSageStep supports ReLU/None activations and use_pp False")
        # dropout: the input dropout (models.py:105-113) and every hidden layer's mask over cat(h, ah * norm) share ONE p (GcnSAGE's
        # constructor); the output layer has none
        ps = {float(model.dropout.p)} | {float(l.dropout.p) if l.dropout else 0.0 for l in model.layers[:-1]}
        if len(ps) != 1 or (model.layers[-1].dropout and model.layers[-1].dropout.p > 0):
            raise ValueError("FusedGcnSageStep: the input and every hidden layer need the same dropout p, the output layer none")
        p = ps.pop()
        if not 0.0 <= p < 1.0:
            raise ValueError(f"FusedGcnSageStep supports dropout 0 <= p < 1 (got {p}): p = 1 drops every input")
        self.dropout_p = p
        self.dropout_seed = int(torch.initial_seed() if dropout_seed is None else dropout_seed) & ((1 << 64) - 1)
        super().__init__(model, **kw)
        self.rank = 0
        if self.distributed:
            import torch.distributed as dist
            self.rank = int(dist.get_rank(self.group))
        self.lib = _lib.load()
        # slices of the flat gradient, in model.parameters() order
        self._gslice = {}
        off = 0
        for p in (q for q in model.parameters() if q.requires_grad):
            self._gslice[id(p)] = self.flat_grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        # data-parallel overlap (GTE_DP_OVERLAP=1): the flat gradient is [layer 0 | layers 1..]; the upper slice is all-reduced
        # while layer 0's backward (the longest: its dW GEMM alone is a quarter of the step) still runs.  Off by default: with
        # ONE rank (RCCL process group, trivial collective) the split step costs 0.804 ms against 0.760 ms for one all-reduce
        # behind one graph (0.748 ms without data parallelism) -- cutting the graph and the second collective cost ~45 us,
        # about what hiding a 0.5 MB all-reduce can win back on 8 GPUs.  To be re-measured on a multi-GPU node.
        self._n0 = sum(p.numel() for p in model.layers[0].parameters() if p.requires_grad)
        first_upper = next((p for p in model.layers[1].parameters() if p.requires_grad), None) if len(model.layers) > 1 else None
        self._dp_split = (_switch("GTE_DP_OVERLAP", "0") and first_upper is not None and self.dropout_p == 0
                          and self._gslice[id(first_upper)].storage_offset() == self._n0)
        self._graph_bufs = {}                         # (captured batch, buffer-set key of either schedule) -> its private set
        self._reserved = {}                           # input width -> capacity asked for by reserve()
        self._calls = CallSchedule(self)              # the call-by-call schedule: its own buffer sets and weight images
        self._plan = OneCallPlan(self)                # the one-call plans: their buffer sets, weight images and the images' freshness
        self._private_key = None
        self._graphs = {}
        self._graph_owner = {}
        # transform-then-aggregate where a layer narrows + q-form backward (see _transform_first / _qform); "0" keeps
        # the reference's aggregate-then-transform order everywhere (same math, different summation order)
        self.transform_first = _switch("GTE_TRANSFORM_FIRST")
        self.tail_split = _switch("GTE_TAIL_SPLIT")
        # single-GPU steps: the Adam update runs inside the gradient-fold launch (gte_fold_defer_flush_adam)
        self.fuse_adam = _switch("GTE_FUSE_ADAM")
        self._fuse_adam_req, self._adam_fused = False, False
        self.adam_fused_steps = 0                     # steps whose optimiser update ran inside the fold launch
        self.fused_head = _switch("GTE_FUSED_HEAD")
        self.fuse_head_gemm = _switch("GTE_FUSE_HEAD_GEMM")     # (out_gemm plans: the fused head on the GEMM output path)
        # dX of a planes layer with the LayerNorm(+ReLU) backward of the planes layer below as its epilogue (gte_gemm_p3_nt_ln_bwd)
        self.fuse_ln_dx = _switch("GTE_FUSE_LN_DX")
        # ... and of the last hidden layer inside the output layer's backward (gte_sage_narrow_bwd_ln_p3)
        self.fuse_ln_narrow = _switch("GTE_FUSE_LN_NARROW")
        # dX of layer 1 with the whole backward of a short-input layer 0 as its epilogue (gte_gemm_p3_nt_smallk_bwd)
        self.fuse_smallk_dx = _switch("GTE_FUSE_SMALLK_DX")
        # LayerNorm(+ReLU) forward of the last hidden layer inside the output layer's forward kernel (gte_sage_narrow_fwd_ln):
        # one launch and one pass over [n, hidden] less
        self.fuse_ln_fwd = _switch("GTE_FUSE_LN_FWD")
        self._tail_ws = None
        # planes path (GTE_PLANES=0 disables): in the split-bf16 GEMM mode the operands of the transform GEMMs are written as P3
        # images (three bf16 planes, csrc/p3.h) by their producers and multiplied by the planes GEMMs (csrc/gemm_p3.hip)
        self.use_planes = _switch("GTE_PLANES")
        # ... for EVERY hidden width up to 1024 and any input width through the one-call plan (padded rows, masked LayerNorm
        # kernels, aggregate-first input layer, output layer on the planes GEMMs); GTE_PLANES_GENERAL=0: the tuned range only
        self.general_planes = _switch("GTE_PLANES_GENERAL")
        # input layer on the CACHED mean aggregate of the input (graph.ResidentPages.build_agg_image: page-local, constant over a
        # run): z = [x | ahn] W^T from two resident images behind the batch's row map, no aggregation / q / feature copy in the
        # step for layer 0 (GTE_LAYER_CACHED).  Costs a second resident image; GTE_CACHE_AGG=0 turns it off
        self.cache_input_agg = _switch("GTE_CACHE_AGG")
        # weight images in the block-major layout (ops.P3): a K block of the weights is ONE contiguous run, whole cache lines for
        # every NT planes GEMM, and the block-major-weights kernel (gemm_p3_nt_sq_kernel) loads its fragments straight into
        # registers.  GTE_WIMG_BLOCK_MAJOR=0: row-major images (the layout up to round 5; A/B measurements, tests)
        self.block_major_weights = _switch("GTE_WIMG_BLOCK_MAJOR")
        # one-call step: the fold + Adam launch also writes the weight images of the updated parameters
        # (gte_fold_defer_flush_adam_images) and the next step's forward skips their conversion launch; whether the images still
        # follow the parameters is step_plan.ImageFreshness's to say (``_plan.images``; read here as ``_wimg_sig``)
        self.wimg_in_fold = _switch("GTE_WIMG_IN_FOLD")
        # optimiser state on the device, made at the first step (_adam_state)
        self._hyper, self._step_dev, self._ticket, self._hyper_host, self._step_dev_host = None, None, None, None, 0
        # the whole step through ONE C entry point (gte_gcnsage_step) when the configuration allows (GTE_C_STEP=0: call by call)
        self.use_c_step = _switch("GTE_C_STEP")
        # called (once per step, no arguments) right before the LAST big kernel of a step is launched -- layer 0's dW GEMM,
        # MFMA-bound, ~a quarter of the step.  The train loop hangs the assembly of the NEXT batch here (models/loop.py):
        # it then runs on the side stream under that GEMM, and the batch is still in the Infinity Cache when the next
        # step's first GEMM reads it.
        self.before_last_gemm = None
        # measurement hook of the one-call step (bench.py): a list of 2 x n_hidden torch.cuda.Event(enable_timing=True), recorded
        # around the forward transform GEMM of every hidden layer of the NEXT steps (None: off)
        self.fwd_events = None
        if self.dropout_p > 0 and self._plan_kinds(model.layers[0].in_feats, 0) is None:
            # dropout runs on the one-call plan only (the call-by-call schedule has no masks): a model the plan does not cover --
            # hidden width > 1024, more than 8 layers or 16 classes, GTE_C_STEP=0, GTE_PLANES_GENERAL=0, op timers -- is refused
            # here, where the caller can still take the autograd path (model_train.train does)
            raise ValueError(f"FusedGcnSageStep: dropout {self.dropout_p} runs on the one-call plan, which does not cover this model / "
                             "configuration; use TrainStep")

    # -- buffers -------------------------------------------------------------------------------------
    def _ws_dw_bytes(self, i: int, dims, cap: int) -> int:
        """Workspace of layer i's weight-gradient launch: split-K slabs of the dW GEMM; for the input layer additionally the
        partials of the one-pass short-input backward -- only where that path exists (k1 + k2 <= 28: at F0 = 831 the size
        functions, which do not check support, would ask for 764 + 382 MB per buffer set)."""
        lib = self.lib
        need = [lib.gte_sage_linear_dw_workspace_bytes(dims[i + 1], dims[i], dims[i], cap),
                lib.gte_sage_qform_dw_workspace_bytes(dims[i + 1], dims[i], cap)]
        if i == 0 and lib.gte_sage_smallk_bwd_supported(2 * dims[0], dims[1]):
            need.append(lib.gte_sage_smallk_bwd_workspace_bytes(cap, 2 * dims[0], dims[1]))
        if i == 0 and len(dims) > 2 and lib.gte_gemm_p3_nt_smallk_bwd_supported(2 * dims[0], dims[1]):
            need.append(lib.gte_gemm_p3_nt_smallk_bwd_workspace_bytes(cap, 2 * dims[0], dims[1]))
        return max(need)

    def _tail_workspace(self) -> torch.Tensor:
        """Scratch of the GEMM tail split (gte_gemm_set_tail_workspace), made at first use: both schedules register the same one."""
        if self._tail_ws is None:
            self._tail_ws = torch.empty(int(self.lib.gte_gemm_tail_workspace_bytes()), dtype=torch.uint8, device=self.flat_param.device)
        return self._tail_ws

    def _private_set(self, key, n: int, alloc):
        """The exact-size buffer set ``key`` of the batch being captured (made by ``alloc(n)`` at first use, never reallocated)."""
        k2 = (self._private_key, key)
        full = self._graph_bufs.get(k2)
        if full is None:
            full = self._graph_bufs[k2] = alloc(n)
        if full["cap"] < n:
            raise RuntimeError(f"captured batch buffers hold {full['cap']} nodes; asked for {n} (a captured batch must not change)")
        return full

    def plan_buffers(self, batch, private_key=None):
        """(buffer set, layer kinds, out_gemm) of the one-call plan a training step on ``batch`` runs on -- the shared set, or the
        private set of the batch captured under ``private_key`` (capture(): ``id`` of its graph) -- for tests and tools that read
        what a step left behind.  None when that step is not on a plan (call-by-call schedule), or no such step has run yet."""
        return self._plan.buffers(batch, private_key)

    def reserve(self, n_nodes: int, f0: int, cached: bool = False) -> None:
        """Size the shared per-batch buffers for batches of up to ``n_nodes`` nodes (the train loop knows the largest batch
        its page table can produce): no reallocation -- a device synchronisation plus ~12 KB per node of new buffers -- later,
        in the middle of an epoch.  A one-call plan takes the recorded capacity when it allocates its set at the first step
        (``cached``: the batches bring the aggregate image); the call-by-call schedule's set is allocated here."""
        self._reserved[f0] = max(self._reserved.get(f0, 0), row_capacity(n_nodes))
        if self._plan_kinds(f0, 0, cached) is not None:
            return                      # a one-call plan allocates its own set (OneCallPlan._buffers) at this capacity on first use
        self._calls.reserve(n_nodes, f0)

    def _narrow(self, layer, fin: int) -> bool:
        return (not isinstance(layer.lynorm, nn.LayerNorm) and layer.activation is None and layer.linear.bias is not None
                and bool(self.lib.gte_sage_narrow_supported(fin, layer.out_feats)))

    def _narrow_padded(self, layer, fin: int) -> bool:
        """The narrow output kernels on PADDED hidden rows (gte_sage_narrow_fwd_pad / gte_sage_narrow_bwd_ln_p3_pad): a hidden width
        that is not a multiple of 8 -- 100 / 139 / 149 / 157 / 206 / 218 of the reference's scaled runs -- up to 256 after padding
        to 16; needs the fused head and the LayerNorm backward inside the output layer's backward (the padded form has no other)."""
        return (self.general_planes and self.fused_head and self.fuse_ln_narrow and fin % 8 != 0
                and bool(self.lib.gte_sage_narrow_pad_supported(fin, _c16(fin), layer.out_feats)))

    def _fused_head(self, i: int, layer, fin: int) -> bool:
        """Output layer + weighted CE as gte_head_agg_ce / gte_sage_narrow_bwd_ce (the last, narrow layer only)."""
        return (self.fused_head and i == len(self.model.layers) - 1 and self._narrow(layer, fin)
                and bool(self.lib.gte_head_supported(fin, layer.out_feats)))

    def _transform_first(self, layer, fin: int) -> bool:
        """Forward as  z = h W_s^T + b + mean-aggregate(h W_n^T)  when the layer narrows (831 -> 256): the aggregation
        moves out_feats columns instead of fin (gte_sage_transform_fwd)."""
        return (self.transform_first and isinstance(layer.lynorm, nn.LayerNorm) and layer.linear.bias is not None
                and not self._narrow(layer, fin) and fin > layer.out_feats)

    # -- planes path ---------------------------------------------------------------------------------
    def _planes_on(self) -> bool:
        return self.use_planes and self.transform_first and ops.get_gemm_mode() == ops.GEMM_SPLIT_BF16

    def _planes_layer(self, i: int, layer, fin: int, n: int = 0) -> bool:
        """Layer i runs  t = h [W_s ; W_n]^T (planes GEMM),  z = t_self + b + mean-aggregate(t_neigh), LayerNorm, ReLU  with P3
        operands: a LayerNorm layer that does not widen (the aggregation then moves out_feats <= fin columns), 16-aligned
        widths the fused aggregation + LayerNorm kernel and the P3 LayerNorm backward cover."""
        fout = layer.out_feats
        return (self._planes_on() and isinstance(layer.lynorm, nn.LayerNorm) and layer.linear.bias is not None
                and not self._narrow(layer, fin) and fin >= fout and fin >= 16 and fout % 16 == 0 and 128 <= fout <= 256
                and (i == 0 or fin % 16 == 0)              # inner layers get their input image from a producer epilogue
                and bool(self.lib.gte_spmm_csr_accumulate_ln_supported(fout))
                and not (n and ops.use_tiled(n, fout, None, fused_ln=True)))

    def wants_p3_features(self, f0: int, train: bool = True) -> bool:
        """True when layer 0 takes its input as a P3 image: the train loop then keeps the resident features as images and
        assembles batches of image rows (graph.ResidentPages.enable_p3)."""
        L = self.model.layers[0]
        return self._layer_kind(0, L, f0, train=train) == LAYER_PLANES

    def _param_sig(self):
        return (self.flat_param._version,) + tuple(p._version for p in self.model.parameters())

    @property
    def _wimg_sig(self):
        """(version counters of the parameters, plan key) the one-call plans' weight images were written from; None: stale.
        Read-only: step_plan.ImageFreshness owns it."""
        return self._plan.images.sig

    def invalidate_weight_images(self) -> None:
        """The parameters were changed behind torch's version counters (a raw ``p.data`` write, a foreign kernel): the next
        forward converts the weight images again."""
        self._plan.images.stale()

    # -- the whole step as one host call (gte_gcnsage_step) ---------------------------------------------
    def _smallk_bwd(self, i: int, layer, fin: int) -> bool:
        """Layer 0 with a short input (BBOX features) and LayerNorm: forward in one pass (gte_sage_linear_fwd_fuses_ln) and the
        whole backward in one pass (gte_sage_smallk_bwd); z is then never saved."""
        return (i == 0 and isinstance(layer.lynorm, nn.LayerNorm) and layer.linear.bias is not None
                and not self._transform_first(layer, fin) and not self._planes_layer(i, layer, fin, 1 << 20)
                and bool(self.lib.gte_sage_linear_fwd_fuses_ln(2 * fin, layer.out_feats))
                and bool(self.lib.gte_sage_smallk_bwd_supported(2 * fin, layer.out_feats)))

    def _cached_layer0(self, L, fin: int) -> bool:
        """Layer 0 can run on the cached mean aggregate of the input (GTE_LAYER_CACHED) when the batch brings it: any LayerNorm
        layer on the planes path (the tuned one-pass kernels of the 13-feature input at aligned hidden widths keep their path)."""
        # (hidden widths below 128 keep the transform-first order: their input GEMM is bound by the operand stream, and the cached
        # form reads two input images where transform-first reads one -- measured (831, 96) 62 against 71 M nodes/s, (781, 100) 58
        # against 66; from 139 columns up the cached form wins 4 - 6 %: profiles/r05/cache_agg_ab.txt)
        return (self.cache_input_agg and self.general_planes and self._planes_on() and isinstance(L.lynorm, nn.LayerNorm)
                and L.linear.bias is not None and (L.activation is None or _is_relu(L.activation))
                and 128 <= L.out_feats <= 1024)

    def wants_agg_image(self, f0: int, train: bool = True) -> bool:
        """True when the train loop (``train`` False: an evaluation loop, which applies no dropout) should keep the image of the
        input's mean aggregate next to the feature image (graph.ResidentPages.enable_p3(agg=True))."""
        L = self.model.layers[0]
        if train and self.dropout_p > 0:
            return False                  # (layer 0 aggregates the DROPPED input: a cached aggregate of x is of no use)
        return (len(self.model.layers) >= 2 and self._cached_layer0(L, f0)
                and self._layer_kind(0, L, f0, train=train) in (LAYER_PLANES, LAYER_AGGFIRST))

    def wants_resident_images(self, f0: int, train: bool = True) -> bool:
        """True when the train loop should keep the resident features as images (and hand out row-map batches): layer 0 takes its
        input as an image (wants_p3_features), or it is a widening aggregate-first layer that can run on the cached aggregate --
        63 / 313 / 363 -> 1000, 63 -> 206 of the reference's runs: without the cache such a layer copies its fp32 rows per batch and
        makes both images per step."""
        if train and self.dropout_p > 0:  # a dropout layer 0 reads the resident feature image through the batch's row map
            return self._layer_kind(0, self.model.layers[0], f0) == LAYER_DROPOUT
        return self.wants_p3_features(f0, train) or self.wants_agg_image(f0, train)

    def _layer_kind(self, i: int, L, fin: int, n: int = 0, cached: bool = False, train: bool = True):
        """How hidden layer i runs on the one-call plan (gte_step_layer.kind): 0 planes layer in transform-first order, 1 the
        one-pass short-input layer (BBOX features), 2 aggregate-first planes input layer (fin < fout), 3 (``cached``: the batch
        brings the resident image of the input's mean aggregate) the input layer on [x | ahn] from two resident images; None: not on the plan.
        Every shape the reference's runs produce is covered (run_multiple_train.sh:8-113: hidden 1000, or
        int(calculate_hidden) = 96 ... 218, with F0 = 13 ... 831): hidden widths up to 1024, any input width."""
        fout = L.out_feats
        if train and self.dropout_p > 0:
            # 4 (GTE_LAYER_DROPOUT): every hidden layer of a training step with dropout, aggregate-first at any depth (the mask sits
            # between the aggregation and W).  Its GEMMs are the planes GEMMs whatever the GEMM mode: the only dropout path
            ok = (isinstance(L.lynorm, nn.LayerNorm) and L.linear.bias is not None and (L.activation is None or _is_relu(L.activation))
                  and self.general_planes and fout <= 1024)
            return LAYER_DROPOUT if ok else None
        if not (self._planes_on() and isinstance(L.lynorm, nn.LayerNorm) and L.linear.bias is not None
                and (L.activation is None or _is_relu(L.activation))):
            return None
        # (an input layer on images -- kind 0 or 2 -- moves to the cached form when the batch brings the second image)
        up = LAYER_CACHED if (i == 0 and cached and self._cached_layer0(L, fin)) else LAYER_PLANES
        if self._planes_layer(i, L, fin, n):
            return up                                            # the tuned range: 128 <= fout <= 256, fout % 16 == 0
        if (i == 0 and not self._transform_first(L, fin) and fout % 16 == 0
                and bool(self.lib.gte_sage_linear_fwd_fuses_ln(2 * fin, fout)) and not ops.use_tiled(n, fin, None)):
            return LAYER_SMALLK
        if not self.general_planes or fout > 1024:
            return None
        # transform-first while the layer does not widen by more than a quarter (the aggregation then moves fout columns: 1000
        # against 831 costs less than a per-batch fp32 copy of the input rows, and layer 0 reads the RESIDENT image through the row
        # map); aggregate-first for a widening input layer (13 / 63 / 313 / 363 -> 1000: aggregate fin columns)
        return up if (i > 0 or 4 * fout <= 5 * fin) else (LAYER_CACHED if up == LAYER_CACHED else LAYER_AGGFIRST)

    def _plan_kinds(self, f0: int, n: int, cached: bool = False, train: bool = True):
        """Layer kinds of the one-call step (gte_gcnsage_step) or None when the configuration needs the call-by-call path.
        ``cached``: the batch carries ``agg_p3`` (the resident image of the input's mean aggregate behind its row map).
        ``train`` False: the evaluation forward (no dropout layers)."""
        layers = list(self.model.layers)
        drop = train and self.dropout_p > 0
        if (not self.use_c_step or not (drop or self._planes_on()) or len(layers) < 2 or len(layers) > 8 or ops._timers is not None):
            return None
        dims = [f0] + [l.out_feats for l in layers]
        last = len(layers) - 1
        Lo = layers[last]
        if (isinstance(Lo.lynorm, nn.LayerNorm) or Lo.activation is not None or Lo.linear.bias is None or Lo.use_pp
                or not 1 <= Lo.out_feats <= 16 or not self.fused_head):
            return None
        if not self.general_planes and not (self._narrow(Lo, dims[last]) and self._fused_head(last, Lo, dims[last])):
            return None
        kinds = []
        for i, L in enumerate(layers[:-1]):
            k = self._layer_kind(i, L, dims[i], n, cached, train)
            if k is None:
                return None
            # (the p = 0 planes layers address their output through 32-bit buffer offsets: [n][2 ld] fp32 must stay below 2 GB.  A
            # dropout layer has no byte bound -- past this size gte_gcnsage_step runs its launches in their wide form, wide_layers()
            # -- only a row bound, DROPOUT_MAX_ROWS, which forward_backward reports)
            if k not in (LAYER_SMALLK, LAYER_DROPOUT) and (n + 256) * 2 * _c16(L.out_feats) * 4 >= (1 << 31):
                return None
            kinds.append(k)
        if drop and n > DROPOUT_MAX_ROWS:
            return None
        return kinds

    def wide_layers(self, g) -> int:
        """Bit mask of the hidden layers a training step on ``g`` runs in the wide addressing form (gte_gcnsage_step_wide_layers on
        the step's own plan: a dropout layer whose row buffers reach 2 GB, or every dropout layer under gte_dropout_set_wide(1) on
        this thread); 0 for a model without dropout or a step that is not on a plan."""
        return self._plan.wide_layers(g)

    def attach_feature_image(self, g) -> bool:
        """Give a graph that is evaluated again and again (the validation graph of train(): the same graph every epoch,
        model_train.py:246,349-353 of the reference) the P3 image of its features, made ONCE: forward_logits then runs the one-call
        plan on the planes kernels instead of the module path.  False when layer 0 does not take an image."""
        if getattr(g, "feat_p3", None) is not None:
            return True
        x = g.ndata.get('feat')
        if x is None or not x.is_cuda or not self.wants_resident_images(x.shape[1]):
            return False
        x = ops._row_major(x.to(torch.float32))
        g.feat_p3 = ops.p3_from_f32(x)
        if self.wants_agg_image(x.shape[1]):
            # ... and the image of the input's mean aggregate (constant too): layer 0 then is ONE launch, [x | ahn] W^T with LayerNorm
            # + ReLU in its epilogue, instead of a GEMM and an aggregation + LayerNorm launch over [n, 2 hidden]
            csr = g.in_csr()
            g.agg_p3 = ops.spmm_csr_p3(csr.indptr, csr.indices, g.in_weights(g.edata.get("feat")), x, x.shape[0], mean=True)
        return True

    @staticmethod
    def _batch_cached(g) -> bool:
        xp, ap = getattr(g, "feat_p3", None), getattr(g, "agg_p3", None)
        return xp is not None and ap is not None and (xp.row_map is None) == (ap.row_map is None)

    def _plan_mode(self, kinds, f0: int):
        """(general, out_gemm) of a plan, a description only -- every plan is bound and buffered the same way: ``general`` = some
        hidden layer lies outside the tuned range (128 <= hidden <= 256, hidden % 16 == 0: no padded rows there) or the output layer
        runs on the planes GEMMs; ``out_gemm`` = the latter (hidden width beyond the narrow kernels: > 256 or not a multiple of 8)."""
        layers = list(self.model.layers)
        dims = [f0] + [l.out_feats for l in layers]
        last = len(layers) - 1
        out_gemm = not (self._narrow(layers[last], dims[last]) and
                        (self._fused_head(last, layers[last], dims[last]) or self._narrow_padded(layers[last], dims[last])))
        gen = out_gemm or any(k in (LAYER_AGGFIRST, LAYER_CACHED, LAYER_DROPOUT)
                              or (k == LAYER_PLANES and not self._planes_layer(i, layers[i], dims[i])) for i, k in enumerate(kinds))
        return gen, out_gemm

    FORWARD_IMAGE_MAX_ELEMS = 1 << 21     # forward_logits: largest fp32 feature matrix that is converted to an image per call

    def forward_logits(self, g) -> torch.Tensor:
        """``model(g)`` without autograd (model_predict.py:141-147, the validation forward of model_train.py:349-353): logits
        [n, n_classes] through ONE host call (gte_gcnsage_forward) on the step's own buffers -- a view that the next step or
        forward on this engine overwrites.  Configurations the one-call plan does not cover -- and large graphs that bring fp32
        features to a planes input layer (a validation graph: the plan would write their image first) -- run the module path."""
        xp, n, f0 = batch_shape(g)
        kinds = self._plan_kinds(f0, n, self._batch_cached(g), train=False) if n > 0 else None
        if kinds is not None and xp is None and kinds[0] == LAYER_PLANES and n * f0 > self.FORWARD_IMAGE_MAX_ELEMS:
            # fp32 features under a planes input layer: the one-call plan would first write their P3 image (65 us at 21.5 k x 831)
            # -- more than the call saves on a graph of this size; the module path multiplies the fp32 rows directly
            # (profiles/debug/val_forward_time.py: 0.241 against 0.275 ms at 21.5 k nodes, 1.24 against 1.43 ms at 124 k)
            kinds = None
        if kinds is None:
            if xp is not None:
                f32_rows(g)     # (the module path reads fp32 rows: a resident batch in image mode carries the image only)
            was = self.model.training
            self.model.eval()                 # (no dropout in the evaluation forward)
            try:
                with torch.no_grad():
                    return self.model(g)
            finally:
                self.model.train(was)
        return self._plan.forward(g, kinds)

    # -- the schedule ----------------------------------------------------------------------------------
    def forward_backward(self, g, labels: torch.Tensor, grad_scale: float = 1.0, upto_layer: int = 0) -> torch.Tensor:
        """Forward, loss and the backward of layers n_layers-1 .. upto_layer (gradients of those layers final on return:
        their folds are flushed).  upto_layer > 0 leaves the rest to :meth:`backward_rest` -- the data-parallel step
        all-reduces the upper layers' gradient slice while the (longest) backward of layer 0 runs."""
        with_adam = bool(self._fuse_adam_req)
        if upto_layer == 0:
            _xp, n, f0 = batch_shape(g)
            kinds = self._plan_kinds(f0, n, self._batch_cached(g))
            if kinds is not None:
                return self._plan.step(g, labels, grad_scale, kinds, with_adam)
        self._refuse_dropout()
        out3, self._adam_fused = self._calls.run(g, labels, grad_scale, len(self.model.layers) - 1, upto_layer, with_adam=with_adam)
        return out3

    def _refuse_dropout(self) -> None:
        if self.dropout_p > 0:
            raise RuntimeError(f"FusedGcnSageStep: dropout {self.dropout_p} runs on the one-call plan only (gte_gcnsage_step with "
                               "GTE_LAYER_DROPOUT layers); this step would take the call-by-call schedule, which applies no masks: "
                               f"a switch changed after construction (use_c_step, op timers) or a batch of more than {DROPOUT_MAX_ROWS} "
                               "nodes (2^30: 32-bit row indices; the plan has no byte bound). Use TrainStep for it.")

    def backward_rest(self, g, from_layer: int) -> None:
        """Backward of layers from_layer-1 .. 0 after ``forward_backward(..., upto_layer=from_layer)`` on the same batch (the same
        graph object, no other batch in between: RuntimeError otherwise)."""
        self._refuse_dropout()
        self._calls.run(g, None, 1.0, from_layer - 1, 0, forward=False)

    def step(self, g, labels: torch.Tensor, n_global: Optional[int] = None,
             loss_scale: Optional[float] = None) -> torch.Tensor:
        scale = self._dp_scale(labels.shape[0], n_global, loss_scale)
        if self.distributed and self.dropout_p > 0:
            # the masks read the device step counter (completed steps) in the forward: bring it up to date first -- what the
            # optimiser launch behind the all-reduce would do (idempotent there)
            self.t += 1
            self._sync_adam_state()
            self.t -= 1
        if self.distributed and self._dp_split:
            out3 = self.forward_backward(g, labels, scale, upto_layer=1)
            pending = [self._all_reduce_async(self.flat_grad[self._n0:])]    # layers 1.. : in flight under layer 0's backward
            self.backward_rest(g, 1)
            pending.append(self._all_reduce_async(self.flat_grad[:self._n0]))
            for w in pending:
                w.wait()
        elif self.distributed:
            out3 = self.forward_backward(g, labels, scale)
            import torch.distributed as dist
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=self.group)
        else:
            # one GPU: nothing sits between the gradient folds and Adam, so the optimiser state is brought up to date FIRST
            # and the step is applied by the fold launch itself (gte_fold_defer_flush_adam)
            self.t += 1
            try:
                self._sync_adam_state()
                out3 = self._forward_backward_adam(g, labels, scale)
            except BaseException:
                self.t -= 1
                raise
            return out3
        self.t += 1
        self._optimizer_step()
        return out3

    def _forward_backward_adam(self, g, labels, scale):
        """forward + backward + optimiser step with self.t already advanced and the device state synced: Adam inside the fold
        launch when the folds cover the whole gradient, its own launch otherwise."""
        self._fuse_adam_req, self._adam_fused = self.fuse_adam, False
        try:
            out3 = self.forward_backward(g, labels, scale)
        finally:
            self._fuse_adam_req = False
        if self._adam_fused:
            self._step_dev_host += 1
            self._adam_fused = False
            self.adam_fused_steps += 1
        else:
            self._adam_dev_launch()
        return out3

    def _all_reduce_async(self, t):
        import torch.distributed as dist
        return dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    # -- optimiser: hyper-parameters and step count live on the device, so the launch is graph-capturable ----------
    def _adam_host_state(self, t_next: int, device_bc: bool = False):
        """{lr, b1, b2, eps, wd, grad_scale, bc1, sqrt(bc2)} for step t_next, bias corrections in double (gte_adam_step).
        ``device_bc``: the bias corrections as the optimiser launch advances them on the device after a step (csrc/gte_common.h:
        from the fp32 betas) -- what a restored step count t_next > 1 must reproduce for a resumed run to equal an uninterrupted one."""
        b1, b2 = float(self.betas[0]), float(self.betas[1])
        c1, c2 = (float(np.float32(b1)), float(np.float32(b2))) if device_bc else (b1, b2)
        return (float(self.lr), b1, b2, float(self.eps), float(self.weight_decay), 1.0,
                float(np.float32(1.0 - c1 ** t_next)), float(np.float32(np.sqrt(1.0 - c2 ** t_next))))

    def _adam_state(self) -> None:
        if self._hyper is None:
            dev = self.flat_param.device
            self._hyper_host = self._adam_host_state(1)
            self._hyper = torch.tensor(self._hyper_host, dtype=torch.float32, device=dev)
            self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            self._ticket = torch.zeros(int(self.lib.gte_adam_ticket_bytes()) // 4, dtype=torch.int32, device=dev)
            self._step_dev_host = 0                   # what the device counter holds (completed optimiser steps)

    def _sync_adam_state(self) -> None:
        """Eager-only: push changed hyper-parameters (lr_scale) / a changed step count (checkpoint restore) to the device.
        The device advances the counter and the bias corrections itself; the host only mirrors the expected values."""
        self._adam_state()
        stale_t = self._step_dev_host != self.t - 1
        want = self._adam_host_state(self.t, device_bc=stale_t and self.t > 1)
        if stale_t or want[:6] != self._hyper_host[:6]:
            if stale_t:
                self._step_dev.fill_(self.t - 1)
                self._step_dev_host = self.t - 1
                self._hyper.copy_(torch.tensor(want, dtype=torch.float32))
            else:
                self._hyper[:6].copy_(torch.tensor(want[:6], dtype=torch.float32))
            self._hyper_host = want

    def _adam_dev_launch(self) -> None:
        P = _lib.ptr
        last = self._plan.images.take_for_optimiser()            # (this launch changes the parameters: stale from here)
        if (last is not None and self.wimg_in_fold and 0 < last[1] <= 12 and not torch.cuda.is_current_stream_capturing()):
            # the optimiser launch behind the all-reduce also writes the weight images of the step that just ran (one launch instead
            # of Adam + a conversion launch in front of the next forward: the one-GPU step has both inside its fold launch)
            wrote = ctypes.c_int(0)
            _lib.check(self.lib.gte_adam_step_dev_images(P(self.flat_param), P(self.flat_grad), P(self.exp_avg), P(self.exp_avg_sq),
                                                         self.flat_param.numel(), P(self._hyper), P(self._step_dev), P(self._ticket),
                                                         last[0], last[1], ctypes.byref(wrote), _lib.current_stream()),
                       "gte_adam_step_dev_images")
            if wrote.value:
                self._plan.images.wrote(last[2], False)
            self._step_dev_host += 1
            return
        _lib.check(self.lib.gte_adam_step_dev(P(self.flat_param), P(self.flat_grad), P(self.exp_avg), P(self.exp_avg_sq),
                                              self.flat_param.numel(), P(self._hyper), P(self._step_dev), P(self._ticket),
                                              _lib.current_stream()), "gte_adam_step_dev")
        self._step_dev_host += 1

    def _optimizer_step(self) -> None:              # called with self.t already advanced
        self._sync_adam_state()
        self._adam_dev_launch()

    # -- HIP graph capture of a step on a RESIDENT batch ------------------------------------------------
    def capture(self, g, labels: torch.Tensor, n_global: Optional[int] = None, loss_scale: Optional[float] = None):
        """Returns ``replay() -> out3``: forward+backward of this batch as one HIP-graph launch, followed
        by Adam -- inside the same graph on one GPU (gte_adam_step_dev reads lr and the step count from device
        memory), eagerly after the all-reduce when distributed.  The batch's tensors must stay alive and unchanged
        in place (resident pages): the cache entry holds a reference to the graph object, so its id cannot be
        reused while the captured graph exists; :meth:`release` drops a captured batch and its ~300 MB of buffers."""
        scale = self._dp_scale(labels.shape[0], n_global, loss_scale)
        key = id(g)
        self._private_key = key                       # this batch's buffers are private to its graph (never reallocated)
        try:
            replay = self._capture(g, labels, scale, key)
            self._graph_owner[key] = (g, labels)
            return replay
        finally:
            self._private_key = None

    def release(self, g=None) -> None:
        """Forget the HIP graph(s) and private buffers captured for ``g`` (all captured batches when None)."""
        keys = list(self._graphs) if g is None else [id(g)]
        for k in keys:
            self._graphs.pop(k, None)
            for kk in [q for q in self._graph_bufs if q[0] == k]:          # (captured batch, buffer-set key)
                self._graph_bufs.pop(kk, None)
            self._graph_owner.pop(k, None)

    def _capture(self, g, labels, scale, key):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                 # warm-up on the side stream: buffers, CSR caches, props
            for _ in range(2):
                self.forward_backward(g, labels, scale)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._adam_state()
        # GTE_DP_GRAPH_COLLECTIVE=1 (experimental, off): the RCCL all-reduce is captured INSIDE the step's HIP graph, so a
        # data-parallel step is one graph launch like the single-GPU step.  Verified with one rank only (1-GPU boxes).
        graph_coll = self.distributed and _switch("GTE_DP_GRAPH_COLLECTIVE", "0")
        in_graph_adam = (not self.distributed) or graph_coll   # otherwise the all-reduce sits between backward and Adam, eagerly
        split = self.distributed and self._dp_split and not graph_coll
        graph = torch.cuda.CUDAGraph()
        graph_b = torch.cuda.CUDAGraph() if split else None
        with torch.cuda.graph(graph):
            if in_graph_adam and not graph_coll:
                out3 = self._forward_backward_adam(g, labels, scale)
            else:
                out3 = self.forward_backward(g, labels, scale, upto_layer=1 if split else 0)
            if graph_coll:
                import torch.distributed as dist
                dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=self.group)
            if in_graph_adam and not graph_coll:
                pass                                  # (applied below, fused into the fold launch when possible)
            elif in_graph_adam:
                self._adam_dev_launch()               # reads lr / step count from device memory at replay time
        if split:                                     # layer 0's backward: replayed while the upper slice is all-reduced
            with torch.cuda.graph(graph_b, pool=graph.pool()):
                self.backward_rest(g, 1)
        if in_graph_adam:
            self._step_dev_host -= 1                  # capturing did not run it

        def replay():
            self._plan.images.stale()                 # the graph updates the parameters; its own forward converts the images
            if in_graph_adam:
                self.t += 1
                self._sync_adam_state()               # no-op unless lr / t were changed from outside
                graph.replay()
                self._step_dev_host += 1
                return out3
            graph.replay()
            if split:
                pending = [self._all_reduce_async(self.flat_grad[self._n0:])]
                graph_b.replay()
                pending.append(self._all_reduce_async(self.flat_grad[:self._n0]))
                for w in pending:
                    w.wait()
            else:
                import torch.distributed as dist
                dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=self.group)
            self.t += 1
            self._optimizer_step()
            return out3
        self._graphs[key] = (graph, graph_b)
        return replay
