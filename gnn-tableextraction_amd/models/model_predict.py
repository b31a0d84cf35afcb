"""Inference entry point on the HIP path: ``test(data, config)``.

Restates ``src/models/model_predict.py:35-174``: rebuild ``GcnSAGE`` from the config, load the best
weights ``WEIGHTS/{logs}.pt`` written by ``EarlyStopping`` (``src/utils/training.py:49``), run the forward
on every page, collect the predictions and per-class precision / recall / F1.  The reference runs ONE forward per
page (launch-latency bound at ~10^2-10^3 nodes); here pages are batched ``config.TRAINING.batch_size`` at a
time (block-diagonal batching does not change a page's logits -- tested bitwise) and split per page after
the arg-max.

Output contract (what post-processing consumes):
  ``{output}/all_pred/{logs}``        pickle of ONE FLAT python list of ints, the pages' node predictions concatenated in
                                      ``data.graphs`` order -- exactly ``pickle.dump(all_pred, open(OUTPUT / 'all_pred' / logs,
                                      'wb'))`` of model_predict.py:151,172-174; ``postprocessing.py:199-216`` slices it
                                      back into pages by ``graph.num_nodes()``
  ``{output}/predictions/{logs}.pkl`` extra, not in the reference: ``{'all_pred': [per-page lists], 'num_nodes': [...]}``
  ``{output}/regions/{logs}.json``    ``test(..., regions=True)`` only: the regions of every page (``extract_regions``) in the layout
                                      the reference's box-level evaluation reads (``regions_json``)
The printed accuracy is the reference's "Mean Test Accuracy": the MEAN OVER PAGES of the per-page accuracy (:150,163),
not the node-weighted accuracy (returned as ``accuracy_nodes``).
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch
import torch.nn.functional as F

from .. import graph as G
from ..components.features.utils import calculate_hidden, get_in_feats_
from ..components.graphs.models import GcnSAGE
from ..utils.config import logs_from_config


def hidden_width(config, in_feats, n_classes):
    mode = config.TRAINING.mode_params
    if mode == 'fixed':
        return config.MODES.fixed.h_layer_dim
    if mode == 'scaled':
        return calculate_hidden(in_feats, n_classes, config.MODES.scaled.params_no, config.TRAINING.n_layers)
    return in_feats / 2


def per_class_prf(y_true: np.ndarray, y_pred: np.ndarray, n_classes: int):
    conf = np.zeros((n_classes, n_classes), dtype=np.float64)
    np.add.at(conf, (y_true, y_pred), 1.0)
    tp = np.diag(conf)
    pred_n, true_n = conf.sum(0), conf.sum(1)
    p = np.where(pred_n > 0, tp / np.maximum(pred_n, 1), 0.0)
    r = np.where(true_n > 0, tp / np.maximum(true_n, 1), 0.0)
    f1 = np.where(p + r > 0, 2 * p * r / np.maximum(p + r, 1e-30), 0.0)
    return p, r, f1, conf


# ---- one forward per page without the per-page launch bill ------------------------------------------------------------
# The reference runs ONE forward per page (model_predict.py:130-154): ~15 launches of a few microseconds of work each --
# launch latency, not arithmetic.  PageForwardGraphs keeps, per size bucket, the page's tensors in fixed
# buffers and the model's forward captured in a HIP graph: a page is one assembly launch (gte_batch_assemble straight from the
# resident dataset into the bucket's buffers), one tiny fill and one graph launch.  Rows past the page's nodes have no edges
# and are ignored.
class PageForwardGraphs:
    BUCKETS = (64, 128, 256, 512, 1024, 2048, 4096)
    EDGES_PER_NODE = 16                                   # k = 5 bidirected: <= 10 in-edges on average

    def __init__(self, model, resident: "G.ResidentPages"):
        if resident.p3_mode:
            raise ValueError("PageForwardGraphs reads fp32 features (ResidentPages not in image mode)")
        self.model, self.res, self.device = model, resident, resident.device
        self._b = {}

    def _bucket(self, n: int, e: int):
        for cap in self.BUCKETS:
            if n <= cap and e <= cap * self.EDGES_PER_NODE:
                return cap
        return None

    def _build(self, cap: int):
        res, dev = self.res, self.device
        bufs = res.alloc_batch_buffers(cap, cap * self.EDGES_PER_NODE, cap * self.EDGES_PER_NODE)
        bufs["indptr"][0].zero_()
        bufs["feat"].zero_()
        g = G.ResidentBatch(cap, cap * self.EDGES_PER_NODE, G.CSR(bufs["indptr"][0], bufs["indices"][0], None),
                            G.CSR(bufs["indptr"][1], bufs["indices"][1], None), bufs["weight"][0], bufs["weight"][1], dev)
        g.ndata["feat"] = bufs["feat"]
        if res.weighted:
            g.edata["feat"] = bufs["weight"][0]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                self.model(g)                             # warm-up outside the capture: workspaces, lazy state
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            logits = self.model(g)
            pred = logits.argmax(dim=1)
        meta = torch.empty(7, dtype=torch.int32, device=dev)
        self._b[cap] = dict(bufs=bufs, graph=graph, logits=logits, pred=pred, meta=meta, g=g)
        return self._b[cap]

    def forward(self, page_id: int):
        """(logits [n, C], predictions [n]) of one page: views of the bucket's buffers, valid until its next use."""
        res = self.res
        n = int(res.node_off_host[page_id + 1] - res.node_off_host[page_id])
        eo = res._sets["in"]["edge_off_host"]
        e = int(eo[page_id + 1] - eo[page_id])
        cap = self._bucket(n, e)
        if cap is None:                                   # larger than the largest bucket: the eager path
            g = res.batch([page_id])
            with torch.no_grad():
                logits = self.model(g)
            return logits, logits.argmax(dim=1)
        b = self._b.get(cap) or self._build(cap)
        e_out = int(res._sets["out"]["edge_off_host"][page_id + 1] - res._sets["out"]["edge_off_host"][page_id])
        meta_h = torch.tensor([page_id, 0, n, 0, e, 0, e_out], dtype=torch.int32)
        b["meta"].copy_(meta_h, non_blocking=True)
        res.assemble(b["meta"], 1, n, e, e_out, b["bufs"])
        b["bufs"]["indptr"][0][n + 1:].fill_(e)           # rows past the page: empty
        b["graph"].replay()
        return b["logits"][:n], b["pred"][:n]


def predict_resident(engine, pipe, batch_pages: int, page_ids=None) -> torch.Tensor:
    """Predictions (arg-max class per node, int64, pages concatenated in ``page_ids`` order -- default: all resident pages) with
    ``batch_pages`` pages per forward.  The reference's loop (model_predict.py:141-151) is one forward per page from the host;
    here a forward is ONE host call (``engine.forward_logits`` -> gte_gcnsage_forward) on a batch that the pipeline
    (``loop.BatchPipeline``) assembled on its side stream while the forward before it ran, and nothing synchronises until the
    caller reads the result."""
    res = pipe.res
    ids = np.arange(len(res.page_sizes()), dtype=np.int64) if page_ids is None else np.asarray(page_ids, dtype=np.int64)
    steps = [ids[i:i + batch_pages] for i in range(0, ids.size, batch_pages)]
    f0 = res.feat.shape[1]
    # (train=False: the evaluation forward applies no dropout -- a dropout model runs the p = 0 plan and wants ITS images)
    want_p3 = bool(engine.wants_resident_images(f0, train=False))
    if want_p3 != bool(res.p3_mode):                       # as loop.run_steps: layer 0 reads the resident feature image
        torch.cuda.synchronize(pipe.device)
        res.enable_p3(agg=bool(engine.wants_agg_image(f0, train=False))) if want_p3 else res.disable_p3()
        pipe._sets, pipe._free_ev = [], [None] * pipe.depth
    pipe.load(steps)
    total = sum(pipe.nodes(s) for s in range(len(steps)))
    pred = torch.empty(total, dtype=torch.int64, device=pipe.device)
    if not steps:
        return pred
    engine.reserve(pipe.max_batch_nodes(), f0, cached=bool(res.p3_mode == "rows" and res.agg_p3 is not None))
    pipe.start(0)
    off = 0
    for s in range(len(steps)):
        if s + 1 < len(steps):
            pipe.start(s + 1)
        g = pipe.get(s)
        logits = engine.forward_logits(g)
        n = pipe.nodes(s)
        torch.argmax(logits, dim=1, out=pred[off:off + n])
        pipe.release(s)
        off += n
    return pred


def extract_regions(data, all_pred, class_group=None, min_words=1, batch_pages=64, device=None):
    """Regions of every page from the node predictions: connected components of the page graph among words of one predicted
    kind, each with the union of its words' boxes (``graph.page_regions`` -> gte_page_regions; the reference's
    ``get_subgraph_bbox`` is a stub, its PyMuPDF block voting is out of scope -- DESIGN 10).

    ``all_pred``: per-page class ids in ``data.graphs`` order (``test()``'s ``'all_pred'``);
    ``class_group[c]`` = region kind of class c, < 0 for none (default ``graph.DEFAULT_CLASS_GROUP``: the reference's category
    values, the three table classes merged into TABLE = 4); boxes from ``data.pages[i]['bboxs']``.  ``batch_pages`` pages go
    through one launch.  Returns, per page, a list of ``(group, [x0, y0, x1, y1], n_words)`` in ascending order of the region's
    first word; regions of fewer than ``min_words`` words are dropped after the compaction."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    sizes = [g.num_nodes() for g in data.graphs]
    if len(all_pred) != len(sizes):
        raise ValueError(f"extract_regions: {len(all_pred)} prediction lists for {len(sizes)} pages")
    table = torch.as_tensor(G.DEFAULT_CLASS_GROUP if class_group is None else class_group, dtype=torch.int32, device=device)
    out = [[] for _ in sizes]
    bp = max(1, int(batch_pages))
    for b0 in range(0, len(sizes), bp):
        ids = range(b0, min(b0 + bp, len(sizes)))
        if sum(sizes[i] for i in ids) == 0:
            continue
        parts = []
        for i in ids:
            h = data.graphs[i].local_var()                # the structure alone: no feature rows travel for this
            h.ndata.clear()
            h.edata.clear()
            parts.append(h.to(device))
        bg = G.batch(parts)
        pred = np.concatenate([np.asarray(all_pred[i], dtype=np.int64).reshape(-1) for i in ids])
        boxes = np.concatenate([np.asarray(data.pages[i]['bboxs'], dtype=np.int32).reshape(-1, 4) for i in ids])
        if pred.shape[0] != bg.num_nodes() or boxes.shape[0] != bg.num_nodes():
            raise ValueError(f"extract_regions: pages {ids.start}..{ids.stop - 1} have {bg.num_nodes()} nodes, {pred.shape[0]} "
                             f"predictions and {boxes.shape[0]} boxes")
        group = table[torch.from_numpy(pred).to(device)]                                  # class -> kind: a gather
        reg = G.page_regions(bg, group, torch.from_numpy(boxes).to(device))
        keep = reg.n_words >= int(min_words)
        for p, k, bx, nw in zip(reg.page[keep].tolist(), reg.group[keep].tolist(), reg.box[keep].tolist(), reg.n_words[keep].tolist()):
            out[b0 + p].append((k, bx, nw))
    return out


def regions_json(data, regions):
    """``{kind_name: {page_name: {'bboxes': [...], 'scores': [...]}}}``: the layout the reference's box-level evaluation reads
    (postprocessing.py:326-345 write_json -> utils/metrics.py), kind names = the lower-case category names; every score is
    1.0, as in the reference's own writer."""
    doc = {name: {} for name in G.GROUP_NAMES.values()}
    for i, page in enumerate(regions):
        name = str(data.pages[i]['page'])
        for kind, box, _ in page:
            entry = doc.setdefault(G.GROUP_NAMES.get(kind, str(kind)), {}).setdefault(name, {'bboxes': [], 'scores': []})
            entry['bboxes'].append([int(v) for v in box])
            entry['scores'].append(1.0)
    return doc


def test(data, config, weights_path=None, save_predictions=True, regions=False):
    """``regions=True``: the result gains ``'regions'`` (``extract_regions`` of the predictions: per page a list of
    ``(group, [x0, y0, x1, y1], n_words)``), and with ``save_predictions`` ``{output}/regions/{logs}.json`` is written
    (``regions_json``).  No region confidence exists yet: every score in that file is 1.0."""
    if not (config.TRAINING.gpu >= 0 and torch.cuda.is_available()):
        raise RuntimeError("model_predict runs on the MI355X HIP path only (no CPU fallback)")
    device = torch.device('cuda', config.TRAINING.gpu)
    n_classes = data.num_classes
    in_feats = get_in_feats_(config)
    logs = logs_from_config(config)
    out_root = config.GENERAL.get('output_dir', 'output')
    weights_path = weights_path or os.path.join(out_root, 'weights', f'{logs}.pt')

    model = GcnSAGE(in_feats, int(hidden_width(config, in_feats, n_classes)), n_classes, config.TRAINING.n_layers,
                    F.relu, config.TRAINING.dropout)
    model.load_state_dict(torch.load(weights_path, map_location='cpu'))
    model = model.to(device).eval()

    bs = max(1, int(config.TRAINING.batch_size))
    all_pred, all_true = [], []
    mean_test_acc = 0.0
    engine = None
    if len(data.graphs) > 0:
        # evaluation applies no dropout: a model trained with --dropout takes the same path (forward_logits binds the p = 0 plan);
        # only a model the engine refuses to build for (a dropout model outside the one-call plan) keeps the module loop below
        from .engine import FusedGcnSageStep
        try:
            engine = FusedGcnSageStep(model)
        except ValueError:
            if not config.TRAINING.dropout:
                raise
    if engine is not None:
        # the shipped configuration: pages resident in HBM, batches assembled on the device one forward ahead, one host call per
        # forward (predict_resident); one device -> host copy of all predictions at the end
        from .loop import BatchPipeline
        pipe = BatchPipeline(G.ResidentPages(data.graphs, device))
        flat_pred = predict_resident(engine, pipe, bs).cpu().numpy()
        off = 0
        for g in data.graphs:
            n = g.num_nodes()
            pp, tt = flat_pred[off:off + n], g.ndata['label'].long().cpu().numpy()
            all_pred.append(pp)
            all_true.append(tt)
            mean_test_acc += float((pp == tt).sum()) / max(n, 1)                          # per-page accuracy (:150)
            off += n
    else:
        with torch.no_grad():
            for b0 in range(0, len(data.graphs), bs):
                pages = [g.to(device) for g in data.graphs[b0:b0 + bs]]
                bg = G.batch(pages)
                pred = model(bg).argmax(dim=1).cpu().numpy()
                off = np.cumsum([0] + [g.num_nodes() for g in pages])
                for i, g in enumerate(pages):
                    pp, tt = pred[off[i]:off[i + 1]], g.ndata['label'].long().cpu().numpy()
                    all_pred.append(pp)
                    all_true.append(tt)
                    mean_test_acc += float((pp == tt).sum()) / max(g.num_nodes(), 1)      # per-page accuracy (:150)
    y_pred, y_true = np.concatenate(all_pred), np.concatenate(all_true)
    p, r, f1, conf = per_class_prf(y_true, y_pred, n_classes)
    acc_nodes = float((y_pred == y_true).mean()) if len(y_true) else 0.0
    acc = mean_test_acc / max(len(data.graphs), 1)
    print("Mean Test Accuracy {:.4f}".format(acc))                                        # :163
    print(" -> node accuracy {:.4f} | macro-F1 {:.4f}".format(acc_nodes, float(f1.mean())))
    flat = [int(v) for a in all_pred for v in a.tolist()]
    if save_predictions:
        ap_dir = os.path.join(out_root, 'all_pred')                                       # OUTPUT / 'all_pred' (:172)
        os.makedirs(ap_dir, exist_ok=True)
        with open(os.path.join(ap_dir, logs), 'wb') as f:
            pickle.dump(flat, f)                                                          # the reference's artefact (:174)
        pred_dir = os.path.join(out_root, 'predictions')
        os.makedirs(pred_dir, exist_ok=True)
        with open(os.path.join(pred_dir, f'{logs}.pkl'), 'wb') as f:
            pickle.dump({'all_pred': [a.tolist() for a in all_pred], 'num_nodes': [len(a) for a in all_pred]}, f)
    result = {'accuracy': acc, 'accuracy_nodes': acc_nodes, 'precision': p, 'recall': r, 'f1': f1, 'confusion': conf,
              'all_pred': all_pred, 'all_pred_flat': flat}
    if regions:
        result['regions'] = extract_regions(data, all_pred, batch_pages=bs, device=device)
        if save_predictions:
            import json
            reg_dir = os.path.join(out_root, 'regions')
            os.makedirs(reg_dir, exist_ok=True)
            with open(os.path.join(reg_dir, f'{logs}.json'), 'w') as f:
                json.dump(regions_json(data, result['regions']), f)
    return result
