"""Inference entry point on the HIP path: ``test(data, config)``.

Restates ``src/models/model_predict.py:35-174``: rebuild ``GcnSAGE`` from the config, load the best
weights ``WEIGHTS/{logs}.pt`` written by ``EarlyStopping`` (``src/utils/training.py:49``), run the forward
on every page, collect the predictions and per-class precision / recall / F1.  The reference runs ONE forward per
page (launch-latency bound at ~10^2-10^3 nodes); here pages are batched ``config.TRAINING.batch_size`` at a
time (block-diagonal batching does not change a page's logits -- tested bitwise) and split per page after
the arg-max.

Post-processing (``components/graphs/postprocessing.py``) and evaluation (``utils/metrics.py``) live in their own modules, as in
the reference; ``test()`` only calls them.  Output contract (what post-processing consumes):
  ``{output}/all_pred/{logs}``        pickle of ONE FLAT python list of ints, the pages' node predictions concatenated in
                                      ``data.graphs`` order -- exactly ``pickle.dump(all_pred, open(OUTPUT / 'all_pred' / logs,
                                      'wb'))`` of model_predict.py:151,172-174; ``postprocessing.py:199-216`` slices it
                                      back into pages by ``graph.num_nodes()``
  ``{output}/predictions/{logs}.pkl`` extra, not in the reference: ``{'all_pred': [per-page lists], 'num_nodes': [...]}``
  ``{output}/regions/{logs}.json``    ``test(..., regions=True)`` only: the regions of every page (``postprocessing.extract_regions``) in the layout
                                      the reference's box-level evaluation reads (``regions_json``)
                                      (``region_scores=True``: with the regions' confidences as scores; ``box_eval=True``: the
                                      result also holds that evaluation, ``metrics.evaluate_regions``)
  ``{output}/tables/{logs}.json``     ``tables=True`` only: ``{page: [table, ...]}``, the grid of every predicted table
                                      (``postprocessing.extract_tables`` / ``tables_json``)
``predict(data, config)`` is the label-free sibling (the reference's ``GenericPapers2Graphs`` route, loader.py:431-573): the same
forward on pages without ground truth, a confidence per word, the same artefacts (``predictions/{logs}.pkl`` gains
``'confidence'``), no metric.
The printed accuracy is the reference's "Mean Test Accuracy": the MEAN OVER PAGES of the per-page accuracy (:150,163),
not the node-weighted accuracy (returned as ``accuracy_nodes``).
"""
from __future__ import annotations

import json
import os
import pickle

import numpy as np
import torch
import torch.nn.functional as F

from .. import graph as G
from .. import ops
from ..components.features.utils import calculate_hidden, get_in_feats_
from ..components.graphs.models import GcnSAGE
from ..components.graphs import postprocessing as PP
from ..utils.config import logs_from_config
from ..utils import metrics


def hidden_width(config, in_feats, n_classes):
    mode = config.TRAINING.mode_params
    if mode == 'fixed':
        return config.MODES.fixed.h_layer_dim
    if mode == 'scaled':
        return calculate_hidden(in_feats, n_classes, config.MODES.scaled.params_no, config.TRAINING.n_layers)
    return in_feats / 2


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


def predict_resident(engine, pipe, batch_pages: int, page_ids=None, return_logits=False, head=False, return_prob=False):
    """Predictions (arg-max class per node, int64, pages concatenated in ``page_ids`` order -- default: all resident pages) with
    ``batch_pages`` pages per forward.  The reference's loop (model_predict.py:141-151) is one forward per page from the host;
    here a forward is ONE host call (``engine.forward_logits`` -> gte_gcnsage_forward) on a batch that the pipeline
    (``loop.BatchPipeline``) assembled on its side stream while the forward before it ran, and nothing synchronises until the
    caller reads the result.

    ``return_logits=True``: returns ``(pred, logits)``, the logits of all nodes as ONE device tensor float32 [nodes, n_classes]
    in the same order (every batch's view is copied out before the next forward overwrites the engine's buffer).

    ``head=True``: every batch's arg-max launch is ONE ``ops.predict_head`` launch (gte_predict_head) that also writes the
    confidence of every node -- the softmax probability of its predicted class, float32 -- and, with ``return_prob=True``, the
    whole softmax row, straight into the batch's slices of the flat results.  Returns ``(pred, conf)`` or ``(pred, conf, prob)``,
    with ``return_logits=True`` the logits appended last.  ``head=False`` (default): as above, ``return_prob`` is not accepted."""
    if return_prob and not head:
        raise ValueError("predict_resident: return_prob needs head=True")
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
    all_logits = None
    conf = torch.empty(total, dtype=torch.float32, device=pipe.device) if head else None
    prob = None

    def result():
        empty = torch.empty((0, 0), dtype=torch.float32, device=pipe.device)          # (no step: the class count is unknown)
        out = (pred,) + ((conf,) if head else ()) + ((empty if prob is None else prob,) if return_prob else ())
        out += ((empty if all_logits is None else all_logits,) if return_logits else ())
        return out if len(out) > 1 else pred

    if not steps:
        return result()
    engine.reserve(pipe.max_batch_nodes(), f0, cached=bool(res.p3_mode == "rows" and res.agg_p3 is not None))
    pipe.start(0)
    off = 0
    for s in range(len(steps)):
        if s + 1 < len(steps):
            pipe.start(s + 1)
        g = pipe.get(s)
        logits = engine.forward_logits(g)
        n = pipe.nodes(s)
        if head:
            if return_prob and prob is None:
                prob = torch.empty((total, logits.shape[1]), dtype=torch.float32, device=pipe.device)
            ops.predict_head(logits, n, out_pred=pred[off:off + n], out_conf=conf[off:off + n],
                             out_prob=prob[off:off + n] if return_prob else None)
        else:
            torch.argmax(logits, dim=1, out=pred[off:off + n])
        if return_logits:
            if all_logits is None:
                all_logits = torch.empty((total, logits.shape[1]), dtype=torch.float32, device=pipe.device)
            all_logits[off:off + n].copy_(logits[:n])
        pipe.release(s)
        off += n
    return result()


def test(data, config, weights_path=None, save_predictions=True, regions=False, region_scores=False, box_eval=False, blocks=False,
         block_scores=False, block_eval=False, doc_eval=False, tables=False, table_eval=False):
    """``tables=True``: the result gains ``'tables'`` = ``extract_tables(data, all_pred)`` -- per page the grid of every predicted
    table: rows, columns, cells and their texts (gte_table_grid; the default column gap is not validated on real pages, see
    ``postprocessing.table_batch``) -- and with ``save_predictions`` ``{output}/tables/{logs}.json`` is written (``tables_json``).

    ``table_eval=True`` (implies ``tables``): the result gains ``'table_eval'`` = ``evaluate_regions(table_structure_json(...),
    gt, float_boxes=True)``, gt = the ``'table'``, ``'table-row'`` and ``'table-col'`` kinds of ``blocks_gt_json(data)`` (the pages
    carry ``'annotations'``; PubTables-1M's TABLE, TABLE_ROW and TABLE_COL): AP at IoU 0.50 .. 0.95 of the predicted table, row
    and column boxes.

    ``doc_eval=True``: the result gains ``'doc_eval'`` = ``metrics.evaluate_doc`` of the pages' labels, ``all_pred`` and the
    word boxes ``data.pages[i]['bboxs']``: area-weighted precision / recall / F1 per class (the reference's ``evaluate_doc``,
    models/evaluate.py:142-209), both as the reference computes them (``'reference'``) and by the DocBank formula (``'docbank'``);
    one line per class is printed.  A page without ``'bboxs'`` raises ``ValueError``.

    ``blocks=True``: the result gains ``'blocks'`` = ``extract_blocks(data, all_pred)`` (the pages carry their layout blocks
    as ``data.pages[i]['blocks']``), and with ``save_predictions`` ``{output}/blocks/{logs}.json`` is written (``blocks_json``).

    ``block_scores=True`` (implies ``blocks``): ``extract_blocks(..., logits=...)`` -- every page of ``'blocks'`` gains
    ``'scores'`` and ``'n_words'`` per final block (gte_block_scores, from the model's own logits), and the JSON carries these
    scores in place of 1.0.

    ``block_eval`` (implies ``block_scores``): ``True`` -- the ground truth is ``blocks_gt_json(data)``, the pages carry
    ``'annotations'`` -- or a ground-truth document ``{kind: {page: [box, ...]}}``.  The result gains ``'block_eval'`` =
    ``evaluate_regions(blocks_json(...), gt, float_boxes=True)``: the reference's AP at IoU 0.50 .. 0.95 of the document it
    evaluates itself (models/evaluate.py:64-131).

    ``regions=True``: the result gains ``'regions'`` (``extract_regions`` of the predictions: per page a list of
    ``(group, [x0, y0, x1, y1], n_words)``), and with ``save_predictions`` ``{output}/regions/{logs}.json`` is written
    (``regions_json``) with every score 1.0.

    ``region_scores=True`` (implies ``regions``): the tuples are ``(group, box, n_words, score)``, score = the region's
    confidence from the model's own logits (gte_page_regions_scored), and the JSON carries these scores.

    ``box_eval=True`` (implies ``region_scores``): the result gains ``'box_eval'`` = ``evaluate_regions`` of the scored regions
    against the ground-truth regions that the same component rule forms from the pages' labels (``extract_regions(data,
    labels)``: the only box-level ground truth that pre-built pages carry) -- the reference's AP at IoU 0.50 .. 0.95 and mAP."""
    if not getattr(data, 'labeled', True):
        raise ValueError("test(): the pages carry no labels (labeled == False, from_boxes(unlabeled=True)); use predict()")
    region_scores = bool(region_scores or box_eval)
    regions = bool(regions or region_scores)
    want_block_eval = block_eval is not False and block_eval is not None
    block_scores = bool(block_scores or want_block_eval)
    blocks = bool(blocks or block_scores)
    want_logits = region_scores or block_scores
    run = _forward_pages(data, config, weights_path, want_logits)
    device, n_classes, logs, out_root, bs = run['device'], run['n_classes'], run['logs'], run['out_root'], run['bs']
    flat_pred, flat_logits = run['pred'], run['logits']
    all_pred, all_true = [], []
    mean_test_acc, off = 0.0, 0
    for g in data.graphs:
        n = g.num_nodes()
        pp, tt = flat_pred[off:off + n], g.ndata['label'].long().cpu().numpy()
        all_pred.append(pp)
        all_true.append(tt)
        mean_test_acc += float((pp == tt).sum()) / max(n, 1)                              # per-page accuracy (:150)
        off += n
    y_pred, y_true = np.concatenate(all_pred), np.concatenate(all_true)
    p, r, f1, conf = metrics.per_class_prf(y_true, y_pred, n_classes)
    acc_nodes = float((y_pred == y_true).mean()) if len(y_true) else 0.0
    acc = mean_test_acc / max(len(data.graphs), 1)
    print("Mean Test Accuracy {:.4f}".format(acc))                                        # :163
    print(" -> node accuracy {:.4f} | macro-F1 {:.4f}".format(acc_nodes, float(f1.mean())))
    flat = [int(v) for a in all_pred for v in a.tolist()]
    write_json = _json_writer(out_root, logs)
    if save_predictions:
        _save_predictions(out_root, logs, flat, all_pred)
    result = {'accuracy': acc, 'accuracy_nodes': acc_nodes, 'precision': p, 'recall': r, 'f1': f1, 'confusion': conf,
              'all_pred': all_pred, 'all_pred_flat': flat}
    if regions:
        result['regions'] = PP.extract_regions(data, all_pred, batch_pages=bs, device=device, logits=flat_logits if region_scores else None)
        doc = PP.regions_json(data, result['regions']) if (save_predictions or box_eval) else None
        if save_predictions:
            write_json('regions', doc)
        if box_eval:
            labels = [g.ndata['label'].long().cpu().numpy() for g in data.graphs]
            gt = PP.regions_gt_json(data, PP.extract_regions(data, labels, batch_pages=bs, device=device))
            result['box_eval'] = metrics.evaluate_regions(doc, gt, device=device)
    if blocks:
        result['blocks'] = PP.extract_blocks(data, all_pred, batch_pages=bs, device=device, logits=flat_logits if block_scores else None)
        doc = PP.blocks_json(data, result['blocks']) if (save_predictions or want_block_eval) else None
        if save_predictions:
            write_json('blocks', doc)
        if want_block_eval:
            gt = PP.blocks_gt_json(data) if block_eval is True else block_eval
            result['block_eval'] = metrics.evaluate_regions(doc, gt, device=device, float_boxes=True)
    if tables or table_eval:
        _add_tables(result, data, all_pred, bs, device, write_json if save_predictions else None)
        if table_eval:
            gt = {kind: pages for kind, pages in PP.blocks_gt_json(data).items() if kind in ('table', 'table-row', 'table-col')}
            result['table_eval'] = metrics.evaluate_regions(PP.table_structure_json(data, result['tables']), gt, device=device,
                                                            float_boxes=True)
    if doc_eval:
        for i, page in enumerate(data.pages):
            if 'bboxs' not in page:
                raise ValueError(f"test(doc_eval=True): page {i} carries no 'bboxs'")
        boxes = [np.asarray(page['bboxs']).reshape(-1, 4) for page in data.pages]
        ev = result['doc_eval'] = metrics.evaluate_doc(all_true, all_pred, boxes, device=device)
        for c in range(ev['n_classes']):                                                  # evaluate.py:207, without its class names
            ref, bank = ev['reference'], ev['docbank']
            print(f"class {c}: precision {ref['precision'][c]} - recall {ref['recall'][c]} - f1 {ref['f1'][c]}"
                  f" (DocBank: {bank['precision'][c]} - {bank['recall'][c]} - {bank['f1'][c]})")
    return result


def _add_tables(result, data, all_pred, bs, device, write_json):
    """``tables=True`` of ``test()`` and ``predict()``: ``result['tables']`` and, with a writer, ``tables/{logs}.json``."""
    result['tables'] = PP.extract_tables(data, all_pred, batch_pages=bs, device=device)
    if write_json is not None:
        write_json('tables', PP.tables_json(data, result['tables']))


def _json_writer(out_root, logs):
    def write_json(sub, doc):                                                             # {output}/{sub}/{logs}.json
        os.makedirs(os.path.join(out_root, sub), exist_ok=True)
        with open(os.path.join(out_root, sub, f'{logs}.json'), 'w') as f:
            json.dump(doc, f)
    return write_json


def _save_predictions(out_root, logs, flat, all_pred, extra=None):
    """The two prediction artefacts of the module docstring; ``extra``: further keys of ``predictions/{logs}.pkl``."""
    ap_dir = os.path.join(out_root, 'all_pred')                                           # OUTPUT / 'all_pred' (:172)
    os.makedirs(ap_dir, exist_ok=True)
    with open(os.path.join(ap_dir, logs), 'wb') as f:
        pickle.dump(flat, f)                                                              # the reference's artefact (:174)
    pred_dir = os.path.join(out_root, 'predictions')
    os.makedirs(pred_dir, exist_ok=True)
    with open(os.path.join(pred_dir, f'{logs}.pkl'), 'wb') as f:
        pickle.dump(dict({'all_pred': [a.tolist() for a in all_pred], 'num_nodes': [len(a) for a in all_pred]}, **(extra or {})), f)


def _forward_pages(data, config, weights_path, want_logits, head=False, want_prob=False):
    """What ``test()`` and ``predict()`` share: the model rebuilt from the config with the best weights, and one forward over
    every page -- the resident engine path, or the module loop for a model the engine refuses.  Reads no label.
    -> dict: ``device``, ``n_classes``, ``logs``, ``out_root``, ``bs``; ``pred`` (host int64 [nodes], pages in ``data.graphs``
    order); ``logits`` (device float32 [nodes, C], None unless ``want_logits``); with ``head`` (the arg-max through
    ``ops.predict_head``) also ``conf`` (host float32 [nodes]) and, with ``want_prob``, ``prob`` (host float32 [nodes, C])."""
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
    engine = None
    flat_logits = None                                     # region_scores: the logits of all nodes, pages in data.graphs order
    flat_conf = flat_prob = None
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
        out = predict_resident(engine, pipe, bs, return_logits=want_logits, head=head, return_prob=want_prob)
        out = list(out) if isinstance(out, tuple) else [out]
        flat_pred = out.pop(0).cpu().numpy()
        if head:
            flat_conf = out.pop(0).cpu().numpy()
        if want_prob:
            flat_prob = out.pop(0).cpu().numpy()
        if want_logits:
            flat_logits = out.pop(0)
    else:
        preds, kept, confs, probs = [], [], [], []
        with torch.no_grad():
            for b0 in range(0, len(data.graphs), bs):
                logits = model(G.batch([g.to(device) for g in data.graphs[b0:b0 + bs]]))
                if want_logits:
                    kept.append(logits.float().clone())
                if head:
                    hp = ops.predict_head(logits.float(), want_prob=want_prob)
                    preds.append(hp[0].cpu().numpy())
                    confs.append(hp[1].cpu().numpy())
                    if want_prob:
                        probs.append(hp[2].cpu().numpy())
                else:
                    preds.append(logits.argmax(dim=1).cpu().numpy())
        flat_pred = np.concatenate(preds)
        if kept:
            flat_logits = torch.cat(kept)
        if head:
            flat_conf = np.concatenate(confs)
            flat_prob = np.concatenate(probs) if want_prob else None
    if want_logits and flat_logits is None:
        flat_logits = torch.empty((0, n_classes), dtype=torch.float32, device=device)
    return dict(device=device, n_classes=n_classes, logs=logs, out_root=out_root, bs=bs, pred=flat_pred, logits=flat_logits,
                conf=flat_conf, prob=flat_prob)


def predict(data, config, weights_path=None, save_predictions=True, probabilities=False, regions=False, region_scores=False,
            blocks=False, block_scores=False, tables=False):
    """The label-free sibling of ``test()``: the classes of the words of pages WITHOUT ground truth
    (``PrebuiltPages.from_boxes(..., unlabeled=True)``; the reference's ``GenericPapers2Graphs`` route), and a confidence per
    word.  On a labelled set the labels are ignored.  The model, the weights, the resident engine path and its fallback are
    ``test()``'s; the arg-max is ``ops.predict_head`` (gte_predict_head: one launch per batch for class, confidence and softmax
    row).  Nothing is computed from labels and no accuracy is printed.

    Returns ``'all_pred'`` (int arrays per page), ``'all_pred_flat'`` (one flat list), ``'confidence'`` (float32 arrays per
    page: the softmax probability of the predicted class, NaN for a row of non-finite logits); ``probabilities=True``:
    ``'probabilities'`` (float32 [n_p, C] per page); ``regions`` / ``region_scores`` / ``blocks`` / ``block_scores``: ``'regions'``
    and ``'blocks'`` as in ``test()`` (the ``*_scores`` imply their route); ``tables``: ``'tables'`` as in ``test()``.
    ``save_predictions`` writes what ``test()`` writes (module docstring), ``predictions/{logs}.pkl`` with the further key
    ``'confidence'`` (per-page lists)."""
    region_scores, block_scores = bool(region_scores), bool(block_scores)
    regions = bool(regions or region_scores)
    blocks = bool(blocks or block_scores)
    run = _forward_pages(data, config, weights_path, region_scores or block_scores, head=True, want_prob=bool(probabilities))
    device, logs, out_root, bs = run['device'], run['logs'], run['out_root'], run['bs']
    all_pred, confidence, all_prob, off = [], [], [], 0
    for g in data.graphs:
        n = g.num_nodes()
        all_pred.append(run['pred'][off:off + n])
        confidence.append(run['conf'][off:off + n])
        if probabilities:
            all_prob.append(run['prob'][off:off + n])
        off += n
    flat = [int(v) for a in all_pred for v in a.tolist()]
    write_json = _json_writer(out_root, logs)
    if save_predictions:
        _save_predictions(out_root, logs, flat, all_pred, extra={'confidence': [c.tolist() for c in confidence]})
    result = {'all_pred': all_pred, 'all_pred_flat': flat, 'confidence': confidence}
    if probabilities:
        result['probabilities'] = all_prob
    if regions:
        result['regions'] = PP.extract_regions(data, all_pred, batch_pages=bs, device=device, logits=run['logits'] if region_scores else None)
        if save_predictions:
            write_json('regions', PP.regions_json(data, result['regions']))
    if blocks:
        result['blocks'] = PP.extract_blocks(data, all_pred, batch_pages=bs, device=device, logits=run['logits'] if block_scores else None)
        if save_predictions:
            write_json('blocks', PP.blocks_json(data, result['blocks']))
    if tables:
        _add_tables(result, data, all_pred, bs, device, write_json if save_predictions else None)
    return result
