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
                                      (``region_scores=True``: with the regions' confidences as scores; ``box_eval=True``: the
                                      result also holds that evaluation, ``evaluate_regions``)
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


def predict_resident(engine, pipe, batch_pages: int, page_ids=None, return_logits=False):
    """Predictions (arg-max class per node, int64, pages concatenated in ``page_ids`` order -- default: all resident pages) with
    ``batch_pages`` pages per forward.  The reference's loop (model_predict.py:141-151) is one forward per page from the host;
    here a forward is ONE host call (``engine.forward_logits`` -> gte_gcnsage_forward) on a batch that the pipeline
    (``loop.BatchPipeline``) assembled on its side stream while the forward before it ran, and nothing synchronises until the
    caller reads the result.

    ``return_logits=True``: returns ``(pred, logits)``, the logits of all nodes as ONE device tensor float32 [nodes, n_classes]
    in the same order (every batch's view is copied out before the next forward overwrites the engine's buffer)."""
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
    if not steps:
        return (pred, torch.empty((0, 0), dtype=torch.float32, device=pipe.device)) if return_logits else pred
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
        if return_logits:
            if all_logits is None:
                all_logits = torch.empty((total, logits.shape[1]), dtype=torch.float32, device=pipe.device)
            all_logits[off:off + n].copy_(logits[:n])
        pipe.release(s)
        off += n
    return (pred, all_logits) if return_logits else pred


def extract_regions(data, all_pred, class_group=None, min_words=1, batch_pages=64, device=None, logits=None):
    """Regions of every page from the node predictions: connected components of the page graph among words of one predicted
    kind, each with the union of its words' boxes (``graph.page_regions`` -> gte_page_regions; the reference's
    ``get_subgraph_bbox`` is a stub; its own route, layout blocks labelled by word vote, is ``extract_blocks``).

    ``all_pred``: per-page class ids in ``data.graphs`` order (``test()``'s ``'all_pred'``);
    ``class_group[c]`` = region kind of class c, < 0 for none (default ``graph.DEFAULT_CLASS_GROUP``: the reference's category
    values, the three table classes merged into TABLE = 4); boxes from ``data.pages[i]['bboxs']``.  ``batch_pages`` pages go
    through one launch.  Returns, per page, a list of ``(group, [x0, y0, x1, y1], n_words)`` in ascending order of the region's
    first word; regions of fewer than ``min_words`` words are dropped after the compaction.

    ``logits`` (float [all nodes, n_classes], the pages concatenated in ``data.graphs`` order; a tensor on any device or an array):
    the tuples become ``(group, box, n_words, score)``, score = the region's confidence from the same launch
    (gte_page_regions_scored: the mean over the region's words of the softmax mass on the classes of its kind)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    sizes = [g.num_nodes() for g in data.graphs]
    if len(all_pred) != len(sizes):
        raise ValueError(f"extract_regions: {len(all_pred)} prediction lists for {len(sizes)} pages")
    node_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if logits is not None:
        logits = torch.as_tensor(logits)
        if logits.dim() != 2 or logits.shape[0] != int(node_off[-1]):
            raise ValueError(f"extract_regions: logits of shape {tuple(logits.shape)} for {int(node_off[-1])} nodes")
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
        if logits is None:
            reg = G.page_regions(bg, group, torch.from_numpy(boxes).to(device))
        else:
            reg = G.page_regions(bg, group, torch.from_numpy(boxes).to(device),
                                 logits=logits[int(node_off[ids.start]):int(node_off[ids.stop])].to(device), class_group=table)
        keep = reg.n_words >= int(min_words)
        rows = [reg.page[keep].tolist(), reg.group[keep].tolist(), reg.box[keep].tolist(), reg.n_words[keep].tolist()]
        if logits is not None:
            rows.append(reg.score[keep].tolist())
        for p, *rest in zip(*rows):
            out[b0 + p].append(tuple(rest))
    return out


def regions_json(data, regions):
    """``{kind_name: {page_name: {'bboxes': [...], 'scores': [...]}}}``: the layout the reference's box-level evaluation reads
    (postprocessing.py:326-345 write_json -> utils/metrics.py), kind names = the lower-case category names; the score of a
    region is its confidence where its tuple carries one (``extract_regions(..., logits=...)``) and 1.0, as in the reference's
    own writer, otherwise."""
    doc = {name: {} for name in G.GROUP_NAMES.values()}
    for i, page in enumerate(regions):
        name = str(data.pages[i]['page'])
        for kind, box, *rest in page:
            entry = doc.setdefault(G.GROUP_NAMES.get(kind, str(kind)), {}).setdefault(name, {'bboxes': [], 'scores': []})
            entry['bboxes'].append([int(v) for v in box])
            entry['scores'].append(float(rest[1]) if len(rest) > 1 else 1.0)
    return doc


def regions_gt_json(data, regions):
    """``{kind_name: {page_name: [box, ...]}}``: regions as the GROUND-TRUTH document of the box-level evaluation
    (``evaluate_regions``; the layout of the reference's ground-truth JSON, utils/metrics.py ``gt_boxes``)."""
    doc = {name: {} for name in G.GROUP_NAMES.values()}
    for i, page in enumerate(regions):
        name = str(data.pages[i]['page'])
        for kind, box, *_ in page:
            doc.setdefault(G.GROUP_NAMES.get(kind, str(kind)), {}).setdefault(name, []).append([int(v) for v in box])
    return doc


def evaluate_regions(pred_doc, gt_doc, iou_thrs=None, count_unpaired=False, device=None):
    """Box-level evaluation of predicted regions: the reference's AP at IoU thresholds (``get_avg_precision_at_iou`` of
    src/utils/metrics.py:162-244 per kind and threshold, their mean as in evaluate.py:116-129), with the box matching of all
    pages, kinds and thresholds in ONE launch (``graph.box_match`` -> gte_box_match) and the curve from its integer counts.

    ``pred_doc[kind][page] = {'bboxes': [[x0, y0, x1, y1], ...], 'scores': [...]}`` (``regions_json``), ``gt_doc[kind][page] =
    [[x0, y0, x1, y1], ...]`` (``regions_gt_json``); ``iou_thrs``: 1 .. 16 ascending thresholds (default
    ``np.linspace(0.5, 0.95, 10)``).  What the reference computes is NOT the textbook sweep, and this restates it exactly:

    * only PAIRED pages count: a page enters a kind's sums when it is a key of both ``pred_doc[kind]`` and ``gt_doc[kind]``.  The
      boxes of a page that only one of the two knows are ignored (metrics.py:202-206) -- unless ``count_unpaired=True``, which
      is NOT the reference: it counts the ground truths of such a page as false negatives and its predictions (those that the
      page's state below keeps) as false positives;
    * the score thresholds are the distinct scores of all the kind's predictions, ascending (unpaired pages included);
    * a page's state LAGS: at threshold t it keeps its predictions with score >= c, c = the largest of the page's OWN scores
      <= t (all of them below its first own score) -- a page is re-pruned only when the sweep reaches one of its own scores, so
      a lower-scored box survives until the page's next own score;
    * per page: IoU with the +1 pixel convention, candidates ``iou > thr`` strictly, greedy matching in descending IoU (among
      equal IoUs the larger ``pred_index * n_gt + gt_index`` first; predictions in stable ascending score order); tp = matches,
      fp = kept predictions - tp, fn = ground truths - tp;
    * precision = sum tp / (sum tp + sum fp), recall with fn, 0.0 on a zero denominator; AP = the mean over the recall levels
      ``linspace(0, 1, 11)`` of the largest precision at ``recall >= level`` (0.0 where there is none).

    Returns ``{kind: {'ap': [per IoU threshold], 'map': mean, 'precisions': [[...] per IoU threshold], 'recalls': [[...]],
    'thresholds': [score thresholds]}, ..., 'map': mean of the kinds' 'map'}`` over the kinds of ``gt_doc`` and ``pred_doc``."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    iou_thrs = np.linspace(0.5, 0.95, 10) if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    kinds = list(gt_doc) + [k for k in pred_doc if k not in gt_doc]
    # ---- the cells: one per (kind, page) that counts, predictions in stable ascending score order --------------------------
    cells, pbox, gbox, po, go = [], [], [], [0], [0]
    for kind in kinds:
        preds, gts = pred_doc.get(kind, {}), gt_doc.get(kind, {})
        pages = [pg for pg in gts if pg in preds or count_unpaired] + [pg for pg in preds if pg not in gts and count_unpaired]
        for pg in pages:
            sc = np.asarray(preds[pg]['scores'], dtype=np.float64).reshape(-1) if pg in preds else np.zeros(0)
            bx = np.asarray(preds[pg]['bboxes'], dtype=np.int64).reshape(-1, 4) if pg in preds else np.zeros((0, 4), dtype=np.int64)
            gb = np.asarray(gts.get(pg, []), dtype=np.int64).reshape(-1, 4)
            if sc.shape[0] != bx.shape[0]:
                raise ValueError(f"evaluate_regions: {kind} / {pg}: {bx.shape[0]} boxes, {sc.shape[0]} scores")
            for what, a in (("predicted", bx), ("ground-truth", gb)):
                if a.size and ((a[:, 0] > a[:, 2]).any() or (a[:, 1] > a[:, 3]).any() or np.abs(a).max() >= 1 << 24):
                    raise ValueError(f"evaluate_regions: {kind} / {pg}: a {what} box is malformed (metrics.py:35-40) or outside +-2^24")
            order = np.argsort(sc, kind='stable')
            cells.append((kind, sc[order]))
            pbox.append(bx[order])
            gbox.append(gb)
            po.append(po[-1] + bx.shape[0])
            go.append(go[-1] + gb.shape[0])
    tp = np.zeros((iou_thrs.size, 0), dtype=np.int64)
    if cells:
        tp = G.box_match(torch.from_numpy(np.concatenate(pbox).astype(np.int32)).to(device), po,
                         torch.from_numpy(np.concatenate(gbox).astype(np.int32)).to(device), go, iou_thrs).cpu().numpy().astype(np.int64)
    # ---- the sweep: a page's counts change only at its own scores -> per-event deltas, one cumulative sum -------------------
    out = {}
    for kind in kinds:
        thr = np.unique(np.asarray([s for e in pred_doc.get(kind, {}).values() for s in e['scores']], dtype=np.float64))
        d_tp, d_fp, d_fn = (np.zeros((iou_thrs.size, thr.size), dtype=np.int64) for _ in range(3))
        for b, (ck, sc) in enumerate(cells):
            if ck != kind or thr.size == 0:
                continue
            r, g = sc.shape[0], go[b + 1] - go[b]
            own = np.unique(sc)                                              # the page's own scores, ascending
            k = np.concatenate([[0], np.searchsorted(sc, own[1:], side='left')]).astype(np.int64) if r else np.zeros(1, dtype=np.int64)
            at = np.concatenate([[0], np.searchsorted(thr, own[1:])]).astype(np.int64) if r else np.zeros(1, dtype=np.int64)
            t = tp[:, po[b] + k] if r else np.zeros((iou_thrs.size, 1), dtype=np.int64)      # [n_iou, events]
            for acc, val in ((d_tp, t), (d_fp, (r - k)[None, :] - t), (d_fn, g - t)):
                val = np.diff(val, axis=1, prepend=0)                        # the first event carries the whole state k = 0
                acc[:, at] += val                                             # (own scores are distinct: so are the columns)
        s_tp, s_fp, s_fn = (np.cumsum(d, axis=1) for d in (d_tp, d_fp, d_fn))
        with np.errstate(divide='ignore', invalid='ignore'):
            prec = np.where(s_tp + s_fp > 0, s_tp / (s_tp + s_fp), 0.0)
            rec = np.where(s_tp + s_fn > 0, s_tp / (s_tp + s_fn), 0.0)
        ap = []
        for j in range(iou_thrs.size):
            levels = [prec[j][rec[j] >= lv] for lv in np.linspace(0.0, 1.0, 11)]
            ap.append(float(np.mean([a.max() if a.size else 0.0 for a in levels])))
        out[kind] = {'ap': ap, 'map': float(np.mean(ap)), 'precisions': prec.tolist(), 'recalls': rec.tolist(),
                     'thresholds': thr.tolist()}
    out['map'] = float(np.mean([out[k]['map'] for k in kinds])) if kinds else 0.0
    return out


# ---- the reference's own route from word predictions to page objects: layout blocks labelled by word vote, tables assembled ----
# category values of src/utils/const.py Categories_names that the assembly names
_TABLE, _FIGURE, _COLH, _SP, _TCELL = 4, 5, 7, 8, 10


def _y_mid(b):
    return (b[3] + b[1]) / 2


def _x_mid(b):
    return (b[2] + b[0]) / 2


def _x_meets(interval, b):
    return interval[0] <= b[2] and interval[1] >= b[0]


def _hull(group):
    return [min([b[0] for b in group]), min([b[1] for b in group]), max([b[2] for b in group]), max([b[3] for b in group])]


def _overlaps_strictly(a, b):
    """``intersect`` of the reference's graphs/utils.py:27-34: normalised corners, both axes strictly."""
    left, top = max(min(a[0], a[2]), min(b[0], b[2])), max(min(a[1], a[3]), min(b[1], b[3]))
    right, bottom = min(max(a[0], a[2]), max(b[0], b[2])), min(max(a[1], a[3]), max(b[1], b[3]))
    return bool(left < right and top < bottom)


def assemble_tables(blocks, labels):
    """Tables from labelled layout blocks: ``get_tables_bbox`` of the reference (postprocessing_2.py:21-195) restated -- its
    behaviour exactly, including what looks accidental there, and the same operations on Python floats, so the result is bit
    for bit the reference's (tests/golden/blocks_cases.json decides).  Plain Python on lists: a page has tens of blocks and
    every rule depends on order.

    ``blocks``: ``[x0, y0, x1, y1]`` per block, ``labels``: their category values.  Neither list is changed.  Returns ``(blocks,
    labels, headers)``: the page's blocks after the assembly (untouched blocks are the caller's own objects), their categories,
    and the merged column-header / spanning-cell boxes.

    1. Per class -- column header, spanning cell, table cell, in this order -- the class's blocks form COLUMN GROUPS: a block joins
       the first group whose x-interval it meets (closed), else opens a group.  A group's interval is the x-range of its FIRST
       block and never widens (group 0 takes the class's first block's).  Inside a group the blocks stand by y-centre, a newcomer
       before the first centre ``>=`` its own.
    2. A group is split where other blocks stand between two of its members: over ALL blocks now in the list (the merged ones
       appended for an earlier class included) that meet the group's interval, count those whose y-centre lies strictly between
       two consecutive member centres; the SECOND such block splits the group behind the lower of the two members.  The count never
       resets: a group is split at most once.
    3. Every part becomes one block, the hull of its members, appended with the class's label; header and spanning hulls are also
       the ``headers``.  Only the table-cell groups hand their intervals on.  Then the classes' original blocks leave the list.
    4. Per handed-on interval: the blocks whose x-centre lies strictly inside, in stable order of y-centre.  Walking the
       consecutive pairs, a header directly followed by a cell block -- or by a spanning block and then a cell block -- gives a
       TABLE, the hull of the header and the cell block.  The walk does not skip what it merged.  The merged blocks are deleted
       by descending index, duplicates kept as in the reference (a block named twice would take its successor along; the
       handed-on intervals are pairwise disjoint -- a group opens only where no interval is met -- so none is).
    5. The remaining cell blocks become TABLE.  Every block that is no table and strictly overlaps a table (as the tables stand
       before this step) is absorbed: the table is replaced by the hull of itself and what it overlaps.

    A class whose first block has inverted x-corners leaves group 0 empty and raises ``ValueError`` (the hull of nothing), as the
    reference does."""
    blocks, labels = list(blocks), list(labels)
    members = {cls: [i for i, l in enumerate(labels) if l == cls] for cls in (_COLH, _SP, _TCELL)}
    handed_on, headers = [], []
    for cls, ids in members.items():
        if not ids:
            continue
        first = blocks[ids[0]]
        groups = [{'x': [first[0], first[2]], 'blocks': [], 'mids': []}]
        for i in ids:
            b = blocks[i]
            for g in groups:
                if _x_meets(g['x'], b):
                    mid = _y_mid(b)
                    at = next((k for k, m in enumerate(g['mids']) if not m < mid), len(g['mids']))
                    g['blocks'].insert(at, b)
                    g['mids'].insert(at, mid)
                    break
            else:
                groups.append({'x': [b[0], b[2]], 'blocks': [b], 'mids': [_y_mid(b)]})
        cuts = []
        for g in groups:
            cut, between, mids = None, 0, g['mids']
            for b in blocks:
                if not _x_meets(g['x'], b):
                    continue
                mid = _y_mid(b)
                for k in range(len(mids) - 1):
                    if mid < mids[k]:
                        break
                    if mids[k] < mid < mids[k + 1]:
                        between += 1
                        if between == 2:
                            cut = k + 1
                        break
            cuts.append(cut)
        for g, cut in zip(groups, cuts):
            parts = [g['blocks']] if cut is None else [part for part in (g['blocks'][:cut], g['blocks'][cut:]) if part]
            for part in parts:
                box = _hull(part)
                blocks.append(box)
                labels.append(cls)
                if cls != _TCELL:
                    headers.append(box)
        if cls == _TCELL:
            handed_on.extend(g['x'] for g in groups)
    for i in sorted((i for ids in members.values() for i in ids), reverse=True):
        del blocks[i], labels[i]

    mids = [_y_mid(b) for b in blocks]
    by_y = sorted(range(len(blocks)), key=lambda k: mids[k])
    merged = []
    for x in handed_on:
        col = [k for k in by_y if x[0] < _x_mid(blocks[k]) < x[1]]
        for at in range(len(col) - 1):
            if labels[col[at]] != _COLH:
                continue
            head, nxt = col[at], col[at + 1]
            if labels[nxt] == _TCELL:
                took = [head, nxt]
            elif at + 2 == len(col):
                break
            elif labels[nxt] == _SP and labels[col[at + 2]] == _TCELL:
                took = [head, nxt, col[at + 2]]
            else:
                continue
            a, b = blocks[head], blocks[took[-1]]
            blocks.append([min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])])
            labels.append(_TABLE)
            merged.extend(took)
    for i in sorted(merged, reverse=True):
        del blocks[i], labels[i]

    labels = [_TABLE if l == _TCELL else l for l in labels]
    tables = [i for i, l in enumerate(labels) if l == _TABLE]
    absorbed = [[b for k, b in enumerate(blocks) if labels[k] != _TABLE and _overlaps_strictly(blocks[t], b)] for t in tables]
    gone = {k for k, b in enumerate(blocks) if labels[k] != _TABLE and any(_overlaps_strictly(blocks[t], b) for t in tables)}
    for t, inside in zip(tables, absorbed):
        if inside:
            blocks.append(_hull(inside + [blocks[t]]))
            labels.append(_TABLE)
            gone.add(t)
    for i in sorted(gone, reverse=True):
        del blocks[i], labels[i]
    return blocks, labels, headers


def extract_blocks(data, all_pred, class_category=None, blocks=None, images=None, scale=0.36, rescale=True, batch_pages=64,
                   device=None):
    """Page objects by the reference's own route (``get_objects_bboxs``, postprocessing_2.py:197-309): the layout blocks that a
    PDF text extractor delivers for every page are labelled by the vote of the words inside them (``graph.block_vote`` ->
    gte_block_vote: ONE launch per ``batch_pages`` pages, in place of the reference's words x blocks loop in Python), the
    column-header, spanning-cell and table-cell blocks are assembled into tables (``assemble_tables``, on the host, per page, on
    the unscaled blocks), and the page's images become FIGURE blocks.

    ``all_pred``: per-page class ids in ``data.graphs`` order (``test()``'s ``'all_pred'``); ``class_category[c]`` = the
    reference's original category value of class c (default ``graph.DEFAULT_CLASS_CATEGORY``, its ``LableModification.revert``);
    word boxes from ``data.pages[i]['bboxs']``.  ``blocks``: per page a sequence of ``[x0, y0, x1, y1]`` in PDF points, the text
    blocks in the extractor's order (default ``data.pages[i]['blocks']``; a page without that key raises ``ValueError``);
    ``images``: per page a sequence of image boxes, ``[x0, y0, x1, y1]`` or a dict with a ``'bbox'`` (default
    ``data.pages[i].get('images', ())``): those higher than 10 are kept, every coordinate truncated with ``int()``
    (postprocessing_2.py:264-270).  A block is compared with the word boxes after division by ``scale`` (the reference's
    SCALE_FACTOR); ``rescale=True`` divides every output coordinate by ``scale`` (postprocessing_2.py:306), ``rescale=False``
    gives the output of the reference's postprocessing.py.

    Returns per page a dict: ``'blocks'`` / ``'labels'`` after table assembly and figures; ``'voted_labels'`` per input block;
    ``'headers'`` (never rescaled, as in the reference); ``'word_block'`` the page-local block index of every word or -1;
    ``'votes'`` the input blocks' counters [blocks, categories].

    Out of scope: obtaining the blocks from a PDF (the caller's extractor); block confidences (the reference writes 1.0;
    ``'votes'`` is there for callers who want a share); feeding the float-valued block document to ``evaluate_regions``, which
    takes integer boxes."""
    n_pages = len(data.graphs)
    if len(all_pred) != n_pages:
        raise ValueError(f"extract_blocks: {len(all_pred)} prediction lists for {n_pages} pages")
    for what, seq in (("block", blocks), ("image", images)):
        if seq is not None and len(seq) != n_pages:
            raise ValueError(f"extract_blocks: {len(seq)} {what} lists for {n_pages} pages")
    if not float(scale) > 0.0:
        raise ValueError(f"extract_blocks: scale = {scale}")
    scale = float(scale)
    table = np.asarray(G.DEFAULT_CLASS_CATEGORY if class_category is None else class_category, dtype=np.int64).reshape(-1)
    n_cat = max(len(G.CATEGORY_NAMES), int(table.max()) + 1 if table.size else 0)
    page_blocks = []
    for i in range(n_pages):
        if blocks is not None:
            pb = blocks[i]
        elif 'blocks' in data.pages[i]:
            pb = data.pages[i]['blocks']
        else:
            raise ValueError(f"extract_blocks: page {i} ({data.pages[i].get('page')}) carries no 'blocks'")
        pb = np.asarray(pb, dtype=np.float64)
        if pb.size == 0:
            pb = pb.reshape(0, 4)
        if pb.ndim != 2 or pb.shape[1] != 4:
            raise ValueError(f"extract_blocks: the blocks of page {i} ({data.pages[i].get('page')}) have shape {pb.shape}")
        page_blocks.append(pb)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    out = []
    bp = max(1, int(batch_pages))
    for b0 in range(0, n_pages, bp):
        ids = range(b0, min(b0 + bp, n_pages))
        pred = [np.asarray(all_pred[i], dtype=np.int64).reshape(-1) for i in ids]
        boxes = [np.asarray(data.pages[i]['bboxs'], dtype=np.int32).reshape(-1, 4) for i in ids]
        for i, p, b in zip(ids, pred, boxes):
            if p.shape[0] != b.shape[0]:
                raise ValueError(f"extract_blocks: page {i} has {p.shape[0]} predictions and {b.shape[0]} boxes")
            if p.size and (p.min() < 0 or p.max() >= table.size):
                raise ValueError(f"extract_blocks: page {i} holds a class outside the {table.size} of class_category")
        node_off = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).astype(np.int64)
        block_off = np.concatenate([[0], np.cumsum([page_blocks[i].shape[0] for i in ids])]).astype(np.int64)
        cat = table[np.concatenate(pred)].astype(np.int32)
        scaled = np.concatenate([page_blocks[i] for i in ids]) / scale                     # float64: bit for bit b / sf
        vote = G.block_vote(torch.from_numpy(np.concatenate(boxes)).to(device), node_off, torch.from_numpy(cat).to(device),
                            torch.from_numpy(scaled).to(device), block_off, n_cat=n_cat, double_cat=2)
        word_block, votes, label = vote.word_block.cpu().numpy(), vote.votes.cpu().numpy(), vote.label.cpu().numpy()
        for k, i in enumerate(ids):
            n0, n1, k0, k1 = int(node_off[k]), int(node_off[k + 1]), int(block_off[k]), int(block_off[k + 1])
            voted = [int(v) for v in label[k0:k1]]
            new_blocks, new_labels, headers = assemble_tables(page_blocks[i].tolist(), voted)
            for img in (images[i] if images is not None else data.pages[i].get('images', ())):
                box = img['bbox'] if isinstance(img, dict) else img
                if box[3] - box[1] > 10:
                    new_blocks.append([int(v) for v in box])
                    new_labels.append(_FIGURE)
            if rescale:
                new_blocks = [[v / scale for v in b] for b in new_blocks]
            wb = word_block[n0:n1].astype(np.int64)
            out.append({'blocks': new_blocks, 'labels': new_labels, 'voted_labels': voted, 'headers': headers,
                        'word_block': np.where(wb >= 0, wb - k0, -1).tolist(), 'votes': votes[k0:k1].tolist()})
    return out


def blocks_json(data, result):
    """``{kind_name: {page_name: {'bboxes': [...], 'scores': [1.0, ...]}}}`` of ``extract_blocks``' result: the layout of the
    reference's ``write_json`` (postprocessing_2.py:328-348, its ``ours_bboxs.json``) -- all thirteen lower-case category names
    as keys, a page only under the kinds it has, coordinates as floats, every score 1.0."""
    doc = {name: {} for name in G.CATEGORY_NAMES}
    for i, page in enumerate(result):
        name = str(data.pages[i]['page'])
        for box, label in zip(page['blocks'], page['labels']):
            entry = doc[G.CATEGORY_NAMES[label]].setdefault(name, {'bboxes': [], 'scores': []})
            entry['bboxes'].append([float(v) for v in box])
            entry['scores'].append(1.0)
    return doc


def test(data, config, weights_path=None, save_predictions=True, regions=False, region_scores=False, box_eval=False, blocks=False):
    """``blocks=True``: the result gains ``'blocks'`` = ``extract_blocks(data, all_pred)`` (the pages carry their layout blocks
    as ``data.pages[i]['blocks']``), and with ``save_predictions`` ``{output}/blocks/{logs}.json`` is written (``blocks_json``).

    ``regions=True``: the result gains ``'regions'`` (``extract_regions`` of the predictions: per page a list of
    ``(group, [x0, y0, x1, y1], n_words)``), and with ``save_predictions`` ``{output}/regions/{logs}.json`` is written
    (``regions_json``) with every score 1.0.

    ``region_scores=True`` (implies ``regions``): the tuples are ``(group, box, n_words, score)``, score = the region's
    confidence from the model's own logits (gte_page_regions_scored), and the JSON carries these scores.

    ``box_eval=True`` (implies ``region_scores``): the result gains ``'box_eval'`` = ``evaluate_regions`` of the scored regions
    against the ground-truth regions that the same component rule forms from the pages' labels (``extract_regions(data,
    labels)``: the only box-level ground truth that pre-built pages carry) -- the reference's AP at IoU 0.50 .. 0.95 and mAP."""
    region_scores = bool(region_scores or box_eval)
    regions = bool(regions or region_scores)
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
    flat_logits = None                                     # region_scores: the logits of all nodes, pages in data.graphs order
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
        if region_scores:
            flat_pred, flat_logits = predict_resident(engine, pipe, bs, return_logits=True)
            flat_pred = flat_pred.cpu().numpy()
        else:
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
        kept = []
        with torch.no_grad():
            for b0 in range(0, len(data.graphs), bs):
                pages = [g.to(device) for g in data.graphs[b0:b0 + bs]]
                bg = G.batch(pages)
                logits = model(bg)
                if region_scores:
                    kept.append(logits.float().clone())
                pred = logits.argmax(dim=1).cpu().numpy()
                off = np.cumsum([0] + [g.num_nodes() for g in pages])
                for i, g in enumerate(pages):
                    pp, tt = pred[off[i]:off[i + 1]], g.ndata['label'].long().cpu().numpy()
                    all_pred.append(pp)
                    all_true.append(tt)
                    mean_test_acc += float((pp == tt).sum()) / max(g.num_nodes(), 1)      # per-page accuracy (:150)
        if kept:
            flat_logits = torch.cat(kept)
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
        if region_scores and flat_logits is None:
            flat_logits = torch.empty((0, n_classes), dtype=torch.float32, device=device)
        result['regions'] = extract_regions(data, all_pred, batch_pages=bs, device=device, logits=flat_logits if region_scores else None)
        doc = regions_json(data, result['regions']) if (save_predictions or box_eval) else None
        if save_predictions:
            import json
            reg_dir = os.path.join(out_root, 'regions')
            os.makedirs(reg_dir, exist_ok=True)
            with open(os.path.join(reg_dir, f'{logs}.json'), 'w') as f:
                json.dump(doc, f)
        if box_eval:
            labels = [g.ndata['label'].long().cpu().numpy() for g in data.graphs]
            gt = regions_gt_json(data, extract_regions(data, labels, batch_pages=bs, device=device))
            result['box_eval'] = evaluate_regions(doc, gt, device=device)
    if blocks:
        result['blocks'] = extract_blocks(data, all_pred, batch_pages=bs, device=device)
        if save_predictions:
            import json
            blk_dir = os.path.join(out_root, 'blocks')
            os.makedirs(blk_dir, exist_ok=True)
            with open(os.path.join(blk_dir, f'{logs}.json'), 'w') as f:
                json.dump(blocks_json(data, result['blocks']), f)
    return result
