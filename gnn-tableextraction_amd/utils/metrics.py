"""Evaluation (the reference's ``utils/metrics.py`` and ``models/evaluate.py``): per-class precision / recall / F1 of node
predictions, and the box-level AP of predicted regions.

``evaluate_regions`` is three public stages in a row -- ``region_cells`` (host) -> ``box_match`` (gte_box_match, ONE launch) ->
``average_precisions`` (host, numpy) -- so that the host stages run (and are tested) without a device, with a CPU oracle in place
of the launch.  ``float_boxes=True`` takes the documents' boxes as float64 through the same stages (gte_box_match_f64): the block
route's document, which is what the reference itself evaluates.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib


def per_class_prf(y_true: np.ndarray, y_pred: np.ndarray, n_classes: int):
    conf = np.zeros((n_classes, n_classes), dtype=np.float64)
    np.add.at(conf, (y_true, y_pred), 1.0)
    tp = np.diag(conf)
    pred_n, true_n = conf.sum(0), conf.sum(1)
    p = np.where(pred_n > 0, tp / np.maximum(pred_n, 1), 0.0)
    r = np.where(true_n > 0, tp / np.maximum(true_n, 1), 0.0)
    f1 = np.where(p + r > 0, 2 * p * r / np.maximum(p + r, 1e-30), 0.0)
    return p, r, f1, conf


class RegionCells(NamedTuple):
    """Result of :func:`region_cells`: one cell per (kind, page) that counts, in the order of ``kinds`` and of the pages."""
    kinds: list               # the kinds of gt_doc, then those only pred_doc knows
    thresholds: dict          # kind -> float64 [T]: the distinct scores of ALL the kind's predictions, ascending
    kind: list                # per cell: its kind
    scores: list              # per cell: float64 [r] the page's scores in stable ascending order
    pred_box: np.ndarray      # int32 [R, 4]  the cells' predictions concatenated, inside a cell in the order of ``scores``
    pred_off: list            # [cells + 1]                                                  (float64 with ``float_boxes``)
    gt_box: np.ndarray        # int32 [G, 4]  the cells' ground truths concatenated
    gt_off: list              # [cells + 1]


def region_cells(pred_doc, gt_doc, count_unpaired=False, float_boxes=False) -> RegionCells:
    """Stage one of :func:`evaluate_regions`: the documents (layouts there) as cells -- the paired pages of every kind (all pages
    with ``count_unpaired``), each page's predictions in stable ascending score order, the boxes concatenated with offsets: the
    arguments of :func:`box_match`.  ``ValueError`` on unequal box / score counts and on a malformed box; no device is touched.

    ``float_boxes=False`` casts every coordinate to an integer (a float document is truncated); ``True`` keeps float64 boxes and
    raises ``ValueError`` for a box with a non-finite value, inverted corners or a value outside +-2^24."""
    box_type = np.float64 if float_boxes else np.int64
    kinds = list(gt_doc) + [k for k in pred_doc if k not in gt_doc]
    kind_of, scores, pbox, gbox, po, go = [], [], [], [], [0], [0]
    for kind in kinds:
        preds, gts = pred_doc.get(kind, {}), gt_doc.get(kind, {})
        pages = [pg for pg in gts if pg in preds or count_unpaired] + [pg for pg in preds if pg not in gts and count_unpaired]
        for pg in pages:
            sc = np.asarray(preds[pg]['scores'], dtype=np.float64).reshape(-1) if pg in preds else np.zeros(0)
            bx = np.asarray(preds[pg]['bboxes'], dtype=box_type).reshape(-1, 4) if pg in preds else np.zeros((0, 4), dtype=box_type)
            gb = np.asarray(gts.get(pg, []), dtype=box_type).reshape(-1, 4)
            if sc.shape[0] != bx.shape[0]:
                raise ValueError(f"evaluate_regions: {kind} / {pg}: {bx.shape[0]} boxes, {sc.shape[0]} scores")
            for what, a in (("predicted", bx), ("ground-truth", gb)):
                if float_boxes:
                    if a.size and not (np.isfinite(a).all() and (a[:, 0] <= a[:, 2]).all() and (a[:, 1] <= a[:, 3]).all()
                                       and np.abs(a).max() <= 1 << 24):
                        raise ValueError(f"evaluate_regions: {kind} / {pg}: a {what} box is non-finite, malformed (metrics.py:35-40) "
                                         f"or outside +-2^24")
                elif a.size and ((a[:, 0] > a[:, 2]).any() or (a[:, 1] > a[:, 3]).any() or np.abs(a).max() >= 1 << 24):
                    raise ValueError(f"evaluate_regions: {kind} / {pg}: a {what} box is malformed (metrics.py:35-40) or outside +-2^24")
            order = np.argsort(sc, kind='stable')
            kind_of.append(kind)
            scores.append(sc[order])
            pbox.append(bx[order])
            gbox.append(gb)
            po.append(po[-1] + bx.shape[0])
            go.append(go[-1] + gb.shape[0])
    thresholds = {kind: np.unique(np.asarray([s for e in pred_doc.get(kind, {}).values() for s in e['scores']], dtype=np.float64))
                  for kind in kinds}
    out_type = np.float64 if float_boxes else np.int32
    cat = lambda parts: np.concatenate(parts).astype(out_type) if parts else np.zeros((0, 4), dtype=out_type)
    return RegionCells(kinds, thresholds, kind_of, scores, cat(pbox), po, cat(gbox), go)


def box_match(pred_box: torch.Tensor, pred_off, gt_box: torch.Tensor, gt_off, iou_thr, float_boxes=False, return_iou=False):
    """Match counts of the box-level evaluation (gte_box_match, one launch): ``tp`` int32 [n_thr, R] on the device.

    Cell b (one page and kind) holds the predictions ``pred_box[pred_off[b]:pred_off[b + 1]]`` (int [R, 4], inside a cell ASCENDING
    by score) and the ground truths ``gt_box[gt_off[b]:gt_off[b + 1]]``; the offsets are host sequences.
    ``tp[j, pred_off[b] + k]`` = greedy matches (descending IoU, ``iou > iou_thr[j]`` strictly, +1 pixel convention; include/gte.h)
    between the cell's ground truths and its predictions ``k ..``, i.e. after pruning its k lowest-scored boxes.  ``iou_thr``:
    1 .. 16 ascending thresholds.  Raises ``ValueError`` naming the first cell whose candidate pairs exceed
    ``gte_box_match_max_candidates()``; ``GteError`` when a cell has more than ``gte_box_match_max_boxes()`` boxes on a side.
    One synchronisation (the cells' status words are read before the result is handed out).

    ``float_boxes=True``: the boxes are taken as float64 (gte_box_match_f64: the reference's ``calc_iou_individual`` in IEEE
    double, operation by operation); a non-finite, inverted or ``|v| > 2^24`` box overlaps nothing.  With ``return_iou=True``
    (float boxes only) the result is ``(tp, iou)``, ``iou`` float64 the cells' R_b x G_b IoU matrices, row-major, concatenated."""
    _lib.require_device(pred_box, "box_match")
    _lib.require_device(gt_box, "box_match")
    lib, P = _lib.load(), _lib.ptr
    dev = pred_box.device
    if return_iou and not float_boxes:
        raise ValueError("box_match: return_iou needs float_boxes")
    box_type = torch.float64 if float_boxes else torch.int32
    pred_box = pred_box.to(box_type).reshape(-1, 4).contiguous()
    gt_box = gt_box.to(dev).to(box_type).reshape(-1, 4).contiguous()
    po, d_po = _lib.partition_offsets(pred_off, pred_box.shape[0], "box_match: the prediction offsets", dev)
    go, d_go = _lib.partition_offsets(gt_off, gt_box.shape[0], "box_match: the ground-truth offsets", dev)
    if po.size != go.size:
        raise ValueError(f"box_match: offsets of {po.size - 1} / {go.size - 1} cells do not partition the predicted and the ground-truth boxes")
    cells = po.size - 1
    thr = np.ascontiguousarray(np.asarray(iou_thr, dtype=np.float64).reshape(-1))
    tp = torch.empty((thr.size, pred_box.shape[0]), dtype=torch.int32, device=dev)
    status = torch.empty(cells, dtype=torch.int32, device=dev)
    iou = None
    if float_boxes:
        d_io = None
        if return_iou:
            io = np.concatenate([[0], np.cumsum(np.diff(po).astype(np.int64) * np.diff(go).astype(np.int64))]).astype(np.int64)
            d_io = torch.from_numpy(io).to(dev)
            iou = torch.empty(int(io[-1]), dtype=torch.float64, device=dev)
        _lib.check(lib.gte_box_match_f64(P(pred_box), P(d_po), P(gt_box), P(d_go), cells, int(np.diff(po).max()) if cells else 0,
                                         int(np.diff(go).max()) if cells else 0, thr.ctypes.data_as(ctypes.c_void_p), thr.size,
                                         P(tp), P(status), None if iou is None else P(iou), None if d_io is None else P(d_io),
                                         _lib.current_stream()), "gte_box_match_f64")
    else:
        _lib.check(lib.gte_box_match(P(pred_box), P(d_po), P(gt_box), P(d_go), cells, int(np.diff(po).max()) if cells else 0,
                                     int(np.diff(go).max()) if cells else 0, thr.ctypes.data_as(ctypes.c_void_p), thr.size, P(tp),
                                     P(status), _lib.current_stream()), "gte_box_match")
    bad = torch.nonzero(status).flatten()
    if bad.numel():
        b = int(bad[0])
        raise ValueError(f"box_match: cell {b} ({int(po[b + 1] - po[b])} predicted x {int(go[b + 1] - go[b])} ground-truth boxes) has more "
                         f"than {lib.gte_box_match_max_candidates()} pairs above IoU {thr[0]} (status {int(status[b])})")
    return (tp, iou) if return_iou else tp


def average_precisions(cells: RegionCells, tp):
    """Stage three of :func:`evaluate_regions`: the cells and their match counts (``tp`` integer array [n_iou, R], the host copy of
    :func:`box_match`'s result) -> the result of :func:`evaluate_regions`.  The sweep of a kind is one cumulative sum: a page's
    counts change only at its own scores, so every cell adds per-event deltas at the positions of its scores among the kind's
    thresholds.  Pure numpy."""
    tp = np.asarray(tp, dtype=np.int64)
    n_iou, po, go = tp.shape[0], cells.pred_off, cells.gt_off
    out = {}
    for kind in cells.kinds:
        thr = cells.thresholds[kind]
        d_tp, d_fp, d_fn = (np.zeros((n_iou, thr.size), dtype=np.int64) for _ in range(3))
        for b, (ck, sc) in enumerate(zip(cells.kind, cells.scores)):
            if ck != kind or thr.size == 0:
                continue
            r, g = sc.shape[0], go[b + 1] - go[b]
            own = np.unique(sc)                                              # the page's own scores, ascending
            k = np.concatenate([[0], np.searchsorted(sc, own[1:], side='left')]).astype(np.int64) if r else np.zeros(1, dtype=np.int64)
            at = np.concatenate([[0], np.searchsorted(thr, own[1:])]).astype(np.int64) if r else np.zeros(1, dtype=np.int64)
            t = tp[:, po[b] + k] if r else np.zeros((n_iou, 1), dtype=np.int64)              # [n_iou, events]
            for acc, val in ((d_tp, t), (d_fp, (r - k)[None, :] - t), (d_fn, g - t)):
                val = np.diff(val, axis=1, prepend=0)                        # the first event carries the whole state k = 0
                acc[:, at] += val                                             # (own scores are distinct: so are the columns)
        s_tp, s_fp, s_fn = (np.cumsum(d, axis=1) for d in (d_tp, d_fp, d_fn))
        with np.errstate(divide='ignore', invalid='ignore'):
            prec = np.where(s_tp + s_fp > 0, s_tp / (s_tp + s_fp), 0.0)
            rec = np.where(s_tp + s_fn > 0, s_tp / (s_tp + s_fn), 0.0)
        ap = []
        for j in range(n_iou):
            levels = [prec[j][rec[j] >= lv] for lv in np.linspace(0.0, 1.0, 11)]
            ap.append(float(np.mean([a.max() if a.size else 0.0 for a in levels])))
        out[kind] = {'ap': ap, 'map': float(np.mean(ap)), 'precisions': prec.tolist(), 'recalls': rec.tolist(),
                     'thresholds': thr.tolist()}
    out['map'] = float(np.mean([out[k]['map'] for k in cells.kinds])) if cells.kinds else 0.0
    return out


def evaluate_regions(pred_doc, gt_doc, iou_thrs=None, count_unpaired=False, device=None, float_boxes=False):
    """Box-level evaluation of predicted regions: the reference's AP at IoU thresholds (``get_avg_precision_at_iou`` of
    src/utils/metrics.py:162-244 per kind and threshold, their mean as in evaluate.py:116-129), with the box matching of all
    pages, kinds and thresholds in ONE launch (``box_match`` -> gte_box_match) and the curve from its integer counts.

    ``pred_doc[kind][page] = {'bboxes': [[x0, y0, x1, y1], ...], 'scores': [...]}`` (``postprocessing.regions_json``),
    ``gt_doc[kind][page] = [[x0, y0, x1, y1], ...]`` (``postprocessing.regions_gt_json``); ``iou_thrs``: 1 .. 16 ascending
    thresholds (default ``np.linspace(0.5, 0.95, 10)``).  What the reference computes is NOT the textbook sweep, and this restates
    it exactly:

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
    'thresholds': [score thresholds]}, ..., 'map': mean of the kinds' 'map'}`` over the kinds of ``gt_doc`` and ``pred_doc``.

    ``float_boxes=True``: the boxes are float64 and the IoU is the reference's ``calc_iou_individual`` on floats, bit for bit
    (gte_box_match_f64) -- for the block route's document (``postprocessing.blocks_json``, coordinates divided by 0.36) against
    annotation boxes (``postprocessing.blocks_gt_json``), the evaluation of the reference's models/evaluate.py:64-131.  ``False``
    casts every coordinate to an integer."""
    iou_thrs = np.linspace(0.5, 0.95, 10) if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    cells = region_cells(pred_doc, gt_doc, count_unpaired, float_boxes)
    tp = np.zeros((iou_thrs.size, 0), dtype=np.int64)
    if cells.kind:
        device = _lib.default_device(device)
        tp = box_match(torch.from_numpy(cells.pred_box).to(device), cells.pred_off, torch.from_numpy(cells.gt_box).to(device),
                       cells.gt_off, iou_thrs, float_boxes=float_boxes).cpu().numpy()
    return average_precisions(cells, tp)


# ---- area-weighted precision / recall / F1 per class: the DocBank token metric, and the reference's evaluate_doc ------------------
# Three public stages in a row, as evaluate_regions: doc_cells (host) -> area_confusion (gte_doc_eval, ONE C call) -> doc_prf
# (host, numpy), so that the host stages run (and are tested) without a device, with a CPU oracle in place of the call.
class DocCells(NamedTuple):
    """Result of :func:`doc_cells`: the arguments of :func:`area_confusion`."""
    gt: np.ndarray            # int32 [N]  all pages concatenated
    pred: np.ndarray          # int32 [N]
    bbox: np.ndarray          # int32 [N, 4]
    n_classes: int


def _doc_flat(x, what, paged, width=None):
    """``x`` -- one array, or a sequence with one array per page when ``paged`` -- as (one integer array, the pages' sizes)."""
    def one(a):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if width is not None and a.size % width:
            raise ValueError(f"evaluate_doc: {what} of {a.size} values are not rows of {width}")
        a = a.reshape(-1) if width is None else a.reshape(-1, width)
        if a.dtype.kind not in 'iu':
            if a.dtype.kind not in 'fb' or not (np.isfinite(a).all() and (a == np.trunc(a)).all()):
                raise ValueError(f"evaluate_doc: {what} are not integral")
        if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
            raise ValueError(f"evaluate_doc: {what} do not fit 32 bits")
        return a.astype(np.int64)
    if not paged:
        return one(x), None
    parts = [one(a) for a in x]
    empty = np.zeros(0 if width is None else (0, width), dtype=np.int64)
    return (np.concatenate(parts) if parts else empty), [a.shape[0] for a in parts]


def doc_cells(labels, preds, boxes, n_classes=None) -> DocCells:
    """Stage one of :func:`evaluate_doc`; no device is touched.  ``labels``, ``preds`` (integers) and ``boxes`` ([., 4] integers,
    x0, y0, x1, y1) are either flat arrays over all nodes, or sequences with one array per page (``labels`` decides: a list or
    tuple whose first element is itself an array or a sequence), concatenated in that order.  ``n_classes``: default ``max(gt) + 1``,
    as the reference's loop runs.  ``ValueError`` on a page-count mismatch, on unequal lengths (per page and in all), on values
    that are not integral or do not fit 32 bits, on ``n_classes < 1`` (or no node to take it from), and where
    ``max|area| * N >= 2^62``: the int64 sums of gte_doc_eval could overflow."""
    paged = isinstance(labels, (list, tuple)) and len(labels) > 0 and np.ndim(labels[0]) >= 1
    if paged:
        for what, x in (("predictions", preds), ("boxes", boxes)):
            if not isinstance(x, (list, tuple)) or len(x) != len(labels):
                raise ValueError(f"evaluate_doc: {len(labels)} pages of labels, but the {what} are not {len(labels)} pages")
    gt, gt_pages = _doc_flat(labels, "labels", paged)
    pred, pred_pages = _doc_flat(preds, "predictions", paged)
    bbox, box_pages = _doc_flat(boxes, "boxes", paged, width=4)
    if gt_pages != pred_pages or gt_pages != box_pages:
        bad = next(i for i, sizes in enumerate(zip(gt_pages, pred_pages, box_pages)) if len(set(sizes)) > 1)
        raise ValueError(f"evaluate_doc: page {bad} has {gt_pages[bad]} labels, {pred_pages[bad]} predictions, {box_pages[bad]} boxes")
    n = gt.shape[0]
    if pred.shape[0] != n or bbox.shape[0] != n:
        raise ValueError(f"evaluate_doc: {n} labels, {pred.shape[0]} predictions, {bbox.shape[0]} boxes")
    if n_classes is None:
        if n == 0:
            raise ValueError("evaluate_doc: no node to take n_classes from")
        n_classes = int(gt.max()) + 1
    n_classes = int(n_classes)
    if n_classes < 1:
        raise ValueError(f"evaluate_doc: n_classes {n_classes} (the largest label is {int(gt.max()) if n else None})")
    w, h = bbox[:, 2] - bbox[:, 0], bbox[:, 3] - bbox[:, 1]
    largest = int((np.abs(w).astype(np.uint64) * np.abs(h).astype(np.uint64)).max()) if n else 0       # (< 2^64: exact in uint64)
    if largest * n >= 1 << 62:
        raise ValueError(f"evaluate_doc: max|area| * N = {largest} * {n} reaches 2^62: the int64 sums could overflow")
    return DocCells(gt.astype(np.int32), pred.astype(np.int32), np.ascontiguousarray(bbox.astype(np.int32)), n_classes)


def area_confusion(gt, pred, bbox, n_classes, device=None):
    """Stage two of :func:`evaluate_doc`, the one C call (gte_doc_eval; include/gte.h has the contract): ``gt``, ``pred`` int32
    [N] and ``bbox`` int32 [N, 4] (host arrays or tensors) -> ``(area, count, lead)`` as numpy int64.  ``area[g, p]`` /
    ``count[g, p]`` [C + 1, C + 1]: summed box area / number of the nodes labelled ``g`` and predicted ``p``, index ``C`` = none
    of the classes; ``lead`` [2, C]: the area that the reference's evaluate_doc loses from its false positives (row 0) and false
    negatives (row 1).  ``GteError`` above ``gte_doc_eval_max_classes()`` classes.  One synchronisation (the copy back)."""
    lib, P = _lib.load(), _lib.ptr
    device = _lib.default_device(device)
    as_dev = lambda a, shape: torch.as_tensor(a).to(device=device, dtype=torch.int32).reshape(shape).contiguous()
    d_gt, d_pred, d_box = as_dev(gt, (-1,)), as_dev(pred, (-1,)), as_dev(bbox, (-1, 4))
    for t in (d_gt, d_pred, d_box):
        _lib.require_device(t, "area_confusion")
    n, C = d_gt.shape[0], int(n_classes)
    if d_pred.shape[0] != n or d_box.shape[0] != n:
        raise ValueError(f"area_confusion: {n} labels, {d_pred.shape[0]} predictions, {d_box.shape[0]} boxes")
    side = max(C, 0) + 1
    area = torch.empty((side, side), dtype=torch.int64, device=device)
    count = torch.empty((side, side), dtype=torch.int64, device=device)
    lead = torch.empty((2, max(C, 0)), dtype=torch.int64, device=device)
    ws = torch.empty(max(int(lib.gte_doc_eval_workspace_bytes(n, C)), 8), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.gte_doc_eval(P(d_gt), P(d_pred), P(d_box), n, C, P(area), P(count), P(lead), P(ws), ws.numel(),
                                    _lib.current_stream()), "gte_doc_eval")
    return area.cpu().numpy(), count.cpu().numpy(), lead.cpu().numpy()


def doc_prf(area, count, lead, mode='reference'):
    """Stage three of :func:`evaluate_doc`: the sums of :func:`area_confusion` -> a dict of ``precision``, ``recall``, ``f1``
    (float64 [C]) and ``tp_area``, ``fp_area``, ``fn_area`` (int64 [C]).  Pure numpy.

    ``tp = area[c, c]``; ``mode='docbank'``: ``fp`` = the area predicted ``c`` but not labelled ``c``, ``fn`` = labelled but not
    predicted -- the DocBank definition.  ``mode='reference'``: ``fp - lead[0]``, ``fn - lead[1]``, the numbers that the
    reference's evaluate_doc prints (models/evaluate.py:182-202: its ``np.delete`` takes a two-column index array, so the first
    ``t_c`` entries of a class's predicted / labelled list leave the false positives / negatives next to the true positives, and
    the result depends on node order).  ``p = tp / (tp + fp)``, ``r = tp / (tp + fn)``, ``f1 = 2 p r / (p + r)``: float64 divisions
    of the int64 sums, ``0 / 0`` NaN, as numpy gives them there."""
    area, count, lead = (np.asarray(a, dtype=np.int64) for a in (area, count, lead))
    C = area.shape[0] - 1
    if area.shape != (C + 1, C + 1) or count.shape != area.shape or lead.shape != (2, C):
        raise ValueError(f"doc_prf: area {area.shape}, count {count.shape}, lead {lead.shape} are not [C+1, C+1] twice and [2, C]")
    if mode not in ('reference', 'docbank'):
        raise ValueError(f"doc_prf: mode {mode!r} is neither 'reference' nor 'docbank'")
    tp = np.diagonal(area)[:C].copy()
    fp = area[:, :C].sum(axis=0) - tp
    fn = area[:C, :].sum(axis=1) - tp
    if mode == 'reference':
        fp, fn = fp - lead[0], fn - lead[1]
    with np.errstate(divide='ignore', invalid='ignore'):
        p, r = tp / (tp + fp), tp / (tp + fn)
        f1 = (2 * p * r) / (p + r)
    return {'precision': p, 'recall': r, 'f1': f1, 'tp_area': tp, 'fp_area': fp, 'fn_area': fn}


def evaluate_doc(labels, preds, boxes, n_classes=None, device=None):
    """Area-weighted precision / recall / F1 per class (the reference's ``evaluate_doc``, models/evaluate.py:142-209: the DocBank
    token metric, a word counting with the area of its box), all sums in ONE C call on the device.  Arguments as
    :func:`doc_cells`.  Returns ``{'n_classes': C, 'reference': doc_prf(mode='reference'), 'docbank': doc_prf(mode='docbank'),
    'area', 'count', 'lead'}`` -- both the numbers the reference prints and those of the formula it quotes, from the same pass."""
    cells = doc_cells(labels, preds, boxes, n_classes)
    area, count, lead = area_confusion(cells.gt, cells.pred, cells.bbox, cells.n_classes, device=device)
    return {'n_classes': cells.n_classes, 'reference': doc_prf(area, count, lead, 'reference'),
            'docbank': doc_prf(area, count, lead, 'docbank'), 'area': area, 'count': count, 'lead': lead}
