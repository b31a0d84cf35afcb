"""CPU reference of the box-level evaluation on FLOAT boxes (gte_box_match_f64 of include/gte.h, metrics.evaluate_regions(...,
float_boxes=True)), written from the definitions; pure Python / numpy (it also runs where the GPU tests run).

The evaluation is the one tests/boxeval_ref.py restates (its points 1-6: paired pages, lagging page state, strict thresholds,
greedy matching, ties to the larger pair index); what changes is the IoU, and with it every function that reaches it -- those are
carried here in their own copies.  On floats the IoU is not a quotient of exact integers: every intermediate rounds, so the bits
depend on the order of the operations.  The order is calc_iou_individual's (src/utils/metrics.py:42-53):
    disjoint (x2_t < x1_p or x2_p < x1_t or y2_t < y1_p or y2_p < y1_t) -> 0.0
    inter = ((far_x - near_x) + 1) * ((far_y - near_y) + 1)
    area  = ((x2 - x1) + 1) * ((y2 - y1) + 1)                       per box
    iou   = inter / ((true_area + pred_area) - inter)
in IEEE double, one rounding per operation.  tests/golden/boxeval_float_cases.json (tools/make_boxeval_float_golden.py: the
reference's own functions on generated float documents, with the reference's IoU of every pair stored beside the curves) pins
this restatement to it, bit for bit.  A box is well formed when its four values are finite, x0 <= x1, y0 <= y1 and |v| <= 2^24;
any other box overlaps nothing (the reference raises on inverted corners and has no other rule)."""
import math

import numpy as np

MAX_COORD = float(1 << 24)


def well_formed(b):
    x0, y0, x1, y1 = (float(v) for v in b)
    return all(math.isfinite(v) and abs(v) <= MAX_COORD for v in (x0, y0, x1, y1)) and x0 <= x1 and y0 <= y1


def iou(p, t):
    """IoU of two float boxes (x0, y0, x1, y1) on Python floats: IEEE double, the reference's order of operations."""
    if not (well_formed(p) and well_formed(t)):
        return 0.0
    px0, py0, px1, py1 = (float(v) for v in p)
    tx0, ty0, tx1, ty1 = (float(v) for v in t)
    if tx1 < px0 or px1 < tx0 or ty1 < py0 or py1 < ty0:
        return 0.0
    far_x, near_x, far_y, near_y = min(tx1, px1), max(tx0, px0), min(ty1, py1), max(ty0, py0)
    inter = ((far_x - near_x) + 1.0) * ((far_y - near_y) + 1.0)
    true_area = ((tx1 - tx0) + 1.0) * ((ty1 - ty0) + 1.0)
    pred_area = ((px1 - px0) + 1.0) * ((py1 - py0) + 1.0)
    return inter / ((true_area + pred_area) - inter)


def iou_matrix(pred, gt):
    """iou() of every pair as float64 [R, G]: the same operations in the same order on numpy arrays (numpy neither reorders nor
    contracts) -- the same bits (tests/test_boxeval_float_ref_cpu.py compares the two)."""
    p, t = np.asarray(pred, dtype=np.float64).reshape(-1, 1, 4), np.asarray(gt, dtype=np.float64).reshape(1, -1, 4)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        ok = lambda b: np.isfinite(b).all(axis=-1) & (np.abs(b) <= MAX_COORD).all(axis=-1) & (b[..., 0] <= b[..., 2]) & (b[..., 1] <= b[..., 3])
        disjoint = (t[..., 2] < p[..., 0]) | (p[..., 2] < t[..., 0]) | (t[..., 3] < p[..., 1]) | (p[..., 3] < t[..., 1])
        none = disjoint | ~(ok(p) & ok(t))
        inter = ((np.minimum(t[..., 2], p[..., 2]) - np.maximum(t[..., 0], p[..., 0])) + 1.0) * \
                ((np.minimum(t[..., 3], p[..., 3]) - np.maximum(t[..., 1], p[..., 1])) + 1.0)
        area = lambda b: ((b[..., 2] - b[..., 0]) + 1.0) * ((b[..., 3] - b[..., 1]) + 1.0)
        union = (area(t) + area(p)) - inter
        return np.where(none, 0.0, inter / np.where(none, 1.0, union))


def candidates(pred, gt, thr):
    """[(iou, pred_index * n_gt + gt_index)] of the pairs with a finite iou > thr, in matching order (IoU, then pair index,
    descending)."""
    if len(pred) == 0 or len(gt) == 0:
        return []
    m = iou_matrix(pred, gt).reshape(-1)
    pairs = np.nonzero(np.isfinite(m) & (m > thr))[0]
    return sorted(zip(m[pairs].tolist(), pairs.tolist()), reverse=True)


def match_count(pred, gt, thr):
    """tp of one page: greedy matching of the candidates in descending (IoU, pair index)."""
    n_gt = len(gt)
    used_p, used_t = set(), set()
    for _, pair in candidates(pred, gt, thr):
        ip, it = divmod(pair, n_gt)
        if ip not in used_p and it not in used_t:
            used_p.add(ip)
            used_t.add(it)
    return len(used_p)


def has_shared_tie(pred, gt, thr):
    """True when two candidates of equal IoU share a prediction or a ground truth: the only case in which the order among equal
    IoUs (unspecified in the reference) can reach the result."""
    n_gt = len(gt)
    c = candidates(pred, gt, thr)
    for a in range(len(c)):
        for b in range(a + 1, len(c)):
            if c[b][0] != c[a][0]:
                break
            pa, ta = divmod(c[a][1], n_gt)
            pb, tb = divmod(c[b][1], n_gt)
            if pa == pb or ta == tb:
                return True
    return False


def box_match_ref(pred_box, pred_off, gt_box, gt_off, iou_thr, return_iou=False):
    """tp [n_thr, R] of gte_box_match_f64: tp[j][pred_off[b] + k] = match_count(cell b's predictions k.., its ground truths,
    iou_thr[j]), from ONE sorted candidate list per cell (pruning the first k predictions keeps the order of the remaining
    candidates).  ``return_iou``: also the cells' IoU matrices, row-major, concatenated."""
    pred_box, gt_box = np.asarray(pred_box, dtype=np.float64).reshape(-1, 4), np.asarray(gt_box, dtype=np.float64).reshape(-1, 4)
    tp = np.zeros((len(iou_thr), pred_box.shape[0]), dtype=np.int32)
    ious = []
    for b in range(len(pred_off) - 1):
        r, n_gt = pred_off[b + 1] - pred_off[b], gt_off[b + 1] - gt_off[b]
        if r == 0 or n_gt == 0:
            continue
        m = iou_matrix(pred_box[pred_off[b]:pred_off[b + 1]], gt_box[gt_off[b]:gt_off[b + 1]]).reshape(-1)
        ious.append(m)
        pairs = np.nonzero(np.isfinite(m) & (m > min(iou_thr)))[0]
        cand = sorted(zip(m[pairs].tolist(), pairs.tolist()), reverse=True)
        for j, thr in enumerate(iou_thr):
            for k in range(r):
                used_p, used_t = set(), set()
                for v, pair in cand:
                    if not v > thr:
                        break
                    ip, it = divmod(pair, n_gt)
                    if ip >= k and ip not in used_p and it not in used_t:
                        used_p.add(ip)
                        used_t.add(it)
                tp[j, pred_off[b] + k] = len(used_p)
    if return_iou:
        return tp, (np.concatenate(ious) if ious else np.zeros(0))
    return tp


def avg_precision_at_iou(gt_boxes, pred_boxes, iou_thr, count_unpaired=False):
    """One kind and one IoU threshold: {'avg_prec', 'precisions', 'recalls', 'model_thrs'} -- boxeval_ref.avg_precision_at_iou
    with this module's match_count.  A plain loop over thresholds x pages, on purpose."""
    thresholds = sorted({float(s) for e in pred_boxes.values() for s in e['scores']})
    pages = {}
    for pg in list(gt_boxes) + [p for p in pred_boxes if p not in gt_boxes]:
        if (pg in gt_boxes and pg in pred_boxes) or count_unpaired:
            e = pred_boxes.get(pg, {'bboxes': [], 'scores': []})
            order = np.argsort(np.asarray(e['scores'], dtype=np.float64), kind='stable').tolist()
            pages[pg] = ([float(e['scores'][i]) for i in order], [e['bboxes'][i] for i in order], gt_boxes.get(pg, []))
    precisions, recalls, seen = [], [], {}
    for t in thresholds:
        tp = fp = fn = 0
        for pg, (scores, boxes, gt) in pages.items():
            own = [s for s in scores if s <= t]
            c = max(own) if own else None
            kept = [b for s, b in zip(scores, boxes) if c is None or s >= c]
            if (pg, len(kept)) not in seen:               # (kept is a suffix of the page's sorted boxes: its length names it)
                seen[pg, len(kept)] = match_count(kept, gt, iou_thr)
            m = seen[pg, len(kept)]
            tp, fp, fn = tp + m, fp + len(kept) - m, fn + len(gt) - m
        precisions.append(tp / (tp + fp) if tp + fp else 0.0)
        recalls.append(tp / (tp + fn) if tp + fn else 0.0)
    levels = []
    for level in np.linspace(0.0, 1.0, 11):
        at = [p for p, r in zip(precisions, recalls) if r >= level]
        levels.append(max(at) if at else 0.0)
    return {'avg_prec': float(np.mean(levels)), 'precisions': precisions, 'recalls': recalls, 'model_thrs': thresholds}


def evaluate_doc_ref(pred_doc, gt_doc, iou_thrs=None, count_unpaired=False):
    """The result of metrics.evaluate_regions(..., float_boxes=True), from avg_precision_at_iou."""
    iou_thrs = np.linspace(0.5, 0.95, 10) if iou_thrs is None else iou_thrs
    kinds = list(gt_doc) + [k for k in pred_doc if k not in gt_doc]
    out = {}
    for kind in kinds:
        res = [avg_precision_at_iou(gt_doc.get(kind, {}), pred_doc.get(kind, {}), float(t), count_unpaired) for t in iou_thrs]
        ap = [r['avg_prec'] for r in res]
        out[kind] = {'ap': ap, 'map': float(np.mean(ap)), 'precisions': [r['precisions'] for r in res],
                     'recalls': [r['recalls'] for r in res], 'thresholds': res[0]['model_thrs'] if res else []}
    out['map'] = float(np.mean([out[k]['map'] for k in kinds])) if kinds else 0.0
    return out
