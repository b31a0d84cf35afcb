"""CPU reference of the box-level evaluation (gte_box_match of include/gte.h, metrics.evaluate_regions) and of the region
confidence (gte_page_regions_scored), written from their definitions; pure Python / numpy (it also runs where the GPU tests run).

The evaluation restates what the reference's get_avg_precision_at_iou (src/utils/metrics.py:162-244) computes, which is not the
textbook sweep -- tests/golden/boxeval_cases.json (tools/make_boxeval_golden.py: the reference's own functions on generated
documents) pins this restatement to it:
  1. only PAIRED pages count: pages that are keys of both the ground-truth and the prediction dict of a kind;
  2. the thresholds are the distinct scores of all predictions of the kind, ascending;
  3. a page's state lags: at threshold t it keeps its predictions with score >= c, c = the largest of the page's own scores <= t
     (every box below the page's first own score);
  4. per page: +1 pixel IoU, disjointness first (touching boxes overlap), candidates iou > thr strictly, greedy in descending IoU;
  5. precision / recall from the summed counts (0.0 on a zero denominator), AP = mean over linspace(0, 1, 11) of the largest
     precision at recall >= level;
  6. ties: among equal IoUs the larger pred_index * n_gt + gt_index first."""
import numpy as np


def iou(p, t):
    """IoU of two integer boxes (x0, y0, x1, y1), +1 pixel convention; Python ints, so the quotient is int / int."""
    px0, py0, px1, py1 = (int(v) for v in p)
    tx0, ty0, tx1, ty1 = (int(v) for v in t)
    if tx1 < px0 or px1 < tx0 or ty1 < py0 or py1 < ty0:
        return 0.0
    inter = (min(tx1, px1) - max(tx0, px0) + 1) * (min(ty1, py1) - max(ty0, py0) + 1)
    return inter / ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) + (px1 - px0 + 1) * (py1 - py0 + 1) - inter)


def candidates(pred, gt, thr):
    """[(iou, pred_index * n_gt + gt_index)] of the pairs with iou > thr, in matching order (point 6)."""
    if len(pred) == 0 or len(gt) == 0:
        return []
    m = iou_matrix(pred, gt).reshape(-1)                  # (== iou() of every pair, bit for bit: tests/test_boxeval_ref_cpu.py)
    pairs = np.nonzero(m > thr)[0]
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
    IoUs (point 6; unspecified in the reference) can reach the result."""
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


def iou_matrix(pred, gt):
    """iou() of every pair as float64 [R, G]: int64 operands below 2^53 converted exactly, one IEEE division -- the same bits."""
    p, t = np.asarray(pred, dtype=np.int64).reshape(-1, 1, 4), np.asarray(gt, dtype=np.int64).reshape(1, -1, 4)
    disjoint = (t[..., 2] < p[..., 0]) | (p[..., 2] < t[..., 0]) | (t[..., 3] < p[..., 1]) | (p[..., 3] < t[..., 1])
    inter = (np.minimum(t[..., 2], p[..., 2]) - np.maximum(t[..., 0], p[..., 0]) + 1) * \
            (np.minimum(t[..., 3], p[..., 3]) - np.maximum(t[..., 1], p[..., 1]) + 1)
    area = lambda b: (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1)
    union = area(t) + area(p) - inter
    return np.where(disjoint, 0.0, inter / np.where(disjoint, 1, union))


def box_match_ref(pred_box, pred_off, gt_box, gt_off, iou_thr):
    """tp [n_thr, R] of gte_box_match: tp[j][pred_off[b] + k] = match_count(cell b's predictions k.., its ground truths,
    iou_thr[j]).  The same walks from ONE sorted candidate list per cell: pruning the first k predictions shifts every pair index
    by k * n_gt and so keeps the order of the remaining candidates (tests/test_boxeval_ref_cpu.py compares the two)."""
    pred_box, gt_box = np.asarray(pred_box).reshape(-1, 4), np.asarray(gt_box).reshape(-1, 4)
    tp = np.zeros((len(iou_thr), pred_box.shape[0]), dtype=np.int32)
    for b in range(len(pred_off) - 1):
        r, n_gt = pred_off[b + 1] - pred_off[b], gt_off[b + 1] - gt_off[b]
        if r == 0 or n_gt == 0:
            continue
        m = iou_matrix(pred_box[pred_off[b]:pred_off[b + 1]], gt_box[gt_off[b]:gt_off[b + 1]]).reshape(-1)
        pairs = np.nonzero(m > min(iou_thr))[0]
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
    return tp


def avg_precision_at_iou(gt_boxes, pred_boxes, iou_thr, count_unpaired=False):
    """Points 1-5 for one kind and one IoU threshold: {'avg_prec', 'precisions', 'recalls', 'model_thrs'}.  gt_boxes[page] =
    [box, ...], pred_boxes[page] = {'bboxes', 'scores'}.  A plain loop over thresholds x pages, on purpose."""
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
    """The result of metrics.evaluate_regions, from avg_precision_at_iou."""
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


def region_scores_ref(comp, group, logits, class_group):
    """float64 [n]: at every root (comp[v] == v) the mean over the region's members of the softmax mass of their logits on the
    classes c with class_group[c] == the member's kind (0 for a row with a non-finite logit); 0 at every other row."""
    comp, group = np.asarray(comp, dtype=np.int64), np.asarray(group, dtype=np.int64)
    logits, class_group = np.asarray(logits, dtype=np.float64), np.asarray(class_group, dtype=np.int64)
    n = comp.shape[0]
    p = np.zeros(n, dtype=np.float64)
    ok = np.isfinite(logits).all(axis=1) & (comp >= 0)
    z = logits[ok]
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p[ok] = (e * (class_group[None, :] == group[ok][:, None])).sum(axis=1) / e.sum(axis=1)
    total, count = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64)
    member = comp >= 0
    np.add.at(total, comp[member], p[member])
    np.add.at(count, comp[member], 1)
    return np.where(count > 0, total / np.maximum(count, 1), 0.0)
