"""CPU reference of the word labels (gte_word_labels / gte_word_labels_compact of include/gte.h, graph.label_words), written from
the contract there; plain Python / numpy (it also runs where the GPU tests run).

The rule restates get_label() and the two loops of get_nodes() of the reference's GraphBuilder.get_graph(set_labels=True)
(builder.py:151-167, 195-216); tests/golden/word_labels_cases.json (tools/make_word_labels_golden.py: the reference's own
functions on hand-made and random pages) pins this restatement to it:
  1. the centre of a word is ((x0 + x2) / 2, (y0 + y3) / 2) in integers, the division truncating towards zero;
  2. the page's annotations are scanned in index order; one whose category is in ``skip`` or outside [0, n_cat) is passed over;
     the first of the others whose rectangle AS GIVEN strictly contains the centre (float64; a NaN or inverted rectangle
     contains nothing) wins;
  3. word_ann = the winner (-1: none); word_label = its category, -1 where that is ``figure_cat`` (the word is dropped), 0 where
     there is no winner;
  4. the node list of a page: its ``figure_cat`` annotations in annotation order (box clamped to +-2^30, NaN -> 0, truncated to
     int32; src = -1 - annotation index), then its words with label >= 0 in word order (src = word index); label through
     ``cat_map``."""
import numpy as np

SKIP = (4, 9, 11, 12)            # TABLE, TABLE_GCELL, TABLE_COL, TABLE_ROW (builder.py:159)
FIGURE = 5
N_CAT = 13
# LableModification.origin_to_conv of the shipped configuration (labels.py:13-19), -1 for None
CAT_MAP = (0, 1, 2, 3, -1, 4, 5, 6, 7, -1, 8, -1, -1)
LIM = 1 << 30


def trunc_half(a, b):
    """(a + b) / 2 with C's integer division (towards zero), on Python ints."""
    s = int(a) + int(b)
    return -((-s) // 2) if s < 0 else s // 2


def centre(word):
    return trunc_half(word[0], word[2]), trunc_half(word[1], word[3])


def label_page(words, ann_box, ann_cat, n_cat=N_CAT, skip=SKIP, figure_cat=FIGURE):
    """One page -> (word_label [n], word_ann [n] page-local or -1) as Python lists."""
    rects = [[float(v) for v in r] for r in np.asarray(ann_box, dtype=np.float64).reshape(-1, 4).tolist()]
    cats = [int(c) for c in ann_cat]
    labels, anns = [], []
    scanned = [(j, r, c) for j, (r, c) in enumerate(zip(rects, cats)) if c not in skip and 0 <= c < n_cat]
    for w in np.asarray(words).reshape(-1, 4).tolist():
        cx, cy = (float(v) for v in centre(w))                           # |.| < 2^31: exact
        label, hit = 0, -1
        for j, r, c in scanned:
            if cx > r[0] and cx < r[2] and cy > r[1] and cy < r[3]:
                label, hit = (-1 if c == figure_cat else c), j
                break
        labels.append(label)
        anns.append(hit)
    return labels, anns


def clamp_coord(v):
    v = float(v)
    if v != v:
        return 0
    return int(max(-float(LIM), min(float(LIM), v)))


def nodes_page(words, ann_box, ann_cat, labels, cat_map=None, n_cat=N_CAT, figure_cat=FIGURE):
    """One page -> (boxes [m][4], labels [m], src [m] page-local: -1 - annotation for a figure node, else the word)."""
    conv = (lambda c: c) if cat_map is None else (lambda c: int(cat_map[c]))
    words = np.asarray(words).reshape(-1, 4).tolist()
    boxes, out, src = [], [], []
    for j, (r, c) in enumerate(zip(np.asarray(ann_box, dtype=np.float64).reshape(-1, 4).tolist(), ann_cat)):
        if int(c) == figure_cat:
            boxes.append([clamp_coord(v) for v in r])
            out.append(conv(figure_cat))
            src.append(-1 - j)
    for i, (w, l) in enumerate(zip(words, labels)):
        if l >= 0:
            boxes.append([int(v) for v in w])
            out.append(conv(l) if l < n_cat else -1)
            src.append(i)
    return boxes, out, src


def label_batch(bbox, node_off, ann_box, ann_cat, ann_off, n_cat=N_CAT, skip=SKIP, figure_cat=FIGURE):
    """gte_word_labels for a batch: (word_label int32 [n], word_ann int32 [n] GLOBAL or -1, page_counts int32 [P, 2])."""
    bbox, ann_box = np.asarray(bbox).reshape(-1, 4), np.asarray(ann_box, dtype=np.float64).reshape(-1, 4)
    ann_cat = np.asarray(ann_cat).reshape(-1)
    n_pages = len(node_off) - 1
    word_label = np.zeros(bbox.shape[0], dtype=np.int32)
    word_ann = np.full(bbox.shape[0], -1, dtype=np.int32)
    counts = np.zeros((n_pages, 2), dtype=np.int32)
    for p in range(n_pages):
        n0, n1, a0, a1 = int(node_off[p]), int(node_off[p + 1]), int(ann_off[p]), int(ann_off[p + 1])
        l, a = label_page(bbox[n0:n1], ann_box[a0:a1], ann_cat[a0:a1], n_cat, skip, figure_cat)
        word_label[n0:n1] = l
        word_ann[n0:n1] = [a0 + j if j >= 0 else -1 for j in a]
        counts[p] = (int((ann_cat[a0:a1] == figure_cat).sum()), sum(1 for v in l if v >= 0))
    return word_label, word_ann, counts


def compact_batch(bbox, node_off, ann_box, ann_cat, ann_off, word_label, cat_map=None, n_cat=N_CAT, figure_cat=FIGURE):
    """gte_word_labels_compact for a batch with the right out_off: (out_bbox int32 [m, 4], out_label int32 [m], out_src int32 [m]
    GLOBAL, out_off int64 [P + 1])."""
    bbox, ann_box = np.asarray(bbox).reshape(-1, 4), np.asarray(ann_box, dtype=np.float64).reshape(-1, 4)
    ann_cat, word_label = np.asarray(ann_cat).reshape(-1), np.asarray(word_label).reshape(-1)
    boxes, labels, srcs, off = [], [], [], [0]
    for p in range(len(node_off) - 1):
        n0, n1, a0, a1 = int(node_off[p]), int(node_off[p + 1]), int(ann_off[p]), int(ann_off[p + 1])
        b, l, s = nodes_page(bbox[n0:n1], ann_box[a0:a1], ann_cat[a0:a1], word_label[n0:n1].tolist(), cat_map, n_cat, figure_cat)
        boxes += b
        labels += l
        srcs += [n0 + v if v >= 0 else -1 - (a0 + (-1 - v)) for v in s]
        off.append(len(boxes))
    return (np.asarray(boxes, dtype=np.int32).reshape(-1, 4), np.asarray(labels, dtype=np.int32), np.asarray(srcs, dtype=np.int32),
            np.asarray(off, dtype=np.int64))
