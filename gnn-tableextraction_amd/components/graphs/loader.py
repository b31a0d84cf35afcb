"""Pre-built page-graph dataset: the OUTPUT CONTRACT of the reference's ``Papers2Graphs`` after
``modify_graphs`` (src/components/graphs/loader.py:206-393) without the PDF pipeline behind it.

The train loop needs from ``data``: ``num_classes``, ``stats``, ``graphs`` (each with
``ndata['feat'|'label']`` and ``edata['feat']``), ``split(n)`` (95/5, ``random.sample`` seeded 42:
loader.py:48,395-420), ``label_tranformer`` and ``__len__``.  DGL's ``.bin`` cache cannot be read
without DGL, so the on-disk format here is one ``.npz`` holding the concatenated COO, features,
labels and per-page offsets (``save`` / ``load``).
"""
from __future__ import annotations

import random
from typing import List, Optional, Sequence

import numpy as np
import torch

from ...graph import PageGraph
from ...data import synthetic as S

# src/components/graphs/labels.py:13-19: 13 categories minus the never-instantiated {4, 9, 11, 12}
ORIGIN_TO_CONV = {0: 0, 1: 1, 2: 2, 3: 3, 5: 4, 6: 5, 7: 6, 8: 7, 10: 8, 4: None, 9: None, 11: None, 12: None}
# builder.py:159, 164: the categories get_label passes over (TABLE, TABLE_GCELL, TABLE_COL, TABLE_ROW) and the one that drops a word
SKIPPED, FIGURE = (4, 9, 11, 12), 5


class LabelTransformer:
    def __init__(self):
        self.origin_to_conv = dict(ORIGIN_TO_CONV)
        self.conv_to_origin = {v: k for k, v in ORIGIN_TO_CONV.items() if v is not None}


class PrebuiltPages:
    def __init__(self, pages: Sequence[S.Page], num_classes: int = 9, rate: float = 0.95, seed: int = 42,
                 float_labels: bool = True, labeled: bool = True):
        """``labeled=False``: pages without ground truth (``from_boxes(unlabeled=True)``; ``Page.label`` is None): the graphs
        carry no ``ndata['label']`` and ``stats`` counts nothing.  Such a set is for ``model_predict.predict()`` only."""
        self.page_arrays = list(pages)
        self.labeled = bool(labeled)
        self.num_classes = num_classes
        self.rate, self.seed = rate, seed
        self.label_tranformer = LabelTransformer()          # (sic) the reference's attribute name
        self.graphs: List[PageGraph] = []
        counts = np.zeros(num_classes, dtype=np.int64)
        for p in self.page_arrays:
            g = PageGraph(p.src, p.dst, p.num_nodes)
            g.ndata['feat'] = torch.from_numpy(p.feat)
            # the reference stores labels as float32 and casts at the loss (loader.py:350-354)
            if self.labeled:
                g.ndata['label'] = torch.from_numpy(p.label.astype(np.float32) if float_labels else p.label)
            g.edata['feat'] = torch.from_numpy(p.weight)
            self.graphs.append(g)
            if self.labeled:
                counts += np.bincount(p.label, minlength=num_classes)
        total = max(int(counts.sum()), 1)
        self.stats = {'numbers': counts.tolist(), 'percentages': [round(c / total, 2) for c in counts.tolist()]}
        self.pages = [{'page': f'synthetic_{i}', 'bboxs': p.bbox, 'texts': None} for i, p in enumerate(self.page_arrays)]

    def __len__(self):
        return len(self.graphs)

    def split(self, num_graphs: Optional[int] = None):
        n = min(num_graphs or len(self), len(self))
        train_amount = int(n * self.rate)
        rnd = random.Random(self.seed)
        train_idx = rnd.sample(range(0, n), train_amount)
        val_idx = sorted(set(range(0, n)) - set(train_idx))
        return [self.graphs[i] for i in train_idx], [self.graphs[i] for i in val_idx], (train_idx, val_idx)

    # ---- on-disk format replacing save_graphs(.bin) + save_info(.pkl) (loader.py:98-113) ----------
    def save(self, path: str) -> None:
        src, dst, w, feat, label, off = S.concat_pages(self.page_arrays)
        eoff = np.cumsum([0] + [len(p.src) for p in self.page_arrays])
        arrays = dict(src=src, dst=dst, weight=w, feat=feat, label=label, node_off=off, edge_off=eoff,
                      bbox=np.concatenate([p.bbox for p in self.page_arrays]), num_classes=self.num_classes)
        if not self.labeled:                                # an unlabelled set: no 'label' entry; load() tells by its absence
            del arrays['label']
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path: str, **kw) -> "PrebuiltPages":
        z = np.load(path)
        no, eo = z["node_off"], z["edge_off"]
        labeled = "label" in z.files
        pages = []
        for i in range(len(no) - 1):
            n0, n1, e0, e1 = int(no[i]), int(no[i + 1]), int(eo[i]), int(eo[i + 1])
            pages.append(S.Page((z["src"][e0:e1] - n0).astype(np.int32), (z["dst"][e0:e1] - n0).astype(np.int32),
                                z["weight"][e0:e1], z["feat"][n0:n1], z["label"][n0:n1] if labeled else None, z["bbox"][n0:n1]))
        if not labeled:
            kw = dict(kw, labeled=False)
        return cls(pages, num_classes=int(z["num_classes"]), **kw)

    @classmethod
    def from_boxes(cls, page_boxes, page_sizes, page_texts, page_labels, device, k: int = 5, max_dist: int = 500,
                   bidirectional: bool = True, range_island: int = 0, extra_feats=None, mode: str = "knn",
                   page_annotations=None, converted: bool = True, **kw) -> "PrebuiltPages":
        """Pages from word boxes with the graph stage on the DEVICE: k-NN edges, island removal,
        to_simple + to_bidirected, edge weights (graph.knn_graph_from_boxes) and the 13 BBOX node features
        (graph.bbox_features) -- what builder.get_graph + loader.modify_graphs + nlp/bbox.py do per page in Python.
        ``page_boxes[p]`` int [n_p, 4], ``page_sizes[p]`` = (width, height), ``page_texts[p]`` the words (for the character
        histogram; None -> empty texts), ``page_labels[p]`` converted class ids, ``extra_feats[p]`` optional float32 [n_p, F']
        columns appended behind them (SPACY embeddings, which need a language model and stay pre-computed).
        ``repr_embedder`` (keyword, default None): a ``components.nlp.repr.Repr``; its P REPR columns (50 in the reference) follow
        the 13 BBOX columns and precede ``extra_feats`` -- the order of the reference's feature list -- computed on the device
        (graph.repr_features) from the texts of the node lists.  Token j of a page belongs to node j of the list BEFORE island
        removal (an empty word shifts the tokens of its page, as in the reference); the rows are then filtered as the BBOX rows
        are.  None leaves every result as it was.
        ``scibert_embedder`` (keyword, default None): a ``components.nlp.scibert.SciBERT``; its D SCIBERT columns (768 in the
        reference) follow the REPR columns and precede ``extra_feats``: ``[BBOX 13 | REPR P | SCIBERT D | extra_feats]``.  They are
        computed on the device (graph.token_pool, one launch) from the texts of the node lists BEFORE island removal -- which words
        pool their ``[SEP]`` depends on the longest word of the page as the reference sees it -- and written for the kept rows
        only, straight into their columns of the final matrix.  None leaves every result as it was.

        ``page_annotations`` INSTEAD of ``page_labels`` (exactly one of the two, the other None): ``page_annotations[p]`` rows
        ``[x0, y0, x1, y1, category]`` with ORIGINAL category ids, what ``postprocessing.blocks_gt_json`` reads.  The node list
        is then built as ``GraphBuilder.get_graph(set_labels=True)`` builds it (graph.label_words: labels by the first
        annotation that holds a word's centre, words inside a FIGURE dropped, every FIGURE a node "IMAGE!" in front of its
        page's words) and the path above runs on it; ``converted`` applies ``LableModification``'s conversion (False: original
        ids, ``num_classes`` 13).  ``extra_feats`` must then be a callable ``(page_texts, page_boxes) -> [n_p, F'] arrays`` of the
        FINAL node lists: arrays per input word cannot line up once figure nodes are added and words dropped.  A
        ``repr_embedder`` and a ``scibert_embedder`` read the texts of those node lists, ``"IMAGE!"`` for a figure node.
        ``pages[i]`` gains ``'annotations'`` (as given) and ``'texts'`` (of the final nodes).

        ``unlabeled=True`` (keyword, default False): the words of a document without ground truth -- the reference's ``GenericPapers2Graphs``
        (loader.py:431-573: ``get_graph(..., set_labels=False)``, so no labels, no FIGURE nodes, no island removal).
        ``page_labels`` and ``page_annotations`` must both be None and ``range_island`` 0 (island removal reads labels);
        ``ValueError`` otherwise, before any device call.  The labels route runs without labels -- the same graph, edge weights
        and feature columns, every word kept -- and the result has ``labeled == False``: graphs without ``ndata['label']``,
        ``stats`` of zero counts, ``num_classes`` from the keyword (default 9).  It is input to ``model_predict.predict()``;
        ``train()`` and ``test()`` refuse it."""
        repr_embedder = kw.pop('repr_embedder', None)
        scibert_embedder = kw.pop('scibert_embedder', None)
        if kw.pop('unlabeled', False):
            if page_labels is not None or page_annotations is not None:
                raise ValueError("from_boxes: unlabeled=True takes neither page_labels nor page_annotations (got "
                                 f"{'page_labels' if page_labels is not None else 'page_annotations'})")
            if range_island != 0:
                raise ValueError(f"from_boxes: unlabeled=True needs range_island 0 (got {range_island}): island removal reads labels")
            return cls._from_node_lists(page_boxes, page_sizes, page_texts, None, device, k, max_dist, bidirectional, 0,
                                        extra_feats, mode, dict(kw, labeled=False), repr_embedder=repr_embedder,
                                        scibert_embedder=scibert_embedder)[0]
        if (page_labels is None) == (page_annotations is None):
            raise ValueError("from_boxes: exactly one of page_labels and page_annotations must be given, for all pages (got "
                             f"{'both' if page_labels is not None else 'neither'})")
        if page_annotations is not None:
            return cls._from_annotations(page_boxes, page_sizes, page_texts, page_annotations, device, converted, extra_feats,
                                         dict(k=k, max_dist=max_dist, bidirectional=bidirectional, range_island=range_island,
                                              mode=mode), kw, repr_embedder=repr_embedder,
                                         scibert_embedder=scibert_embedder)
        return cls._from_node_lists(page_boxes, page_sizes, page_texts, page_labels, device, k, max_dist, bidirectional,
                                    range_island, extra_feats, mode, kw, repr_embedder=repr_embedder,
                                    scibert_embedder=scibert_embedder)[0]

    @classmethod
    def _from_node_lists(cls, page_boxes, page_sizes, page_texts, page_labels, device, k, max_dist, bidirectional, range_island,
                         extra_feats, mode, kw, extra_feats_fn=None, repr_embedder=None, scibert_embedder=None):
        """from_boxes for node lists that carry their labels -> (dataset, keep: bool [N] on the device over the given nodes).
        ``extra_feats_fn(page_texts, page_boxes)``: the extra columns as a callable on the node lists that are left after island
        removal."""
        from ... import graph as G
        from ..nlp.bbox import Bbox
        device = torch.device(device)
        n_pages = len(page_boxes)
        sizes = [len(b) for b in page_boxes]
        node_off = np.concatenate([[0], np.cumsum(sizes)])
        bbox = torch.from_numpy(np.concatenate([np.asarray(b, dtype=np.int32).reshape(-1, 4) for b in page_boxes])).to(device)
        labels = None                                      # (page_labels None: the unlabelled route -- no labels anywhere below)
        if page_labels is not None:
            labels = torch.from_numpy(np.concatenate([np.asarray(l, dtype=np.int64) for l in page_labels])).to(device)
        g, keep = G.knn_graph_from_boxes(bbox, node_off, np.asarray(page_sizes, dtype=np.int32), k=k, max_dist=max_dist,
                                         bidirectional=bidirectional, labels=labels, range_island=range_island,
                                         mode=mode)                  # PREPROCESS.mode: 'knn' | 'visibility' (loader.py:80)
        texts = page_texts if page_texts is not None else [[""] * n for n in sizes]
        parts = [Bbox(device).features(page_boxes, texts)[keep]]
        if repr_embedder is not None:                      # [BBOX | REPR | SCIBERT | extra]: the order of the reference's feature list
            parts.append(repr_embedder.features(texts)[keep])
        scibert_at = len(parts)                            # (its columns are written in place once the whole width is known)
        if extra_feats is not None:
            parts.append(torch.from_numpy(np.concatenate([np.asarray(e, dtype=np.float32) for e in extra_feats])).to(device)[keep])
        if extra_feats_fn is not None:
            keep_h = keep.cpu().numpy()
            kept = [keep_h[int(node_off[p]):int(node_off[p + 1])] for p in range(n_pages)]
            final_texts = [[t for t, ok in zip(texts[p], kept[p].tolist()) if ok] for p in range(n_pages)]
            final_boxes = [np.asarray(page_boxes[p], dtype=np.int32).reshape(-1, 4)[kept[p]] for p in range(n_pages)]
            extra = extra_feats_fn(final_texts, final_boxes)
            extra = torch.from_numpy(np.concatenate([np.asarray(e, dtype=np.float32).reshape(len(t), -1)
                                                     for e, t in zip(extra, final_texts)])).to(device)
            parts.append(extra)
        if scibert_embedder is None:
            feat = torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]
        else:
            # the SCIBERT columns go straight into their slice of the final matrix, for the kept rows only (graph.token_pool:
            # row_map): no [N, D] temporary, no [keep] copy of it, no cat
            widths = [p.shape[1] for p in parts[:scibert_at]] + [scibert_embedder.n_out] + [p.shape[1] for p in parts[scibert_at:]]
            cols = np.concatenate([[0], np.cumsum(widths)])
            feat = torch.empty((parts[0].shape[0], int(cols[-1])), dtype=torch.float32, device=device)
            for j, p in enumerate(parts[:scibert_at] + [None] + parts[scibert_at:]):
                if p is not None:
                    feat[:, int(cols[j]):int(cols[j + 1])] = p
            row_map = torch.where(keep, torch.cumsum(keep, 0) - 1, -1)
            scibert_embedder.features(texts, out=feat[:, int(cols[scibert_at]):int(cols[scibert_at + 1])], row_map=row_map)
        # per-page host arrays (the dataset object's contract: .graphs[i] with ndata feat/label, edata feat, .pages[i]['bboxs'])
        src, dst = (t.cpu().numpy() for t in g.edges())
        w = g.edata['feat'].cpu().numpy()
        feat_h, bbox_h = feat.cpu().numpy(), g.ndata['bbox'].cpu().numpy()
        lab_h = None if labels is None else g.ndata['label'].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(g.batch_num_nodes_)])
        eoff = np.searchsorted(dst, off)                   # edges are sorted by destination
        pages = []
        for p in range(n_pages):
            n0, n1, e0, e1 = int(off[p]), int(off[p + 1]), int(eoff[p]), int(eoff[p + 1])
            pages.append(S.Page((src[e0:e1] - n0).astype(np.int32), (dst[e0:e1] - n0).astype(np.int32), w[e0:e1],
                                np.ascontiguousarray(feat_h[n0:n1]), None if lab_h is None else lab_h[n0:n1].astype(np.int64),
                                bbox_h[n0:n1]))
        out = cls(pages, **kw)
        g.ndata['feat'] = feat
        out.whole = g                                       # the batched device graph, for callers that stay on the device
        return out, keep

    @staticmethod
    def check_annotations(page_annotations, n_pages: int):
        """Host validation of ``page_annotations`` (no device needed) -> (ann_box float64 [A, 4], ann_cat int32 [A], ann_off int64
        [P + 1]).  ``ValueError`` naming the page for: a page count other than ``n_pages``; a row that is not five numbers; a
        category that is not an integer in 0 .. 12; a FIGURE annotation (it becomes a node with an int32 box) with a
        non-integral coordinate or one beyond +-2^30."""
        import math
        import numbers
        if len(page_annotations) != n_pages:
            raise ValueError(f"from_boxes: page_annotations names {len(page_annotations)} pages, page_boxes {n_pages}")
        boxes, cats, off = [], [], [0]
        for p, rows in enumerate(page_annotations):
            for row in rows:
                row = row.tolist() if isinstance(row, np.ndarray) else row
                if (not isinstance(row, (list, tuple)) or len(row) != 5
                        or not all(isinstance(v, numbers.Real) and not isinstance(v, bool) for v in row)):
                    raise ValueError(f"from_boxes: page {p}: annotation {row!r} is not five numbers [x0, y0, x1, y1, category]")
                c = row[4]
                if not math.isfinite(c) or int(c) != c or not 0 <= int(c) < len(ORIGIN_TO_CONV):
                    raise ValueError(f"from_boxes: page {p}: annotation {row!r}: the category is not an integer in 0 .. "
                                     f"{len(ORIGIN_TO_CONV) - 1}")
                if int(c) == FIGURE:
                    for v in row[:4]:
                        if not math.isfinite(v) or abs(v) > 2 ** 30 or int(v) != v:
                            raise ValueError(f"from_boxes: page {p}: FIGURE annotation {row!r} becomes a node: its coordinates "
                                             f"must be whole numbers within +-2^30")
                boxes.append([float(v) for v in row[:4]])
                cats.append(int(c))
            off.append(len(cats))
        return (np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(cats, dtype=np.int32),
                np.asarray(off, dtype=np.int64))

    @classmethod
    def _from_annotations(cls, page_boxes, page_sizes, page_texts, page_annotations, device, converted, extra_feats, graph_kw, kw,
                          repr_embedder=None, scibert_embedder=None):
        from ... import graph as G
        n_pages = len(page_boxes)
        ann_box, ann_cat, ann_off = cls.check_annotations(page_annotations, n_pages)
        if extra_feats is not None and not callable(extra_feats):
            raise ValueError("from_boxes: with page_annotations extra_feats must be a callable (page_texts, page_boxes) -> arrays "
                             "of the final node lists: arrays per input word cannot line up once figure nodes are added and "
                             "words inside a figure dropped")
        device = torch.device(device)
        sizes = [len(b) for b in page_boxes]
        node_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        bbox = torch.from_numpy(np.concatenate([np.asarray(b, dtype=np.int32).reshape(-1, 4) for b in page_boxes] +
                                               [np.zeros((0, 4), dtype=np.int32)])).to(device)
        cat_map = [-1 if ORIGIN_TO_CONV[c] is None else ORIGIN_TO_CONV[c] for c in range(len(ORIGIN_TO_CONV))] if converted else None
        out_bbox, out_label, out_src, out_off, _, _ = G.label_words(bbox, node_off, ann_box, ann_cat, ann_off, cat_map=cat_map,
                                                                    skip=SKIPPED, figure_cat=FIGURE, n_cat=len(ORIGIN_TO_CONV))
        box_h, lab_h, src_h, off_h = (t.cpu().numpy() for t in (out_bbox, out_label, out_src, out_off))
        texts = page_texts if page_texts is not None else [[""] * n for n in sizes]
        new_boxes, new_labels, new_texts = [], [], []
        for p in range(n_pages):
            o0, o1 = int(off_h[p]), int(off_h[p + 1])
            new_boxes.append(box_h[o0:o1])
            new_labels.append(lab_h[o0:o1].astype(np.int64))
            new_texts.append(["IMAGE!" if s < 0 else texts[p][s - int(node_off[p])] for s in src_h[o0:o1].tolist()])
        if not converted:
            kw = dict(kw)
            kw.setdefault('num_classes', len(ORIGIN_TO_CONV))
        out, keep = cls._from_node_lists(new_boxes, page_sizes, new_texts, new_labels, device, graph_kw['k'], graph_kw['max_dist'],
                                         graph_kw['bidirectional'], graph_kw['range_island'], None, graph_kw['mode'], kw,
                                         extra_feats_fn=extra_feats, repr_embedder=repr_embedder,
                                         scibert_embedder=scibert_embedder)
        keep_h = keep.cpu().numpy()
        for p in range(n_pages):
            o0, o1 = int(off_h[p]), int(off_h[p + 1])
            out.pages[p]['annotations'] = page_annotations[p]
            out.pages[p]['texts'] = [t for t, kept in zip(new_texts[p], keep_h[o0:o1].tolist()) if kept]
        return out

    @classmethod
    def synthetic(cls, n_pages: int, in_feats: int = 13, **kw) -> "PrebuiltPages":
        return cls(S.make_pages(n_pages, in_feats=in_feats), **kw)
