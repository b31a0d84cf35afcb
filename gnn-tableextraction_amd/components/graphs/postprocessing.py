"""From node predictions to page objects: the reference's ``components/graphs/postprocessing*.py``.

Three routes, each an entry point that is public stages in a row -- host packing, ONE launch per ``batch_pages`` pages, host
unpacking -- so that the host stages run (and are tested) without a device, with a CPU oracle in place of the launch:
  ``extract_regions`` = ``region_batches`` -> ``page_regions`` (gte_page_regions[_scored]) -> ``region_tuples``
  ``extract_blocks``  = ``pack_blocks`` -> ``block_vote`` (gte_block_vote) -> ``blocks_to_pages`` (with ``assemble_tables``)
                        and, with ``logits``: -> ``pack_final_blocks`` -> ``block_scores`` (gte_block_scores) -> ``attach_block_scores``
  ``extract_tables``  = ``region_batches`` -> ``page_regions`` -> ``table_batch`` -> ``table_grids`` (gte_table_grid) ->
                        ``tables_from_grids``: what is IN a predicted table -- rows, columns, cells, texts (``table_csv``)
``regions_json`` / ``regions_gt_json`` / ``blocks_json`` / ``blocks_gt_json`` / ``table_structure_json`` lay the results out as the
documents the reference's box-level evaluation reads (``utils.metrics.evaluate_regions``; the block documents hold floats:
``float_boxes=True``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from ... import _lib
from ... import graph as G

# group id of each of the 9 converted classes = the reference's ORIGINAL category value (src/utils/const.py Categories_names):
# other -> no region, text 1, title 2, list 3, figure 5, caption 6, and the three table classes (column header, spanning cell,
# table cell) -> 4, the TABLE category that "has no nodes" upstream.
DEFAULT_CLASS_GROUP = (-1, 1, 2, 3, 5, 6, 4, 4, 4)
GROUP_NAMES = {1: "text", 2: "title", 3: "list", 4: "table", 5: "figure", 6: "caption"}      # lower-case category names
# original category value of each of the 9 converted classes, the table classes NOT merged (column header 7, spanning cell 8,
# table cell 10): the reference's LableModification.revert for to_remove = [4, 9, 11, 12] -- what the block route votes with
DEFAULT_CLASS_CATEGORY = (0, 1, 2, 3, 5, 6, 7, 8, 10)
# the thirteen lower-case category names, in category order: the keys of the block document (write_json)
CATEGORY_NAMES = ("other", "text", "title", "list", "table", "figure", "caption", "table-colh", "table-sp", "table-gcell",
                  "table-tcell", "table-col", "table-row")


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _page_words(data, all_pred, ids, what):
    """Per page of ``ids``: (predictions int64 [n], word boxes int32 [n, 4] from ``data.pages[i]['bboxs']``), equally long."""
    pred = [np.asarray(all_pred[i], dtype=np.int64).reshape(-1) for i in ids]
    boxes = [np.asarray(data.pages[i]['bboxs'], dtype=np.int32).reshape(-1, 4) for i in ids]
    for i, p, b in zip(ids, pred, boxes):
        if p.shape[0] != b.shape[0]:
            raise ValueError(f"{what}: page {i} has {p.shape[0]} predictions and {b.shape[0]} boxes")
    return pred, boxes


# ---- connected regions of one predicted kind ------------------------------------------------------------------------------
class PageRegions(NamedTuple):
    """Result of :func:`page_regions`: ``comp`` per node, then the regions in ascending root order."""
    comp: torch.Tensor        # int32 [n]    smallest node id of the node's region, -1 for nodes outside every region
    root: torch.Tensor        # int64 [R]    the region's smallest node
    page: torch.Tensor        # int64 [R]    page of the batch
    group: torch.Tensor       # int32 [R]    region kind
    box: torch.Tensor         # int32 [R, 4] union of the words' boxes (x0, y0, x1, y1)
    n_words: torch.Tensor     # int32 [R]
    score: Optional[torch.Tensor] = None      # float32 [R]  region confidence (page_regions(..., logits=...) only)


def page_regions(g: G.PageGraph, group: torch.Tensor, bbox: torch.Tensor, logits: Optional[torch.Tensor] = None,
                 class_group=None) -> PageRegions:
    """Regions of a batched page graph (a :class:`PageGraph` from ``graph.batch`` / ``graph.knn_graph_from_boxes``, or a
    :class:`ResidentBatch`): the connected components of ``g`` restricted to nodes of one ``group`` (int [n]; < 0: in no region),
    each with the union of its words' boxes (``bbox`` int [n, 4]) -- one launch of gte_page_regions over ``g.in_csr()`` and the
    batch's page offsets, then a torch compaction of the root rows (``nonzero`` on the counts: plumbing, one synchronisation).

    With ``logits`` (float [n, C], the model's output for the batch) the same launch (gte_page_regions_scored) also gives every
    region a confidence, ``score``: the mean over its words of the softmax mass on the classes of the region's kind,
    ``class_group[c]`` = kind of class c (default :data:`DEFAULT_CLASS_GROUP`; the table ``group`` was derived from)."""
    _lib.require_device(group, "page_regions")
    _lib.require_device(bbox, "page_regions")
    lib, P = _lib.load(), _lib.ptr
    dev = group.device
    n = g.num_nodes()
    group = group.to(torch.int32).contiguous()
    bbox = bbox.to(torch.int32).contiguous()
    if group.numel() != n or tuple(bbox.shape) != (n, 4):
        raise ValueError(f"page_regions: the graph has {n} nodes, group has {group.numel()} entries, bbox is {tuple(bbox.shape)}")
    off_h, node_off = _lib.partition_offsets(_offsets(g.batch_num_nodes_), n, "page_regions: the batch's page offsets", dev)
    pages = off_h.size - 1
    csr = g.in_csr()
    _lib.require_device(csr.indptr, "page_regions")
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    rbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    largest = int(np.diff(off_h).max()) if pages else 0
    score = None
    if logits is None:
        if class_group is not None:
            raise ValueError("page_regions: class_group without logits")
        _lib.check(lib.gte_page_regions(P(csr.indptr), P(csr.indices), P(node_off), pages, n, largest,
                                        P(group), P(bbox), P(comp), P(rbox), P(count), _lib.current_stream()), "gte_page_regions")
    else:
        _lib.require_device(logits, "page_regions")
        logits = logits.to(torch.float32).contiguous()
        table = torch.as_tensor(DEFAULT_CLASS_GROUP if class_group is None else class_group, dtype=torch.int32).to(dev).contiguous()
        if logits.dim() != 2 or logits.shape[0] != n or logits.shape[1] < 1 or table.numel() != logits.shape[1]:
            raise ValueError(f"page_regions: the graph has {n} nodes, logits is {tuple(logits.shape)}, class_group has "
                             f"{table.numel()} entries")
        score = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(lib.gte_page_regions_scored(P(csr.indptr), P(csr.indices), P(node_off), pages, n, largest, P(group), P(bbox),
                                               P(logits), logits.shape[1], P(table), P(comp), P(rbox), P(count), P(score),
                                               _lib.current_stream()), "gte_page_regions_scored")
    root = torch.nonzero(count).flatten()
    page = torch.bucketize(root, node_off[1:].long(), right=True)
    return PageRegions(comp, root, page, group[root], rbox[root], count[root], None if score is None else score[root])


def region_batches(data, all_pred, class_group=None, batch_pages=64, device=None):
    """Stage one of :func:`extract_regions`, a generator: per ``batch_pages`` pages that hold a node, ``(ids, g, group, bbox)`` on
    ``device`` -- ``ids`` the batch's range of page indices, ``g`` the pages' structure-only block-diagonal graph (``graph.batch``),
    ``group`` int32 [n] the kind of every word's predicted class (``class_group``), ``bbox`` int32 [n, 4] the words' boxes."""
    device = _lib.default_device(device)
    sizes = [g.num_nodes() for g in data.graphs]
    if len(all_pred) != len(sizes):
        raise ValueError(f"extract_regions: {len(all_pred)} prediction lists for {len(sizes)} pages")
    table = torch.as_tensor(DEFAULT_CLASS_GROUP if class_group is None else class_group, dtype=torch.int32, device=device)
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
        pred, boxes = (np.concatenate(a) for a in _page_words(data, all_pred, ids, "extract_regions"))
        if pred.shape[0] != bg.num_nodes():
            raise ValueError(f"extract_regions: pages {ids.start}..{ids.stop - 1} have {bg.num_nodes()} nodes, {pred.shape[0]} "
                             f"predictions and boxes")
        yield ids, bg, table[torch.from_numpy(pred).to(device)], torch.from_numpy(boxes).to(device)      # class -> kind: a gather


def region_tuples(reg: PageRegions, n_pages, min_words=1):
    """Stage three of :func:`extract_regions`: the regions of one batch of ``n_pages`` pages as per-page lists of ``(group,
    [x0, y0, x1, y1], n_words)`` -- ``(..., score)`` when ``reg`` carries scores -- in ascending order of the region's first word,
    without the regions of fewer than ``min_words`` words."""
    keep = reg.n_words >= int(min_words)
    rows = [reg.page[keep].tolist(), reg.group[keep].tolist(), reg.box[keep].tolist(), reg.n_words[keep].tolist()]
    if reg.score is not None:
        rows.append(reg.score[keep].tolist())
    out = [[] for _ in range(n_pages)]
    for p, *rest in zip(*rows):
        out[p].append(tuple(rest))
    return out


def extract_regions(data, all_pred, class_group=None, min_words=1, batch_pages=64, device=None, logits=None):
    """Regions of every page from the node predictions: connected components of the page graph among words of one predicted
    kind, each with the union of its words' boxes (``page_regions`` -> gte_page_regions; the reference's ``get_subgraph_bbox`` is
    a stub; its own route, layout blocks labelled by word vote, is ``extract_blocks``).

    ``all_pred``: per-page class ids in ``data.graphs`` order (``test()``'s ``'all_pred'``);
    ``class_group[c]`` = region kind of class c, < 0 for none (default ``DEFAULT_CLASS_GROUP``: the reference's category
    values, the three table classes merged into TABLE = 4); boxes from ``data.pages[i]['bboxs']``.  ``batch_pages`` pages go
    through one launch.  Returns, per page, a list of ``(group, [x0, y0, x1, y1], n_words)`` in ascending order of the region's
    first word; regions of fewer than ``min_words`` words are dropped after the compaction.

    ``logits`` (float [all nodes, n_classes], the pages concatenated in ``data.graphs`` order; a tensor on any device or an array):
    the tuples become ``(group, box, n_words, score)``, score = the region's confidence from the same launch
    (gte_page_regions_scored: the mean over the region's words of the softmax mass on the classes of its kind)."""
    device = _lib.default_device(device)
    table = torch.as_tensor(DEFAULT_CLASS_GROUP if class_group is None else class_group, dtype=torch.int32, device=device)
    node_off = _offsets([g.num_nodes() for g in data.graphs])
    if logits is not None:
        logits = torch.as_tensor(logits)
        if logits.dim() != 2 or logits.shape[0] != int(node_off[-1]):
            raise ValueError(f"extract_regions: logits of shape {tuple(logits.shape)} for {int(node_off[-1])} nodes")
    out = [[] for _ in data.graphs]
    for ids, bg, group, bbox in region_batches(data, all_pred, table, batch_pages, device):
        rows = None if logits is None else logits[int(node_off[ids.start]):int(node_off[ids.stop])].to(device)
        reg = page_regions(bg, group, bbox, logits=rows, class_group=None if rows is None else table)
        out[ids.start:ids.stop] = region_tuples(reg, len(ids), min_words)
    return out


def regions_json(data, regions):
    """``{kind_name: {page_name: {'bboxes': [...], 'scores': [...]}}}``: the layout the reference's box-level evaluation reads
    (postprocessing.py:326-345 write_json -> utils/metrics.py), kind names = the lower-case category names; the score of a
    region is its confidence where its tuple carries one (``extract_regions(..., logits=...)``) and 1.0, as in the reference's
    own writer, otherwise."""
    doc = {name: {} for name in GROUP_NAMES.values()}
    for i, page in enumerate(regions):
        name = str(data.pages[i]['page'])
        for kind, box, *rest in page:
            entry = doc.setdefault(GROUP_NAMES.get(kind, str(kind)), {}).setdefault(name, {'bboxes': [], 'scores': []})
            entry['bboxes'].append([int(v) for v in box])
            entry['scores'].append(float(rest[1]) if len(rest) > 1 else 1.0)
    return doc


def regions_gt_json(data, regions):
    """``{kind_name: {page_name: [box, ...]}}``: regions as the GROUND-TRUTH document of the box-level evaluation
    (``utils.metrics.evaluate_regions``; the layout of the reference's ground-truth JSON, utils/metrics.py ``gt_boxes``)."""
    return {kind: {name: entry['bboxes'] for name, entry in pages.items()} for kind, pages in regions_json(data, regions).items()}


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


def _block_launch_inputs(what, bbox, node_off, block_box, block_off, per_word, per_block):
    """The input check of the two block launches (``what``: "block_vote" / "block_scores"): ``bbox`` int32 [n, 4] and
    ``block_box`` float64 [B, 4] on one device, with the caller's own tensors of one row per word / per block (``per_word`` /
    ``per_block``: name -> tensor; their dtype and rank are the caller's to check, before this); the two host offset sequences
    partition the words and the blocks into the same pages.  ``ValueError`` otherwise; the offsets are the first device access.
    Returns (device, n, B, pages, the two int32 offset tensors on the device, the largest page's word count, its block count)."""
    named = {"bbox": bbox, **per_word, "block_box": block_box, **per_block}
    for t in named.values():
        _lib.require_device(t, what)
    if bbox.dtype != torch.int32 or block_box.dtype != torch.float64:
        raise ValueError(f"{what}: bbox {bbox.dtype} must be int32, block_box {block_box.dtype} float64")
    if bbox.dim() != 2 or bbox.shape[1] != 4 or block_box.dim() != 2 or block_box.shape[1] != 4 \
            or any(t.shape[0] != bbox.shape[0] for t in per_word.values()) \
            or any(t.shape[0] != block_box.shape[0] for t in per_block.values()):
        raise ValueError(f"{what}: " + ", ".join(f"{name} is {tuple(t.shape)}" for name, t in named.items()))
    dev = bbox.device
    if any(t.device != dev for t in named.values()):
        raise ValueError(f"{what}: {', '.join(named)} live on different devices")
    n, nb = bbox.shape[0], block_box.shape[0]
    no, d_no = _lib.partition_offsets(node_off, n, f"{what}: the word offsets", dev)
    bo, d_bo = _lib.partition_offsets(block_off, nb, f"{what}: the block offsets", dev)
    if no.size != bo.size:
        raise ValueError(f"{what}: offsets of {no.size - 1} / {bo.size - 1} pages do not partition the words and the blocks")
    pages = no.size - 1
    return dev, n, nb, pages, d_no, d_bo, int(np.diff(no).max()) if pages else 0, int(np.diff(bo).max()) if pages else 0


class BlockVote(NamedTuple):
    """Result of :func:`block_vote`."""
    word_block: torch.Tensor  # int32 [n]        global index of the word's block, -1 for a word outside every block
    votes: torch.Tensor       # int32 [B, n_cat] the blocks' counters
    label: torch.Tensor       # int32 [B]        the lowest category with the largest count (0 for a block without votes)


def block_vote(bbox: torch.Tensor, node_off, word_cat: torch.Tensor, block_box: torch.Tensor, block_off, n_cat: int = 13,
               double_cat: int = 2) -> BlockVote:
    """Layout blocks labelled by the vote of their words (gte_block_vote, one launch; the words x blocks loop of the reference's
    ``get_objects_bboxs``, postprocessing_2.py:240-258).

    ``bbox`` int32 [n, 4] word boxes and ``word_cat`` int32 [n] their categories (the reference's ORIGINAL category values:
    :data:`DEFAULT_CLASS_CATEGORY` of the predicted class), pages concatenated; ``block_box`` float64 [B, 4] the pages' layout
    blocks ALREADY divided by the scale factor on the host; ``node_off`` / ``block_off`` host sequences [pages + 1].  A word goes
    to the first block of its page that its rectangle meets (closed test, corners normalised) and adds 2 to the block's counter
    of its category if that is ``double_cat`` (TITLE; -1: none), else 1; a category outside ``[0, n_cat)`` casts no vote.
    Raises ``ValueError`` on shapes, dtypes or offsets that do not fit, ``GteError`` when a page has more than
    ``gte_block_vote_max_page_blocks()`` blocks.  No synchronisation."""
    lib, P = _lib.load(), _lib.ptr
    if word_cat.dtype != torch.int32 or word_cat.dim() != 1:
        raise ValueError(f"block_vote: word_cat {word_cat.dtype} {tuple(word_cat.shape)} must be int32 [n]")
    dev, n, nb, pages, d_no, d_bo, _, max_blocks = _block_launch_inputs("block_vote", bbox, node_off, block_box, block_off,
                                                                        {"word_cat": word_cat}, {})
    if not 1 <= int(n_cat) <= lib.gte_block_vote_max_categories():
        raise ValueError(f"block_vote: n_cat = {n_cat} outside 1 .. {lib.gte_block_vote_max_categories()}")
    bbox, word_cat, block_box = bbox.contiguous(), word_cat.contiguous(), block_box.contiguous()
    word_block = torch.empty(n, dtype=torch.int32, device=dev)
    votes = torch.empty((nb, int(n_cat)), dtype=torch.int32, device=dev)
    label = torch.empty(nb, dtype=torch.int32, device=dev)
    _lib.check(lib.gte_block_vote(P(bbox), P(d_no), P(word_cat), P(block_box), P(d_bo), pages, n, nb, max_blocks, int(n_cat),
                                  int(double_cat), P(word_block), P(votes), P(label), _lib.current_stream()), "gte_block_vote")
    return BlockVote(word_block, votes, label)


class BlockBatch(NamedTuple):
    """One launch's worth of :func:`pack_blocks`: host arrays, the pages of ``ids`` concatenated."""
    ids: range                # the batch's page indices
    bbox: np.ndarray          # int32 [n, 4]   word boxes
    node_off: np.ndarray      # int64 [pages + 1]
    word_cat: np.ndarray      # int32 [n]      the reference's category of every word's predicted class
    block_box: np.ndarray     # float64 [B, 4] layout blocks divided by the scale (bit for bit the reference's b / sf)
    block_off: np.ndarray     # int64 [pages + 1]
    page_blocks: list         # per page float64 [blocks, 4]: the blocks as delivered (what the assembly works on)
    n_cat: int                # categories to count: the thirteen, or more where ``class_category`` names a higher value


def pack_blocks(data, all_pred, class_category=None, blocks=None, images=None, scale=0.36, batch_pages=64):
    """Stage one of :func:`extract_blocks`: every argument check (``ValueError``; no device is touched) and the packing, a
    :class:`BlockBatch` per ``batch_pages`` pages.  ``images`` is only checked for its length."""
    n_pages = len(data.graphs)
    if len(all_pred) != n_pages:
        raise ValueError(f"extract_blocks: {len(all_pred)} prediction lists for {n_pages} pages")
    for what, seq in (("block", blocks), ("image", images)):
        if seq is not None and len(seq) != n_pages:
            raise ValueError(f"extract_blocks: {len(seq)} {what} lists for {n_pages} pages")
    if not float(scale) > 0.0:
        raise ValueError(f"extract_blocks: scale = {scale}")
    table = np.asarray(DEFAULT_CLASS_CATEGORY if class_category is None else class_category, dtype=np.int64).reshape(-1)
    n_cat = max(len(CATEGORY_NAMES), int(table.max()) + 1 if table.size else 0)
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
    out = []
    bp = max(1, int(batch_pages))
    for b0 in range(0, n_pages, bp):
        ids = range(b0, min(b0 + bp, n_pages))
        pred, boxes = _page_words(data, all_pred, ids, "extract_blocks")
        for i, p in zip(ids, pred):
            if p.size and (p.min() < 0 or p.max() >= table.size):
                raise ValueError(f"extract_blocks: page {i} holds a class outside the {table.size} of class_category")
        mine = [page_blocks[i] for i in ids]
        out.append(BlockBatch(ids, np.concatenate(boxes), _offsets([b.shape[0] for b in boxes]), table[np.concatenate(pred)].astype(np.int32),
                              np.concatenate(mine) / float(scale), _offsets([b.shape[0] for b in mine]), mine, n_cat))
    return out


def blocks_to_pages(data, batch: BlockBatch, word_block, votes, label, images=None, scale=0.36, rescale=True):
    """Stage three of :func:`extract_blocks`: a batch's vote (host arrays as :class:`BlockVote` names them: ``word_block`` [n]
    global or -1, ``votes`` [B, n_cat], ``label`` [B]) -> the batch's per-page dicts: ``assemble_tables`` on the unscaled blocks
    and their voted labels, the figure rule on the page's images, the rescale, the page-local word index."""
    out, scale = [], float(scale)
    for k, i in enumerate(batch.ids):
        n0, n1, k0, k1 = int(batch.node_off[k]), int(batch.node_off[k + 1]), int(batch.block_off[k]), int(batch.block_off[k + 1])
        voted = [int(v) for v in label[k0:k1]]
        new_blocks, new_labels, headers = assemble_tables(batch.page_blocks[k].tolist(), voted)
        for img in (images[i] if images is not None else data.pages[i].get('images', ())):
            box = img['bbox'] if isinstance(img, dict) else img
            if box[3] - box[1] > 10:
                new_blocks.append([int(v) for v in box])
                new_labels.append(_FIGURE)
        if rescale:
            new_blocks = [[v / scale for v in b] for b in new_blocks]
        wb = np.asarray(word_block[n0:n1], dtype=np.int64)
        out.append({'blocks': new_blocks, 'labels': new_labels, 'voted_labels': voted, 'headers': headers,
                    'word_block': np.where(wb >= 0, wb - k0, -1).tolist(), 'votes': np.asarray(votes[k0:k1]).tolist()})
    return out


class BlockScores(NamedTuple):
    """Result of :func:`block_scores`."""
    score: torch.Tensor       # float32 [B]  mean over the words that meet the block of their softmax mass on the block's classes; 1.0 without words
    n_words: torch.Tensor     # int32 [B]    the words that meet the block


def category_class_masks(class_category=None, n_cat=13):
    """uint32 [n_cat]: bit c of mask k is set when ``class_category[c] == k`` (default :data:`DEFAULT_CLASS_CATEGORY`) -- the
    classes whose softmax mass counts for a block of category k.  TABLE (4) also takes the classes of the column-header,
    spanning-cell and table-cell categories (7, 8, 10): ``assemble_tables`` merges those blocks into tables and relabels the
    remaining cell blocks, so a final TABLE block is made of words of these classes.  Host only."""
    table = np.asarray(DEFAULT_CLASS_CATEGORY if class_category is None else class_category, dtype=np.int64).reshape(-1)
    if not 1 <= table.size <= 32 or int(n_cat) < 1:
        raise ValueError(f"category_class_masks: {table.size} classes, n_cat = {n_cat}")
    masks = np.zeros(int(n_cat), dtype=np.uint32)
    for c, k in enumerate(table.tolist()):
        if 0 <= k < masks.size:
            masks[k] |= np.uint32(1 << c)
        if k in (_COLH, _SP, _TCELL) and _TABLE < masks.size:
            masks[_TABLE] |= np.uint32(1 << c)
    return masks


def block_scores(bbox: torch.Tensor, node_off, logits: torch.Tensor, block_box: torch.Tensor, block_off, block_cat: torch.Tensor,
                 cat_classes) -> BlockScores:
    """Confidence of final layout blocks (gte_block_scores, one launch).

    ``bbox`` int32 [n, 4] word boxes and ``logits`` float32 [n, C] their logit rows (C <= 16; a row stride is passed on), pages
    concatenated; ``block_box`` float64 [B, 4] the pages' FINAL blocks in word coordinates, ``block_cat`` int32 [B] their
    categories; ``cat_classes`` [n_cat] host sequence of class masks (:func:`category_class_masks`); ``node_off`` / ``block_off``
    host sequences [pages + 1].  A word counts in EVERY block of its page that its rectangle meets (``block_vote``'s closed
    test); ``score`` = the mean over those words of the softmax mass on the classes of the block's category (2^-19 fixed point:
    within 2^-18 of the mean; a row with a non-finite logit adds 0), 1.0 for a block no word meets.  Raises ``ValueError`` on
    shapes, dtypes or offsets that do not fit, ``GteError`` when a page exceeds ``gte_block_scores_max_page_blocks()`` blocks
    or ``gte_block_scores_max_page_words()`` words.  No synchronisation."""
    lib, P = _lib.load(), _lib.ptr
    if logits.dtype != torch.float32 or logits.dim() != 2 or block_cat.dtype != torch.int32 or block_cat.dim() != 1:
        raise ValueError(f"block_scores: logits {logits.dtype} {tuple(logits.shape)} must be float32 [n, C], block_cat {block_cat.dtype} "
                         f"{tuple(block_cat.shape)} int32 [B]")
    masks = np.ascontiguousarray(np.asarray(cat_classes, dtype=np.uint32).reshape(-1))
    if not 1 <= logits.shape[1] <= lib.gte_block_scores_max_classes():
        raise ValueError(f"block_scores: {logits.shape[1]} classes outside 1 .. {lib.gte_block_scores_max_classes()}")
    if not 1 <= masks.size <= lib.gte_block_scores_max_categories():
        raise ValueError(f"block_scores: {masks.size} class masks outside 1 .. {lib.gte_block_scores_max_categories()}")
    dev, n, nb, pages, d_no, d_bo, max_words, max_blocks = _block_launch_inputs(
        "block_scores", bbox, node_off, block_box, block_off, {"logits": logits}, {"block_cat": block_cat})
    if logits.stride(1) != 1 and logits.shape[0] > 0:
        logits = logits.contiguous()
    ld = int(logits.stride(0)) if logits.shape[0] > 1 else int(logits.shape[1])
    bbox, block_box, block_cat = bbox.contiguous(), block_box.contiguous(), block_cat.contiguous()
    d_masks = torch.from_numpy(masks.view(np.int32)).to(dev)
    score = torch.empty(nb, dtype=torch.float32, device=dev)
    n_words = torch.empty(nb, dtype=torch.int32, device=dev)
    _lib.check(lib.gte_block_scores(P(bbox), P(d_no), P(logits), ld, int(logits.shape[1]), P(block_box), P(d_bo), P(block_cat),
                                    P(d_masks), masks.size, pages, n, nb, max_words, max_blocks, P(score), P(n_words),
                                    _lib.current_stream()), "gte_block_scores")
    return BlockScores(score, n_words)


class FinalBlocks(NamedTuple):
    """One launch's worth of :func:`pack_final_blocks`: host arrays, the batch's pages concatenated."""
    block_box: np.ndarray     # float64 [B, 4] the final blocks in word coordinates (the unscaled block / scale: one float64 division)
    block_off: np.ndarray     # int64 [pages + 1]
    block_cat: np.ndarray     # int32 [B]      their categories


def pack_final_blocks(pages, scale=0.36, rescaled=True) -> FinalBlocks:
    """Stage four of :func:`extract_blocks` with ``logits``: the ``'blocks'`` / ``'labels'`` of a batch's page dicts
    (``blocks_to_pages``) as the arguments of :func:`block_scores`.  The blocks enter as they stand before the rescale divided by
    ``scale`` -- the operation ``pack_blocks`` applies to the input blocks; ``rescaled`` says that ``blocks_to_pages`` has done
    that division already (``rescale=True``: the boxes are taken bit for bit)."""
    boxes = [np.asarray(p['blocks'], dtype=np.float64).reshape(-1, 4) for p in pages]
    cats = [np.asarray(p['labels'], dtype=np.int32).reshape(-1) for p in pages]
    box = np.concatenate(boxes) if boxes else np.zeros((0, 4))
    return FinalBlocks(box if rescaled else box / float(scale), _offsets([b.shape[0] for b in boxes]),
                       np.concatenate(cats) if cats else np.zeros(0, dtype=np.int32))


def attach_block_scores(pages, final: FinalBlocks, score, n_words):
    """Stage six: the launch's host arrays (``score`` [B], ``n_words`` [B]) onto the batch's page dicts as ``'scores'`` (floats)
    and ``'n_words'`` (ints) per final block.  Returns ``pages``."""
    score, n_words = np.asarray(score, dtype=np.float64).reshape(-1), np.asarray(n_words, dtype=np.int64).reshape(-1)
    for k, p in enumerate(pages):
        k0, k1 = int(final.block_off[k]), int(final.block_off[k + 1])
        p['scores'], p['n_words'] = score[k0:k1].tolist(), n_words[k0:k1].tolist()
    return pages


def extract_blocks(data, all_pred, class_category=None, blocks=None, images=None, scale=0.36, rescale=True, batch_pages=64,
                   device=None, logits=None):
    """Page objects by the reference's own route (``get_objects_bboxs``, postprocessing_2.py:197-309): the layout blocks that a
    PDF text extractor delivers for every page are labelled by the vote of the words inside them (``block_vote`` ->
    gte_block_vote: ONE launch per ``batch_pages`` pages, in place of the reference's words x blocks loop in Python), the
    column-header, spanning-cell and table-cell blocks are assembled into tables (``assemble_tables``, on the host, per page, on
    the unscaled blocks), and the page's images become FIGURE blocks.

    ``all_pred``: per-page class ids in ``data.graphs`` order (``test()``'s ``'all_pred'``); ``class_category[c]`` = the
    reference's original category value of class c (default ``DEFAULT_CLASS_CATEGORY``, its ``LableModification.revert``);
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

    ``logits`` (device tensor float [all nodes, C <= 16], the pages concatenated in ``data.graphs`` order: what
    ``predict_resident(return_logits=True)`` returns): every page dict gains ``'scores'`` and ``'n_words'`` per FINAL block, one
    more launch per batch (``pack_final_blocks`` -> ``block_scores`` -> ``attach_block_scores``): the mean over the words that
    meet the block -- every block they meet -- of the softmax mass on the classes of the block's category
    (``category_class_masks(class_category)``), 1.0 (the reference's constant) for a block no word meets.  Without ``logits``
    nothing changes.  The float-valued document of the result (``blocks_json``) is scored by
    ``utils.metrics.evaluate_regions(..., float_boxes=True)``.

    Out of scope: obtaining the blocks from a PDF (the caller's extractor)."""
    batches = pack_blocks(data, all_pred, class_category, blocks, images, scale, batch_pages)
    if logits is not None:
        total = sum(int(b.node_off[-1]) for b in batches)
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] != total:
            raise ValueError(f"extract_blocks: logits must be a tensor [{total} nodes, classes], got "
                             f"{tuple(logits.shape) if hasattr(logits, 'shape') else type(logits).__name__}")
    device = _lib.default_device(device)
    if logits is not None:
        logits = logits.to(device=device, dtype=torch.float32)
    out, first = [], 0
    for b in batches:
        d_bbox = torch.from_numpy(b.bbox).to(device)
        vote = block_vote(d_bbox, b.node_off, torch.from_numpy(b.word_cat).to(device),
                          torch.from_numpy(b.block_box).to(device), b.block_off, n_cat=b.n_cat, double_cat=2)
        pages = blocks_to_pages(data, b, *(t.cpu().numpy() for t in vote), images=images, scale=scale, rescale=rescale)
        if logits is not None:
            final = pack_final_blocks(pages, scale, rescaled=rescale)
            got = block_scores(d_bbox, b.node_off, logits[first:first + int(b.node_off[-1])], torch.from_numpy(final.block_box).to(device),
                               final.block_off, torch.from_numpy(final.block_cat).to(device), category_class_masks(class_category, b.n_cat))
            attach_block_scores(pages, final, *(t.cpu().numpy() for t in got))
        first += int(b.node_off[-1])
        out += pages
    return out


def blocks_json(data, result):
    """``{kind_name: {page_name: {'bboxes': [...], 'scores': [...]}}}`` of ``extract_blocks``' result: the layout of the
    reference's ``write_json`` (postprocessing_2.py:328-348, its ``ours_bboxs.json``) -- all thirteen lower-case category names
    as keys, a page only under the kinds it has, coordinates as floats; a block's score is its confidence where the page carries
    ``'scores'`` (``extract_blocks(..., logits=...)``) and 1.0, the reference's constant, otherwise."""
    doc = {name: {} for name in CATEGORY_NAMES}
    for i, page in enumerate(result):
        name = str(data.pages[i]['page'])
        scores = page.get('scores')
        for j, (box, label) in enumerate(zip(page['blocks'], page['labels'])):
            entry = doc[CATEGORY_NAMES[label]].setdefault(name, {'bboxes': [], 'scores': []})
            entry['bboxes'].append([float(v) for v in box])
            entry['scores'].append(1.0 if scores is None else float(scores[j]))
    return doc


def blocks_gt_json(data):
    """``{kind_name: {page_name: [[x0, y0, x1, y1], ...]}}``: the GROUND-TRUTH document of the block route's evaluation from
    ``data.pages[i]['annotations']``, rows ``[x0, y0, x1, y1, category]`` -- what the reference's ``get_groundtruth_bboxs``
    (models/evaluate.py:26-62) reads from ``test.json``, here kept per category (its lower-case name, in category order; only the
    categories that occur).  A page without the key or a row that is no five numbers with a category in 0 .. 12 raises
    ``ValueError``."""
    found = {}
    for i, page in enumerate(data.pages):
        if 'annotations' not in page:
            raise ValueError(f"blocks_gt_json: page {i} ({page.get('page')}) carries no 'annotations'")
        name = str(page['page'])
        for row in page['annotations']:
            if len(row) != 5 or int(row[4]) != row[4] or not 0 <= int(row[4]) < len(CATEGORY_NAMES):
                raise ValueError(f"blocks_gt_json: page {i} ({name}): {row!r} is no [x0, y0, x1, y1, category]")
            found.setdefault(int(row[4]), {}).setdefault(name, []).append([float(v) for v in row[:4]])
    return {CATEGORY_NAMES[c]: found[c] for c in sorted(found)}


# ---- the grid of a predicted table: rows, columns, cells (no reference counterpart; the projection profile on the device) --------
DEFAULT_COL_ROLES = (_COLH, _TCELL)                       # words that build the column profile: a spanning cell would bridge columns
DEFAULT_ROW_ROLES = (_COLH, _SP, _TCELL)


class TableGrids(NamedTuple):
    """Result of :func:`table_grids` (gte_table_grid; the rule: include/gte.h)."""
    cell: torch.Tensor          # int32 [n, 4]  (r0, r1, c0, c1): the word's span in row / column bands; -1 on an axis it meets no band of
    cell_box: torch.Tensor      # int32 [n, 4]  (start of column c0, start of row r0, end of column c1, end of row r1); 0 on such an axis
    table_shape: torch.Tensor   # int32 [T, 2]  (n_rows, n_cols)
    table_box: torch.Tensor     # int32 [T, 4]  union of the table's words
    table_words: torch.Tensor   # int32 [T]
    table_status: torch.Tensor  # int32 [T]     0 fine, 1 no word, 2 too large for a grid / bad gap, 3 bad page


class TableBatch(NamedTuple):
    """Result of :func:`table_batch`: the tables of one batch of pages, in ascending root order."""
    table: torch.Tensor         # int32 [n]     root of the word's TABLE region, -1 for every other word
    root: torch.Tensor          # int32 [T]
    page: torch.Tensor          # int32 [T]     page of the batch
    gap: torch.Tensor           # int32 [T, 2]  (gap_x, gap_y)
    score: Optional[torch.Tensor] = None      # float32 [T]  the regions' confidences, where the regions carry them


def role_mask(roles) -> int:
    """Bit mask of a sequence of categories 0 .. 31 (an int is taken as the mask itself)."""
    if isinstance(roles, (int, np.integer)):
        mask = int(roles)
    else:
        roles = [int(r) for r in roles]
        if any(not 0 <= r < 32 for r in roles):
            raise ValueError(f"table grids: the roles {roles} must lie in 0 .. 31")
        mask = sum({1 << r for r in roles})
    if not 0 <= mask < 1 << 32:
        raise ValueError(f"table grids: role mask {mask} does not fit 32 bits")
    return mask


def table_grids(table: torch.Tensor, bbox: torch.Tensor, role: torch.Tensor, node_off, table_root: torch.Tensor,
                table_page: torch.Tensor, table_gap: torch.Tensor, col_roles=DEFAULT_COL_ROLES, row_roles=DEFAULT_ROW_ROLES) -> TableGrids:
    """Rows, columns and cells of the listed tables (gte_table_grid: ONE launch, one workgroup per table; the rule is the contract
    text in include/gte.h).  ``table`` int32 [n] the id of every word's table (< 0: none), ``bbox`` int32 [n, 4], ``role`` int32 [n]
    the words' categories, pages concatenated; ``node_off`` host sequence [pages + 1]; ``table_root`` / ``table_page`` int32 [T]
    and ``table_gap`` int32 [T, 2] on the device (:func:`table_batch` makes them); ``col_roles`` / ``row_roles``: the categories
    (or a bit mask) whose words build the column / row profile.  ``cell`` is pre-filled with -1 and ``cell_box`` with 0: words of
    no listed table keep that.  ``ValueError`` on shapes, dtypes or offsets that do not fit.  No synchronisation."""
    lib, P = _lib.load(), _lib.ptr
    named = {"table": table, "bbox": bbox, "role": role, "table_root": table_root, "table_page": table_page, "table_gap": table_gap}
    for t in named.values():
        _lib.require_device(t, "table_grids")
    dev = bbox.device
    if any(t.dtype != torch.int32 for t in named.values()) or any(t.device != dev for t in named.values()):
        raise ValueError("table_grids: " + ", ".join(f"{k} {t.dtype} on {t.device}" for k, t in named.items()) + " must be int32 on one device")
    n, nt = bbox.shape[0], table_root.numel()
    if bbox.dim() != 2 or bbox.shape[1] != 4 or tuple(table.shape) != (n,) or tuple(role.shape) != (n,) or table_root.dim() != 1 \
            or tuple(table_page.shape) != (nt,) or tuple(table_gap.shape) != (nt, 2):
        raise ValueError("table_grids: " + ", ".join(f"{k} is {tuple(t.shape)}" for k, t in named.items()))
    off_h, d_off = _lib.partition_offsets(node_off, n, "table_grids: the word offsets", dev)
    cols, rows = role_mask(col_roles), role_mask(row_roles)
    cell = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
    cell_box = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    shape = torch.empty((nt, 2), dtype=torch.int32, device=dev)
    box = torch.empty((nt, 4), dtype=torch.int32, device=dev)
    words = torch.empty(nt, dtype=torch.int32, device=dev)
    status = torch.empty(nt, dtype=torch.int32, device=dev)
    _lib.check(lib.gte_table_grid(P(bbox.contiguous()), P(d_off), off_h.size - 1, n, P(table.contiguous()), P(role.contiguous()),
                                  P(table_root.contiguous()), P(table_page.contiguous()), P(table_gap.contiguous()), nt, cols, rows,
                                  P(cell), P(cell_box), P(shape), P(box), P(words), P(status), _lib.current_stream()), "gte_table_grid")
    return TableGrids(cell, cell_box, shape, box, words, status)


def table_batch(reg: PageRegions, bbox: torch.Tensor, role: torch.Tensor, node_off, col_gap='auto', row_gap=0, col_gap_em=0.5,
                table_group=_TABLE, min_words=1) -> TableBatch:
    """The TABLE regions of a batch as the arguments of :func:`table_grids` (torch plumbing, no launch of the library's): the
    regions of kind ``table_group`` with at least ``min_words`` words, in ascending root order -- one to one, in order, the
    kind-4 tuples of ``region_tuples`` -- their pages, ``table`` (``reg.comp`` for the words of these regions, -1 elsewhere) and
    the gaps.  ``bbox`` int [n, 4], ``role`` int [n] (checked against ``node_off``, the host offsets of the batch's pages).

    A gap is an int, used as it is, or ``'auto'``: ``floor(col_gap_em * (sum / count))`` over the table's words of their heights
    ``|y1 - y0|`` -- the sums exact integers, the quotient and the product in float64 -- clamped to ``0 .. gte_table_grid_max_gap()``.
    Half a line height is meant to lie between the space inside a cell (a word space, about a quarter of the height) and the
    gutter between two columns.  THE DEFAULT IS NOT VALIDATED ON ANY REAL PAGE: none has been seen; only synthetic tables
    (tests/table_grid_ref.py) come back exactly under it.  Rows use gap 0 by default: lines of one row share their pixels."""
    lib = _lib.load()
    dev = reg.comp.device
    n = reg.comp.numel()
    off = np.asarray(node_off, dtype=np.int64).reshape(-1)
    if tuple(bbox.shape) != (n, 4) or role.numel() != n or off.size < 1 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError(f"table_batch: {n} nodes, bbox is {tuple(bbox.shape)}, role has {role.numel()} entries, node_off ends at "
                         f"{int(off[-1]) if off.size else None}")
    keep = (reg.group == int(table_group)) & (reg.n_words >= int(min_words))
    root = reg.root[keep]
    nt = root.numel()
    is_root = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    is_root[root] = True
    comp = reg.comp.long()
    table = torch.where(is_root[comp.clamp(min=0)] & (comp >= 0), reg.comp, torch.full_like(reg.comp, -1))
    max_gap = lib.gte_table_grid_max_gap()
    gaps = []
    for what, g in (("col_gap", col_gap), ("row_gap", row_gap)):
        if isinstance(g, str):
            if g != 'auto':
                raise ValueError(f"table_batch: {what} = {g!r} is neither an int nor 'auto'")
            member = table >= 0
            height = (bbox[:, 3].long() - bbox[:, 1].long()).abs()
            total = torch.zeros(n + 1, dtype=torch.int64, device=dev).index_add_(0, table[member].long(), height[member])
            mean = total[root].double() / reg.n_words[keep].double()
            gaps.append(torch.floor(float(col_gap_em) * mean).clamp(0, max_gap).to(torch.int32))
        else:
            gaps.append(torch.full((nt,), int(g), dtype=torch.int32, device=dev))
    return TableBatch(table.to(torch.int32), root.to(torch.int32), reg.page[keep].to(torch.int32), torch.stack(gaps, dim=1).contiguous(),
                      None if reg.score is None else reg.score[keep])


def tables_from_grids(table, bbox, role, node_off, table_root, table_page, grids, texts, col_roles=DEFAULT_COL_ROLES,
                      row_roles=DEFAULT_ROW_ROLES, score=None, header_role=_COLH):
    """Stage five of :func:`extract_tables`: pure host code on numpy arrays (no device is touched) -- the launch's arguments and
    its six outputs (``grids``: a :class:`TableGrids` of host arrays, or of a CPU oracle's) as per-page lists of tables, in
    ascending root order.  ``texts``: per page the words' texts (None: every text is ``''``).  A table is a dict:

    ``'box'``, ``'n_rows'``, ``'n_cols'``, ``'n_words'``, ``'status'`` (gte_table_grid's; a table with a status other than 0 has
    no bands and all its words are ``'loose'``), ``'score'`` when ``score`` [T] is given;
    ``'rows'`` / ``'cols'``: ``[lo, hi]`` per band;  ``'header_rows'``: the rows where strictly more than half of the row-profile
    words are column headers (``header_role``);
    ``'cells'``: one entry per distinct span ``(r0, r1, c0, c1)``, ordered by ``(r0, c0, r1, c1)`` -- ``'row': [r0, r1]``,
    ``'col': [c0, c1]``, ``'role'`` (the lowest category with the most words), ``'words'`` (page-local indices ordered by
    ``(y_lo, x_lo, index)``), ``'text'`` (their texts joined by one space), ``'box'`` (the span's ``cell_box``);
    ``'loose'``: the words with -1 on an axis (page-local indices, ascending);
    ``'grid'``: ``n_rows`` x ``n_cols`` strings, a cell's text at ``(r0, c0)`` and ``''`` elsewhere; cells that share a position
    are joined by one space in cell order."""
    table, role = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (table, role))
    bbox = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    node_off = np.asarray(node_off, dtype=np.int64).reshape(-1)
    table_root, table_page = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (table_root, table_page))
    cell, cell_box, shape, tbox, n_words, status = (np.asarray(a, dtype=np.int64) for a in grids)
    cols, rows = role_mask(col_roles), role_mask(row_roles)
    in_mask = lambda r, mask: (r >= 0) & (r < 32) & (((mask >> np.clip(r, 0, 31)) & 1) == 1)
    lo_y, lo_x = np.minimum(bbox[:, 1], bbox[:, 3]), np.minimum(bbox[:, 0], bbox[:, 2])
    out = [[] for _ in range(node_off.size - 1)]
    for t in np.argsort(table_root, kind='stable'):
        p = int(table_page[t])
        if not 0 <= p < len(out):
            continue
        n0, n1 = int(node_off[p]), int(node_off[p + 1])
        v = n0 + np.nonzero(table[n0:n1] == table_root[t])[0] if table_root[t] >= 0 else np.zeros(0, dtype=np.int64)
        words_text = (lambda i: '') if texts is None or texts[p] is None else (lambda i, tx=texts[p]: str(tx[i - n0]))
        nr, nc = (int(s) for s in shape[t]) if status[t] == 0 else (0, 0)
        entry = {'box': [int(c) for c in tbox[t]], 'n_rows': nr, 'n_cols': nc, 'n_words': int(n_words[t]), 'status': int(status[t])}
        if score is not None:
            entry['score'] = float(score[t])
        row_band, col_band = [None] * nr, [None] * nc
        head, total = [0] * nr, [0] * nr
        if status[t] == 0:
            for i in v[in_mask(role[v], cols)]:           # a profile word sits in one band and carries its extent
                col_band[cell[i, 2]] = [int(cell_box[i, 0]), int(cell_box[i, 2])]
            for i in v[in_mask(role[v], rows)]:
                row_band[cell[i, 0]] = [int(cell_box[i, 1]), int(cell_box[i, 3])]
                total[cell[i, 0]] += 1
                head[cell[i, 0]] += int(role[i] == header_role)
        entry['rows'], entry['cols'] = row_band, col_band
        entry['header_rows'] = [r for r in range(nr) if 2 * head[r] > total[r]]
        placed = v[(cell[v] >= 0).all(axis=1)] if status[t] == 0 else v[:0]
        entry['loose'] = sorted(int(i - n0) for i in set(v.tolist()) - set(placed.tolist()))
        by_span = {}
        for i in sorted(placed.tolist(), key=lambda i: (lo_y[i], lo_x[i], i)):
            by_span.setdefault((int(cell[i, 0]), int(cell[i, 2]), int(cell[i, 1]), int(cell[i, 3])), []).append(i)
        grid = [['' for _ in range(nc)] for _ in range(nr)]
        cells = []
        for (r0, c0, r1, c1), ids in sorted(by_span.items()):
            values, counts = np.unique(role[ids], return_counts=True)      # ascending: the first maximum is the lowest category
            text = ' '.join(words_text(i) for i in ids)
            cells.append({'row': [r0, r1], 'col': [c0, c1], 'role': int(values[counts.argmax()]),
                          'words': [int(i - n0) for i in ids], 'text': text, 'box': [int(c) for c in cell_box[ids[0]]]})
            grid[r0][c0] = text if not grid[r0][c0] else grid[r0][c0] + ' ' + text
        entry['cells'], entry['grid'] = cells, grid
        out[p].append(entry)
    return out


def extract_tables(data, all_pred, class_category=None, col_gap='auto', row_gap=0, col_gap_em=0.5, col_roles=DEFAULT_COL_ROLES,
                   row_roles=DEFAULT_ROW_ROLES, min_words=1, batch_pages=64, device=None, logits=None):
    """The grid of every predicted table: ``region_batches`` -> ``page_regions`` -> ``table_batch`` -> ``table_grids``
    (gte_table_grid, ONE launch per ``batch_pages`` pages) -> ``tables_from_grids``.  The tables of a page correspond one to one,
    in order, to the kind-4 tuples of ``extract_regions`` for the same arguments: a table is a connected region of words whose
    predicted class is column header, spanning cell or table cell.  Inside it the words of the ``col_roles`` categories build the
    column profile (default: headers and table cells -- a spanning cell would bridge the columns it spans; it still receives its
    span ``'col': [c0, c1]``) and those of ``row_roles`` the row profile; ``role`` of a word is the original category of its
    predicted class (``class_category``, default ``DEFAULT_CLASS_CATEGORY``).  Two profile words share a column when the free
    space between them is at most ``col_gap`` pixels, ``'auto'``: ``floor(col_gap_em * mean word height of the table)``
    (``table_batch``: NOT VALIDATED ON ANY REAL PAGE), and a row when it is at most ``row_gap``.

    Texts from ``data.pages[i]['texts']`` (a page without them gets ``''``), boxes from ``data.pages[i]['bboxs']``.  ``logits``
    as for ``extract_regions``: every table gains ``'score'``, its region's confidence.  Returns per page a list of table dicts
    (``tables_from_grids``).  A table wider or higher than ``gte_table_grid_max_extent()`` pixels comes back with ``'status'`` 2
    and no grid."""
    device = _lib.default_device(device)
    cat = np.asarray(DEFAULT_CLASS_CATEGORY if class_category is None else class_category, dtype=np.int64).reshape(-1)
    group = [(_TABLE if int(k) in (_COLH, _SP, _TCELL) else (int(k) if int(k) in GROUP_NAMES and int(k) != _TABLE else -1)) for k in cat]
    d_cat = torch.from_numpy(cat.astype(np.int32)).to(device)
    node_off = _offsets([g.num_nodes() for g in data.graphs])
    if logits is not None:
        logits = torch.as_tensor(logits)
        if logits.dim() != 2 or logits.shape[0] != int(node_off[-1]):
            raise ValueError(f"extract_tables: logits of shape {tuple(logits.shape)} for {int(node_off[-1])} nodes")
    for i, p in enumerate(all_pred):                      # on the host, before a class id becomes a device index
        p = np.asarray(p, dtype=np.int64).reshape(-1)
        if p.size and (p.min() < 0 or p.max() >= cat.size):
            raise ValueError(f"extract_tables: page {i} holds a class outside the {cat.size} of class_category")
    d_group = torch.as_tensor(group, dtype=torch.int32, device=device)
    out = [[] for _ in data.graphs]
    for ids, bg, grp, bbox in region_batches(data, all_pred, group, batch_pages, device):
        rows = None if logits is None else logits[int(node_off[ids.start]):int(node_off[ids.stop])].to(device)
        reg = page_regions(bg, grp, bbox, logits=rows, class_group=None if rows is None else d_group)
        pred = np.concatenate(_page_words(data, all_pred, ids, "extract_tables")[0])
        role = d_cat[torch.from_numpy(pred).to(device)]
        off = node_off[ids.start:ids.stop + 1] - node_off[ids.start]
        tb = table_batch(reg, bbox, role, off, col_gap, row_gap, col_gap_em, _TABLE, min_words)
        grids = table_grids(tb.table, bbox, role, off, tb.root, tb.page, tb.gap, col_roles, row_roles)
        texts = [data.pages[i].get('texts') for i in ids]
        out[ids.start:ids.stop] = tables_from_grids(tb.table.cpu().numpy(), bbox.cpu().numpy(), role.cpu().numpy(), off,
                                                    tb.root.cpu().numpy(), tb.page.cpu().numpy(), [a.cpu().numpy() for a in grids], texts,
                                                    col_roles, row_roles, None if tb.score is None else tb.score.cpu().numpy())
    return out


def table_csv(table) -> str:
    """A table's ``'grid'`` as CSV text (the ``csv`` module's default dialect: ``\\r\\n`` line ends, quotes where needed)."""
    import csv
    import io
    buf = io.StringIO()
    csv.writer(buf).writerows(table['grid'])
    return buf.getvalue()


def tables_json(data, tables):
    """``{page_name: [table, ...]}`` of ``extract_tables``' result: every page of the set, the table dicts as they are (they
    hold ints, floats, strings and lists only)."""
    return {str(data.pages[i]['page']): list(page) for i, page in enumerate(tables)}


def table_structure_json(data, tables):
    """The tables' structure as a document in the layout of ``regions_json`` -- ``{kind: {page_name: {'bboxes': [...], 'scores':
    [...]}}}`` -- with the kinds ``'table'`` (the table's box), ``'table-row'`` (``[box.x0, row.lo, box.x1, row.hi]`` per row
    band) and ``'table-col'`` (``[col.lo, box.y0, col.hi, box.y1]`` per column band): what PubTables-1M annotates as TABLE,
    TABLE_ROW and TABLE_COL (categories 4, 12 and 11 of ``blocks_gt_json``).  Every box of a table scores the table's
    ``'score'``, or 1.0 where it has none."""
    doc = {'table': {}, 'table-row': {}, 'table-col': {}}
    for i, page in enumerate(tables):
        name = str(data.pages[i]['page'])
        for tab in page:
            x0, y0, x1, y1 = tab['box']
            boxes = {'table': [[x0, y0, x1, y1]], 'table-row': [[x0, lo, x1, hi] for lo, hi in tab['rows']],
                     'table-col': [[lo, y0, hi, y1] for lo, hi in tab['cols']]}
            for kind, found in boxes.items():
                if found:
                    entry = doc[kind].setdefault(name, {'bboxes': [], 'scores': []})
                    entry['bboxes'] += [[int(c) for c in b] for b in found]
                    entry['scores'] += [float(tab.get('score', 1.0))] * len(found)
    return doc
