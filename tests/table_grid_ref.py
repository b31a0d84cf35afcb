"""CPU reference of gte_table_grid (include/gte.h), written from its rule: per table and axis a boolean occupancy array over the
pixels the profile words cover, the bands as the cumulative sum of its run starts.  numpy only (it also runs where the GPU tests
run).  ``synthetic_table`` draws the R x C tables of the tests that ask what the grid MEANS."""
import numpy as np

MAX_EXTENT = 8192
MAX_GAP = 1024
COORD_MAX = 1 << 30


def axis_ref(lo, hi, profile, gap):
    """One axis of one table.  ``lo`` / ``hi``: the members' two corners in any order, ``profile``: bool per member, ``gap``: int.
    Returns None for status 2, else ``(band0, band1, start, end, extents)``: per member the bands of the first / last occupied
    pixel inside its interval (-1, -1: none) with the start of the first band and the end of the last one (0, 0: none), and the
    list of the bands' extents ``(lo, hi)`` in page coordinates."""
    a, b = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    hi1 = np.maximum(hi, lo + 1)
    profile = np.asarray(profile, dtype=bool)
    origin = int(lo.min())
    if hi1.max() - origin > MAX_EXTENT or not 0 <= gap <= MAX_GAP or lo.min() < -COORD_MAX or hi1.max() > COORD_MAX:
        return None
    occ = np.zeros(int(hi1.max() - origin) + gap + 1, dtype=bool)      # (one free pixel behind the last: every run ends inside)
    for l, h in zip(lo[profile], hi1[profile]):
        occ[l - origin:h + gap - origin] = True
    starts = occ & ~np.concatenate([[False], occ[:-1]])
    band = np.cumsum(starts) - 1                          # of every occupied pixel
    run_start = np.nonzero(starts)[0]
    run_end = np.nonzero(occ & ~np.concatenate([occ[1:], [False]]))[0] + 1
    extents = [(int(s) + origin, int(e) - gap + origin) for s, e in zip(run_start, run_end)]
    n = lo.shape[0]
    band0, band1 = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    start, end = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for v in range(n):
        inside = np.nonzero(occ[lo[v] - origin:hi1[v] - origin])[0]
        if inside.size:
            band0[v], band1[v] = band[lo[v] - origin + inside[0]], band[lo[v] - origin + inside[-1]]
            start[v], end[v] = extents[band0[v]][0], extents[band1[v]][1]
    return band0, band1, start, end, extents


def _mask(roles):
    if isinstance(roles, (int, np.integer)):
        return int(roles)
    return sum({1 << int(r) for r in roles})


def table_grid_ref(bbox, node_off, table, role, table_root, table_page, table_gap, col_roles, row_roles, cell=None, cell_box=None):
    """``(cell [n, 4], cell_box [n, 4], table_shape [T, 2], table_box [T, 4], table_words [T], table_status [T])`` as int32 arrays.
    ``cell`` / ``cell_box``: what the rows hold before the call (default: -1 / 0, the wrapper's pre-fill); rows of words of no
    listed table come back as they went in."""
    bbox = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    node_off, table, role = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (node_off, table, role))
    table_root, table_page = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (table_root, table_page))
    table_gap = np.asarray(table_gap, dtype=np.int64).reshape(-1, 2)
    n, n_pages, nt = bbox.shape[0], node_off.shape[0] - 1, table_root.shape[0]
    col_roles, row_roles = _mask(col_roles), _mask(row_roles)
    cell = np.full((n, 4), -1, dtype=np.int64) if cell is None else np.array(cell, dtype=np.int64).reshape(n, 4)
    cell_box = np.zeros((n, 4), dtype=np.int64) if cell_box is None else np.array(cell_box, dtype=np.int64).reshape(n, 4)
    shape, box = np.zeros((nt, 2), dtype=np.int64), np.zeros((nt, 4), dtype=np.int64)
    words, status = np.zeros(nt, dtype=np.int64), np.zeros(nt, dtype=np.int64)
    in_roles = lambda r, mask: np.array([0 <= int(k) < 32 and bool((mask >> int(k)) & 1) for k in r], dtype=bool)
    for t in range(nt):
        p = int(table_page[t])
        if not 0 <= p < n_pages or node_off[p] < 0 or node_off[p + 1] > n or node_off[p + 1] < node_off[p]:
            status[t] = 3
            continue
        v = np.arange(node_off[p], node_off[p + 1])
        v = v[table[v] == table_root[t]] if table_root[t] >= 0 else v[:0]
        if v.size == 0:
            status[t] = 1
            continue
        words[t] = v.size
        b = bbox[v]
        x = axis_ref(b[:, 0], b[:, 2], in_roles(role[v], col_roles), int(table_gap[t, 0]))
        y = axis_ref(b[:, 1], b[:, 3], in_roles(role[v], row_roles), int(table_gap[t, 1]))
        lo, hi = np.minimum(b[:, :2], b[:, 2:]), np.maximum(b[:, :2], b[:, 2:])
        hi1 = np.maximum(hi, lo + 1)
        if lo.min() >= -COORD_MAX and hi1.max() <= COORD_MAX:
            box[t] = [lo[:, 0].min(), lo[:, 1].min(), hi1[:, 0].max(), hi1[:, 1].max()]
        if x is None or y is None:
            status[t] = 2
            cell[v], cell_box[v] = -1, 0
            continue
        shape[t] = [len(y[4]), len(x[4])]
        cell[v] = np.stack([y[0], y[1], x[0], x[1]], axis=1)
        cell_box[v] = np.stack([x[2], y[2], x[3], y[3]], axis=1)
    return tuple(a.astype(np.int32) for a in (cell, cell_box, shape, box, words, status))


# ---- synthetic tables whose grid is known ------------------------------------------------------------------------------------
GUTTER, LEADING, WORD_SPACE = 30, 10, 7


def synthetic_table(rng, n_rows, n_cols, x0=40, y0=60, header=True, shuffle=True):
    """An ``n_rows`` x ``n_cols`` table: every cell holds 1 - 3 words 7 px apart on one line, the columns stand 30 px and the rows
    10 px apart, words are 19 - 24 px high and 12 - 60 px wide; the first row holds column headers (category 7) when ``header``,
    every other word is a table cell (10).  Node order shuffled.  Returns a dict of arrays per word -- ``bbox`` int32 [n, 4],
    ``role``, ``row``, ``col``, ``text`` (list) -- and ``rows`` / ``cols``: the bands' extents ``[lo, hi]``, ``cell_text[r][c]``."""
    n_words = rng.integers(1, 4, (n_rows, n_cols))
    widths = [[rng.integers(12, 61, n_words[r, c]) for c in range(n_cols)] for r in range(n_rows)]
    col_w = [max(int(widths[r][c].sum()) + WORD_SPACE * (len(widths[r][c]) - 1) for r in range(n_rows)) for c in range(n_cols)]
    col_x = x0 + np.concatenate([[0], np.cumsum([w + GUTTER for w in col_w[:-1]])]).astype(np.int64)
    bbox, role, row, col, text = [], [], [], [], []
    y = y0
    cell_text = [["" for _ in range(n_cols)] for _ in range(n_rows)]
    for r in range(n_rows):
        heights = [rng.integers(19, 25, n_words[r, c]) for c in range(n_cols)]
        tallest = max(int(h.max()) for h in heights)
        for c in range(n_cols):
            x, names = int(col_x[c]), []
            for k, (w, h) in enumerate(zip(widths[r][c], heights[c])):
                bbox.append([x, y, x + int(w), y + int(h)])
                role.append(7 if header and r == 0 else 10)
                row.append(r)
                col.append(c)
                names.append(f"r{r}c{c}w{k}")
                x += int(w) + WORD_SPACE
            text += names
            cell_text[r][c] = " ".join(names)
        y += tallest + LEADING
    order = rng.permutation(len(bbox)) if shuffle else np.arange(len(bbox))
    bbox = np.asarray(bbox, dtype=np.int32)[order]
    row, col = np.asarray(row)[order], np.asarray(col)[order]
    rows = [[int(bbox[row == r, 1].min()), int(bbox[row == r, 3].max())] for r in range(n_rows)]
    cols = [[int(bbox[col == c, 0].min()), int(bbox[col == c, 2].max())] for c in range(n_cols)]
    return {"bbox": bbox, "role": np.asarray(role, dtype=np.int32)[order], "row": row, "col": col,
            "text": [text[i] for i in order], "rows": rows, "cols": cols, "cell_text": cell_text}


PAGE_SIZE = (1600, 1000)                                  # holds the widest table: 6 columns of <= 194 px + gutters
CLASS_OF_ROLE = {1: 1, 7: 6, 8: 7, 10: 8}                 # converted class id of a category (postprocessing.DEFAULT_CLASS_CATEGORY)


def synthetic_page(rng, n_rows, n_cols):
    """A page that holds one ``synthetic_table`` under a line of three TEXT words, the words of both shuffled together.  Returns
    the table's dict with ``bbox`` / ``role`` / ``text`` of ALL words, ``row`` / ``col`` -1 for the text words, and further
    ``classes`` (converted class ids), ``member`` (bool), ``box`` (the table's union box) and ``annotations``: rows ``[x0, y0, x1,
    y1, category]`` for the table (4), its rows (12: the table's x range, the row's y range) and its columns (11)."""
    tab = synthetic_table(rng, n_rows, n_cols, shuffle=False)
    n = len(tab["text"])
    line = np.asarray([[40 + 90 * k, 14, 40 + 90 * k + int(rng.integers(30, 70)), 36] for k in range(3)], dtype=np.int32)
    order = rng.permutation(n + 3)
    bbox = np.concatenate([tab["bbox"], line])[order]
    box = [int(tab["bbox"][:, 0].min()), int(tab["bbox"][:, 1].min()), int(tab["bbox"][:, 2].max()), int(tab["bbox"][:, 3].max())]
    role = np.concatenate([tab["role"], [1, 1, 1]])[order].astype(np.int32)
    ann = [box + [4]] + [[box[0], lo, box[2], hi, 12] for lo, hi in tab["rows"]] + [[lo, box[1], hi, box[3], 11] for lo, hi in tab["cols"]]
    return dict(tab, bbox=bbox, role=role, text=[(tab["text"] + ["t0", "t1", "t2"])[i] for i in order],
                row=np.concatenate([tab["row"], [-1] * 3])[order], col=np.concatenate([tab["col"], [-1] * 3])[order],
                classes=np.asarray([CLASS_OF_ROLE[int(r)] for r in role], dtype=np.int64), member=order < n, box=box,
                annotations=[[float(v) for v in row[:4]] + [row[4]] for row in ann])


def auto_gap(bbox, em=0.5):
    """The wrapper's ``'auto'`` column gap of one table: floor(em * mean word height), the mean a float64 quotient of exact sums."""
    b = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    return int(min(max(np.floor(em * (float(np.abs(b[:, 3] - b[:, 1]).sum()) / float(b.shape[0]))), 0), MAX_GAP))
