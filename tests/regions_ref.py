"""CPU reference of gte_page_regions (include/gte.h), written from its definition: a union-find over the CSR entries whose two
endpoints lie on one page and carry the same non-negative group.  numpy only (it also runs where the GPU tests run)."""
import numpy as np


def page_regions_ref(indptr, indices, node_off, group, bbox):
    """(comp [n], region_box [n, 4], region_count [n]) as int32 arrays.

    comp[v] = smallest node id of v's component of the undirected graph {u, v}: u -> v or v -> u in the CSR, group[u] == group[v]
    >= 0 (-1 where group[v] < 0); roots (comp[v] == v) carry the member count and the union box, every other row zeros."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    node_off, group = np.asarray(node_off, dtype=np.int64), np.asarray(group, dtype=np.int64)
    bbox = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    n = group.shape[0]
    assert indptr.shape[0] == n + 1 and bbox.shape[0] == n and node_off[0] == 0 and node_off[-1] == n
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    src = indices[:indptr[-1]]
    page_of = np.searchsorted(node_off[1:], np.arange(n), side="right")
    inside = (src >= 0) & (src < n)
    src_c = np.where(inside, src, 0)
    ok = inside & (page_of[src_c] == page_of[dst]) & (group[src_c] == group[dst]) & (group[dst] >= 0) & (src != dst)
    pairs = np.unique(np.stack([np.minimum(src[ok], dst[ok]), np.maximum(src[ok], dst[ok])], axis=1), axis=0) if ok.any() else []

    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)             # the smaller id stays the root: root == min(component)
    root = np.array([find(v) for v in range(n)], dtype=np.int64)
    member = group >= 0
    comp = np.where(member, root, -1)
    count = np.zeros(n, dtype=np.int64)
    np.add.at(count, root[member], 1)
    big = np.iinfo(np.int64).max
    lo = np.full((n, 2), big, dtype=np.int64)
    hi = np.full((n, 2), -big, dtype=np.int64)
    np.minimum.at(lo, root[member], bbox[member, :2])
    np.maximum.at(hi, root[member], bbox[member, 2:])
    box = np.concatenate([lo, hi], axis=1)
    box[count == 0] = 0
    return comp.astype(np.int32), box.astype(np.int32), count.astype(np.int32)


def in_csr(src, dst, n):
    """in-edge CSR (rows = destinations, stable) of a COO edge list: (indptr [n + 1], indices [E]) int32."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(dst, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=indptr[1:])
    return indptr.astype(np.int32), src[order].astype(np.int32)


def regions_list(comp, box, count, node_off, group, min_words=1):
    """The compacted per-page form of postprocessing.extract_regions: per page [(group, [x0, y0, x1, y1], n_words)] in ascending
    root order."""
    node_off = np.asarray(node_off, dtype=np.int64)
    out = [[] for _ in range(len(node_off) - 1)]
    for r in np.nonzero(count)[0]:
        if count[r] >= min_words:
            p = int(np.searchsorted(node_off[1:], r, side="right"))
            out[p].append((int(group[r]), [int(v) for v in box[r]], int(count[r])))
    return out
