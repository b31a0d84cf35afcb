"""Reference of the batch assembly (gte_batch_assemble, gte_batch_assemble_rows, gte_batch_csr, gte_batch_rows), NumPy only.

A RESIDENT SET is a dict in the layout documented at the top of csrc/batch_ops.hip:
    node_off  int32 [P + 1]
    feat      float32 [N, F]           label  float32 [N] | None
    dirs      list (in-direction, out-direction) of dicts
        edge_off     int32 [P + 1]
        indptr_loc   int32 [N + P]     page p's n_p + 1 entries (counting from 0) start at node_off[p] + p
        indices_loc  int32 [E]         column ids local to the page
        weight       float32 [E] | None
``assemble_ref`` walks the chosen pages one by one and appends each page's rows and entries: plain loops, none of the kernels'
offset arithmetic.  Every output is an integer or a copied bit pattern, so callers compare exactly (as int32 views).

tests/test_batch_ref_cpu.py pins this file to data.synthetic.concat_pages + the oracle's COO -> CSR."""
import numpy as np

# bit patterns of the generated float arrays: a running counter above these bases is a distinct finite positive float per entry
FEAT_BITS, LABEL_BITS, WEIGHT_BITS = 0x3F800000, 0x40800000, 0x3E000000


def _counter_floats(n, base):
    return (np.arange(n, dtype=np.int64) + base).astype(np.int32).view(np.float32)


def make_resident(triples, n_cols, weighted=True, labelled=True, seed=0):
    """Resident set from (n_nodes, n_in_entries, n_out_entries) per page.  At this level the arrays need not describe a graph (the
    kernels do index arithmetic only): indices_loc, feat, label and weight hold DISTINCT values, so a swapped or shifted dword
    shows; each page's indptr is a random ascending split of its entries over its rows (0 first, the entry count last)."""
    rng = np.random.default_rng(seed)
    triples = [tuple(int(v) for v in t) for t in triples]
    for n, ei, eo in triples:
        assert n >= 0 and ei >= 0 and eo >= 0 and (n > 0 or (ei == 0 and eo == 0)), "a page without nodes has no entries"
    node_off = np.zeros(len(triples) + 1, dtype=np.int64)
    for p, (n, _, _) in enumerate(triples):
        node_off[p + 1] = node_off[p] + n
    n_tot = int(node_off[-1])
    dirs = []
    for d in range(2):
        edge_off = np.zeros(len(triples) + 1, dtype=np.int64)
        indptr_loc = []
        for p, t in enumerate(triples):
            n, e = t[0], t[1 + d]
            edge_off[p + 1] = edge_off[p] + e
            cuts = np.sort(rng.integers(0, e + 1, size=max(n - 1, 0)))
            indptr_loc.append(np.concatenate([[0], cuts, [e]] if n > 0 else [[0]]).astype(np.int32))
            assert indptr_loc[-1].size == n + 1
        e_tot = int(edge_off[-1])
        dirs.append(dict(edge_off=edge_off.astype(np.int32), indptr_loc=np.concatenate(indptr_loc).astype(np.int32),
                         indices_loc=(5 + 3 * np.arange(e_tot, dtype=np.int64) + d).astype(np.int32),
                         weight=_counter_floats(e_tot, WEIGHT_BITS + (d << 22)) if weighted else None))
    return dict(node_off=node_off.astype(np.int32), feat=_counter_floats(n_tot * n_cols, FEAT_BITS).reshape(n_tot, n_cols),
                label=_counter_floats(n_tot, LABEL_BITS) if labelled else None, dirs=dirs)


def resident_from_pages(pages, coo_to_csr):
    """Resident set of real page graphs (data.synthetic.Page): per page its OWN two CSRs by ``coo_to_csr(key_other, key, n, w) ->
    (indptr, indices, w_sorted, perm)`` (the oracle's stable COO -> CSR).  The out-direction carries the weights the models' backward
    uses: w / in_degree(destination), fp32 (graph.PageGraph.out_weights(w, mean=True))."""
    node_off, edge_off = [0], [[0], [0]]
    parts = [dict(indptr_loc=[], indices_loc=[], weight=[]) for _ in range(2)]
    for p in pages:
        n = p.num_nodes
        node_off.append(node_off[-1] + n)
        ip_in, idx_in, w_in, _ = coo_to_csr(p.src, p.dst, n, p.weight)
        deg = np.diff(ip_in.astype(np.int64)).astype(np.float32)
        inv = np.where(deg > 0, np.float32(1.0) / np.maximum(deg, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        ip_out, idx_out, w_out, _ = coo_to_csr(p.dst, p.src, n, p.weight)
        w_out = (w_out * inv[idx_out]).astype(np.float32)
        for d, (ip, idx, w) in enumerate(((ip_in, idx_in, w_in), (ip_out, idx_out, w_out))):
            assert ip.size == n + 1 and ip[0] == 0 and ip[-1] == idx.size == p.src.size
            edge_off[d].append(edge_off[d][-1] + idx.size)
            parts[d]["indptr_loc"].append(ip)
            parts[d]["indices_loc"].append(idx)
            parts[d]["weight"].append(w)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt) for x in xs]) if xs else np.zeros(0, dtype=dt)
    dirs = [dict(edge_off=np.asarray(edge_off[d], dtype=np.int32), indptr_loc=cat(parts[d]["indptr_loc"], np.int32),
                 indices_loc=cat(parts[d]["indices_loc"], np.int32), weight=cat(parts[d]["weight"], np.float32)) for d in range(2)]
    return dict(node_off=np.asarray(node_off, dtype=np.int32), feat=np.concatenate([p.feat for p in pages], axis=0).astype(np.float32),
                label=np.concatenate([p.label for p in pages]).astype(np.float32), dirs=dirs)


def assemble_ref(resident, page_ids, row_map_pad=0, n_res=None):
    """What the kernels must write for the batch ``page_ids`` -> dict of
        b_node_off [nb + 1], b_edge_off [2][nb + 1]                         (the caller-side prefix sums)
        indptr_out [2][n_out + 1], indices_out [2][e_out], weight_out [2][e_out]  (ones where the set has no weights)
        feat_out [n_out, F], label_out [n_out] | None
        row_map [n_out + row_map_pad]: the resident row of every batch row, then row_map_pad entries equal to n_res."""
    node_off = resident["node_off"]
    n_res = int(node_off[-1]) if n_res is None else int(n_res)
    n_cols = resident["feat"].shape[1]
    b_node_off, b_edge_off = [0], [[0], [0]]
    feat_rows, labels, row_map = [], [], []
    indptr, indices, weight = [[], []], [[], []], [[], []]
    for p in page_ids:
        p = int(p)
        first, last = int(node_off[p]), int(node_off[p + 1])
        rows_before = b_node_off[-1]
        for r in range(first, last):
            row_map.append(r)
        feat_rows.append(resident["feat"][first:last])
        if resident["label"] is not None:
            labels.append(resident["label"][first:last])
        for d, s in enumerate(resident["dirs"]):
            e_first, e_last = int(s["edge_off"][p]), int(s["edge_off"][p + 1])
            entries_before = b_edge_off[d][-1]
            local = s["indptr_loc"][first + p: last + p + 1]                 # the page's own indptr: n_p + 1 entries
            assert int(local[0]) == 0 and int(local[-1]) == e_last - e_first
            for r in range(last - first):
                indptr[d].append(int(local[r]) + entries_before)
            for e in range(e_first, e_last):
                indices[d].append(int(s["indices_loc"][e]) + rows_before)
            weight[d].append(s["weight"][e_first:e_last] if s["weight"] is not None else np.ones(e_last - e_first, dtype=np.float32))
            b_edge_off[d].append(entries_before + (e_last - e_first))
        b_node_off.append(rows_before + (last - first))
    for d in range(2):
        indptr[d].append(b_edge_off[d][-1])
    row_map.extend([n_res] * int(row_map_pad))
    i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)
    return dict(b_node_off=i32(b_node_off), b_edge_off=[i32(b_edge_off[0]), i32(b_edge_off[1])],
                indptr_out=[i32(indptr[0]), i32(indptr[1])], indices_out=[i32(indices[0]), i32(indices[1])],
                weight_out=[np.concatenate(weight[d] + [np.zeros(0, dtype=np.float32)]).astype(np.float32) for d in range(2)],
                feat_out=np.concatenate(feat_rows + [np.zeros((0, n_cols), dtype=np.float32)], axis=0),
                label_out=None if resident["label"] is None else np.concatenate(labels + [np.zeros(0, dtype=np.float32)]),
                row_map=i32(row_map), n_out=b_node_off[-1], e_out=[b_edge_off[0][-1], b_edge_off[1][-1]])


def bits(a):
    """int32 view of an int32 / float32 array (exact comparison of copied floats)"""
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.int32 else a.view(np.int32)
