"""CPU-only: tests/batch_ref.py (the reference of tests/test_gpu_batch_assemble.py) against an independent construction -- the
chosen pages concatenated on the host (data.synthetic.concat_pages) and the oracle's COO -> CSR of the union, which is what
graph.batch yields on the CPU -- and the host-side argument checks of the batch entry points (they return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.data import synthetic as S
from oracle import gcnsage_cpu as oc
from tests import batch_ref as ref


def hand_page(n, edges, in_feats, seed):
    """a page from an explicit edge list [(src, dst)], distinct weights and features"""
    rng = np.random.default_rng(seed)
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return S.Page(e[:, 0].copy(), e[:, 1].copy(), (0.25 + rng.random(len(e)) / 2).astype(np.float32),
                  rng.standard_normal((n, in_feats)).astype(np.float32), rng.integers(0, 9, n).astype(np.int64),
                  np.zeros((n, 4), dtype=np.int32))


def edge_pages(in_feats):
    """the pages make_pages never makes: one node and no edge; an isolated node; one directed edge (in- and out-CSR differ);
    parallel edges and a self loop; no node at all"""
    return [hand_page(1, [], in_feats, 1),
            hand_page(4, [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)], in_feats, 2),
            hand_page(2, [(1, 0)], in_feats, 3),
            hand_page(3, [(0, 1), (0, 1), (2, 2), (1, 0), (0, 1)], in_feats, 4),
            hand_page(0, [], in_feats, 5)]


def all_pages(in_feats=7):
    return S.make_pages(4, in_feats=in_feats, n_words=23) + edge_pages(in_feats) + S.make_pages(2, in_feats=in_feats, first_id=9)


def page_graphs(pages, device="cpu"):
    gs = []
    for p in pages:
        g = G.PageGraph(p.src, p.dst, p.num_nodes, device=device)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat).to(device), torch.from_numpy(p.label.astype(np.float32)).to(device)
        g.edata["feat"] = torch.from_numpy(p.weight).to(device)
        gs.append(g)
    return gs


ID_LISTS = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [4], [8], [8, 4, 8, 8, 5, 0, 5, 8], [6, 6], [4, 8]]


@pytest.mark.parametrize("ids", ID_LISTS, ids=lambda v: "-".join(map(str, v)))
def test_reference_equals_the_host_concatenation_and_the_oracle_csr(ids):
    pages = all_pages()
    res = ref.resident_from_pages(pages, oc.coo_to_in_csr)
    got = ref.assemble_ref(res, ids, row_map_pad=3, n_res=1000)
    chosen = [pages[i] for i in ids]
    src, dst, w, feat, label, off = S.concat_pages(chosen)
    n = int(off[-1])
    np.testing.assert_array_equal(got["b_node_off"], off)
    np.testing.assert_array_equal(got["feat_out"], feat)
    np.testing.assert_array_equal(got["label_out"], label.astype(np.float32))
    ip_in, idx_in, w_in, _ = oc.coo_to_in_csr(src, dst, n, w)
    ip_out, idx_out, w_out, _ = oc.coo_to_in_csr(dst, src, n, w)
    w_out = w_out * oc.in_degree_norm(ip_in).reshape(-1)[idx_out]
    for d, (ip, idx, ww) in enumerate(((ip_in, idx_in, w_in), (ip_out, idx_out, w_out))):
        np.testing.assert_array_equal(got["indptr_out"][d], ip)
        np.testing.assert_array_equal(got["indices_out"][d], idx)
        np.testing.assert_array_equal(ref.bits(got["weight_out"][d]), ref.bits(ww.astype(np.float32)))
        np.testing.assert_array_equal(got["b_edge_off"][d], np.concatenate([[0], np.cumsum([p.src.size for p in chosen])]))
    first = np.concatenate([[0], np.cumsum([p.num_nodes for p in pages])])
    want_map = [first[i] + r for i in ids for r in range(pages[i].num_nodes)] + [1000] * 3
    np.testing.assert_array_equal(got["row_map"], np.asarray(want_map, dtype=np.int32).reshape(-1))
    # ... and graph.batch on the CPU yields exactly that
    hb = G.batch(page_graphs(chosen))
    for d, csr in enumerate((hb.in_csr(), hb.out_csr())):
        np.testing.assert_array_equal(csr.indptr.numpy(), got["indptr_out"][d])
        np.testing.assert_array_equal(csr.indices.numpy(), got["indices_out"][d])
    wt = hb.edata["feat"]
    np.testing.assert_array_equal(ref.bits(hb.in_weights(wt).numpy()), ref.bits(got["weight_out"][0]))
    np.testing.assert_array_equal(ref.bits(hb.out_weights(wt, True).numpy()), ref.bits(got["weight_out"][1]))


def test_generated_sets_are_in_the_documented_layout_and_unweighted_sets_give_ones():
    triples = [(3, 4, 2), (0, 0, 0), (1, 0, 0), (5, 9, 11), (0, 0, 0), (2, 1, 0)]
    res = ref.make_resident(triples, n_cols=3, weighted=False, labelled=False, seed=5)
    assert res["node_off"].tolist() == [0, 3, 3, 4, 9, 9, 11] and res["label"] is None
    for d, s in enumerate(res["dirs"]):
        assert s["edge_off"].tolist() == np.concatenate([[0], np.cumsum([t[1 + d] for t in triples])]).tolist()
        assert s["indptr_loc"].size == 11 + len(triples) and s["weight"] is None
        for p, t in enumerate(triples):
            ip = s["indptr_loc"][res["node_off"][p] + p: res["node_off"][p + 1] + p + 1]
            assert ip[0] == 0 and ip[-1] == t[1 + d] and (np.diff(ip) >= 0).all()
        assert np.unique(s["indices_loc"]).size == s["indices_loc"].size
    assert np.unique(res["feat"].view(np.int32)).size == res["feat"].size and np.isfinite(res["feat"]).all()
    got = ref.assemble_ref(res, [3, 1, 0, 3, 4], row_map_pad=2)
    assert got["b_node_off"].tolist() == [0, 5, 5, 8, 13, 13] and got["n_out"] == 13 and got["e_out"] == [22, 24]
    assert got["b_edge_off"][0].tolist() == [0, 9, 9, 13, 22, 22] and got["label_out"] is None
    assert got["row_map"].tolist() == [4, 5, 6, 7, 8, 0, 1, 2, 4, 5, 6, 7, 8, 11, 11]
    assert got["weight_out"][0].tolist() == [1.0] * 22 and got["indptr_out"][1][-1] == 24 and got["indptr_out"][1].size == 14
    np.testing.assert_array_equal(got["feat_out"], res["feat"][[4, 5, 6, 7, 8, 0, 1, 2, 4, 5, 6, 7, 8]])
    empty = ref.assemble_ref(res, [1, 4], row_map_pad=2)
    assert empty["n_out"] == 0 and empty["indptr_out"][0].tolist() == [0] and empty["row_map"].tolist() == [11, 11]
    assert empty["feat_out"].shape == (0, 3) and empty["indices_out"][1].size == 0


@pytest.mark.parametrize("ids", ID_LISTS, ids=lambda v: "-".join(map(str, v)))
def test_batch_meta_offsets_are_the_reference_prefix_sums(ids):
    """ResidentPages built on the CPU from the page graphs (its constructor is host code) and over reference arrays"""
    pages = all_pages()
    res = ref.resident_from_pages(pages, oc.coo_to_in_csr)
    want = ref.assemble_ref(res, ids)
    t = torch.from_numpy
    sets = {name: dict(edge_off=t(s["edge_off"]), edge_off_host=t(s["edge_off"]).long(), indptr_loc=t(s["indptr_loc"]),
                       indices_loc=t(s["indices_loc"]), weight=t(s["weight"])) for name, s in zip(("in", "out"), res["dirs"])}
    over_arrays = G.ResidentPages.from_arrays("cpu", t(res["node_off"]).long(), t(res["feat"]), t(res["label"]).reshape(-1, 1), sets,
                                              True, {"in": 0, "out": 0})
    built = G.ResidentPages(page_graphs(pages), "cpu")
    for rp in (over_arrays, built):
        meta, n_out, e_in, e_out, n_sizes = rp.batch_meta(ids)
        nb = len(ids)
        assert meta.dtype == torch.int32 and meta.numel() == nb + 3 * (nb + 1)
        assert meta[:nb].tolist() == ids and (n_out, e_in, e_out) == (want["n_out"], want["e_out"][0], want["e_out"][1])
        np.testing.assert_array_equal(meta[nb:2 * nb + 1].numpy(), want["b_node_off"])
        np.testing.assert_array_equal(meta[2 * nb + 1:3 * nb + 2].numpy(), want["b_edge_off"][0])
        np.testing.assert_array_equal(meta[3 * nb + 2:].numpy(), want["b_edge_off"][1])
        assert n_sizes.tolist() == [pages[i].num_nodes for i in ids]
    # the constructor's resident arrays are the reference's, array by array
    np.testing.assert_array_equal(built.node_off.numpy(), res["node_off"])
    np.testing.assert_array_equal(built.feat.numpy(), res["feat"])
    np.testing.assert_array_equal(built.label.reshape(-1).numpy(), res["label"])
    for name, s in zip(("in", "out"), res["dirs"]):
        for key in ("edge_off", "indptr_loc", "indices_loc"):
            np.testing.assert_array_equal(built._sets[name][key].numpy(), s[key], err_msg=f"{name} {key}")
        np.testing.assert_array_equal(ref.bits(built._sets[name]["weight"].numpy()), ref.bits(s["weight"]))


def test_resident_pages_of_edgeless_pages_only():
    """a dataset of one-word pages has no edge at all: every array of the CSRs is empty or zero"""
    pages = [hand_page(1, [], 5, 1), hand_page(1, [], 5, 2), hand_page(2, [], 5, 3)]
    res = ref.resident_from_pages(pages, oc.coo_to_in_csr)
    built = G.ResidentPages(page_graphs(pages), "cpu")
    assert built.max_deg == {"in": 0, "out": 0}
    for name, s in zip(("in", "out"), res["dirs"]):
        assert s["edge_off"].tolist() == [0, 0, 0, 0] and s["indptr_loc"].tolist() == [0] * 7
        for key in ("edge_off", "indptr_loc", "indices_loc"):
            np.testing.assert_array_equal(built._sets[name][key].numpy(), s[key], err_msg=f"{name} {key}")
    meta, n_out, e_in, e_out, _ = built.batch_meta([2, 0])
    assert (n_out, e_in, e_out) == (3, 0, 0) and meta.tolist() == [2, 0, 0, 2, 3, 0, 0, 0, 0, 0, 0]


# ---- host-side argument checks: every call below returns before any launch (no device is needed, none is touched) ----------------
INVALID, UNSUPPORTED = -1, -4


def _valid():
    """arguments of gte_batch_assemble_rows that pass every check (never sent as they are); pointers name host memory nobody reads"""
    buf = np.zeros(64, dtype=np.int32)
    a = buf.ctypes.data
    arrays = lambda: _lib.BatchArrays(a, a, a, a, a, a, a, a)
    return dict(keep=buf, pages=a, n_batch=2, node_off=a, b_node_off=a, in_edges=arrays(), out_edges=arrays(), feat=a, ld_feat=8, n_cols=8,
                feat_out=a, label=a, label_out=a, n_out=5, row_map=a, row_map_pad=1, n_res=9)


def _assemble(**change):
    v = _valid()
    v.update(change)
    adr = lambda s: None if s is None else ctypes.addressof(s)
    return _lib.load().gte_batch_assemble(v["pages"], v["n_batch"], v["node_off"], v["b_node_off"], adr(v["in_edges"]), adr(v["out_edges"]),
                                          v["feat"], v["ld_feat"], v["n_cols"], v["feat_out"], v["label"], v["label_out"], v["n_out"], None)


def _assemble_rows(**change):
    v = _valid()
    v.update(change)
    adr = lambda s: None if s is None else ctypes.addressof(s)
    return _lib.load().gte_batch_assemble_rows(v["pages"], v["n_batch"], v["node_off"], v["b_node_off"], adr(v["in_edges"]),
                                               adr(v["out_edges"]), v["feat"], v["ld_feat"], v["n_cols"], v["feat_out"], v["label"],
                                               v["label_out"], v["n_out"], v["row_map"], v["row_map_pad"], v["n_res"], None)


def _arrays_without(field):
    a = _valid()["pages"]
    s = _lib.BatchArrays(a, a, a, a, a, a, a, a)
    setattr(s, field, None)
    return s


@pytest.mark.parametrize("call", [_assemble, _assemble_rows], ids=["assemble", "assemble_rows"])
def test_batch_assemble_rejects_bad_arguments_before_any_launch(call):
    lib = _lib.load()
    err = lambda: lib.gte_last_error()
    assert call(n_batch=0) == INVALID and b"bad sizes" in err()
    assert call(n_batch=65536) == INVALID and b"bad sizes" in err()
    assert call(n_batch=-3) == INVALID and call(n_out=-1) == INVALID and call(n_cols=0) == INVALID
    assert call(feat_out=None) == INVALID and b"null pointer" in err()                       # feat without feat_out
    assert call(pages=None) == INVALID and call(node_off=None) == INVALID and call(b_node_off=None) == INVALID
    assert call(ld_feat=9) == UNSUPPORTED and b"packed" in err()
    assert call(ld_feat=7) == UNSUPPORTED
    assert call(label_out=None) == INVALID and b"label" in err()                             # label without label_out
    assert call(label=None) == INVALID and b"label" in err()
    for field in ("edge_off", "indptr_loc", "b_edge_off", "indptr_out"):
        assert call(in_edges=_arrays_without(field)) == INVALID and b"null CSR pointer" in err(), field
        assert call(out_edges=_arrays_without(field)) == INVALID and b"null CSR pointer" in err(), field


def test_batch_assemble_needs_features_and_assemble_rows_a_map():
    lib = _lib.load()
    assert _assemble(feat=None, feat_out=None) == INVALID and b"null pointer" in lib.gte_last_error()      # no feat and no row map
    assert _assemble(feat=None) == INVALID
    assert _assemble_rows(row_map=None) == INVALID and b"null row map" in lib.gte_last_error()
    assert _assemble_rows(row_map=None, feat=None, feat_out=None) == INVALID
    assert _assemble_rows(row_map_pad=-1) == INVALID and b"row map" in lib.gte_last_error()
    assert _assemble_rows(n_res=-1) == INVALID and _assemble_rows(n_res=1 << 31) == INVALID
    assert _assemble_rows(feat=None) == INVALID and _assemble_rows(feat_out=None) == INVALID              # one of the pair only


def test_batch_rows_and_batch_csr_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.int32)
    a = buf.ctypes.data
    rows = lambda n_batch=2, inp=a, ld_in=8, out=a, ld_out=8, n_out=5, n_cols=8, pages=a: lib.gte_batch_rows(
        pages, n_batch, a, a, inp, ld_in, out, ld_out, n_out, n_cols, None)
    assert rows(ld_in=7) == INVALID and b"ld < n_cols" in lib.gte_last_error()
    assert rows(ld_out=7) == INVALID and b"ld < n_cols" in lib.gte_last_error()
    assert rows(n_batch=0) == INVALID and rows(n_cols=0) == INVALID and rows(n_out=-1) == INVALID
    assert rows(inp=None) == INVALID and rows(out=None) == INVALID and rows(pages=None) == INVALID
    assert rows(n_out=0) == 0                                                                # nothing to move: no launch
    csr = lambda n_batch=2, n_out=5, e_out=6, indptr_loc=a, indptr_out=a, indices_loc=a, indices_out=a: lib.gte_batch_csr(
        a, n_batch, a, a, a, a, indptr_loc, indices_loc, a, indptr_out, indices_out, a, n_out, e_out, None)
    assert csr(n_batch=0) == INVALID and csr(n_out=-1) == INVALID and csr(e_out=-1) == INVALID
    assert csr(indptr_loc=None) == INVALID and csr(indptr_out=None) == INVALID and b"null pointer" in lib.gte_last_error()
    assert csr(indices_loc=None) == INVALID and csr(indices_out=None) == INVALID and b"null indices" in lib.gte_last_error()
