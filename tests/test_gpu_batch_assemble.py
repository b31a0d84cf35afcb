"""Batch assembly on the device -- gte_batch_assemble, gte_batch_assemble_rows, their deferral into the fold launch, the older pieces
gte_batch_csr / gte_batch_rows, and ResidentPages.batch on top -- against tests/batch_ref.py by direct C-ABI calls.  Every output is
an integer or a copied bit pattern: all comparisons are exact, on int32 views.

Every output array is cut out of a sentinel-filled tensor with GUARD dwords on each side, at a dword offset 0..3 behind a 16-byte
boundary (so every head length of a destination-aligned copy occurs), every input at such an offset too (every source
misalignment); after the call and ONE synchronise the payload must be the reference and every other dword the sentinel."""
import ctypes

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.data import synthetic as S
from oracle import gcnsage_cpu as oc
from tests import batch_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
GUARD = 8


class In:
    """an input array at dword offset ``off`` behind a 16-byte boundary"""

    def __init__(self, a, off):
        a = ref.bits(a).reshape(-1)
        self.big = torch.zeros(off + a.size + 4, dtype=torch.int32, device=DEV)
        assert self.big.data_ptr() % 16 == 0
        if a.size:
            self.big[off:off + a.size] = torch.from_numpy(a).to(DEV)
        self.ptr = self.big.data_ptr() + 4 * off


class Out:
    """an output array of n dwords at dword offset ``off`` behind a 16-byte boundary, in a sentinel-filled tensor"""

    def __init__(self, n, off):
        self.n, self.lo = int(n), GUARD + off
        self.big = torch.full((self.lo + self.n + GUARD + 3,), SENTINEL, dtype=torch.int32, device=DEV)
        assert self.big.data_ptr() % 16 == 0
        self.ptr = self.big.data_ptr() + 4 * self.lo

    def assert_holds(self, want, what):
        """want: the payload (any shape; int32 or float32), or None = the call must not have written a single dword"""
        got = self.big.cpu().numpy()
        assert (got[:self.lo] == SENTINEL).all() and (got[self.lo + self.n:] == SENTINEL).all(), f"{what}: a guard dword was written"
        if want is None:
            assert (got == SENTINEL).all(), f"{what}: written, but the call must leave it alone"
        else:
            want = ref.bits(want).reshape(-1)
            assert want.size == self.n
            np.testing.assert_array_equal(got[self.lo:self.lo + self.n], want, err_msg=what)


_WANT = {}


def want_of(res, ids, pad=0):
    """the reference of one (set, page list, map padding): for the module's shared sets computed once and shared (never modified)"""
    name = next((k for k, s in _SETS.items() if s is res), None)
    if name is None:
        return ref.assemble_ref(res, ids, pad, int(res["node_off"][-1]))
    key = (name, tuple(int(i) for i in ids), int(pad))
    if key not in _WANT:
        _WANT[key] = ref.assemble_ref(res, ids, pad, int(res["node_off"][-1]))
    return _WANT[key]


class Call:
    """One gte_batch_assemble (row_map_pad None) or gte_batch_assemble_rows call: inputs uploaded, outputs allocated.
    dirs: how many CSR directions are passed (2: both, 1: in-edges only, 0: neither); weight_out / feat False: passed as NULL."""

    def __init__(self, res, ids, in_off=0, out_off=0, dirs=2, weight_out=True, feat=True, row_map_pad=None):
        self.res, self.ids, self.pad, self.n_dirs = res, [int(i) for i in ids], row_map_pad, dirs
        self.want = w = want_of(res, ids, row_map_pad or 0)
        self.n_out, self.f, self.n_res = w["n_out"], res["feat"].shape[1], int(res["node_off"][-1])
        k_in, k_out = [in_off], [out_off]

        def inp(a):
            k_in[0] += 1
            return None if a is None else In(a, k_in[0] % 4)

        def out(n, have=True):
            k_out[0] += 1
            return Out(n, k_out[0] % 4) if have else None

        self.pages, self.node_off, self.b_node_off = inp(np.asarray(self.ids, dtype=np.int32)), inp(res["node_off"]), inp(w["b_node_off"])
        self.feat, self.label = inp(res["feat"] if feat else None), inp(res["label"])
        self.feat_out, self.label_out = out(self.n_out * self.f, feat), out(self.n_out, res["label"] is not None)
        self.row_map = out(self.n_out + (row_map_pad or 0), row_map_pad is not None)
        self.dir_in, self.dir_out, self.descs = [], [], []
        for d in range(dirs):
            s = res["dirs"][d]
            i = dict(edge_off=inp(s["edge_off"]), indptr_loc=inp(s["indptr_loc"]), indices_loc=inp(s["indices_loc"]), weight=inp(s["weight"]),
                     b_edge_off=inp(w["b_edge_off"][d]))
            o = dict(indptr=out(self.n_out + 1), indices=out(w["e_out"][d]), weight=out(w["e_out"][d], weight_out))
            p = lambda x: None if x is None else x.ptr
            self.descs.append(_lib.BatchArrays(p(i["edge_off"]), p(i["indptr_loc"]), p(i["indices_loc"]), p(i["weight"]), p(i["b_edge_off"]),
                                               p(o["indptr"]), p(o["indices"]), p(o["weight"])))
            self.dir_in.append(i)
            self.dir_out.append(o)

    def launch(self, stream=None):
        lib = _lib.load()
        p = lambda x: None if x is None else x.ptr
        adr = lambda d: ctypes.addressof(self.descs[d]) if d < self.n_dirs else None
        st = _lib.current_stream() if stream is None else stream
        head = (p(self.pages), len(self.ids), p(self.node_off), p(self.b_node_off), adr(0), adr(1), p(self.feat),
                self.f if self.feat else 0, self.f if self.feat else 0, p(self.feat_out), p(self.label), p(self.label_out), self.n_out)
        if self.pad is None:
            return lib.gte_batch_assemble(*head, st)
        return lib.gte_batch_assemble_rows(*head, p(self.row_map), self.pad, self.n_res, st)

    def outputs(self):
        """(name, Out, reference payload) of every output array that was passed"""
        w = self.want
        items = [("feat_out", self.feat_out, w["feat_out"]), ("label_out", self.label_out, w["label_out"]),
                 ("row_map", self.row_map, w["row_map"])]
        for d, o in enumerate(self.dir_out):
            items += [(f"indptr_out[{d}]", o["indptr"], w["indptr_out"][d]), (f"indices_out[{d}]", o["indices"], w["indices_out"][d]),
                      (f"weight_out[{d}]", o["weight"], w["weight_out"][d])]
        return [it for it in items if it[1] is not None]

    def assert_reference(self):
        for name, o, want in self.outputs():
            o.assert_holds(want, name)

    def assert_untouched(self):
        for name, o, _ in self.outputs():
            o.assert_holds(None, name)

    def run(self):
        _lib.check(self.launch(), "gte_batch_assemble")
        torch.cuda.synchronize()
        self.assert_reference()
        return self


# ---- run lengths ------------------------------------------------------------------------------------------------------------------
# From copy_run (csrc/batch_assemble.h), 256 threads: a run of n dwords is `head` = 0..3 single dwords up to the destination's next
# 16-byte boundary (at most n), body = (n - head) / 4 pieces of 16 bytes, and n - head - 4 body tail dwords.  Thread t takes pieces
# t, t + 256, ...: four at a time while c + 768 < body, then one at a time.  So the paths change at
#   n = 0 (nothing), 1..3 (head or tail only, head cut at n), 4, 5, 7, 8 (body of 0 or 1 piece by alignment), 15, 16, 17 (3..4 pieces)
#   body = 255, 256, 257     the last thread of the one-at-a-time loop has / has no piece; thread 0 takes a second one
#   body = 768, 769          769 is the first body whose thread 0 enters the four-at-a-time loop
#   body = 1023, 1024, 1025  every thread exactly four pieces at 1024; 1025: thread 0 goes on in the one-at-a-time loop
#   body = 2049              two rounds of the four-at-a-time loop and one more piece
# n = 4 body + k, k = 0..3, gives that body for every head <= k (k = 3: for every destination alignment).
SHORT_RUNS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17]
BODIES = [255, 256, 257, 768, 769, 1023, 1024, 1025, 2049]
RUN_LENGTHS = SHORT_RUNS + [4 * b + k for b in BODIES for k in range(4)]


def _run_length_triples():
    m = len(RUN_LENGTHS)
    triples = [(n, RUN_LENGTHS[(i + 5) % m] if n else 0, RUN_LENGTHS[(i + 11) % m] if n else 0) for i, n in enumerate(RUN_LENGTHS)]
    for d in (1, 2):                                       # (the page without nodes cannot carry its entry count: one more page)
        for missing in sorted(set(RUN_LENGTHS) - {t[d] for t in triples}):
            triples.append((1, missing, 0) if d == 1 else (1, 0, missing))
    for d in range(3):
        assert set(RUN_LENGTHS) <= {t[d] for t in triples}
    return triples


_SETS = {}


def resident(name):
    """the resident sets of this module, generated once each"""
    if name not in _SETS:
        if name == "runs":
            _SETS[name] = ref.make_resident(_run_length_triples(), n_cols=1, seed=1)
        elif name in ("geometry", "geometry_unweighted", "geometry_unlabelled"):
            # pages 0, 3, 4, 9: empty; 7: forty rows = five workgroups at 831 columns; the rest one to three rows
            triples = [(0, 0, 0), (2, 3, 1), (1, 0, 0), (0, 0, 0), (0, 0, 0), (3, 5, 7), (1, 1, 1), (40, 61, 58), (2, 0, 4), (0, 0, 0),
                       (3, 17, 2)]
            _SETS[name] = ref.make_resident(triples, n_cols=831, weighted=name != "geometry_unweighted",
                                            labelled=name != "geometry_unlabelled", seed=2)
    return _SETS[name]


def _bodies_of(out, b_off):
    """16-byte pieces of every run that starts at b_off[i] (dwords) of the output array ``out``"""
    got = set()
    for i in range(len(b_off) - 1):
        n = int(b_off[i + 1] - b_off[i])
        head = min((-(out.lo + int(b_off[i]))) % 4, n)
        got.add((n - head) // 4)
    return got


@pytest.mark.parametrize("out_off", [0, 1, 2, 3])
def test_every_run_length_at_every_destination_alignment(out_off):
    res = resident("runs")
    n_pages = len(res["node_off"]) - 1
    ids = np.random.default_rng(40 + out_off).permutation(n_pages)
    c = Call(res, ids, in_off=(3 * out_off + 1) % 4, out_off=out_off)
    sizes = np.diff(c.want["b_node_off"])
    assert set(RUN_LENGTHS) <= set(sizes.tolist()) and all(set(RUN_LENGTHS) <= set(np.diff(b).tolist()) for b in c.want["b_edge_off"])
    for o, b in ((c.label_out, c.want["b_node_off"]), (c.dir_out[0]["indices"], c.want["b_edge_off"][0]),
                 (c.dir_out[1]["weight"], c.want["b_edge_off"][1])):
        assert set(BODIES) <= _bodies_of(o, b)
    c.run()


# ---- widths -----------------------------------------------------------------------------------------------------------------------
# rows_per_wg = max(1, 32768 / (4 n_cols)): 8192, 2730, 2048, 1638, 630, 512, 130, 9, 9, 2, 1 and (8193: 0, clamped) 1
WIDTHS = [1, 3, 4, 5, 13, 16, 63, 831, 832, 4096, 4097, 8193]


def _width_triples(n_cols):
    """hundreds of pages of 1..3 nodes (one feature workgroup walks many of them), empty ones among them, and one page that spans
    many workgroups; a tenth of that for the widest rows (the same geometry in workgroups, 7 MB instead of 100)"""
    rng = np.random.default_rng(n_cols)
    small, big = (300, 3000) if n_cols <= 1024 else (40, 100)
    triples = []
    for k in range(small):
        n = int(rng.integers(0, 4)) if k % 10 else 0
        triples.append((n, int(rng.integers(0, 7)) if n else 0, int(rng.integers(0, 7)) if n else 0))
    triples.insert(small // 2, (big, 37, 41))
    return triples


@pytest.mark.parametrize("n_cols", WIDTHS)
def test_feature_rows_at_every_rows_per_workgroup(n_cols):
    triples = _width_triples(n_cols)
    res = ref.make_resident(triples, n_cols=n_cols, seed=n_cols)
    ids = np.random.default_rng(n_cols + 1).permutation(len(triples))
    c = Call(res, ids, in_off=n_cols % 4, out_off=(n_cols // 4 + 1) % 4)
    rows_per_wg = max(1, 32768 // (4 * n_cols))
    big = max(t[0] for t in triples)
    if n_cols > 1:
        assert big > rows_per_wg                                          # the large page meets a workgroup boundary
    assert c.n_out <= 4000
    c.run()


# ---- page geometry ----------------------------------------------------------------------------------------------------------------
GEOMETRY = {"empty_first": [0, 1, 7, 5], "empty_last": [5, 7, 1, 9], "empty_middle_and_two_in_a_row": [1, 3, 7, 4, 9, 5, 0, 0, 10],
            "one_page": [7], "one_small_page": [2], "a_page_twice": [5, 7, 5, 10, 7], "twice_in_a_row": [6, 6, 6],
            "descending": [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], "ascending": list(range(11))}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_page_geometry(name):
    ids = GEOMETRY[name]
    Call(resident("geometry"), ids, in_off=len(ids) % 4, out_off=(len(ids) + 2) % 4).run()
    Call(resident("geometry"), ids, in_off=1, out_off=3, row_map_pad=G.ROW_MAP_PAD).run()


# ---- variants ---------------------------------------------------------------------------------------------------------------------
IDS = [8, 0, 7, 5, 5, 3, 10, 1]


@pytest.mark.parametrize("dirs", [2, 1, 0], ids=["both_directions", "in_edges_only", "no_csr"])
@pytest.mark.parametrize("pad", [None, 0, 1, G.ROW_MAP_PAD], ids=["assemble", "map_pad0", "map_pad1", "map_pad_loop"])
def test_directions_and_row_map_padding(dirs, pad):
    c = Call(resident("geometry"), IDS, in_off=2, out_off=1, dirs=dirs, row_map_pad=pad).run()
    assert len(c.outputs()) == 2 + 3 * dirs + (pad is not None)


@pytest.mark.parametrize("pad", [None, 0, G.ROW_MAP_PAD], ids=["assemble", "map_pad0", "map_pad_loop"])
def test_unweighted_sets_write_ones_and_no_weight_out_writes_nothing(pad):
    c = Call(resident("geometry_unweighted"), IDS, in_off=3, out_off=2, row_map_pad=pad).run()
    assert all(c.descs[d].weight is None and c.descs[d].weight_out for d in range(2))
    assert (c.want["weight_out"][0] == 1.0).all() and c.want["weight_out"][0].size == c.want["e_out"][0] > 0
    for name in ("geometry", "geometry_unweighted"):
        c = Call(resident(name), IDS, in_off=0, out_off=3, weight_out=False, row_map_pad=pad).run()
        assert all(c.descs[d].weight_out is None for d in range(2)) and len(c.outputs()) == 6 + (pad is not None)


@pytest.mark.parametrize("pad", [None, 1], ids=["assemble", "map"])
def test_no_label(pad):
    c = Call(resident("geometry_unlabelled"), IDS, in_off=1, out_off=0, row_map_pad=pad).run()
    assert c.label is None and c.label_out is None


@pytest.mark.parametrize("pad", [0, 1, G.ROW_MAP_PAD])
@pytest.mark.parametrize("dirs", [2, 0])
def test_row_map_without_features(dirs, pad):
    """gte_batch_assemble_rows with feat == NULL: the map, labels and CSRs only (what a training step of the image path assembles)"""
    c = Call(resident("geometry"), IDS, in_off=pad % 4, out_off=dirs + 1, dirs=dirs, feat=False, row_map_pad=pad).run()
    assert c.feat is None and c.feat_out is None and c.row_map.n == c.n_out + pad
    assert c.want["row_map"][c.n_out:].tolist() == [c.n_res] * pad


# ---- n_out == 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [[0], [9, 3], [4, 0, 0, 9, 3]], ids=lambda v: "-".join(map(str, v)))
def test_a_batch_of_empty_pages_writes_indptr_zero_and_the_map_padding(ids):
    for kw in (dict(), dict(row_map_pad=G.ROW_MAP_PAD), dict(row_map_pad=G.ROW_MAP_PAD, feat=False), dict(row_map_pad=0, feat=False),
               dict(dirs=1, weight_out=False)):
        c = Call(resident("geometry"), ids, in_off=1, out_off=2, **kw).run()
        assert c.n_out == 0 and all(o["indptr"].n == 1 and c.want["indptr_out"][d].tolist() == [0] for d, o in enumerate(c.dir_out))
        if kw.get("row_map_pad"):
            assert c.want["row_map"].tolist() == [c.n_res] * G.ROW_MAP_PAD


# ---- the pieces: gte_batch_csr, gte_batch_rows ------------------------------------------------------------------------------------
def _csr_cases():
    return {"run_lengths": ("runs", None), "geometry": ("geometry", GEOMETRY["empty_middle_and_two_in_a_row"]),
            "descending": ("geometry", GEOMETRY["descending"]), "unweighted": ("geometry_unweighted", IDS),
            "no_entries": ("geometry", [2, 0, 2]), "one_page": ("geometry", [7]), "empty_pages": ("geometry", [0, 9])}


@pytest.mark.parametrize("name", list(_csr_cases()))
@pytest.mark.parametrize("weight_out", [True, False], ids=["weights", "no_weight_out"])
def test_batch_csr_equals_the_reference(name, weight_out):
    set_name, ids = _csr_cases()[name]
    res = resident(set_name)
    if ids is None:
        ids = np.random.default_rng(40).permutation(len(res["node_off"]) - 1)         # (the page list of the run-length test)
    w = want_of(res, ids)
    lib = _lib.load()
    pages, node_off, b_node_off = In(np.asarray(ids, dtype=np.int32), 1), In(res["node_off"], 2), In(w["b_node_off"], 3)
    for d, s in enumerate(res["dirs"]):
        n_out, e_out = w["n_out"], w["e_out"][d]
        edge_off, b_edge_off, indptr_loc, indices_loc = In(s["edge_off"], 0), In(w["b_edge_off"][d], 1), In(s["indptr_loc"], 2), In(s["indices_loc"], 3)
        weight = None if s["weight"] is None else In(s["weight"], 1)
        indptr, indices, wout = Out(n_out + 1, 1 + d), Out(e_out, 2 + d), Out(e_out, 3 - d)
        rc = lib.gte_batch_csr(pages.ptr, len(ids), node_off.ptr, edge_off.ptr, b_node_off.ptr, b_edge_off.ptr, indptr_loc.ptr,
                               indices_loc.ptr, weight.ptr if weight else None, indptr.ptr, indices.ptr, wout.ptr if weight_out else None,
                               n_out, e_out, _lib.current_stream())
        _lib.check(rc, "gte_batch_csr")
        torch.cuda.synchronize()
        indptr.assert_holds(w["indptr_out"][d], "indptr_out")
        indices.assert_holds(w["indices_out"][d], "indices_out")
        wout.assert_holds(w["weight_out"][d] if weight_out else None, "weight_out")


# scalar kernel below 16 and above 1024; one, two and four 16-byte pieces per lane: both ends of each range; 1030: scalar, f % 4 = 2
ROW_WIDTHS = [1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1030]


@pytest.mark.parametrize("n_cols", ROW_WIDTHS)
def test_batch_rows_equals_the_reference_and_leaves_the_columns_behind_alone(n_cols):
    not_x4 = lambda v: v + 1 if v % 4 == 0 else v
    ld_in, ld_out = not_x4(n_cols + 5), not_x4(n_cols + 2)
    assert ld_in % 4 and ld_out % 4 and ld_in != ld_out
    triples = [(0, 0, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0), (0, 0, 0), (3, 0, 0), (1, 0, 0), (30, 0, 0), (2, 0, 0), (0, 0, 0), (3, 0, 0)]
    res = ref.make_resident(triples, n_cols=ld_in, seed=n_cols)                       # the input matrix with its padding columns
    for ids in (GEOMETRY["empty_middle_and_two_in_a_row"], GEOMETRY["descending"], [7], [2]):
        w = ref.assemble_ref(res, ids)
        n_out = w["n_out"]
        want = np.full((n_out, ld_out), SENTINEL, dtype=np.int32)
        want[:, :n_cols] = ref.bits(w["feat_out"])[:, :n_cols]
        pages, node_off, b_node_off, inp = In(np.asarray(ids, dtype=np.int32), 3), In(res["node_off"], 1), In(w["b_node_off"], 2), In(res["feat"], n_cols % 4)
        out = Out(n_out * ld_out, (n_cols + 1) % 4)
        _lib.check(_lib.load().gte_batch_rows(pages.ptr, len(ids), node_off.ptr, b_node_off.ptr, inp.ptr, ld_in, out.ptr, ld_out, n_out,
                                              n_cols, _lib.current_stream()), "gte_batch_rows")
        torch.cuda.synchronize()
        out.assert_holds(want, f"rows of pages {ids}")


# ---- deferral into the fold launch ------------------------------------------------------------------------------------------------
def test_a_deferred_assembly_waits_for_the_flush_and_the_next_one_launches_itself():
    lib = _lib.load()
    res = resident("geometry")
    first = Call(res, GEOMETRY["empty_middle_and_two_in_a_row"], in_off=1, out_off=2)
    second = Call(res, GEOMETRY["descending"], in_off=2, out_off=3, row_map_pad=G.ROW_MAP_PAD, feat=False)
    direct = Call(res, GEOMETRY["a_page_twice"], in_off=3, out_off=0)
    other = Call(res, GEOMETRY["empty_last"], in_off=0, out_off=1, row_map_pad=1)
    side = torch.cuda.Stream(device=DEV)
    st = _lib.current_stream()
    assert side.cuda_stream != st
    torch.cuda.synchronize()
    is_open = False
    assert lib.gte_batch_assemble_defer(1) == 0
    try:
        # no deferral is open: the call launches
        _lib.check(direct.launch(), "direct")
        torch.cuda.synchronize()
        direct.assert_reference()
        _lib.check(lib.gte_fold_defer_begin(st), "gte_fold_defer_begin")
        is_open = True
        _lib.check(first.launch(), "deferred")
        torch.cuda.synchronize()
        first.assert_untouched()
        _lib.check(second.launch(), "second")                              # one job per deferral: this one launches on its own
        torch.cuda.synchronize()
        second.assert_reference()
        first.assert_untouched()
        is_open = False
        _lib.check(lib.gte_fold_defer_flush(), "gte_fold_defer_flush")
        torch.cuda.synchronize()
        first.assert_reference()
        second.assert_reference()
        # a deferral open on ANOTHER stream: the call launches on its own stream
        _lib.check(lib.gte_fold_defer_begin(side.cuda_stream), "gte_fold_defer_begin")
        is_open = True
        _lib.check(other.launch(), "other stream")
        torch.cuda.synchronize()
        other.assert_reference()
        is_open = False
        _lib.check(lib.gte_fold_defer_flush(), "gte_fold_defer_flush")
        torch.cuda.synchronize()
    finally:
        was = lib.gte_batch_assemble_defer(0)
        if is_open:
            lib.gte_fold_defer_flush()
        torch.cuda.synchronize()
    assert was == 1
    # defer(0) inside an open deferral: launched at once
    again = Call(res, IDS, in_off=1, out_off=1)
    _lib.check(lib.gte_fold_defer_begin(st), "gte_fold_defer_begin")
    try:
        _lib.check(again.launch(), "defer off")
        torch.cuda.synchronize()
        again.assert_reference()
    finally:
        _lib.check(lib.gte_fold_defer_flush(), "gte_fold_defer_flush")
        torch.cuda.synchronize()


# ---- through Python: ResidentPages.batch --------------------------------------------------------------------------------------------
def _hand_page(n, edges, in_feats, seed):
    rng = np.random.default_rng(seed)
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return S.Page(e[:, 0].copy(), e[:, 1].copy(), (0.25 + rng.random(len(e)) / 2).astype(np.float32),
                  rng.standard_normal((n, in_feats)).astype(np.float32), rng.integers(0, 9, n).astype(np.int64), np.zeros((n, 4), dtype=np.int32))


def _python_pages(in_feats=21):
    """a one-node page without edges, a page with an isolated node (3), ordinary pages, one directed edge"""
    return [_hand_page(1, [], in_feats, 1), _hand_page(4, [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)], in_feats, 2),
            S.make_page(0, in_feats=in_feats, n_words=23), _hand_page(2, [(1, 0)], in_feats, 3), S.make_page(1, in_feats=in_feats, n_words=37),
            _hand_page(1, [], in_feats, 4)]


def _graphs(pages):
    gs = []
    for p in pages:
        g = G.PageGraph(p.src, p.dst, p.num_nodes)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
        g.edata["feat"] = torch.from_numpy(p.weight)
        gs.append(g)
    return gs


PY_IDS = [[0], [5, 0], [3, 1, 0, 2, 5, 1, 4], [4, 3, 2, 1, 0], [1]]


def _assert_csrs_and_labels(rb, want):
    host = lambda t: t.cpu().numpy()
    for d, csr in enumerate((rb.in_csr(), rb.out_csr())):
        np.testing.assert_array_equal(host(csr.indptr), want["indptr_out"][d])
        np.testing.assert_array_equal(host(csr.indices), want["indices_out"][d])
    np.testing.assert_array_equal(ref.bits(host(rb.in_weights(rb.edata["feat"]))), ref.bits(want["weight_out"][0]))
    np.testing.assert_array_equal(ref.bits(host(rb.out_weights(rb.edata["feat"], True))), ref.bits(want["weight_out"][1]))
    np.testing.assert_array_equal(ref.bits(host(rb.ndata["label"])), ref.bits(want["label_out"]))
    assert rb.num_nodes() == want["n_out"] and rb.num_edges() == want["e_out"][0]


@pytest.mark.parametrize("mode", ["fp32", "rows", "copy"])
def test_resident_pages_batch_with_one_word_pages_equals_the_reference(mode, monkeypatch):
    pages = _python_pages()
    res = ref.resident_from_pages(pages, oc.coo_to_in_csr)
    rp = G.ResidentPages(_graphs(pages), DEV)
    assert rp.max_deg["in"] == int(max(np.diff(oc.coo_to_in_csr(p.src, p.dst, p.num_nodes)[0]).max() for p in pages))
    if mode != "fp32":
        monkeypatch.setenv("GTE_P3_ROWS", "1" if mode == "rows" else "0")
        rp.enable_p3()
        assert rp.p3_mode == mode
    for ids in PY_IDS:
        want = ref.assemble_ref(res, ids, G.ROW_MAP_PAD, rp.n_nodes)
        rb = rp.batch(ids)
        torch.cuda.synchronize()
        _assert_csrs_and_labels(rb, want)
        assert rb.batch_num_nodes().tolist() == [pages[i].num_nodes for i in ids]
        if mode == "fp32":
            np.testing.assert_array_equal(ref.bits(rb.ndata["feat"].cpu().numpy()), ref.bits(want["feat_out"]))
        elif mode == "rows":
            assert "feat" not in rb.ndata and rb.feat_p3.res_rows == rp.n_nodes and rb.feat_p3.rows == want["n_out"]
            np.testing.assert_array_equal(rb.feat_p3.row_map.cpu().numpy(), want["row_map"])
        else:
            assert "feat" not in rb.ndata and rb.feat_p3.row_map is None and rb.feat_p3.rows == want["n_out"]
            rows = torch.from_numpy(want["row_map"][:want["n_out"]].astype(np.int64)).to(DEV)
            assert torch.equal(rb.feat_p3.data[:want["n_out"]], rp.feat_p3.data[rows])
