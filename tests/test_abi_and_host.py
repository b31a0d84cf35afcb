"""CPU-only: the C-ABI library loads and exports every symbol include/gte.h declares; host-side
graph logic (CSR build, batching, duck type) against the oracle's own CSR builder; the product
path refuses to run without a device (no silent fallback)."""
import os
import re

import numpy as np
import pytest
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.components.features.utils import calculate_hidden, get_in_feats_
from gnn_tableextraction_amd.data import synthetic as S
from oracle import gcnsage_cpu as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "gte.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gte_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = declared_symbols()
    assert len(syms) >= 16
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/gte.h but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert lib.gte_version() == 400
    assert lib.gte_coo_to_csr_workspace_bytes(1000, 8000) > 2 * 8000 * 4
    assert lib.gte_weighted_ce_workspace_bytes(1000) >= 4 * 3 * 4


def test_layer_kind_names_mirror_the_header_enum():
    text = open(os.path.join(ROOT, "include", "gte.h")).read()
    enum = dict(re.findall(r"GTE_(LAYER_[A-Z]+) = (\d+)", re.search(r"enum gte_layer_kind \{(.*?)\}", text).group(1)))
    assert len(enum) == 5
    for name, value in enum.items():
        assert getattr(_lib, name) == int(value)


def test_which_products_take_the_block_major_weights_kernel():
    """gte_gemm_p3_nt_plan (host logic only, run here without a GPU): the dispatch rule of the NT planes GEMMs.  The headline step's
    layer-0 forward ([x | cached ahn] W^T, K = 2 x 831, LayerNorm epilogue) and dX + LayerNorm backward (K = 2 x 256) take the
    block-major-weights kernel on the smallest row tile that covers the batch in one round of 256 CUs; products with several
    columns of tiles, short K loops, row-major weights and badly padded K do not."""
    import ctypes
    lib = _lib.load()

    def plan(m, n, k1, k2, bm=1, epi=0):
        rt = ctypes.c_int(-1)
        r = lib.gte_gemm_p3_nt_plan(m, n, k1, k2, bm, epi, 256, ctypes.byref(rt))
        return r, rt.value
    assert plan(24400, 256, 831, 831, epi=4) == (1, 96)            # layer-0 forward of the headline, <= 24 576 rows
    assert plan(25300, 256, 831, 831, epi=4) == (1, 128)           # ... above: 128-row tiles on 198 CUs
    assert plan(24400, 256, 256, 256, epi=1) == (1, 96)            # dX + LayerNorm backward of layer 0
    assert plan(12000, 256, 831, 831, epi=4) == (1, 64) and plan(6000, 256, 831, 831, epi=4) == (1, 32)
    assert plan(24400, 256, 831, 831, bm=0, epi=4) == (0, 96)      # row-major weights: the loader-wave kernel
    assert plan(24400, 512, 256, 0) == (0, 0)                      # layer-1 forward: two columns of tiles
    assert plan(22500, 192, 831, 0) == (1, 96)                     # (831, 96): the narrow input GEMM, 2 x 96 columns
    assert plan(22500, 96, 831, 0)[0] == 0                         # half-empty tile column: the tile chooser
    assert plan(24400, 218, 218, 218, epi=3) == (0, 96)            # 2 x 14 K blocks: below 32 (the row tile rule is the epilogue launches')
    assert plan(24400, 256, 144, 0, epi=1)[0] == 0                 # 9 K blocks
    assert plan(24400, 160, 363, 363, epi=4) == (1, 96)            # 46 blocks in slots of four: padded to 48 (4 %)
    assert plan(24400, 256, 272, 272, epi=1) == (1, 96)            # 34 blocks padded to 36: 5.9 % <= 1 / 12
    assert plan(24400, 256, 528, 0, epi=1)[0] == 0                 # 33 blocks padded to 36: 9.1 % > 1 / 12
    assert lib.gte_gemm_p3_nt_plan(10, 10, 0, 0, 1, 0, 256, None) == -1 and lib.gte_gemm_p3_nt_plan(10, 10, 16, 0, 1, 2, 256, None) == -1


def test_bad_arguments_return_error_codes_not_crashes():
    lib = _lib.load()
    rc = lib.gte_spmm_csr(None, None, None, None, 4, None, 4, 10, 4, 0, 0, None)
    assert rc == -1 and b"null" in lib.gte_last_error()
    rc = lib.gte_spmm_csr(None, None, None, None, 2, None, 4, 10, 4, 0, 7, None)
    assert rc == -1
    assert lib.gte_adam_step(None, None, None, None, 10, 0.01, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, None) == -1
    with pytest.raises(_lib.GteError):
        _lib.check(rc, "probe")


def test_workspace_queries_cover_every_smaller_node_count():
    """The step engine sizes its workspaces ONCE for a node capacity and runs any batch up to it: every workspace query
    must be non-decreasing in the node count.  (The split-K slab count of a plan is not -- 896 K tiles give 35 splits,
    846 give 36 -- so the queries answer with the plan's monotonic bound; a 64-wide hidden layer once came out 2.8 % short.)"""
    lib = _lib.load()
    rng = np.random.default_rng(0)
    queries = [
        lambda n: lib.gte_sage_qform_dw_workspace_bytes(64, 831, n), lambda n: lib.gte_sage_qform_dw_workspace_bytes(256, 831, n),
        lambda n: lib.gte_sage_qform_dw_workspace_bytes(256, 256, n), lambda n: lib.gte_sage_qform_dw_workspace_bytes(1000, 831, n),
        lambda n: lib.gte_sage_linear_dw_workspace_bytes(256, 831, 831, n), lambda n: lib.gte_sage_linear_dw_workspace_bytes(64, 13, 13, n),
        lambda n: lib.gte_gemm_workspace_bytes(256, 831, n), lambda n: lib.gte_gemm_workspace_bytes(9, 256, n),
        lambda n: lib.gte_ln_relu_bwd_workspace_bytes(n, 256), lambda n: lib.gte_weighted_ce_workspace_bytes(n),
        lambda n: lib.gte_sage_narrow_bwd_workspace_bytes(n, 256, 9), lambda n: lib.gte_head_agg_ce_workspace_bytes(n),
        lambda n: lib.gte_sage_narrow_bwd_ln_workspace_bytes(n, 256),
    ]
    sizes = sorted(set(rng.integers(1, 120_000, 400).tolist() + [1, 31, 32, 33, 27060, 28672, 100_000]))
    for q in queries:
        vals = [q(n) for n in sizes]
        assert all(a <= b for a, b in zip(vals, vals[1:])), [(n, v) for n, v in zip(sizes, vals)][:5]


def test_no_cpu_fallback():
    g = G.PageGraph([0, 1], [1, 0], 2)
    g.ndata["h"] = torch.ones(2, 4)
    g.edata["feat"] = torch.ones(2)
    with pytest.raises(_lib.GteError):
        g.update_all(gte.function.u_mul_e("h", "feat", "m"), gte.function.sum("m", "h"))
    model = gte.GcnSAGE(4, 8, 9, 2, torch.relu, 0)
    g.ndata["feat"] = torch.ones(2, 4)
    with pytest.raises(_lib.GteError):
        model(g)


def test_host_csr_matches_oracle_builder():
    rng = np.random.default_rng(0)
    n, e = 50, 400
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    g = G.PageGraph(src, dst, n)
    ip, ix, _, perm = oc.coo_to_in_csr(src, dst, n)
    csr = g.in_csr()
    np.testing.assert_array_equal(csr.indptr.numpy(), ip)
    np.testing.assert_array_equal(csr.indices.numpy(), ix)
    np.testing.assert_array_equal(csr.perm.numpy(), perm)
    rip, rix, _, _ = oc.coo_to_in_csr(dst, src, n)
    np.testing.assert_array_equal(g.out_csr().indptr.numpy(), rip)
    np.testing.assert_array_equal(g.out_csr().indices.numpy(), rix)
    np.testing.assert_array_equal(g.in_degrees().numpy(), np.bincount(dst, minlength=n))
    np.testing.assert_allclose(g.inv_in_degree().numpy(), oc.in_degree_norm(ip)[:, 0])
    w = torch.from_numpy(rng.random(e).astype(np.float32))
    np.testing.assert_array_equal(g.in_weights(w).numpy(), w.numpy()[perm])


def test_batch_is_block_diagonal_and_reuses_csr():
    pages = S.make_pages(4, in_feats=13)
    gs = []
    for p in pages:
        g = G.PageGraph(p.src, p.dst, p.num_nodes)
        g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label)
        g.edata["feat"] = torch.from_numpy(p.weight)
        g.in_csr(), g.out_csr()
        gs.append(g)
    b = G.batch(gs)
    src, dst, w, feat, label, off = S.concat_pages(pages)
    assert b.num_nodes() == off[-1] and b.num_edges() == len(src)
    np.testing.assert_array_equal(b.ndata["feat"].numpy(), feat)
    np.testing.assert_array_equal(b.edata["feat"].numpy(), w)
    ip, ix, _, perm = oc.coo_to_in_csr(src, dst, int(off[-1]))
    assert b._in_csr is not None          # concatenated, not re-sorted
    np.testing.assert_array_equal(b.in_csr().indptr.numpy(), ip)
    np.testing.assert_array_equal(b.in_csr().indices.numpy(), ix)
    np.testing.assert_array_equal(b.in_csr().perm.numpy(), perm)
    fresh = G.PageGraph(src, dst, int(off[-1]))
    np.testing.assert_array_equal(fresh.out_csr().indices.numpy(), b.out_csr().indices.numpy())
    assert b.batch_num_nodes().tolist() == [p.num_nodes for p in pages]
    # no edge crosses a page
    page_of = np.searchsorted(off, np.arange(off[-1]), side="right")
    assert (page_of[src] == page_of[dst]).all()


def test_graph_duck_type_surface():
    g = G.graph(([0, 1, 2], [1, 2, 0]), num_nodes=4)
    assert g.num_nodes() == 4 and g.number_of_edges() == 3
    lv = g.local_var()
    lv.ndata["h"] = torch.zeros(4, 2)
    assert "h" not in g.ndata and lv.ndata.pop("h").shape == (4, 2)
    with g.local_scope():
        g.ndata["tmp"] = torch.zeros(4)
    assert "tmp" not in g.ndata
    assert g.in_degrees().tolist() == [1, 1, 1, 0]
    assert g.to("cpu") is g


def test_synthetic_pages_follow_the_contract():
    p = S.make_page(3, in_feats=831)
    assert p.feat.shape == (p.num_nodes, 831) and p.feat.dtype == np.float32
    assert 20 <= p.num_nodes <= 2000 and p.label.max() < 9
    assert p.weight.min() >= 0 and p.weight.max() <= 1
    pairs = set(zip(p.src.tolist(), p.dst.tolist()))
    assert len(pairs) == len(p.src)                       # to_simple
    assert all((b, a) in pairs for a, b in pairs)         # to_bidirected
    d = S.box_distance_matrix(p.bbox)
    assert (d[p.dst, p.src] <= 500).all()
    q = S.make_page(3, in_feats=831)
    np.testing.assert_array_equal(p.feat, q.feat)         # seeded
    assert S.make_page(0, n_words=200).num_nodes == 200


def test_box_distance_hand_cases():
    b = np.array([[0, 0, 10, 10], [20, 0, 30, 10], [13, 14, 20, 20], [5, 5, 8, 8], [10, 10, 12, 12]])
    d = S.box_distance_matrix(b)
    assert d[0, 1] == 10          # side by side: horizontal gap
    assert d[0, 2] == 5           # diagonal 3,4 -> int(sqrt(25))
    assert d[0, 3] == 0           # contained
    assert d[0, 4] == 0           # touching corners count as intersecting
    assert (d == d.T).all()


def test_shape_helpers():
    class C:
        class PREPROCESS:
            padding = False
            features = ["BBOX", "REPR", "SCIBERT"]
    assert get_in_feats_(C) == 831
    C.PREPROCESS.features = ["BBOX"]
    assert get_in_feats_(C) == 13
    C.PREPROCESS.padding = True
    assert get_in_feats_(C) == 831
    for args in [(13, 9, 100000, 3), (831, 9, 100000, 3), (10000, 8, 100000, 3)]:
        assert calculate_hidden(*args) == pytest.approx(oc.calculate_hidden(*args), rel=1e-12)
    assert int(calculate_hidden(13, 9, 100000, 3)) == 218 and int(calculate_hidden(831, 9, 100000, 3)) == 96


@pytest.mark.parametrize("name,seed", [("page200_f13_l2", 2), ("page200_f13_l3_cw", 3), ("page300_f831_l3", 4)])
def test_parameter_init_reproduces_the_reference_rng_stream(name, seed):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    n, f0, hid, ncls, nl, _ = z["meta"]
    torch.manual_seed(seed)
    m = gte.GcnSAGE(int(f0), int(hid), int(ncls), int(nl), torch.nn.functional.relu, 0)
    sd = m.state_dict()
    ref_keys = sorted(k[len("state0."):] for k in z.files if k.startswith("state0."))
    assert sorted(sd.keys()) == ref_keys                  # checkpoint-compatible key set
    for k in ref_keys:
        np.testing.assert_array_equal(sd[k].numpy(), z["state0." + k])


# ---------------------------------------------------------------- bench.py host logic (no GPU)
def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_bench_gpus_flag_must_agree_with_the_launcher(monkeypatch):
    import argparse
    b = _bench()
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(SystemExit):
        b.maybe_spawn(argparse.Namespace(gpus=2))            # torchrun started 4 ranks, the flag says 2: loud, not silent
    b.maybe_spawn(argparse.Namespace(gpus=4))                # agreeing: returns, the rank continues
    monkeypatch.delenv("WORLD_SIZE")
    b.maybe_spawn(argparse.Namespace(gpus=1))                # one GPU: nothing to start
    monkeypatch.setattr(b.torch.cuda, "device_count", lambda: 1)
    with pytest.raises(SystemExit):
        b.maybe_spawn(argparse.Namespace(gpus=8))            # more ranks than GPUs on this node


def test_bench_epoch_steps_follow_the_train_loop_plan():
    b = _bench()
    from gnn_tableextraction_amd import distributed as D
    sizes = list(np.random.default_rng(0).integers(20, 2000, 530))
    epochs, nxt = b.epoch_steps(sizes, 100, 42, 3, 12)       # 5 steps per epoch (tail of 30 pages dropped), 12 steps wanted
    assert [len(e) for e in epochs] == [5, 5, 2] and nxt == 6
    want = [r[0] for r in D.plan_epoch(sizes, 100, 1, seed=42, epoch=3)]
    assert all((a == w).all() for a, w in zip(epochs[0], want))
    flat = [i for e in epochs[:1] for ids in e for i in ids.tolist()]
    assert len(set(flat)) == len(flat) == 500                # an epoch never revisits a page


def test_bench_output_dump_is_float_and_bounded(tmp_path):
    """bench.py --dump-outputs: float32 files (float64 kept), and above the size limit a seeded sample -- the same elements in
    every run -- of each array larger than its share."""
    b = _bench()
    big = np.arange(5000, dtype=np.float64).reshape(50, 100)
    arrays = {"a": torch.arange(6, dtype=torch.int64), "b": big, "c": np.ones(10, np.float16)}
    assert b.write_outputs(str(tmp_path / "x"), arrays) == ["a", "b", "c"]
    got = {k: np.load(tmp_path / "x" / f"{k}.npy") for k in "abc"}
    assert got["a"].dtype == np.float32 and got["c"].dtype == np.float32 and got["b"].dtype == np.float64
    np.testing.assert_array_equal(got["b"], big)
    b.write_outputs(str(tmp_path / "y"), arrays, max_bytes=3000)
    b.write_outputs(str(tmp_path / "z"), arrays, max_bytes=3000)
    y, z = (np.load(tmp_path / d / "b.npy") for d in "yz")
    assert y.nbytes <= 1000 and np.array_equal(y, z) and np.isin(y, big).all() and (np.diff(y) > 0).all()
    np.testing.assert_array_equal(np.load(tmp_path / "y" / "a.npy"), np.arange(6, dtype=np.float32))


def test_the_shipped_library_reads_one_environment_variable():
    """no globals besides a read-only device-props cache.  The measurement switches of earlier rounds (17 getenv reads)
    are compiled into libgte_hip_measure.so only; the shipped library holds the name of ONE variable, GTE_GEMM_MODE (include/gte.h),
    and both builds export the same symbols."""
    import re
    import subprocess
    lib = os.path.join(ROOT, "gnn-tableextraction_amd", "libgte_hip.so")
    names = set(re.findall(rb"(?<![A-Z0-9_])GTE_[A-Z0-9_]{3,}(?=\x00)", open(lib, "rb").read()))
    assert names == {b"GTE_GEMM_MODE"}, names
    measure = os.path.join(ROOT, "gnn-tableextraction_amd", "libgte_hip_measure.so")
    if os.path.exists(measure):
        syms = lambda p: {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", p], capture_output=True, text=True).stdout.splitlines()
                          if " T " in l and l.split()[-1].startswith("gte_")}
        assert syms(lib) == syms(measure) and len(syms(lib)) > 100
        assert len(set(re.findall(rb"(?<![A-Z0-9_])GTE_[A-Z0-9_]{3,}(?=\x00)", open(measure, "rb").read()))) >= 15


def test_no_kernel_of_the_library_spills():
    """Every kernel of libgte_hip.so keeps its working set in registers: ScratchSize == 0 in hipcc's kernel-resource-usage remarks
    (csrc/_build/*.ru, written by the Makefile next to every object; compiled here when the logs are missing).  Round 3 shipped
    two spilling instantiations on dispatchable paths (a 192-row tile with a LayerNorm-backward epilogue: 140 bytes per lane; the
    class-count-wide TN GEMM: 148)."""
    import glob
    import sys
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import resource_usage as ru
    import hashlib
    csrc = os.path.join(ROOT, "gnn-tableextraction_amd", "csrc")
    hdrs = sorted(os.path.basename(h) for h in glob.glob(os.path.join(csrc, "*.h"))) + ["../../include/gte.h"]   # Makefile: HDRS (every header)
    table = {}
    for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        log = os.path.join(csrc, "_build", os.path.basename(src)[:-4] + ".ru")
        # a log is trusted by the key on its first line (sha256 of the source + headers it came from), never by its mtime
        key = hashlib.sha256(b"".join(open(os.path.join(csrc, f), "rb").read() for f in [os.path.basename(src)] + hdrs)).hexdigest()
        text = open(log).read() if os.path.exists(log) else ""
        if text.startswith(f"# key {key}"):
            table.update(ru.parse(text))
        else:
            table.update(ru.compile_usage(src))
    assert len(table) > 150, "kernel-resource-usage remarks not found"
    # (rocPRIM's radix sort inside gte_coo_to_csr / gte_knn_csr -- the vendor's header library, once per graph, off the step path --
    # spills 80 bytes in its onesweep kernels: not ours to fix)
    spills = {k: v["scratch"] for k, v in table.items() if v.get("scratch", 0) > 0 and "7rocprim" not in k}
    assert not spills, f"kernels with scratch memory: {spills}"
    # the planes GEMMs of the step keep one or two workgroups per CU: occupancy as designed
    names = ru.demangle(list(table))
    p3 = [k for k in table if "gemm_p3_" in names[k]]
    assert p3 and all(table[k]["vgprs"] + table[k].get("agprs", 0) <= 512 for k in p3)


# ---------------------------------------------------------------- the planes GEMMs' argument checks (no GPU)
_P = 0x10000          # a dummy address: every call of the table returns before anything dereferences it or launches a kernel
_L22, _L23 = 1 << 22, 1 << 23
_P3_PARAMS = {
    "gte_gemm_p3_nt": "a1 lda1 k1 a2 lda2 k2 b ldb bias bias_cols c ldc m n relu accumulate stream",
    "gte_gemm_p3_nt_rows": "a_res ldpa k a_rows n_res_rows b ldpb bias bias_cols c ldc m n relu accumulate stream",
    "gte_gemm_p3_nt_rows2": "a_res ldpa a2_res ldpa2 k a_rows n_res_rows b ldpb bias bias_cols c ldc m n relu accumulate stream",
    "gte_gemm_p3_nt_ln_fwd": "a1 lda1 k1 a2 lda2 k2 b ldb bias gamma beta eps relu z ldz y ldy yp3 ldyp3 stats m n stream",
    "gte_gemm_p3_nt_rows2_ln_fwd": "a_res ldpa a2_res ldpa2 k a_rows n_res_rows b ldb bias gamma beta eps relu z ldz y ldy yp3 ldyp3 "
                                   "stats m n stream",
    "gte_gemm_p3_nt_ln_bwd": "a1 lda1 k1 a2 lda2 k2 b ldb z ldz stats gamma beta relu dz lddz dzp3 ldp3 dgamma dbeta dbias m n "
                             "workspace workspace_bytes stream",
    "gte_gemm_p3_nt_smallk_bwd": "a1 lda1 kg1 a2 lda2 kg2 b ldb x ldx k1 ahn ldahn k2 W ldw bias gamma beta stats relu dW lddw dbias "
                                 "dgamma dbeta m n workspace workspace_bytes stream",
    "gte_gemm_p3_tn": "a lda a2 lda2 b ldb b2 ldb2 nseg c ldc m n k workspace workspace_bytes stream",
    "gte_gemm_p3_tn_rows": "a ldpa a2 ldpa2 b_res ldpb b_rows n_res_rows nseg c ldc m n k workspace workspace_bytes stream",
    "gte_gemm_p3_tn_rows2": "a ldpa b_res ldpb b2_res ldpb2 b_rows n_res_rows nseg c ldc m n k workspace workspace_bytes stream",
}


def _p3_valid_calls(lib):
    """A VALID argument set per entry point (never issued as it stands: it would launch).  NT: m = 100, n = 64, K = 32 (two blocks:
    192-byte rows; 384 with two segments); TN: m = n = 128 over k = 512 rows: four K splits on any device with two CUs or more."""
    out = dict(bias=None, bias_cols=0, c=_P, ldc=64, m=100, n=64, relu=0, accumulate=0, stream=None)
    ln_f = dict(bias=None, gamma=_P, beta=_P, eps=1e-5, relu=1, z=_P, ldz=64, y=_P, ldy=64, yp3=_P, ldyp3=384, stats=_P, m=100, n=64, stream=None)
    seg1 = dict(a1=_P, lda1=192, k1=32, a2=None, lda2=0, k2=0, b=_P, ldb=192)
    res2 = dict(a_res=_P, ldpa=192, a2_res=_P, ldpa2=192, k=32, a_rows=_P, n_res_rows=1000, b=_P)
    tn_ws = 4 * 128 * 128 * 4
    tn_out = dict(c=_P, ldc=128, m=128, n=128, k=512, workspace=_P, workspace_bytes=tn_ws, stream=None)
    return {
        "gte_gemm_p3_nt": dict(seg1, **out),
        "gte_gemm_p3_nt_rows": dict(a_res=_P, ldpa=192, k=32, a_rows=_P, n_res_rows=1000, b=_P, ldpb=192, **out),
        "gte_gemm_p3_nt_rows2": dict(res2, ldpb=384, **out),
        "gte_gemm_p3_nt_ln_fwd": dict(seg1, **ln_f),
        "gte_gemm_p3_nt_rows2_ln_fwd": dict(res2, ldb=384, **ln_f),
        "gte_gemm_p3_nt_ln_bwd": dict(seg1, z=_P, ldz=64, stats=_P, gamma=_P, beta=_P, relu=1, dz=_P, lddz=64, dzp3=_P, ldp3=384, dgamma=_P,
                                      dbeta=_P, dbias=_P, m=100, n=64, workspace=_P,
                                      workspace_bytes=lib.gte_gemm_p3_nt_ln_bwd_workspace_bytes(100, 64), stream=None),
        "gte_gemm_p3_nt_smallk_bwd": dict(a1=_P, lda1=192, kg1=32, a2=None, lda2=0, kg2=0, b=_P, ldb=192, x=_P, ldx=13, k1=13, ahn=_P, ldahn=13,
                                          k2=13, W=_P, ldw=26, bias=_P, gamma=_P, beta=_P, stats=_P, relu=1, dW=_P, lddw=26, dbias=_P,
                                          dgamma=_P, dbeta=_P, m=100, n=64, workspace=_P,
                                          workspace_bytes=lib.gte_gemm_p3_nt_smallk_bwd_workspace_bytes(100, 26, 64), stream=None),
        "gte_gemm_p3_tn": dict(a=_P, lda=768, a2=None, lda2=0, b=_P, ldb=768, b2=None, ldb2=0, nseg=0, **tn_out),
        "gte_gemm_p3_tn_rows": dict(a=_P, ldpa=768, a2=None, ldpa2=0, b_res=_P, ldpb=768, b_rows=_P, n_res_rows=1000, nseg=0, **tn_out),
        "gte_gemm_p3_tn_rows2": dict(a=_P, ldpa=768, b_res=_P, ldpb=384, b2_res=_P, ldpb2=384, b_rows=_P, n_res_rows=1000, nseg=64, **tn_out),
    }


def _p3_invalid_calls(lib):
    """(entry point, what is wrong with the valid call, return code).  -1 invalid argument, -3 workspace too small, -4 unsupported,
    0 nothing to do.  A call that passes a check it is meant to PASS (a stride one below the limit, the last row count below
    2 GB) is wrong in a way that is only looked at later -- an empty resident image, a workspace one byte short -- so that it
    still returns before a launch; the plain gte_gemm_p3_nt / _nt_ln_fwd have no later check, their limits are those of the
    row-map forms, which run the same code."""
    ln_ws, sk_ws = lib.gte_gemm_p3_nt_ln_bwd_workspace_bytes, lambda m: lib.gte_gemm_p3_nt_smallk_bwd_workspace_bytes(m, 26, 64)
    tn_ws = 4 * 128 * 128 * 4
    two = dict(k2=16, a2=_P, lda2=96, ldb=288)             # a second K segment of one block
    nt, rows, rows2 = "gte_gemm_p3_nt", "gte_gemm_p3_nt_rows", "gte_gemm_p3_nt_rows2"
    lnf, lnf2, lnb, sk = "gte_gemm_p3_nt_ln_fwd", "gte_gemm_p3_nt_rows2_ln_fwd", "gte_gemm_p3_nt_ln_bwd", "gte_gemm_p3_nt_smallk_bwd"
    tn, tnr, tnr2 = "gte_gemm_p3_tn", "gte_gemm_p3_tn_rows", "gte_gemm_p3_tn_rows2"
    t = []
    # ---- gte_gemm_p3_nt
    t += [(nt, dict(m=-1), -1), (nt, dict(n=-1), -1), (nt, dict(k1=0), -1), (nt, dict(k2=-1), -1), (nt, dict(m=1 << 31), -1),
          (nt, dict(m=0, a1=None), 0), (nt, dict(n=0, c=None), 0),
          (nt, dict(a1=None), -1), (nt, dict(b=None), -1), (nt, dict(c=None), -1), (nt, dict(two, a2=None), -1),
          (nt, dict(lda1=191), -1), (nt, dict(two, lda2=95), -1), (nt, dict(ldb=176), -1), (nt, dict(ldb=-(64 * 96 - 16)), -1),
          (nt, dict(ldc=63), -1),
          (nt, dict(lda1=_L22), -4), (nt, dict(lda2=_L22), -4), (nt, dict(ldb=_L22), -4), (nt, dict(m=256, ldc=1 << 20), -4),
          (nt, dict(lda1=191, ldb=_L22), -1), (nt, dict(c=None, lda1=_L22), -1), (nt, dict(m=-1, lda1=_L22), -1),
          (nt, dict(m=0, lda1=_L22), 0)]
    # ---- gte_gemm_p3_nt_rows / _rows2
    t += [(rows, dict(a_rows=None), -1), (rows, dict(a_rows=None, ldpa=_L22), -1), (rows, dict(k=0), -1), (rows, dict(a_res=None), -1),
          (rows, dict(ldpa=191), -1), (rows, dict(ldpb=176), -1), (rows, dict(ldpa=_L22), -4), (rows, dict(ldpa=_L22 - 1, n_res_rows=0), -1),
          (rows, dict(ldpb=_L22), -4), (rows, dict(ldpb=_L22 - 16, n_res_rows=0), -1),
          (rows, dict(m=256, ldc=1 << 20, n_res_rows=0), -4), (rows, dict(m=256, ldc=(1 << 20) - 1, n_res_rows=0), -1),
          (rows, dict(n_res_rows=0), -1), (rows, dict(n_res_rows=-5), -1), (rows, dict(ldpa=_L22, n_res_rows=0), -4),
          (rows, dict(m=0, n_res_rows=0), 0),
          (rows2, dict(a_rows=None), -1), (rows2, dict(a2_res=None), -1), (rows2, dict(a2_res=None, ldpa=_L22), -1),
          (rows2, dict(ldpa2=191), -1), (rows2, dict(ldpb=368), -1), (rows2, dict(ldpa2=_L22), -4),
          (rows2, dict(ldpa2=_L22 - 1, n_res_rows=0), -1), (rows2, dict(n_res_rows=0), -1), (rows2, dict(ldpa=_L22, n_res_rows=0), -4)]
    # ---- gte_gemm_p3_nt_ln_fwd / _rows2_ln_fwd
    t += [(lnf, dict(m=-1), -1), (lnf, dict(n=0), -1), (lnf, dict(n=257, ldz=260, ldy=260, ldyp3=1632), -1), (lnf, dict(k1=0), -1),
          (lnf, dict(k2=-1), -1), (lnf, dict(m=0, a1=None), 0),
          (lnf, dict(a1=None), -1), (lnf, dict(b=None), -1), (lnf, dict(z=None), -1), (lnf, dict(gamma=None), -1), (lnf, dict(beta=None), -1),
          (lnf, dict(y=None, yp3=None), -1), (lnf, dict(two, a2=None), -1),
          (lnf, dict(lda1=191), -1), (lnf, dict(two, lda2=95), -1), (lnf, dict(ldb=176), -1), (lnf, dict(ldz=63), -1), (lnf, dict(ldy=63), -1),
          (lnf, dict(n=62, ldz=63), -1), (lnf, dict(ldyp3=368), -1), (lnf, dict(ldyp3=392), -1),
          (lnf, dict(lda1=_L22), -4), (lnf, dict(lda2=_L22), -4), (lnf, dict(ldb=_L22), -4),
          (lnf, dict(n=257, lda1=_L22), -1), (lnf, dict(z=None, lda1=_L22), -1), (lnf, dict(ldz=63, ldb=_L22), -1),
          (lnf2, dict(a_rows=None), -1), (lnf2, dict(a2_res=None), -1), (lnf2, dict(a_rows=None, ldpa=_L22), -1),
          (lnf2, dict(n_res_rows=0), -1), (lnf2, dict(ldpa=_L22, n_res_rows=0), -4), (lnf2, dict(ldpa=_L22 - 1, n_res_rows=0), -1),
          (lnf2, dict(ldpa2=_L22, n_res_rows=0), -4), (lnf2, dict(ldpa2=_L22 - 1, n_res_rows=0), -1),
          (lnf2, dict(ldb=_L22 - 16, n_res_rows=0), -1), (lnf2, dict(z=None, n_res_rows=0), -1)]
    # ---- gte_gemm_p3_nt_ln_bwd (its lda1 limit lies behind the 2 GB bound: 257 rows of 8 MB are more)
    t += [(lnb, dict(m=-1), -1), (lnb, dict(n=0), -1), (lnb, dict(k1=0), -1), (lnb, dict(k2=-1), -1), (lnb, dict(n=257), -4),
          (lnb, dict(n=257, m=0), -4), (lnb, dict(n=257, m=-1), -1), (lnb, dict(n=257, a1=None), -4), (lnb, dict(m=0, a1=None), 0),
          (lnb, dict(a1=None), -1), (lnb, dict(b=None), -1), (lnb, dict(z=None), -1), (lnb, dict(stats=None), -1), (lnb, dict(gamma=None), -1),
          (lnb, dict(beta=None), -1), (lnb, dict(dz=None, dzp3=None), -1), (lnb, dict(workspace=None), -1), (lnb, dict(two, a2=None), -1),
          (lnb, dict(lda1=191), -1), (lnb, dict(two, lda2=95), -1), (lnb, dict(ldb=176), -1), (lnb, dict(ldz=63), -1), (lnb, dict(lddz=63), -1),
          (lnb, dict(ldp3=368), -1), (lnb, dict(ldp3=392), -1),
          (lnb, dict(lda1=_L23), -4), (lnb, dict(lda2=_L23), -4), (lnb, dict(lda2=_L23 - 1, workspace_bytes=ln_ws(100, 64) - 1), -3),
          (lnb, dict(ldb=_L23), -4), (lnb, dict(ldb=_L23 - 16, workspace_bytes=ln_ws(100, 64) - 1), -3),
          (lnb, dict(lda1=1 << 20, m=1792, workspace_bytes=ln_ws(1792, 64)), -4),
          (lnb, dict(lda1=1 << 20, m=1791, workspace_bytes=ln_ws(1791, 64) - 1), -3),
          (lnb, dict(two, lda2=1 << 20, m=1792, workspace_bytes=ln_ws(1792, 64)), -4),
          (lnb, dict(two, lda2=1 << 20, m=1791, workspace_bytes=ln_ws(1791, 64) - 1), -3),
          (lnb, dict(workspace_bytes=ln_ws(100, 64) - 1), -3), (lnb, dict(workspace_bytes=ln_ws(100, 64) - 1, ldb=_L23), -4),
          (lnb, dict(workspace_bytes=ln_ws(100, 64) - 1, z=None), -1), (lnb, dict(ldz=63, ldb=_L23), -1)]
    # ---- gte_gemm_p3_nt_smallk_bwd
    t += [(sk, dict(m=-1), -1), (sk, dict(n=0), -1), (sk, dict(kg1=0), -1), (sk, dict(kg2=-1), -1), (sk, dict(k1=0), -1), (sk, dict(k2=-1), -1),
          (sk, dict(k1=15, k2=14, ldx=15, ldahn=14, ldw=29, lddw=29), -4), (sk, dict(n=62), -4), (sk, dict(n=260), -4),
          (sk, dict(n=62, a1=None), -4), (sk, dict(n=62, m=-1), -1), (sk, dict(n=62, m=0), -4), (sk, dict(m=0, a1=None), 0),
          (sk, dict(a1=None), -1), (sk, dict(b=None), -1), (sk, dict(x=None), -1), (sk, dict(ahn=None), -1), (sk, dict(W=None), -1),
          (sk, dict(bias=None), -1), (sk, dict(gamma=None), -1), (sk, dict(beta=None), -1), (sk, dict(stats=None), -1), (sk, dict(dW=None), -1),
          (sk, dict(workspace=None), -1), (sk, dict(kg2=16, a2=None, lda2=96, ldb=288), -1),
          (sk, dict(lda1=191), -1), (sk, dict(kg2=16, a2=_P, lda2=95, ldb=288), -1), (sk, dict(ldb=176), -1), (sk, dict(ldx=12), -1),
          (sk, dict(ldahn=12), -1), (sk, dict(ldw=25), -1), (sk, dict(lddw=25), -1),
          (sk, dict(lda1=_L23), -4), (sk, dict(lda2=_L23), -4), (sk, dict(lda2=_L23 - 1, workspace_bytes=sk_ws(100) - 1), -3),
          (sk, dict(ldb=_L23), -4), (sk, dict(ldb=_L23 - 16, workspace_bytes=sk_ws(100) - 1), -3),
          (sk, dict(lda1=1 << 20, m=1792, workspace_bytes=sk_ws(1792)), -4),
          (sk, dict(lda1=1 << 20, m=1791, workspace_bytes=sk_ws(1791) - 1), -3),
          (sk, dict(kg2=16, a2=_P, lda2=1 << 20, ldb=288, m=1792, workspace_bytes=sk_ws(1792)), -4),
          (sk, dict(kg2=16, a2=_P, lda2=1 << 20, ldb=288, m=1791, workspace_bytes=sk_ws(1791) - 1), -3),
          (sk, dict(workspace_bytes=sk_ws(100) - 1), -3), (sk, dict(workspace_bytes=sk_ws(100) - 1, ldb=_L23), -4),
          (sk, dict(workspace_bytes=sk_ws(100) - 1, ldw=25), -1), (sk, dict(x=None, ldb=_L23), -1)]
    # ---- gte_gemm_p3_tn / _tn_rows / _tn_rows2 (the split plan in front of the row-map and workspace checks asks for the device's
    # CU count: a query, no launch; 256 without a device)
    short = dict(workspace_bytes=tn_ws - 1)
    t += [(tn, dict(m=0), -1), (tn, dict(n=0), -1), (tn, dict(k=-1), -1), (tn, dict(nseg=-1), -1), (tn, dict(nseg=60), -1),
          (tn, dict(a=None), -1), (tn, dict(b=None), -1), (tn, dict(c=None), -1),
          (tn, dict(lda=752), -1), (tn, dict(ldb=752), -1), (tn, dict(a2=_P, lda2=752), -1), (tn, dict(nseg=64, b2=_P, ldb2=368), -1),
          (tn, dict(ldc=127), -1),
          (tn, dict(lda=_L23), -4), (tn, dict(ldb=_L23), -4), (tn, dict(lda2=_L23), -4), (tn, dict(ldb2=_L23), -4),
          (tn, dict(short, lda=_L23 - 16), -3), (tn, dict(short, ldb=_L23 - 16), -3), (tn, dict(ldc=1 << 21), -4),
          (tn, dict(short, ldc=(1 << 21) - 1), -3),
          (tn, short, -3), (tn, dict(workspace=None), -3), (tn, dict(c=None, lda=_L23), -1), (tn, dict(short, ldc=1 << 21), -4),
          (tn, dict(short, ldc=127), -1),
          (tnr, dict(b_rows=None), -1), (tnr, dict(b_rows=None, ldpb=_L23), -1), (tnr, dict(n_res_rows=0), -1), (tnr, dict(short, n_res_rows=0), -1),
          (tnr, dict(n_res_rows=0, ldpb=_L23), -4), (tnr, dict(n_res_rows=0, ldpb=_L23 - 16), -1), (tnr, short, -3),
          (tnr2, dict(b_rows=None), -1), (tnr2, dict(b2_res=None), -1), (tnr2, dict(nseg=0), -1), (tnr2, dict(nseg=0, ldpb=_L23), -1),
          (tnr2, dict(ldpb2=768), -4), (tnr2, dict(ldpb2=768, n_res_rows=0), -4), (tnr2, dict(ldpb2=768, c=None), -1),
          (tnr2, dict(ldpb2=368), -1), (tnr2, dict(n_res_rows=0), -1), (tnr2, dict(short, n_res_rows=0), -1), (tnr2, short, -3)]
    return t


def test_planes_gemm_entry_points_refuse_invalid_calls_with_their_codes():
    """Every public planes-GEMM entry point against a table of invalid calls: negative sizes, each required pointer null, each leading
    dimension below its minimum, row strides at the limit and below it, the 2 GB operand bound where an entry point has one, an
    empty resident image, differing row strides behind one row map, a workspace one byte short, and calls wrong in two ways (which
    return the code of the check that stands first).  All return before the first launch: the pointers are dummies."""
    lib = _lib.load()
    valid = _p3_valid_calls(lib)
    assert set(valid) == set(_P3_PARAMS)
    table = _p3_invalid_calls(lib)
    assert {name for name, _, _ in table} == set(_P3_PARAMS) and len(table) >= 200
    wrong = []
    for name, change, want in table:
        assert set(change) <= set(valid[name]), (name, change)
        args = dict(valid[name], **change)
        got = getattr(lib, name)(*[args[k] for k in _P3_PARAMS[name].split()])
        if got != want:
            wrong.append((name, change, want, got, lib.gte_last_error().decode()))
    assert not wrong, wrong
    # the fragments other tests and callers look for in the message
    args = dict(valid["gte_gemm_p3_nt_rows"], n_res_rows=0)
    assert lib.gte_gemm_p3_nt_rows(*[args[k] for k in _P3_PARAMS["gte_gemm_p3_nt_rows"].split()]) == -1
    assert b"empty resident image" in lib.gte_last_error()
    args = dict(valid["gte_gemm_p3_tn"], a=None)
    assert lib.gte_gemm_p3_tn(*[args[k] for k in _P3_PARAMS["gte_gemm_p3_tn"].split()]) == -1 and b"null" in lib.gte_last_error()
