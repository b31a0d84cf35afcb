"""tests/spmm_ref.py against independent references, its graphs against the structure they claim, its exact cases against their
representability premise, and its power to detect a subtly wrong row kernel: a float32 emulation of spmm_csr_kernel passes the exact
ladder cases bit for bit, five mutants of it do not.  No GPU.  ``-s`` prints what each mutant broke and the emulations' worst
error / bound ratios."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import gcnsage_cpu as oc
from tests import spmm_ref as sr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnn-tableextraction_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_named_thresholds_are_the_kernels():
    csr, tiled = _source("spmm_csr.hip"), _source("spmm_tiled.hip")

    def const(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert const(csr, r"constexpr int kEdgeUnroll = (\d+);") == sr.UNROLL
    assert const(csr, r"constexpr int EP_SEG = (\d+);") == sr.EP_SEG
    assert const(tiled, r"constexpr int TILE_R = (\d+);") == sr.TILE_R
    assert const(tiled, r"constexpr int UMAX = (\d+);") == sr.UMAX
    assert const(tiled, r"constexpr int EMAX = (\d+);") == sr.EMAX
    assert const(tiled, r"#define GTE_TILED_EMAX_FULL (\d+)") == sr.EMAX_FULL
    assert const(tiled, r"#define GTE_TILED_FC (\d+)") == sr.TILED_FC
    # dispatch(): the chunk counts at which the lane-group form changes, and the forms
    assert re.findall(r"if \(nchunk <= (\d+)\) GTE_L\((\d+), (\d+)\);", csr) == [("16", "16", "1"), ("32", "32", "1"), ("64", "32", "2"),
                                                                                   ("128", "64", "2")]
    assert "if (nchunk <= 8 && T::EPC <= 8) {\n        if (nchunk <= 4 && T::EPC == 4) GTE_L(4, 1);\n        GTE_L(8, 1);" in csr
    assert "if (nchunk <= 64) GTE_EP(1); else if (nchunk <= 128) GTE_EP(2); else GTE_EP(4);" in csr


def test_widths_stand_on_both_sides_of_every_dispatch_threshold():
    forms = [sr.row_group(f) for f in sr.F32_WIDTHS]
    assert [sr.row_group(f) for f in (19, 20, 35, 36, 67, 68, 131, 132, 259, 260, 515, 516)] == \
        [(4, 1), (8, 1), (8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (32, 2), (32, 2), (64, 2), (64, 2), (64, 4)]
    assert set(forms) == {(4, 1), (8, 1), (16, 1), (32, 1), (32, 2), (64, 2), (64, 4)}
    assert 1027 // 4 == 256 and 1028 // 4 == 257                                  # the second feature block of GTE_L(64, 4) begins
    assert [sr.row_group(f, True) for f in sr.BF16_WIDTHS] == \
        [(8, 1), (8, 1), (8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (32, 2), (32, 2), (64, 2), (64, 2), (64, 4), (64, 4), (64, 4)]
    assert 2055 // 8 == 256 and 2056 // 8 == 257
    assert [sr.edge_cpl(f) for f in sr.EDGE_WIDTHS] == [1, 1, 1, 1, 1, 2, 2, 4, 4]
    # every width with a tail (F % 4, F % 8) and without; the tiled widths: generic, generic, generic, then the full kernel's drained
    # tails at 4, 5, 6, 7 chunks and its main loop's at 8
    assert [f // sr.TILED_FC if f % sr.TILED_FC == 0 and f >= 4 * sr.TILED_FC else 0 for f in sr.TILED_WIDTHS] == [0, 0, 0, 4, 5, 6, 7, 8]


# ---------------------------------------------------------------------------------------------------------------- the reference
def _random_graph(n=150, e=1100, seed=0):
    rng = np.random.default_rng(seed)
    dst = np.sort(rng.integers(0, n, e))
    dst[dst == 7] = 8
    return sr.Graph(np.bincount(dst, minlength=n), rng.integers(0, n, e))


@pytest.mark.parametrize("graph", ["ladder", "random"])
@pytest.mark.parametrize("mean", [False, True])
def test_ref_matches_the_oracle_loop_and_torch_sparse(graph, mean):
    g = sr.ladder_graph() if graph == "ladder" else _random_graph()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((g.n, 37))
    w = rng.uniform(-1, 1, g.nnz)
    base = rng.standard_normal((g.n, 37))
    for wv in (w, None):
        got = sr.ref(g.indptr, g.indices, wv, x, mean, block=16)
        want = oc.spmm_csr_numpy(g.indptr, g.indices, wv, x, mean=mean)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)
        a = torch.sparse_csr_tensor(torch.from_numpy(g.indptr.astype(np.int64)), torch.from_numpy(g.indices.astype(np.int64)),
                                    torch.from_numpy(np.ones(g.nnz) if wv is None else wv), size=(g.n, g.n), dtype=torch.float64)
        via_torch = (a @ torch.from_numpy(x)).numpy()
        if mean:
            via_torch = via_torch / np.maximum(g.deg, 1)[:, None]
        np.testing.assert_allclose(got, via_torch, rtol=1e-13, atol=1e-13)
        assert (got[g.deg == 0] == 0).all() and (g.deg == 0).any()
        with_base = sr.ref(g.indptr, g.indices, wv, x, mean, base=base)
        np.testing.assert_array_equal(with_base[g.deg == 0], base[g.deg == 0])     # rows without edges: base unchanged
        np.testing.assert_allclose(with_base, want + base, rtol=1e-13, atol=1e-13)
        m = sr.mag(g.indptr, g.indices, wv, x, mean)
        np.testing.assert_allclose(m, oc.spmm_csr_numpy(g.indptr, g.indices, None if wv is None else np.abs(wv), np.abs(x), mean=mean),
                                   rtol=1e-13, atol=1e-13)
        assert (m >= np.abs(got) * (1 - 1e-12)).all()


def test_bf16_round_is_torch_s():
    rng = np.random.default_rng(4)
    a = np.concatenate([rng.standard_normal(5000) * 2.0 ** rng.integers(-40, 40, 5000), np.arange(-300, 300),
                        [1.00390625, 1.01171875, 257.0, 255.5, 0.0]]).astype(np.float32)          # ties to even among them
    want = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(sr.bits(sr.bf16_round(a)), sr.bits(want))
    # half an ulp: attained at 1 + 2^-8, never exceeded, and between 2^-9 |a| and 2^-8 |a|
    err, h = np.abs(want.astype(np.float64) - a), sr.bf16_half_ulp(a)
    assert (err <= h).all() and err[-5] == h[-5] == 2.0 ** -8 and sr.bf16_half_ulp(0.0) == 0
    assert (h[a != 0] > 2.0 ** -9 * np.abs(a[a != 0])).all() and (h <= 2.0 ** -8 * np.abs(a)).all()


# ---------------------------------------------------------------------------------------------------------------- the graphs
def test_ladder_graph_structure():
    g = sr.ladder_graph()
    assert g.n == sr.LADDER_N == 131
    assert list(g.deg[:22]) == sr.LADDER and list(g.deg[22:44]) == sr.LADDER[::-1]
    assert g.deg[44:].max() <= 6
    for G in (4, 8, 16, 32, 64):
        rpw = 64 // G
        assert g.n % (4 * rpw) != 0 and (rpw == 1 or g.n % rpw != 0)        # the last block, and its last wave, are partial
        for d in sr.LADDER:                                                    # the two copies of a degree sit on different lane groups
            r1, r2 = sr.LADDER.index(d), 22 + sr.LADDER[::-1].index(d)
            assert rpw == 1 or r1 % rpw != r2 % rpw, (G, d)
        # degrees G - 1, G, G + 1, beyond G, and every remainder modulo the unroll
        assert {G - 1, G, G + 1} <= set(sr.LADDER) and max(sr.LADDER) > 3 * G
    assert {d % sr.UNROLL for d in g.deg if d > 4} == {0, 1, 2, 3}
    assert g.indices.min() >= 0 and g.indices.max() < g.n and len(np.unique(g.indices)) > 120
    for node in (0, sr.OTHER):
        named = g.names(node)
        partial_quad = g.deg % 4 != 0
        assert (named & partial_quad).any() and (~named & partial_quad).sum() >= 20 and (~named & (g.deg > 0) & ~partial_quad).any()
    assert g.names(0)[1] and g.names(0)[3] and g.names(sr.OTHER)[2] and not g.names(0)[5] and not g.names(sr.OTHER)[5]
    # tile 0 holds the 128-, 129- and 200-edge rows: past EMAX_FULL, the direct-gather path of both tiled kernels
    assert sr.tile_facts(g)[0][0] > sr.EMAX_FULL


def test_segment_graphs_structure():
    S = sr.EP_SEG
    g = sr.segment_graph()
    assert list(g.indptr) == [0, 0, 0, 3, 64, 64, 128, 256, 257, 257, 257, 319, 449, 512, 712, 717, 717]
    lo, hi = g.indptr[:-1], g.indptr[1:]
    assert g.deg[0] == 0 and g.deg[1] == 0                                           # leading empty rows
    assert hi[3] % S == 0 and g.deg[3] > 0 and g.deg[4] == 0                         # a row ends on a boundary, an empty row follows
    assert lo[5] % S == 0 and g.deg[5] == S                                          # exactly one aligned segment
    assert lo[6] % S == 0 and g.deg[6] == 2 * S                                      # exactly two: TAIL + HEAD only
    assert lo[11] % S == S - 1 and hi[11] % S == 1 and hi[11] // S - lo[11] // S == 3      # four segments, one-edge TAIL and HEAD
    assert lo[13] % S == 0 and (hi[13] - 1) // S - lo[13] // S == 3 and hi[13] % S != 0    # starts on a boundary, spans four
    assert g.deg[15] == 0 and g.deg[7] == 1 and g.deg[8] == 0 and g.deg[9] == 0      # trailing empty row; empty rows inside a segment
    inside = sr.inside_one_segment(g)
    assert list(np.flatnonzero(~inside)) == [6, 11, 13] and inside[5] and inside[3]
    g1, g2 = sr.segment_graph(1), sr.segment_graph(2)
    assert g1.nnz == 768 and g1.nnz % S == 0 and g1.deg[15] == 0 and g1.deg[16] == 51
    assert g2.nnz == 769 and g2.deg[17] == 1 and g2.indptr[17] % S == 0              # a one-edge last segment
    for gg in (g, g1, g2):
        assert gg.indices.max() < gg.n


def test_tile_graph_structure():
    g = sr.tile_graph()
    facts = dict(zip(sr.TILE_NAMES, sr.tile_facts(g)))
    assert g.n % sr.TILE_R == 7 and len(facts) == 8
    assert [facts[k][0] for k in ("e448", "e449", "e512", "e513")] == [sr.EMAX, sr.EMAX + 1, sr.EMAX_FULL, sr.EMAX_FULL + 1]
    assert all(facts[k][1] <= 96 for k in ("e448", "e449", "e512", "e513"))           # the edge count alone decides
    assert facts["u128"] == (sr.UMAX, sr.UMAX) and facts["u129"] == (sr.UMAX + 1, sr.UMAX + 1)
    assert facts["empty"] == (0, 0) and 0 < facts["partial"][0] < sr.EMAX

    def staged(emax):
        return [ne <= emax and nu <= sr.UMAX for ne, nu in sr.tile_facts(g)]
    assert staged(sr.EMAX) == [True, False, False, False, True, False, True, True]
    assert staged(sr.EMAX_FULL) == [True, True, True, False, True, False, True, True]
    deg = g.deg[:4 * sr.TILE_R].reshape(4, sr.TILE_R)
    assert [sorted(set(r)) for r in deg] == [[14], [14, 15], [16], [16, 17]]


def test_cycle_graph():
    g = sr.cycle_graph(1000)
    assert g.n == 1000 and set(g.deg) == {0, 1, 2, 3, 4, 5} and g.indices.max() < sr.LADDER_N


# ---------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("bf16", [False, True])
def test_exact_cases_are_representable_in_every_order(bf16):
    """every value, every CSR-order prefix sum and every result (sum, and sum + base) is exact in the OUTPUT type; weights and values
    are such that any regrouping stays exact too: all terms are multiples of 0.5 (fp32) or integers (bf16) and the sum of the
    absolute terms stays below 2^24 (fp32) / at 256 or below (bf16)"""
    out_type = sr.bf16_round if bf16 else (lambda a: np.asarray(a, dtype=np.float32))
    for g in (sr.ladder_graph(), sr.segment_graph(2), sr.tile_graph()):
        for f in (13, 72 if bf16 else 20):
            w, x, base = sr.exact_case(g, f, bf16)
            for arr in (w, x, base):
                np.testing.assert_array_equal(out_type(arr), arr)
            assert set(np.unique(w)) <= ({1.0, 2.0} if bf16 else {0.5, 1.0, 2.0})
            assert np.abs(x).max() <= (1 if bf16 else 8) and (x == np.round(x)).all()
            if bf16:
                assert (w[g.deg[g.row_of_edge] > 64] == 1).all()
            terms = x[g.indices].astype(np.float64) * w[:, None]
            total_abs = sr.mag(g.indptr, g.indices, w, x, False)
            assert total_abs.max() + 50 <= (256 if bf16 else 2 ** 24)
            assert (terms * 2 == np.round(terms * 2)).all() and (not bf16 or (terms == np.round(terms)).all())
            prefix = np.cumsum(terms, axis=0)
            prefix -= np.concatenate([np.zeros((1, f)), prefix])[g.indptr[:-1][g.row_of_edge]]      # per-row prefixes
            np.testing.assert_array_equal(out_type(prefix.astype(np.float32)).astype(np.float64), prefix)
            s = sr.ref(g.indptr, g.indices, w, x, False)
            for val in (s, s + base):
                np.testing.assert_array_equal(out_type(val.astype(np.float32)).astype(np.float64), val)
            # expect_exact is the reference wherever nothing rounds, and within half an ulp of the output type elsewhere
            np.testing.assert_array_equal(sr.expect_exact(g, w, x, False, base, bf16).astype(np.float64), s + base)
            m = sr.expect_exact(g, w, x, True, None, bf16).astype(np.float64)
            rm = sr.ref(g.indptr, g.indices, w, x, True)
            assert (np.abs(m - rm) <= 2.0 ** -23 * np.abs(rm) + (sr.bf16_half_ulp(rm) if bf16 else 0)).all()
            pow2 = sr.exact_rows(g, True, True)
            assert list(np.unique(g.deg[pow2])) == [d for d in np.unique(g.deg) if d & (d - 1) == 0]
            if not bf16:                                   # a power-of-two degree divides exactly
                np.testing.assert_array_equal(m[pow2 & (g.deg > 0)], rm[pow2 & (g.deg > 0)])


# ---------------------------------------------------------------------------------------------------------------- detection power
EMU_WIDTHS = [13, 19, 67, 260]            # G = 4 (with and without a 3-wide tail), 16, 64


@pytest.mark.parametrize("mean", [False, True])
def test_emulation_passes_the_exact_ladder_bitwise(mean):
    g = sr.ladder_graph()
    for f in EMU_WIDTHS:
        for weights in (True, False):
            w, x, base = sr.exact_case(g, f, weights=weights)
            assert sr.same_bits(sr.emulate_rows(g, w, x, mean), sr.expect_exact(g, w, x, mean))
            rows = sr.exact_rows(g, mean, True)
            assert sr.same_bits(sr.emulate_rows(g, w, x, mean, base)[rows], sr.expect_exact(g, w, x, mean, base)[rows])
            assert sr.same_bits(sr.emulate_segments(g, w, x, mean), sr.expect_exact(g, w, x, mean))
    for f in (13, 72):
        w, x, base = sr.exact_case(g, f, bf16=True)
        assert sr.same_bits(sr.emulate_rows(g, w, x, mean, bf16=True), sr.expect_exact(g, w, x, mean, bf16=True))


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_mutants_fail_the_exact_ladder(mutant):
    g = sr.ladder_graph()
    mean = mutant == "mean_deg_plus_1"
    broken = {}
    for f in EMU_WIDTHS:
        w, x, _ = sr.exact_case(g, f)
        got, want = sr.emulate_rows(g, w, x, mean, mutant=mutant), sr.expect_exact(g, w, x, mean)
        bad = sr.bits(got) != sr.bits(want)
        broken[f] = (int(bad.any(axis=1).sum()), sorted(set(g.deg[bad.any(axis=1)].tolist()))[:8], int(bad.any(axis=0).sum()))
    print(f"\n{mutant}: " + "; ".join(f"F={f}: {r} rows (degrees {d}...), {c} columns" for f, (r, d, c) in broken.items()))
    expected_widths = {"tail_reads_col0": [13, 19, 67], "skip_second_trip": EMU_WIDTHS}.get(mutant, EMU_WIDTHS)
    for f in expected_widths:
        assert broken[f][0] > 0, (mutant, f)
    if mutant == "tail_reads_col0":
        assert broken[260][0] == 0 and all(broken[f][2] <= 3 for f in (13, 19, 67))      # only the tail columns
    if mutant == "skip_second_trip":
        G = {f: sr.row_group(f)[0] for f in EMU_WIDTHS}
        assert all(min(broken[f][1]) > G[f] for f in EMU_WIDTHS)                          # only rows beyond one trip
        assert broken[260][1][0] == 65                                                   # G = 64: the rows no earlier test had
    if mutant == "drop_last_mod4":
        assert all(d % 4 == 1 for f in EMU_WIDTHS for d in broken[f][1])


@pytest.mark.parametrize("kind", sr.BOUND_KINDS)
def test_both_summation_orders_stay_inside_the_bound(kind):
    worst = {}
    for base_graph in (sr.ladder_graph(), sr.segment_graph(2)):
        for f in (13, 67):
            g, w, x, base = sr.bound_case(base_graph, f, kind)
            assert 2.0 ** -60 < np.abs(x[x != 0]).min() and np.abs(x).max() < 2.0 ** 60
            for mean in (False, True):
                r = sr.ref(g.indptr, g.indices, w, x, mean)
                b = sr.bound(g, w, x, mean, r)
                for name, got in (("rows", sr.emulate_rows(g, w, x, mean)), ("segments", sr.emulate_segments(g, w, x, mean))):
                    worst[name] = max(worst.get(name, 0.0), sr.ratio(got, r, b))
                ra = sr.ref(g.indptr, g.indices, w, x, mean, base)
                worst["rows+base"] = max(worst.get("rows+base", 0.0),
                                         sr.ratio(sr.emulate_rows(g, w, x, mean, base), ra, sr.bound(g, w, x, mean, ra, base)))
            if kind == "cancel":      # the odd rows do cancel: their sums are far below their terms
                s, m = np.abs(sr.ref(g.indptr, g.indices, w, x, False)), sr.mag(g.indptr, g.indices, w, x, False)
                odd = (np.arange(g.n) % 2 == 1) & (g.deg >= 2) & (g.deg % 2 == 0)
                assert np.median(s[odd] / m[odd]) < 5e-3
    print(f"\n{kind}: worst error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # ... and a mutant is far outside it
    g, w, x, _ = sr.bound_case(sr.ladder_graph(), 13, kind)
    r = sr.ref(g.indptr, g.indices, w, x, False)
    assert sr.ratio(sr.emulate_rows(g, w, x, False, mutant="drop_last_mod4"), r, sr.bound(g, w, x, False, r)) > 100
