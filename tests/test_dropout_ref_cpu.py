"""tests/dropout_ref.py against the library's host masks (gte_dropout_mask_host), its case lists against what they claim, and its
power to detect a subtly wrong dropout aggregation kernel: a float32 emulation of each kernel of csrc/dropout.hip equals the exact
expectation bit for bit and stays below half the bound on every bound case; eight mutants of it fail the exact cases.  No GPU.
``-s`` prints what each mutant broke, the emulations' worst error / bound ratios and the swept-p count."""
import os
import re

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import ops
from tests import dropout_ref as dr
from tests import spmm_ref as sr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnn-tableextraction_amd", "csrc")


def host_mask(p, seed, rank, step, site, n_rows, n_cols):
    return ops.dropout_mask(p, seed, rank, step, site, n_rows, n_cols).numpy()


# ---------------------------------------------------------------------------------------------------------------- the contract
def test_named_dispatch_is_the_kernels():
    with open(os.path.join(CSRC, "dropout.hip")) as f:
        text = f.read()
    assert re.search(r"constexpr int kEdgeUnroll = (\d+);", text).group(1) == str(dr.UNROLL)
    fwd = text[text.index('extern "C" int gte_spmm_dropout_p3'):text.index('extern "C" int gte_spmm_dropout_bwd')]
    bwd = text[text.index('extern "C" int gte_spmm_dropout_bwd'):]
    assert "const int64_t nqp = p3::blocks(n_feat) * 4;" in fwd
    assert re.search(r"if \(nqp <= gte::kWave\) GTE_DROP_FWD\(1\);\s+else if \(nqp <= 2 \* gte::kWave\) GTE_DROP_FWD\(2\);\s+else GTE_DROP_FWD\(4\);", fwd)
    assert "const int64_t nq = n4 / 4;" in bwd
    assert re.search(r"if \(nq <= gte::kWave\) GTE_DROP_BWD\(1\);\s+else if \(nq <= 2 \* gte::kWave\) GTE_DROP_BWD\(2\);\s+else GTE_DROP_BWD\(4\);", bwd)
    assert "qb += gte::kWave * CPL" in text
    assert [dr.producer_cpl(f) for f in (256, 257, 512, 513)] == [1, 2, 2, 4] and [dr.bwd_cpl(f) for f in (256, 257, 512, 513)] == [1, 2, 2, 4]
    assert [dr.producer_passes(f) for f in (1024, 1025)] == [1, 2] and [dr.bwd_passes(f) for f in (1024, 1025)] == [1, 2]


def test_case_lists_contain_what_they_claim():
    for g in (dr.ladder_graph(), dr.bwd_graph(), dr.confine_graph(0), dr.confine_graph(dr.OTHER)):
        assert g.n == dr.LADDER_N and {0, 1, 2, 3, 5} <= set(g.deg.tolist()) and g.deg.max() >= 129
        assert g.indices.min() >= 0 and g.indices.max() < g.n
    assert not np.array_equal(dr.bwd_graph().indices, dr.ladder_graph().indices)
    for widths, cpl, passes in ((dr.PRODUCER_WIDTHS, dr.producer_cpl, dr.producer_passes), (dr.BWD_WIDTHS, dr.bwd_cpl, dr.bwd_passes)):
        for c in (1, 2, 4):
            assert {f % 4 for f in widths if cpl(f) == c} == {0, 1, 2, 3}, (c, widths)
        assert any(passes(f) == 2 for f in widths) and any(passes(f) == 1 and cpl(f) == 4 for f in widths)
        assert max(passes(f) for f in widths) == 2
    # the widths the issue names are all there
    assert set(dr.PRODUCER_WIDTHS) >= {1, 3, 4, 5, 13, 16, 17, 255, 256, 257, 259, 510, 512, 513, 831, 1023, 1024, 1025, 1030}
    assert set(dr.BWD_WIDTHS) >= {1, 3, 13, 255, 256, 257, 258, 511, 512, 513, 1000, 1024, 1025, 1027, 1030}
    assert dr.PRODUCER_BOUND_WIDTHS == [13, 259, 1030] and dr.BWD_BOUND_WIDTHS == [13, 258, 1030] and dr.BOUND_P == [0.1, 0.3, 0.9]
    assert set(dr.PRODUCER_BOUND_WIDTHS + dr.CONFINE_WIDTHS + dr.COORD_WIDTHS) <= set(dr.PRODUCER_WIDTHS)
    # coordinates: a seed with the high word set, rank 3, sites 1, 2 and 7, every step
    assert any(s >> 32 for s, _, _, _ in dr.COORDS) and {r for _, r, _, _ in dr.COORDS} >= {0, 3}
    assert {site for _, _, _, site in dr.COORDS} == {1, 2, 7} and {st for _, _, st, _ in dr.COORDS} >= set(dr.STEPS)
    assert {0.1, 0.2, 0.3, 0.5, 0.9, dr.P_SWEPT, dr.P_LOW, dr.P_HIGH} == set(dr.SELF_P)
    # the row map names no row by its own number
    n = dr.LADDER_N
    for f in (13, 1030):
        rows = dr.row_map(n, n + dr.RES_EXTRA, seed=f)
        assert (rows != np.arange(n)).all() and len(set(rows.tolist())) == n and rows.max() < n + dr.RES_EXTRA
    # the confinement graph: the poisoned node is the last edge of a 5-edge row, and rows 1 / 3 (node 0), 2 (OTHER) still name it
    for node in (0, dr.OTHER):
        g = dr.confine_graph(node)
        assert g.deg[38] == 5 and g.indices[g.indptr[39] - 1] == node and g.names(node)[38]
        assert (~g.names(node) & (g.deg % 4 != 0)).any() and not g.names(node)[5]


# ---------------------------------------------------------------------------------------------------------------- the masks
@pytest.mark.parametrize("f", sorted(set(dr.PRODUCER_WIDTHS + dr.BWD_WIDTHS)))
def test_numpy_masks_equal_the_host_masks_at_every_width(f):
    c = dr.coords(f)
    for site, cols in ((0, f), (c["site"], 2 * f)):
        for p in dr.EXACT_P:
            np.testing.assert_array_equal(dr.keep(p, c["seed"], c["rank"], c["step"], site, dr.LADDER_N, cols),
                                          host_mask(p, c["seed"], c["rank"], c["step"], site, dr.LADDER_N, cols))


@pytest.mark.parametrize("seed,rank,step,site", dr.COORDS)
def test_numpy_masks_equal_the_host_masks_at_every_coordinate(seed, rank, step, site):
    for f in dr.COORD_WIDTHS:
        for p in (0.5, 0.3):
            for st, cols in ((0, f), (site, 2 * f)):
                np.testing.assert_array_equal(dr.keep(p, seed, rank, step, st, dr.LADDER_N, cols),
                                              host_mask(p, seed, rank, step, st, dr.LADDER_N, cols))


def test_step_is_cut_to_32_bits_and_rows_and_columns_are_coordinates():
    for step in dr.STEPS:
        np.testing.assert_array_equal(dr.keep(0.3, 77, 1, step, 2, 9, 26), host_mask(0.3, 77, 1, step, 2, 9, 26))
    np.testing.assert_array_equal(host_mask(0.3, 77, 1, 2 ** 32 + 5, 2, 9, 26), host_mask(0.3, 77, 1, 5, 2, 9, 26))
    assert not np.array_equal(host_mask(0.3, 77, 1, 2 ** 32 + 5, 2, 9, 26), host_mask(0.3, 77, 1, 2 ** 32 - 1, 2, 9, 26))
    full = dr.keep(0.3, 77, 1, 5, 2, 40, 50)
    np.testing.assert_array_equal(dr.keep(0.3, 77, 1, 5, 2, 0, 13, rows=[31, 7, 39], col0=13), full[[31, 7, 39], 13:26])


def test_host_mask_with_a_row_stride_leaves_the_guard_bytes():
    n, c = 17, 13
    buf = torch.full((n, c + 5), 0x55, dtype=torch.uint8)
    got = ops.dropout_mask(0.3, 5, 2, 9, 3, n, c, out=buf[:, :c])
    assert got.data_ptr() == buf.data_ptr() and bool((buf[:, c:] == 0x55).all())
    np.testing.assert_array_equal(buf[:, :c].numpy(), dr.keep(0.3, 5, 2, 9, 3, n, c))


def test_both_ends_of_the_threshold():
    assert dr.threshold(dr.P_LOW) == 0 and dr.scale_f32(dr.P_LOW) == np.float32(1.0)
    assert host_mask(dr.P_LOW, 3, 0, 1, 1, 64, 257).all() and dr.keep(dr.P_LOW, 3, 0, 1, 1, 64, 257).all()
    assert np.float32(dr.P_HIGH) == dr.P_HIGH < 1.0 and float(np.nextafter(np.float32(dr.P_HIGH), np.float32(2))) == 1.0
    assert dr.threshold(dr.P_HIGH) == 2 ** 32 - 2 ** 8 and (2 ** 32 - dr.threshold(dr.P_HIGH)) / 2 ** 32 == 2.0 ** -24
    assert dr.scale_f32(dr.P_HIGH) == np.float32(2.0 ** 24)
    m = host_mask(dr.P_HIGH, 3, 0, 1, 1, 512, 2048)                      # 2^20 draws at 2^-24: almost surely none kept, a few at most
    assert m.sum() <= 3
    np.testing.assert_array_equal(m, dr.keep(dr.P_HIGH, 3, 0, 1, 1, 512, 2048))
    # the clamps proper: dropout::threshold never leaves [0, 2^32 - 1] (the entry points refuse p outside (0, 1) before it)
    assert dr.threshold(0.0) == 0 and dr.threshold(-1.0) == 0 and dr.threshold(1.0) == dr.M32 and dr.threshold(7.0) == dr.M32
    for p in (0.1, 0.2, 0.3, 0.5, 0.9, dr.P_SWEPT):
        assert dr.threshold(p) == int(float(np.float32(p)) * 2 ** 32 + 0.5)


def test_the_scale_comes_from_the_fp32_value_of_p():
    """p = k / 1000, k = 1 ... 999: at 359 of them fp32(1 / (1 - p)) computed from the double p differs (by one ulp) from the
    scale the ABI defines, fp32(1 / (1 - fp32(p))).  P_SWEPT is one of them: the self-image case at P_SWEPT fails for a library or
    a reference that takes the scale from the double."""
    differ = [k for k in range(1, 1000) if np.float32(1.0 / (1.0 - k / 1000)) != dr.scale_f32(k / 1000)]
    print(f"\n    p = k / 1000: the scale from the double p differs from scale_f32(p) at {len(differ)} of 999 values")
    assert len(differ) == 359
    assert round(dr.P_SWEPT * 1000) in differ and dr.P_SWEPT in dr.SELF_P
    assert all(dr.scale_f32(p) == np.float32(s) for p, s in ((0.5, 2.0), (0.75, 4.0)))


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_refs_equal_a_plain_loop():
    g = dr.ladder_graph()
    rng = np.random.default_rng(1)
    f, p, seed, rank, step, site = 7, 0.3, 11, 2, 4, 3
    x = rng.standard_normal((g.n, f)).astype(np.float32)
    w = rng.uniform(-1, 1, g.nnz).astype(np.float32)
    s = float(dr.scale_f32(p))
    m0, m = host_mask(p, seed, rank, step, 0, g.n, f), host_mask(p, seed, rank, step, site, g.n, 2 * f)
    for in_drop in (False, True):
        xd = np.where(m0 == 1, x * np.float32(s), np.float32(0)) if in_drop else x
        want = np.zeros((g.n, f))
        for v in range(g.n):
            for e in range(g.indptr[v], g.indptr[v + 1]):
                want[v] += float(w[e]) * xd[g.indices[e]].astype(np.float64) / g.deg[v]
        got_s, got_a = dr.producer_ref(g, w, x, p, seed, rank, step, site, in_drop)
        np.testing.assert_array_equal(got_s, np.where(m[:, :f] == 1, xd * np.float32(s), np.float32(0)))
        np.testing.assert_allclose(got_a, np.where(m[:, f:] == 1, want * s, 0.0), rtol=1e-13, atol=1e-13)
        assert (got_a[g.deg == 0] == 0).all()
    agg_col = 12
    G = rng.standard_normal((g.n, agg_col + 8)).astype(np.float32)
    want = np.where(m[:, :f] == 1, G[:, :f].astype(np.float64) * s, 0.0)
    for v in range(g.n):
        for e in range(g.indptr[v], g.indptr[v + 1]):
            u = g.indices[e]
            want[v] += float(w[e]) * np.where(m[u, f:] == 1, (G[u, agg_col:agg_col + f] * np.float32(s)).astype(np.float64), 0.0)
    np.testing.assert_allclose(dr.bwd_ref(g, w, G, agg_col, f, p, seed, rank, step, site), want, rtol=1e-13, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------- detection power
def _producer_x(res, rows, n, resident):
    return res[rows] if resident else res[:n]


@pytest.mark.parametrize("f", dr.PRODUCER_WIDTHS)
def test_producer_emulation_equals_the_exact_expectation_bitwise(f):
    c = dr.coords(f)
    for i, (in_drop, resident, weights) in enumerate([(False, False, True), (True, True, True), (True, False, False)]):
        g, w, res, rows = dr.producer_exact_case(f, weights)
        x = _producer_x(res, rows, g.n, resident)
        p = dr.EXACT_P[(i + f) % 2]
        got = dr.emulate_producer(g, w, x, p, in_drop=in_drop, x_rows=rows if resident else None, **c)
        want = dr.producer_expect(g, w, x, p, in_drop=in_drop, **c)
        assert dr.same_bits(got[0], want[0]) and dr.same_bits(got[1], want[1]), (f, in_drop, resident)
        ref_s, ref_a = dr.producer_ref(g, w, x, p, in_drop=in_drop, **c)
        assert dr.same_bits(want[0], ref_s)
        assert sr.ratio(want[1], ref_a, dr.producer_bound(g, w, x, p, in_drop=in_drop, **c)) <= 1.0


@pytest.mark.parametrize("f", dr.BWD_WIDTHS)
def test_bwd_emulation_equals_the_exact_expectation_bitwise(f):
    c = dr.coords(f)
    for agg_col in (dr.c16(f), dr.c4(f)):
        g, w, G = dr.bwd_exact_case(f, agg_col, agg_col + dr.c4(f))
        p = dr.EXACT_P[f % 2]
        got = dr.emulate_bwd(g, w, G, agg_col, f, p, **c)
        assert dr.same_bits(got, dr.bwd_expect(g, w, G, agg_col, f, p, **c)), (f, agg_col)


def _broken(got, want):
    bad = sr.bits(got) != sr.bits(want)
    return int(bad.any(axis=1).sum()), np.flatnonzero(bad.any(axis=1)), np.flatnonzero(bad.any(axis=0))


MUTANT_WIDTHS = [6, 13, 256, 1030]


@pytest.mark.parametrize("mutant", dr.PRODUCER_MUTANTS)
def test_producer_mutants_fail_the_exact_cases(mutant):
    assert set(MUTANT_WIDTHS) <= set(dr.PRODUCER_WIDTHS)
    seen = {}
    for f in MUTANT_WIDTHS:
        c = dr.coords(f)
        g, w, res, rows = dr.producer_exact_case(f)
        for in_drop, resident in ((False, False), (True, False), (True, True)):
            x = _producer_x(res, rows, g.n, resident)
            got = dr.emulate_producer(g, w, x, 0.5, in_drop=in_drop, x_rows=rows if resident else None, mutant=mutant, **c)
            want = dr.producer_expect(g, w, x, 0.5, in_drop=in_drop, **c)
            assert dr.same_bits(got[0], want[0]) or mutant == "g"                  # only the wrong column reaches the self image
            seen[f, in_drop, resident] = _broken(got[1], want[1]) + (_broken(got[0], want[0])[0],)
    print(f"\n    {mutant} ({dr.MUTANTS[mutant]}): " +
          "; ".join(f"F={f} in_drop={int(d)} map={int(r)}: {v[0]} rows" for (f, d, r), v in seen.items()))
    hit = {k for k, v in seen.items() if v[0] > 0}
    assert hit, f"no exact case rejects mutant {mutant}"
    every = set(seen)
    if mutant in ("a", "c", "h"):
        assert hit == every
    if mutant in ("c", "h"):                                    # only rows whose last quad has a lane past the row end
        assert all((g.deg[v[1]] % 4 != 0).all() for v in seen.values())
    if mutant == "b":
        assert hit == {k for k in every if k[1] and k[2]}        # needs the input mask and a row map
    if mutant == "d":
        assert hit == {k for k in every if k[1]}
    if mutant == "e":
        assert hit == {k for k in every if k[0] % 4 != 0}
    if mutant == "g":
        assert hit == {k for k in every if k[0] == 1030}
        assert all(v[2].min() >= 1024 and v[3] > 0 for k, v in seen.items() if k[0] == 1030)


@pytest.mark.parametrize("mutant", dr.BWD_MUTANTS)
def test_bwd_mutants_fail_the_exact_cases(mutant):
    assert set(MUTANT_WIDTHS) <= set(dr.BWD_WIDTHS)
    seen = {}
    for f in MUTANT_WIDTHS:
        c = dr.coords(f)
        agg_col = dr.c16(f)
        g, w, G = dr.bwd_exact_case(f, agg_col, 2 * agg_col)
        seen[f] = _broken(dr.emulate_bwd(g, w, G, agg_col, f, 0.5, mutant=mutant, **c), dr.bwd_expect(g, w, G, agg_col, f, 0.5, **c))
    print(f"\n    {mutant} ({dr.MUTANTS[mutant]}): " + "; ".join(f"F={f}: {v[0]} rows" for f, v in seen.items()))
    hit = {f for f, v in seen.items() if v[0] > 0}
    assert hit, f"no exact case rejects mutant {mutant}"
    if mutant in ("a", "c", "f"):
        assert hit == set(MUTANT_WIDTHS)
    if mutant == "c":
        assert all((g.deg[v[1]] % 4 != 0).all() for v in seen.values())
    if mutant == "e":
        assert hit == {f for f in MUTANT_WIDTHS if f % 4 != 0}
    if mutant == "g":
        assert hit == {1030} and seen[1030][2].min() >= 1024


def test_every_mutant_is_rejected_somewhere():
    assert sorted(set(dr.PRODUCER_MUTANTS) | set(dr.BWD_MUTANTS)) == sorted(dr.MUTANTS) == list("abcdefgh")


def _emulation_ratio(kernel, f, kind):
    c = dict(dr.BASE)
    worst = 0.0
    if kernel == "producer":
        g, w, x = dr.producer_bound_case(f, kind)
        assert 2.0 ** -60 < np.abs(x[x != 0]).min() and np.abs(x).max() < 2.0 ** 60
        for p in dr.BOUND_P:
            for in_drop in (False, True):
                got_s, got_a = dr.emulate_producer(g, w, x, p, in_drop=in_drop, **c)
                ref_s, ref_a = dr.producer_ref(g, w, x, p, in_drop=in_drop, **c)
                assert dr.same_bits(got_s, ref_s)
                worst = max(worst, sr.ratio(got_a, ref_a, dr.producer_bound(g, w, x, p, in_drop=in_drop, **c)))
        return worst
    agg_col = dr.c16(f)
    g, w, G = dr.bwd_bound_case(f, kind, agg_col, 2 * agg_col)
    for p in dr.BOUND_P:
        got = dr.emulate_bwd(g, w, G, agg_col, f, p, **c)
        assert dr.same_bits(got[g.deg == 0], dr.bwd_self_f32(G, f, p, **c)[g.deg == 0])
        worst = max(worst, sr.ratio(got, dr.bwd_ref(g, w, G, agg_col, f, p, **c), dr.bwd_bound(g, w, G, agg_col, f, p, **c)))
    return worst


@pytest.mark.parametrize("kind", sr.BOUND_KINDS)
@pytest.mark.parametrize("kernel,f", [("producer", f) for f in dr.PRODUCER_BOUND_WIDTHS] + [("bwd", f) for f in dr.BWD_BOUND_WIDTHS])
def test_emulation_stays_inside_the_bound_and_below_half_of_it(kernel, f, kind):
    """CONDITION: a correct kernel (the emulation) leaves half of the bound unused on every bound case.
    MEASURED (both kinds alike, worst over p = 0.1, 0.3, 0.9): producer F = 13 0.366, 259 0.368, 1030 0.394; backward F = 13 0.356,
    258 0.410, 1030 0.444.  The worst elements sit on rows of degree 1 and 2.  (With the aggregated operand of the backward taken as
    the exact product G s instead of its fp32 value, the one agg term of an out-degree-1 row is rounded three times against a bound
    of 1 + 3 units and the emulation reaches 0.583 at F = 1030: the derivation in tests/dropout_ref.py counts that operand as the
    forward counts x', and pins the elementwise product bit for bit on the rows without out-edges instead.)"""
    r = _emulation_ratio(kernel, f, kind)
    print(f"\n    {kernel} {kind} F={f}: worst error / bound of the emulation {r:.3f}")
    assert 0.0 < r <= 1.0
    assert r < 0.5, f"{kernel} {kind} F={f}: the emulation uses {r:.3f} of the bound"


@pytest.mark.parametrize("kind", sr.BOUND_KINDS)
def test_a_mutant_is_far_outside_the_bound(kind):
    c = dict(dr.BASE)
    g, w, x = dr.producer_bound_case(13, kind)
    bad = dr.emulate_producer(g, w, x, 0.3, in_drop=True, mutant="h", **c)[1]
    assert sr.ratio(bad, dr.producer_ref(g, w, x, 0.3, in_drop=True, **c)[1], dr.producer_bound(g, w, x, 0.3, in_drop=True, **c)) > 100
    agg_col = 16
    g, w, G = dr.bwd_bound_case(13, kind, agg_col, 2 * agg_col)
    bad = dr.emulate_bwd(g, w, G, agg_col, 13, 0.3, mutant="c", **c)
    assert sr.ratio(bad, dr.bwd_ref(g, w, G, agg_col, 13, 0.3, **c), dr.bwd_bound(g, w, G, agg_col, 13, 0.3, **c)) > 100
