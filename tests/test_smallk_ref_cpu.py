"""The float64 reference, the bounds and the inputs of tests/test_gpu_smallk_bwd.py (tests/smallk_ref.py), checked without a GPU:

  * the reference against torch autograd in float64 through linear + layer_norm + relu on a well-conditioned case;
  * a float32 emulation of gte_smallk_bwd_step and of both kernels' summation orders (stand-alone: 16 rows per lane and trip, four
    waves, the block fold; epilogue: 16 rows per lane, eight waves, the tile fold; each inside and outside a fold deferral) stays
    within the bounds on every case the GPU tests run, both grid-stride cases (smallk_ref.stride_case) included;
  * mutants of that emulation each break a bound by more than 10x on at least one of those cases: z with the bias added last, 1 / n
    of the padded width, no c2 term, the mask on xhat, the clamped row M - 1 counted again behind the last row, the second grid-stride
    trip skipped, the second operand read with the first one's leading dimension, a non-zero padding column of the staged inputs;
  * on these inputs the reference's float32 mask equals the float64 mask on the same statistics outside the planted exact ties, i.e.
    the GPU tests neutralise nothing (the count per row kind is printed; the cap of layernorm_cases holds trivially).
Run with ``-s`` to see the ratios."""
import numpy as np
import pytest
import torch

from tests import layernorm_cases as lc
from tests import smallk_ref as sk

STRIDE_CASES = [sk.stride_case(n) for n in sk.STRIDE_NS]


def _all_cases():
    return sk.cases("standalone") + sk.cases("epilogue") + STRIDE_CASES


def _forward(case):
    form, k1, k2, n, m, relu, idx = case
    d = sk.make_inputs(case)
    z, y, mean, rstd = sk.emulate_forward(d["xin"], k1, k2, d["W"], d["bias"], d["gamma"], d["beta"], d["eps"], relu)
    return d, z, y, mean, rstd


def _emulated(case, deferred=False, mutant=None):
    """error / bound of the four outputs of the emulated backward on one case, the reference on the emulated forward's z and stats"""
    form, k1, k2, n, m, relu, idx = case
    d, z, y, mean, rstd = _forward(case)
    got = sk.emulate_backward(form, d["dy"], d["xin"], k1, k2, d["W"], d["bias"], d["gamma"], d["beta"], mean, rstd, relu, deferred, mutant)
    return sk.ratios(form, got, d["dy"], d["xin"], z, mean, rstd, d["gamma"], d["beta"], relu)


def test_reference_matches_torch_autograd_in_float64():
    rng = np.random.default_rng(5)
    m, k, n = 37, 26, 100
    xin, w, bias = rng.standard_normal((m, k)), rng.standard_normal((n, k)) / 5, rng.standard_normal(n)
    gamma, beta, dy = 1 + 0.3 * rng.standard_normal(n), 0.3 * rng.standard_normal(n), rng.standard_normal((m, n))
    for relu in (True, False):
        t = [torch.from_numpy(a).requires_grad_(True) for a in (w, bias, gamma, beta)]
        zt = torch.from_numpy(xin) @ t[0].T + t[1]
        yt = torch.nn.functional.layer_norm(zt, (n,), t[2], t[3], 1e-5)
        (yt.relu() if relu else yt).backward(torch.from_numpy(dy))
        z = xin @ w.T + bias
        mean = z.mean(axis=1)
        rstd = 1 / np.sqrt(((z - mean[:, None]) ** 2).mean(axis=1) + 1e-5)
        dw, dgamma, dbeta, dbias = sk.backward(dy, xin, z, mean, rstd, gamma, beta, relu)[:4]
        for got, want in ((dw, t[0].grad), (dbias, t[1].grad), (dgamma, t[2].grad), (dbeta, t[3].grad)):
            np.testing.assert_allclose(got, want.numpy(), rtol=1e-11, atol=1e-12)


def test_reference_conventions():
    """an all-zero row of z with beta_j == 0 is an exact tie: mask32 false, not ambiguous, no gradient"""
    z = np.array([[0, 0, 0, 0], [1, 2, 3, 6]], np.float32)
    gamma, beta = np.array([1, -1, 2, 0], np.float32), np.array([0, 0, 0.5, 0], np.float32)
    mean, rstd = np.array([0, 3], np.float32), np.array([316.0, 0.5], np.float32)
    assert sk.mask32(z, mean, rstd, gamma, beta).tolist() == [[False, False, True, False], [False, True, True, False]]
    assert not sk.ambiguous(z, mean, rstd, gamma, beta)[0].any() and sk.ambiguous(z, mean, rstd, gamma, beta)[1].tolist() == [False] * 3 + [True]
    dbeta = sk.backward(np.ones((2, 4)), np.ones((2, 3)), z, mean, rstd, gamma, beta, True, sk.mask32(z, mean, rstd, gamma, beta))[2]
    assert dbeta.tolist() == [0, 1, 2, 0]
    assert sk.colsum_roundings("standalone", 1) == 16 + 3 + 5 + 3 and sk.colsum_roundings("standalone", sk.M_STRIDE) == 32 + 3 + 130 + 3
    assert sk.colsum_roundings("epilogue", 257) == 16 + 8 + 7 + 3


def test_case_tables_cover_what_the_kernels_switch_on():
    sa, ep = sk.cases("standalone"), sk.cases("epilogue")
    for cs_, ns, ms in ((sa, {4, 8, 64, 100, 200, 252, 256}, set(sk.SA_MS)), (ep, {4, 100, 200, 252, 256}, set(sk.EP_MS))):
        assert {c[1:3] for c in cs_} == set(sk.KLADDER) and {c[3] for c in cs_} == ns and {c[4] for c in cs_} == ms
        assert {c[5] for c in cs_} == {True, False}
    for kk in ((8, 8), (13, 13), (14, 14)):                               # both instantiations and K = 28 (the largest LDS request) at n = 256
        assert any(c[1:4] == kk + (256,) for c in sa)
    assert any(c[1:4] == (14, 14, 256) for c in ep)
    kinds = set()
    for c in sa + ep:
        kinds |= set(sk.plants(c[4], c[6]).values())
    assert kinds == set(lc.KINDS)


def test_faithful_emulation_stays_within_the_bounds_on_every_gpu_case():
    worst = {}
    for case in _all_cases():
        for deferred in (False, True):
            r = _emulated(case, deferred)
            key = (case[0], deferred)
            worst[key] = [max(a, b) for a, b in zip(worst.get(key, [0.0] * 4), r)]
            assert max(r) <= 1.0, (case, deferred, r)
    for (form, deferred), r in worst.items():
        print(f"faithful emulation, {form}{' (deferred fold)' if deferred else ''}: worst ratio to the bound  "
              + "  ".join(f"{nm} {v:.3f}" for nm, v in zip(sk.NAMES, r)))


@pytest.mark.parametrize("mutant", sk.MUTANTS)
def test_every_mutant_breaks_a_bound_by_ten_times(mutant):
    worst, where = 0.0, None
    cases = STRIDE_CASES if mutant == "second_trip_skipped" else _all_cases()[:-len(STRIDE_CASES)]
    for case in cases:
        form, k1, k2, n, m, relu, idx = case
        if (mutant == "inv_n_padded" and n == 256) or (mutant == "pad_column" and (k1 + k2) % 4 == 0) or (mutant == "a2_with_lda1" and k2 == 0) \
                or (mutant == "clamped_row_counted" and m % 2 == 0) or (mutant == "mask_xhat" and not relu):
            continue
        r = max(_emulated(case, False, mutant))
        if r > worst:
            worst, where = r, case
        if worst > 10.0:
            break
    print(f"mutant {mutant}: ratio to the bound {worst:.3e} at (form, k1, k2, n, M, relu, idx) = {where}")
    assert worst > 10.0


def test_float32_mask_equals_the_float64_mask_outside_the_exact_ties():
    """per row kind: elements where the reference's float32 mask is not to be trusted (smallk_ref.ambiguous).  The GPU tests give them
    dy = 0; here their share stays under the cap of layernorm_cases in every case (constant rows not counted, as there)."""
    count, total, worst = {}, {}, 0.0
    for case in _all_cases():
        if not case[5]:
            continue
        d, z, y, mean, rstd = _forward(case)
        m32 = sk.mask32(z, mean, rstd, d["gamma"], d["beta"])
        assert np.array_equal(y > 0, m32), case                          # the emulated forward's y > 0 IS mask32: the same arithmetic
        amb = sk.ambiguous(z, mean, rstd, d["gamma"], d["beta"])
        share = lc.neutralise(d["dy"], amb, z)[1]
        worst = max(worst, share)
        assert share <= lc.AMBIGUOUS_CAP, (case, share)
        for row in range(case[4] if case[4] < 1000 else 0):
            kind = d["plant"].get(row, "ordinary")
            count[kind] = count.get(kind, 0) + int(amb[row].sum())
            total[kind] = total.get(kind, 0) + amb.shape[1]
        tie = lc.zero_rows(z)[:, None] & (d["beta"] == 0)[None, :]
        assert not m32[tie].any() and not amb[tie].any()
    print("elements with an untrustworthy float32 mask per row kind: " + ", ".join(f"{k} {count[k]} of {total[k]}" for k in sorted(count))
          + f";  largest neutralised share of a case {100 * worst:.4f} %")
