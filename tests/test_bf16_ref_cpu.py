"""tests/bf16_ref.py on the CPU: the integer rounding against torch's bfloat16 conversion, the ELU band as a condition on the inputs of
the device test, the float64 product against a triple loop, and the properties the device tests rely on in the input makers."""
import numpy as np
import torch

from tests import bf16_ref as R


def _torch_bf16_bits(x32):
    return torch.from_numpy(np.ascontiguousarray(x32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_to_bf16_equals_torch_bit_for_bit_on_random_values_and_every_edge():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32)          # every exponent, subnormals and NaNs included
    x = np.concatenate([bits.view(np.float32), (3.0 * rng.standard_normal(20_000)).astype(np.float32), R.hand_list()])
    got, want = R.to_bf16(x), _torch_bf16_bits(x)
    nan = np.isnan(x)
    assert nan.sum() > 100 and (~nan).sum() > 200_000
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert R.is_nan_bf16(got[nan]).all() and R.is_nan_bf16(want[nan]).all()
    np.testing.assert_array_equal(R.from_bf16(got[~nan]).view(np.uint32), got[~nan].astype(np.uint32) << 16)


def test_to_bf16_edges_by_hand():
    def f(bits):
        return int(R.to_bf16(np.array([bits], dtype=np.uint32).view(np.float32))[0])
    assert f(0x3F808000) == 0x3F80 and f(0x3F818000) == 0x3F82                         # ties: to the even mantissa
    assert f(0x3F807FFF) == 0x3F80 and f(0x3F808001) == 0x3F81
    assert f(R.FLT_MAX_BITS) == 0x7F80 and f(R.FIRST_TO_INF_BITS) == 0x7F80 and f(R.FIRST_TO_INF_BITS - 1) == 0x7F7F
    assert f(0x80000000 | R.FIRST_TO_INF_BITS) == 0xFF80
    assert f(0x00000000) == 0x0000 and f(0x80000000) == 0x8000 and f(0x7F800000) == 0x7F80 and f(0xFF800000) == 0xFF80
    assert f(0x00008000) == 0x0000 and f(0x00008001) == 0x0001 and f(0x00018000) == 0x0002    # 2^-134 ties to 0; subnormals kept
    assert f(0x00000001) == 0x0000 and f(0x80000001) == 0x8000                         # 2^-149 -> a zero of its sign
    x = np.array([1e-40, 2.0 ** -133], dtype=np.float32)
    assert (R.from_bf16(R.to_bf16(x)) > 0).all()
    for nan in (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001):
        assert R.is_nan_bf16(f(nan)), hex(nan)
    h = R.hand_list()
    assert np.isnan(h).sum() >= 5 and (np.abs(h[np.isfinite(h)]) < 2.0 ** -126).sum() >= 256 and np.isinf(h).sum() == 2


def test_elu_bf16_neighbours_fixed_points_and_band_share():
    rng = np.random.default_rng(1)
    x = (3.0 * rng.standard_normal(100_000)).astype(np.float32)
    want, lo, hi, band = R.elu_bf16(x)
    neg = x <= 0
    share = band[neg].mean()
    print(f"in_band share of non-positive 3 * randn inputs: {100 * share:.3f} % of {int(neg.sum())}")
    assert 0 < share <= 0.01
    assert not band[~neg].any()
    e = np.where(x > 0, x.astype(np.float64), np.expm1(x.astype(np.float64)))
    lo64, hi64 = R.from_bf16(lo).astype(np.float64), R.from_bf16(hi).astype(np.float64)
    assert (lo64 <= e).all() and (e <= hi64).all()
    step = R._ordinal(hi) - R._ordinal(lo)
    assert set(np.unique(step)) <= {0, 1}                                              # neighbours, or the value itself
    assert ((want == lo) | (want == hi)).all()
    np.testing.assert_array_equal(want[~neg], R.to_bf16(x[~neg]))                      # positive values: the plain rounding
    # the fixed points
    inf = np.float32(np.inf)
    fx = np.array([0.0, -0.0, inf, -inf, -20.0, -25.0, -100.0, -1e30, np.nan, 2.5], dtype=np.float32)
    w, l, h, b = R.elu_bf16(fx)
    assert list(w[:8]) == [0x0000, 0x8000, 0x7F80, 0xBF80, 0xBF80, 0xBF80, 0xBF80, 0xBF80]
    assert R.is_nan_bf16(w[8]) and w[9] == 0x4020 and not b.any()
    assert (l[:4] == w[:4]).all() and (h[:4] == w[:4]).all()                           # exact values: no neighbours
    assert (l[4:8] == 0xBF80).all() and (h[4:6] == 0xBF7F).all() and (h[6:8] == 0xBF80).all()   # just above -1; -1 in float64
    # the whole hand list goes through without a warning or an out-of-order neighbour
    w, l, h, b = R.elu_bf16(R.hand_list())
    ok = ~R.is_nan_bf16(w)
    assert (R._ordinal(l[ok]) <= R._ordinal(w[ok])).all() and (R._ordinal(w[ok]) <= R._ordinal(h[ok])).all()


def test_gemm_equals_a_float64_triple_loop_and_follows_ieee_on_non_finite_operands():
    a, b = R.normal(5, 3, 16, 0)
    c, unit = R.gemm(a, b)
    af, bf = R.from_bf16(a), R.from_bf16(b)
    for i in range(5):
        for j in range(3):
            s, u = 0.0, 0.0
            for k in range(16):
                s += float(af[i, k]) * float(bf[j, k])
                u += abs(float(af[i, k])) * abs(float(bf[j, k]))
            assert abs(c[i, j] - s) <= 4 * 2.0 ** -53 * u and abs(unit[i, j] - u * 2.0 ** -24) <= 1e-12 * unit[i, j]
    a, b = a.copy(), b.copy()
    a[0, 0], a[1, 1], a[1, 2] = 0x0000, 0x7F80, 0xFF80                                 # 0, +inf, -inf
    b[0, 0], b[1, 1], b[1, 2] = 0x7F80, 0x3F80, 0x3F80                                 # inf; 1, 1
    a[2, 5] = 0x7FC0
    c, _ = R.gemm(a, b)
    assert np.isnan(c[0, 0])                                                           # 0 * inf
    assert np.isnan(c[1, 1])                                                           # inf - inf
    assert np.isnan(c[2]).all() and np.isfinite(c[3:, 1:]).all() and np.isfinite(c[0, 1:]).all()
    assert np.isinf(c[3:, 0]).all() and (np.sign(c[3:, 0]) == np.sign(R.from_bf16(a[3:, 0]))).all()      # x * inf keeps x's sign


def test_exact_regimes_are_exactly_representable_in_fp32():
    for kind in ("integers", "one_hot"):
        for m, n, k in [(33, 36, 24), (65, 129, 72), (257, 257, 1024), (5, 9, 0)]:
            a, b = R.MAKERS[kind](m, n, k, 7)
            c, unit = R.gemm(a, b)
            assert c.shape == (m, n)
            np.testing.assert_array_equal(c, c.astype(np.float32).astype(np.float64))
            if kind == "integers":
                assert unit.max() * 2.0 ** 24 < 2.0 ** 24 if k else (c == 0).all()     # every partial sum stays an exact integer
            elif k:
                assert (np.count_nonzero(R.from_bf16(a), axis=1) == 1).all() and (c != 0).all()
                assert np.array_equal(np.nonzero(a)[1], (7 * np.arange(m)) % k)


def test_rounding_regimes_have_the_properties_their_names_promise():
    m, n, k = 64, 48, 40
    a, b = R.cancelling(m, n, k, 3)
    c, unit = R.gemm(a, b)
    assert np.median(np.abs(c) / (unit * 2.0 ** 24)) < 1e-3                            # |C| << sum |a b|
    a, b = R.wide(m, n, k, 3)
    mag = np.abs(R.from_bf16(a)).max(axis=1)
    assert mag.max() / mag.min() > 2.0 ** 30
    a, b = R.MAKERS["tiny(-70)"](m, n, k, 3)
    c, unit = R.gemm(a, b)
    assert 0 < np.abs(c).max() < 2.0 ** -126                                           # fp32 subnormal results
    a, b = R.MAKERS["tiny(-60)"](m, n, k, 3)
    assert (R.from_bf16(a) != 0).mean() > 0.99
    assert R.cast_inputs(3, 7, 0).shape == (3, 7) and np.isin(R.hand_list(), R.cast_inputs(300, 13, 0)).mean() > 0.9
