"""The GAT's bf16 projection (csrc/gemm_bf16.hip) against the references of tests/bf16_ref.py: gte_cast_bf16 bit for bit against the
integer rounding and a float64 ELU, gte_gemm_bf16_nt bit for bit where the arithmetic is exact and in rounding units where it is
not, both store epilogues, the argument checks, and _Linear / the bf16 hand-off of components/graphs/gat.py.  The C entry points
are called through ``_lib`` directly so that strides, padding and alignment are the test's.  Every output is a window of a larger
buffer filled with a sentinel, and everything outside the window must still be the sentinel afterwards.

Rounding bounds of the product, in units of unit = 2^-24 sum_k |a_k b_k| (one fp32 rounding at the magnitude of the dot product):
  derived     products of bf16 values are exact in fp32 (8 x 8 significand bits), so any order of correctly rounded fp32 additions
              stays within K units;
  yardstick   the fp32 MFMA kernel (ops.gemm in f32 mode, not code under test) on the same operands widened to fp32: the bf16
              kernel's largest error is at most 1.25 x that kernel's + 1 (the convention of tests/test_gemm_split.py without its
              allowance for dropped split terms).

Measured on an MI355X (``pytest -s`` prints every case and this table): largest error of the bf16 kernel / of the fp32 MFMA kernel, in
units, per regime and shape (M, N, K):

regime       (300,256,832)  (257,36,256)  (129,130,40)  (1000,64,16)  (64,256,1024)
normal        1.898/0.806    1.150/1.587   1.001/1.587   1.164/1.626    1.605/0.584
wide          1.633/1.020    1.414/1.640   1.229/1.410   1.251/1.564    1.534/0.573
cancelling    0.008/0.019    0.023/0.029   0.142/0.197   0.314/0.361    0.006/0.013
tiny(-60)     1.898/0.806    1.150/1.587   1.001/1.587   1.164/1.626    1.605/0.584

Every entry is far inside K units; the closest to 1.25 x fp32 + 1 is normal at (300, 256, 832): 1.898 against 2.008.  tiny(-60) takes
the draws of normal scaled by 2^-60 and reproduces its figures digit for digit, although a good part of its products lies below
2^-126: neither kernel flushes or rounds a subnormal product.  tiny(-70), where every product and every result (largest 2^-133) is an
fp32 subnormal: nothing was flushed -- the largest error beyond K units is 5 x 2^-149 (the products themselves no longer fit the
subnormal grid) against the (K + 1) 2^23 x 2^-149 the bound allows, and of 183 206 results two are 0 where the exact value is just
above 2^-148.  _Linear's gradients in the split mode: dx 3.0 / dw 2.8 units at (257, 40 -> 36), 4.0 / 4.9 at (300, 831 -> 64).

gte_cast_bf16 with ELU: outside the band of tests/bf16_ref.elu_bf16 (16 fp32 ulps around a bf16 midpoint) every result equalled the
float64 ELU rounded to bf16; ELU(-0) came out as +0 until the kernel kept zeros out of expm1f.
"""
import functools
import threading

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import bf16_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1
SENT = float(np.float32(7.5e29))        # fp32 outputs: never a result of these inputs
SENT_B = 0x5A5A                         # bf16 outputs (a finite bf16 pattern none of the inputs rounds to by accident in bulk)
NAN_B = 0x7FC0                          # padding of the operands past K: reading it shows
WORST = {}                              # (regime, shape) -> (bf16 kernel, fp32 kernel), largest error in units


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k):
    """operands and reference of one case, made once and shared (nobody writes to them)"""
    a, b = R.MAKERS[kind](m, n, k, 1000003 * m + 1009 * n + k)
    c, unit = R.gemm(a, b)
    for x in (a, b, c, unit):
        x.setflags(write=False)
    return a, b, c, unit


def dev_bits(bits, ld, pad=NAN_B):
    """device image [rows, ld] of a bf16 matrix (int16 storage); the columns past its own and a tail hold ``pad``"""
    rows, cols = bits.shape
    host = np.full((rows, ld), pad, dtype=np.uint16)
    host[:, :cols] = bits
    flat = np.concatenate([host.reshape(-1), np.full(8, pad, dtype=np.uint16)])
    return torch.from_numpy(flat.view(np.int16)).to(DEV)


def run_gemm(a_bits, b_bits, lda=None, ldb=None, col0=3, extra_cols=5, extra_rows=2):
    """gte_gemm_bf16_nt into the window [0:M, col0:col0+N] of a sentinel-filled buffer: (the window, nothing else was written)"""
    lib, st = _lib.load(), _lib.current_stream()
    (m, k), n = a_bits.shape, b_bits.shape[0]
    lda, ldb = k if lda is None else lda, k if ldb is None else ldb
    A, B = dev_bits(a_bits, lda), dev_bits(b_bits, ldb)
    ldc = col0 + n + extra_cols
    buf = torch.full((m + extra_rows, ldc), SENT, dtype=torch.float32, device=DEV)
    c_ptr = buf.data_ptr() + 4 * col0
    assert col0 != 3 or c_ptr % 16 == 12
    _lib.check(lib.gte_gemm_bf16_nt(A.data_ptr(), lda, B.data_ptr(), ldb, c_ptr, ldc, m, n, k, st), "gte_gemm_bf16_nt")
    win = buf[:m, col0:col0 + n].cpu().numpy()
    buf[:m, col0:col0 + n] = SENT
    return win, bool((buf == SENT).all())


def units(got, c, unit):
    return float((np.abs(got.astype(np.float64) - c) / np.maximum(unit, 1e-300)).max()) if c.size else 0.0


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nregime / shape: largest error of the bf16 kernel (of the fp32 MFMA kernel), in units 2^-24 sum |a b|")
        for k in sorted(WORST):
            print(f"{k[0]:<11} {str(k[1]):<18} {WORST[k][0]:7.2f} ({WORST[k][1]:.2f})")


# ---------------------------------------------------------------------------------------------------------------------
# (a) gte_cast_bf16
# ---------------------------------------------------------------------------------------------------------------------
CAST_SHAPES = [(1, 1, 0, 0), (3, 7, 2, 8), (65, 8, 0, 0), (257, 9, 3, 16), (300, 13, 0, 8), (33, 831, 1, 0), (1000, 64, 0, 8),
               (2, 1024, 0, 0)]


def run_cast(x, ldx, ldy, act, extra_rows=2):
    """gte_cast_bf16 of the host matrix x into a sentinel-filled [rows + extra_rows, ldy] buffer, returned whole as bits"""
    lib, st = _lib.load(), _lib.current_stream()
    rows, cols = x.shape
    xh = np.full((rows, ldx), np.float32(np.nan), dtype=np.float32)          # what lies past cols must not reach the padding
    xh[:, :cols] = x
    xd = torch.from_numpy(xh).to(DEV)
    yd = torch.full((rows + extra_rows, ldy), SENT_B, dtype=torch.int16, device=DEV)
    _lib.check(lib.gte_cast_bf16(xd.data_ptr(), ldx, yd.data_ptr(), ldy, rows, cols, act, st), "gte_cast_bf16")
    return yd.cpu().numpy().view(np.uint16)


def check_cast_frame(y, rows, cols):
    cp = -(-cols // 8) * 8
    assert (y[:rows, cols:cp] == 0).all(), "padding columns must be +0"
    assert (y[:rows, cp:] == SENT_B).all() and (y[rows:] == SENT_B).all(), "written past cols_pad or past the last row"


@pytest.mark.parametrize("rows,cols,dx,dy", CAST_SHAPES)
def test_cast_is_round_to_nearest_even_bit_for_bit(rows, cols, dx, dy):
    x = R.cast_inputs(rows, cols, 17 * rows + cols)
    cp = -(-cols // 8) * 8
    y = run_cast(x, cols + dx, cp + dy, 0)
    check_cast_frame(y, rows, cols)
    got, want = y[:rows, :cols], R.to_bf16(x)
    nan = np.isnan(x)
    assert np.array_equal(R.is_nan_bf16(got), nan)
    bad = (got != want) & ~nan
    assert not bad.any(), [(hex(int(b)), hex(int(g)), hex(int(w))) for b, g, w in
                           zip(x[bad].view(np.uint32)[:8], got[bad][:8], want[bad][:8])]


@pytest.mark.parametrize("rows,cols,dx,dy", CAST_SHAPES)
def test_cast_through_elu_equals_the_float64_elu_outside_the_rounding_band(rows, cols, dx, dy):
    x = R.cast_inputs(rows, cols, 17 * rows + cols)
    want, lo, hi, band = R.elu_bf16(x)
    # the band holds 0.06 % of 3 * randn (tests/test_bf16_ref_cpu.py caps it at 1 %) and, by construction, the hand list's small
    # negative ties: there expm1(v) = v to far below an fp32 ulp, which IS a rounding midpoint
    drawn = (x <= 0) & ~np.isin(x, R.hand_list())
    assert drawn.sum() < 100 or band[drawn].mean() <= 0.01                  # a condition on the inputs, not a tolerance
    cp = -(-cols // 8) * 8
    y = run_cast(x, cols + dx, cp + dy, 1)
    check_cast_frame(y, rows, cols)
    got = y[:rows, :cols]
    nan = np.isnan(x)
    assert np.array_equal(R.is_nan_bf16(got), nan)
    bad = (got != want) & ~nan & ~band
    assert not bad.any(), [(float(v), hex(int(v_)), hex(int(g)), hex(int(w))) for v, v_, g, w in
                           zip(x[bad][:8], x[bad].view(np.uint32)[:8], got[bad][:8], want[bad][:8])]
    gv = R.from_bf16(got[band])
    assert ((gv == R.from_bf16(lo[band])) | (gv == R.from_bf16(hi[band]))).all()
    pos = x > 0
    np.testing.assert_array_equal(got[pos], R.to_bf16(x[pos]))


def test_cast_elu_fixed_points():
    inf = np.float32(np.inf)
    x = np.array([[0.0, -0.0, inf, -inf, -20.0, -25.0, -100.0, -1e30, -3.0e38, np.nan, 2.5, 1e-40, 3.3e38]], dtype=np.float32)
    want = [0x0000, 0x8000, 0x7F80, 0xBF80, 0xBF80, 0xBF80, 0xBF80, 0xBF80, 0xBF80, None, 0x4020] + [int(w) for w in R.to_bf16(x[0, 11:])]
    y = run_cast(x, x.shape[1], 16, 1)
    check_cast_frame(y, 1, x.shape[1])
    for j, w in enumerate(want):
        if w is None:
            assert R.is_nan_bf16(y[0, j])
        else:
            assert int(y[0, j]) == w, (j, float(x[0, j]), hex(int(y[0, j])), hex(w))


# ---------------------------------------------------------------------------------------------------------------------
# (b) the product where fp32 accumulation is exact
# ---------------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(1, 1, 8), (31, 9, 16), (33, 36, 24), (63, 127, 32), (64, 128, 40), (65, 129, 72), (127, 257, 64), (128, 130, 832),
                (129, 1, 256), (257, 257, 1024), (897, 128, 16), (129, 1025, 8), (5, 9, 0)]


@pytest.mark.parametrize("kind", ["integers", "one_hot"])
@pytest.mark.parametrize("m,n,k", EXACT_SHAPES)
def test_gemm_is_bit_exact_where_fp32_accumulation_is(kind, m, n, k):
    a, b, c, unit = case(kind, m, n, k)
    want = c.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), c)
    if kind == "integers":
        assert unit.size == 0 or unit.max() * 2.0 ** 24 < 2.0 ** 24        # every partial sum is an integer below 2^24
    if k == 0:
        assert (want == 0).all()
    for lda in (k, k + 8):
        for ldb in (k, k + 8):
            got, clean = run_gemm(a, b, lda, ldb)
            diff = got.view(np.uint32) != want.view(np.uint32)
            assert not diff.any(), (lda, ldb, int(diff.sum()), np.argwhere(diff)[:4].tolist())
            assert clean, (lda, ldb, "wrote outside the [M, N] window")


# ---------------------------------------------------------------------------------------------------------------------
# (c) the product's rounding
# ---------------------------------------------------------------------------------------------------------------------
ROUND_SHAPES = [(300, 256, 832), (257, 36, 256), (129, 130, 40), (1000, 64, 16), (64, 256, 1024)]


def fp32_kernel(a_bits, b_bits):
    a32, b32 = torch.from_numpy(R.from_bf16(a_bits)).to(DEV), torch.from_numpy(R.from_bf16(b_bits)).to(DEV)
    prev = ops.set_gemm_mode("f32")
    try:
        return ops.gemm(a32, b32, trans_b=True).cpu().numpy()
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.parametrize("kind", ["normal", "wide", "cancelling", "tiny(-60)"])
@pytest.mark.parametrize("m,n,k", ROUND_SHAPES)
def test_gemm_rounding_within_k_units_and_not_above_the_fp32_kernel(kind, m, n, k):
    a, b, c, unit = case(kind, m, n, k)
    got, clean = run_gemm(a, b)
    e_bf, e_32 = units(got, c, unit), units(fp32_kernel(a, b), c, unit)
    WORST[(kind, (m, n, k))] = (e_bf, e_32)
    print(f"{kind} {(m, n, k)}: bf16 kernel {e_bf:.3f} units, fp32 kernel {e_32:.3f} units")
    assert clean
    assert np.isfinite(got).all()
    assert e_bf <= k, (e_bf, k)
    assert e_bf <= 1.25 * e_32 + 1.0, (e_bf, e_32)


@pytest.mark.parametrize("m,n,k", ROUND_SHAPES)
def test_gemm_of_subnormal_products_loses_less_than_a_flush_per_term(m, n, k):
    a, b, c, unit = case("tiny(-70)", m, n, k)
    got, clean = run_gemm(a, b)
    err = np.abs(got.astype(np.float64) - c)
    over = float((err - k * unit).max())
    zeros = int(((got == 0) & (np.abs(c) > 2.0 ** -148)).sum())
    print(f"tiny(-70) {(m, n, k)}: largest error beyond K units {over / 2.0 ** -149:.2f} x 2^-149 (allowed {(k + 1) * 2 ** 23}); "
          f"{zeros} of {c.size} results are 0 where the product is above 2^-148; max |C| = 2^{np.log2(np.abs(c).max()):.1f}")
    assert clean
    assert (err <= k * unit + (k + 1) * 2.0 ** -126).all()


# ---------------------------------------------------------------------------------------------------------------------
# (d) non-finite operands
# ---------------------------------------------------------------------------------------------------------------------
def test_gemm_non_finite_operands_reach_the_outputs_ieee_says_and_nothing_outside_the_window():
    m, n, k = 129, 130, 40
    a, b, _, _ = case("normal", m, n, k)
    a, b = a.copy(), b.copy()
    INF, NINF, ONE = 0x7F80, 0xFF80, 0x3F80
    a[20, 9] = NAN_B                                       # a NaN in A: row 20 of C
    a[5, 3], a[5, 4] = 0x0000, ONE                         # the chosen row: a zero and a non-zero value ...
    b[7, 3], b[7, 4] = INF, NINF                           # ... against +inf and -inf in one row of B: column 7 of C
    a[40, 10], a[40, 12] = INF, NINF                       # +inf in A against a -inf product in the same dot product: row 40
    a[128, 6] = INF                                        # the second row tile, whose 127 rows past M are staged zeros
    b[129, 5] = NINF                                       # the second column tile, whose columns past N are staged zeros
    c, unit = R.gemm(a, b)
    assert np.isnan(c[5, 7]) and np.isnan(c[20]).all() and np.isnan(c[40]).any() and np.isinf(c[40]).any()
    assert np.isnan(c[:, 7]).sum() > 10 and np.isinf(c[:, 7]).sum() > 10 and np.isinf(c[128]).sum() > 100
    got, clean = run_gemm(a, b, k + 8, k + 8)
    assert np.array_equal(np.isnan(got), np.isnan(c))
    assert np.array_equal(got == np.inf, c == np.inf) and np.array_equal(got == -np.inf, c == -np.inf)
    fin = np.isfinite(c)
    assert fin.sum() > 0.9 * c.size
    assert (np.abs(got[fin].astype(np.float64) - c[fin]) <= k * unit[fin]).all()
    assert clean, "0 * inf of the staged rows / columns past M / N reached memory"


# ---------------------------------------------------------------------------------------------------------------------
# (e) the two store epilogues
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,ldc,plain", [(2, 130, 4_128_000, False), (2, 130, 4_130_000, True), (130, 130, 2_080_000, False),
                                           (130, 130, 2_100_000, True)],
                         ids=["descriptor-17MB", "plain-17MB", "descriptor-1GB-offsets-near-2^31", "plain-1GB-four-tiles"])
def test_gemm_store_epilogues_write_the_window_and_nothing_else(m, n, ldc, plain):
    """the kernel takes the buffer-descriptor stores while (M + 128) ldc 4 < 2^31 and plain guarded stores beyond.  What this pins is
    each path's own result next to the switch, not the switch: it is conservative (the largest row a tile touches is below M + 128, and
    an int offset that wraps lands above 2^31, outside every descriptor), so a kernel forced onto the descriptor stores passes the
    two plain cases as well -- only a C of 2 GB and more, whose descriptor size no longer fits an int, could tell."""
    assert ((m + 128) * ldc * 4 >= 2 ** 31) == plain
    k = 40
    lib, st = _lib.load(), _lib.current_stream()
    a, b, c, _ = case("integers", m, n, k)
    want = c.astype(np.float32)
    A, B = dev_bits(a, k), dev_bits(b, k)
    col0 = 3
    flat = torch.full((col0 + (m - 1) * ldc + n + 61,), SENT, dtype=torch.float32, device=DEV)
    try:
        _lib.check(lib.gte_gemm_bf16_nt(A.data_ptr(), k, B.data_ptr(), k, flat.data_ptr() + 4 * col0, ldc, m, n, k, st),
                   "gte_gemm_bf16_nt")
        changed = int(torch.count_nonzero(flat != SENT))
        got = torch.as_strided(flat, (m, n), (ldc, 1), col0).cpu().numpy()
    finally:
        del flat
        torch.cuda.empty_cache()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert changed == int((want != np.float32(SENT)).sum()) == m * n


# ---------------------------------------------------------------------------------------------------------------------
# (f) argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_their_codes_without_a_launch():
    """every buffer is large enough for the call even if a check were missing"""
    lib, st = _lib.load(), _lib.current_stream()
    x = torch.zeros(4096, dtype=torch.float32, device=DEV)
    y = torch.full((4096,), SENT_B, dtype=torch.int16, device=DEV)
    c = torch.full((4096,), SENT, dtype=torch.float32, device=DEV)
    ab = torch.zeros(4096, dtype=torch.int16, device=DEV)
    px, py, pc, pa = x.data_ptr(), y.data_ptr(), c.data_ptr(), ab.data_ptr()

    def cast(x=px, ldx=16, y=py, ldy=16, rows=4, cols=13, act=0):
        return lib.gte_cast_bf16(x, ldx, y, ldy, rows, cols, act, st)

    def gemm(A=pa, lda=16, B=pa, ldb=16, C=pc, ldc=16, M=4, N=9, K=16):
        return lib.gte_gemm_bf16_nt(A, lda, B, ldb, C, ldc, M, N, K, st)

    assert cast(rows=-1) == INVALID and cast(cols=0) == INVALID and cast(cols=-3) == INVALID
    assert cast(ldx=12) == INVALID and cast(ldy=8) == INVALID and cast(ldy=20) == INVALID
    assert cast(y=py + 8) == INVALID and cast(y=py + 2) == INVALID
    assert cast(act=2) == INVALID and cast(act=-1) == INVALID
    assert cast(x=0) == INVALID and cast(y=0) == INVALID
    assert b"cast_bf16" in lib.gte_last_error()
    assert cast(rows=0, x=0, y=0) == 0
    assert gemm(M=-1) == INVALID and gemm(N=-1) == INVALID and gemm(K=-8) == INVALID
    assert gemm(K=12, lda=16, ldb=16) == INVALID and gemm(lda=20) == INVALID and gemm(ldb=20) == INVALID
    assert gemm(lda=8) == INVALID and gemm(ldb=8) == INVALID and gemm(ldc=8) == INVALID
    assert gemm(A=pa + 8) == INVALID and gemm(B=pa + 8) == INVALID
    assert gemm(A=0) == INVALID and gemm(B=0) == INVALID and gemm(C=0) == INVALID
    assert b"gemm_bf16_nt" in lib.gte_last_error()
    assert gemm(M=0, A=0, B=0, C=0) == 0 and gemm(N=0, A=0, B=0, C=0) == 0
    torch.cuda.synchronize()
    assert bool((y == SENT_B).all()) and bool((c == SENT).all())          # no refused call launched anything
    assert cast() == 0 and gemm() == 0                                     # the valid calls these are variations of
    torch.cuda.synchronize()
    assert not bool((y[:64] == SENT_B).any()) and bool((y[64:] == SENT_B).all())
    cw = c[:64].view(4, 16)
    assert bool((cw[:, :9] == 0).all()) and bool((cw[:, 9:] == SENT).all()) and bool((c[64:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# (g) _Linear and the hand-off between GAT layers
# ---------------------------------------------------------------------------------------------------------------------
def _pad8(bits):
    rows, cols = bits.shape
    out = np.zeros((rows, -(-cols // 8) * 8), dtype=np.uint16)
    out[:, :cols] = bits
    return out


@pytest.fixture
def f32_process_mode():
    """the process-wide GEMM mode set to the one _Linear.backward does NOT use, so that a mode left behind shows"""
    prev = ops.set_gemm_mode("f32")
    try:
        yield ops.GEMM_F32
    finally:
        _lib.load().gte_gemm_set_thread_mode(-1)
        ops.set_gemm_mode(prev)


class _ModeProbe(torch.autograd.Function):
    seen = []

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        _ModeProbe.seen.append((threading.get_ident(), _lib.load().gte_gemm_get_mode()))
        return g


def mode_in_the_backward_thread():
    """(thread, GEMM mode that thread would run in) of autograd's backward thread of the device: the override _Linear.backward
    sets is per host thread, so the thread that calls .backward() cannot see a mode that was left behind"""
    t = torch.zeros(1, device=DEV, requires_grad=True)
    _ModeProbe.seen.clear()
    _ModeProbe.apply(t).sum().backward()
    return _ModeProbe.seen[0]


@pytest.mark.parametrize("n,fin,fout", [(257, 40, 36), (300, 831, 64)])
def test_linear_bf16_forward_is_the_c_abi_product_and_its_gradients_are_fp32_accurate(n, fin, fout, f32_process_mode, monkeypatch):
    from gnn_tableextraction_amd.components.graphs.gat import _Linear
    lib = _lib.load()
    g = torch.Generator().manual_seed(n + fin)
    x, w, dy = torch.randn(n, fin, generator=g), torch.randn(fout, fin, generator=g) * 0.1, torch.randn(n, fout, generator=g)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    z = _Linear.apply(xd, wd, None, True)
    a_bits, b_bits = _pad8(R.to_bf16(x.numpy())), _pad8(R.to_bf16(w.numpy()))
    want, clean = run_gemm(a_bits, b_bits)
    assert clean and np.array_equal(z.detach().cpu().numpy().view(np.uint32), want.view(np.uint32))
    c, unit = R.gemm(a_bits, b_bits)
    assert units(want, c, unit) <= a_bits.shape[1]

    seen, real = [], ops.gemm
    monkeypatch.setattr(ops, "gemm", lambda *p, **kw: (seen.append((threading.get_ident(), lib.gte_gemm_get_mode())), real(*p, **kw))[1])
    z.backward(dy.to(DEV))
    monkeypatch.setattr(ops, "gemm", real)
    assert [mode for _, mode in seen] == [ops.GEMM_SPLIT_BF16, ops.GEMM_SPLIT_BF16]      # dX and dW ran in the split mode ...
    assert mode_in_the_backward_thread() == (seen[0][0], f32_process_mode)              # ... and that thread is back in the process mode
    assert lib.gte_gemm_get_mode() == f32_process_mode
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (x64 @ w64.t()).backward(dy.double())
    u_dx = (dy.double().abs() @ w.double().abs()) * 2.0 ** -24
    u_dw = (dy.double().abs().t() @ x.double().abs()) * 2.0 ** -24
    e_dx = float(((xd.grad.cpu().double() - x64.grad).abs() / u_dx).max())
    e_dw = float(((wd.grad.cpu().double() - w64.grad).abs() / u_dw).max())
    print(f"_Linear backward ({n}, {fin} -> {fout}): dx {e_dx:.2f} units, dw {e_dw:.2f} units")
    assert e_dx < 12.0 and e_dw < 12.0, (e_dx, e_dw)


def test_linear_backward_restores_the_gemm_mode_when_a_gemm_raises(f32_process_mode, monkeypatch):
    from gnn_tableextraction_amd.components.graphs.gat import _Linear
    lib = _lib.load()
    xd = torch.randn(33, 16, device=DEV).requires_grad_(True)
    wd = torch.randn(9, 16, device=DEV).requires_grad_(True)
    z = _Linear.apply(xd, wd, None, True)
    seen = []

    def boom(*p, **kw):
        seen.append((threading.get_ident(), lib.gte_gemm_get_mode()))
        raise RuntimeError("gemm made to fail")
    monkeypatch.setattr(ops, "gemm", boom)
    with pytest.raises(RuntimeError, match="gemm made to fail"):
        z.backward(torch.ones_like(z))
    monkeypatch.undo()
    assert [mode for _, mode in seen] == [ops.GEMM_SPLIT_BF16]
    assert mode_in_the_backward_thread() == (seen[0][0], f32_process_mode)
    assert lib.gte_gemm_get_mode() == f32_process_mode


def _graph(n, e, seed):
    from gnn_tableextraction_amd import graph as G
    rng = np.random.default_rng(seed)
    return G.PageGraph(rng.integers(0, n, e), rng.integers(0, n, e), n, device=DEV)


def test_hand_off_copy_gives_the_projection_of_the_cast_route_bit_for_bit():
    from gnn_tableextraction_amd.components.graphs.gat import GATLayer, _Linear
    n = 300
    g = _graph(n, 2500, 5)
    torch.manual_seed(3)
    kw = dict(gather_dtype=torch.bfloat16, compute_dtype=torch.bfloat16)
    l1, l2 = GATLayer(13, 16, 4, **kw).to(DEV), GATLayer(64, 8, 4, **kw).to(DEV)
    x = torch.randn(n, 13, device=DEV) * 3.0
    with torch.no_grad():
        out, out_b = l1(g, x, None, fuse_elu=True, emit_bf16=True)
        assert out_b is not None and out_b.shape == (n, 64) and out_b.dtype == torch.bfloat16
        bits = out_b.view(torch.int16).cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(bits, R.to_bf16(out.cpu().numpy()))         # the copy IS the rounding of the fp32 output
        z_copy, z_cast = _Linear.apply(out, l2.fc, out_b, True), _Linear.apply(out, l2.fc, None, True)
        assert torch.equal(z_copy, z_cast)
        want, clean = run_gemm(bits, R.to_bf16(l2.fc.detach().cpu().numpy()))
        assert clean and np.array_equal(z_copy.cpu().numpy().view(np.uint32), want.view(np.uint32))
        (o_copy, _), (o_cast, _) = l2(g, out, out_b, fuse_elu=True), l2(g, out, None, fuse_elu=True)
        assert torch.equal(o_copy, o_cast)


def test_no_hand_off_copy_where_the_width_is_no_multiple_of_eight():
    from gnn_tableextraction_amd.components.graphs.gat import GATLayer, _Linear, _bf16_copy
    n = 120
    g = _graph(n, 900, 6)
    torch.manual_seed(4)
    kw = dict(gather_dtype=torch.bfloat16, compute_dtype=torch.bfloat16)
    l1, l2 = GATLayer(9, 7, 3, **kw).to(DEV), GATLayer(21, 5, 3, **kw).to(DEV)
    x = torch.randn(n, 9, device=DEV)
    with torch.no_grad():
        out, out_b = l1(g, x, None, fuse_elu=True, emit_bf16=True)
        assert out_b is None and out.shape == (n, 21)
        o2, _ = l2(g, out, out_b, fuse_elu=True)
        assert o2.shape == (n, 15) and bool(torch.isfinite(o2).all())
        xb = _bf16_copy(out)
        assert xb.shape == (n, 24) and bool((xb[:, 21:] == 0).all())
        assert torch.equal(_Linear.apply(out, l2.fc, None, True), _Linear.apply(out, l2.fc, xb, True))
