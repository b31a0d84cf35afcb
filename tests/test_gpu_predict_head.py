"""gte_predict_head / ops.predict_head against tests/predict_head_ref.py (numpy float64, written from the contract in
include/gte.h) on the case table of that file: n in {0, 1, 63, 64, 65, 257} x (C, ld) x normal rows scaled by 1, 30 and 1e4 with
the special rows (ties, -inf, +inf, NaN, +-3.0e38) among them.  The padding columns of the logits are NaN -- a kernel that reads
them answers wrongly -- and every output lies inside a frame of sentinels that must stay as it was.

Tolerance.  pred is exact.  conf / prob: NaN exactly where the reference has NaN, elsewhere float32(reference) or the float32 next
to it: the device's and numpy's double exp each err by about 1 ulp of double, 2^-28 of a float32 ulp, so only a value on a float32
rounding boundary can differ, and then by one."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, ops
from tests import predict_head_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID_ARGUMENT = -1                                                   # GTE_ERR_INVALID_ARGUMENT of include/gte.h
SENT_I, SENT_F = -7777, -123.25


@pytest.fixture(scope="module")
def table():
    """[(n, C, ld, logits, (pred, conf, prob) of the reference)]: computed once."""
    return [(n, c, ld, x, ref.predict_head(x)) for n, c, ld, x in ref.cases()]


def padded(x, ld):
    """x [n, C] as a view of a device matrix [n, ld] whose other columns are NaN"""
    full = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    full[:, :x.shape[1]] = torch.from_numpy(x).to(DEV)
    return full[:, :x.shape[1]]


def framed(n, c):
    """pred, conf and prob as views into buffers that hold a sentinel everywhere -> (views, buffers)"""
    bp = torch.full((n + 2,), SENT_I, dtype=torch.int64, device=DEV)
    bc = torch.full((n + 2,), SENT_F, dtype=torch.float32, device=DEV)
    bq = torch.full((n + 2, c + 3), SENT_F, dtype=torch.float32, device=DEV)
    return (bp[1:n + 1], bc[1:n + 1], bq[1:n + 1, 1:c + 1]), (bp, bc, bq)


def assert_frame_untouched(n, c, bufs, prob_written=True):
    bp, bc, bq = (b.cpu().numpy() for b in bufs)
    assert bp[0] == SENT_I and bp[n + 1] == SENT_I and bc[0] == SENT_F and bc[n + 1] == SENT_F
    frame = np.ones_like(bq, dtype=bool)
    if prob_written:
        frame[1:n + 1, 1:c + 1] = False
    assert (bq[frame] == SENT_F).all()


def test_case_table_equals_the_reference(table):
    for n, c, ld, x, (want_pred, want_conf, want_prob) in table:
        what = f"n={n} C={c} ld={ld}"
        logits = padded(x, ld)
        (vp, vc, vq), bufs = framed(n, c)
        out = ops.predict_head(logits, out_pred=vp, out_conf=vc, out_prob=vq)
        assert len(out) == 3 and out[0] is vp and out[1] is vc and out[2] is vq
        pred, conf, prob = (t.cpu().numpy() for t in out)
        assert_frame_untouched(n, c, bufs)
        assert np.array_equal(pred, want_pred), what
        ref.assert_within_one_ulp(conf, want_conf, what + " conf")
        ref.assert_within_one_ulp(prob, want_prob, what + " prob")

        # without prob: the same bits in pred and conf, prob's buffer untouched; a second run: the same bits again
        (wp, wc, _), bufs2 = framed(n, c)
        out2 = ops.predict_head(logits, out_pred=wp, out_conf=wc)
        assert len(out2) == 2
        assert_frame_untouched(n, c, bufs2, prob_written=False)
        assert torch.equal(wp, vp) and np.array_equal(wc.cpu().numpy().view(np.uint32), conf.view(np.uint32)), what
        again = ops.predict_head(logits, want_prob=True)
        assert again[0].dtype == torch.int64 and again[1].dtype == torch.float32 and tuple(again[2].shape) == (n, c)
        for a, b in zip(again, (pred, conf, prob)):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8)), what


def test_the_special_rows_are_what_the_contract_says(table):
    n, c, ld, x, _ = next(t for t in table if t[0] == 65 and t[1] == 9 and t[2] == 12)
    pred, conf, prob = (t.cpu().numpy() for t in ops.predict_head(padded(x, ld), want_prob=True))
    sp = slice(2, 12)
    assert pred[sp].tolist() == [0, 0, 8, 0, 5, 0, 4, 1, 0, 1]
    assert np.isnan(conf[sp]).tolist() == [False] * 5 + [True] * 3 + [False] * 2
    assert conf[2] == np.float32(1.0 / 9.0) and (prob[2] == conf[2]).all()
    assert prob[6, 4] == 0.0 and abs(float(prob[6].sum()) - 1.0) < 1e-6
    assert conf[10] == np.float32(0.2) and prob[10].tolist() == [np.float32(0.2), 0.0] * 4 + [np.float32(0.2)]


def test_n_rows_of_a_longer_buffer_and_a_grid_stride_size():
    """``n`` below the rows of ``logits`` (the engine's batch buffer): rows past n are neither read into results nor written;
    a size above one round of the grid's blocks (4096 x 256 lanes) takes the grid-stride loop."""
    x = ref.case_logits(257, 9, 5)
    want = ref.predict_head(x[:100])
    pred, conf = ops.predict_head(padded(x, 12), n=100)
    assert tuple(pred.shape) == (100,) and np.array_equal(pred.cpu().numpy(), want[0])
    ref.assert_within_one_ulp(conf.cpu().numpy(), want[1])
    n = 4096 * 256 + 77
    big = torch.from_numpy(np.tile(x, (n // 257 + 1, 1))[:n]).to(DEV)
    pred, conf, prob = ops.predict_head(big, want_prob=True)
    small = ops.predict_head(torch.from_numpy(x).to(DEV), want_prob=True)
    reps = n // 257 + 1
    for got, one in zip((pred, conf, prob), small):
        tiled = one.repeat((reps,) + (1,) * (one.dim() - 1))[:n]
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                           tiled.view(torch.int32) if tiled.dtype == torch.float32 else tiled)


def test_invalid_arguments_return_the_error_code_and_write_nothing():
    lib, P = _lib.load(), _lib.ptr
    n, c = 5, 9
    logits = torch.zeros((n, c), dtype=torch.float32, device=DEV)
    (vp, vc, vq), bufs = framed(n, c)
    ldq = vq.stride(0)
    st = _lib.current_stream()
    bad = [
        (P(logits), c, n, 0, P(vp), P(vc), P(vq), ldq),                 # n_classes outside 1 .. 16
        (P(logits), c, n, 17, P(vp), P(vc), P(vq), 32),
        (P(logits), c, n, -3, P(vp), P(vc), None, 0),
        (P(logits), c - 1, n, c, P(vp), P(vc), P(vq), ldq),             # ld_logits < C
        (P(logits), c, n, c, P(vp), P(vc), P(vq), c - 1),               # prob given, ld_prob < C
        (None, c, n, c, P(vp), P(vc), P(vq), ldq),                      # a NULL array with n_nodes > 0
        (P(logits), c, n, c, None, P(vc), P(vq), ldq),
        (P(logits), c, n, c, P(vp), None, P(vq), ldq),
        (P(logits), c, -1, c, P(vp), P(vc), P(vq), ldq),                # n_nodes < 0
    ]
    for args in bad:
        assert lib.gte_predict_head(*args, st) == INVALID_ARGUMENT, args
        assert b"predict_head" in lib.gte_last_error()
    torch.cuda.synchronize()
    bp, bc, bq = (b.cpu().numpy() for b in bufs)
    assert (bp == SENT_I).all() and (bc == SENT_F).all() and (bq == SENT_F).all()
    # n_nodes == 0: success, no launch, NULL arrays allowed; ld_prob is not looked at without prob
    assert lib.gte_predict_head(None, c, 0, c, None, None, None, 0, st) == 0
    assert lib.gte_predict_head(P(logits), c, n, c, P(vp), P(vc), None, 0, st) == 0
    assert (bufs[2].cpu().numpy() == SENT_F).all() and (bufs[0][1:n + 1] == 0).all()


def test_the_wrapper_checks_its_tensors():
    x = torch.zeros((4, 9), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.GteError, match="no CPU fallback"):
        ops.predict_head(x.cpu())
    with pytest.raises(TypeError, match="2-D float32"):
        ops.predict_head(x.double())
    with pytest.raises(ValueError, match="outside 0 .. 4"):
        ops.predict_head(x, n=5)
    with pytest.raises(ValueError, match="out_pred"):
        ops.predict_head(x, out_pred=torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="out_conf"):
        ops.predict_head(x, out_conf=torch.zeros(8, dtype=torch.float32, device=DEV)[::2])
    with pytest.raises(ValueError, match="out_prob"):
        ops.predict_head(x, out_prob=torch.zeros((4, 8), dtype=torch.float32, device=DEV))
    with pytest.raises(_lib.GteError, match="n_classes"):
        ops.predict_head(torch.zeros((4, 17), dtype=torch.float32, device=DEV))
