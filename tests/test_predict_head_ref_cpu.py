"""tests/predict_head_ref.py against torch on the CPU, on the case table that the GPU test uses: the arg-max rule is
torch.argmax's, and the float64 softmax differs from torch.softmax only in the summation order of at most 16 terms."""
import numpy as np
import pytest
import torch

from tests import predict_head_ref as ref


def test_the_rules_the_contract_quotes():
    assert int(torch.argmax(torch.tensor([[1.0, float("nan"), 3.0, float("nan")]]), 1)) == 1
    assert int(torch.argmax(torch.full((1, 5), float("-inf")), 1)) == 0
    pred, conf, prob = ref.predict_head(np.asarray([[1.0, np.nan, 3.0, np.nan], [-np.inf] * 4, [0.0, np.inf, 0.0, 1.0],
                                                    [2.0, -np.inf, 2.0, 0.0]], dtype=np.float32))
    assert pred.tolist() == [1, 0, 1, 0]
    assert np.isnan(conf[:3]).all() and np.isnan(prob[:3]).all()
    assert prob[3, 1] == 0.0 and prob[3, 0] == prob[3, 2] == conf[3] and abs(prob[3].sum() - 1.0) < 1e-15


def test_the_table_holds_every_special_row():
    sp = ref.special_rows(9)
    assert len(sp) == 10 and np.isnan(sp).any(1).sum() == 1 and np.isposinf(sp).any(1).sum() == 1
    assert np.isneginf(sp).all(1).sum() == 1 and np.isneginf(sp).any(1).sum() == 2 and (np.abs(sp) == np.float32(3.0e38)).all(1).sum() == 2
    table = list(ref.cases())
    assert len(table) == len(ref.NS) * len(ref.SHAPES)
    for n, c, ld, x in table:
        assert x.shape == (n, c) and x.dtype == np.float32 and ld >= c
        if n >= 63:
            assert np.array_equal(x[2:12], ref.special_rows(c), equal_nan=True)


@pytest.mark.parametrize("n", ref.NS)
def test_reference_equals_torch_on_the_case_table(n):
    for n_, c, ld, x in ref.cases():
        if n_ != n:
            continue
        pred, conf, prob = ref.predict_head(x)
        t = torch.from_numpy(x)
        assert np.array_equal(pred, torch.argmax(t, 1).numpy()), (n, c)
        want = torch.softmax(t.double(), 1).numpy()
        assert np.array_equal(np.isnan(prob), np.isnan(want)), (n, c)
        ok = ~np.isnan(want)
        assert (np.abs(prob[ok] - want[ok]) <= 1e-14 * np.abs(want[ok])).all(), (n, c)
        if n:
            want_conf = want[np.arange(n), pred]
            assert np.array_equal(np.isnan(conf), np.isnan(want_conf)), (n, c)
            ok = ~np.isnan(want_conf)
            assert (np.abs(conf[ok] - want_conf[ok]) <= 1e-14 * np.abs(want_conf[ok])).all(), (n, c)
            assert np.array_equal(conf, prob[np.arange(n), pred], equal_nan=True)
