"""Dropout keep bits (csrc/dropout.h) on the host: gte_dropout_mask_host against a Philox4x32-10 written here in numpy, the
Random123 known answer, keep rates and independence between masks that differ in one coordinate -- and the engine's plan choice
for a dropout model (host logic only).  No GPU needed."""
import numpy as np
import pytest
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import ops
from tests.dropout_ref import keep as numpy_mask, philox4x32_10


def host_mask(p, seed, rank, step, site, n_rows, n_cols):
    return ops.dropout_mask(p, seed, rank, step, site, n_rows, n_cols).numpy()


def test_philox_known_answer():
    got = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # the library's Philox through its mask: with p = 2^-32 the threshold is 1 -- a word is dropped iff it is 0; instead compare
    # the bits at a threshold that splits the known words: 0x9B00DBD8 < 0xA0000000 <= 0xBC57AC4C
    p = float(np.float32(0xA0000000 / 2 ** 32))
    thr = int(p * 2 ** 32 + 0.5)
    assert 0x9B00DBD8 < thr <= 0xBC57AC4C
    m = host_mask(p, 0, 0, 0, 0, 1, 4)
    assert m.tolist() == [[0, 1, 1, 0]]          # 6627e8d5 < thr, e169c58d >= thr, bc57ac4c >= thr, 9b00dbd8 < thr


@pytest.mark.parametrize("p,seed,rank,step,site,n,c", [
    (0.1, 42, 0, 0, 0, 37, 13), (0.5, 42, 0, 3, 1, 65, 1662), (0.9, (1 << 40) + 7, 3, 12345, 2, 17, 437),
    (0.2, 2 ** 64 - 1, 7, 2 ** 31, 5, 5, 1), (0.37, 0, 1, 1, 3, 129, 2002)])
def test_host_mask_equals_numpy_philox(p, seed, rank, step, site, n, c):
    np.testing.assert_array_equal(host_mask(p, seed, rank, step, site, n, c), numpy_mask(p, seed, rank, step, site, n, c))


def _bounds(k, n, q, sigmas=6.0):
    sd = np.sqrt(n * q * (1 - q))
    return abs(k - n * q) <= sigmas * sd + 1


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate_within_binomial_bounds(p):
    m = host_mask(p, 2024, 0, 5, 1, 400, 1003)
    assert _bounds(int(m.sum()), m.size, 1 - p), (m.mean(), 1 - p)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("which", ["seed", "rank", "step", "site", "row", "col"])
def test_masks_differing_in_one_coordinate_are_independent(p, which):
    """Two masks that differ only in one argument agree at the rate of independent draws, p^2 + (1 - p)^2."""
    base = dict(seed=77, rank=0, step=9, site=1)
    a = host_mask(p, base["seed"], base["rank"], base["step"], base["site"], 600, 516)
    if which in ("row", "col"):
        # shifted by one row / by one column (a column shift also moves across the four words of a Philox call)
        big = host_mask(p, base["seed"], base["rank"], base["step"], base["site"], 601, 517)
        b = big[1:, :516] if which == "row" else big[:600, 1:]
    else:
        kw = dict(base)
        kw[which] += 1
        b = host_mask(p, kw["seed"], kw["rank"], kw["step"], kw["site"], 600, 516)
    agree = int((a == b).sum())
    q = p * p + (1 - p) * (1 - p)
    assert _bounds(agree, a.size, q), (which, agree / a.size, q)


def test_mask_rejects_p_outside_the_open_interval():
    for p in (0.0, 1.0, -0.1):
        with pytest.raises(gte._lib.GteError):
            host_mask(p, 1, 0, 0, 0, 4, 4)


def test_engine_runs_every_hidden_layer_as_a_dropout_layer():
    """A dropout model takes the one-call plan with GTE_LAYER_DROPOUT (4) at every hidden layer, reads the resident feature image
    (no cached aggregate: layer 0 aggregates the dropped input), and evaluates on the plan of a dropout-free model; p = 1 is
    refused."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    for f0, hid, nl in [(831, 256, 3), (13, 218, 3), (831, 1000, 3), (63, 206, 4)]:
        torch.manual_seed(0)
        eng = FusedGcnSageStep(gte.GcnSAGE(f0, hid, 9, nl, torch.nn.functional.relu, 0.1), dropout_seed=5)
        kinds = eng._plan_kinds(f0, 20000)
        assert kinds == [4] * (nl - 1), (f0, hid, kinds)
        assert eng.wants_resident_images(f0) and not eng.wants_agg_image(f0)
        assert eng.dropout_p == pytest.approx(0.1) and eng.dropout_seed == 5
        torch.manual_seed(0)
        ref = FusedGcnSageStep(gte.GcnSAGE(f0, hid, 9, nl, torch.nn.functional.relu, 0))
        assert eng._plan_kinds(f0, 20000, train=False) == ref._plan_kinds(f0, 20000)
    with pytest.raises(ValueError):
        FusedGcnSageStep(gte.GcnSAGE(13, 64, 9, 3, torch.nn.functional.relu, 1.0))
    # the call-by-call schedule refuses dropout loudly instead of training without masks
    eng = FusedGcnSageStep(gte.GcnSAGE(13, 64, 9, 3, torch.nn.functional.relu, 0.2))
    eng.use_c_step = False
    assert eng._plan_kinds(13, 1000) is None
    with pytest.raises(RuntimeError, match="one-call plan only"):
        eng._refuse_dropout()


def test_train_keeps_the_autograd_path_for_dropout_models_the_plan_does_not_cover(monkeypatch):
    """train()'s engine choice (model_train.train_engine): the fused step for a covered dropout model, TrainStep -- as before dropout
    ran on the fused step -- for one the one-call plan does not run (hidden width > 1024, GTE_C_STEP=0), and for p = 1."""
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep, TrainStep
    from gnn_tableextraction_amd.models.model_train import train_engine
    quiet = lambda *a, **k: None
    mk = lambda hid, p: gte.GcnSAGE(13, hid, 9, 3, torch.nn.functional.relu, p)
    assert type(train_engine(mk(218, 0.2), 0.2, 42, say=quiet)) is FusedGcnSageStep
    assert type(train_engine(mk(2048, 0.2), 0.2, 42, say=quiet)) is TrainStep
    assert type(train_engine(mk(2048, 0), 0.0, 42, say=quiet)) is FusedGcnSageStep       # (p = 0: unchanged)
    assert type(train_engine(mk(64, 1.0), 1.0, 42, say=quiet)) is TrainStep
    with pytest.raises(ValueError, match="one-call plan"):
        FusedGcnSageStep(mk(2048, 0.2))
    monkeypatch.setenv("GTE_C_STEP", "0")
    with pytest.raises(ValueError, match="one-call plan"):
        FusedGcnSageStep(mk(218, 0.2))
    assert type(train_engine(mk(218, 0.2), 0.2, 42, say=quiet)) is TrainStep
