"""The float64 oracle of the loss and optimiser kernels (tests/lossoptim_ref.py) is right: against torch in float64 and against
the documented special cases worked out by hand.  No GPU."""
import numpy as np
import pytest
import torch

from tests import lossoptim_ref as ref


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,c", [(1, 9), (37, 2), (300, 9), (129, 16)])
def test_ce_matches_torch_cross_entropy_in_float64(n, c, weighted):
    rng = np.random.default_rng(100 * n + c)
    logits = (3 * rng.standard_normal((n, c))).astype(np.float32)
    y = rng.integers(0, c, n)
    if n > 1:
        y[rng.random(n) < 0.2] = -100                                   # torch's ignore_index
        y[0] = 0                                                        # (at least one node counts)
    cw = (0.5 + rng.random(c)).astype(np.float32) if weighted else None
    lt = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    crit = torch.nn.CrossEntropyLoss(weight=None if cw is None else torch.from_numpy(cw.astype(np.float64)), ignore_index=-100)
    want = crit(lt, torch.from_numpy(y))
    want.backward()
    for gs in (1.0, 0.25):
        loss, sum_w, n_correct, dl = ref.ce(logits, y, cw, gs)
        assert abs(loss - want.item()) <= 1e-12 * abs(want.item())
        assert _rel(dl, gs * lt.grad.numpy()) <= 1e-12
        assert bool((dl[y < 0] == 0).all())
    w_each = np.ones(n) if cw is None else cw.astype(np.float64)[np.maximum(y, 0)]
    assert abs(sum_w - w_each[y >= 0].sum()) <= 1e-12 * sum_w
    assert n_correct == int(((logits.argmax(1) == y) & (y >= 0)).sum())
    # float32 labels holding integers are the same labels
    assert ref.ce(logits, y.astype(np.float32), cw, 1.0)[0] == ref.ce(logits, y, cw, 1.0)[0]


def test_adam_matches_torch_adam_in_float64():
    rng = np.random.default_rng(3)
    n, lr, b1, b2, eps, wd = 1000, 0.01, 0.5, 0.75, 1e-8, 5e-4          # betas exactly representable in float32
    # (lr, eps and wd enter the oracle float32-rounded: torch gets the same values)
    lr_, eps_, wd_ = (float(np.float32(x)) for x in (lr, eps, wd))
    p = rng.standard_normal(n)
    pt = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr_, betas=(b1, b2), eps=eps_, weight_decay=wd_)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = ref.adam(p, g, m, v, t, lr, b1, b2, eps, wd, 1.0)
        assert _rel(p, pt.detach().numpy()) <= 1e-12
        st = opt.state[pt]
        assert _rel(m, st["exp_avg"].numpy()) <= 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) <= 1e-12
    # grad_scale multiplies the gradient and nothing else
    a = ref.adam(p, g, m, v, 6, lr, b1, b2, eps, wd, 0.125)
    b = ref.adam(p, 0.125 * g, m, v, 6, lr, b1, b2, eps, wd, 1.0)
    assert all(_rel(x, y) <= 1e-15 for x, y in zip(a, b))


def test_hyper_parameters_enter_float32_rounded():
    bc1, bc2s = ref.bias_corrections(0.9, 0.999, 1)
    assert bc1 == 1.0 - float(np.float32(0.9)) and bc2s == np.sqrt(1.0 - float(np.float32(0.999)))
    assert abs(bc2s ** 2 / (1.0 - 0.999) - 1.0) > 1e-5                   # not the double 0.999: the ABI carries floats
    bc1, bc2s = ref.bias_corrections(0.5, 0.75, 3)
    assert bc1 == 0.875 and bc2s == np.sqrt(1.0 - 0.421875)


def test_all_labels_ignored_gives_zeros():
    logits = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [5.0, -5.0, 0.5]], dtype=np.float32)
    for labels in (np.array([-1, 3, -100]), np.array([-1.0, 3.0, 10.0], dtype=np.float32)):
        loss, sum_w, n_correct, dl = ref.ce(logits, labels, None, 1.0)
        assert (loss, sum_w, n_correct) == (0.0, 0.0, 0) and dl.shape == (3, 3) and bool((dl == 0).all())


def test_a_tie_counts_the_first_maximum():
    logits = np.array([[2.0, 2.0, 1.0], [0.0, 3.0, 3.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    assert ref.ce(logits, np.array([0, 1, 0]), None, 1.0)[2] == 3
    assert ref.ce(logits, np.array([1, 2, 2]), None, 1.0)[2] == 0
    # by hand: row 0 has lse = 2 + log(2 + 1/e), nll for label 0 = log(2 + 1/e)
    loss = ref.ce(logits[:1], np.array([0]), None, 1.0)[0]
    assert abs(loss - np.log(2.0 + np.exp(-1.0))) <= 1e-15


def test_a_zero_weight_class_drops_out_of_the_sum_of_weights():
    logits = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    cw = np.array([0.0, 2.0, 0.5], dtype=np.float32)
    loss, sum_w, n_correct, dl = ref.ce(logits, np.array([0, 1, 2]), cw, 1.0)
    assert sum_w == 2.5 and abs(loss - np.log(3.0)) <= 1e-15               # every nll is log 3
    assert n_correct == 1                                                  # the tie goes to class 0: node 0 counts, weight 0 or not
    assert bool((dl[0] == 0).all())
    np.testing.assert_allclose(dl[1], 2.0 / 2.5 * (np.full(3, 1 / 3) - np.array([0.0, 1.0, 0.0])), rtol=1e-15)
    # a batch whose only present class has weight 0: sum_w == 0, zeros and no NaN
    loss, sum_w, n_correct, dl = ref.ce(logits, np.array([0, 0, 0]), cw, 1.0)
    assert (loss, sum_w) == (0.0, 0.0) and n_correct == 3 and bool((dl == 0).all())


def test_head_is_the_ce_of_the_aggregate_and_its_transposed_gradient():
    """3 nodes, edges 0->1 (w 2), 2->1 (w 4), 1->0 (w 1): mean over in-edges, q through the out-edges with w / in-degree(dst)."""
    indptr, indices, ew = np.array([0, 1, 3, 3]), np.array([1, 0, 2]), np.array([1.0, 2.0, 4.0], dtype=np.float32)
    ts = np.array([[1.0, 0.0], [0.0, 0.0], [0.5, 0.5]], dtype=np.float32)
    tn = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=np.float32)
    rindptr, rindices = np.array([0, 1, 2, 3]), np.array([1, 0, 1])     # out-edges of 0: ->1; of 1: ->0; of 2: ->1
    w_out = np.array([2.0 / 2, 1.0 / 1, 4.0 / 2], dtype=np.float32)
    labels = np.array([0, 1, 5])
    h = ref.head(indptr, indices, ew, ts, tn, labels, None, 0.5, rindptr, rindices, w_out)
    want_logits = np.array([[1.0 + 3.0, 0.0 + 4.0], [(2 * 1 + 4 * 5) / 2, (2 * 2 + 4 * 6) / 2], [0.5, 0.5]])
    np.testing.assert_allclose(h["logits"], want_logits, rtol=1e-15)
    loss, sum_w, n_correct, dl = ref.ce(want_logits.astype(np.float32), labels, None, 0.5)
    assert h["loss"] == loss and h["sum_w"] == sum_w == 2.0 and h["n_correct"] == n_correct and h["alpha"] == 0.25
    np.testing.assert_allclose(h["dl"], dl, rtol=1e-15)
    np.testing.assert_allclose(h["q"], np.stack([1.0 * dl[1], 1.0 * dl[0], 2.0 * dl[1]]), rtol=1e-15)
    np.testing.assert_allclose(h["gbias"], ref.colsum(dl), rtol=1e-15)
    none = ref.head(indptr, indices, ew, ts, tn, np.array([-1, 2, 5]), None, 0.5, rindptr, rindices, w_out)
    assert none["alpha"] == 0.0 and not none["dl"].any() and not none["q"].any() and not none["gbias"].any()
