"""MeanSAGE on the HIP path end to end: ``model(g)``, the ReLU + L2-normalise kernel pair inside the layer's autograd node, and
training through TrainStep (HIP cross-entropy, HIP Adam) -- against ``oracle.gcnsage_cpu.meansage_forward`` +
``torch.nn.CrossEntropyLoss`` + ``torch.optim.Adam`` in float64 on the CPU.  The graph is the golden case meansage_120 (120 nodes,
F0 = 20, hidden 32, 9 classes, n_layers = 2).  Run with ``-m gpu`` on an MI355X."""
import os

import numpy as np
import pytest
import torch

import gnn_tableextraction_amd as gte
from gnn_tableextraction_amd import graph as G, ops
from gnn_tableextraction_amd.models import model_train
from gnn_tableextraction_amd.models.engine import TrainStep
from oracle import gcnsage_cpu as oc
from tests import poststep
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, WD = 0.01, 5e-4
# Seed of the initial weights and of the labels of the step tests.  Chosen on the CPU (seeds 0, 1, 2, ... tried in order, the first
# that qualifies; seed 0 leaves a pre-activation 3.8e-7 from zero, seed 1 none closer than 1.5e-4): with it no hidden
# pre-activation of the float64 oracle lies within 1e-5 of zero, so no ReLU decision of the device can differ from the oracle's and
# a tie is not what the tolerances absorb.  _case() asserts it.
SEED = 1


def _golden():
    return np.load(os.path.join(GOLDEN_DIR, "meansage_120.npz"))


def _class_weights():
    return np.load(os.path.join(GOLDEN_DIR, "page200_f13_l3_cw.npz"))["class_weights"].astype(np.float32)


def _device_graph(z):
    g = G.PageGraph(z["src"], z["dst"], int(z["meta"][0]), device=DEV)
    g.ndata["feat"] = torch.from_numpy(z["x"]).to(DEV)
    g.edata["feat"] = torch.from_numpy(z["w"]).to(DEV)
    return g


def _linears(state):
    """[(weight, bias)] in layer order from a MeanSAGE state_dict"""
    n = 1 + max(int(k.split(".")[1]) for k in state)
    return [(state[f"layers.{i}.linear.weight"], state[f"layers.{i}.linear.bias"]) for i in range(n)]


def hidden_preactivations(ws, og, x):
    """the oracle's z of every hidden layer: meansage_forward over the first k + 1 layers ends with layer k's linear map"""
    with torch.no_grad():
        return [oc.meansage_forward(ws[:k + 1], og, x) for k in range(len(ws) - 1)]


class Oracle:
    """float64: meansage_forward -> CrossEntropyLoss(weight) -> backward -> torch.optim.Adam(lr, weight_decay)"""

    def __init__(self, state, og, x, class_weights=None):
        self.names = sorted(state, key=lambda k: (int(k.split(".")[1]), k.endswith("bias")))
        self.p = {k: state[k].detach().double().clone().requires_grad_(True) for k in self.names}
        self.og, self.x = og, torch.as_tensor(x).double()
        self.opt = torch.optim.Adam([self.p[k] for k in self.names], lr=LR, weight_decay=WD)
        self.loss_fn = torch.nn.CrossEntropyLoss(weight=None if class_weights is None else torch.as_tensor(class_weights).double())

    def forward(self):
        return oc.meansage_forward(_linears(self.p), self.og, self.x)

    def step(self, labels):
        loss = self.loss_fn(self.forward(), torch.as_tensor(labels).long())
        self.opt.zero_grad()
        loss.backward()
        grads = {k: v.grad.detach().clone().numpy() for k, v in self.p.items()}
        self.opt.step()
        return float(loss.detach()), grads


def _case(seed=SEED):
    """(z, model on the host with the seed's weights, its initial state, oracle graph, labels generator)"""
    z = _golden()
    n, f0, hid, ncls, nl, _ = (int(v) for v in z["meta"])
    torch.manual_seed(seed)
    m = gte.MeanSAGE(f0, hid, ncls, nl)
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    og = oc.OracleGraph(z["src"], z["dst"], n, z["w"])
    pre = hidden_preactivations(_linears({k: v.double() for k, v in state0.items()}), og, torch.from_numpy(z["x"]).double())
    margin = min(float(p.abs().min()) for p in pre)
    assert margin > 1e-5, f"seed {seed}: a hidden pre-activation of the oracle lies {margin:.2e} from zero, choose another seed"
    rng = np.random.default_rng(seed)
    return z, m, state0, og, rng, ncls, n


# ---------------------------------------------------------------- 1. forward and calling convention
@pytest.mark.parametrize("mode", ["split_bf16", "f32"])
def test_forward_from_the_graph_alone_matches_the_golden_logits_without_torch_arithmetic(mode):
    prev = ops.set_gemm_mode(mode)
    try:
        z = _golden()
        n, f0, hid, ncls, nl, _ = (int(v) for v in z["meta"])
        m = gte.MeanSAGE(f0, hid, ncls, nl)
        m.load_state_dict({k[len("state0."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("state0.")})
        m = m.to(DEV)
        g = _device_graph(z)
        with torch.no_grad():
            explicit = m(g, g.ndata["feat"], g.edata["feat"])              # the reference's call; also warms every cache
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
                out = m(g)
            torch.cuda.synchronize()
        assert torch.equal(out, explicit)
        np.testing.assert_allclose(out.cpu().numpy(), z["out"], rtol=1e-5, atol=1e-5)
        seen = {e.name for e in prof.events()}
        assert seen, "the profiler recorded nothing"
        for op in ("aten::relu", "aten::linalg_vector_norm", "aten::div", "aten::clamp_min"):
            assert op not in seen, f"{op} ran in MeanSAGE.forward"
        # no edge weights on the graph: 1.0, as in GcnSAGELayer
        g1 = G.PageGraph(z["src"], z["dst"], n, device=DEV)
        g1.ndata["feat"] = g.ndata["feat"]
        with torch.no_grad():
            unit = m(g1)
            want = m(g, g.ndata["feat"], torch.ones_like(g.edata["feat"]))
        assert torch.equal(unit, want)
    finally:
        ops.set_gemm_mode(prev)


# ---------------------------------------------------------------- 2. one TrainStep step
@pytest.mark.parametrize("weighted", [False, True])
def test_one_train_step_matches_the_float64_oracle(weighted):
    z, m, state0, og, rng, ncls, n = _case()
    labels = rng.integers(0, ncls, n)
    cw = _class_weights() if weighted else None
    oracle = Oracle(state0, og, z["x"], cw)
    want_loss, want_grads = oracle.step(labels)

    m = m.to(DEV)
    g = _device_graph(z)
    step = TrainStep(m, lr=LR, weight_decay=WD, class_weights=None if cw is None else torch.from_numpy(cw).to(DEV))
    out3 = step.step(g, torch.from_numpy(labels).to(DEV)).cpu().numpy()
    print(f"loss {out3[0]:.7f} oracle {want_loss:.7f}")
    assert abs(float(out3[0]) - want_loss) < 1e-5
    for k, p in m.named_parameters():
        ref = want_grads[k]
        got = p.grad.cpu().numpy()
        print(f"grad {k}: max|d| = {np.abs(got - ref).max():.3e} of max {np.abs(ref).max():.3e}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6 + 1e-4 * np.abs(ref).max(), err_msg=k)
    for k, p in m.named_parameters():
        g_eff = want_grads[k] + WD * state0[k].double().numpy()
        tol = poststep.step_tolerance(g_eff, float(np.abs(g_eff).max()), lr=LR)
        diff = np.abs(p.detach().cpu().numpy().astype(np.float64) - oracle.p[k].detach().numpy())
        print(f"post-step {k}: max|d| = {diff.max():.3e}")
        assert (diff <= tol).all(), f"{k}: a parameter differs after the step by more than its gradient's conditioning allows"


# ---------------------------------------------------------------- 3. five consecutive steps
def test_five_steps_follow_the_float64_oracle():
    z, m, state0, og, rng, ncls, n = _case()
    label_sets = [rng.integers(0, ncls, n) for _ in range(5)]
    oracle = Oracle(state0, og, z["x"])
    want = [oracle.step(y)[0] for y in label_sets]
    m = m.to(DEV)
    g = _device_graph(z)
    step = TrainStep(m, lr=LR, weight_decay=WD)
    got = [step.step(g, torch.from_numpy(y).to(DEV)) for y in label_sets]
    got = [float(o[0]) for o in got]
    print("loss per step:", got, "oracle:", want)
    assert step.t == 5 and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)


# ---------------------------------------------------------------- 4. evaluate()
def test_evaluate_returns_the_oracles_loss_accuracy_and_predictions():
    z, m, state0, og, rng, ncls, n = _case()
    labels = rng.integers(0, ncls, n)
    oracle = Oracle(state0, og, z["x"])
    with torch.no_grad():
        logits = oracle.forward()
        want_loss = float(oracle.loss_fn(logits, torch.from_numpy(labels).long()))
    top2 = logits.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-4                  # no arg-max of the oracle is a near tie
    want_pred = logits.argmax(1).numpy()
    loss, acc, pred = model_train.evaluate(m.to(DEV), _device_graph(z), torch.from_numpy(labels).to(DEV))
    assert abs(loss - want_loss) < 1e-5
    assert np.array_equal(pred.cpu().numpy(), want_pred)
    assert acc == float((want_pred == labels).sum()) / n
    assert not m.training


# ---------------------------------------------------------------- 5. isolated nodes and an all-zero page
def test_a_batch_with_isolated_nodes_and_an_all_zero_page_trains_finite():
    tiny = np.load(os.path.join(GOLDEN_DIR, "tiny_6n_10e.npz"))
    f0, hid, ncls = 3, 8, 9
    rng = np.random.default_rng(3)

    def page(src, dst, n, feat):
        g = G.PageGraph(src, dst, n, device=DEV)
        g.ndata["feat"] = torch.from_numpy(feat.astype(np.float32)).to(DEV)
        g.edata["feat"] = torch.from_numpy(rng.random(len(src)).astype(np.float32)).to(DEV)
        return g
    none = np.zeros(0, dtype=np.int64)
    pages = [page(none, none, 1, rng.standard_normal((1, f0))),            # a single node without edges
             page(tiny["src"], tiny["dst"], 6, np.zeros((6, f0))),           # a page whose features are all zero
             page(tiny["src"], tiny["dst"], 6, rng.standard_normal((6, f0))),
             page(none, none, 1, rng.standard_normal((1, f0)))]
    g = G.batch(pages)
    n = g.num_nodes()
    assert n == 14
    torch.manual_seed(1)
    m = gte.MeanSAGE(f0, hid, ncls, 2).to(DEV)
    with torch.no_grad():
        for layer in m.layers:
            layer.linear.bias.zero_()                                       # zero-norm hidden rows need a zero bias
    hidden = []
    hooks = [layer.register_forward_hook(lambda mod, i, o: hidden.append(o.detach().clone())) for layer in m.layers[:-1]]
    step = TrainStep(m, lr=LR, weight_decay=WD)
    out3 = step.step(g, torch.from_numpy(rng.integers(0, ncls, n)).to(DEV)).cpu().numpy()
    for h in hooks:
        h.remove()
    assert len(hidden) == 2
    for h in hidden:
        assert bool((h[1:7] == 0).all()), "the all-zero page must give zero hidden rows"
        assert bool(torch.isfinite(h).all())
    assert np.isfinite(out3).all()
    for k, p in m.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), f"{k}: gradient not finite"
        assert bool(torch.isfinite(p).all()), f"{k}: parameter not finite after the step"
    assert any(float(p.grad.abs().max()) > 0 for p in m.parameters())
