"""The label-free route end to end: PrebuiltPages.from_boxes(unlabeled=True) against the labels route on the same words,
model_predict.predict() against test(), and the confidences against tests/predict_head_ref.py on the engine's own logits."""
import os
import pickle

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import graph as G
from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
from gnn_tableextraction_amd.models import model_predict
from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
from gnn_tableextraction_amd.models.loop import BatchPipeline
from tests import blocks_ref, predict_head_ref as ref
from tests.predict_setup import config_and_weights
from tests.test_gpu_from_annotations import SIZE, make_page

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("knn", "visibility")
SEED = 5            # of the untrained weights: these words then fall into four classes of 40 to 270 words (seed 3: one class)


@pytest.fixture(scope="module")
def words():
    rng = np.random.default_rng(91)
    made = [make_page(rng, with_figure=False), make_page(rng), make_page(rng, with_figure=False)]
    boxes, texts = [m[0] for m in made], [m[1] for m in made]
    labels = [rng.integers(0, 9, len(b)) for b in boxes]
    return boxes, texts, labels


@pytest.fixture(scope="module")
def sets(words):
    """mode -> (labelled set, unlabelled set) on the same boxes and texts, both with the same layout blocks on their pages"""
    boxes, texts, labels = words
    out = {}
    for mode in MODES:
        lab = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, labels, DEV, mode=mode, range_island=0)
        unl = PrebuiltPages.from_boxes(boxes, [SIZE] * 3, texts, None, DEV, mode=mode, range_island=0, unlabeled=True)
        rng = np.random.default_rng(5)
        for pl, pu in zip(lab.pages, unl.pages):
            pl["blocks"] = blocks_ref.synthetic_blocks(pl["bboxs"], rng)
            pu["blocks"] = [list(b) for b in pl["blocks"]]
        out[mode] = (lab, unl)
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_unlabeled_pages_are_the_labelled_pages_without_labels(sets, words, mode):
    lab, unl = sets[mode]
    assert lab.labeled is True and unl.labeled is False
    assert unl.num_classes == 9 and unl.stats == {"numbers": [0] * 9, "percentages": [0.0] * 9} and sum(lab.stats["numbers"]) > 300
    assert len(unl) == len(lab) == 3 and unl.whole.batch_num_nodes_ == [len(b) for b in words[0]]      # every word kept
    for a, b in zip(unl.whole.edges(), lab.whole.edges()):
        assert torch.equal(a, b)
    assert unl.whole.num_edges() > 3 * unl.whole.num_nodes() / 2
    assert torch.equal(unl.whole.edata["feat"], lab.whole.edata["feat"])
    assert torch.equal(unl.whole.ndata["feat"], lab.whole.ndata["feat"]) and tuple(unl.whole.ndata["feat"].shape)[1] == 13
    assert torch.equal(unl.whole.ndata["bbox"], lab.whole.ndata["bbox"])
    assert "label" not in unl.whole.ndata and "label" in lab.whole.ndata
    for g, w, pg, pw, arr in zip(unl.graphs, lab.graphs, unl.pages, lab.pages, unl.page_arrays):
        assert "label" not in g.ndata and arr.label is None
        for a, b in zip(g.edges(), w.edges()):
            assert torch.equal(a, b)
        assert torch.equal(g.edata["feat"], w.edata["feat"]) and torch.equal(g.ndata["feat"], w.ndata["feat"])
        np.testing.assert_array_equal(pg["bboxs"], pw["bboxs"])
        assert pg["texts"] == pw["texts"] and pg["page"] == pw["page"]
    train, val, _ = unl.split()
    assert len(train) + len(val) == 3
    extra = [np.full((len(b), 2), 0.5, dtype=np.float32) for b in words[0]]
    wide = PrebuiltPages.from_boxes(words[0], [SIZE] * 3, words[1], None, DEV, mode=mode, extra_feats=extra, unlabeled=True,
                                    num_classes=4)
    assert wide.num_classes == 4 and tuple(wide.whole.ndata["feat"].shape)[1] == 15
    assert torch.equal(wide.whole.ndata["feat"][:, :13], lab.whole.ndata["feat"]) and bool((wide.whole.ndata["feat"][:, 13:] == 0.5).all())


@pytest.mark.parametrize("mode", MODES)
def test_predict_equals_test_without_reading_a_label(sets, mode, tmp_path, capsys):
    lab, unl = sets[mode]
    cfg, _, logs = config_and_weights(tmp_path, batch_size=2, seed=SEED)
    want = model_predict.test(lab, cfg, regions=True, region_scores=True, blocks=True, block_scores=True)
    files = {sub: open(tmp_path / sub / f"{logs}.json", "rb").read() for sub in ("regions", "blocks")}
    flat_file = open(tmp_path / "all_pred" / logs, "rb").read()
    capsys.readouterr()
    got = model_predict.predict(unl, cfg, probabilities=True, regions=True, region_scores=True, blocks=True, block_scores=True)
    assert "Accuracy" not in capsys.readouterr().out
    assert set(got) == {"all_pred", "all_pred_flat", "confidence", "probabilities", "regions", "blocks"}
    assert len(got["all_pred"]) == 3 and all(np.array_equal(a, b) for a, b in zip(got["all_pred"], want["all_pred"]))
    assert got["all_pred_flat"] == want["all_pred_flat"] and len(set(got["all_pred_flat"])) >= 4
    assert got["regions"] == want["regions"] and sum(len(r) for r in got["regions"]) > 0 and all(len(r) == 4 for page in got["regions"] for r in page)
    assert got["blocks"] == want["blocks"] and all("scores" in r for r in got["blocks"])
    for sub in ("regions", "blocks"):
        assert open(tmp_path / sub / f"{logs}.json", "rb").read() == files[sub], sub
    assert open(tmp_path / "all_pred" / logs, "rb").read() == flat_file
    saved = pickle.load(open(tmp_path / "predictions" / f"{logs}.pkl", "rb"))
    assert set(saved) == {"all_pred", "num_nodes", "confidence"} and saved["num_nodes"] == [len(a) for a in got["all_pred"]]
    assert saved["all_pred"] == [a.tolist() for a in got["all_pred"]]
    assert all(np.array_equal(np.asarray(s, dtype=np.float32), c) for s, c in zip(saved["confidence"], got["confidence"]))
    for p, c, q in zip(got["all_pred"], got["confidence"], got["probabilities"]):
        assert c.dtype == np.float32 and q.dtype == np.float32 and q.shape == (len(p), 9) and c.shape == (len(p),)
        assert same_bits(c, q[np.arange(len(p)), p]) and (c >= np.float32(1 / 9)).all() and (c <= 1).all()

    # the options off: the plain keys, nothing written
    plain = model_predict.predict(unl, cfg, save_predictions=False)
    assert set(plain) == {"all_pred", "all_pred_flat", "confidence"}
    assert all(same_bits(a, b) for a, b in zip(plain["confidence"], got["confidence"]))
    only = model_predict.predict(unl, cfg, save_predictions=False, regions=True, blocks=True)
    assert set(only) == set(plain) | {"regions", "blocks"}
    assert [[r[:3] for r in page] for page in only["regions"]] == [[r[:3] for r in page] for page in got["regions"]]

    # on the labelled set: the same bits, the labels ignored
    again = model_predict.predict(lab, cfg, save_predictions=False, probabilities=True)
    for key in ("all_pred", "confidence", "probabilities"):
        assert all(same_bits(a, b) for a, b in zip(again[key], got[key])), key
    with pytest.raises(ValueError, match=r"predict\(\)"):
        model_predict.test(unl, cfg)


def test_confidences_equal_the_reference_on_the_engines_logits(sets, tmp_path):
    _, unl = sets["knn"]
    cfg, model, _ = config_and_weights(tmp_path, batch_size=2, seed=SEED)
    engine = FusedGcnSageStep(model.to(DEV).eval())
    pipe = BatchPipeline(G.ResidentPages(unl.graphs, DEV))
    # head=False: what the function returned before -- the per-batch arg-max, and (pred, logits)
    old = model_predict.predict_resident(engine, pipe, 2)
    assert isinstance(old, torch.Tensor) and old.dtype == torch.int64
    old2 = model_predict.predict_resident(engine, pipe, 2, return_logits=True)
    assert isinstance(old2, tuple) and len(old2) == 2 and torch.equal(old2[0], old)
    logits = old2[1]
    assert tuple(logits.shape) == (unl.whole.num_nodes(), 9) and torch.equal(torch.argmax(logits, 1), old)
    with pytest.raises(ValueError, match="head=True"):
        model_predict.predict_resident(engine, pipe, 2, return_prob=True)

    pred, conf = model_predict.predict_resident(engine, pipe, 2, head=True)
    full = model_predict.predict_resident(engine, pipe, 2, head=True, return_prob=True, return_logits=True)
    assert len(full) == 4 and torch.equal(full[3], logits) and torch.equal(full[0], pred) and torch.equal(pred, old)
    assert same_bits(full[1].cpu().numpy(), conf.cpu().numpy())
    assert len(model_predict.predict_resident(engine, pipe, 2, head=True, return_logits=True)) == 3
    want_pred, want_conf, want_prob = ref.predict_head(logits.cpu().numpy())
    assert np.array_equal(pred.cpu().numpy(), want_pred)
    ref.assert_within_one_ulp(conf.cpu().numpy(), want_conf, "conf")
    ref.assert_within_one_ulp(full[2].cpu().numpy(), want_prob, "prob")
    sub = model_predict.predict_resident(engine, pipe, 2, page_ids=[2, 0], head=True)
    n = [g.num_nodes() for g in unl.graphs]
    assert same_bits(sub[1].cpu().numpy(), np.concatenate([conf.cpu().numpy()[n[0] + n[1]:], conf.cpu().numpy()[:n[0]]]))

    out = model_predict.predict(unl, cfg, save_predictions=False, probabilities=True)
    assert same_bits(np.concatenate(out["confidence"]), conf.cpu().numpy())
    assert same_bits(np.concatenate(out["probabilities"]), full[2].cpu().numpy())
    assert not os.path.exists(tmp_path / "all_pred")


def test_save_and_load_round_trip(sets, tmp_path):
    _, unl = sets["visibility"]
    cfg, _, _ = config_and_weights(tmp_path, batch_size=4, seed=SEED)
    unl.save(str(tmp_path / "pages.npz"))
    assert "label" not in np.load(tmp_path / "pages.npz").files
    back = PrebuiltPages.load(str(tmp_path / "pages.npz"))
    assert back.labeled is False and back.num_classes == 9 and back.stats == unl.stats and len(back) == 3
    for g, w in zip(back.graphs, unl.graphs):
        assert "label" not in g.ndata and torch.equal(g.ndata["feat"], w.ndata["feat"]) and torch.equal(g.edata["feat"], w.edata["feat"])
        for a, b in zip(g.edges(), w.edges()):
            assert torch.equal(a, b)
    want = model_predict.predict(unl, cfg, save_predictions=False)
    got = model_predict.predict(back, cfg, save_predictions=False)
    for key in ("all_pred", "confidence"):
        assert all(same_bits(a, b) for a, b in zip(got[key], want[key])), key


def test_the_module_loop_takes_the_head_too(sets, tmp_path, monkeypatch):
    """A dropout model that the engine refuses keeps the module loop: there the head runs once per batch on the module's logits."""
    from gnn_tableextraction_amd.models import engine as engine_mod
    _, unl = sets["knn"]
    cfg, model, _ = config_and_weights(tmp_path, batch_size=2, seed=SEED)
    cfg.TRAINING.dropout = 0.5

    def refuse(*a, **k):
        raise ValueError("outside the one-call plan")
    monkeypatch.setattr(engine_mod, "FusedGcnSageStep", refuse)
    monkeypatch.setattr(model_predict, "predict_resident", None)                          # (not taken: calling it would fail)
    out = model_predict.predict(unl, cfg, save_predictions=False, probabilities=True, regions=True, region_scores=True)
    model = model.to(DEV).eval()
    with torch.no_grad():
        logits = torch.cat([model(G.batch([g.to(DEV) for g in unl.graphs[b0:b0 + 2]])).float() for b0 in (0, 2)])
    want_pred, want_conf, want_prob = ref.predict_head(logits.cpu().numpy())
    assert np.array_equal(np.concatenate(out["all_pred"]), want_pred) and len(set(want_pred.tolist())) >= 4
    ref.assert_within_one_ulp(np.concatenate(out["confidence"]), want_conf, "conf")
    ref.assert_within_one_ulp(np.concatenate(out["probabilities"]), want_prob, "prob")
    assert [len(c) for c in out["confidence"]] == [g.num_nodes() for g in unl.graphs]
    assert all(len(r) == 4 for page in out["regions"] for r in page) and sum(len(page) for page in out["regions"]) > 0
