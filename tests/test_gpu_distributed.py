"""Two data-parallel ranks of the REAL step engine (FusedGcnSageStep, HIP kernels) on one GPU over gloo -- the box has a
single MI355X, RCCL refuses two ranks on one device, gloo all-reduces GPU tensors through the host.  Everything except
the transport is the shipped multi-GPU path: per-rank loss scaling n_local / n_global, one all-reduce of the flat
gradient (or two around layer 0's backward, GTE_DP_OVERLAP=1), HIP-graph replay followed by the eager all-reduce + Adam.  Replicas must stay bit-identical and match the
single-process step on the union batch (reference semantics: mean CE over all nodes of the step)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

F0, HID, NPAGES, BATCH, STEPS = 63, 96, 16, 4, 2
SHAPES = {"narrow": (63, 96), "planes": (160, 128)}      # "planes": both hidden layers multiply P3 images (the default path of cfg2)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _graph(gte, G, S, pages, ids, dev):
    src, dst, w, feat, label, off = S.concat_pages([pages[i] for i in ids])
    g = G.PageGraph(src, dst, int(off[-1]), device=dev)
    g.ndata["feat"] = torch.from_numpy(feat).to(dev)
    g.edata["feat"] = torch.from_numpy(w).to(dev)
    return g, torch.from_numpy(label).to(dev)


def _worker(rank, world, port, out_dir, overlap, shape="narrow"):
    F0, HID = SHAPES[shape]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      GTE_DP_OVERLAP=overlap)
    import torch.distributed as dist
    import gnn_tableextraction_amd as gte
    from gnn_tableextraction_amd import distributed as D, graph as G
    from gnn_tableextraction_amd.data import synthetic as S
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = "cuda:0"
    pages = S.make_pages(NPAGES, in_feats=F0)
    sizes = [p.num_nodes for p in pages]
    plan = D.plan_epoch(sizes, BATCH, world, seed=42, epoch=0)
    counts = D.step_node_counts(plan, sizes)
    torch.manual_seed(100 + rank)                                # different per rank: the engine's broadcast must fix it
    model = gte.GcnSAGE(F0, HID, 9, 3, torch.nn.functional.relu, 0).to(dev)
    tr = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4, distributed=True)
    losses = []
    for s in range(STEPS):
        g, y = _graph(gte, G, S, pages, plan[s][rank], dev)
        n_global = int(counts[s].sum())
        if s == 0:
            out3 = tr.step(g, y, n_global=n_global)               # eager path
        else:
            replay = tr.capture(g, y, n_global=n_global)          # HIP graph + eager all-reduce + Adam
            out3 = replay()
        losses.append(float(out3[0]))
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, f"param_{rank}.npy"), tr.flat_param.detach().cpu().numpy())
    np.save(os.path.join(out_dir, f"loss_{rank}.npy"), np.array(losses))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("shape", ["narrow", "planes"])
@pytest.mark.parametrize("overlap", ["0", "1"])       # one all-reduce behind one graph (default) / two around layer 0's backward
def test_two_ranks_on_one_gpu_equal_the_single_process_step(tmp_path, overlap, shape):
    F0, HID = SHAPES[shape]
    import gnn_tableextraction_amd as gte
    from gnn_tableextraction_amd import distributed as D, graph as G
    from gnn_tableextraction_amd.data import synthetic as S
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path), overlap, shape), nprocs=world, join=True,
                       start_method="spawn")
    p0, p1 = np.load(tmp_path / "param_0.npy"), np.load(tmp_path / "param_1.npy")
    np.testing.assert_array_equal(p0, p1)                        # replicas stay bit-identical

    dev = "cuda:0"
    pages = S.make_pages(NPAGES, in_feats=F0)
    sizes = [p.num_nodes for p in pages]
    plan = D.plan_epoch(sizes, BATCH, world, seed=42, epoch=0)
    torch.manual_seed(100)                                       # rank 0's weights win the broadcast
    model = gte.GcnSAGE(F0, HID, 9, 3, torch.nn.functional.relu, 0).to(dev)
    tr = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4)
    for s in range(STEPS):
        g, y = _graph(gte, G, S, pages, np.concatenate(plan[s]), dev)
        tr.step(g, y)
    want = tr.flat_param.detach().cpu().numpy()
    # different summation order (two partial gradients added by the all-reduce) + Adam's conditioning near g ~ eps:
    # almost every parameter to 1e-5, none further than a fraction of lr
    bad = ~np.isclose(p0, want, rtol=1e-4, atol=2e-5)
    assert bad.mean() < 1e-3 and np.abs(p0 - want).max() < 5e-3
    l0 = np.load(tmp_path / "loss_0.npy")
    assert len(l0) == STEPS and np.isfinite(l0).all()


def test_bench_self_spawned_two_ranks_share_the_gpu():
    """`python bench.py --gpus 2` starts its own two ranks (here: both on the one GPU over gloo, GTE_BENCH_SHARE_GPU=1 -- the
    N > 1 code path of bench.py, not a measurement) and prints ONE line with n_gpus = 2.  The long run is on: its step count is
    derived from the rank's own pages and must be agreed between the ranks (an all-reduce per step: a rank that plans one step
    more hangs or trips the transport's size check -- round 2 shipped that bug for an hour)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GTE_BENCH_SHARE_GPU="1", MASTER_PORT=str(_free_port()))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "4", "--warmup", "2",
                        "--long-run-seconds", "0.05", "--resident-pages", "300", "--no-cpu-baseline"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{\"metric\"")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["long_run"]["steps"] >= 4
    assert d["value"] > 0 and np.isfinite(d["final_loss"])


# ---------------------------------------------------------------------------------------------------------------------
# train() end to end with two ranks (the box has one GPU: both ranks on cuda:0, gloo): the eval confusion-matrix all-reduce
# and the early-stop broadcast of model_train.py:230-249 run every epoch
def _train_worker(rank, world, port, out_dir, budget_gb=None, wide=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      GTE_KEEP_LAST_RUN="1")
    os.environ.pop("GTE_RESIDENT_BUDGET_GB", None)
    if budget_gb is not None:
        os.environ.update(GTE_RESIDENT_BUDGET_GB=str(budget_gb), GTE_WINDOW_PASSES="2")
    import torch.distributed as dist
    from gnn_tableextraction_amd.components.graphs.loader import PrebuiltPages
    from gnn_tableextraction_amd.models import model_train
    from gnn_tableextraction_amd.parsers.graphs import parse_args_ModelTrain
    dist.init_process_group("gloo", rank=rank, world_size=world)       # train() finds the group initialised and keeps it
    # wide: BBOX + REPR + SPACY = 363 input features, hidden 128 -- the input layer runs on the cached mean aggregate of the input
    # (a second resident image; the windows of a host-resident set compute theirs per upload)
    data = PrebuiltPages.synthetic(80 if wide else 40, in_feats=363 if wide else 13)
    for p, g in zip(data.page_arrays, data.graphs):                   # learnable labels (as test_gpu_train_entry.py)
        y = (p.feat[:, 1] // 260).astype(np.int64).clip(0, 8)
        p.label[:] = y
        g.ndata['label'] = torch.from_numpy(y.astype(np.float32))
    feats = ["BBOX", "REPR", "SPACY"] if wide else ["BBOX"]
    cfg = parse_args_ModelTrain(argv=["--mode=knn", "--features"] + feats + ["--n_layers=3", "--mode_params=fixed",
                                      f"--h_layer_dim={128 if wide else 64}",
                                      "--batch_size=4", "--n_epochs=3", "--lr=0.01", "--output_dir", os.path.join(out_dir, f"rank{rank}")])
    metrics = model_train.train(data, cfg)
    run = model_train.LAST_RUN
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, f"train_param_{rank}.npy"), run["step"].flat_param.detach().cpu().numpy())
    np.save(os.path.join(out_dir, f"train_m_{rank}.npy"), run["step"].exp_avg.detach().cpu().numpy())
    np.save(os.path.join(out_dir, f"train_metrics_{rank}.npy"),
            np.array([metrics.val.loss, metrics.val.acc, metrics.train.loss] + list(metrics.f1_vect)))
    if run["windows"] is not None:
        np.save(os.path.join(out_dir, f"train_windows_{rank}.npy"), np.array(run["windows"], dtype=np.float64))
    open(os.path.join(out_dir, f"train_tier_{rank}.txt"), "w").write(run["tier"])
    dist.barrier()
    dist.destroy_process_group()


def test_train_end_to_end_with_two_ranks_keeps_the_replicas_identical(tmp_path):
    """train(data, config) under WORLD_SIZE = 2: pages sharded per step, flat-gradient all-reduce, validation sharded with one
    all-reduce of (loss sum, correct, n, confusion matrix), early-stop flag broadcast from rank 0.  Both ranks end with the
    same parameters and optimiser state bit for bit and report the same (all-reduced) validation metrics; rank 0 alone
    writes the checkpoint, weights and results files."""
    world = 2
    mp.start_processes(_train_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    for name in ("train_param", "train_m"):
        a, b = np.load(tmp_path / f"{name}_0.npy"), np.load(tmp_path / f"{name}_1.npy")
        np.testing.assert_array_equal(a, b)
    m0, m1 = np.load(tmp_path / "train_metrics_0.npy"), np.load(tmp_path / "train_metrics_1.npy")
    np.testing.assert_array_equal(m0[:2], m1[:2])                       # all-reduced validation loss / accuracy
    np.testing.assert_array_equal(m0[3:], m1[3:])                       # per-class F1 from the all-reduced confusion matrix
    assert np.isfinite(m0).all() and m0[0] < np.log(9.0)
    assert os.path.isdir(tmp_path / "rank0" / "checkpoints") and os.path.isdir(tmp_path / "rank0" / "weights")
    assert not os.path.exists(tmp_path / "rank1" / "checkpoints") and not os.path.exists(tmp_path / "rank1" / "results")


def test_windowed_residency_with_two_ranks(tmp_path):
    """GTE_RESIDENT_BUDGET_GB below the training set's size: every rank keeps only ITS pages (about half of them) in pinned host
    memory and a window of those in HBM (models/residency.py); the step streams of both ranks are computed on every rank
    (global node counts without communication); replicas stay bit-identical."""
    world = 2
    # 38 training pages x ~230 nodes x 13 features x 4 B ~ 0.45 MB: a 0.0006 GB budget per rank forces several windows
    mp.start_processes(_train_worker, args=(world, _free_port(), str(tmp_path), 0.0006), nprocs=world, join=True, start_method="spawn")
    p0, p1 = (np.load(os.path.join(tmp_path, f"train_param_{r}.npy")) for r in range(world))
    np.testing.assert_array_equal(p0, p1)
    w0, w1 = (np.load(os.path.join(tmp_path, f"train_windows_{r}.npy")) for r in range(world))
    assert w0[0] >= 2 and w1[0] >= 2                          # several windows per rank
    assert abs(w0[3] - w1[3]) <= 1 and w0[3] + w1[3] == 38    # each rank holds about half of the 38 training pages
    assert w0[1] > 0 and w0[2] <= 0.0006e9 * 1.6              # something was uploaded; the device slots respect the budget (+ CSR slack)
    m0, m1 = (np.load(os.path.join(tmp_path, f"train_metrics_{r}.npy")) for r in range(world))
    np.testing.assert_array_equal(m0[:2], m1[:2])             # all-reduced validation loss / accuracy (the train loss is rank-local)
    np.testing.assert_array_equal(m0[3:], m1[3:])
    assert np.isfinite(m0).all()


def test_a_budget_the_ranks_share_fits_makes_every_rank_hold_only_its_own_pages(tmp_path):
    """GTE_RESIDENT_BUDGET_GB between set / world and set: round 4 compared the per-rank SHARE with the budget and then let every
    rank hold the WHOLE set.  Now a rank holds the pages it owns (residency.OwnedResident: one window, resident for good) and plans
    over them; replicas stay bit-identical and the validation metrics are the all-reduced ones."""
    world = 2
    # 38 training pages ~ 8 700 nodes x ~175 B in resident form ~ 1.5 MB: 1 MB holds a rank's half, not the set
    mp.start_processes(_train_worker, args=(world, _free_port(), str(tmp_path), 0.001), nprocs=world, join=True, start_method="spawn")
    assert [open(os.path.join(tmp_path, f"train_tier_{r}.txt")).read() for r in range(world)] == ["owned", "owned"]
    p0, p1 = (np.load(os.path.join(tmp_path, f"train_param_{r}.npy")) for r in range(world))
    np.testing.assert_array_equal(p0, p1)
    w0, w1 = (np.load(os.path.join(tmp_path, f"train_windows_{r}.npy")) for r in range(world))
    assert w0[0] == 1 and w1[0] == 1 and w0[3] + w1[3] == 38 and abs(w0[3] - w1[3]) <= 1
    assert w0[2] <= 0.001e9                                   # the bytes a rank holds respect the budget
    m0, m1 = (np.load(os.path.join(tmp_path, f"train_metrics_{r}.npy")) for r in range(world))
    np.testing.assert_array_equal(m0[:2], m1[:2])
    assert np.isfinite(m0).all() and m0[0] < np.log(9.0)


def _one_rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    import torch.distributed as dist
    import gnn_tableextraction_amd as gte
    from gnn_tableextraction_amd import graph as G
    from gnn_tableextraction_amd.data import synthetic as S
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    from gnn_tableextraction_amd.models.loop import BatchPipeline, run_steps
    dist.init_process_group("gloo", rank=0, world_size=1)
    dev = "cuda:0"
    out = {}
    for f0, hid in ((831, 256), (363, 149), (13, 256)):
        pages = S.make_pages(12, in_feats=f0)
        graphs = []
        for p in pages:
            g = gte.PageGraph(p.src, p.dst, p.num_nodes)
            g.ndata["feat"], g.ndata["label"] = torch.from_numpy(p.feat), torch.from_numpy(p.label.astype(np.float32))
            g.edata["feat"] = torch.from_numpy(p.weight)
            graphs.append(g)
        steps = [np.array([(3 * s + j) % 12 for j in range(5)]) for s in range(4)]
        res = {}
        for dp in (False, True):
            torch.manual_seed(5)
            model = gte.GcnSAGE(f0, hid, 9, 3, torch.nn.functional.relu, 0).to(dev)
            tr = FusedGcnSageStep(model, lr=0.01, weight_decay=5e-4, distributed=dp)
            pipe = BatchPipeline(G.ResidentPages(graphs, dev))
            losses = []
            counts = [int(sum(pages[i].num_nodes for i in ids)) for ids in steps]
            run_steps(tr, pipe, steps, n_global=counts if dp else None, on_step=lambda s, g, o: losses.append(float(o[0])))
            torch.cuda.synchronize()
            res[dp] = (np.array(losses), tr.flat_param.detach().cpu().numpy(), tr.exp_avg_sq.detach().cpu().numpy(), tr._wimg_sig is not None)
        out[f"{f0}_{hid}"] = res
    import pickle
    pickle.dump(out, open(os.path.join(out_dir, "one_rank.pkl"), "wb"))
    dist.destroy_process_group()


def test_data_parallel_step_with_one_rank_is_bitwise_the_single_gpu_step(tmp_path):
    """The data-parallel step (fold launch -> all-reduce -> ONE launch for Adam + the weight images of the next forward,
    gte_adam_step_dev_images) with a world of one rank against the one-GPU step (Adam and the images inside the fold launch): the
    same arithmetic in a different launch -- losses, parameters and optimiser state bit for bit over four steps of the train loop,
    and the images really were left by the optimiser launch (the next forward skipped their conversion)."""
    import pickle
    mp.start_processes(_one_rank_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    out = pickle.load(open(tmp_path / "one_rank.pkl", "rb"))
    for k, res in out.items():
        (l0, p0, v0, _), (l1, p1, v1, fresh) = res[False], res[True]
        np.testing.assert_array_equal(l0, l1, err_msg=k)
        np.testing.assert_array_equal(p0, p1, err_msg=k)
        np.testing.assert_array_equal(v0, v1, err_msg=k)
        assert fresh, f"{k}: the data-parallel optimiser launch did not leave the weight images behind"


def test_windowed_residency_with_the_cached_aggregate_and_two_ranks(tmp_path):
    """train() at 363 input features / hidden 128 under a budget below a rank's share: the windows carry the image of the input's
    mean aggregate (computed per upload on the copy stream) and the input layer runs on it; two ranks keep bit-identical replicas,
    the run learns."""
    world = 2
    # 76 training pages ~ 17 500 nodes x (2 x 2 208 B of images + ~120 B of CSRs) ~ 80 MB: 30 MB per rank (a slot of ~13 MB holds the
    # largest page) forces three or four windows per rank
    mp.start_processes(_train_worker, args=(world, _free_port(), str(tmp_path), 0.03, True), nprocs=world, join=True, start_method="spawn")
    assert [open(os.path.join(tmp_path, f"train_tier_{r}.txt")).read() for r in range(world)] == ["windowed", "windowed"]
    p0, p1 = (np.load(os.path.join(tmp_path, f"train_param_{r}.npy")) for r in range(world))
    np.testing.assert_array_equal(p0, p1)
    w0 = np.load(os.path.join(tmp_path, "train_windows_0.npy"))
    assert w0[0] >= 2 and w0[1] > 0
    m0 = np.load(os.path.join(tmp_path, "train_metrics_0.npy"))
    assert np.isfinite(m0).all() and m0[0] < np.log(9.0)
