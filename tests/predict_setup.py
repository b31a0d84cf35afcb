"""What every test of ``model_predict.test()`` sets up first: a config whose output goes to a temporary directory and the weights
of a seeded, untrained model where ``test()`` looks for them."""
import os

import torch

from gnn_tableextraction_amd import GcnSAGE
from gnn_tableextraction_amd.parsers.graphs import parse_args_ModelTrain
from gnn_tableextraction_amd.utils.config import logs_from_config


def config_and_weights(tmp_path, batch_size=4, seed=3):
    """(config for ``--output_dir tmp_path``, the model whose weights now lie under ``weights/{logs}.pt``, ``logs``): BBOX features,
    3 layers, 64 hidden units, 9 classes, no dropout."""
    cfg = parse_args_ModelTrain(argv=["--mode=knn", "--features", "BBOX", "--n_layers=3", "--mode_params=fixed", "--h_layer_dim=64",
                                      f"--batch_size={batch_size}", "--n_epochs=1", "--output_dir", str(tmp_path)])
    torch.manual_seed(seed)
    model = GcnSAGE(13, 64, 9, 3, torch.nn.functional.relu, 0)
    logs = logs_from_config(cfg)
    os.makedirs(tmp_path / "weights", exist_ok=True)
    torch.save(model.state_dict(), tmp_path / "weights" / f"{logs}.pt")
    return cfg, model, logs
