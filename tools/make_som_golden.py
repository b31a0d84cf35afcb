"""Golden cases of the one-dimensional self-organising map  --  TEST INFRASTRUCTURE, run on the build machine only (it needs the
reference tree).

Imports the REFERENCE's ``MiniSom`` (src/components/tables/som/som.py, loaded by file path at run time: the package around it
imports libraries that are not needed here); none of its text is held in this repository.  For a few (seed, data, iterations)
cases it trains ``MiniSom(units, 1, 1, sigma, learning_rate, random_seed=seed).train_random(data, iterations)`` as
``Preprocessor.train_som`` does -- the data a list of one-element lists of np.float32 -- and writes tests/golden/som_cases.json:
the inputs and the weights only, as ``float.hex`` strings (the parity asserted by tests/test_gmm_host.py is equality).

    python tools/make_som_golden.py [reference/src]        # writes tests/golden/som_cases.json
"""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [  # name, seed, units, sigma, learning rate, iterations, data seed, n samples, log space
    ("default_10", 42, 10, 0.03, 0.3, 300, 1, 500, False),
    ("wide_sigma_7", 7, 7, 0.8, 0.5, 250, 2, 64, False),
    ("log_space_10", 42, 10, 0.03, 0.3, 300, 3, 400, True),
    ("one_unit", 3, 1, 0.03, 0.3, 20, 4, 5, False),
    ("one_iteration", 0, 4, 0.3, 0.3, 1, 5, 9, False),
]


def case_data(data_seed, n, log_space):
    from gnn_tableextraction_amd.components.tables.numerals import weighted_log
    rng = np.random.RandomState(data_seed)
    values = (rng.lognormal(1.0, 2.0, size=n) * rng.choice([-1.0, 1.0, 1.0, 1.0], size=n)).astype(np.float32)
    if log_space:
        values = np.array([weighted_log(v) for v in values], dtype=np.float32)
    return values


def main(src_root):
    path = os.path.join(src_root, "components", "tables", "som", "som.py")
    spec = importlib.util.spec_from_file_location("reference_som", path)
    som = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(som)
    out = []
    for name, seed, units, sigma, lr, iters, data_seed, n, log_space in CASES:
        values = case_data(data_seed, n, log_space)
        data = [[v] for v in values]                                     # what train_som hands over
        m = som.MiniSom(units, 1, 1, sigma=sigma, learning_rate=lr, random_seed=seed)
        with contextlib.redirect_stdout(io.StringIO()):
            m.train_random(data, iters)
        weights = m.get_weights().reshape(units)
        out.append({"name": name, "seed": seed, "units": units, "sigma": sigma, "learning_rate": lr, "iterations": iters,
                    "data": [float(v).hex() for v in values], "weights": [float(v).hex() for v in weights]})
        print(name, weights)
    dst = os.path.join(ROOT, "tests", "golden", "som_cases.json")
    with open(dst, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        from oracle.make_aux_golden import REF                          # where the other golden tools read the reference
        main(REF)
