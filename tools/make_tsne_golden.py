"""tests/golden/tsne_quality.json: the quality scikit-learn's exact t-SNE reaches on the matrix of the end-to-end test of
tests/test_gpu_tsne.py -- ``tests/tsne_ref.cluster_distances()``, the [200, 200] distances of four seeded Gaussian clusters.
``TSNE(n_components=3, method='exact', init='random', metric='precomputed', random_state=s)`` for s = 0 .. 3 on the CPU; recorded:
each ``kl_divergence_``, each ``n_iter_`` and the scikit-learn version.  The device route must reach a KL divergence no worse
than max + (max - min) of these.
usage: python tools/make_tsne_golden.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                     # noqa: E402
import sklearn                                                         # noqa: E402
from sklearn.manifold import TSNE                                      # noqa: E402
from tests import tsne_ref as ref                                      # noqa: E402


def main():
    D = ref.cluster_distances()
    runs = []
    for seed in range(4):
        est = TSNE(n_components=3, method="exact", init="random", metric="precomputed", random_state=seed).fit(D)
        runs.append({"random_state": seed, "kl_divergence": float(est.kl_divergence_), "n_iter": int(est.n_iter_)})
        print(runs[-1], flush=True)
    record = {"matrix": "tests/tsne_ref.cluster_distances(): 4 clusters x 50 points, 5 dimensions, centres at scale 6, seed 0",
              "n_components": 3, "perplexity": 30.0, "sklearn": sklearn.__version__, "numpy": np.__version__, "runs": runs}
    path = os.path.join(ROOT, "tests", "golden", "tsne_quality.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


main()
