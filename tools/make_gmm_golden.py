"""How far summation order alone moves scikit-learn's own Gaussian-mixture fit  --  TEST INFRASTRUCTURE, run where scikit-learn
(1.7.2) is installed.

For every fit case of tests/gmm_ref.py (FIT_CASES) and both types it fits scikit-learn's estimator (``hard``: the subclass of
tests/gmm_ref.py) to ``x`` and to ``x[::-1]`` from the same initial parameters and writes
    d = the largest relative difference between the two fits in weights, means, covariances and the lower bound
to tests/golden/gmm_sensitivity.json.  tests/test_gmm_ref_cpu.py and tests/test_gpu_gmm.py allow ``1000 * max(d, eps)`` between
scikit-learn, the numpy oracle and the device.  The tool asserts what the tests rely on: both orders run the same number of
iterations and converge, and no ``|change|`` of the forward run lies within 1e-6 of ``tol``.

    python tools/make_gmm_golden.py        # writes tests/golden/gmm_sensitivity.json
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gmm_ref as ref                                         # noqa: E402

TOL = 1e-3


def fitted(x, hard, K, w, mu, prec):
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # a fit that does not converge is no case
        return ref.sklearn_estimator(hard, K, w, mu, prec, tol=TOL).fit(x.reshape(-1, 1))


def main():
    import sklearn
    out = {}
    for name, (n, K, _) in ref.FIT_CASES.items():
        x, w, mu, prec = ref.fit_case(name)
        out[name] = {}
        for kind in ("soft", "hard"):
            a, b = fitted(x, kind == "hard", K, w, mu, prec), fitted(x[::-1].copy(), kind == "hard", K, w, mu, prec)
            assert a.n_iter_ == b.n_iter_ and a.converged_ and b.converged_, (name, kind, a.n_iter_, b.n_iter_)
            assert all(abs(abs(c) - TOL) > 1e-6 for c in a.changes_), (name, kind, a.changes_)
            d = max(ref.rel_diff(b.weights_, a.weights_), ref.rel_diff(b.means_, a.means_), ref.rel_diff(b.covariances_, a.covariances_),
                    ref.rel_diff([b.lower_bound_], [a.lower_bound_]))
            out[name][kind] = d
            print(f"{name} {kind}: n {n} K {K} n_iter {a.n_iter_} last change {a.changes_[-1]:.3e} d {d:.3e}")
    path = ref.GOLDEN
    with open(path, "w") as f:
        json.dump({"sklearn_version": sklearn.__version__, **out}, f, indent=1)
    print(path)


if __name__ == "__main__":
    main()
