"""The training methods of the reference's ``Preprocessor`` (src/components/tables/preprocessor.py) that produce files.

``train_repr`` (:282-342): REPR prototypes and embeddings from representation counts.  The all-pairs similarity matrix comes from
one HIP launch (components/tables/levenshtein.py); affinity propagation is scikit-learn's on the host, as in the reference, or --
with ``affinity='device'`` -- HIP sweeps with the same result (components/tables/affinity.py); t-SNE is scikit-learn's on the host
or -- with ``tsne='device'`` -- the exact method in HIP kernels (components/tables/tsne.py).
What this does NOT produce is ``i_embedding`` (the [C, P] output rows of the prototypes): the reference trains it with the
``tblemb`` package, which it does not ship.  It stays the caller's.

``train_som`` (:88-133) and ``train_gmm`` (:137-279): numeral prototypes from numeral counts ``nc``.  The samples are
components/tables/numerals.py's; the self-organising map is sequential host numpy (components/tables/som.py); the Gaussian
mixture's EM iterations and the posterior of every distinct numeral run in HIP kernels (components/tables/gmm.py), without
scikit-learn.  The reference's ``train_gmm`` cannot finish as written (it pickles into a file opened for reading, its random
initialisation mixes scalars and arrays on a current numpy, its hard EM is written against a scikit-learn API that 1.7.2 no
longer has); this one returns what it would have pickled.  Counting ``nc`` from a corpus and the plots are not restated."""
from __future__ import annotations

import os
import pickle
from typing import Dict, List, Optional

import numpy as np

from .levenshtein import LevenshteinSimilitudes
from .vocabulator import build_repr_vocab


def repr_words(rc: Dict[str, int], limit: int = 2000, align: bool = False) -> List[str]:
    """The words that ``train_repr`` works on, in its order.  Default (preprocessor.py:293-296): all tokens of ``rc`` -- the
    unknown token included, wherever its count puts it -- by count descending in Python's stable order, the first ``limit`` of
    them.  ``align=True``: ``idx2repr`` of ``build_repr_vocab(rc, limit)`` instead, the unknown token first."""
    if align:
        return build_repr_vocab(rc, max_vocab=limit)[0]
    return sorted(rc, key=rc.get, reverse=True)[:max(int(limit), 0)]


def train_repr(rc: Dict[str, int], n_components: int = 3, limit: int = 2000, device=None, similarity=None, random_state=None,
               tsne_kwargs: Optional[dict] = None, align: bool = False, affinity: str = "host", tsne: str = "host") -> dict:
    """``{'centers', 'labels', 'words', 'embeddings'}`` as the reference pickles them (preprocessor.py:335-340):
    ``words`` numpy str [n], n = min(limit, len(rc)); ``centers`` the indices into ``words`` of the affinity-propagation
    exemplars; ``labels`` int [n], the cluster of every word; ``embeddings`` float [n, n_components], the t-SNE embedding.

    Steps, as there: ``repr_words(rc, limit)``; the similarity matrix ``LevenshteinSimilitudes().init_weights()
    .calculate_similarity(words, device=device)`` on the HIP device -- or the caller's ``similarity`` [n, n] over those words in
    that order, which lets the rest run without a GPU; ``AffinityPropagation(affinity='precomputed', damping=0.9)``; the matrix
    squared, NaN replaced by the mean and infinities by the maximum of the finite entries; ``TSNE(n_components,
    metric='precomputed', init='random', **tsne_kwargs)``.  ``random_state`` goes to both estimators.

    Differences from the reference, all deliberate:
      * ``init='random'``: the reference calls TSNE with its default ``init='pca'``, which scikit-learn (1.7.2 was tried) rejects
        together with ``metric='precomputed'``; its call cannot run on such a version.
      * its debug prints of ``words[1968]`` and four more (``ord`` of a whole word: a TypeError for any word longer than one
        character) are dropped.
      * nothing is written: ``write_embed_repr`` does that.
      * ``align``.  The reference's embedder indexes ``embeddings`` with ``repr2idx`` ids although the orders differ: ``words`` is
        sorted with the unknown token in place, ``idx2repr`` puts it first, so every token ranked above the unknown one reads
        its neighbour's row.  The default keeps that.  ``align=True`` works on ``idx2repr`` order throughout (``repr_words(rc,
        limit, align=True)``), so row ``repr2idx[t]`` of ``embeddings`` is token ``t``'s and ``centers`` / ``labels`` index the
        same order: a deviation from the reference.
    ``affinity``: where the clustering runs.  'host' (the default) is scikit-learn's ``AffinityPropagation``; 'device' is
    ``components/tables/affinity.affinity_propagation`` with the same damping and ``random_state`` -- the sweeps in HIP kernels on
    ``device``, centres and labels equal to scikit-learn's.
    ``tsne``: where the embedding is computed.  'host' (the default) is scikit-learn's ``TSNE`` as above (Barnes-Hut:
    ``n_components`` <= 3).  'device' is ``components/tables/tsne.tsne`` on the same cleaned squared matrix with ``random_state`` and
    ``tsne_kwargs`` passed on: scikit-learn's EXACT method (conditional and joint probabilities and the 1000 iterations in HIP
    kernels on ``device``, float64), which takes the reference's own ``n_components=4``.  The descent is chaotic, so its
    coordinates are not scikit-learn's; the quality reached (the KL divergence) is.  ``tsne_kwargs`` there: ``perplexity``,
    ``early_exaggeration``, ``learning_rate``, ``max_iter``, ``n_iter_without_progress``, ``min_grad_norm``, ``init``.
    With ``affinity='device', tsne='device'`` scikit-learn is not imported at all.
    scikit-learn is imported here, not at module level: nothing else in the package needs it."""
    if affinity not in ("host", "device"):
        raise ValueError(f"train_repr: affinity must be 'host' or 'device', got {affinity!r}")
    if tsne not in ("host", "device"):
        raise ValueError(f"train_repr: tsne must be 'host' or 'device', got {tsne!r}")
    words = repr_words(rc, limit, align=align)
    n = len(words)
    if similarity is None:
        matrix = LevenshteinSimilitudes().init_weights().calculate_similarity(words, device=device)
    else:
        matrix = np.array(similarity, dtype=np.float64)
    if matrix.shape != (n, n):
        raise ValueError(f"train_repr: the similarity matrix is {matrix.shape}, {n} words need ({n}, {n})")
    if affinity == "device":
        from .affinity import affinity_propagation
        centers, labels = affinity_propagation(matrix, damping=0.9, random_state=random_state, device=device)
        if tsne == "host":
            try:
                from sklearn.manifold import TSNE
            except ImportError as e:
                raise ImportError("train_repr: scikit-learn is needed for the one stage that stays on the host, the t-SNE embedding "
                                  "(sklearn.manifold.TSNE); tsne='device' needs none") from e
    else:
        try:
            from sklearn.cluster import AffinityPropagation
            if tsne == "host":
                from sklearn.manifold import TSNE
        except ImportError as e:
            raise ImportError("train_repr: scikit-learn is needed for the stages that stay on the host, the affinity propagation "
                              "(sklearn.cluster.AffinityPropagation) and, with tsne='host', the t-SNE embedding "
                              "(sklearn.manifold.TSNE)") from e
        affprop = AffinityPropagation(affinity="precomputed", damping=0.9, random_state=random_state).fit(matrix)
        centers, labels = affprop.cluster_centers_indices_, affprop.labels_

    matrix = np.square(matrix)
    finite = matrix[matrix != np.inf]
    mean_, max_ = np.nanmean(finite), np.nanmax(finite)                    # (preprocessor.py:317-320)
    matrix = np.nan_to_num(matrix, nan=mean_, posinf=max_, neginf=max_)
    if tsne == "device":
        from .tsne import tsne as device_tsne
        embeddings = device_tsne(matrix, n_components, random_state=random_state, device=device, **(tsne_kwargs or {}))
    else:
        embeddings = TSNE(n_components=n_components, metric="precomputed", init="random", random_state=random_state,
                          **(tsne_kwargs or {})).fit_transform(matrix)
    return {"centers": centers, "labels": labels, "words": np.asarray(words), "embeddings": embeddings}


def write_embed_repr(directory, result: dict, n_components: int, limit: int) -> str:
    """Pickles ``result`` as ``<directory>/embed-repr-<len(centers)>-<n_components>-<limit>.dat`` (preprocessor.py:341) and
    returns the path.  As there, ``limit`` is the number of words that were taken: a ``limit`` above it is lowered to it, and
    that number is what ``Repr.from_reference_files`` wants as ``top_k``."""
    limit = min(int(limit), len(result["words"]))
    os.makedirs(str(directory), exist_ok=True)
    path = os.path.join(str(directory), f"embed-repr-{len(result['centers'])}-{n_components}-{limit}.dat")
    with open(path, "wb") as f:
        pickle.dump(result, f)
    return path


GMM_INIT_MODES = ("rd", "fp", "km")
GMM_TYPES = ("soft", "hard")


def train_som(nc: Dict[str, int], prototypes: int = 10, sigma: float = 0.03, lr: float = 0.3, iters: int = 10000,
              log_space: bool = False, random_seed: int = 42) -> np.ndarray:
    """float64 [prototypes]: the weights of the reference's ``train_som`` (preprocessor.py:88-133): ``nc`` unfolded and shuffled
    (``numeral_samples`` without a cap, as there), ``weighted_log`` when ``log_space``, then the 1-D map of components/tables/som.py
    trained for ``iters`` random updates.  ``random_seed`` seeds both the shuffle and the map, as the reference's ``RANDOM_SEED``
    does.  Nothing is written: ``write_som_prototypes`` does that."""
    from .numerals import numeral_samples
    from .som import train_som_1d
    data = numeral_samples(nc, random_state=random_seed, cap=None, log_space=log_space)
    if data.shape[0] < 1:
        raise ValueError("train_som: nc holds no valid numeral")
    return train_som_1d(data, prototypes, sigma=sigma, learning_rate=lr, num_iteration=iters, random_seed=random_seed)


def train_gmm(nc: Dict[str, int], components: int = 20, iters: int = 100, gmm_init_mode: str = "rd", gmm_type: str = "soft",
              prototypes=None, log_space: bool = False, random_state: int = 42, device=None) -> dict:
    """``{'gmm', 'posterior', 'numerals'}``: the mixture that the reference's ``train_gmm`` (preprocessor.py:137-279) fits to the
    numerals of ``nc`` and the posterior it pickles.  ``gmm``: a ``components/tables/gmm.GmmResult`` (``weights_``, ``means_``,
    ``covariances_``, ... as the estimator's); ``numerals``: the valid keys of ``nc`` in dictionary order; ``posterior`` float64
    [len(numerals), components]: ``predict_proba`` of their values (``weighted_log`` of them when ``log_space``).

    Steps, as there: ``numeral_samples(nc, random_state, cap=2 000 000, log_space)``; prototypes -- ``'rd'``:
    ``np.random.RandomState(random_state).choice(data, components)``, with replacement as the reference draws them; ``'fp'``: the
    caller's ``prototypes`` (``train_som``'s, for example; the reference unpickles them); then ``init_from_prototypes`` (its
    quirks are named there) and ``iters`` EM iterations at scikit-learn's default ``tol`` and ``reg_covar``, ``gmm_type`` 'soft'
    (``GaussianMixture``) or 'hard' (``HardEMGaussianMixture``), on the HIP ``device``.
    ``'km'`` raises ``NotImplementedError``: it is scikit-learn's KMeans initialisation on up to 2 000 000 points, out of scope.
    Any other mode or type raises ``ValueError`` before any other work.
    Differences from the reference, all deliberate: nothing is written (``write_gmm_files`` does that) or plotted; the posterior
    is computed in float64 (there the float32 points make scikit-learn compute in float32) and only for the valid numerals (there
    ``np.array(list(nc.keys()), dtype=np.float32)`` raises on an invalid one); a cluster with zero standard deviation is a
    ``ValueError`` here and a LinAlgError there."""
    if gmm_init_mode not in GMM_INIT_MODES:
        raise ValueError(f"train_gmm: gmm_init_mode must be one of {GMM_INIT_MODES}, got {gmm_init_mode!r}")
    if gmm_type not in GMM_TYPES:
        raise ValueError(f"train_gmm: gmm_type must be one of {GMM_TYPES}, got {gmm_type!r}")
    if gmm_init_mode == "km":
        raise NotImplementedError("train_gmm: gmm_init_mode='km' (scikit-learn's KMeans initialisation) is not restated; "
                                  "use 'rd' or 'fp'")
    components = int(components)
    if gmm_init_mode == "fp":
        if prototypes is None:
            raise ValueError("train_gmm: gmm_init_mode='fp' needs prototypes (train_som's, for example)")
        prototypes = np.asarray(prototypes, dtype=np.float64).reshape(-1)
        if prototypes.shape[0] != components:
            raise ValueError(f"train_gmm: {prototypes.shape[0]} prototypes for {components} components")
    from . import gmm as gmm_mod
    from .numerals import numeral_samples, valid_numerals, weighted_log
    data = numeral_samples(nc, random_state=random_state, cap=2_000_000, log_space=log_space)
    if data.shape[0] < 1:
        raise ValueError("train_gmm: nc holds no valid numeral")
    if gmm_init_mode == "rd":
        prototypes = np.random.RandomState(random_state).choice(data, components)
    weights, means, precisions = gmm_mod.init_from_prototypes(data, prototypes)
    prepared = gmm_mod.prepare(data, weights, means, precisions, hard=gmm_type == "hard", max_iter=int(iters))
    result = gmm_mod.run(prepared, device)
    keys, values = valid_numerals(nc)
    points = np.array(values, dtype=np.float32)
    if log_space:
        points = np.array([weighted_log(v) for v in points], dtype=np.float32)
    posterior = gmm_mod.predict_proba(result, points.astype(np.float64), device) if keys else np.zeros((0, components))
    return {"gmm": result, "posterior": posterior, "numerals": keys}


def write_gmm_files(directory, out: dict, components: int, gmm_init_mode: str, gmm_type: str, log_space: bool = False):
    """Pickles ``out['gmm']`` as ``<directory>/gmm[_log]/gmm-<C>-<mode>-<type>.dat`` and ``out['posterior']`` as
    ``gmm_posterior-<C>-<mode>-<type>.dat`` next to it (preprocessor.py:268, 277; both opened for writing) and returns the two
    paths.  The model is pickled as a plain dict of its attributes, not as a scikit-learn estimator."""
    folder = os.path.join(str(directory), "gmm_log" if log_space else "gmm")
    os.makedirs(folder, exist_ok=True)
    tag = f"{components}-{gmm_init_mode}-{gmm_type}"
    model = out["gmm"]
    model = model._asdict() if hasattr(model, "_asdict") else model
    paths = (os.path.join(folder, f"gmm-{tag}.dat"), os.path.join(folder, f"gmm_posterior-{tag}.dat"))
    for path, obj in zip(paths, (model, out["posterior"])):
        with open(path, "wb") as f:
            pickle.dump(obj, f)
    return paths


def write_som_prototypes(directory, weights, prototypes: int, sigma: float, lr: float, log_space: bool = False) -> str:
    """Pickles the map's weights as ``<directory>/som[_log]/prototypes-<P>-<sigma>-<lr>.dat`` (preprocessor.py:124-132) and returns
    the path."""
    folder = os.path.join(str(directory), "som_log" if log_space else "som")
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, f"prototypes-{prototypes}-{sigma}-{lr}.dat")
    with open(path, "wb") as f:
        pickle.dump(np.asarray(weights), f)
    return path
