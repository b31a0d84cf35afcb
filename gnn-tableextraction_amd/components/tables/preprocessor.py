"""REPR prototypes and embeddings from representation counts: ``Preprocessor.train_repr`` of the reference
(src/components/tables/preprocessor.py:282-342).  The all-pairs similarity matrix comes from one HIP launch
(components/tables/levenshtein.py); affinity propagation is scikit-learn's on the host, as in the reference, or -- with
``affinity='device'`` -- HIP sweeps with the same result (components/tables/affinity.py); t-SNE is scikit-learn's on the host or
-- with ``tsne='device'`` -- the exact method in HIP kernels (components/tables/tsne.py).

What this does NOT produce is ``i_embedding`` (the [C, P] output rows of the prototypes): the reference trains it with the
``tblemb`` package, which it does not ship.  It stays the caller's."""
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
