"""``affinity`` of the reference's src/utils/matrixes.py -- ``AffinityPropagation(affinity='precomputed', damping=0.9)`` on a
similarity matrix, returning ``(cluster_centers_indices_, labels_)`` -- with the sweeps on the HIP device
(components/tables/affinity.py) and scikit-learn's results."""
from __future__ import annotations

from ..components.tables.affinity import affinity_propagation


def affinity(matrix, device=None, random_state=None):
    """``(centers, labels)`` of affinity propagation with damping 0.9 over the precomputed similarities ``matrix`` [n, n].
    ``device``: the HIP device (None: the current one); ``random_state`` seeds the degeneracy noise as scikit-learn's does."""
    return affinity_propagation(matrix, damping=0.9, random_state=random_state, device=device)
