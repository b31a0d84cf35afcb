"""The REPR vocabulary of a corpus: counts of word shapes, and the vocabulary files that the REPR embedder reads
(``Vocabulator.build_repr_vocab`` and ``dump`` of the reference, src/components/tables/vocabulator.py:66-73, 223-231).  Host only.

Counting uses the project's own ``components.nlp.repr.page_tokens``: exactly the tokens that ``Repr.token_ids`` will later look up
are counted.  The reference counts with its ``Manager`` chain instead (it needs ``bs4``, collapses every repeated character and
drops number signs), which produces shapes that its own embedder's normaliser never produces; that chain is deliberately not
restated.  A caller who has the reference's ``rc.dat`` passes that dictionary to ``build_repr_vocab`` / ``train_repr`` instead."""
from __future__ import annotations

import os
import pickle
from typing import Dict, Iterable, List, Sequence, Set, Tuple

from ..nlp.repr import UNK, page_tokens


def count_representations(page_texts: Iterable[Sequence[str]], unk: str = UNK) -> Dict[str, int]:
    """token -> count over all pages (``page_texts``: one list of word texts per page), seeded with ``{unk: 1}`` as the
    reference's counter is."""
    rc = {unk: 1}
    for words in page_texts:
        for tok in page_tokens(words):
            rc[tok] = rc.get(tok, 0) + 1
    return rc


def build_repr_vocab(rc: Dict[str, int], max_vocab: int = 2000, unk: str = UNK) -> Tuple[List[str], Dict[str, int], Set[str]]:
    """(idx2repr, repr2idx, repr_vocab) as vocabulator.py:223-231: the unknown token first, then the other tokens by count
    descending -- Python's stable sort, so tokens of equal count keep the order of ``rc`` -- ``max_vocab - 1`` of them."""
    if unk not in rc:
        raise ValueError(f"build_repr_vocab: rc has no {unk!r} entry (count_representations seeds one)")
    rest = {t: c for t, c in rc.items() if t != unk}
    idx2repr = [unk] + sorted(rest, key=rest.get, reverse=True)[:max(int(max_vocab) - 1, 0)]
    repr2idx = {t: i for i, t in enumerate(idx2repr)}
    return idx2repr, repr2idx, set(repr2idx)


def dump_repr_files(directory, rc, idx2repr, repr2idx, repr_vocab) -> None:
    """The four pickles of the reference's ``Vocabulator.dump`` under its file names: ``rc.dat``, ``repr_vocab.dat``,
    ``idx2repr.dat``, ``repr2idx.dat`` (the last is what ``Repr.from_reference_files`` reads)."""
    os.makedirs(str(directory), exist_ok=True)
    for name, obj in (("rc.dat", rc), ("repr_vocab.dat", repr_vocab), ("idx2repr.dat", idx2repr), ("repr2idx.dat", repr2idx)):
        with open(os.path.join(str(directory), name), "wb") as f:
            pickle.dump(obj, f)
