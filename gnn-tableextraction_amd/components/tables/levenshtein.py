"""Weighted Levenshtein similarities of word shapes: the interface of the reference's ``LevenshteinSimilitudes``
(src/components/tables/levenshtein.py), with the Python double loop of n^2 calls into the ``weighted_levenshtein`` extension
replaced by ONE launch of gte_lev_matrix_f64 over all pairs.

Host side: only the string work -- words to code points, the sorted set of code points as the compact alphabet, the dense cost
tables over that alphabet.  Every distance is computed in csrc/lev_matrix.hip by the recurrence stated in include/gte.h, which is
the recurrence of ``weighted_levenshtein.lev`` (equal characters copy the diagonal cell, NO minimum is taken there).  That library
is not a dependency and was not available when this was written: parity is with the recurrence (tests/lev_ref.py) and the hand
cases of tests/golden/lev_cases.json, not with recorded library output.

Costs are kept as three defaults plus per-character overrides, not as the reference's 10001-wide arrays (its substitution table
alone is 800 MB).  A code point above 10000 indexes past those arrays and raises in the reference; here it takes the default costs
(or its override, if one was set)."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from ... import _lib, graph as G

BOM = "\ufeff"


def _point(ch) -> int:
    if isinstance(ch, str):
        if len(ch) != 1:
            raise ValueError(f"LevenshteinSimilitudes: {ch!r} is not one character")
        return ord(ch)
    return int(ch)


def alphabet_of(*word_lists: Sequence[str]) -> List[int]:
    """The sorted set of code points of all words of all lists: code point ``alphabet[k]`` has the compact id ``k``."""
    return sorted({ord(ch) for words in word_lists for w in words for ch in w})


def encode(words: Sequence[str], alphabet: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """(uint16 [total] compact ids of all words, concatenated; int32 [n + 1] offsets): word p is ``chars[off[p]:off[p+1]]``."""
    ids = {c: k for k, c in enumerate(alphabet)}
    off = np.zeros(len(words) + 1, dtype=np.int64)
    np.cumsum([len(w) for w in words], out=off[1:])
    chars = np.fromiter((ids[ord(ch)] for w in words for ch in w), dtype=np.uint16, count=int(off[-1]))
    return chars, off.astype(np.int32)


class LevenshteinSimilitudes:
    """Drop-in for the reference's class: ``LevenshteinSimilitudes().init_weights().calculate_similarity(words)``."""

    def __init__(self):
        self.init_weights_uniform()

    def init_weights_uniform(self) -> "LevenshteinSimilitudes":
        """Every insertion, deletion and substitution costs 1.0; all overrides are dropped."""
        self.default_insert = self.default_delete = self.default_substitute = 1.0
        self.insert_overrides: Dict[int, float] = {}
        self.delete_overrides: Dict[int, float] = {}
        self.substitute_overrides: Dict[Tuple[int, int], float] = {}
        return self

    def set_insert(self, ch, cost: float) -> "LevenshteinSimilitudes":
        self.insert_overrides[_point(ch)] = float(cost)
        return self

    def set_delete(self, ch, cost: float) -> "LevenshteinSimilitudes":
        self.delete_overrides[_point(ch)] = float(cost)
        return self

    def set_substitute(self, src, dst, cost: float) -> "LevenshteinSimilitudes":
        """The cost of replacing ``src`` (a character of the first word) by ``dst`` (of the second); one direction only."""
        self.substitute_overrides[(_point(src), _point(dst))] = float(cost)
        return self

    def init_weights(self) -> "LevenshteinSimilitudes":
        """The reference's overrides (levenshtein.py:33-46), on top of what is set already, as there."""
        for ch, cost in (("%", 1.5), (".", 2.0), (",", 2.0)):
            self.set_delete(ch, cost).set_insert(ch, cost)
        self.set_substitute(".", ",", 1.9).set_substitute(",", ".", 1.9)
        self.set_substitute("w", "x", 1.9).set_substitute("x", "w", 1.9)
        return self.set_substitute("x", "%", 5.0)                          # (one direction only, as there)

    def tables(self, alphabet: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Dense float64 tables over a compact alphabet: insert [A], delete [A], substitute [A, A] (row: the character that is
        replaced).  Overrides of characters outside the alphabet do not appear."""
        ids = {c: k for k, c in enumerate(alphabet)}
        n = len(alphabet)
        ins = np.full(n, self.default_insert, dtype=np.float64)
        dele = np.full(n, self.default_delete, dtype=np.float64)
        sub = np.full((n, n), self.default_substitute, dtype=np.float64)
        for c, cost in self.insert_overrides.items():
            if c in ids:
                ins[ids[c]] = cost
        for c, cost in self.delete_overrides.items():
            if c in ids:
                dele[ids[c]] = cost
        for (a, b), cost in self.substitute_overrides.items():
            if a in ids and b in ids:
                sub[ids[a], ids[b]] = cost
        return ins, dele, sub

    def prepare(self, words: Sequence[str]):
        """The host work of ``calculate_similarity``, no device involved: (src words, dst words, alphabet).  ``dst`` are the words
        as they stand, ``src`` the words without U+FEFF: the reference strips only the first argument of ``lev``.  ``ValueError``
        for a word longer than the kernel's limit (64 characters) or more distinct characters than its tables take (1024)."""
        lib = _lib.load()
        max_len, max_alpha = lib.gte_lev_max_len(), lib.gte_lev_max_alphabet()
        dst = [str(w) for w in words]
        src = [w.replace(BOM, "") for w in dst]
        for w in dst:
            if len(w) > max_len:
                raise ValueError(f"LevenshteinSimilitudes: the word {w!r} has {len(w)} characters, the kernel takes {max_len}")
        alphabet = alphabet_of(src, dst) or [0]                            # (only empty words: one character that no word holds)
        if len(alphabet) > max_alpha:
            raise ValueError(f"LevenshteinSimilitudes: {len(alphabet)} distinct characters, the kernel takes {max_alpha}")
        return src, dst, alphabet

    def calculate_similarity(self, words: Sequence[str], weights=None, device=None) -> np.ndarray:
        """numpy float64 [n, n] with ``matrix[i, j] = -lev(words[j] without U+FEFF -> words[i])`` (levenshtein.py:50-63).  The
        asymmetry is the reference's own: only the first argument is stripped, so a word that holds U+FEFF has a non-zero entry
        on the diagonal.  ``weights`` other than None calls ``init_weights()`` first, as there.  ``device``: the HIP device of
        the launch (None: the current one); the distances, the negation and the transposition run there."""
        if weights is not None:
            self.init_weights()
        src, dst, alphabet = self.prepare(words)
        if not dst:
            return np.zeros((0, 0), dtype=np.float64)
        device = _lib.default_device(device)
        up = lambda a: torch.from_numpy(a).to(device)                      # noqa: E731
        src_chars, src_off = encode(src, alphabet)
        dst_chars, dst_off = encode(dst, alphabet)
        ins, dele, sub = self.tables(alphabet)
        dist = G.lev_matrix(up(src_chars), up(src_off), up(dst_chars), up(dst_off), up(ins), up(dele), up(sub),
                            max_len=max(len(w) for w in dst))              # [j, i]: lev(src[j] -> dst[i])
        return (-dist).t().contiguous().cpu().numpy()
