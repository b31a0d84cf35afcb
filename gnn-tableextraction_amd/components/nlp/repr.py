"""REPR embedder on the device: the interface of the reference's ``Repr`` (src/components/nlp/repr.py:30-143:
``_online_batch_(bboxs, texts, titles)``, called per batch through ``_generate_features`` at src/models/model_train.py:293), with
the tensor expansion per page and the Python assignment per word replaced by ONE launch of gte_repr_features over all pages.

Host side: only the string work -- the normaliser, the whitespace split and the dictionary lookup (``Repr.token_ids``).
Everything arithmetic -- the float64 distances to the prototypes, the clamped inverse-distance weights, the first-index arg-max
and the row copy (or the float32 mix of ``combined=True``) -- runs in csrc/repr_features.hip.

The normaliser restates the reference's ``CustomNormalizer`` (repr.py:21-28) with ``unicodedata`` and ``re``: the ``tokenizers``
library is not needed.  What is restated is what that library DOES with the reference's six steps (recorded with tokenizers
0.22.2 in tests/golden/repr_cases.json by tools/make_repr_golden.py): NFKC, digit -> ``x`` and letter -> ``w``, ``x+`` -> ``x``,
``w+`` -> ``w``.  The fifth step's pattern (a look-behind that holds a group) is rejected by the library's regex engine and
``encode`` carries on with what the first four steps produced, so the fifth step and the ``lowercase`` behind it have NO effect:
``-5`` stays ``-x``, a Greek capital omega followed by ``-7`` becomes ``w-x``."""
from __future__ import annotations

import os
import pickle
import re
import unicodedata
from typing import List, Sequence

import numpy as np
import torch

from ... import graph as G

UNK = "<UNK_W>"
# the pre-tokeniser splits where the library's WhitespaceSplit does: at characters with the Unicode White_Space property.
# str.split() would also split at U+001C .. U+001F, which that property does not hold.
_WHITE_SPACE = "\t\n\x0b\x0c\r \x85\xa0\u1680\u2000-\u200a\u2028\u2029\u202f\u205f\u3000"
_SPLIT = re.compile(f"[^{_WHITE_SPACE}]+")
_XS, _WS = re.compile("x+"), re.compile("w+")


def normalise(text: str) -> str:
    """The effective steps of the reference's normaliser (see the module docstring): NFKC; every digit (``str.isdigit``) ->
    ``x``, every other letter (``str.isalpha``) -> ``w``; runs of ``x`` and of ``w`` collapsed to one."""
    text = unicodedata.normalize("NFKC", text)
    text = "".join("x" if ch.isdigit() else "w" if ch.isalpha() else ch for ch in text)
    return _WS.sub("w", _XS.sub("x", text))


def page_tokens(words: Sequence[str]) -> List[str]:
    """The normalised tokens of one page (repr.py:103-106): every word loses its ASCII spaces, the words are joined with one
    space, the string is normalised and split at whitespace."""
    joined = " ".join("".join(w.split(" ")) for w in words)
    return _SPLIT.findall(normalise(joined))


class Repr:
    """Drop-in for the reference's REPR embedder: ``Repr(repr2idx, embeddings, prototypes, i_embedding, device)(bboxs, texts,
    titles) -> List[Tensor[n_p, P]]``.  The reference returns one padded tensor [pages, longest page, P]; the first n_p rows of
    its page i are the same values.  Where the reference raises because the longest page has fewer tokens than words, the rows
    without a token are zero here.

    ``repr2idx``: normalised token -> id, with ``"<UNK_W>"`` (``ValueError`` without it: the reference fails only once it meets
    an unknown word); ``embeddings`` float64 [V, D]; ``prototypes`` float64 [C, D]; ``i_embedding`` float64 [C, P] (the reference:
    C = 47, P = 50).  The arrays are uploaded once."""

    def __init__(self, repr2idx, embeddings, prototypes, i_embedding, device="cuda:0", alpha: float = 1.0):
        if UNK not in repr2idx:
            raise ValueError(f"Repr: repr2idx has no {UNK!r} entry: unknown tokens could not be looked up")
        self.repr2idx = dict(repr2idx)
        self.unk = int(self.repr2idx[UNK])
        emb, cen, ipr = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (embeddings, prototypes, i_embedding))
        if emb.ndim != 2 or cen.ndim != 2 or ipr.ndim != 2 or cen.shape[1] != emb.shape[1] or ipr.shape[0] != cen.shape[0]:
            raise ValueError(f"Repr: embeddings {emb.shape}, prototypes {cen.shape} and i_embedding {ipr.shape} do not fit together "
                             f"([V, D], [C, D], [C, P])")
        self.device = torch.device(device)
        self.alpha = float(alpha)
        self.n_vocab, self.n_out = emb.shape[0], ipr.shape[1]
        self.embeddings, self.centers, self.i_prototypes = (torch.from_numpy(a).to(self.device) for a in (emb, cen, ipr))

    @classmethod
    def from_reference_files(cls, tables_preprocess_dir, repr_pts_dir, run_name, epoch_no, centroids_no, alpha_no, component_no,
                             top_k, device="cuda:0", alpha: float = 1.0) -> "Repr":
        """From the pickles that the reference's ``inizialize`` reads (repr.py:53-61), with the keys it takes from them:
        ``<repr_pts_dir>/<run_name>/trained_prototypes_epoch<epoch_no>_<centroids_no>_<alpha_no>.dat`` (``'prototypes'``,
        ``'i_embedding'``), ``<tables_preprocess_dir>/embed-repr-<centroids_no>-<component_no>-<top_k>.dat`` (``'embeddings'``)
        and ``<tables_preprocess_dir>/repr2idx.dat`` (the dictionary)."""
        def load(*parts):
            with open(os.path.join(*[str(p) for p in parts]), "rb") as f:
                return pickle.load(f)
        train = load(repr_pts_dir, run_name, f"trained_prototypes_epoch{epoch_no}_{centroids_no}_{alpha_no}.dat")
        embed = load(tables_preprocess_dir, f"embed-repr-{centroids_no}-{component_no}-{top_k}.dat")
        repr2idx = load(tables_preprocess_dir, "repr2idx.dat")
        return cls(repr2idx, embed["embeddings"], train["prototypes"], train["i_embedding"], device=device, alpha=alpha)

    def token_ids(self, page_texts) -> np.ndarray:
        """int32 [sum n_p]: the token id of every node, -1 for "no token" (repr.py:103-106 and the alignment of
        graphs/utils.py:22-23).  Token j of a page belongs to node j: surplus tokens are dropped, nodes beyond the last token get
        -1 (the zero padding of repr.py:136-139).  An EMPTY word (or one of whitespace only) yields no token, so all later words
        of its page take the token of their successor: that is the reference's behaviour and is kept.  Unknown tokens map to
        the id of ``"<UNK_W>"``.  A page with any token id outside [0, V) falls back to ``embeddings[0]`` as a whole
        (repr.py:120-123): every token id of that page becomes 0."""
        out = []
        for words in page_texts:
            ids = [self.repr2idx.get(t, self.unk) for t in page_tokens(words)]
            if any(not 0 <= i < self.n_vocab for i in ids):
                ids = [0] * len(ids)
            n = len(words)
            out.append(np.asarray(ids[:n] + [-1] * (n - len(ids)), dtype=np.int32))
        return np.concatenate(out) if out else np.zeros(0, dtype=np.int32)

    def features(self, page_texts, combined: bool = False, out=None) -> torch.Tensor:
        """All pages at once: float32 [sum n_p, P] on the device, one launch."""
        tok = torch.from_numpy(self.token_ids(page_texts)).to(self.device)
        return G.repr_features(tok, self.embeddings, self.centers, self.i_prototypes, alpha=self.alpha, combined=combined, out=out)

    def _online_batch_(self, bboxs, texts, titles=None):
        return self.__call__(bboxs, texts, titles)

    def __call__(self, bboxs, texts, titles=None, split=None, combined: bool = False):
        feats = self.features(texts, combined=combined)
        return list(torch.split(feats, [len(t) for t in texts]))
