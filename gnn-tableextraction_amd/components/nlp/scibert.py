"""SCIBERT embedder on the device: the interface of the reference's ``SciBERT`` (src/components/nlp/scibert.py:13-160:
``_online_batch_(bboxs, texts, titles)``, called per batch through ``_generate_features`` at src/models/model_train.py:293).  The
reference never runs the transformer: it row-normalises the model's input-embedding matrix once, looks up the WordPiece ids of every
word and pools the rows under a mask.  Its artefacts are a vocabulary and one [V, D] float matrix.

Host side: only the string work -- the BERT tokeniser and the page-dependent mask (``SciBERT.token_ids``).  The gather and the
reduction run in csrc/token_pool.hip, ONE launch of gte_token_pool_f32 for all pages where the reference runs an embedding lookup
to [n_p, L, D], a masked product and a reduction per page.

The tokeniser restates, with ``unicodedata`` and ``re``, what the ``transformers`` / ``tokenizers`` libraries DO on the recorded
corpus (tests/golden/scibert_cases.json, written by tools/make_scibert_golden.py with transformers 5.15.0 / tokenizers 0.22.2);
neither library is needed at run time.  In the order the library applies them:
  1. the literal texts of the special tokens (``[PAD] [UNK] [CLS] [SEP] [MASK]``, those the vocabulary holds) are cut out of the raw
     word wherever they stand and become their ids as they are; only the text between them goes through 2 - 5;
  2. cleaning: U+0000, U+FFFD and the characters of the categories Cc, Cf and Co other than tab, line feed and carriage return
     are dropped (U+0085 and U+001C among them, so they do NOT split a word); tab, line feed, carriage return and the characters
     with the White_Space property that are left become a space;
  3. a space is put on both sides of every CJK ideograph;
  4. with ``do_lower_case``: NFD, the marks of category Mn dropped, then every character lower-cased on its own (a capital sigma
     at the end of a word becomes the ordinary small sigma, not the final one);
  5. the text is split at spaces, every punctuation character (ASCII punctuation or a category P*) is a piece of its own, and
     every piece goes through greedy longest-match WordPiece with ``##``: a piece of more than 100 characters, or one with a
     stretch that matches nothing, is ``[UNK]`` as a whole.
"""
from __future__ import annotations

import json
import os
import re
import unicodedata
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from ... import graph as G

REQUIRED = ("[UNK]", "[CLS]", "[SEP]", "[PAD]")
SPECIAL = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")
MAX_PIECE_CHARS = 100
# the characters with the Unicode White_Space property that cleaning has not dropped (U+0009 .. U+000D, U+0085 are Cc: tab, line feed and
# carriage return are kept by name, the others dropped)
_SPACES = frozenset("\t\n\r \xa0\u1680\u2028\u2029\u202f\u205f\u3000" + "".join(chr(c) for c in range(0x2000, 0x200B)))
_ASCII_PUNCT = frozenset("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~")
_CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF),
        (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def _is_cjk(ch: str) -> bool:
    cp = ord(ch)
    return any(lo <= cp <= hi for lo, hi in _CJK)


def _is_punct(ch: str) -> bool:
    return ch in _ASCII_PUNCT or unicodedata.category(ch).startswith("P")


def normalise(text: str, do_lower_case: bool = True) -> str:
    """Steps 2 - 4 of the module docstring."""
    out = []
    for ch in text:
        if ch in _SPACES:
            out.append(" ")
        elif ch == "\x00" or ch == "\ufffd" or unicodedata.category(ch) in ("Cc", "Cf", "Co"):
            continue
        elif _is_cjk(ch):
            out.append(" " + ch + " ")
        else:
            out.append(ch)
    text = "".join(out)
    if do_lower_case:
        text = "".join(ch for ch in unicodedata.normalize("NFD", text) if unicodedata.category(ch) != "Mn")
        text = "".join(ch.lower() for ch in text)
    return text


def split_pieces(text: str) -> List[str]:
    """Step 5, first half: the pieces of a normalised text -- split at spaces, every punctuation character on its own."""
    pieces, cur = [], []
    for ch in text:
        if ch == " " or _is_punct(ch):
            if cur:
                pieces.append("".join(cur))
                cur = []
            if ch != " ":
                pieces.append(ch)
        else:
            cur.append(ch)
    if cur:
        pieces.append("".join(cur))
    return pieces


class SciBERT:
    """Drop-in for the reference's SCIBERT embedder: ``SciBERT(vocab, embeddings, device)(bboxs, texts, titles) ->
    List[Tensor[n_p, D]]``, the reference's list of one tensor per page.  A page without words yields a [0, D] tensor (the reference
    raises there).

    ``vocab``: the tokens in id order, or a token -> id mapping, with ``[UNK]``, ``[CLS]``, ``[SEP]`` and ``[PAD]``; ``embeddings``
    float [V, D]: the model's input-embedding matrix (``model.get_input_embeddings().weight``).  It is uploaded once as float32 and
    row-normalised on the device with ``torch.nn.functional.normalize`` (p = 2, eps 1e-12: scibert.py:46); ``normalized=True`` takes a
    table that is normalised already.  ``pooling`` 'mean' or 'max' (``specifics.pooling``); ``max_length`` 16 in the reference.
    A vocabulary without ``[MASK]`` does not treat that text as a special token (the library would give it the id V, which names no
    row of the table)."""

    def __init__(self, vocab, embeddings, device="cuda:0", pooling: str = "mean", do_lower_case: bool = True, max_length: int = 16,
                 normalized: bool = False):
        self.vocab: Dict[str, int] = {t: int(i) for t, i in vocab.items()} if hasattr(vocab, "items") else \
            {t: i for i, t in enumerate(vocab)}
        missing = [t for t in REQUIRED if t not in self.vocab]
        if missing:
            raise ValueError(f"SciBERT: vocab has no {', '.join(missing)} entry")
        if pooling not in ("mean", "max"):
            raise ValueError(f"SciBERT: pooling must be 'mean' or 'max', got {pooling!r}")
        if not isinstance(max_length, int) or not 3 <= max_length <= 33:
            raise ValueError(f"SciBERT: max_length must be an integer in 3 .. 33, got {max_length!r}")
        table = embeddings.detach().cpu() if isinstance(embeddings, torch.Tensor) else torch.from_numpy(np.asarray(embeddings))
        n_ids = max(self.vocab.values()) + 1
        if table.dim() != 2 or not table.is_floating_point() or table.shape[0] != n_ids or min(self.vocab.values()) < 0:
            raise ValueError(f"SciBERT: embeddings must be a float matrix with one row per vocabulary id [{n_ids}, D], got "
                             f"{table.dtype} {tuple(table.shape)}")
        self.pooling, self.do_lower_case, self.max_length = pooling, bool(do_lower_case), max_length
        self.width = max_length - 1                          # positions 1 .. max_length - 1 of the reference's row
        self.unk, self.sep = self.vocab["[UNK]"], self.vocab["[SEP]"]
        specials = [t for t in SPECIAL if t in self.vocab]
        self._special = re.compile("(" + "|".join(re.escape(t) for t in specials) + ")")
        self._memo: Dict[str, Tuple[int, ...]] = {}
        self.device = torch.device(device)
        self.n_vocab, self.n_out = int(table.shape[0]), int(table.shape[1])
        table = table.to(torch.float32).to(self.device)
        self.table = (table if normalized else torch.nn.functional.normalize(table)).contiguous()

    @classmethod
    def from_model_dir(cls, path, device="cuda:0", pooling: str = "mean", max_length: int = 16) -> "SciBERT":
        """From a local model directory, what the reference's ``from_pretrained(model_path, local_files_only=True)`` reads:
        ``vocab.txt`` (one token per line, the line number is the id), ``do_lower_case`` from ``tokenizer_config.json`` where that
        file states it (True otherwise) and the tensor whose key ends in ``word_embeddings.weight`` from ``pytorch_model.bin``
        (``torch.load(..., weights_only=True)``), or from ``model.safetensors`` if the ``safetensors`` library imports.  Nothing
        outside ``path`` is read."""
        path = os.fspath(path)
        with open(os.path.join(path, "vocab.txt"), encoding="utf-8") as f:
            vocab = [line.rstrip("\n") for line in f]
        do_lower_case = True
        config = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(config):
            with open(config, encoding="utf-8") as f:
                do_lower_case = bool(json.load(f).get("do_lower_case", True))
        weights = None
        if os.path.exists(os.path.join(path, "pytorch_model.bin")):
            weights = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        elif os.path.exists(os.path.join(path, "model.safetensors")):
            try:
                from safetensors.torch import load_file
            except ImportError as e:
                raise ValueError(f"SciBERT: path {path!r} holds model.safetensors only and the safetensors library is missing") from e
            weights = load_file(os.path.join(path, "model.safetensors"), device="cpu")
        if weights is None:
            raise ValueError(f"SciBERT: path {path!r} holds neither pytorch_model.bin nor model.safetensors")
        keys = [k for k in weights if k.endswith("word_embeddings.weight")]
        if len(keys) != 1:
            raise ValueError(f"SciBERT: path {path!r}: {len(keys)} tensors end in 'word_embeddings.weight' (one expected)")
        return cls(vocab, weights[keys[0]], device=device, pooling=pooling, do_lower_case=do_lower_case, max_length=max_length)

    # ---- the tokeniser ----------------------------------------------------------------------------------------------------
    def wordpiece(self, piece: str) -> List[int]:
        if len(piece) > MAX_PIECE_CHARS:
            return [self.unk]
        ids, start = [], 0
        while start < len(piece):
            end = len(piece)
            while end > start:
                i = self.vocab.get(("##" if start else "") + piece[start:end])
                if i is not None:
                    break
                end -= 1
            if end == start:
                return [self.unk]                            # a stretch that matches nothing: the whole piece
            ids.append(i)
            start = end
        return ids

    def tokenize(self, text: str) -> List[int]:
        """The WordPiece ids of one text, without ``[CLS]`` / ``[SEP]`` and without truncation."""
        ids = []
        for k, part in enumerate(self._special.split(text)):
            if k % 2:
                ids.append(self.vocab[part])
            else:
                for piece in split_pieces(normalise(part, self.do_lower_case)):
                    ids.extend(self.wordpiece(piece))
        return ids

    def word_ids(self, word: str) -> Tuple[int, ...]:
        """The ids that the reference's row holds between ``[CLS]`` and ``[SEP]`` for one word: the word without its ASCII spaces
        (scibert.py:72), cut to ``max_length - 2`` pieces.  Memoised per distinct word: pages repeat their words heavily."""
        word = "".join(word.split(" "))
        got = self._memo.get(word)
        if got is None:
            got = self._memo[word] = tuple(self.tokenize(word)[:self.max_length - 2])
        return got

    def token_ids(self, page_texts) -> np.ndarray:
        """int32 [sum n_p, max_length - 1]: positions 1 .. max_length - 1 of the reference's padded row of every word, with -1
        wherever the reference's modified mask is 0 (position 0, ``[CLS]``, is always masked and is left out).  A word of m pieces
        is ``[CLS] p_1 .. p_m [SEP]`` padded to the page's longest row, L = 2 + the page's largest m; the reference then clears
        the mask of column 0 and of column L - 1 of the PAGE (scibert.py:149-150), not of each word's ``[SEP]``.  So a word takes part
        with its pieces and, unless it is among the page's longest, with its ``[SEP]``; an empty word beside longer ones with
        ``[SEP]`` alone; a page of empty words only with nothing."""
        rows = []
        for words in page_texts:
            ids = [self.word_ids(w) for w in words]
            page = np.full((len(ids), self.width), -1, dtype=np.int32)
            longest = max((len(i) for i in ids), default=0)
            for r, i in enumerate(ids):
                row = (i + (self.sep,))[:longest]            # columns 1 .. L - 2 of the reference's row: L - 1 is masked
                page[r, :len(row)] = row
            rows.append(page)
        return np.concatenate(rows) if rows else np.zeros((0, self.width), dtype=np.int32)

    # ---- the embedder -----------------------------------------------------------------------------------------------------
    def features(self, page_texts, out=None, row_map=None) -> torch.Tensor:
        """All pages at once: float32 [sum n_p, D] on the device, one launch.  ``out`` / ``row_map``: as graph.token_pool."""
        tok = torch.from_numpy(self.token_ids(page_texts)).to(self.device)
        return G.token_pool(tok, self.table, mode=self.pooling, row_map=row_map, out=out)

    def _online_batch_(self, bboxs, texts, titles=None):
        return self.__call__(bboxs, texts, titles)

    def __call__(self, bboxs, texts, titles=None, split=None):
        texts = texts if isinstance(texts, list) else [texts]
        feats = self.features(texts)
        return list(torch.split(feats, [len(t) for t in texts]))
