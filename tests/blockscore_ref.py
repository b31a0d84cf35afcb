"""CPU reference of the block confidences (gte_block_scores of include/gte.h, postprocessing.block_scores), written from the
definition in float64; plain Python / numpy (it also runs where the GPU tests run).

  1. a word MEETS a block under the closed rectangle test of the block vote (tests/blocks_ref.py: meets), and counts in EVERY
     block of its page that it meets;
  2. p(word, k) = the softmax mass of the word's logit row on the classes whose bit is set in cat_classes[k] (a category
     outside the table: no class); 0 for a row that holds a non-finite logit -- such a row still counts as a word;
  3. n_words[j] = the words that meet block j; score[j] = the mean of p(word, category of j) over them, 1.0 where there is none
     (the constant the reference writes for every block, postprocessing_2.py:337).
The device forms p in fp32 and sums it in 2^-19 fixed point: within 2^-18 of this (tests/test_gpu_block_scores.py).

``Rule`` names the five choices of the definition; every field other than its default is a MUTANT that
tests/test_blockscore_ref_cpu.py shows to fail the hand case -- nothing else passes one."""
from typing import NamedTuple

import numpy as np

from tests.blocks_ref import meets


class Rule(NamedTuple):
    every_block: bool = True          # False: a word counts in its first block only (the vote's rule)
    closed: bool = True               # False: touching rectangles do not meet
    count_non_finite: bool = True     # False: a row with a non-finite logit is left out of n_words
    empty_score: float = 1.0          # the score of a block no word meets


def meets_open(word, block):
    if any(v != v for v in block):
        return False
    left, top = max(min(word[0], word[2]), min(block[0], block[2])), max(min(word[1], word[3]), min(block[1], block[3]))
    right, bottom = min(max(word[0], word[2]), max(block[0], block[2])), min(max(word[1], word[3]), max(block[1], block[3]))
    return left < right and top < bottom


def word_mass(row, mask):
    """Point 2 for one logit row (float64 softmax, max-subtracted) and one class mask."""
    row = np.asarray(row, dtype=np.float64)
    if not np.isfinite(row).all():
        return 0.0
    e = np.exp(row - row.max())
    return float(sum(e[c] for c in range(row.size) if (int(mask) >> c) & 1) / e.sum())


def score_page(bboxs, logits, blocks, cats, cat_classes, rule=Rule()):
    """One page -> (score [blocks] float64, n_words [blocks] int)."""
    words = [[int(v) for v in w] for w in np.asarray(bboxs).reshape(-1, 4).tolist()]
    blocks = [[float(v) for v in b] for b in np.asarray(blocks, dtype=np.float64).reshape(-1, 4).tolist()]
    logits = np.asarray(logits, dtype=np.float64).reshape(len(words), -1) if words else np.zeros((0, 1))
    masks = [int(cat_classes[int(k)]) if 0 <= int(k) < len(cat_classes) else 0 for k in cats]
    total, count = [0.0] * len(blocks), [0] * len(blocks)
    test = meets if rule.closed else meets_open
    for w, row in zip(words, logits):
        hits = [j for j, b in enumerate(blocks) if test(w, b)]
        for j in hits if rule.every_block else hits[:1]:
            if rule.count_non_finite or np.isfinite(row).all():
                total[j] += word_mass(row, masks[j])
                count[j] += 1
    return [t / c if c else rule.empty_score for t, c in zip(total, count)], count


def block_scores_ref(bbox, node_off, logits, block_box, block_off, block_cat, cat_classes, rule=Rule()):
    """The ABI's outputs for a batch: (score float64 [B], n_words int32 [B])."""
    bbox, block_box = np.asarray(bbox).reshape(-1, 4), np.asarray(block_box, dtype=np.float64).reshape(-1, 4)
    logits = np.asarray(logits)
    score, n_words = np.zeros(block_box.shape[0], dtype=np.float64), np.zeros(block_box.shape[0], dtype=np.int32)
    for p in range(len(node_off) - 1):
        n0, n1, b0, b1 = int(node_off[p]), int(node_off[p + 1]), int(block_off[p]), int(block_off[p + 1])
        s, c = score_page(bbox[n0:n1], logits[n0:n1], block_box[b0:b1], np.asarray(block_cat)[b0:b1], cat_classes, rule)
        score[b0:b1], n_words[b0:b1] = s, c
    return score, n_words


def block_scores_fast(bbox, node_off, logits, block_box, block_off, block_cat, cat_classes):
    """block_scores_ref in numpy (the same float64 definition, vectorised per page): for the pages of thousands of words that the
    device tests use.  tests/test_blockscore_ref_cpu.py compares the two."""
    bbox, block_box = np.asarray(bbox, dtype=np.int64).reshape(-1, 4), np.asarray(block_box, dtype=np.float64).reshape(-1, 4)
    logits, block_cat = np.asarray(logits, dtype=np.float64), np.asarray(block_cat, dtype=np.int64)
    n_cls = logits.shape[1]
    masks = np.asarray([int(m) for m in cat_classes], dtype=np.int64)
    score, n_words = np.ones(block_box.shape[0], dtype=np.float64), np.zeros(block_box.shape[0], dtype=np.int32)
    for p in range(len(node_off) - 1):
        n0, n1, b0, b1 = int(node_off[p]), int(node_off[p + 1]), int(block_off[p]), int(block_off[p + 1])
        if n1 == n0 or b1 == b0:
            continue
        w, b, z = bbox[n0:n1].astype(np.float64), block_box[b0:b1], logits[n0:n1]
        wlo, whi = np.minimum(w[:, :2], w[:, 2:]), np.maximum(w[:, :2], w[:, 2:])
        blo, bhi = np.minimum(b[:, :2], b[:, 2:]), np.maximum(b[:, :2], b[:, 2:])
        with np.errstate(invalid='ignore'):
            hit = ((blo[None, :, :] <= whi[:, None, :]) & (wlo[:, None, :] <= bhi[None, :, :])).all(axis=2) & ~np.isnan(b).any(axis=1)[None, :]
        ok = np.isfinite(z).all(axis=1)
        e = np.zeros_like(z)
        e[ok] = np.exp(z[ok] - z[ok].max(axis=1, keepdims=True))
        k = block_cat[b0:b1]
        mk = np.where((k >= 0) & (k < masks.size), masks[np.clip(k, 0, masks.size - 1)], 0)
        sel = ((mk[:, None] >> np.arange(n_cls)[None, :]) & 1).astype(np.float64)       # [blocks, classes]
        mass = np.zeros((n1 - n0, b1 - b0))
        mass[ok] = (e[ok] @ sel.T) / e[ok].sum(axis=1, keepdims=True)
        cnt = hit.sum(axis=0)
        n_words[b0:b1] = cnt
        score[b0:b1] = np.where(cnt > 0, (mass * hit).sum(axis=0) / np.maximum(cnt, 1), 1.0)
    return score, n_words
