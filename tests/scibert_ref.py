"""Token pooling in float32 numpy, written from the contract of gte_token_pool_f32 in include/gte.h, and the reference's padded page
batch with its modified mask (the host rule of ``SciBERT.token_ids``).  Pinned against the reference's recorded outputs by
tests/test_scibert_ref_cpu.py; the oracle of the GPU tests.

Every operation is an elementwise numpy operation on float32 arrays, rounded once: the rows are added one position at a time in
position order, so nothing depends on numpy's reduction order."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scibert_cases.json")


def golden():
    with open(GOLDEN) as f:
        data = json.load(f)
    for key in ("embeddings", "normalized"):
        data[key] = np.asarray(data[key], dtype=np.float32)
    for page in data["pages"]:
        for key in ("mean", "max"):
            page[key] = np.asarray(page[key], dtype=np.float32).reshape(len(page["words"]), -1)
    return data


def pool(tok, table, mode):
    """float32 [n, D]: mode 'mean' or 'max' of the table rows that the ids of ``tok`` [n, W] name; ids outside [0, V) are skipped."""
    tok = np.asarray(tok, dtype=np.int64)
    table = np.asarray(table, dtype=np.float32)
    n, v, d = tok.shape[0], table.shape[0], table.shape[1]
    acc = np.zeros((n, d), dtype=np.float32)
    count = np.zeros(n, dtype=np.int64)
    for j in range(tok.shape[1]):
        part = (tok[:, j] >= 0) & (tok[:, j] < v)
        if not part.any():
            continue
        x = table[tok[part, j]]
        if mode == "mean":
            acc[part] = acc[part] + x                                    # float32 + float32, rounded once
        else:
            acc[part] = np.where(x > acc[part], x, acc[part])
        count += part
    if mode == "mean":
        has = count > 0
        acc[has] = acc[has] / count[has].astype(np.float32)[:, None]     # float32 / float32: correctly rounded
    assert acc.dtype == np.float32
    return acc


def mean_bound(tok, table, recorded):
    """Per element, the gap that two float32 summation orders of the c terms plus the final rounding can open between a mean
    and ``recorded``: 2^-23 * ((c - 1) / c * sum_j |x_j| + |recorded|)."""
    tok = np.asarray(tok, dtype=np.int64)
    table = np.asarray(table, dtype=np.float64)
    part = (tok >= 0) & (tok < table.shape[0])
    mags = (np.abs(table)[np.where(part, tok, 0)] * part[:, :, None]).sum(axis=1)
    c = np.maximum(part.sum(axis=1), 1)[:, None].astype(np.float64)
    return 2.0 ** -23 * ((c - 1) / c * mags + np.abs(np.asarray(recorded, dtype=np.float64)))


def page_rows(pieces, cls, sep, pad):
    """The reference's batch of one page, from the pieces of its words (each already cut to max_length - 2):
    (input_ids [n, L], mask [n, L]) with L = 2 + the largest number of pieces.  Row i is ``cls pieces_i sep pad ..``; the mask is 1
    on the first len_i = m_i + 2 columns, and then column 0 and column L - 1 of the page are cleared."""
    length = 2 + max(len(p) for p in pieces)
    ids = np.full((len(pieces), length), pad, dtype=np.int64)
    mask = np.zeros((len(pieces), length), dtype=np.int64)
    for i, p in enumerate(pieces):
        row = [cls] + list(p) + [sep]
        ids[i, :len(row)] = row
        mask[i, :len(row)] = 1
    mask[:, 0] = 0
    mask[:, -1] = 0
    return ids, mask


def page_ids(pieces, cls, sep, pad, width):
    """int32 [n, width]: positions 1 .. width of the reference's rows, -1 where the modified mask is 0 or the row has ended."""
    out = np.full((len(pieces), width), -1, dtype=np.int32)
    if len(pieces):
        ids, mask = page_rows(pieces, cls, sep, pad)
        held = np.where(mask == 1, ids, -1)[:, 1:1 + width]
        out[:, :held.shape[1]] = held
    return out
