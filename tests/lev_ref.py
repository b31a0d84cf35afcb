"""Weighted Levenshtein distance in plain Python and numpy, written from the recurrence of gte_lev_matrix_f64 in include/gte.h:

    d[0][0] = 0;  d[i][0] = d[i-1][0] + del[a[i-1]];  d[0][j] = d[0][j-1] + ins[b[j-1]]
    d[i][j] = d[i-1][j-1]                                                          if a[i-1] == b[j-1]  (NO minimum is taken)
            = min(d[i-1][j] + del[a[i-1]], d[i][j-1] + ins[b[j-1]], d[i-1][j-1] + sub[a[i-1]][b[j-1]])   otherwise

Pinned on hand cases by tests/test_lev_ref_cpu.py; the oracle of the GPU tests.  Every cell is one of three float64 sums, each
rounded once, or a copy, so ``lev`` (one pair, Python floats) and ``matrix`` (all dst words at once, numpy) agree bit for bit with
each other and with any other evaluation of the recurrence.  ``lev_full_min`` is the OTHER rule (equal characters are a
substitution of cost 0 that competes in the minimum); it exists only to prove that test data tells the two rules apart."""
import json
import os

import numpy as np

BOM = "\ufeff"


class Costs:
    """Costs over characters: a default plus overrides.  ``ins`` / ``dele``: {character: cost}; ``sub``: {(from, to): cost}."""

    def __init__(self, ins=None, dele=None, sub=None, default=1.0):
        self.ins_, self.dele_, self.sub_, self.default = dict(ins or {}), dict(dele or {}), dict(sub or {}), float(default)

    def ins(self, ch):
        return self.ins_.get(ch, self.default)

    def dele(self, ch):
        return self.dele_.get(ch, self.default)

    def sub(self, a, b):
        return self.sub_.get((a, b), self.default)

    def dense(self, alphabet):
        """float64 tables over a list of characters: ins [A], dele [A], sub [A, A] (row: the character that is replaced)."""
        ins = np.array([self.ins(c) for c in alphabet], dtype=np.float64)
        dele = np.array([self.dele(c) for c in alphabet], dtype=np.float64)
        sub = np.array([[self.sub(a, b) for b in alphabet] for a in alphabet], dtype=np.float64).reshape(len(alphabet), len(alphabet))
        return ins, dele, sub


class Tables:
    """Costs over compact ids: the dense tables themselves."""

    def __init__(self, ins, dele, sub):
        self.ins_t, self.dele_t, self.sub_t = (np.asarray(t, dtype=np.float64) for t in (ins, dele, sub))

    def ins(self, c):
        return float(self.ins_t[c])

    def dele(self, c):
        return float(self.dele_t[c])

    def sub(self, a, b):
        return float(self.sub_t[a, b])


def uniform():
    return Costs()


def reference():
    """``LevenshteinSimilitudes.init_weights`` of the reference (src/components/tables/levenshtein.py:33-46)."""
    signs = {"%": 1.5, ".": 2.0, ",": 2.0}
    return Costs(ins=signs, dele=signs, sub={(".", ","): 1.9, (",", "."): 1.9, ("w", "x"): 1.9, ("x", "w"): 1.9, ("x", "%"): 5.0})


def _dp(a, b, costs, copy_on_equal):
    row = [0.0]
    for ch in b:
        row.append(row[-1] + costs.ins(ch))
    for x in a:
        new = [row[0] + costs.dele(x)]
        for j, y in enumerate(b, start=1):
            by_sub = row[j - 1] + (0.0 if x == y else costs.sub(x, y))
            if x == y and copy_on_equal:
                new.append(row[j - 1])
            else:
                new.append(min(row[j] + costs.dele(x), new[j - 1] + costs.ins(y), by_sub))
        row = new
    return row[-1]


def lev(a, b, costs):
    """lev(a -> b) of two sequences (strings, or sequences of ids with ``Tables``) by the recurrence above."""
    return _dp(a, b, costs, True)


def lev_full_min(a, b, costs):
    """The other rule: equal characters cost 0 as a substitution, and the minimum is taken all the same."""
    return _dp(a, b, costs, False)


def matrix_ids(src, dst, ins, dele, sub):
    """float64 [len(src), len(dst)]: lev(src[p] -> dst[q]) for words given as sequences of compact ids, all dst words at once."""
    ins, dele, sub = (np.asarray(t, dtype=np.float64) for t in (ins, dele, sub))
    n_dst = len(dst)
    out = np.zeros((len(src), n_dst), dtype=np.float64)
    if n_dst == 0 or len(src) == 0:
        return out
    len_b = np.array([len(w) for w in dst], dtype=np.int64)
    width = int(len_b.max())
    b = np.zeros((n_dst, max(width, 1)), dtype=np.int64)                   # padded with id 0: the padding is never read out
    for q, w in enumerate(dst):
        b[q, :len(w)] = np.asarray(w, dtype=np.int64)
    ins_b = ins[b]
    first = np.zeros((n_dst, width + 1), dtype=np.float64)
    for j in range(1, width + 1):
        first[:, j] = first[:, j - 1] + ins_b[:, j - 1]
    pick = np.arange(n_dst)
    for p, a in enumerate(src):
        row = first
        for x in a:
            x = int(x)
            equal, sub_x = b == x, sub[x][b]
            new = np.empty_like(row)
            new[:, 0] = row[:, 0] + dele[x]
            for j in range(1, width + 1):
                least = np.minimum(np.minimum(row[:, j] + dele[x], new[:, j - 1] + ins_b[:, j - 1]), row[:, j - 1] + sub_x[:, j - 1])
                new[:, j] = np.where(equal[:, j - 1], row[:, j - 1], least)
            row = new
        out[p] = row[pick, len_b]
    return out


def compact(costs, *word_lists):
    """(alphabet: the sorted characters of all words; the dense tables over it; every list as lists of compact ids)."""
    alphabet = sorted({ch for words in word_lists for w in words for ch in w})
    ids = {ch: k for k, ch in enumerate(alphabet)}
    return alphabet, costs.dense(alphabet), [[[ids[ch] for ch in w] for w in words] for words in word_lists]


def matrix(src, dst, costs):
    """float64 [len(src), len(dst)]: lev(src[p] -> dst[q]) for lists of strings under ``Costs``."""
    alphabet, tables, (src_ids, dst_ids) = compact(costs, src, dst)
    if not alphabet:
        return np.zeros((len(src), len(dst)), dtype=np.float64)
    return matrix_ids(src_ids, dst_ids, *tables)


def similarity(words, costs):
    """``calculate_similarity`` of the reference (levenshtein.py:50-63): m[i, j] = -lev(words[j] without U+FEFF -> words[i])."""
    words = [str(w) for w in words]
    return -matrix([w.replace(BOM, "") for w in words], words, costs).T


def golden():
    """tests/golden/lev_cases.json: hand cases under the reference's costs."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lev_cases.json")) as f:
        return json.load(f)
