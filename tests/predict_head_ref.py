"""The per-word head in float64 numpy, written from the contract of gte_predict_head in include/gte.h -- not from the kernel.
Also the case table that the CPU test (against torch) and the GPU test (against this file) share, and the 1-ulp rule."""
import numpy as np

NS = (0, 1, 63, 64, 65, 257)
SHAPES = ((1, 1), (2, 2), (9, 9), (9, 12), (13, 16), (16, 16), (16, 19))        # (C, ld)
SCALES = (1.0, 30.0, 1e4)


def predict_head(logits):
    """logits float32 [n, C] -> (pred int64 [n], conf float64 [n], prob float64 [n, C]); the caller rounds to float32."""
    logits = np.asarray(logits, dtype=np.float32)
    n, c = logits.shape
    pred = np.zeros(n, dtype=np.int64)
    conf = np.zeros(n, dtype=np.float64)
    prob = np.zeros((n, c), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(n):
            row = logits[i]
            m, arg = row[0], 0
            for j in range(1, c):                       # the first maximum; a NaN beats every number and the first NaN stays
                if not np.isnan(m) and (row[j] > m or np.isnan(row[j])):
                    m, arg = row[j], j
            e = [np.exp(np.float64(row[j]) - np.float64(m)) for j in range(c)]
            s = np.float64(0.0)
            for j in range(c):                          # index order
                s = s + e[j]
            pred[i] = arg
            conf[i] = e[arg] / s
            for j in range(c):
                prob[i, j] = e[j] / s
    return pred, conf, prob


def special_rows(c):
    """The fixed rows of the case table for ``c`` classes, float32 [rows, c]."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    base = (np.arange(c, dtype=np.float32) * np.float32(0.37)) % np.float32(2.0) - np.float32(1.0)     # distinct-ish, in [-1, 1)
    rows = []
    rows.append(np.full(c, 0.75, dtype=np.float32))                                   # all equal
    r = base.copy(); r[0] = 5.0; rows.append(r)                                       # maximum at 0
    r = base.copy(); r[c - 1] = 5.0; rows.append(r)                                   # maximum at C-1
    r = base.copy(); r[0] = 5.0; r[c - 1] = 5.0; rows.append(r)                       # at both: the tie goes to 0
    r = base.copy(); r[c // 2] = -inf; rows.append(r)                                 # one -inf
    rows.append(np.full(c, -inf, dtype=np.float32))                                   # -inf only
    r = base.copy(); r[c // 2] = inf; rows.append(r)                                  # one +inf
    r = base.copy(); r[min(1, c - 1)] = nan; r[c - 1] = nan; rows.append(r)           # NaN at two places
    r = np.where(np.arange(c) % 2 == 0, np.float32(3.0e38), np.float32(-3.0e38)).astype(np.float32); rows.append(r)
    r = -r; rows.append(r)                                                            # +-3.0e38, either sign first
    return np.stack(rows)


def case_logits(n, c, seed):
    """float32 [n, c]: seeded normal rows scaled by 1, 30 and 1e4 in turn, with the special rows laid over rows 2 .. 11 (every n
    of the table from 63 up holds all of them; n = 0 and n = 1 are normal rows only)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c)).astype(np.float32)
    x *= np.asarray(SCALES, dtype=np.float32)[np.arange(n) % len(SCALES)][:, None]
    sp = special_rows(c)
    if n >= 3:
        k = min(len(sp), n - 2)                                                       # rows 0 and 1 stay normal
        x[2:2 + k] = sp[:k]
    return x


def cases():
    """Yields (n, C, ld, logits float32 [n, C]) over the whole table."""
    for a, n in enumerate(NS):
        for b, (c, ld) in enumerate(SHAPES):
            yield n, c, ld, case_logits(n, c, 1000 + 10 * a + b)


def assert_within_one_ulp(got, want64, what=""):
    """``got`` float32 against the float64 reference: NaN exactly where the reference has NaN; elsewhere float32(reference) or
    the float32 next to it."""
    got = np.asarray(got, dtype=np.float32)
    want64 = np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, what
    nan = np.isnan(want64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other places than the reference"
    with np.errstate(over="ignore", under="ignore"):
        want = want64.astype(np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    ok = nan | (got == want) | (got == lo) | (got == hi)
    assert ok.all(), f"{what}: {int((~ok).sum())} entries further than 1 ulp, first at {np.argwhere(~ok)[0].tolist()}: " \
                     f"{got[~ok][0]!r} vs {want[~ok][0]!r}"
