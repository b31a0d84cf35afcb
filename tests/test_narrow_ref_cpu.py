"""tests/narrow_ref.py on a machine without a GPU: a float32 emulation of every kernel family's summation order (csrc/narrow_layer.hip)
stays inside the bounds on every bound case and is bit for bit the float64 reference on every exact case, and six mutants of the
emulation are rejected by the same checks.

Families: the plain kernels (an fma chain per lane, the xor butterfly of the wave, rows of a wave on one chain, the four waves added
through LDS, narrow_fold_kernel), the 32-row matrix-pipe forward (k-blocks of 8 on two accumulator chains), the 16-row one (one chain),
the matrix-pipe backward (32 rows per block on the accumulator chain of a workgroup, narrow_fold16_kernel).  A matrix-pipe
instruction is emulated as one fma per product it adds, in k order; an fma as the float64 sum of the exact product rounded to float32.

Every mutant is rejected by EVERY bound kind and by the exact case at every shape below (test_every_mutant_is_rejected asserts it
case by case), so no bound had to be tightened for its job.
"""
import numpy as np
import pytest

from tests import narrow_ref as nr

F32 = np.float32


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def add(a, b):
    return (np.asarray(a, F32) + np.asarray(b, F32)).astype(F32)


# ---- forward -------------------------------------------------------------------------------------------------------------------------
def emul_fwd(h, W, bias, f_true, width, mutant=None):
    """h [n, width] (zeros behind f_true), W [C, 2 f_true] -> t_self, t_neigh as the kernel of nr.fwd_family(width) sums them"""
    n, c = h.shape[0], W.shape[0]
    W = W.copy()
    if mutant == "swap":                                       # W_s and W_n swapped for the last class
        W[c - 1] = np.concatenate([W[c - 1, f_true:], W[c - 1, :f_true]])
    img = np.zeros((2, c, width), dtype=F32)                   # the weight image: columns behind f_true are zero
    img[0, :, :f_true], img[1, :, :f_true] = W[:, :f_true], W[:, f_true:]
    family = nr.fwd_family(width)
    drop = f_true - 1 if mutant == "drop_k" else -1            # the last true k term, in the last k-block
    out = []
    for seg in range(2):
        w = img[seg]
        if family == "fma":
            lanes = 64 * nr.nj(width)
            hv, wv = np.zeros((n, lanes), F32), np.zeros((c, lanes), F32)
            hv[:, :width], wv[:, :width] = h, w
            if drop >= 0:
                wv[:, drop] = 0
            a = np.zeros((n, c, 64), F32)
            for j in range(nr.nj(width)):                      # lane l owns k = l + 64 j
                a = fma(hv[:, None, 64 * j:64 * j + 64], wv[None, :, 64 * j:64 * j + 64], a)
            lane = np.arange(64)
            for off in (32, 16, 8, 4, 2, 1):
                a = add(a, a[:, :, lane ^ off])
            t = a[:, np.arange(c), np.arange(c)]               # lane c keeps class c
        else:
            step = lambda acc, k: acc if k == drop else fma(h[:, k, None], w[None, :, k], acc)
            if family == "mfma32":
                acc = [np.zeros((n, c), F32), np.zeros((n, c), F32)]
                for u in range(width // 8):
                    for t4 in range(4):                        # instruction t of block u adds k = 8 u + t and 8 u + 4 + t
                        acc[u & 1] = step(step(acc[u & 1], 8 * u + t4), 8 * u + 4 + t4)
                t = add(acc[0], acc[1])
            else:
                t = np.zeros((n, c), F32)
                for u in range(width // 16):
                    for t4 in range(4):
                        for kq in range(4):
                            t = step(t, 16 * u + 4 * kq + t4)
        if bias is not None and (seg == 0 or mutant == "bias_neigh"):
            t = add(t, bias[None, :])
        out.append(t)
    return out


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def fold16(p):
    """narrow_fold16_kernel over p [count, ...]"""
    count = p.shape[0]
    parts = []
    for sl in range(16):
        s0, s1 = np.zeros(p.shape[1:], F32), np.zeros(p.shape[1:], F32)
        b = sl
        while b + 16 < count:
            s0, s1 = add(s0, p[b]), add(s1, p[b + 16])
            b += 32
        if b < count:
            s0 = add(s0, p[b])
        parts.append(add(s0, s1))
    v = np.zeros(p.shape[1:], F32)
    for t in parts:
        v = add(v, t)
    return v


def fold4(p):
    """narrow_fold_kernel over p [count, ...]"""
    s = [np.zeros(p.shape[1:], F32) for _ in range(4)]
    for b in range(p.shape[0]):
        s[b % 4] = add(s[b % 4], p[b])
    return add(add(add(s[0], s[1]), s[2]), s[3])


def emul_bwd(dl, q, h, W, alpha, f_true, width, cus, ln=False, mutant=None):
    """-> dh [n, f_true], dW [C, 2 f_true], dbias [C] as the kernel of nr.bwd_family(width) sums them"""
    n, c = dl.shape
    a = F32(alpha)
    D = (dl * a).astype(F32)
    Q = q.astype(F32) if mutant == "alpha_dl_only" else (q * a).astype(F32)
    ws, wn = W[:, :f_true], W[:, f_true:]
    ht = h[:, :f_true]
    DQ = np.concatenate([D, Q], axis=1)                        # [n, 2 C]
    rows = list(range(n)) + ([n - 1] if mutant == "clamp_leak" else [])      # row n - 1 counted twice
    # dh: one chain per element; the matrix-pipe kernel interleaves nothing else (kk = 0 .. NCT-1 are dl's classes, then q's)
    dh = np.zeros((n, f_true), F32)
    cl = range(c - 1) if mutant == "dh_miss_class" else range(c)
    if nr.bwd_family(width) == "fma":
        for cc in cl:
            dh = fma(Q[:, cc, None], wn[None, cc, :], fma(D[:, cc, None], ws[None, cc, :], dh))
        grid = nr.bwd_grid(n, width, cus)
        slots = 4 * grid
        acc, gb = np.zeros((slots, 2 * c, f_true), F32), np.zeros((slots, c), F32)
        for r in rows:                                         # wave (r % slots) takes its rows in order
            s = r % slots
            acc[s] = fma(DQ[r, :, None], ht[r, None, :], acc[s])
            gb[s] = add(gb[s], D[r])
        acc, gb = acc.reshape(grid, 4, 2 * c, f_true), gb.reshape(grid, 4, c)
        part, pb = acc[:, 0], gb[:, 0]
        for w in range(1, 4):
            part, pb = add(part, acc[:, w]), add(pb, gb[:, w])
        dW2, db = fold4(part), fold4(pb)
    else:
        for cc in cl:
            dh = fma(D[:, cc, None], ws[None, cc, :], dh)
        for cc in cl:
            dh = fma(Q[:, cc, None], wn[None, cc, :], dh)
        grid = nr.bwd_grid(n, width, cus, ln)
        acc, gb = np.zeros((grid, 2 * c, f_true), F32), np.zeros((grid, c), F32)
        for r in rows:                                         # workgroup g walks the row blocks g, g + grid, ...
            g = (r // 32) % grid
            acc[g] = fma(DQ[r, :, None], ht[r, None, :], acc[g])
            gb[g] = add(gb[g], D[r])
        dW2, db = fold16(acc), fold16(gb)
    return dh, np.concatenate([dW2[:c], dW2[c:]], axis=1), db


# ---- the checks both the emulation and its mutants go through --------------------------------------------------------------------------
CUS = 4                                                        # a small device: the matrix-pipe backward walks several row blocks
# (n, f, n_pad or None, c): one shape per family
SHAPES = [(77, 13, None, 5), (70, 100, None, 9), (37, 250, None, 16), (77, 24, None, 8), (129, 48, None, 12), (300, 64, None, 9),
          (97, 100, 112, 9), (45, 5, 16, 4)]
ALPHA = {"exact": 0.25, "scales": 0.37, "cancel": 1.7, "gauss": 0.013}


def cases(n, f, c):
    return [nr.exact_case(n, f, c)] + nr.bound_cases(n, f, c)


def fwd_ok(case, n_pad, mutant=None):
    width = n_pad or case.f
    h = case.padded(n_pad) if n_pad else case.h
    ts, tn = emul_fwd(h, case.W, case.bias, case.f, width, mutant)
    rs, rn = nr.fwd(h, case.W, case.bias, case.f)
    if case.exact:
        return nr.same_bits(ts, nr.exact32(rs)) and nr.same_bits(tn, nr.exact32(rn))
    bs, bn = nr.fwd_bound(h, case.W, case.bias, case.f, width)
    return nr.ratio(ts, rs, bs) <= 1.0 and nr.ratio(tn, rn, bn) <= 1.0


def bwd_ok(case, n_pad, mutant=None):
    width = n_pad or case.f
    al = ALPHA[case.kind]
    got = emul_bwd(case.dl, case.q, case.h, case.W, al, case.f, width, CUS, bool(n_pad), mutant)
    ref = nr.bwd(case.dl, case.q, case.h, case.W, al)
    if case.exact:
        return all(nr.same_bits(g, nr.exact32(r)) for g, r in zip(got, ref))
    bnd = nr.bwd_bound(case.dl, case.q, case.h, case.W, nr.dw_chain(case.n, width, CUS, ln=bool(n_pad)), al)
    return all(nr.ratio(g, r, b) <= 1.0 for g, r, b in zip(got, ref, bnd))


@pytest.mark.parametrize("n,f,n_pad,c", SHAPES)
def test_the_emulation_is_inside_the_bounds_and_bitwise_on_exact_cases(n, f, n_pad, c):
    for case in cases(n, f, c):
        assert fwd_ok(case, n_pad), f"forward {case.kind}"
        assert bwd_ok(case, n_pad), f"backward {case.kind}"


FWD_MUTANTS = ["drop_k", "swap", "bias_neigh"]
BWD_MUTANTS = ["clamp_leak", "dh_miss_class", "alpha_dl_only"]


@pytest.mark.parametrize("mutant", FWD_MUTANTS + BWD_MUTANTS)
def test_every_mutant_is_rejected(mutant):
    ok = fwd_ok if mutant in FWD_MUTANTS else bwd_ok
    for n, f, n_pad, c in SHAPES:
        for case in cases(n, f, c):
            assert not ok(case, n_pad, mutant), f"{mutant} survived the {case.kind} case at n={n} f={f} n_pad={n_pad} c={c}"


def test_chain_lengths_are_no_looser_than_any_order():
    for f in range(1, 257):
        assert nr.fwd_chain(f) <= f
    for n in (1, 31, 77, 2055, 24495, 262221):
        for f in (13, 256):
            for ln in (False, True):
                assert nr.dw_chain(n, f, 256, ln) <= n
    # the instantiation tables of the dispatch
    assert [nr.nct(c) for c in (1, 4, 5, 8, 9, 12, 13, 16)] == [4, 4, 8, 8, 12, 12, 16, 16]
    assert [nr.nctm(c) for c in (4, 5, 8, 9, 12, 13)] == [4, 8, 8, 16, 16, 16]
    assert [nr.fwd_family(f) for f in (13, 24, 48)] == ["fma", "mfma32", "mfma16"]
    assert all(f % 8 == 0 and f % 16 for f in nr.MFMA32_WIDTHS) and all(f % 16 == 0 for f in nr.MFMA16_WIDTHS)
    assert sorted({f % 4 for f, _ in nr.PADDED}) == [0, 1, 2, 3] and all(p % 16 == 0 and f < p for f, p in nr.PADDED)


def test_out3_and_alpha_follow_ce_fold():
    p = nr.exact_partials(129, 3)
    assert p.shape == (3, 3) and nr.alpha(p, 2.0) == F32(0.25)
    o = nr.out3(p)
    assert o.dtype == np.float32 and o[1] == 8.0 and o[0] == F32(p[:, 0].astype(np.float64).sum() / 8.0) and o[2] == p[:, 2].sum()
    z = np.zeros((2, 3), F32)
    assert nr.alpha(z, 1.0) == 0.0 and nr.out3(z)[0] == 0.0                      # no weight: loss 0, alpha 0
    pb = nr.bound_partials(1000)
    assert nr.alpha(pb, 0.37) == F32(F32(0.37) / F32(pb[:, 1].astype(np.float64).sum()))
