"""gte_token_pool_f32 against tests/scibert_ref.py (float32 numpy with sequential adds, pinned on the reference's recorded outputs
by tests/test_scibert_ref_cpu.py): EQUAL by value in both modes -- the kernel and the oracle perform the same float32 operations in
the same order.

Every case runs through both access forms (16-byte where the table, dim, out and ldo allow it, dword otherwise: which one a call
takes is read from gte_token_pool_access_bytes and asserted) into a sentinel-filled buffer wider and longer than the result, and
every element outside the named row slices must keep the sentinel.  Shapes: D = 768 (three chunks of a wave in the 16-byte form,
twelve in the dword form), 12 (three lanes), 5 (dword only), 260 (a chunk plus one lane); width 15 and 1; words with 0, 1 and 15 ids
that take part; ids -1, V, V + 7 and INT32_MAX mixed in; 0, 1, 7 and 300 words, and more than the 2048 workgroups x 4 words of one
pass of the grid at D = 8."""
import ctypes

import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from tests import scibert_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = 50
SENTINEL = -12345.5
INT32_MAX = 2 ** 31 - 1
MODES = ("mean", "max")


def make_case(n, width, d, seed):
    rng = np.random.default_rng(seed)
    table = rng.normal(size=(V, d)).astype(np.float32)
    table[3] = -np.abs(table[3])                                         # a row below zero everywhere: max gives 0 for it alone
    table[4, 0] = 1e8                                                    # order matters in float32: (1e8 + x) - 1e8 != x
    table[5, 0] = -1e8
    table[7, 0] = 3.0                                                    # (1e8 + 3) - 1e8 = 0, (1e8 - 1e8) + 3 = 3
    tok = rng.integers(0, V, size=(n, width)).astype(np.int32)
    fill = rng.random((n, width))
    tok[fill < 0.45] = -1                                                # the masked positions, anywhere in the row
    tok[(fill >= 0.45) & (fill < 0.50)] = V                              # ids that name no row
    tok[(fill >= 0.50) & (fill < 0.53)] = V + 7
    tok[(fill >= 0.53) & (fill < 0.56)] = INT32_MAX
    if n >= 7:
        tok[0] = -1                                                      # c = 0
        tok[1] = [V, -1, INT32_MAX, V + 7][:width] + [-1] * max(0, width - 4)       # c = 0 from ids that name no row
        tok[2] = -1
        tok[2, width - 1] = 3                                            # c = 1, at the last position
        tok[3] = rng.integers(0, V, size=width)                          # c = width
        tok[4] = ([4, 7, 5] * width)[:width]
        tok[5] = ([4, 5, 7] * width)[:width]
    return tok, table


def on_device(a, misalign=False):
    """A device copy of ``a``; ``misalign``: 4 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    if not misalign:
        return torch.from_numpy(a).to(DEV)
    flat = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = flat[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return view


def run(tok, table, mode, form, row_map=None, n_rows=None, ldo=None, col=None, sentinel=True):
    """One call into a sentinel-filled buffer [n_rows + 2, ldo]; the result is the slice [1 : 1 + n_rows, col : col + D].  ``form``
    16 or 4 with ldo / col None chooses a layout that takes that form.  -> the slice as numpy, after checking everything else."""
    n, d = tok.shape[0], table.shape[1]
    n_rows = n if n_rows is None else n_rows
    if ldo is None:
        ldo, col = (d + 8, 4) if form == 16 else (d + 7, 3)
    wide = torch.full((n_rows + 2, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    out = wide[1:1 + n_rows, col:col + d]
    dev_table = on_device(table, misalign=(form == 4 and ldo % 4 == 0 and col % 4 == 0))
    lib = _lib.load()
    if n_rows > 1:
        assert lib.gte_token_pool_access_bytes(_lib.ptr(dev_table), d, _lib.ptr(out), out.stride(0)) == form
    res = G.token_pool(on_device(tok), dev_table, mode=mode, row_map=None if row_map is None else on_device(row_map), out=out)
    assert res.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got = wide.cpu().numpy()
    if sentinel:
        named = np.zeros(n_rows, dtype=bool)
        named[np.arange(n) if row_map is None else row_map[row_map >= 0]] = True
        assert np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL)
        assert np.all(got[:, :col] == SENTINEL) and np.all(got[:, col + d:] == SENTINEL)
        assert np.all(got[1:1 + n_rows][~named] == SENTINEL)
    return got[1:1 + n_rows, col:col + d]


def expect(tok, table, mode, row_map=None, n_rows=None):
    """(rows that must hold a result, their values)."""
    want = ref.pool(tok, table, mode)
    if row_map is None:
        return np.arange(tok.shape[0]), want
    kept = row_map >= 0
    return row_map[kept], want[kept]


def forms_for(d):
    return (16, 4) if d % 4 == 0 else (4,)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [768, 12, 5, 260])
def test_every_width_of_row_in_both_access_forms(d, mode):
    tok, table = make_case(300, 15, d, seed=d)
    counts = ((tok >= 0) & (tok < V)).sum(axis=1)
    assert {0, 1, 15} <= set(counts.tolist())
    rows, want = expect(tok, table, mode)
    if mode == "mean":
        assert want[4, 0] != want[5, 0]                                  # the order of the adds shows in the data
    results = []
    for form in forms_for(d):
        got = run(tok, table, mode, form)
        np.testing.assert_array_equal(got[rows], want)
        results.append(got)
    if len(results) == 2:
        assert results[0].tobytes() == results[1].tobytes()              # the same bits through both forms
    assert not want[0].any() and not want[1].any()                       # c = 0: zeros, from -1 and from ids that name no row


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [0, 1, 7, 300])
@pytest.mark.parametrize("width", [15, 1])
def test_word_counts_and_widths(width, n, mode):
    tok, table = make_case(n, width, 12, seed=100 + n + width)
    rows, want = expect(tok, table, mode)
    for form in (16, 4):
        got = run(tok, table, mode, form)
        np.testing.assert_array_equal(got[rows], want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", [32, 17])
def test_widths_above_one_batch_of_reads(width, mode):
    tok, table = make_case(65, width, 20, seed=width)
    tok[6] = np.arange(width) % V                                        # every position takes part: two batches
    rows, want = expect(tok, table, mode)
    for form in (16, 4):
        np.testing.assert_array_equal(run(tok, table, mode, form)[rows], want)


@pytest.mark.parametrize("mode", MODES)
def test_more_words_than_one_pass_of_the_grid(mode):
    n = 2048 * 4 * 2 + 13
    tok, table = make_case(n, 15, 8, seed=5)
    rows, want = expect(tok, table, mode)
    for form in (16, 4):
        np.testing.assert_array_equal(run(tok, table, mode, form, sentinel=False)[rows], want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["permutation", "dropped", "all_dropped"])
@pytest.mark.parametrize("d", [768, 5])
def test_row_map(d, kind, mode):
    n = 300
    tok, table = make_case(n, 15, d, seed=7)
    rng = np.random.default_rng(8)
    if kind == "permutation":
        row_map, n_rows = rng.permutation(n).astype(np.int64), n
    elif kind == "dropped":                                              # what island removal leaves: the kept words, in order
        keep = rng.random(n) < 0.6
        row_map, n_rows = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64), int(keep.sum())
        row_map[~keep & (rng.random(n) < 0.5)] = -5                      # any negative row is a dropped word
    else:
        row_map, n_rows = np.full(n, -1, dtype=np.int64), 3
    rows, want = expect(tok, table, mode, row_map)
    for form in forms_for(d):
        got = run(tok, table, mode, form, row_map=row_map, n_rows=n_rows)
        np.testing.assert_array_equal(got[rows], want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ldo,col,form", [(768, 0, 16), (831, 63, 4), (832, 64, 16), (832, 63, 4)])
def test_the_feature_matrix_layouts(ldo, col, form, mode):
    tok, table = make_case(300, 15, 768, seed=9)
    rows, want = expect(tok, table, mode)
    got = run(tok, table, mode, form, ldo=ldo, col=col)
    np.testing.assert_array_equal(got[rows], want)
    keep = np.arange(300) % 3 != 1
    row_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    rows, want = expect(tok, table, mode, row_map)
    got = run(tok, table, mode, form, row_map=row_map, n_rows=int(keep.sum()), ldo=ldo, col=col)
    np.testing.assert_array_equal(got[rows], want)


def test_packed_output_and_a_misaligned_table_take_the_dword_form():
    tok, table = make_case(300, 15, 12, seed=10)
    want = ref.pool(tok, table, "mean")
    packed = G.token_pool(on_device(tok), on_device(table))              # out allocated: ldo == dim
    assert packed.is_contiguous() and tuple(packed.shape) == (300, 12)
    np.testing.assert_array_equal(packed.cpu().numpy(), want)
    shifted = on_device(table, misalign=True)
    lib = _lib.load()
    assert lib.gte_token_pool_access_bytes(_lib.ptr(shifted), 12, _lib.ptr(packed), 12) == 4
    assert lib.gte_token_pool_access_bytes(_lib.ptr(on_device(table)), 12, _lib.ptr(packed), 12) == 16
    got = G.token_pool(on_device(tok), shifted)
    assert got.cpu().numpy().tobytes() == packed.cpu().numpy().tobytes()
    tok64 = G.token_pool(on_device(tok.astype(np.int64)), on_device(table), mode="max")       # int64 ids are narrowed
    np.testing.assert_array_equal(tok64.cpu().numpy(), ref.pool(tok, table, "max"))


def test_a_non_default_stream_an_empty_vocabulary_and_the_wrapper_errors():
    tok, table = make_case(300, 15, 12, seed=11)
    args = on_device(tok), on_device(table)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = G.token_pool(*args)
    stream.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), ref.pool(tok, table, "mean"))
    none = G.token_pool(args[0], torch.zeros((0, 12), dtype=torch.float32, device=DEV))       # no row at all: every id is skipped
    assert not none.cpu().numpy().any()
    out = torch.zeros((10, 12), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="mode"):
        G.token_pool(*args, mode="sum")
    with pytest.raises(ValueError, match="float32 matrix"):
        G.token_pool(args[0], args[1].double())
    with pytest.raises(ValueError, match="tok must be"):
        G.token_pool(args[0][:, 0], args[1])
    with pytest.raises(ValueError, match="row_map names rows of"):
        G.token_pool(*args, row_map=torch.zeros(300, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="row_map names row 10"):
        G.token_pool(*args, row_map=torch.arange(300, dtype=torch.int64, device=DEV) % 11, out=out)
    with pytest.raises(ValueError, match="one integer row per word"):
        G.token_pool(*args, row_map=torch.zeros(299, dtype=torch.int64, device=DEV), out=out)
    with pytest.raises(ValueError, match="unit column stride"):
        G.token_pool(*args, out=torch.zeros((300, 24), dtype=torch.float32, device=DEV)[:, ::2])
    with pytest.raises(ValueError, match="out must be"):
        G.token_pool(*args, out=out)                                     # 10 rows for 300 words without a row_map
    assert not out.cpu().numpy().any()


def test_argument_errors_return_their_code_without_a_launch():
    lib = _lib.load()
    tok, table = make_case(7, 15, 12, seed=12)
    t, tb = on_device(tok), on_device(table)
    out = torch.full((7, 12), SENTINEL, dtype=torch.float32, device=DEV)
    rm = torch.arange(7, dtype=torch.int64, device=DEV)
    p = _lib.ptr
    INVALID, UNSUPPORTED = -1, -4
    assert lib.gte_token_pool_max_width() == 32 and lib.gte_token_pool_max_dim() == 4096

    def call(tok=p(t), n=7, width=15, table=p(tb), v=V, dim=12, mode=0, row_map=p(rm), out=p(out), ldo=12):
        return lib.gte_token_pool_f32(tok, n, width, table, v, dim, mode, row_map, out, ldo, _lib.current_stream())
    bad = [(dict(n=-1), INVALID, b"sizes"), (dict(v=-1), INVALID, b"sizes"), (dict(width=0), INVALID, b"sizes"),
           (dict(dim=0), INVALID, b"sizes"), (dict(v=2 ** 31), INVALID, b"int32"), (dict(ldo=11), INVALID, b"ldo"),
           (dict(mode=2), INVALID, b"mode"), (dict(mode=-1), INVALID, b"mode"), (dict(width=33), UNSUPPORTED, b"limits"),
           (dict(dim=4097, ldo=4097), UNSUPPORTED, b"limits"), (dict(tok=None), INVALID, b"null"), (dict(out=None), INVALID, b"null"),
           (dict(table=None), INVALID, b"null"), (dict(tok=p(t) + 2), INVALID, b"aligned"), (dict(table=p(tb) + 1), INVALID, b"aligned"),
           (dict(out=p(out) + 2), INVALID, b"aligned"), (dict(row_map=p(rm) + 4), INVALID, b"aligned")]
    for kw, code, text in bad:
        assert call(**kw) == code, kw
        assert text in lib.gte_last_error(), (kw, lib.gte_last_error())
    assert call(n=0, tok=None, out=None, table=None) == 0                # nothing to do: no launch, nothing looked at
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)                                    # none of the calls above launched anything
    assert call() == 0 and call(row_map=None, mode=1) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), ref.pool(tok, table, "max"))
