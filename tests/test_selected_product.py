"""Selected-key product Y = A[I, :] X / A[:, J]' X (include/dsa.h: dsa_mat_spmm_selected[_dev]; csrc/selprod.hip).

Expected values never come from the library: `expected_selected` cuts the cells of the selected keys out of the ORACLE's exported
layout (slot order, live partitions only) and sums them with `expected_spmm` of test_spmm, the numpy walk that adds the terms of a
row left to right with one multiply and one add per term.  That is row `key - 1` of the full walk at ny_full = max(size, max key)
without materialising ny_full rows (a selection holds the key 2^40).  Where the keys lie inside the size the two are compared as
well.  Every comparison is bitwise (uint64 views); there are no tolerances.  Y is pre-filled with a sentinel, the padding of X is
NaN."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode
from test_spmm import _bits, _expect, _same_bits, expected_spmm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
EARG, EMODE = 1, 5
SENTINEL = -7.25
KS_GOLDEN = (1, 2, 3, 4, 5, 8, 16, 17, 33)
BIG = (1 << 31) + 5
P_F64, P_I64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
NAMES = ("mat_spmm_selected", "mat_spmm_selected_dev")


def layout_cells(L):
    """(outer, idx, val) of one orientation from its exported layout: the cells of every live partition in slot order, `outer` the
    key of the cell's partition (ascending), idx the cell's key - 1"""
    occ = L["occ"].astype(bool)
    keys, vals = L["keys"][occ], L["vals"][occ]
    sems, col_keys = L["semaphores"], L["col_keys"]
    live = (sems != 0) & (L["col_live"] != 0)
    is_sem = keys == 0
    assert not occ.any() or is_sem[0], "a cell in front of the first semaphore"
    pid = vals[is_sem].astype(np.int64)
    part = pid[np.cumsum(is_sem) - 1]
    cell = ~is_sem & live[part - 1]
    outer = col_keys[part[cell] - 1].astype(np.int64)
    assert np.all(np.diff(outer) >= 0)
    return outer, keys[cell].astype(np.int64) - 1, vals[cell].copy()


def expected_selected(L, sel, X):
    """row j = the walk over the cells of the live partition whose key is sel[j] (none: +0.0)"""
    outer, idx, val = layout_cells(L)
    sel = np.asarray(sel, dtype=np.int64)
    lo, hi = np.searchsorted(outer, sel, side="left"), np.searchsorted(outer, sel, side="right")
    cnt = hi - lo
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    pos = np.repeat(lo - ptr[:-1], cnt) + np.arange(ptr[-1])
    return expected_spmm(ptr, idx[pos], val[pos], X, len(sel))


def _expect_sel(b, transpose, sel, X):
    """b: an oracle-bound matrix"""
    return expected_selected(b.export_layout(COLMAJOR if transpose else ROWMAJOR), sel, X)


def _dev(a, transpose, sel, X, ldx=None, ldy=None):
    """dsa_mat_spmm_selected_dev on torch tensors; the padding of X is NaN (never used), Y is pre-filled with the sentinel"""
    import torch
    nx, k = X.shape
    ldx, ldy = ldx or k, ldy or k
    xh = np.full((nx, ldx), np.nan)
    xh[:, :k] = X
    xd = torch.from_numpy(xh).to("cuda")
    sd = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int64)).to("cuda")
    yd = torch.full((len(sel), ldy), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a.matmul_selected_dev(sd.data_ptr(), len(sel), xd.data_ptr(), nx, k, yd.data_ptr(), ldx=ldx, ldy=ldy, transpose=transpose)
    a.sync()
    return yd.cpu().numpy()


def _host(hip, a, transpose, sel, X, ldx=None, ldy=None):
    """dsa_mat_spmm_selected on host arrays with leading dimensions"""
    nx, k = X.shape
    ldx, ldy = ldx or k, ldy or k
    xh = np.full((nx, ldx), np.nan)
    xh[:, :k] = X
    s = np.ascontiguousarray(sel, dtype=np.int64)
    y = np.full((len(s), ldy), SENTINEL)
    hip.call("mat_spmm_selected", a.h, 1 if transpose else 0, s.ctypes.data_as(P_I64), len(s), xh.ctypes.data_as(P_F64), nx, k, ldx,
             y.ctypes.data_as(P_F64), ldy)
    return y


def _check(hip, a, b, make_sel, ks, seed=0, dims=None, full=False):
    """both transposes, every k, both entry points against the walk over the oracle's layout.  make_sel(transpose, dim) gives the
    keys; X is sized by size(b) unless dims = (m, n) is given; full: the keys inside the size are compared with the full walk too"""
    rng = np.random.default_rng(seed)
    m, n = dims or b.size()
    for transpose, nx, dim in ((False, n, m), (True, m, n)):
        L = b.export_layout(COLMAJOR if transpose else ROWMAJOR)
        sel = np.asarray(make_sel(transpose, dim), dtype=np.int64)
        for k in ks:
            X = rng.standard_normal((nx, k))
            exp = expected_selected(L, sel, X)
            if full:
                inside = sel <= dim
                _same_bits(exp[inside], _expect(b, transpose, X, dim)[sel[inside] - 1])
            _same_bits(_dev(a, transpose, sel, X), exp)
            _same_bits(_host(hip, a, transpose, sel, X), exp)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_selected_product_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    assert hasattr(dsa.DynamicSparseMatrix, "matmul_selected") and hasattr(dsa.DynamicSparseMatrix, "matmul_selected_dev")
    assert hasattr(dsa.Transposed, "matmul_selected")


def test_oracle_binding_has_no_selected_product(dsa, oracle):
    assert not oracle.has(NAMES[0]) and not oracle.has(NAMES[1])
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul_selected([1], np.ones((2, 2)))
    with pytest.raises(dsa.DsaArgumentError):
        a.T.matmul_selected([1], np.ones((2, 2)))
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul_selected_dev(0, 0, 0, 0, 1, 0)


def test_helper_is_the_full_walk_at_the_selected_rows(dsa, oracle):
    """expected_selected == rows sel - 1 of the full walk of test_spmm, and +0.0 for keys without a live partition"""
    rng = np.random.default_rng(5)
    m, n = 70, 50
    I, J = rng.integers(1, m + 1, 600), rng.integers(1, n + 1, 600)
    b = dsa.dynamicsparse(I, J, rng.standard_normal(600), m, n, binding=oracle)
    b.deleterow(int(I[0]))
    b.deletecolumn(int(J[1]))
    for transpose, nx, dim in ((False, n, m), (True, m, n)):
        X = rng.standard_normal((nx, 3))
        sel = np.concatenate([rng.permutation(dim) + 1, [int(I[0]) if not transpose else int(J[1]), 3, 3]])
        exp = _expect_sel(b, transpose, sel, X)
        _same_bits(exp, _expect(b, transpose, X, dim)[sel - 1])
        far = _expect_sel(b, transpose, [dim + 3, 1 << 40], X)
        assert (_bits(far) == 0).all()
        assert (_bits(exp[-3]) == 0).all()                           # the deleted key


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_cases_exact(dsa, hip, oracle, sc):
    import torch
    a = run_scenario(dsa, hip, sc)
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        x = torch.ones((4, 2), dtype=torch.float64, device="cuda")
        y = torch.full((4, 2), SENTINEL, dtype=torch.float64, device="cuda")
        s = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device="cuda")
        xh, yh, sh = np.ones((4, 2)), np.full((4, 2), SENTINEL), np.array([1, 2, 3, 4], dtype=np.int64)
        torch.cuda.synchronize()
        for tr in (0, 1):
            with pytest.raises(dsa.DsaError) as ei:
                a.matmul_selected_dev(s.data_ptr(), 4, x.data_ptr(), 4, 2, y.data_ptr(), transpose=bool(tr))
            assert ei.value.code == EMODE
            with pytest.raises(dsa.DsaError) as ei:
                hip.call("mat_spmm_selected", a.h, tr, sh.ctypes.data_as(P_I64), 4, xh.ctypes.data_as(P_F64), 4, 2, 2,
                         yh.ctypes.data_as(P_F64), 2)
            assert ei.value.code == EMODE
        torch.cuda.synchronize()
        assert (y == SENTINEL).all() and (yh == SENTINEL).all()
        return
    assert a.size() == b.size()

    def sel(transpose, dim):
        every = np.arange(dim, 0, -1, dtype=np.int64)                # all keys, reversed
        return np.concatenate([every, every[:5], every[::3], [dim + 3, 1 << 40]])

    _check(hip, a, b, sel, KS_GOLDEN, full=True)


def _random_pair(dsa, hip, oracle, rng, m=700, n=500, nnz=6000):
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.standard_normal(nnz)
    return (I, J), tuple(dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))


@pytest.mark.gpu
def test_random_matrix_after_each_change(dsa, hip, oracle):
    rng = np.random.default_rng(11)
    m, n = 700, 500
    (I, J), (a, b) = _random_pair(dsa, hip, oracle, rng, m, n)
    ks = (1, 8, 13)
    extra = {False: [], True: []}                                    # keys every later selection holds, per transpose

    def sel(transpose, dim):
        # a random permutation with repeats; keys up to dim + 60 own no partition
        return np.concatenate([rng.permutation(dim + 60) + 1, rng.integers(1, dim + 61, 150), extra[transpose]]).astype(np.int64)

    _check(hip, a, b, sel, ks, 1)
    # mixed writes, a quarter of them zeros (deletions)
    I2, J2 = rng.integers(1, m + 1, 3000), rng.integers(1, n + 1, 3000)
    V2 = np.where(rng.random(3000) < 0.25, 0.0, rng.standard_normal(3000))
    for x in (a, b):
        x.set_batch(I2, J2, V2)
    _check(hip, a, b, sel, ks, 2)
    # tombstones in both orientations; the deleted keys are selected and give +0.0 rows
    c1, c2 = (int(c) for c in np.unique(J[:20])[:2])
    r1 = int(I[5])
    for x in (a, b):
        x.deletecolumn(c1)
        x.deletecolumn(c2)
        x.deleterow(r1)
    extra[True] += [c1, c2]
    extra[False] += [r1]
    X = rng.standard_normal((m, 3))
    assert (_bits(_expect_sel(b, True, [c1, c2], X)) == 0).all()
    assert (_bits(_dev(a, True, [c1, c2], X)) == 0).all()
    assert (_bits(_dev(a, False, [r1], rng.standard_normal((n, 3)))) == 0).all()
    _check(hip, a, b, sel, ks, 3)
    # new columns, keys in random order (pending / unsorted table entries)
    newc = rng.permutation(np.arange(n + 1, n + 41))
    I3 = rng.integers(1, m + 1, len(newc))
    V3 = rng.standard_normal(len(newc))
    for x in (a, b):
        x.set_batch(I3, newc, V3)
    assert a.size() == b.size() == (m, n + 40)
    _check(hip, a, b, sel, ks, 4)
    # a zero written beyond size(m, 2): an empty live partition outside the size, selected
    for x in (a, b):
        x[3, n + 100] = 0.0
    assert a.size() == b.size() and a.size()[1] < n + 100
    extra[True] += [n + 100]
    _check(hip, a, b, sel, ks, 5)


EDGE_LENGTHS = (65, 0, 1, 63, 64, 511, 512, 513, 200, 224, 300, 1300)               # cells of rows 1 .. 12


def _spans(L):
    """{key: (lo, hi)}: the slot span of every live partition, 0-based, from the exported tables (the next live semaphore ends it,
    the capacity ends the last one)"""
    sems, ck = L["semaphores"].astype(np.int64), L["col_keys"].astype(np.int64)
    live = np.nonzero((sems != 0) & (L["col_live"] != 0))[0]
    cap = int(L["info"]["capacity"])
    ends = np.concatenate([sems[live][1:] - 1, [cap]])
    return {int(ck[e]): (int(sems[e]), int(hi)) for e, hi in zip(live, ends)}, cap


@pytest.mark.gpu
def test_span_and_grid_edges(dsa, hip, oracle):
    rng = np.random.default_rng(91)
    m, n = len(EDGE_LENGTHS), 1400
    I = np.concatenate([np.full(c, r + 1) for r, c in enumerate(EDGE_LENGTHS)])
    J = np.concatenate([rng.choice(n, c, replace=False) + 1 for c in EDGE_LENGTHS])
    V = rng.standard_normal(len(I))
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    L = b.export_layout(ROWMAJOR)
    spans, cap = _spans(L)
    occ = L["occ"].astype(bool)
    words = {}
    for r, c in enumerate(EDGE_LENGTHS):
        if c == 0:
            assert r + 1 not in spans
            continue
        lo, hi = spans[r + 1]
        assert int(occ[lo:hi].sum()) == c, (r + 1, lo, hi)
        words[c] = (hi - 1) // 64 - lo // 64 + 1
    # the spans really cross what the kernel cuts them at.  The structure keeps gaps, so a span is longer than its cells: the
    # lengths of the issue and three more (200, 224, 300) give spans inside one word, across word boundaries, of one full load, of
    # exactly two loads, of three and of more; first and last words are masked on both sides
    loads = {c: -(-w // 9) for c, w in words.items()}
    assert words[1] == 1 and words[63] >= 2 and words[64] >= 2 and words[65] >= 2 and words[65] <= 9, words
    assert {1, 2, 3} <= set(loads.values()) and loads[1300] > 3, loads
    assert min(loads[511], loads[512], loads[513]) >= 2, loads
    assert any(w in (9, 10) for w in words.values()), words          # a span that ends at / just behind the ninth word
    assert any(lo % 64 for lo, _ in spans.values()) and any(hi % 64 for _, hi in spans.values())
    # the first partition of the slot array and the last one, whose span ends at the capacity
    assert min(lo for lo, _ in spans.values()) == spans[1][0] and spans[m][1] == cap and cap % 64 == 0
    for nsel in (1, 3, 4, 5, 4 * 3 + 1):                             # the last workgroup is partly empty
        sel = np.concatenate([[m, 1], rng.permutation(m) + 1])[:nsel]
        for transpose, nx in ((False, n), (True, m)):
            keys = sel if not transpose else rng.integers(1, n + 1, nsel)
            for k in (1, 8):
                X = rng.standard_normal((nx, k))
                exp = _expect_sel(b, transpose, keys, X)
                _same_bits(_dev(a, transpose, keys, X), exp)
                _same_bits(_host(hip, a, transpose, keys, X), exp)
    every = np.arange(1, m + 1)
    for k in (1, 3, 8, 16):
        X = rng.standard_normal((n, k))
        _same_bits(_dev(a, False, every, X), _expect(b, False, X, m))


@pytest.mark.gpu
def test_leading_dimensions_padding_and_absent_keys(dsa, hip, oracle):
    rng = np.random.default_rng(21)
    m, n = 700, 500
    I, J = rng.integers(1, m + 1, 3000), rng.integers(1, n + 1, 3000)
    I[I % 9 == 0] += 1                       # rows 9, 18, ... own no partition
    V = rng.standard_normal(3000)
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    assert a.size() == b.size() == (m, n)
    for transpose, nx, dim in ((False, n, m), (True, m, n)):
        sel = np.concatenate([rng.permutation(dim) + 1, [dim + 1, 1 << 40]])
        for k in (1, 3, 8, 13, 20):
            X = rng.standard_normal((nx, k))
            exp = _expect_sel(b, transpose, sel, X)
            for got in (_dev(a, transpose, sel, X, k + 3, k + 5), _host(hip, a, transpose, sel, X, k + 3, k + 5)):
                assert got.shape == (len(sel), k + 5)
                assert (got[:, k:] == SENTINEL).all()
                _same_bits(got[:, :k], exp)
                assert (_bits(got[-2:, :k]) == 0).all()              # beyond the size: +0.0, sign bit clear
                if not transpose:
                    absent = np.nonzero(~np.isin(sel, I))[0]
                    assert len(absent) >= m // 9
                    assert (_bits(got[absent, :k]) == 0).all()


@pytest.mark.gpu
def test_wide_keys(dsa, hip, oracle):
    # a column key beyond int32: the rowmajor orientation stores int64 keys; nx = 7 leaves the wide cells outside X
    I = np.array([1, 2, 3, 3, 4], dtype=np.int64)
    J = np.array([1, 7, 2, BIG, BIG], dtype=np.int64)
    V = np.array([1.5, -2.0, 3.25, 4.0, 0.125])
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    rng = np.random.default_rng(31)
    rows = np.array([3, 4, 1, 2, 3, 9], dtype=np.int64)              # rows 3 and 4 hold the wide cell
    cols = np.array([BIG, 1, 7, 2, BIG, 5, BIG + 1], dtype=np.int64)
    for k in (1, 3, 8, 17):
        X = rng.standard_normal((7, k))
        exp = _expect_sel(b, False, rows, X)
        assert exp[1].tolist() == [0.0] * k                          # row 4 holds a wide cell only: it contributes nothing
        _same_bits(exp[:5], _expect(b, False, X, 4)[rows[:5] - 1])
        _same_bits(_dev(a, False, rows, X), exp)
        _same_bits(_host(hip, a, False, rows, X), exp)
        Xt = rng.standard_normal((4, k))                             # A[:, cols]' X: the key BIG is found through the int64 table
        expt = _expect_sel(b, True, cols, Xt)
        assert (expt[0] != 0.0).all() and (_bits(expt[0]) == _bits(expt[4])).all() and (_bits(expt[-2:]) == 0).all()
        _same_bits(_dev(a, True, cols, Xt), expt)
        _same_bits(_host(hip, a, True, cols, Xt), expt)
    # int64 key storage with every remaining key inside X: a wide key written and deleted again (the arrays are widened once)
    (I, J), (a, b) = _random_pair(dsa, hip, oracle, rng, 60, 50, 400)
    dims = a.size()
    for x in (a, b):
        x[5, BIG] = 2.0
        x[5, BIG] = 0.0
    assert a.size() == b.size() == (dims[0], BIG)

    def sel(transpose, dim):
        return np.concatenate([rng.permutation(dim) + 1, [BIG] if transpose else [5, 5]])

    _check(hip, a, b, sel, (1, 4, 8, 16), 32, dims=dims)


@pytest.mark.gpu
def test_long_row_among_ordinary_rows(dsa, hip, oracle):
    rng = np.random.default_rng(41)
    m, n, long_row, Lc = 300, 30000, 7, 20000
    I = np.concatenate([np.full(Lc, long_row), rng.integers(1, m + 1, 3000)])
    J = np.concatenate([rng.choice(n, Lc, replace=False) + 1, rng.integers(1, n + 1, 3000)])
    V = rng.random(len(I)) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    assert len(b.row_view(long_row)) >= Lc
    rows = np.array([5, 6, long_row, 8, 200, long_row, 9, 300, 1], dtype=np.int64)
    cols = J[:Lc][rng.permutation(Lc)[:2000]].astype(np.int64)
    LR, LC = b.export_layout(ROWMAJOR), b.export_layout(COLMAJOR)
    for k in (1, 8):
        X = rng.random((n, k)) + 0.5
        exp = expected_selected(LR, rows, X)
        _same_bits(exp, _expect(b, False, X, m)[rows - 1])
        got, again = _dev(a, False, rows, X), _dev(a, False, rows, X)
        _same_bits(got, exp)                                         # no length limit: the long row is in reference order
        _same_bits(again, got)                                       # the same bits on a second call
        _same_bits(_host(hip, a, False, rows, X), exp)
        Xt = rng.random((m, k)) + 0.5                                # 2000 of the long row's columns
        _same_bits(_dev(a, True, cols, Xt), expected_selected(LC, cols, Xt))


@pytest.mark.gpu
def test_agrees_with_the_full_product(dsa, hip, oracle):
    import torch
    rng = np.random.default_rng(51)
    (_, _), (a, _b) = _random_pair(dsa, hip, oracle, rng)
    m, n = a.size()
    for transpose, nx, dim in ((False, n, m), (True, m, n)):
        keys = np.concatenate([rng.permutation(dim) + 1, rng.integers(1, dim + 1, 100)])
        for k in (1, 6, 17):
            X = rng.standard_normal((nx, k))
            full = a.matmul(X, transpose=transpose)
            _same_bits(a.matmul_selected(keys, X, transpose=transpose), full[keys - 1])
            Xd = torch.from_numpy(X).to("cuda")
            fulld = a.matmul(Xd, transpose=transpose)
            got = a.matmul_selected(torch.from_numpy(keys).to("cuda"), Xd, transpose=transpose)
            assert torch.equal(got.view(torch.int64), fulld[torch.from_numpy(keys - 1).to("cuda")].view(torch.int64))
            _same_bits(got.cpu().numpy(), full[keys - 1])


@pytest.mark.gpu
def test_argument_errors_leave_y_untouched(dsa, hip):
    import torch
    a = dsa.dynamicsparse([1, 2, 3], [1, 2, 3], [1.0, 2.0, 3.0], binding=hip)
    x = torch.ones((3, 8), dtype=torch.float64, device="cuda")
    y = torch.full((3, 8), SENTINEL, dtype=torch.float64, device="cuda")
    s = torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda")
    xh, yh, sh = np.ones((3, 8)), np.full((3, 8), SENTINEL), np.array([1, 2, 3], dtype=np.int64)
    VP = C.c_void_p
    sp, xp, yp = VP(s.data_ptr()), VP(x.data_ptr()), VP(y.data_ptr())
    shp, xhp, yhp = sh.ctypes.data_as(P_I64), xh.ctypes.data_as(P_F64), yh.ctypes.data_as(P_F64)
    dev, host = hip._mat_spmm_selected_dev, hip._mat_spmm_selected
    torch.cuda.synchronize()
    for k, ldx, ldy in ((0, 8, 8), (4, 3, 8), (4, 8, 3), (-1, 8, 8)):
        assert dev(a.h, 0, sp, 3, xp, 3, k, ldx, yp, ldy) == EARG, (k, ldx, ldy)
        assert host(a.h, 0, shp, 3, xhp, 3, k, ldx, yhp, ldy) == EARG, (k, ldx, ldy)
    for tr in (0, 1):
        assert dev(a.h, tr, sp, -1, xp, 3, 2, 8, yp, 8) == EARG                  # nsel < 0
        assert dev(a.h, tr, sp, 3, xp, -1, 2, 8, yp, 8) == EARG                  # nx < 0
        assert dev(a.h, tr, None, 3, xp, 3, 2, 8, yp, 8) == EARG                 # NULL sel / x / y
        assert dev(a.h, tr, sp, 3, None, 3, 2, 8, yp, 8) == EARG
        assert dev(a.h, tr, sp, 3, xp, 3, 2, 8, None, 8) == EARG
        assert host(a.h, tr, shp, -1, xhp, 3, 2, 8, yhp, 8) == EARG
        assert host(a.h, tr, shp, 3, xhp, -1, 2, 8, yhp, 8) == EARG
        assert host(a.h, tr, None, 3, xhp, 3, 2, 8, yhp, 8) == EARG
        assert host(a.h, tr, shp, 3, None, 3, 2, 8, yhp, 8) == EARG
        assert host(a.h, tr, shp, 3, xhp, 3, 2, 8, None, 8) == EARG
        for bad in (0, -5):                                                      # the host entry sees the keys: the 0-based mistake
            badk = np.array([1, bad, 3], dtype=np.int64)
            assert host(a.h, tr, badk.ctypes.data_as(P_I64), 3, xhp, 3, 2, 8, yhp, 8) == EARG
        assert dev(a.h, tr, sp, 0, xp, 3, 2, 8, yp, 8) == 0                      # nsel = 0: nothing is launched
        assert dev(a.h, tr, None, 0, xp, 3, 2, 8, None, 8) == 0
        assert host(a.h, tr, shp, 0, xhp, 3, 2, 8, yhp, 8) == 0
    a.sync()
    torch.cuda.synchronize()
    assert (y == SENTINEL).all() and (yh == SENTINEL).all()
    # the device entry cannot report a key: 0 gives a +0.0 row, the others their product
    s0 = torch.tensor([0, 2, -5], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert dev(a.h, 0, VP(s0.data_ptr()), 3, xp, 3, 2, 8, yp, 8) == 0
    a.sync()
    got = y.cpu().numpy()
    assert (_bits(got[0, :2]) == 0).all() and (got[1, :2] == 2.0).all() and (_bits(got[2, :2]) == 0).all()
    assert (got[:, 2:] == SENTINEL).all()
    # nx = 0: zero rows in columns 0 .. k - 1 only, on both entries
    y.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert dev(a.h, 0, sp, 3, None, 0, 2, 8, yp, 8) == 0
    assert host(a.h, 0, shp, 3, None, 0, 2, 8, yhp, 8) == 0
    a.sync()
    for got in (y.cpu().numpy(), yh):
        assert (_bits(got[:, :2]) == 0).all() and (got[:, 2:] == SENTINEL).all()


@pytest.mark.gpu
def test_dev_call_on_a_caller_stream(dsa, hip, oracle):
    import torch
    rng = np.random.default_rng(61)
    (_, _), (a, b) = _random_pair(dsa, hip, oracle, rng)
    m, n = a.size()
    s = torch.cuda.Stream()
    hip.call("mat_set_stream", a.h, C.c_void_p(s.cuda_stream))
    try:
        for transpose, nx, dim in ((False, n, m), (True, m, n)):
            X = rng.standard_normal((nx, 8))
            sel = rng.integers(1, dim + 20, 300)
            _same_bits(_dev(a, transpose, sel, X), _expect_sel(b, transpose, sel, X))      # _dev ends with dsa_mat_sync
    finally:
        hip.call("mat_set_stream", a.h, C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.gpu
def test_python_surface(dsa, hip, oracle):
    import torch
    rng = np.random.default_rng(71)
    (_, _), (a, b) = _random_pair(dsa, hip, oracle, rng)
    m, n = a.size()
    X = rng.standard_normal((n, 10))
    Xt = rng.standard_normal((m, 10))
    rows = np.concatenate([rng.permutation(m)[:200] + 1, [m + 7, 3, 3]]).astype(np.int64)
    cols = np.concatenate([rng.permutation(n)[:150] + 1, [n + 7]]).astype(np.int64)
    exp, expt = _expect_sel(b, False, rows, X), _expect_sel(b, True, cols, Xt)
    for keys in (rows.tolist(), rows):                                   # a list, a numpy array
        Y = a.matmul_selected(keys, X)
        assert isinstance(Y, np.ndarray) and Y.shape == (len(rows), 10)
        _same_bits(Y, exp)
    _same_bits(a.matmul_selected(cols, Xt, transpose=True), expt)
    _same_bits(a.T.matmul_selected(cols, Xt), expt)
    _same_bits(a.transpose().matmul_selected(cols.tolist(), Xt), expt)
    y1 = a.matmul_selected(rows, X[:, 0].copy())
    assert y1.shape == (len(rows),)
    _same_bits(y1, exp[:, 0])
    _same_bits(a.matmul_selected(rows, X[:, ::2]), _expect_sel(b, False, rows, X[:, ::2]))      # not contiguous: copied
    Xd = torch.from_numpy(X).to("cuda")
    rd = torch.from_numpy(rows).to("cuda")
    for keys in (rows.tolist(), rows, rd):                               # ... and an int64 CUDA tensor
        Yd = a.matmul_selected(keys, Xd)
        assert isinstance(Yd, torch.Tensor) and Yd.is_cuda and Yd.device == Xd.device and tuple(Yd.shape) == (len(rows), 10)
        _same_bits(Yd.cpu().numpy(), exp)
    _same_bits(a.matmul_selected(rd, Xd[:, ::2]).cpu().numpy(), _expect_sel(b, False, rows, X[:, ::2]))       # column-strided: copied
    _same_bits(a.matmul_selected(rd, Xd[:, 2:7]).cpu().numpy(), _expect_sel(b, False, rows, X[:, 2:7]))       # row-strided: ldx = 10
    _same_bits(a.T.matmul_selected(torch.from_numpy(cols).to("cuda"), torch.from_numpy(Xt).to("cuda")).cpu().numpy(), expt)
    yd1 = a.matmul_selected(rd, Xd[:, 0])
    assert tuple(yd1.shape) == (len(rows),)
    _same_bits(yd1.cpu().numpy(), exp[:, 0])
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul_selected(rows, torch.from_numpy(X))                     # a CPU tensor
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul_selected(rows, Xd.to(torch.float32))
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul_selected(rd.to(torch.int32), Xd)                        # a CUDA key tensor of the wrong dtype
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul_selected([1, 0], X)                                     # a key < 1 on the host entry
