"""Dense multi-vector product Y = A X / A' X (include/dsa.h: dsa_mat_spmm_dense[_dev]; csrc/spmm.hip).

Expected values never come from the kernel: `expected_spmm` is a numpy walk over a compressed form of the matrix — the ORACLE's exported
layout through `expected_compressed` (the full-size test: the product's own to_csr() / to_csc(), pinned against the oracle elsewhere) —
that adds the terms of every row rank by rank, i.e. left to right in ascending key order with one multiply and one add per term: the
reference's order (src/operations.jl:101) bit for bit.  Comparisons are bitwise (uint64 views).  The kernel keeps the reference order
for rows of any length (it has no length limit L), so the long-row test asserts bitwise too, besides the 1e-12 bound it is allowed.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode, expected_compressed

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
EARG, EMODE = 1, 5
SENTINEL = -7.25
KS_GOLDEN = (1, 2, 3, 4, 5, 8, 16, 17, 33)


def expected_spmm(ptr, idx, val, X, ny):
    """Y[r] = 0.0 + val * X[idx] over the cells ptr[r] .. ptr[r + 1] of row r, left to right (idx 0-based; a cell whose idx is
    outside X contributes nothing).  Rank by rank: numpy's separate multiply and add are not fused."""
    X = np.asarray(X, dtype=np.float64)
    nx, k = X.shape
    Y = np.zeros((ny, k))
    ptr = np.asarray(ptr, dtype=np.int64)
    cnt = np.diff(ptr[:ny + 1])
    r = 0
    while True:
        rows = np.nonzero(cnt > r)[0]
        if len(rows) == 0:
            return Y
        pos = ptr[rows] + r
        ok = (idx[pos] >= 0) & (idx[pos] < nx)
        rows, pos = rows[ok], pos[ok]
        Y[rows] += val[pos, None] * X[idx[pos]]
        r += 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, exp):
    assert got.shape == exp.shape, (got.shape, exp.shape)
    eq = _bits(got) == _bits(exp)
    assert eq.all(), (np.argwhere(~eq)[:5].tolist(), got[~eq][:5], exp[~eq][:5])


def _expect(src, transpose, X, ny):
    """src: an oracle-bound matrix (its exported layout) or a (ptr, idx, val) triple"""
    if isinstance(src, tuple):
        ptr, idx, val = src
    else:
        ptr, idx, val = expected_compressed(src.export_layout(COLMAJOR if transpose else ROWMAJOR), ny)
    return expected_spmm(ptr, idx, val, X, ny)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_spmm_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in ("mat_spmm_dense", "mat_spmm_dense_dev"):
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    assert hasattr(dsa.DynamicSparseMatrix, "matmul") and hasattr(dsa.DynamicSparseMatrix, "matmul_dev")
    assert hasattr(dsa.DynamicSparseMatrix, "__matmul__") and hasattr(dsa.Transposed, "__matmul__")


def test_oracle_binding_has_no_spmm(dsa, oracle):
    assert not oracle.has("mat_spmm_dense") and not oracle.has("mat_spmm_dense_dev")
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul(np.ones((2, 2)))
    with pytest.raises(dsa.DsaArgumentError):
        a.T @ np.ones((2, 2))
    with pytest.raises(dsa.DsaArgumentError):
        a.matmul_dev(0, 0, 1, 0, 0)


@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_helper_matches_the_oracle_product(dsa, oracle, sc):
    """expected_spmm at k = 1 is the oracle's dense product bit for bit, at k = 3 column by column"""
    a = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, a):
        return
    rng = np.random.default_rng(3)
    m, n = a.size()
    for transpose, nx, ny in ((False, n, m), (True, m, n)):
        X = rng.standard_normal((nx, 3))
        Y3 = _expect(a, transpose, X, ny)
        for j in range(3):
            y = a.mul(X[:, j].copy(), transpose=transpose)
            _same_bits(_expect(a, transpose, X[:, j:j + 1], ny)[:, 0], y)
            _same_bits(Y3[:, j], y)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a, transpose, X, ny, ldx=None, ldy=None):
    """dsa_mat_spmm_dense_dev on torch tensors; the padding of X is NaN (never used), Y is pre-filled with the sentinel"""
    import torch
    nx, k = X.shape
    ldx, ldy = ldx or k, ldy or k
    xh = np.full((nx, ldx), np.nan)
    xh[:, :k] = X
    xd = torch.from_numpy(xh).to("cuda")
    yd = torch.full((ny, ldy), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a.matmul_dev(xd.data_ptr(), nx, k, yd.data_ptr(), ny, ldx=ldx, ldy=ldy, transpose=transpose)
    a.sync()
    return yd.cpu().numpy()


def _host(hip, a, transpose, X, ny, ldx=None, ldy=None):
    """dsa_mat_spmm_dense on host arrays with leading dimensions"""
    nx, k = X.shape
    ldx, ldy = ldx or k, ldy or k
    xh = np.full((nx, ldx), np.nan)
    xh[:, :k] = X
    y = np.full((ny, ldy), SENTINEL)
    hip.call("mat_spmm_dense", a.h, 1 if transpose else 0, xh.ctypes.data_as(C.POINTER(C.c_double)), nx, k, ldx,
             y.ctypes.data_as(C.POINTER(C.c_double)), ny, ldy)
    return y


def _check(hip, a, src, ks, seed=0, host=True, dims=None):
    """both transposes, every k: the device entry point and (host=True) the host one against the expected product; X and Y are
    sized by size(a) unless dims = (m, n) is given"""
    rng = np.random.default_rng(seed)
    m, n = dims or a.size()
    for transpose, nx, ny in ((False, n, m), (True, m, n)):
        for k in ks:
            X = rng.standard_normal((nx, k))
            exp = _expect(src, transpose, X, ny)
            _same_bits(_dev(a, transpose, X, ny), exp)
            if host:
                _same_bits(_host(hip, a, transpose, X, ny), exp)
                if dims is None:                                     # matmul sizes Y by size(a)
                    _same_bits(a.matmul(X, transpose=transpose), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_cases_exact(dsa, hip, oracle, sc):
    import torch
    a = run_scenario(dsa, hip, sc)
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        x = torch.ones((4, 2), dtype=torch.float64, device="cuda")
        y = torch.full((4, 2), SENTINEL, dtype=torch.float64, device="cuda")
        xh, yh = np.ones((4, 2)), np.full((4, 2), SENTINEL)
        for tr in (0, 1):
            with pytest.raises(dsa.DsaError) as ei:
                a.matmul_dev(x.data_ptr(), 4, 2, y.data_ptr(), 4, transpose=bool(tr))
            assert ei.value.code == EMODE
            with pytest.raises(dsa.DsaError) as ei:
                hip.call("mat_spmm_dense", a.h, tr, xh.ctypes.data_as(C.POINTER(C.c_double)), 4, 2, 2,
                         yh.ctypes.data_as(C.POINTER(C.c_double)), 4, 2)
            assert ei.value.code == EMODE
        torch.cuda.synchronize()
        assert (y == SENTINEL).all() and (yh == SENTINEL).all()
        return
    assert a.size() == b.size()
    _check(hip, a, b, KS_GOLDEN)


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
    _check(hip, a, b, ks, 1)
    # mixed writes, a quarter of them zeros (deletions)
    I2, J2 = rng.integers(1, m + 1, 3000), rng.integers(1, n + 1, 3000)
    V2 = np.where(rng.random(3000) < 0.25, 0.0, rng.standard_normal(3000))
    for x in (a, b):
        x.set_batch(I2, J2, V2)
    _check(hip, a, b, ks, 2)
    # tombstones in both orientations
    c1, c2 = (int(c) for c in np.unique(J[:20])[:2])
    for x in (a, b):
        x.deletecolumn(c1)
        x.deletecolumn(c2)
        x.deleterow(int(I[5]))
    _check(hip, a, b, ks, 3)
    # new columns, keys in random order
    newc = rng.permutation(np.arange(n + 1, n + 41))
    I3 = rng.integers(1, m + 1, len(newc))
    V3 = rng.standard_normal(len(newc))
    for x in (a, b):
        x.set_batch(I3, newc, V3)
    assert a.size() == b.size() == (m, n + 40)
    _check(hip, a, b, ks, 4)
    # a zero written beyond size(m, 2): an empty partition outside the size
    for x in (a, b):
        x[3, n + 100] = 0.0
    assert a.size() == b.size() and a.size()[1] < n + 100
    _check(hip, a, b, ks, 5)


@pytest.mark.gpu
def test_leading_dimensions_padding_and_empty_rows(dsa, hip, oracle):
    rng = np.random.default_rng(21)
    m, n = 700, 500
    I, J = rng.integers(1, m + 1, 3000), rng.integers(1, n + 1, 3000)
    I[I % 9 == 0] += 1                       # rows 9, 18, ... own no partition
    V = rng.standard_normal(3000)
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    assert a.size() == b.size() == (m, n)
    for transpose, nx, ny in ((False, n, m), (True, m, n)):
        for k in (1, 3, 8, 13, 20):
            X = rng.standard_normal((nx, k))
            exp = _expect(b, transpose, X, ny)
            for got in (_dev(a, transpose, X, ny, k + 3, k + 5), _host(hip, a, transpose, X, ny, k + 3, k + 5)):
                assert got.shape == (ny, k + 5)
                assert (got[:, k:] == SENTINEL).all()
                _same_bits(got[:, :k], exp)
            if not transpose:
                empty = np.setdiff1d(np.arange(1, m + 1), I) - 1
                assert len(empty) >= m // 9
                assert (_bits(got[empty, :k]) == 0).all()          # +0.0: sign bit clear


@pytest.mark.gpu
def test_wide_keys(dsa, hip, oracle):
    # a column key beyond int32: the rowmajor orientation stores int64 keys; nx = 7 leaves the wide cells outside X
    big = (1 << 31) + 5
    I = np.array([1, 2, 3, 3, 4], dtype=np.int64)
    J = np.array([1, 7, 2, big, big], dtype=np.int64)
    V = np.array([1.5, -2.0, 3.25, 4.0, 0.125])
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    rng = np.random.default_rng(31)
    for k in (1, 3, 8, 17):
        X = rng.standard_normal((7, k))
        exp = _expect(b, False, X, 4)
        assert exp[3].tolist() == [0.0] * k                          # row 4 holds a wide cell only
        _same_bits(_dev(a, False, X, 4), exp)
        _same_bits(_host(hip, a, False, X, 4), exp)
        Xt = rng.standard_normal((4, k))                             # A' X: the partition `big` lies outside 1..ny and writes nothing
        _same_bits(_dev(a, True, Xt, 7), _expect(b, True, Xt, 7))
    # int64 key storage with every remaining key inside X: a wide key written and deleted again (the arrays are widened once)
    (I, J), (a, b) = _random_pair(dsa, hip, oracle, rng, 60, 50, 400)
    dims = a.size()
    for x in (a, b):
        x[5, big] = 2.0
        x[5, big] = 0.0
    assert a.size() == b.size() == (dims[0], big)                    # the size keeps the deleted column: X and Y stay dims-sized
    assert int(I.max()) <= dims[0] and int(J.max()) <= dims[1]       # every stored key lies inside X
    _check(hip, a, b, (1, 4, 8, 16), 32, dims=dims)


@pytest.mark.gpu
def test_long_row_among_ordinary_rows(dsa, hip, oracle):
    rng = np.random.default_rng(41)
    m, n, long_row, L = 300, 30000, 7, 20000
    I = np.concatenate([np.full(L, long_row), rng.integers(1, m + 1, 3000)])
    J = np.concatenate([rng.choice(n, L, replace=False) + 1, rng.integers(1, n + 1, 3000)])
    V = rng.random(len(I)) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    assert len(b.row_view(long_row)) >= L
    for k in (1, 8):
        X = rng.random((n, k)) + 0.5
        exp = _expect(b, False, X, m)
        got, again = _dev(a, False, X, m), _dev(a, False, X, m)
        ordinary = np.arange(m) != long_row - 1
        _same_bits(got[ordinary], exp[ordinary])
        rel = np.abs(got[long_row - 1] - exp[long_row - 1]) / exp[long_row - 1]
        print("long row, k = %d: max relative deviation %.3e" % (k, rel.max()))
        assert (rel <= 1e-12).all(), rel
        _same_bits(again, got)                                       # deterministic from run to run
        _same_bits(got, exp)                                         # no length limit: the long row is in reference order too
        Xt = rng.random((m, k)) + 0.5                                # the long row as one cell of 20 000 columns
        _same_bits(_dev(a, True, Xt, n), _expect(b, True, Xt, n))


@pytest.mark.gpu
def test_columns_agree_with_the_single_product(dsa, hip, oracle):
    rng = np.random.default_rng(51)
    (_, _), (a, _b) = _random_pair(dsa, hip, oracle, rng)
    m, n = a.size()
    for transpose, nx in ((False, n), (True, m)):
        X = rng.standard_normal((nx, 6))
        Y = a.matmul(X, transpose=transpose)
        for j in range(6):
            np.testing.assert_allclose(Y[:, j], a.mul(X[:, j].copy(), transpose=transpose), rtol=1e-12, atol=1e-13)


@pytest.mark.gpu
def test_argument_errors_leave_y_untouched(dsa, hip):
    import torch
    a = dsa.dynamicsparse([1, 2, 3], [1, 2, 3], [1.0, 2.0, 3.0], binding=hip)
    x = torch.ones((3, 8), dtype=torch.float64, device="cuda")
    y = torch.full((3, 8), SENTINEL, dtype=torch.float64, device="cuda")
    xh, yh = np.ones((3, 8)), np.full((3, 8), SENTINEL)
    P = C.POINTER(C.c_double)
    torch.cuda.synchronize()
    for k, ldx, ldy in ((0, 8, 8), (4, 3, 8), (4, 8, 3), (-1, 8, 8)):
        rc = hip._mat_spmm_dense_dev(a.h, 0, C.c_void_p(x.data_ptr()), 3, k, ldx, C.c_void_p(y.data_ptr()), 3, ldy)
        assert rc == EARG, (k, ldx, ldy, rc)
        rc = hip._mat_spmm_dense(a.h, 0, xh.ctypes.data_as(P), 3, k, ldx, yh.ctypes.data_as(P), 3, ldy)
        assert rc == EARG, (k, ldx, ldy, rc)
    assert hip._mat_spmm_dense_dev(a.h, 0, C.c_void_p(x.data_ptr()), -1, 2, 8, C.c_void_p(y.data_ptr()), 3, 8) == EARG
    assert hip._mat_spmm_dense_dev(a.h, 0, None, 3, 2, 8, C.c_void_p(y.data_ptr()), 3, 8) == EARG
    assert hip._mat_spmm_dense_dev(a.h, 0, C.c_void_p(x.data_ptr()), 3, 2, 8, None, 3, 8) == EARG
    a.sync()
    torch.cuda.synchronize()
    assert (y == SENTINEL).all() and (yh == SENTINEL).all()
    # empty shapes: ny = 0 launches nothing, nx = 0 zeroes Y
    assert hip._mat_spmm_dense_dev(a.h, 0, C.c_void_p(x.data_ptr()), 3, 2, 8, None, 0, 8) == 0
    assert hip._mat_spmm_dense_dev(a.h, 0, None, 0, 2, 8, C.c_void_p(y.data_ptr()), 3, 8) == 0
    a.sync()
    got = y.cpu().numpy()
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
        for transpose, nx, ny in ((False, n, m), (True, m, n)):
            X = rng.standard_normal((nx, 8))
            _same_bits(_dev(a, transpose, X, ny), _expect(b, transpose, X, ny))      # _dev ends with dsa_mat_sync
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
    exp, expt = _expect(b, False, X, m), _expect(b, True, Xt, n)
    Y = a @ X
    assert isinstance(Y, np.ndarray) and Y.shape == (m, 10)
    _same_bits(Y, exp)
    _same_bits(a.T @ Xt, expt)
    _same_bits(a.transpose().matmul(Xt), expt)
    y1 = a @ X[:, 0].copy()
    assert y1.shape == (m,)
    _same_bits(y1, exp[:, 0])
    np.testing.assert_allclose(y1, a.mul(X[:, 0].copy()), rtol=1e-12, atol=1e-13)
    _same_bits(a @ X[:, ::2], _expect(b, False, X[:, ::2], m))          # not contiguous: copied on the caller's side
    Xd = torch.from_numpy(X).to("cuda")
    Yd = a @ Xd
    assert isinstance(Yd, torch.Tensor) and Yd.is_cuda and Yd.device == Xd.device and tuple(Yd.shape) == (m, 10)
    _same_bits(Yd.cpu().numpy(), exp)
    _same_bits((a @ Xd[:, ::2]).cpu().numpy(), _expect(b, False, X[:, ::2], m))
    _same_bits((a @ Xd[:, 2:7]).cpu().numpy(), _expect(b, False, X[:, 2:7], m))   # a row-strided view goes in as it is (ldx = 10)
    _same_bits((a.T @ torch.from_numpy(Xt).to("cuda")).cpu().numpy(), expt)
    yd1 = a @ Xd[:, 0]
    assert tuple(yd1.shape) == (m,)
    _same_bits(yd1.cpu().numpy(), exp[:, 0])
    with pytest.raises(dsa.DsaArgumentError):
        a @ torch.from_numpy(X)                                          # a CPU tensor
    with pytest.raises(dsa.DsaArgumentError):
        a @ Xd.to(torch.float32)


@pytest.mark.gpu
def test_c3_full_size_exact(dsa, hip):
    """config 3 (1 M x 1 M, 10 M nnz), k = 8, both transposes, bitwise against the numpy walk over to_csr() / to_csc()"""
    sys.path.insert(0, ROOT)
    import bench
    import torch
    m = n = 1_000_000
    I, J, V = bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6)
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    rng = np.random.default_rng(81)
    for transpose, comp in ((False, a.to_csr()), (True, a.to_csc())):
        assert len(comp[1]) == 10_000_000
        X = rng.standard_normal((n, 8))
        exp = _expect(comp, transpose, X, m)
        _same_bits(_dev(a, transpose, X, m), exp)
    torch.cuda.synchronize()
