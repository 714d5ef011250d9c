"""The column-swept SpMV plan at the shapes an x prefetch would have to get right (csrc/spmv.hip: k_spmv_plan).

The prefetch these shapes were chosen for — the waves of an XCD pulling slice s + D of x into L2 while they gather from slice s —
was measured and not kept (it made the product slower at every depth), and its index helper went with it.  What was
kept instead are rounds of one 64-cell chunk with the cell stream one round ahead across the slices.  The shapes stay: a last slice
shorter than the rest, 17 slices, one group, a workgroup count that is no multiple of 8, an x that is only 8-byte aligned, a longer
y, and slices of 0, 1, 63, 64, 65, ... cells, where the next round is the rest of the slice or the start of the next one.  Every
test takes three products, the third from the plan, and compares y byte for byte with a left fold computed here: per row the cells
sorted by column, np.cumsum(v * x[cols])[-1] (numpy multiplies and adds separately and cumsum over a 1-D float64 array is
sequential: the kernel's order).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- helpers (copies of those in tests/test_spmv_plan_stream.py) ----------------------------------------------------------------
def _values(rng, k):
    return rng.integers(1, 1 << 20, k) * 2.0 ** -17


def _x(seed, n):
    return 1.0 + np.random.default_rng(seed).random(n)


def _unique(I, J, n):
    """the distinct (row, column) pairs, in (row, column) order"""
    key = np.unique(np.asarray(I, np.int64) * np.int64(n + 1) + np.asarray(J, np.int64))
    return key // (n + 1), key % (n + 1)


def _left_fold(I, J, V, x, ny):
    """y[row - 1] = ((p0 + p1) + p2) + ... over the row's cells in ascending column order; 0.0 for a row without cells"""
    o = np.lexsort((J, I))
    I, p = np.asarray(I)[o], np.asarray(V)[o] * x[np.asarray(J)[o] - 1]
    y = np.zeros(ny)
    rows, start, cnt = np.unique(I, return_index=True, return_counts=True)
    one = cnt == 1
    y[rows[one] - 1] = p[start[one]]                      # (cumsum of one element)
    for r, a, c in zip(rows[~one], start[~one], cnt[~one]):
        y[r - 1] = np.cumsum(p[a:a + c])[-1]
    return y


def _short_rows(seed, m, n, per_row=3):
    """about per_row cells in every row 1 .. m, none empty, cells in column 1 and in the last row's last column"""
    rng = np.random.default_rng(seed)
    I = np.concatenate([np.arange(1, m + 1), rng.integers(1, m + 1, (per_row - 1) * m), [1, m]])
    J = np.concatenate([rng.integers(1, n + 1, per_row * m), [1, n]])
    return _unique(I, J, n)


def _workgroups(a):
    """workgroups of k_spmv_plan: one wave per group of 4096 slots, four waves per workgroup"""
    groups = (a.info(1)["capacity"] + 4095) // 4096
    return (groups + 3) // 4


def _three_products(a, x, **kw):
    """y of the third product, which the plan computes"""
    i0 = a.info(1)        # ROWMAJOR: the orientation mat * v gathers over
    ys = [a.mul(x, **kw).copy() for _ in range(3)]
    assert a.info(1)["stat_spmv_plan"] - i0["stat_spmv_plan"] > 0
    assert ys[0].tobytes() == ys[1].tobytes()
    return ys[2]


def _check(dsa, hip, m, n, seed, min_workgroups, **kw):
    I, J = _short_rows(seed, m, n)
    V, x = _values(np.random.default_rng(seed + 1), len(I)), _x(seed + 2, n)
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    assert _workgroups(a) >= min_workgroups, a.info(1)["capacity"]
    ny = kw.get("dense_out", m)
    y = _three_products(a, x, **kw)
    assert len(y) == ny and y.tobytes() == _left_fold(I, J, V, x, ny).tobytes()
    return a


# 150 000 rows of three cells fill 2^20 slots or more: 64 workgroups or more, every XCD with several of them
@pytest.mark.parametrize("n", [420_001, 420_015])
def test_last_slice_shorter(dsa, hip, n):
    """width 26 251: the last slice has 26 236 / 26 250 columns, and the last row has a cell in the last column"""
    _check(dsa, hip, 150_000, n, 31, min_workgroups=56)


def test_seventeen_slices(dsa, hip):
    """nx = 1 100 000: 17 slices of 64 706 columns; 300 000 rows of three cells fill 2^21 slots (128 workgroups) or more"""
    _check(dsa, hip, 300_000, 1_100_000, 41, min_workgroups=128)


def test_one_group(dsa, hip):
    """capacity <= 4096: one wave of one workgroup"""
    n = 420_001
    rng = np.random.default_rng(51)
    I, J = _unique(np.repeat(np.arange(1, 201), 5), rng.integers(1, n + 1, 1000), n)
    I, J = _unique(np.concatenate([I, [200]]), np.concatenate([J, [n]]), n)
    V, x = _values(rng, len(I)), _x(52, n)
    a = dsa.dynamicsparse(I, J, V, 200, n, binding=hip)
    assert a.info(1)["capacity"] <= 4096, a.info(1)["capacity"]
    assert _three_products(a, x).tobytes() == _left_fold(I, J, V, x, 200).tobytes()


def test_workgroup_count_not_a_multiple_of_8(dsa, hip):
    """a few groups only: the XCDs hold different numbers of waves, some none"""
    n = 420_015
    I, J = _short_rows(61, 6_000, n)
    V, x = _values(np.random.default_rng(62), len(I)), _x(63, n)
    a = dsa.dynamicsparse(I, J, V, 6_000, n, binding=hip)
    assert _workgroups(a) > 1 and _workgroups(a) % 8 != 0, a.info(1)["capacity"]
    assert _three_products(a, x).tobytes() == _left_fold(I, J, V, x, 6_000).tobytes()


def test_x_aligned_to_8_bytes_only(dsa, hip):
    """x handed over in HBM, 8 bytes behind the start of an (nx + 1)-entry tensor: every slice starts and ends inside a 64-byte line"""
    import torch
    m, n = 150_000, 420_001
    I, J = _short_rows(71, m, n)
    V, x = _values(np.random.default_rng(72), len(I)), _x(73, n)
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    assert _workgroups(a) >= 56
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    hip.call("mat_set_stream", a.h, C.c_void_p(stream.cuda_stream))
    xd = torch.from_numpy(np.concatenate([[0.0], x])).to(dev)       # (copies only: no torch kernel is loaded for this test)
    assert xd.data_ptr() % 64 == 0
    yd = torch.from_numpy(np.zeros(m)).to(dev)
    p0 = a.info(1)["stat_spmv_plan"]
    for _ in range(3):
        hip.call("mat_spmv_dense_dev", a.h, 0, 0, C.c_void_p(xd.data_ptr() + 8), n, C.c_void_p(yd.data_ptr()), m)
    torch.cuda.synchronize()
    assert a.info(1)["stat_spmv_plan"] - p0 > 0
    assert yd.cpu().numpy().tobytes() == _left_fold(I, J, V, x, m).tobytes()


def test_longer_dense_out(dsa, hip):
    """dense_out beyond the last row: the rows behind the last partition are 0.0"""
    m = 150_000
    _check(dsa, hip, m, 420_001, 81, min_workgroups=56, dense_out=m + 3000)


def test_slice_lengths_around_a_chunk(dsa, hip):
    """one group whose slices hold 0, 1, 63, 64, 65, 127, 128, 129, ... cells: a slice that ends with a full round, a round of
    one cell, empty slices between full ones, and the last slice empty"""
    n, m = 420_001, 100
    width = (n + 15) // 16
    counts = [0, 1, 63, 64, 65, 127, 128, 129, 0, 0, 64, 64, 1, 0, 200, 0]
    rng = np.random.default_rng(91)
    I, J = [], []
    for s, c in enumerate(counts):
        lo, hi = s * width + 1, min((s + 1) * width, n)
        cols = rng.choice(np.arange(lo, hi + 1), c, replace=False)       # distinct columns: c distinct cells whatever their rows
        I.append(rng.integers(1, m + 1, c))
        J.append(cols)
    I, J = _unique(np.concatenate(I), np.concatenate(J), n)
    assert len(I) == sum(counts)
    V, x = _values(rng, len(I)), _x(92, n)
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    assert a.info(1)["capacity"] <= 4096, a.info(1)["capacity"]
    assert _three_products(a, x).tobytes() == _left_fold(I, J, V, x, m).tobytes()
