"""The row map of the column-swept SpMV plan (csrc/spmv.hip: k_plan_pass<true>, k_spmv_plan).

The plan keeps, per partition id, the row key clamped to [0, ny + 1] as a 32-bit word, and per group a flag: dense, when its row
keys are consecutive, follow the key in front of the group and leave no row to zero.  A dense group stores acc[i] to
y[row0 - 1 + i] without reading its row map.  Any other group walks its part of the row map, 64 partitions at a time: the row in
front of a lane's row is the entry in front of the lane's own — at a multiple of 64 within the group the last entry of the chunk
before, for the group's first partition the last entry of the group before (0 in front of the table).  Keeping the first 8 * 64
entries in registers instead was measured and not kept; the shapes stay at its bounds: about 60, 250 and 600 rows per group (the
last with groups on both sides of 512, dense and with gaps), a group of more than 1024 rows (no plan: k_spmv_gather), gaps in the
row keys in front of the first partition, at chunk borders, at group borders and behind the last partition, one partition alone,
and writes between products.  Every case takes three products, the third from the plan, and compares y byte for byte with a left fold
computed here: per row the cells sorted by column, np.cumsum(v * x[cols])[-1] (numpy multiplies and adds separately and cumsum over
a 1-D float64 array is sequential: the kernel's order).  Every product goes through the device entry point bench.py calls
(mat_spmv_dense_dev) into a y that was filled with NaN just before: the host entry point keeps one y buffer per handle, which the
two products of k_spmv_gather would leave holding the expected result, zeros included, so that a plan product which stored
nothing would pass.  Here every element of y must have been written by the product under test.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 400_000              # 8 * N bytes of x > 3 MB: the regime where the plan applies
GROUP = 4096             # slots per group (PLAN_GROUP_SLOTS)
REG_ROWS = 8 * 64        # rows per group on both sides of which the shapes lie (eight chunks of 64 partitions)
PLAN_ROWS = 1024         # rows per group the plan accepts


# ---- helpers (copies of those in tests/test_spmv_plan_prefetch.py) --------------------------------------------------------------
def _values(rng, k):
    return rng.integers(1, 1 << 20, k) * 2.0 ** -17


def _x(seed, n=N):
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


# ---- helpers of this file ---------------------------------------------------------------------------------------------------------
def _products(hip, a, x, ny, count):
    """y of `count` products through mat_spmv_dense_dev, each into a device vector pre-filled with NaN; every element written"""
    import torch
    dev = torch.device("cuda:0")
    hip.call("mat_set_stream", a.h, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    xd = torch.from_numpy(x).to(dev)                          # (copies only: no torch kernel is loaded for these tests)
    nan = np.full(ny, np.nan)
    ys = []
    for k in range(count):
        yd = torch.from_numpy(nan).to(dev)
        hip.call("mat_spmv_dense_dev", a.h, 0, 0, C.c_void_p(xd.data_ptr()), len(x), C.c_void_p(yd.data_ptr()), ny)
        torch.cuda.synchronize()
        ys.append(yd.cpu().numpy())
        assert not np.isnan(ys[-1]).any(), (k, int(np.isnan(ys[-1]).sum()))
    return ys


def _three_products(hip, a, x, ny):
    """y of the third product, which the plan computes (the first two: k_spmv_gather; the plan is built behind the second)"""
    i0 = a.info(1)        # ROWMAJOR: the orientation mat * v gathers over
    ys = _products(hip, a, x, ny, 3)
    i1 = a.info(1)
    assert i1["stat_spmv_plan"] - i0["stat_spmv_plan"] == 1 and i1["stat_spmv_plan_builds"] - i0["stat_spmv_plan_builds"] == 1, (i0, i1)
    assert ys[0].tobytes() == ys[1].tobytes()
    return ys[2]


def _rows(seed, rows, per_row):
    """per_row cells (fewer where columns repeat) in every row of `rows`, one of them in column 1 or N"""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, np.int64)
    I = np.concatenate([np.repeat(rows, per_row), rows[:1], rows[-1:]])
    J = np.concatenate([rng.integers(1, N + 1, per_row * len(rows)), [1, N]])
    return _unique(I, J, N)


def _group_of_partition(a):
    """the group (of 4096 slots) that holds each partition's semaphore, in partition order (slot positions count from 1)"""
    sems = a.export_layout(1)["semaphores"]
    assert len(sems) > 0 and np.all(sems > 0) and np.all(np.diff(sems) > 0)
    return (sems - 1) // GROUP


def _rows_per_group(a):
    return np.bincount(_group_of_partition(a))


def _groups(a, ny):
    """per group with partitions: (rows, dense, index within the group of the last partition with absent rows in front of it or
    -1) — dense as the build defines it: keys consecutive from the key in front of the group on, the table's last key == ny"""
    L = a.export_layout(1)
    grp, keys = (L["semaphores"] - 1) // GROUP, L["col_keys"]
    gap = np.concatenate([[keys[0] - 1], np.diff(keys) - 1])
    gap[-1] += ny - keys[-1]                                  # (the fill behind the last partition is its owner's too)
    out = []
    for g in np.unique(grp):
        idx = np.flatnonzero(grp == g)
        holes = np.flatnonzero(gap[idx] > 0)
        out.append((len(idx), len(holes) == 0, int(holes[-1]) if len(holes) else -1))
    return out


# ---- rows per group on both sides of 512 -----------------------------------------------------------------------------------------
def _uniform(seed, m, per_row):
    return _rows(seed, np.arange(1, m + 1), per_row)


def _short_then_long(seed, m_short, m_long, absent):
    """m_short rows of 3 cells, then m_long rows of 9, but the rows in `absent`: the layout spreads the stored entries evenly over
    the slots, so the groups of the first part hold about 2.5 times the rows of the groups of the second part"""
    Ia, Ja = _rows(seed, np.setdiff1d(np.arange(1, m_short + 1), absent), 3)
    Ib, Jb = _rows(seed + 1, np.setdiff1d(np.arange(m_short + 1, m_short + m_long + 1), absent), 9)
    return np.concatenate([Ia, Ib]), np.concatenate([Ja, Jb])


@pytest.mark.parametrize("name, m, lo, hi", [("60", 4_000, 40, 90), ("250", 16_000, 180, 330), ("600", 30_000, 450, 750)])
def test_rows_per_group(dsa, hip, name, m, lo, hi):
    """about 60 / 250 / 600 rows per group (40 / 9 / 3 cells per row).  The first two are dense throughout: one chunk of rows,
    four or five.  The third — its last rows are longer, and 120 rows are absent — has groups with more and with fewer than 512
    rows in one launch, of both kinds dense ones and ones with gaps, and groups with a gap behind their 512th row: the dense ones
    store from their first row on, the others walk the row map"""
    seed = 100 + int(name)
    absent = np.random.default_rng(seed + 4).choice(np.arange(2, m), 120, replace=False)
    I, J = {"60": lambda: _uniform(seed, m, 40), "250": lambda: _uniform(seed, m, 9),
            "600": lambda: _short_then_long(seed, 26_000, 4_000, absent)}[name]()
    V, x = _values(np.random.default_rng(seed + 2), len(I)), _x(seed + 3)
    a = dsa.dynamicsparse(I, J, V, m, N, binding=hip)
    rpg = _rows_per_group(a)
    assert len(rpg) > 4 and lo <= np.median(rpg) <= hi and rpg.max() <= PLAN_ROWS, (len(rpg), np.median(rpg), rpg.max())
    G = _groups(a, m)
    if name == "600":
        for big in (False, True):
            for dense in (False, True):
                assert sum(1 for n, d, _ in G if (n > REG_ROWS) == big and d == dense) >= 2, (big, dense)
        assert sum(1 for n, d, last in G if last >= REG_ROWS) >= 2
    else:
        assert rpg.max() <= REG_ROWS and all(d for _, d, _ in G)
    assert _three_products(hip, a, x, m).tobytes() == _left_fold(I, J, V, x, m).tobytes()


def test_group_of_more_than_1024_rows(dsa, hip):
    """one cell per row: a group holds more rows than the plan accepts.  The build (which fills the row map before it knows)
    reports the plan unusable and every product comes from k_spmv_gather: the same left fold"""
    m = 40_000
    rng = np.random.default_rng(111)
    I, J = np.arange(1, m + 1), rng.integers(1, N + 1, m)
    V, x = _values(rng, m), _x(112)
    a = dsa.dynamicsparse(I, J, V, m, N, binding=hip)
    assert _rows_per_group(a).max() > PLAN_ROWS
    i0 = a.info(1)
    ys = _products(hip, a, x, m, 4)
    i1 = a.info(1)
    assert i1["stat_spmv_plan_builds"] - i0["stat_spmv_plan_builds"] == 1 and i1["stat_spmv_plan"] == i0["stat_spmv_plan"], (i0, i1)
    ref = _left_fold(I, J, V, x, m).tobytes()
    assert all(y.tobytes() == ref for y in ys)


# ---- gaps in the row keys: no group is dense, every zero fill comes from the row map ---------------------------------------------
def test_gaps_at_chunk_and_group_borders(dsa, hip):
    """Two thirds of the rows 6 .. m - 7 are present: absent rows in front of the first partition, between partitions and behind
    the last one up to ny = m + 3000.  Among the gaps are some in front of a group's first partition (prev is the last entry
    of the group before) and some in front of a partition at a multiple of 64 within its group (prev belongs to the chunk before).  Through
    the device entry point, y pre-filled with NaN: every element is written, the zeros included."""
    m, ny = 30_000, 33_000
    rng = np.random.default_rng(121)
    present = np.unique(np.concatenate([rng.choice(np.arange(6, m - 6), (2 * m) // 3, replace=False), [6, m - 7]]))
    I, J = _rows(122, present, 9)
    V, x = _values(rng, len(I)), _x(123)
    a = dsa.dynamicsparse(I, J, V, m, N, binding=hip)
    grp = _group_of_partition(a)
    assert len(grp) == len(present)
    index_in_group = np.arange(len(grp)) - np.searchsorted(grp, grp, side="left")      # (grp ascends with the partition id)
    first = np.flatnonzero((index_in_group == 0) & (grp > grp[0]))      # partitions that open a group, but the first group's
    assert np.bincount(grp).max() <= REG_ROWS and np.bincount(grp).max() > 128
    assert not any(d for _, d, _ in _groups(a, ny))                     # every group has gaps: none takes the dense store
    gap_in_front = np.concatenate([[present[0] - 1], np.diff(present) - 1])
    border = (index_in_group > 0) & (index_in_group % 64 == 0)
    assert np.sum(gap_in_front[first] > 0) >= 3 and np.sum(gap_in_front[first] == 0) >= 3
    assert np.sum(gap_in_front[border] > 0) >= 3 and np.sum(gap_in_front[border] == 0) >= 3
    assert gap_in_front[0] == 5 and ny - present[-1] == 3007

    ref = _left_fold(I, J, V, x, ny)
    assert _three_products(hip, a, x, ny).tobytes() == ref.tobytes()
    absent = np.setdiff1d(np.arange(1, ny + 1), present)
    assert np.all(ref[absent - 1] == 0.0) and np.all(ref[present - 1] > 0.0)


@pytest.mark.parametrize("row, m", [(3, 10), (1, 1)])
def test_one_partition(dsa, hip, row, m):
    """one group, one partition (first partition 0, one row, a table of one entry).  Row 3 of 10: rows 1, 2 in front of it and
    4 .. 10 behind it are zeroed by the lane that stores row 3.  Row 1 of 1: a dense group of one row"""
    rng = np.random.default_rng(131)
    I, J = _unique(np.full(50, row), np.concatenate([rng.integers(1, N + 1, 48), [1, N]]), N)
    V, x = _values(rng, len(I)), _x(132)
    a = dsa.dynamicsparse(I, J, V, m, N, binding=hip)
    inf = a.info(1)
    assert inf["capacity"] <= GROUP and inf["table_len"] == 1, inf
    assert [d for _, d, _ in _groups(a, m)] == [m == 1]
    y = _three_products(hip, a, x, m)
    assert len(y) == m and y.tobytes() == _left_fold(I, J, V, x, m).tobytes()
    assert y[row - 1] > 0.0 and np.all(np.delete(y, row - 1) == 0.0)


# ---- a write drops the plan and its row map -------------------------------------------------------------------------------------
def test_write_between_products(dsa, hip):
    """a[i, j] = v, then addrow of a row key that had no partition: each write drops the plan; the next plan is built with the new
    row map (every partition behind the new one moves up by one id) and the product equals the fold of the matrix as written"""
    m = 20_000
    new_row = 7_777
    rows = np.delete(np.arange(1, m + 1), new_row - 1)
    I, J = _rows(141, rows, 9)
    rng = np.random.default_rng(142)
    V, x = _values(rng, len(I)), _x(143)
    a = dsa.dynamicsparse(I, J, V, m, N, binding=hip)
    assert _three_products(hip, a, x, m).tobytes() == _left_fold(I, J, V, x, m).tobytes()
    t0 = a.info(1)["table_len"]

    k = len(I) // 2
    b0 = a.info(1)["stat_spmv_plan_builds"]
    a[int(I[k]), int(J[k])] = 3.25
    V = V.copy()
    V[k] = 3.25
    assert _three_products(hip, a, x, m).tobytes() == _left_fold(I, J, V, x, m).tobytes()
    assert a.info(1)["stat_spmv_plan_builds"] == b0 + 1

    cols = np.array([11, 4_000, 399_999])
    a.addrow(new_row, cols, np.array([2.0, 3.0, 4.0]))
    I2, J2, V2 = np.concatenate([I, np.full(3, new_row)]), np.concatenate([J, cols]), np.concatenate([V, [2.0, 3.0, 4.0]])
    assert a.info(1)["table_len"] == t0 + 1
    y = _three_products(hip, a, x, m)
    assert a.info(1)["stat_spmv_plan_builds"] == b0 + 2
    ref = _left_fold(I2, J2, V2, x, m)
    assert y.tobytes() == ref.tobytes() and y[new_row - 1] == ref[new_row - 1] > 0.0
