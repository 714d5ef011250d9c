"""The cell stream of the column-swept SpMV plan at its edges (csrc/spmv.hip: k_spmv_plan).

A wave walks the cells of its group slice by slice, in rounds of 64-cell chunks, and adds the cells of one row one after the other.
The shapes here put rows across chunk and round borders, a row at the last lane of a chunk, runs that end with a partial or an exactly
full round, the last cell of the plan's arrays, column indices up to bit 21, groups with close to 1024 rows, absent rows and a longer
y.  Every test takes three products (the third from the plan), asserts that the plan ran unless it says otherwise, and compares y
byte for byte with a left fold computed here: per row the cells sorted by column, np.cumsum(v * x[cols])[-1].  numpy multiplies and
adds separately and cumsum over a 1-D float64 array is sequential, so that is the kernel's order, and it does not depend on
k_spmv_gather.
"""
import numpy as np
import pytest

N = 420_000              # 8 * N bytes of x > 3 MB: the non-temporal regime, where the plan applies
ROUND = 64 * 8           # two rounds of four chunks (one of eight)

pytestmark = pytest.mark.gpu


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


def _plan_products(a, x, **kw):
    """y of the first product (k_spmv_gather) and of the third one, and how many plan products / builds those three added"""
    i0 = a.info(1)        # ROWMAJOR: the orientation mat * v gathers over
    ys = [a.mul(x, **kw).copy() for _ in range(3)]
    i1 = a.info(1)
    assert ys[0].tobytes() == ys[1].tobytes()
    return ys[0], ys[2], i1["stat_spmv_plan"] - i0["stat_spmv_plan"], i1["stat_spmv_plan_builds"] - i0["stat_spmv_plan_builds"]


def _check(dsa, hip, I, J, V, m, n, x, one_group=False, gather_too=False, **kw):
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    if one_group:
        assert a.info(1)["capacity"] <= 4096, a.info(1)["capacity"]
    y1, y3, plans, _ = _plan_products(a, x, **kw)
    assert plans > 0
    ny = kw.get("dense_out", m)
    assert len(y3) == ny
    assert y3.tobytes() == _left_fold(I, J, V, x, ny).tobytes()
    if gather_too:
        assert y3.tobytes() == y1.tobytes()
    return a, y3


def _short_rows(seed, m, n, per_row=3):
    """about per_row cells in every row 1 .. m, none empty, the last row with a cell in the last column"""
    rng = np.random.default_rng(seed)
    I = np.concatenate([np.arange(1, m + 1), rng.integers(1, m + 1, (per_row - 1) * m), [1, m]])
    J = np.concatenate([rng.integers(1, n + 1, per_row * m), [1, n]])
    return _unique(I, J, n)


def test_order_sensitive_short_rows(dsa, hip):
    m = 100_000
    I, J = _short_rows(1, m, N)
    V = _values(np.random.default_rng(2), len(I))
    _check(dsa, hip, I, J, V, m, N, _x(3), gather_too=True)


def _with_long_rows(seed, m, long_rows, first_col):
    """short rows, and in each of long_rows 150 cells in adjacent columns (one slice) in place of the row's own"""
    I, J = _short_rows(seed, m, N)
    keep = ~np.isin(I, long_rows)
    I, J = I[keep], J[keep]
    Il = np.repeat(long_rows, 150)
    Jl = (np.asarray(first_col)[:, None] + np.arange(150)[None, :]).ravel()
    return _unique(np.concatenate([I, Il]), np.concatenate([J, Jl]), N)


def test_runs_that_cross_chunks_and_rounds(dsa, hip):
    """rows of 150 adjacent cells: ranks up to 63 within a chunk, a row in three chunks and in two rounds"""
    m = 60_000
    rng = np.random.default_rng(4)
    long_rows = np.sort(rng.choice(np.arange(2, m), 40, replace=False))
    first_col = rng.integers(1, 60_000, 40)               # slice 0 of 16
    I, J = _with_long_rows(5, m, long_rows, first_col)
    _check(dsa, hip, I, J, _values(rng, len(I)), m, N, _x(6))


def test_long_row_starting_at_lane_63(dsa, hip):
    """one group whose run starts with 63 cells of row 1, so the 150 cells of row 2 start at lane 63 of the first chunk"""
    m = 8
    I = np.concatenate([np.full(63, 1), np.full(150, 2), np.repeat(np.arange(3, m + 1), 3)])
    J = np.concatenate([np.arange(1, 64), np.arange(101, 251), np.arange(300, 300 + 3 * (m - 2))])      # all in slice 0
    rng = np.random.default_rng(7)
    _check(dsa, hip, I, J, _values(rng, len(I)), m, N, _x(8), one_group=True)


def test_one_partial_chunk(dsa, hip):
    """5 rows x 3 cells: one group, one chunk with 15 cells"""
    rng = np.random.default_rng(9)
    I = np.repeat(np.arange(1, 6), 3)
    J = np.sort(rng.choice(np.arange(1, N + 1), 15, replace=False).reshape(5, 3), axis=1).ravel()
    _check(dsa, hip, I, J, _values(rng, 15), 5, N, _x(10), one_group=True)


def test_run_that_ends_with_a_full_round(dsa, hip):
    """one group whose cell count is a multiple of the round: the last chunk has no idle lane"""
    rng = np.random.default_rng(11)
    m = 200
    I, J = _unique(np.repeat(np.arange(1, m + 1), 5), rng.integers(1, N + 1, 5 * m), N)
    extra = 2 * ROUND - len(I)                            # cells added to the last row: columns behind every other of its cells
    assert 0 < extra <= 150
    I = np.concatenate([I, np.full(extra, m)])
    J = np.concatenate([J, N - np.arange(extra)[::-1]])
    I, J = _unique(I, J, N)
    a, _ = _check(dsa, hip, I, J, _values(rng, len(I)), m, N, _x(12), one_group=True)
    assert a.nnz() == 2 * ROUND, a.nnz()


def test_last_cell_of_the_plan(dsa, hip):
    """several groups; the last cell of the last group's run (last row, last column) is the last cell of the plan's arrays"""
    m = 20_000
    I, J = _short_rows(13, m, N)
    assert I[-1] == m and J[-1] == N
    a, _ = _check(dsa, hip, I, J, _values(np.random.default_rng(14), len(I)), m, N, _x(15))
    assert a.info(1)["capacity"] > 4096


@pytest.mark.parametrize("n", [1_100_000, 2_200_000])
def test_column_bits(dsa, hip, n):
    """17 slices and columns >= 2^20; 34 slices and columns with bit 21 set; cells in column 1 and column n"""
    m = 66_000
    I, J = _short_rows(16, m, n)
    assert J.min() == 1 and J.max() == n and 190_000 <= len(I) <= 210_000
    _check(dsa, hip, I, J, _values(np.random.default_rng(17), len(I)), m, n, _x(18, n))


def test_rows_per_group_near_1024(dsa, hip):
    """500 000 rows of one cell: the build's check on the rows of a group decides whether the plan or k_spmv_gather runs, and
    the row field of a cell and the LDS accumulators rely on that check.  y is the left fold either way."""
    m = 500_000
    rng = np.random.default_rng(19)
    I, J = np.arange(1, m + 1), rng.integers(1, N + 1, m)
    V, x = _values(rng, m), _x(20)
    a = dsa.dynamicsparse(I, J, V, m, N, binding=hip)
    _, y3, _, builds = _plan_products(a, x)
    assert builds > 0
    assert y3.tobytes() == _left_fold(I, J, V, x, m).tobytes()


def test_absent_rows_and_a_longer_y(dsa, hip):
    """gaps in the row keys and dense_out beyond the last row: the rows between partitions and behind the last one are 0.0"""
    m = 90_000
    rng = np.random.default_rng(21)
    present = np.unique(np.concatenate([rng.choice(np.arange(5, m + 1), m // 3, replace=False), [5, m]]))
    I = np.concatenate([present, rng.choice(present, 2 * len(present))])
    I, J = _unique(I, rng.integers(1, N + 1, len(I)), N)
    _, y3 = _check(dsa, hip, I, J, _values(rng, len(I)), m, N, _x(22), dense_out=m + 3000)
    absent = np.setdiff1d(np.arange(1, m + 3001), present)
    assert len(absent) > 60_000 and absent[0] == 1 and absent[-1] == m + 3000
    assert np.all(y3[absent - 1] == 0.0) and np.all(y3[present - 1] > 0.0)
