"""The matrix write path strategy by strategy (csrc/matwrite_host.hip): every branch of mat_apply_sets at its thresholds, the delete of
one column or row in its three forms, and single writes with and without tombstones — each on a handle with its own two streams and on
one whose orientations share a stream (sequential instead of side by side).  Tiny shapes; the HIP library against the CPU oracle slot
for slot, with size() and the error code."""
import ctypes as C

import numpy as np
import pytest

from util import SplitMix64, assert_mat_equal, orientation_equal

pytestmark = pytest.mark.gpu

M_ROWS, N_COLS, NNZ = 40, 30, 150
STREAMS = pytest.mark.parametrize("shared", [False, True], ids=["own_streams", "shared_stream"])


def _base_triples():
    """150 seeded entries of a 40 x 30 matrix in which every row and every column holds a cell"""
    g = SplitMix64(2024)
    I = list(range(1, M_ROWS + 1)) + [g.randint(M_ROWS) for _ in range(NNZ - M_ROWS)]
    J = [1 + k % N_COLS for k in range(M_ROWS)] + [g.randint(N_COLS) for _ in range(NNZ - M_ROWS)]
    V = [g.unit12() for _ in range(NNZ)]
    return np.array(I, dtype=np.int64), np.array(J, dtype=np.int64), np.array(V)


BASE = _base_triples()


def share_stream(hip, a):
    import torch
    hip.call("mat_set_stream", a.h, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def pair(dsa, hip, oracle, shared, triples=BASE):
    ms = [dsa.dynamicsparse(*triples, binding=b) for b in (hip, oracle)]
    if shared:
        share_stream(hip, ms[0])
    return ms


def both(dsa, ms, fn):
    """fn on the hip matrix and on the oracle's: the same error code (None: no error) and the same size()"""
    codes = []
    for m in ms:
        try:
            fn(m); codes.append(None)
        except dsa.DsaError as e:
            codes.append(e.code)
    assert codes[0] == codes[1], codes
    assert ms[0].size() == ms[1].size()
    return codes[0]


def mixed_batch(seed, n, rows=None, cols=None):
    """n writes, a quarter of them zeros (deletes); without key lists: rows 1..44 and columns 1..33, a few of them new"""
    g = SplitMix64(seed)
    rows = np.arange(1, M_ROWS + 5) if rows is None else np.asarray(rows)
    cols = np.arange(1, N_COLS + 4) if cols is None else np.asarray(cols)
    I = [int(rows[g.next() % len(rows)]) for _ in range(n)]
    J = [int(cols[g.next() % len(cols)]) for _ in range(n)]
    V = [0.0 if g.next() % 4 == 0 else g.unit12() for _ in range(n)]
    return I, J, V


def _new_column(n):
    return list(range(3, 3 + 2 * n, 2)), [N_COLS + 1] * n, [1.5 + k for k in range(n)]


def _new_row(n):
    return [M_ROWS + 1] * n, list(range(2, 2 + n)), [2.5 + k for k in range(n)]


def _eight_rows_four_columns():
    return [2, 5, 9, 14, 21, 27, 33, 38], [4, 11, 19, 26, 4, 11, 19, 26], [2.5 + k for k in range(8)]


def _square16():
    return list(range(2, 34, 2)), [1 + (7 * k) % 16 for k in range(16)], [0.0 if k % 5 == 0 else 3.5 + k for k in range(16)]


NO_TOMBSTONE_BATCHES = {
    "n200_mixed": lambda: mixed_batch(1, 200),                                       # both orientations through the rounds
    "n16_one_new_column": lambda: _new_column(16),                                   # rounds on rowmajor, sequencer on colmajor
    "n16_one_new_row": lambda: _new_row(16),                                         # the mirror
    "n16_square": _square16,                                                         # 16 rows, 16 columns: the sequencer pair
    "n7": lambda: mixed_batch(2, 7),                                                 # one below the n >= 8 cut
    "n8_eight_rows_four_columns": _eight_rows_four_columns,                          # ni >= 2 * nj && ni >= 8 at its smallest
    "n127": lambda: mixed_batch(3, 127),
    "n128": lambda: mixed_batch(4, 128),                                             # either side of the parallel cut
}


@STREAMS
@pytest.mark.parametrize("name", list(NO_TOMBSTONE_BATCHES))
def test_set_batch_without_tombstones(dsa, hip, oracle, shared, name):
    I, J, V = NO_TOMBSTONE_BATCHES[name]()
    ms = pair(dsa, hip, oracle, shared)
    assert both(dsa, ms, lambda m: m.set_batch(I, J, V)) is None
    assert_mat_equal(*ms)


DEL_COL, DEL_ROW = 15, 20
LIVE_ROWS = [r for r in range(1, M_ROWS + 1) if r != DEL_ROW]
LIVE_COLS = [c for c in range(1, N_COLS + 1) if c != DEL_COL]


def with_tombstones(dsa, hip, oracle, shared, row=True):
    ms = pair(dsa, hip, oracle, shared)
    assert both(dsa, ms, lambda m: m.deletecolumn(DEL_COL)) is None
    if row:
        assert both(dsa, ms, lambda m: m.deleterow(DEL_ROW)) is None
    assert_mat_equal(*ms)
    return ms


@STREAMS
@pytest.mark.parametrize("n", [5, 200])
def test_set_batch_with_tombstones_in_reference_order(dsa, hip, oracle, shared, n):
    """writes to live rows and columns only: no table refuses them; the reference-order loop with the table replay"""
    ms = with_tombstones(dsa, hip, oracle, shared)
    I, J, V = mixed_batch(5 + n, n, LIVE_ROWS, LIVE_COLS)
    assert both(dsa, ms, lambda m: m.set_batch(I, J, V)) is None
    assert_mat_equal(*ms)


@STREAMS
def test_set_batch_of_new_columns_behind_the_last_live_one(dsa, hip, oracle, shared):
    """200 writes into 40 new columns with ascending keys behind column 30 (live) while column 15 is a tombstone: cannot_fail,
    both orientations side by side"""
    ms = with_tombstones(dsa, hip, oracle, shared, row=False)
    g = SplitMix64(9)
    J = [N_COLS + 1 + k // 5 for k in range(200)]
    I = [g.randint(M_ROWS) for _ in range(200)]
    V = [g.unit12() for _ in range(200)]
    assert both(dsa, ms, lambda m: m.set_batch(I, J, V)) is None
    assert_mat_equal(*ms)


@STREAMS
def test_batch_the_rowmajor_table_refuses(dsa, hip, oracle, shared):
    """the first case of test_state_after_a_failed_batch_is_the_references: new row 31 in front of live row 33 while row 105 is a
    tombstone further up.  The same code, the same size() and the same colmajor orientation (it did not refuse) in both stream modes."""
    rng = np.random.default_rng(3)
    keys = np.arange(1, 51, dtype=np.int64) * 3
    I0 = np.repeat(keys, 4); J0 = rng.choice(keys, len(I0))
    V0 = rng.integers(1, 9, len(I0)).astype(np.float64)
    ms = pair(dsa, hip, oracle, shared, (I0, J0, V0))
    for r in (60, 105):
        assert both(dsa, ms, lambda m: m.deleterow(r)) is None
    assert_mat_equal(*ms)
    code = both(dsa, ms, lambda m: m.set_batch([6, 9, 31, 12, 200, 15], [3, 6, 9, 12, 15, 18], [1.5, 0.0, 2.5, 3.5, 4.5, 5.5]))
    assert code == dsa.binding.EASSERT
    assert orientation_equal(ms[0], ms[1], 0), "the orientation that did not refuse the write differs"


def _tables(m):
    return [m.export_layout(o) for o in (0, 1)]


@STREAMS
@pytest.mark.parametrize("what", ["column", "row"])
@pytest.mark.parametrize("case", ["with_cells", "empty", "absent"])
def test_delete_one_partition(dsa, hip, oracle, shared, what, case):
    ms = pair(dsa, hip, oracle, shared)
    column = what == "column"
    delete = (lambda m, k: m.deletecolumn(k)) if column else (lambda m, k: m.deleterow(k))
    key = 11
    if case == "empty":                           # a zero-valued write to a new key creates an empty partition: the pair branch
        key = (N_COLS if column else M_ROWS) + 1
        ij = ([3], [key]) if column else ([key], [3])
        assert both(dsa, ms, lambda m: m.set_batch(ij[0], ij[1], [0.0])) is None
        assert ms[0].nbpartitions(0 if column else 1) == (N_COLS if column else M_ROWS) + 1
        assert_mat_equal(*ms)
    if case == "absent":
        key = 99
        before = _tables(ms[0])
    code = both(dsa, ms, lambda m: delete(m, key))
    if case == "absent":
        assert code == dsa.binding.EARG          # src/pcsr.jl:208
        for La, Lb in zip(before, _tables(ms[0])):      # ... and nothing changed
            for k in ("keys", "vals", "occ", "semaphores", "col_live", "col_keys"):
                assert np.array_equal(La[k], Lb[k]), k
    else:
        assert code is None
    assert_mat_equal(*ms)
    # the tables are usable afterwards: a few writes to what is live, one of them a delete
    assert both(dsa, ms, lambda m: m.set_batch([2, 7, 12, 7, 30], [3, 8, 3, 22, 29], [1.25, 2.25, 0.0, 3.25, 4.25])) is None
    assert_mat_equal(*ms)


@STREAMS
@pytest.mark.parametrize("tombstones", [True, False], ids=["applied_at_once", "queued"])
def test_single_writes_then_a_read(dsa, hip, oracle, shared, tombstones):
    """a[i, j] = v: with tombstones every write is applied in dsa_mat_set, without it is queued until the read"""
    ms = with_tombstones(dsa, hip, oracle, shared) if tombstones else pair(dsa, hip, oracle, shared)
    I, J, V = mixed_batch(77, 12, LIVE_ROWS, LIVE_COLS)
    I.append(4); J.append(N_COLS + 1); V.append(6.5)      # a new column behind the last one
    for i, j, v in zip(I, J, V):
        assert both(dsa, ms, lambda m: m.__setitem__((i, j), v)) is None
    for i, j in zip(I, J):
        assert ms[0][i, j] == ms[1][i, j]
    assert_mat_equal(*ms)
