"""The slot span of the live partition with key k (csrc/find_dev.h: part_span, key_span) at the edges of the table search and of the
tombstone skip, through every caller of the shared lookup: dsa_mat_get, dsa_mat_col_view / dsa_mat_row_view, dsa_mat_select_compressed,
dsa_mat_spmm_selected, dsa_mat_spmv_sparse driven by x, dsa_mat_spgemm_csc.

One matrix per table length T, one or two cells per partition, queried before the deletions (no tombstone: the searches do not read
the liveness bytes) and after them.  T = 4200: the 64-ary search narrows twice; 64 and 65: the narrowing loop is entered only above
64.  The deletions of the long table leave live partitions directly followed by tombstone runs of 1, 63, 64 and 65 entries (the skip
works 64 entries at a time from the entry behind the partition, so a run of 64 ends exactly on a chunk boundary), a tombstoned first
entry, and tombstones from the last live partition to the end of the table (its span ends at the capacity).  Partition keys are the
table positions up to IDENT[T] and 5 more behind it: the table is the identity at some queried positions and not at others (the
direct hit of k_spx_accum), and the 5 keys in between were never written.  `swap` builds the transposed matrix, so the same table is
the row table and is reached through the other orientation of every entry point.

Expected values come from the CPU oracle: its own answers for get, the views and the sparse-x product, and walks over its exported
layout for the rest.  test_oracle_alone checks those walks against the oracle's own product on the CPU, and that the deletions left
the table in the shape described here — tombstones survive to the read: nothing compacts the tables."""
import numpy as np
import pytest

from test_selected_product import _dev as selprod_dev, expected_selected, layout_cells
from test_sparse_x import a_vals, i64, model_mul, x_vals_nz, xdriven
from test_spgemm import assert_same as assert_same_csc, csc_of, expected_csc

COLMAJOR, ROWMAJOR = 0, 1
M_IN = 37                                                   # the inner dimension: rows of the matrix whose column table is walked
LENGTHS = (64, 65, 4200)
IDENT = {64: 40, 65: 40, 4200: 3000}                       # table positions 1..IDENT hold their own index as the key
SHIFT = 5
RUNS = {64: ((10, 1),), 65: ((10, 1),), 4200: ((101, 1), (200, 63), (400, 64), (600, 65))}      # (first position, length) of a tombstone run
TAIL = {64: 3, 65: 3, 4200: 10}                            # tombstoned positions at the end of the table
CASES = [(T, swap) for T in LENGTHS for swap in (False, True)]


def table_keys(T):
    k = np.arange(1, T + 1, dtype=np.int64)
    k[IDENT[T]:] += SHIFT
    return k


def dim_of(T):
    """the outer dimension: wide enough for the queried keys to be few beside it, so that the sparse-x product is driven by x"""
    return max(int(table_keys(T)[-1]), 400)


def deleted_positions(T):
    pos = [1] + [p for first, n in RUNS[T] for p in range(first, first + n)] + list(range(T - TAIL[T] + 1, T + 1))
    return i64(sorted(pos))


def triples(T):
    """(inner key, partition key, value): one cell per partition, a second one in every third"""
    keys = table_keys(T)
    j = np.arange(T, dtype=np.int64)
    two = j[j % 3 == 0]
    inner = np.concatenate([1 + (j * 7) % M_IN, 1 + (two * 7 + 11) % M_IN])
    outer = np.concatenate([keys, keys[two]])
    return inner, outer, a_vals(T, len(outer))


def build(dsa, binding, T, swap):
    inner, outer, V = triples(T)
    dim = dim_of(T)
    if swap:
        return dsa.dynamicsparse(outer, inner, V, dim, M_IN, binding=binding)
    return dsa.dynamicsparse(inner, outer, V, M_IN, dim, binding=binding)


def delete(a, T, swap):
    keys = table_keys(T)
    for p in deleted_positions(T).tolist():
        a.deleterow(int(keys[p - 1])) if swap else a.deletecolumn(int(keys[p - 1]))


def queries(T, after):
    """partition keys to ask for, ascending; `after`: the tombstones are there"""
    keys = table_keys(T)
    dead = set(deleted_positions(T).tolist()) if after else set()
    live = [p for p in range(1, T + 1) if p not in dead]
    pos = {live[0], live[-1], 50 if T > 64 else 20, IDENT[T], IDENT[T] + 1, T // 2, 1, T}      # first / last live, identity or not, deleted ends
    for first, n in RUNS[T]:
        pos |= {first - 1, first, first + n // 2, first + n - 1, first + n}                    # both sides of the run and inside it
    q = {int(keys[p - 1]) for p in pos}
    q |= {IDENT[T] + 2, -3, 0, dim_of(T) + 7}           # never written between two live keys, below 1, above the dimension
    return i64(sorted(q))


def orientation(swap):
    return ROWMAJOR if swap else COLMAJOR


def assert_table_shape(L, T, after):
    """the walked table is what the module docstring says"""
    live = L["col_live"].astype(bool)
    assert len(live) == T and L["info"]["table_len"] == T
    dead = deleted_positions(T) if after else i64([])
    want = np.ones(T, dtype=bool)
    want[dead - 1] = False
    assert np.array_equal(live, want) and np.array_equal(L["semaphores"] != 0, want)
    assert np.array_equal(L["col_keys"][live], table_keys(T)[want])
    if not after:
        return
    assert not live[0] and not live[-TAIL[T]:].any() and live[-TAIL[T] - 1]
    edges = np.flatnonzero(np.diff(np.concatenate(([1], live.astype(np.int8), [1]))))           # starts and ends of the tombstone runs
    runs = (edges[1::2] - edges[0::2]).tolist()
    assert runs == [1] + [n for _, n in RUNS[T]] + [TAIL[T]], runs
    if T > 4096:
        assert {1, 63, 64, 65} <= set(runs)


def expected_select(L, sel, base=0):
    """(ptr, idx, val) of the selected export of the keys `sel` from the oracle's layout"""
    outer, idx, val = layout_cells(L)
    lo, hi = np.searchsorted(outer, sel, side="left"), np.searchsorted(outer, sel, side="right")
    ptr = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
    pos = np.repeat(lo - ptr[:-1], hi - lo) + np.arange(ptr[-1])
    return ptr + base, idx[pos] + base, val[pos]


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def get_queries(T, q):
    """(inner, outer) of the cells to read: the first cell of each queried partition's position and an inner key it does not hold"""
    keys = table_keys(T)
    pos = np.searchsorted(keys, q)
    pos = np.minimum(pos, T - 1)
    inner = 1 + (pos * 7) % M_IN
    return np.concatenate([inner, inner % M_IN + 1]), np.concatenate([q, q])


class Reference:
    """everything the GPU test compares with, computed once per (T, swap, after) on the oracle"""

    def __init__(self, b, T, swap, after):
        self.q = q = queries(T, after)
        self.L = L = b.export_layout(orientation(swap))
        dim = dim_of(T)
        self.inside = q[(q >= 1) & (q <= dim)]
        gi, go = get_queries(T, q)
        self.get_args = (go, gi) if swap else (gi, go)
        self.get = b.get_batch(*self.get_args)
        self.views = [(b.row_view if swap else b.col_view)(int(k)) for k in q.tolist()]
        self.select = expected_select(L, self.inside)
        self.X = np.random.default_rng(T).standard_normal((M_IN, 3))
        self.selprod = expected_selected(L, q, self.X)
        self.xv = x_vals_nz(T, len(self.inside))
        assert xdriven(len(self.inside), dim)
        self.mul = b.mul((self.inside, self.xv), transpose=swap)
        self.cols = [(i64([k]), np.array([v])) for k, v in zip(self.inside.tolist(), self.xv.tolist())]
        self.csc = expected_csc(L, self.cols)


_refs = {}


def references(dsa, oracle, T, swap):
    """[before the deletions, after them]; kept for the module, never modified"""
    if (T, swap) not in _refs:
        b = build(dsa, oracle, T, swap)
        before = Reference(b, T, swap, False)
        delete(b, T, swap)
        _refs[(T, swap)] = (before, Reference(b, T, swap, True), b.nbpartitions(orientation(swap)))
    return _refs[(T, swap)]


@pytest.mark.parametrize("T,swap", CASES)
def test_oracle_alone(dsa, oracle, T, swap):
    before, after, nparts = references(dsa, oracle, T, swap)
    assert nparts == T - len(deleted_positions(T))
    for R, aft in ((before, False), (after, True)):
        assert_table_shape(R.L, T, aft)
        outer, idx, val = layout_cells(R.L)
        cells = {}
        for o, i, v in zip(outer.tolist(), idx.tolist(), val.tolist()):
            cells.setdefault(o, []).append((i + 1, v))
        assert [sorted(v) for v in R.views] == [sorted(cells.get(k, [])) for k in R.q.tolist()]
        inner, out = (R.get_args[1], R.get_args[0]) if swap else R.get_args
        ok = out >= 1                                       # (an inner key 0 is the semaphore's: the reference finds it, src/pcsr.jl:23)
        assert R.get[ok].tolist() == [dict(cells.get(o, [])).get(i, 0.0) for i, o in zip(inner[ok].tolist(), out[ok].tolist())]
        im, vm, _, exact = model_mul(R.L, R.inside, R.xv)
        assert exact and np.array_equal(im, R.mul[0]) and np.array_equal(bits(vm), bits(R.mul[1]))
        hit = np.array([k in cells for k in R.q.tolist()])
        assert np.all(bits(R.selprod[~hit]) == 0) and hit.any() and (~hit).any()
        assert R.select[0][-1] == sum(len(cells.get(k, [])) for k in R.inside.tolist())
    # the deletions took cells away: a deleted key is a hit before and a miss after
    assert len(after.select[1]) < len(before.select[1]) and len(after.mul[0]) <= len(before.mul[0])


def check(a, R, T, swap, after):
    o = orientation(swap)
    q = R.q
    assert np.array_equal(bits(a.get_batch(*R.get_args)), bits(R.get))
    for k, want in zip(q.tolist(), R.views):
        got = (a.row_view if swap else a.col_view)(k)
        assert [c[0] for c in got] == [c[0] for c in want] and np.array_equal(bits([c[1] for c in got]), bits([c[1] for c in want])), k
    got = (a.select_rows if swap else a.select_columns)(R.inside)
    assert np.array_equal(got[0], R.select[0]) and np.array_equal(got[1], R.select[1]) and np.array_equal(bits(got[2]), bits(R.select[2]))
    # the selected product reads the orientation whose partitions are the result's rows: A[:, q]' X for the column table
    # (the device form takes every key; the host form refuses keys below 1)
    y = selprod_dev(a, not swap, q, R.X)
    full = a.matmul(R.X, transpose=not swap)
    assert np.array_equal(bits(y), bits(R.selprod))
    assert np.array_equal(bits(a.matmul_selected(q[q >= 1], R.X, transpose=not swap)), bits(R.selprod[q >= 1]))
    dim = full.shape[0]
    ins = (q >= 1) & (q <= dim)
    assert np.array_equal(bits(y[ins]), bits(full[q[ins] - 1])) and np.all(bits(y[~ins]) == 0)
    yi, yv = a.mul((R.inside, R.xv), transpose=swap)
    assert np.array_equal(yi, R.mul[0])
    np.testing.assert_allclose(yv, R.mul[1], rtol=1e-12, atol=0)
    got = a.matmul_sparse(csc_of(R.cols), transpose=swap)
    assert np.array_equal(got[0], R.csc[0]) and np.array_equal(got[1], R.csc[1])
    np.testing.assert_allclose(got[2], R.csc[2], rtol=1e-12, atol=0)
    assert_same_csc(got, R.csc, 0, (T, swap))               # no float atomics in that product: the bits agree as well
    assert_table_shape(a.export_layout(o), T, after)


@pytest.mark.gpu
@pytest.mark.parametrize("T,swap", CASES)
def test_every_caller_of_the_lookup(dsa, hip, oracle, T, swap):
    before, after, nparts = references(dsa, oracle, T, swap)
    a = build(dsa, hip, T, swap)
    assert a.nbpartitions(orientation(swap)) == T
    check(a, before, T, swap, False)
    delete(a, T, swap)
    assert a.nbpartitions(orientation(swap)) == nparts == T - len(deleted_positions(T))
    check(a, after, T, swap, True)
