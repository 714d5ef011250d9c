"""The sparse-x product dsa_mat_spmv_sparse* (csrc/sparsex.hip, csrc/sparsex_host.hip, the value and the count pass of gather_tile in
csrc/spmv.hip) at the edges of both strategies, against the reference's _mul (src/operations.jl:62-135).

Every case is a SCRIPT: a generator that builds a matrix on the binding it is given, changes it, and yields the products to take,
(matrix, xi, xv, transpose, note).  The CPU half drives each script on the oracle and checks, per product, a plain numpy model of _mul
over the exported layout against ora_mat_spmv_sparse, and that the inputs sum exactly in any order.  The GPU half drives the same script
on the HIP library and on the oracle side by side and demands EQUAL rows and EQUAL values — no tolerance anywhere in this file.

Exactness: A values are integers in [-2^10, 2^10] times 2^-8, x values integers in [-2^6, 2^6] times 2^-6, so every product is an integer
multiple of 2^-14 and a row whose sum of |products| stays below 2^53 such units has one sum whatever the order of the additions (the fp64
atomics of k_spx_accum add in any order).  Non-finite cases: NaN compares with NaN, +-Inf by sign (np.array_equal(equal_nan=True)), the
finite values beside them for equality.

Strategies are reached by shape: 8 nx < ncols is driven by x's entries, 8 nx >= ncols densifies x and gathers over the twin."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from util import splitmix_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_I64, P_F64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
COLMAJOR, ROWMAJOR = 0, 1
UNIT = 2.0 ** -14          # every finite product is a multiple of this


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------
def a_vals(seed, n):
    """integers in [-2^10, 2^10] \\ {0} times 2^-8 (a zero would not be stored)"""
    k = (splitmix_array(seed, n) % np.uint64(2049)).astype(np.int64) - 1024
    k[k == 0] = 1
    return k.astype(np.float64) * 2.0 ** -8


def x_vals(seed, n):
    """integers in [-2^6, 2^6] times 2^-6; every fifth one a STORED zero (it still touches its rows, src/operations.jl:101)"""
    k = (splitmix_array(seed, n) % np.uint64(129)).astype(np.int64) - 64
    k[::5] = 0
    return k.astype(np.float64) * 2.0 ** -6


def x_vals_nz(seed, n):
    """x_vals without the stored zeros (2^-6 in their place)"""
    v = x_vals(seed, n)
    v[v == 0.0] = 2.0 ** -6
    return v


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def xdriven(nx, ncols):
    """csrc/sparsex_host.hip: spx_xdriven"""
    return nx * 8 < max(ncols, 1)


# ---- the model: _mul over the exported layout --------------------------------------------------------------------------------------
def model_mul(L, xi, xv):
    """src/operations.jl:62-135 on mat_export_layout's arrays, partition by partition: for every stored entry of x whose key is a live
    column key, the occupied slots between that column's semaphore and the next live one, result[row] += x_j * a in slot order.
    Returns (touched rows ascending, their values, per row the sum of |products| in units of 2^-14, all products multiples of 2^-14)."""
    live = np.nonzero(L["col_live"])[0]
    lkeys = L["col_keys"][live]
    sem = L["semaphores"][live]                              # 1-based slot of each live column's semaphore
    assert np.all(sem > 0) and np.all(np.diff(sem) > 0) and np.all(np.diff(lkeys) > 0)
    cap = len(L["occ"])
    end = np.append(sem[1:] - 1, cap)                        # last slot (1-based) of each live partition
    acc, mag, exact = {}, {}, True
    pos = np.searchsorted(lkeys, xi)
    for e in np.nonzero((pos < len(lkeys)) & (lkeys[np.minimum(pos, len(lkeys) - 1)] == xi))[0] if len(lkeys) else ():
        p = pos[e]
        sl = slice(sem[p], end[p])                           # 0-based slots sem[p] .. end[p] - 1 = 1-based sem[p] + 1 .. end[p]
        o = L["occ"][sl].astype(bool)
        rows = L["keys"][sl][o]
        with np.errstate(invalid="ignore"):
            prods = xv[e] * L["vals"][sl][o]
        for r, q in zip(rows.tolist(), prods.tolist()):
            acc[r] = acc.get(r, 0.0) + q
            if np.isfinite(q):
                u = abs(q) / UNIT
                exact = exact and u == int(u)
                mag[r] = mag.get(r, 0) + int(u)
    rows = np.array(sorted(acc), dtype=np.int64)
    return rows, np.array([acc[r] for r in rows.tolist()], dtype=np.float64), max(mag.values(), default=0), exact


def model_mul_fast(L, xi, xv):
    """the same walk with numpy doing the loops (the long cases): slot -> live partition in front of it -> x entry of its key;
    np.add.at adds in slot order, which is the order of the walk above"""
    live = np.nonzero(L["col_live"])[0]
    lkeys = L["col_keys"][live]
    sem = L["semaphores"][live]
    assert np.all(sem > 0) and np.all(np.diff(sem) > 0) and np.all(np.diff(lkeys) > 0)
    slots = np.nonzero(L["occ"])[0] + 1
    part = np.searchsorted(sem, slots, side="right") - 1
    cell = part >= 0
    cell[cell] = sem[part[cell]] != slots[cell]
    slots, part = slots[cell], part[cell]
    ck = lkeys[part]
    e = np.searchsorted(xi, ck)
    hit = e < len(xi)
    hit[hit] = xi[e[hit]] == ck[hit]
    rows_all = L["keys"][slots[hit] - 1]
    rows, inv = np.unique(rows_all, return_inverse=True)
    vals = np.zeros(len(rows))
    with np.errstate(invalid="ignore"):
        prods = xv[e[hit]] * L["vals"][slots[hit] - 1]
        np.add.at(vals, inv, prods)
    fin = np.isfinite(prods)
    units = np.abs(prods[fin]) / UNIT
    mag = np.zeros(len(rows))
    np.add.at(mag, inv[fin], units)
    return rows.astype(np.int64), vals, int(mag.max()) if len(mag) else 0, bool(np.all(units == np.rint(units)))


# ---- scripts ----------------------------------------------------------------------------------------------------------------------
# mk(I, J, V, m, n) builds a matrix on the binding under test.  A script yields (matrix, xi, xv, transpose, note); whatever it does to
# the matrix between two yields happens on both sides.  `note`: "finite" (default: the oracle's values must be finite) or "nonfinite".
EDGE_ROWS = (1, 2, 63, 64, 65, 128, 4095, 4096, 4097, 8192, 65535, 65536, 65537, 69632, 4 * 2 ** 20, 4 * 2 ** 20 + 1)


def edge_matrix(m, full_tile_at=None):
    """a few hundred cells in the columns 1..40 of an m x 64 matrix: the first and the last row of the matrix, of 64-row words and of
    4096-row tiles, some rows in between; the columns 41..64 stay absent; column 40 holds the row m alone.  full_tile_at: all 4096 rows
    of that tile (0-based) in column 39: full 64-bit masks in the emit kernel."""
    rows = sorted({r for r in EDGE_ROWS if r <= m} | {m, max(m - 1, 1), max(m - 63, 1), max(m - 64, 1)} |
                  {int(r) for r in 1 + splitmix_array(5 + m, 40) % np.uint64(m)})
    I, J = [], []
    for k, r in enumerate(rows):
        for c in {1 + k % 7, 8 + k % 11, 20 + k % 18}:
            I.append(r); J.append(c)
    I.append(m); J.append(40)
    if full_tile_at is not None:
        I += list(range(full_tile_at * 4096 + 1, full_tile_at * 4096 + 4097)); J += [39] * 4096
    I, J = i64(I), i64(J)
    return I, J, a_vals(77 + m, len(I))


def s_bitmap_edges(m, full_tile_at=None):
    def script(mk):
        I, J, V = edge_matrix(m, full_tile_at)
        a = mk(I, J, V, m, 64)
        xs = [i64([40]),                                              # exactly one touched row (m), driven by x
              i64([41]),                                              # no touched row: an absent column
              i64([1, 3, 8, 20, 37, 39, 40]),                         # 7 entries: driven by x
              i64(range(41, 49)),                                     # 8 absent columns: gather, no touched row
              i64(list(range(40, 48))),                               # gather, exactly one touched row
              i64(range(1, 41)),                                      # gather, everything
              i64(range(2, 64, 2))]
        for q, xi in enumerate(xs):
            yield a, xi, (x_vals_nz if len(xi) == 1 else x_vals)(300 + q, len(xi)), False, "finite"
        # transpose(A) * x: x over the rows; a handful of edge rows (driven by x where 8 nx < m), every eighth row and the edges (gather)
        few = i64(sorted({r for r in (1, 64, 65, 4096, 4097, m) if r <= m}))
        many = np.union1d(np.arange(1, m + 1, 8, dtype=np.int64), few)
        for q, xi in enumerate((few, many)):
            yield a, xi, x_vals(310 + q, len(xi)), True, "finite"
    return script


def landing_matrix():
    """300000 x 100000, one or two cells per row.  Rows 1..8192: cell (r, r) and, for even r < 8192, a second one at (r, r + 1) — the
    columns 1..d hold exactly the rows 1..d.  Rows 8193..300000: 64 rows per column from column 8193 on.  Columns above 20000 are absent."""
    d = np.arange(1, 8193, dtype=np.int64)
    ev = np.arange(2, 8192, 2, dtype=np.int64)
    blk = np.arange(8193, 300001, dtype=np.int64)
    I = np.concatenate([d, ev, blk])
    J = np.concatenate([d, ev + 1, 8193 + (blk - 8193) // 64])
    return I, J, a_vals(9, len(I)), 300000, 100000


def landing_x(count, gather):
    """x whose product touches exactly `count` rows: b whole block columns and d diagonal ones; gather: 12500 absent columns on top"""
    b = max(0, (count - 4000) // 64)
    d = count - 64 * b
    assert 0 < d <= 8192 and b <= (300000 - 8192) // 64
    xi = np.concatenate([np.arange(1, d + 1, dtype=np.int64), np.arange(8193, 8193 + b, dtype=np.int64)])
    if gather:
        xi = np.concatenate([xi, np.arange(50001, 62501, dtype=np.int64)])
    assert xdriven(len(xi), 100000) != gather
    return xi


LANDING_COUNTS = (4095, 4096, 4097, 32768, 32769, 131073, 262145)


def s_landing(mk):
    a = mk(*landing_matrix())
    for q, count in enumerate(LANDING_COUNTS):
        for gather in (False, True):
            xi = landing_x(count, gather)
            yield a, xi, x_vals(40 + q, len(xi)), False, "finite count=%d" % count
        xi = np.arange(1, count + 1, dtype=np.int64)             # transpose: the first `count` rows
        yield a, xi, x_vals(60 + q, len(xi)), True, "finite"


def sprinkle(m, n, cnt, seed):
    I = 1 + (splitmix_array(seed, cnt) % np.uint64(m)).astype(np.int64)
    J = 1 + (splitmix_array(seed + 1, cnt) % np.uint64(n)).astype(np.int64)
    IJ = np.unique(np.stack([I, J], axis=1), axis=0)
    return IJ[:, 0].copy(), IJ[:, 1].copy(), a_vals(seed + 2, len(IJ))


def x_with(cols, n, nx):
    """nx ascending column indices out of 1..n that include `cols`"""
    step = max(n // nx, 1)
    base = np.arange(1, n + 1, step, dtype=np.int64)[:nx]
    xi = np.union1d(base, cols)
    drop = np.setdiff1d(xi, cols)[: len(xi) - nx]
    xi = np.setdiff1d(xi, drop)
    assert len(xi) == nx, (len(xi), nx)
    return xi


def s_upload(mk):
    """x of 4096 / 4097 entries (read straight from pinned memory / copied) driven by x; 65535 / 65536 / 65537 entries (plain / threaded
    upload) under both strategies"""
    for n, nxs in ((40000, (4096, 4097)), (524289, (65535, 65536)), (524288, (65536, 65537))):
        I, J, V = sprinkle(5000, n, 400, 1000 + n)
        for swap in (False, True):                                 # swap: the same x against the transposed matrix, transpose(A') * x
            a = mk(J, I, V, n, 5000) if swap else mk(I, J, V, 5000, n)
            for nx in nxs:
                xi = x_with(np.unique(J)[::2], n, nx)
                yield a, xi, x_vals(nx, nx), swap, "finite %s" % ("xdriven" if xdriven(nx, n) else "gather")
            xi = np.unique(I)[::3]
            yield a, xi, x_vals(n, len(xi)), not swap, "finite"


def order_check_inputs():
    """(nx, i, kind): an equal or a descending pair at i (xi[i] against xi[i - 1]) — the plain check and the four threads' check"""
    out = []
    for nx in (1000, 65537):
        part = (nx + 3) // 4
        for i in sorted({1, nx - 1} | ({part, 2 * part, 3 * part} if nx >= 65536 else set())):
            out += [(nx, i, "equal"), (nx, i, "descending")]
    return out


def table_cases():
    """(name, n, live column keys, keys to delete afterwards, queries): the column tables of k_spx_accum's search.  One cell per column
    unless the script says otherwise; n is large enough for every query set to be driven by x."""
    cases = []

    def add(name, keys, deleted=(), extra=()):
        keys = i64(keys)
        deleted = i64(deleted)
        livek = np.setdiff1d(keys, deleted)
        q = {int(livek[0]) - 1, int(livek[-1]) + 1, int(livek[0]), int(livek[-1]), int(livek[len(livek) // 2])} | {int(k) for k in deleted[:3]} | \
            {int(k) for k in deleted[-2:]} | {int(k) for k in extra}
        gaps = np.nonzero(np.diff(livek) > 1)[0]
        if len(gaps):
            q.add(int(livek[gaps[len(gaps) // 2]]) + 1)                                   # absent between two live keys
        n = max(int(keys[-1]) + 10, 8 * (len(q) + 2) + 1)
        cases.append((name, n, keys, deleted, i64(sorted(q))))

    add("identity_last_column", range(1, 301), extra=(300, 299, 150))
    add("deleted_neighbours", range(1, 501), deleted=[11] + list(range(100, 300)), extra=(10, 12, 99, 300, 301))
    add("even_keys", range(2, 802, 2), extra=(2, 3, 4, 400, 401))
    add("identity_then_gap", list(range(1, 1001)) + list(range(2000, 2101)), extra=(1000, 1001, 1500, 1999, 2000, 2050))
    for T in (1, 64, 65, 66, 129, 4097, 262145):
        add("even_keys_len_%d" % T, np.arange(1, T + 1, dtype=np.int64) * 2, extra=(2, 2 * T, 2 * (T // 2 + 1), 2 * T - 1))
        add("identity_len_%d" % T, np.arange(1, T + 1, dtype=np.int64), extra=(1, T, T // 2 + 1))
    add("even_keys_deleted_runs", np.arange(1, 4098, dtype=np.int64) * 2, deleted=np.arange(1000, 1400, 2), extra=(998, 1400, 1402, 8194))
    return cases


def s_tables(swap):
    """swap: the same tables as ROW tables of the transposed matrix, walked by transpose(A) * x"""
    def script(mk):
        for name, n, keys, deleted, q in table_cases():
            m = 50
            I = 1 + (np.arange(len(keys), dtype=np.int64) * 7) % m
            V = a_vals(len(keys), len(keys))
            a = mk(keys, I, V, n, m) if swap else mk(I, keys, V, m, n)
            for k in deleted.tolist():
                a.deleterow(k) if swap else a.deletecolumn(k)
            assert xdriven(len(q), n), name
            yield a, q, x_vals_nz(len(q), len(q)), swap, "finite " + name
        if not swap:
            # a column key below 1 in front: every index of the table is one off the identity
            I, J, V = sprinkle(50, 400, 300, 31)
            a = mk(I, J, V, 50, 400)
            a[5, -3] = 2.0
            for xi in (i64([-4, -3, 1, 2, 400]), i64([-3, 0, 7, 399, 401])):
                yield a, xi, x_vals_nz(5, 5), False, "finite key_below_1"
    return script


def s_column_lengths(swap):
    def script(mk):
        lens = {1: 1, 2: 63, 3: 64, 4: 65, 5: 1000, 6: 1, 7: 1000}
        I = np.concatenate([np.arange(1, c + 1, dtype=np.int64) * 2 - 1 for c in lens.values()])
        J = np.concatenate([np.full(c, k, dtype=np.int64) for k, c in lens.items()])
        V = a_vals(8, len(I))
        a = mk(J, I, V, 100, 2000) if swap else mk(I, J, V, 2000, 100)
        x = i64([1, 2, 3, 4, 5, 6, 7, 8])
        yield a, x, x_vals_nz(1, 8), swap, "finite"
        # column 6: live and empty; column 7: half of its cells deleted just before the product
        gone = np.arange(1, 1001, 2, dtype=np.int64) * 2 - 1
        if swap:
            a[6, 1] = 0.0
            a.set_batch(np.full(len(gone), 7), gone, np.zeros(len(gone)))
        else:
            a[1, 6] = 0.0
            a.set_batch(gone, np.full(len(gone), 7), np.zeros(len(gone)))
        yield a, x, x_vals_nz(2, 8), swap, "finite"
        yield a, i64([6]), np.array([0.5]), swap, "finite"
    return script


def s_boundary(n):
    def script(mk):
        I, J, V = sprinkle(n, n, min(6 * n, 30000), 500 + n)
        a = mk(I, J, V, n, n)
        assert n % 8 == 0 and n >= 16
        counts = [n // 8, n // 8 - 1]                              # gather, driven by x
        for k in range(8):
            nx = counts[k % 2]
            tr = bool((k // 2) % 2)
            xi = np.unique(1 + (splitmix_array(900 + k, 4 * nx) % np.uint64(n)).astype(np.int64))[:nx]
            assert len(xi) == nx
            yield a, xi, x_vals(910 + k, nx), tr, "finite %s" % ("xdriven" if xdriven(nx, n) else "gather")
    return script


def s_changes(mk):
    """the zero invariant of acc / bm across changes of the matrix, alternating strategies"""
    m, n = 6000, 800
    I, J, V = sprinkle(m, n, 5000, 71)
    a = mk(I, J, V, m, n)
    few, many = np.arange(3, 603, 7, dtype=np.int64), np.arange(1, 801, 2, dtype=np.int64)
    assert xdriven(len(few), n) and not xdriven(len(many), n)

    def products(seed):
        for q, (xi, tr) in enumerate(((few, False), (many, False), (few * 9, True), (many, False))):
            yield a, xi, x_vals(seed + q, len(xi)), tr, "finite"
    yield from products(1)
    I2, J2, V2 = sprinkle(m, n, 700, 72)
    a.set_batch(I2, J2, V2)
    yield from products(2)
    a.deletecolumn(17); a.deletecolumn(5)
    yield from products(3)
    a.deleterow(23); a.deleterow(int(I[0]))
    yield from products(4)
    a[2 * m, 3] = 0.75                                             # m grows past the scratch's rows_cap = max(m + m / 4, 4096)
    a[2 * m, 400] = -0.25
    yield from products(5)


def nonfinite_small():
    """the 4 x 16 case of the issue"""
    return i64([2, 2, 3, 3]), i64([1, 9, 2, 9]), np.array([1.0, np.inf, 2.0, np.nan]), 4, 16


def s_nonfinite_small(mk):
    a = mk(*nonfinite_small())
    yield a, i64([1, 2, 3]), np.array([1.5, 0.0, 2.0]), False, "nonfinite absent gather"          # rows [2, 3], values [1.5, 0.0]
    yield a, i64([1]), np.array([1.5]), False, "nonfinite absent xdriven"
    yield a, i64([1, 9]), np.array([1.5, 1.0]), False, "nonfinite stored gather"
    yield a, i64([9]), np.array([0.0]), False, "nonfinite stored xdriven"
    yield a, i64([2, 3]), np.array([1.0, 0.5]), True, "nonfinite"
    yield a, i64([1, 2]), np.array([1.5, -2.0]), False, "finite"


def s_nonfinite_tile(mk):
    """5000 x 4096: +Inf / -Inf / NaN of A around the tile border, in the columns 4001..4003; rows 4090 and 4100 hold nothing else"""
    m, n = 5000, 4096
    I, J, V = sprinkle(m, 4000, 3000, 91)
    keep = (I != 4090) & (I != 4100)
    I, J, V = I[keep], J[keep], V[keep]
    nf_rows = i64([4090, 4095, 4096, 4097, 4098, 4100, 1, 5000])
    Inf = np.inf
    nI = np.concatenate([nf_rows, nf_rows, nf_rows])
    nJ = np.concatenate([np.full(8, 4001), np.full(8, 4002), np.full(8, 4003)])
    nV = np.concatenate([[Inf, -Inf, np.nan, Inf, -Inf, np.nan, Inf, -Inf], [Inf, Inf, 1.0, -Inf, -Inf, 0.5, -Inf, np.nan], [np.nan] + [0.25] * 7])
    a = mk(np.concatenate([I, nI]), np.concatenate([J, nJ]), np.concatenate([V, nV]), m, n)
    few = np.arange(2, 3000, 9, dtype=np.int64)
    many = np.arange(1, 4001, 4, dtype=np.int64)
    assert xdriven(len(few) + 3, n) and not xdriven(len(many), n)
    nf = i64([4001, 4002, 4003])
    for q, base in enumerate((few, many)):
        yield a, base, x_vals(20 + q, len(base)), False, "nonfinite absent"           # x does not store the columns: finite rows only
        xi = np.concatenate([base, nf])
        yield a, xi, np.concatenate([x_vals(22 + q, len(base)), [1.0, -0.5, 0.0]]), False, "nonfinite stored"      # 0.0 * NaN, Inf sums
        yield a, xi, np.concatenate([x_vals(24 + q, len(base)), [0.0, -0.0, 2.0]]), False, "nonfinite stored zero times Inf"
        xv = x_vals(26 + q, len(base))
        xv[3], xv[10], xv[11], xv[12] = np.inf, np.nan, -0.0, -np.inf
        yield a, base, xv, False, "nonfinite x"
        yield a, base, x_vals(28 + q, len(base)), False, "nonfinite absent"           # after NaN results: finite rows exact again
    rows = np.union1d(np.arange(1, 5001, 6, dtype=np.int64), nf_rows)
    yield a, rows, x_vals(30, len(rows)), True, "nonfinite"
    yield a, np.sort(nf_rows), x_vals_nz(31, len(nf_rows)), True, "nonfinite"


REPAIR_STORED = np.arange(1, 4001, 4, dtype=np.int64)            # the columns x stores in the repair cases: 1000 of 4096, gather
REPAIR_ROWS = {1: "finite", 4095: "finite", 4096: "finite", 4097: "+inf", 4500: "-inf", 5000: "finite"}
REPAIR_DELETED = (4094, 4499)                                     # rows deleted in front of two of them: tombstones in the row table


def repair_matrix():
    """5000 x 4096, every cell placed by hand, for the rows the gather strategy has to sum again (k_spx_repair): each row of REPAIR_ROWS
    holds several finite cells in columns x stores (row 4096: 200 of them, more than a wave's 64 slots) and +-Inf / NaN in columns x does
    NOT store; rows 4097 and 4500 also hold an Inf in a column x stores (13, 17: x = 0.5 there), so the class of the result is decided by
    which cells are left out.  The rows sit at both sides of the 4096-row tile border, at the first and the last row.  The row table has
    gaps (row 2 is absent, the ordinary rows are 3, 6, 9, ...), so only row 1 is a direct hit.  Row 4600 holds nothing but a NaN in an
    absent column (untouched), row 4700 a NaN in a stored column (NaN as in the reference)."""
    S = REPAIR_STORED
    cells = {}

    def finite_cells(r, k):
        for j in range(k):
            c = int(S[(r * 7 + j * 3) % len(S)])
            if c not in (13, 17, 21):
                cells[(r, c)] = None
    for r in list(range(3, 4000, 3)) + [4094, 4098, 4499, 4501]:
        finite_cells(r, 3)
        cells[(r, 2 + 4 * (r % 900))] = None                      # a finite cell in an absent column
    for r in REPAIR_ROWS:
        finite_cells(r, 200 if r == 4096 else 5)
    finite_cells(4700, 4)
    keys = sorted(cells)
    vals = a_vals(123, len(keys))
    for k, v in zip(keys, vals):
        cells[k] = v
    Inf, NaN = np.inf, np.nan
    cells.update({(1, 2): Inf, (4095, 3): NaN, (4095, 4002): -Inf, (4096, 2): -Inf, (4096, 4096): NaN, (4097, 13): Inf, (4097, 3): NaN,
                  (4500, 17): -Inf, (4500, 2): Inf, (5000, 4095): NaN, (5000, 6): Inf, (4600, 2): NaN, (4700, 21): NaN})
    keys = sorted(cells)
    return i64([k[0] for k in keys]), i64([k[1] for k in keys]), np.array([cells[k] for k in keys]), 5000, 4096


def repair_x(seed):
    xv = x_vals_nz(seed, len(REPAIR_STORED))                      # no stored zero: 0 * Inf is not the subject here
    xv[[3, 4, 5]] = 0.5                                            # columns 13, 17, 21
    return REPAIR_STORED, xv


def s_repair(swap):
    """swap: the transposed matrix under transpose = True — the twin that is gathered over and repaired is then the column orientation"""
    def script(mk):
        I, J, V, m, n = repair_matrix()
        a = mk(J, I, V, n, m) if swap else mk(I, J, V, m, n)
        xi, xv = repair_x(1)
        yield a, xi, xv, swap, "nonfinite repair gather"
        for r in REPAIR_DELETED:
            a.deletecolumn(r) if swap else a.deleterow(r)
        xi, xv = repair_x(2)
        yield a, xi, xv, swap, "nonfinite repair gather"
        yield a, xi[:100], xv[:100], swap, "nonfinite repair xdriven"
        few = np.arange(1, 5001, 50, dtype=np.int64)               # the other transpose of the same handle
        yield a, few, x_vals(4, len(few)), not swap, "nonfinite"
        xi, xv = repair_x(3)
        yield a, xi, xv, swap, "nonfinite repair gather"
    return script


SCRIPTS = {
    **{"bitmap_m%d" % m: s_bitmap_edges(m, t) for m, t in ((1, None), (63, None), (64, None), (65, None), (4095, None), (4096, 0), (4097, 0),
                                                            (65536, 15), (65537, 1), (4 * 2 ** 20 + 1, None))},
    "landing": s_landing,
    "upload": s_upload,
    "tables": s_tables(False),
    "tables_swapped": s_tables(True),
    "column_lengths": s_column_lengths(False),
    "column_lengths_swapped": s_column_lengths(True),
    **{"boundary_n%d" % n: s_boundary(n) for n in (16, 4096, 40000)},
    "changes": s_changes,
    "nonfinite_small": s_nonfinite_small,
    "nonfinite_tile": s_nonfinite_tile,
    "repair": s_repair(False),
    "repair_swapped": s_repair(True),
}


def maker(dsa, binding):
    return lambda I, J, V, m, n: dsa.dynamicsparse(I, J, V, m, n, binding=binding)


# ---- CPU: the model against the oracle, and the exact-summation condition, on every input of the GPU tests -----------------------------
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_model_matches_oracle_and_inputs_sum_exactly(dsa, oracle, name):
    steps = strategies = 0
    for b, xi, xv, tr, note in SCRIPTS[name](maker(dsa, oracle)):
        assert np.all(np.diff(xi) > 0), "x must ascend strictly"
        L = b.export_layout(ROWMAJOR if tr else COLMAJOR)
        ie, ve = b.mul((xi, xv), transpose=tr)
        m, n = b.size()
        assert len(ie) == 0 or (ie[0] >= 1 and ie[-1] <= (n if tr else m)), "rows outside 1..m are a documented divergence: keep them out"
        small = len(xi) <= 64 and len(L["occ"]) <= 1 << 16
        for model in ((model_mul, model_mul_fast) if small else (model_mul_fast,)):
            im, vm, mag, exact = model(L, xi, xv)
            assert np.array_equal(im, ie), (name, steps, note)
            assert np.array_equal(vm, ve, equal_nan=True), (name, steps, note)
            # what lets the GPU tests ask for equal values: every finite product a multiple of 2^-14, every row below 2^53 of them
            assert exact and mag < 2 ** 53, (name, steps, mag)
        if note.startswith("finite"):
            assert np.all(np.isfinite(ve)) and np.all(np.isfinite(xv)), (name, steps)
        if "xdriven" in note or "gather" in note:
            assert xdriven(len(xi), m if tr else n) == ("xdriven" in note), (name, steps, note)
        strategies |= 1 if xdriven(len(xi), m if tr else n) else 2
        steps += 1
    assert steps > 0
    if name not in ("tables", "tables_swapped", "column_lengths", "column_lengths_swapped"):          # (those are about k_spx_accum)
        assert strategies == 3, "both strategies must be reached by shape"


@pytest.mark.parametrize("swap", (False, True))
def test_repair_case_rows_are_touched_and_hold_nonfinite_cells_in_absent_columns(dsa, oracle, swap):
    """what makes the repair cases cases: stated on the triples and on the oracle's result, not left to a seed"""
    I, J, V, m, n = repair_matrix()
    xi, xv = repair_x(1)
    assert not xdriven(len(xi), n) and np.all(xv != 0.0)
    stored = np.isin(J, xi)
    for r, cls in REPAIR_ROWS.items():
        mine = I == r
        assert np.sum(mine & stored & np.isfinite(V)) >= 2, r                      # several finite cells x reaches: a wave reduction
        assert np.any(mine & ~stored & ~np.isfinite(V)), r                         # a non-finite cell in a column x does not store
        assert (cls == "finite") == (not np.any(mine & stored & ~np.isfinite(V))), r
    assert np.sum((I == 4096) & stored) > 64                                       # more slots than a wave has lanes
    assert not np.any(I == 2) and all(np.any(I == r) for r in REPAIR_DELETED)      # a gapped row table; the rows deleted later exist
    steps = list(SCRIPTS["repair_swapped" if swap else "repair"](maker(dsa, oracle)))
    for b, sxi, sxv, tr, note in steps:
        if "repair gather" not in note:
            continue
        ie, ve = b.mul((sxi, sxv), transpose=tr)
        got = dict(zip(ie.tolist(), ve.tolist()))
        for r, cls in REPAIR_ROWS.items():
            assert r in got, (r, note)
            assert (np.isfinite(got[r]) if cls == "finite" else got[r] == float(cls)), (r, cls, got[r])
        assert 4600 not in got and np.isnan(got[4700])
        live = b.export_layout(COLMAJOR if tr else ROWMAJOR)["col_live"]           # the twin's table: tombstones after the deletions
    assert not np.all(live)


def test_oracle_on_the_small_nonfinite_case(dsa, oracle):
    b = dsa.dynamicsparse(*nonfinite_small(), binding=oracle)
    ie, ve = b.mul((i64([1, 2, 3]), np.array([1.5, 0.0, 2.0])))
    assert ie.tolist() == [2, 3] and ve.tolist() == [1.5, 0.0]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _same(got_i, got_v, ie, ve, what):
    assert np.array_equal(got_i, ie), (what, len(got_i), len(ie))
    assert np.array_equal(got_v, ve, equal_nan=True), (what, got_v[:8], ve[:8], int(np.sum(~((got_v == ve) | (np.isnan(got_v) & np.isnan(ve))))))


def _dev_product(a, xi, xv, tr, cap):
    import torch
    dev = torch.device("cuda")
    d_xi = torch.from_numpy(np.ascontiguousarray(xi)).to(dev) if len(xi) else torch.zeros(1, dtype=torch.int64, device=dev)
    d_xv = torch.from_numpy(np.ascontiguousarray(xv)).to(dev) if len(xv) else torch.zeros(1, dtype=torch.float64, device=dev)
    d_yi = torch.full((max(cap, 1),), -7, dtype=torch.int64, device=dev)
    d_yv = torch.full((max(cap, 1),), -7.0, dtype=torch.float64, device=dev)
    d_cnt = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    a.mul_dev(d_xi.data_ptr(), d_xv.data_ptr(), len(xi), d_yi.data_ptr(), d_yv.data_ptr(), cap, d_cnt.data_ptr(), transpose=tr)
    a.sync()
    return int(d_cnt.item()), d_yi.cpu().numpy(), d_yv.cpu().numpy()


def _check_step(a, b, xi, xv, tr, what):
    """both entry-point families, twice on the same handle"""
    ie, ve = b.mul((xi, xv), transpose=tr)
    for rep in range(2):
        ia, va = a.mul((xi, xv), transpose=tr)                     # _begin + _fetch
        _same(ia, va, ie, ve, (what, "host", rep))
        k, yi, yv = _dev_product(a, xi, xv, tr, len(ie))
        assert k == len(ie), (what, "dev", rep, k, len(ie))
        _same(yi[:k], yv[:k], ie, ve, (what, "dev", rep))
    return ie, ve


def _wide_keys_if_asked(dsa, hip):
    """in the child process of test_column_location: the switch it was started with is one the library knows and honours"""
    if os.environ.get("DSA_KEYS_WIDE") == "1":
        names, honoured = dsa.dev_switches(hip)
        assert honoured and "DSA_KEYS_WIDE" in names


def _run_script(dsa, hip, oracle, name):
    n = 0
    for (a, xi, xv, tr, note), (b, xi2, xv2, tr2, _) in zip(SCRIPTS[name](maker(dsa, hip)), SCRIPTS[name](maker(dsa, oracle))):
        assert np.array_equal(xi, xi2) and tr == tr2
        # a key below 1 in x: the device entry point documents that it ignores it under the gather strategy (include/dsa.h); the
        # cases here are driven by x, where it does not
        _check_step(a, b, xi, xv, tr, (name, n, note))
        n += 1
    assert n > 0


@pytest.mark.gpu
@pytest.mark.parametrize("m", (1, 63, 64, 65, 4095, 4096, 4097, 65536, 65537, 4 * 2 ** 20 + 1))
def test_bitmap_tile_and_prefix_edges(dsa, hip, oracle, m):
    """64-row words, 4096-row tiles, the 16 tiles of one count workgroup (65536 rows) and the ticket of a second one (65537), a second
    1024-tile prefix round (4 * 2^20 + 1 rows): touched rows at the first and last row of the matrix, a word and a tile; a tile with all
    its rows; products with one touched row and with none; both strategies."""
    _run_script(dsa, hip, oracle, "bitmap_m%d" % m)


@pytest.mark.gpu
def test_landing_area_and_download_pieces(dsa, hip, oracle):
    """4095 / 4096 / 4097 touched rows (the pinned landing area), 32768 / 32769 (one download piece or two), 131073 (eight pieces),
    262145 (four copy threads), under both strategies; the device entry point with cap = 0, count - 1 and count."""
    _run_script(dsa, hip, oracle, "landing")
    a, b = (maker(dsa, x)(*landing_matrix()) for x in (hip, oracle))
    for count in LANDING_COUNTS:
        for tr, gather in ((False, False), (False, True), (True, None)):
            xi = np.arange(1, count + 1, dtype=np.int64) if tr else landing_x(count, gather)       # transpose: the first `count` rows
            xv = x_vals(count, len(xi))
            ie, ve = b.mul((xi, xv), transpose=tr)
            assert len(ie) == count or tr
            for cap in (0, len(ie) - 1, len(ie)):
                k, yi, yv = _dev_product(a, xi, xv, tr, cap)
                assert k == len(ie), (count, tr, gather, cap, k)                   # the count stays right
                _same(yi[:cap], yv[:cap], ie[:cap], ve[:cap], (count, tr, gather, cap))      # the pairs that fit are the first ones
                assert np.all(yi[cap:] == -7) and np.all(yv[cap:] == -7.0)        # nothing behind cap was written
            ia, va = a.mul((xi, xv), transpose=tr)                                 # the following product on the handle
            _same(ia, va, ie, ve, (count, tr, gather, "after cap"))


@pytest.mark.gpu
def test_x_upload_paths(dsa, hip, oracle):
    _run_script(dsa, hip, oracle, "upload")


@pytest.mark.gpu
def test_x_order_check_plain_and_threaded(dsa, hip, oracle):
    """an equal and a descending pair at i = 1, i = nx - 1 and at the borders of the four upload threads' quarters: DSA_EARG, and the
    next product on the handle is right"""
    n = 524288
    I, J, V = sprinkle(5000, n, 400, 1000 + n)
    a, b = (dsa.dynamicsparse(I, J, V, 5000, n, binding=x) for x in (hip, oracle))
    good = {nx: x_with(np.unique(J)[::2], n, nx) for nx in (1000, 65537)}
    for nx, i, kind in order_check_inputs():
        xi = good[nx].copy()
        xv = x_vals(nx + i, nx)
        if kind == "equal":
            xi[i] = xi[i - 1]
        else:
            xi[i - 1], xi[i] = xi[i], xi[i - 1]
        for tr in (False, True):                                   # (transposed: the entries of x above m name no row)
            with pytest.raises(dsa.DsaError) as ei:
                a.mul((xi, xv), transpose=tr)
            assert ei.value.code == dsa.binding.EARG, (nx, i, kind, tr)
            ie, ve = b.mul((good[nx], xv), transpose=tr)
            ia, va = a.mul((good[nx], xv), transpose=tr)
            _same(ia, va, ie, ve, (nx, i, kind, tr, "after EARG"))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ("in_process", "wide_keys_child"))
def test_column_location(dsa, hip, oracle, where):
    """k_spx_accum's direct hit (its three exits) and the 64-ary search with its tombstone walk-back: identity tables, deleted
    neighbours, 200 deleted columns in a row, even keys (no direct hit), a gap, a key below 1, table lengths with zero to three
    narrowing rounds; columns of 0 / 1 / 63 / 64 / 65 / 1000 cells.  Once more with 64-bit keys in a child process, which also runs
    the repair cases of test_nonfinite_values_both_strategies that way."""
    if where == "wide_keys_child":
        env = dict(os.environ, DSA_DEV="1", DSA_KEYS_WIDE="1")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_sparse_x.py"), "-m", "gpu", "-x", "-q", "-k",
                            "(test_column_location and in_process) or (test_nonfinite_values_both_strategies and repair)"],
                           env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert "3 passed" in r.stdout, r.stdout[-1000:]          # the tables, and k_spx_repair on both orientations, with 64-bit keys
        return
    _wide_keys_if_asked(dsa, hip)
    for name in ("tables", "tables_swapped", "column_lengths", "column_lengths_swapped"):
        _run_script(dsa, hip, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (16, 4096, 40000))
def test_strategy_boundary_alternating(dsa, hip, oracle, n):
    """nx = n / 8 (gather) and n / 8 - 1 (driven by x), both transposes, eight products in a row on one handle"""
    _run_script(dsa, hip, oracle, "boundary_n%d" % n)


@pytest.mark.gpu
def test_zero_invariant_across_changes(dsa, hip, oracle):
    """products around set_batch, deletecolumn, deleterow and a write that makes the scratch grow"""
    _run_script(dsa, hip, oracle, "changes")


@pytest.mark.gpu
def test_ecap_and_fetch_modes(dsa, hip, oracle):
    m, n = 6000, 800
    I, J, V = sprinkle(m, n, 5000, 71)
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    yi = np.empty(m, dtype=np.int64); yv = np.empty(m); k = C.c_int64()

    def fetch(cap):
        hip.call("mat_spmv_sparse_fetch", a.h, yi.ctypes.data_as(P_I64), yv.ctypes.data_as(P_F64), cap, C.byref(k))
    with pytest.raises(dsa.DsaError) as ei:                        # _fetch without _begin
        fetch(m)
    assert ei.value.code == dsa.binding.EMODE
    cases = ((np.arange(3, 603, 7, dtype=np.int64), False), (np.arange(1, 801, 2, dtype=np.int64), False),          # driven by x, gather
             (np.arange(3, 6000, 70, dtype=np.int64), True), (np.arange(1, 6001, 2, dtype=np.int64), True))
    for q, (xi, tr) in enumerate(cases):
        assert xdriven(len(xi), m if tr else n) == (q % 2 == 0)
        xv = x_vals(50 + q, len(xi))
        ie, ve = b.mul((xi, xv), transpose=tr)
        assert len(ie) > 4
        for then_fetch in (False, True):
            with pytest.raises(dsa.DsaError) as ei:
                hip.call("mat_spmv_sparse", a.h, int(tr), xi.ctypes.data_as(P_I64), xv.ctypes.data_as(P_F64), len(xi), yi.ctypes.data_as(P_I64),
                         yv.ctypes.data_as(P_F64), 4, C.byref(k))
            assert ei.value.code == dsa.binding.ECAP and k.value == len(ie)
            if then_fetch:                                         # the result stays fetchable
                fetch(m)
                _same(yi[:k.value], yv[:k.value], ie, ve, (q, "fetch after ECAP"))
            _check_step(a, b, xi[::2], xv[::2], tr, (q, then_fetch, "after ECAP"))
        cnt, _, _ = _dev_product(a, xi, xv, tr, len(ie))
        assert cnt == len(ie)
        with pytest.raises(dsa.DsaError) as ei:                    # _fetch after a _dev call
            fetch(m)
        assert ei.value.code == dsa.binding.EMODE
        _check_step(a, b, xi, xv, tr, (q, "after EMODE"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("nonfinite_small", "nonfinite_tile", "repair", "repair_swapped"))
def test_nonfinite_values_both_strategies(dsa, hip, oracle, name):
    """+Inf / -Inf / NaN of A in columns x does not store leave the row finite (or untouched); in columns x stores they make it
    non-finite as in the reference; Inf / NaN / 0.0 / -0.0 in x; a finite product after one that held NaN is exact.  repair: the rows
    the gather strategy sums again (k_spx_repair), placed by hand — see repair_matrix."""
    _wide_keys_if_asked(dsa, hip)
    if name == "nonfinite_small":
        a = dsa.dynamicsparse(*nonfinite_small(), binding=hip)
        for rep in range(2):
            ia, va = a.mul((i64([1, 2, 3]), np.array([1.5, 0.0, 2.0])))
            assert ia.tolist() == [2, 3] and va.tolist() == [1.5, 0.0], (rep, ia, va)
    _run_script(dsa, hip, oracle, name)
