"""Row / column reductions and in-place diagonal scaling (include/dsa.h: dsa_mat_reduce[_dev], dsa_mat_scale[_dev]; csrc/scale.hip).

Expected values never come from the kernels: `expected_reduce` and `expected_scaled_vals` are numpy over the ORACLE's exported layout.
The partition of a slot is the value stored in the semaphore in front of it (checked against the layout's `semaphores` table), its
key `col_keys[id - 1]`.

Tolerances.  absmax and count are exact in any order: bitwise.  A sum of at most two terms is the same in any order: bitwise.  Longer
sums are compared within 2 * n * 2^-53 * sum |term| (n = the row's cells): n * 2^-53 * sum |term| bounds the error of a sum of n terms
in ANY order, and it is taken twice because the expectation's order (slot order) is as arbitrary as the kernel's.  The random case
uses values whose sums and squared sums are exact in binary64 in any order (asserted on the CPU side): every kind is bitwise there.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode, expected_compressed

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
EARG, EBOUNDS, EMODE = 1, 2, 5
SENTINEL = -7.25
KINDS = ("sum", "abssum", "sqsum", "absmax", "count")
KIND_CODE = dict(sum=0, abssum=1, sqsum=2, absmax=3, count=4)
PER = {ROWMAJOR: "row", COLMAJOR: "column"}
SPAN = 512               # slots one wave of the kernels owns
TILE = 2048              # ... and one workgroup
P_F64 = C.POINTER(C.c_double)
NAMES = ("mat_reduce", "mat_reduce_dev", "mat_scale", "mat_scale_dev")
METHODS = ("reduce", "reduce_dev", "row_norms", "col_norms", "scale", "scale_dev")


# ---------------------------------------------------------------------------------------------------------------- helpers
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    eq = _bits(got) == _bits(exp)
    assert eq.all(), (what, np.argwhere(~eq)[:5].tolist(), got[~eq][:5], exp[~eq][:5])


def slot_partitions(L):
    """(cell, is_sem, part) per slot of an exported layout: occupied non-semaphore slots, semaphore slots, and the partition id
    (1-based, 0: none) that owns the slot — the value of the nearest semaphore at or below it"""
    occ = L["occ"].astype(bool)
    keys, vals = L["keys"], L["vals"]
    cap = len(occ)
    is_sem = occ & (keys == 0)
    at = np.maximum.accumulate(np.where(is_sem, np.arange(cap), -1))
    pid = np.where(is_sem, vals, 0.0).astype(np.int64)
    part = np.where(at >= 0, pid[np.maximum(at, 0)], 0)
    # the semaphore table says the same: semaphores[id - 1] is the 1-based slot of partition id's semaphore
    s = np.nonzero(is_sem)[0]
    assert np.array_equal(L["semaphores"][pid[s] - 1], s + 1)
    cell = occ & ~is_sem
    assert not cell.any() or (part[cell] >= 1).all(), "a cell in front of the first semaphore"
    return cell, is_sem, part


def _terms(kind, v):
    if kind == "sum":
        return v.copy()
    if kind == "sqsum":
        return v * v
    if kind == "count":
        return np.ones(len(v))
    return np.abs(v)


def expected_reduce(L, dim, kind):
    """(out, cells, abs_sum, in_bounds) of one orientation: out[key - 1] over the cells of partition `key` added in slot order from
    +0.0 (absmax: the maximum of the bit patterns of |v|, so NaN wins); cells per key; sum of |term| per key; whether the key of every
    partition that has a semaphore lies in 1..dim"""
    cell, is_sem, part = slot_partitions(L)
    ck = L["col_keys"]
    sem_keys = ck[part[is_sem] - 1]
    in_bounds = bool(np.all((sem_keys >= 1) & (sem_keys <= dim)))
    pk = ck[part[cell] - 1]
    ok = (pk >= 1) & (pk <= dim)
    t = _terms(kind, L["vals"][cell])[ok]
    at = pk[ok] - 1
    out = np.zeros(dim)
    cells = np.bincount(at, minlength=dim)[:dim] if dim else np.zeros(0, dtype=np.int64)
    abs_sum = np.zeros(dim)
    np.add.at(abs_sum, at, np.abs(t))
    if kind == "absmax":
        ob = np.zeros(dim, dtype=np.uint64)
        np.maximum.at(ob, at, t.view(np.uint64))
        out = ob.view(np.float64)
    else:
        np.add.at(out, at, t)
    return out, cells, abs_sum, in_bounds


def _assert_reduce(got, exp, kind, what):
    out, cells, abs_sum, _ = exp
    assert got.shape == out.shape, (what, got.shape, out.shape)
    if kind in ("absmax", "count"):
        return _same_bits(got, out, what)
    short = cells <= 2
    _same_bits(got[short], out[short], what)
    bound = 2.0 * cells * 2.0 ** -53 * abs_sum
    bad = ~short & ~(np.abs(got - out) <= bound)
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], got[bad][:5], out[bad][:5], bound[bad][:5])


def _reduce_forms(hip, a, kind, o, dim):
    """the result of the device form, the host form and the two Python forms, the outputs pre-filled with the sentinel"""
    import torch
    d = torch.full((max(dim, 1),), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a.reduce_dev(kind, PER[o], d.data_ptr(), dim)
    a.sync()
    h = np.full(max(dim, 1), SENTINEL)
    hip.call("mat_reduce", a.h, o, KIND_CODE[kind], h.ctypes.data_as(P_F64), dim)
    t = torch.full((dim,), SENTINEL, dtype=torch.float64, device="cuda")
    back = a.reduce(kind, PER[o], out=t)
    assert back is t
    return d.cpu().numpy()[:dim], h[:dim], a.reduce(kind, PER[o]), t.cpu().numpy()


def _check_reduce(dsa, hip, a, b, kinds=KINDS, exact=False, what=""):
    """every kind x both orientations x every form of the HIP matrix `a` against numpy over the layout of the oracle matrix `b`"""
    m, n = b.size()
    assert a.size() == (m, n)
    for o, dim in ((ROWMAJOR, m), (COLMAJOR, n)):
        L = b.export_layout(o)
        for kind in kinds:
            exp = expected_reduce(L, dim, kind)
            tag = (what, PER[o], kind)
            if not exp[3]:
                with pytest.raises(dsa.DsaError) as ei:
                    a.reduce(kind, PER[o])
                assert ei.value.code == EBOUNDS, tag
                continue
            for got in _reduce_forms(hip, a, kind, o, dim):
                if exact:
                    _same_bits(got, exp[0], tag)
                else:
                    _assert_reduce(got, exp, kind, tag)
                assert (_bits(got[exp[1] == 0]) == 0).all(), tag          # +0.0 where nothing is stored


def _triples(b):
    """(I, J, V) of an oracle matrix, 1-based, from its colmajor layout"""
    m, n = b.size()
    ptr, idx, val = expected_compressed(b.export_layout(COLMAJOR), n)
    J = np.repeat(np.arange(1, n + 1), np.diff(ptr))
    return idx + 1, J, val


def expected_scaled_vals(L, o, alpha, r, c):
    """the value array of one orientation after scale: ((v * alpha) * r[i - 1]) * c[j - 1] at occupied non-semaphore slots, three
    separately rounded products; everything else as it was.  colmajor: key = row, partition key = column."""
    cell, _, part = slot_partitions(L)
    key = L["keys"][cell]
    pk = L["col_keys"][part[cell] - 1]
    i, j = (key, pk) if o == COLMAJOR else (pk, key)
    x = L["vals"][cell] * np.float64(alpha)
    if r is not None:
        x = x * np.asarray(r, dtype=np.float64)[i - 1]
    if c is not None:
        x = x * np.asarray(c, dtype=np.float64)[j - 1]
    out = L["vals"].copy()
    out[cell] = x
    return out


def _in_size(L, dim_key, dim_part):
    cell, is_sem, part = slot_partitions(L)
    key, pk = L["keys"][cell], L["col_keys"][part[is_sem] - 1]
    return bool(np.all((key >= 1) & (key <= dim_key)) and np.all((pk >= 1) & (pk <= dim_part)))


def _layouts(a):
    return [a.export_layout(o) for o in (COLMAJOR, ROWMAJOR)]


def _assert_layouts_equal(La, Lb, what, vals=True):
    for o in (COLMAJOR, ROWMAJOR):
        for k in ("keys", "occ", "semaphores", "col_keys", "col_live") + (("vals",) if vals else ()):
            x, y = La[o][k], Lb[o][k]
            if k == "vals":
                # unoccupied slots hold whatever the last move left: only occupied slots are compared
                occ = La[o]["occ"].astype(bool)
                x, y = _bits(x[occ]), _bits(y[occ])
            assert np.array_equal(x, y), (what, o, k)


def _coo(comp, outer_is_row):
    ptr, idx, val = comp
    outer = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    i, j = (outer, np.asarray(idx)) if outer_is_row else (np.asarray(idx), outer)
    order = np.lexsort((j, i))
    return i[order], j[order], _bits(np.asarray(val)[order])


def _scale_and_check(dsa, hip, a, b, alpha, r, c, how="numpy", what=""):
    """scale the HIP matrix `a` and check it slot by slot against numpy over its layouts before; then bring the oracle matrix `b` to
    the same values with value-only overwrites"""
    import torch
    m, n = a.size()
    before, info0 = _layouts(a), [a.info(o) for o in (COLMAJOR, ROWMAJOR)]
    nnz0 = a.nnz()
    if not (_in_size(before[0], m, n) and _in_size(before[1], n, m)):
        with pytest.raises(dsa.DsaError) as ei:
            a.scale(alpha, r, c)
        assert ei.value.code == EBOUNDS, what
        _assert_layouts_equal(_layouts(a), before, what)
        return False
    if how == "numpy":
        assert a.scale(alpha, r, c) is a
    else:
        tr = None if r is None else torch.from_numpy(np.asarray(r, dtype=np.float64)).to("cuda")
        tc = None if c is None else torch.from_numpy(np.asarray(c, dtype=np.float64)).to("cuda")
        if how == "torch":
            # any stride: every second element of a longer tensor
            if tr is not None:
                tr = torch.stack([tr, torch.full_like(tr, np.nan)], dim=1).reshape(-1)[::2]
            a.scale(alpha, tr, tc)
        else:
            torch.cuda.synchronize()
            a.scale_dev(alpha, 0 if tr is None else tr.data_ptr(), m, 0 if tc is None else tc.data_ptr(), n)
            a.sync()
    after = _layouts(a)
    _assert_layouts_equal(after, before, what, vals=False)
    assert [a.info(o) for o in (COLMAJOR, ROWMAJOR)] == info0, what
    assert a.nnz() == nnz0
    for o in (COLMAJOR, ROWMAJOR):
        exp = expected_scaled_vals(before[o], o, alpha, r, c)
        occ = before[o]["occ"].astype(bool)
        eq = _bits(after[o]["vals"][occ]) == _bits(exp[occ])          # cells: the formula; semaphores: unchanged
        assert eq.all(), (what, o, int((~eq).sum()))
    # both orientations describe the same matrix bit for bit
    csc, csr = _coo(a.to_csc(), False), _coo(a.to_csr(), True)
    for x, y in zip(csc, csr):
        assert np.array_equal(x, y), what
    # the oracle gets the same values by overwriting every stored entry
    I, J, V = _triples(b)
    x = V * np.float64(alpha)
    if r is not None:
        x = x * np.asarray(r, dtype=np.float64)[I - 1]
    if c is not None:
        x = x * np.asarray(c, dtype=np.float64)[J - 1]
    assert (x != 0.0).all() or len(x) == 0
    if len(x):
        b.set_batch(I, J, x)
    return True


def _factors(rng, m, n):
    sign = lambda k: np.where(rng.random(k) < 0.5, -1.0, 1.0)
    return float(rng.random() + 0.5), (rng.random(m) + 0.5) * sign(m), (rng.random(n) + 0.5) * sign(n)


def _mixed_batch(dsa, rng, a, b, k=200, stored_keys=False):
    """the same k writes (30 % of them deletions) on both; stored_keys: only rows and columns that hold an entry, so that no new
    partition is created (next to a tombstone the reference refuses one)"""
    m, n = b.size()
    if m == 0 or n == 0:
        return
    if stored_keys:
        Is, Js, _ = _triples(b)
        if len(Is) == 0:
            return
        I2, J2 = rng.choice(np.unique(Is), k), rng.choice(np.unique(Js), k)
    else:
        I2, J2 = rng.integers(1, m + 1, k), rng.integers(1, n + 1, k)
    V2 = np.where(rng.random(k) < 0.3, 0.0, rng.standard_normal(k))
    # should a write fail all the same, both fail alike, and the state behind the failed batch is still compared
    codes = []
    for x in (b, a):
        try:
            x.set_batch(I2, J2, V2)
            codes.append(0)
        except dsa.DsaError as e:
            codes.append(e.code)
    assert codes[0] == codes[1], codes


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_scale_reduce_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    for name in ("DSA_RED_SUM = 0", "DSA_RED_ABSSUM = 1", "DSA_RED_SQSUM = 2", "DSA_RED_ABSMAX = 3", "DSA_RED_COUNT = 4"):
        assert name in hdr, name
    for meth in METHODS:
        assert hasattr(dsa.DynamicSparseMatrix, meth), meth
    assert hasattr(dsa.Transposed, "reduce")


def test_oracle_binding_has_no_scale_or_reduce(dsa, oracle):
    for name in NAMES:
        assert not oracle.has(name), name
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    for call in (lambda: a.reduce("sum", "row"), lambda: a.reduce_dev("sum", "row", 0, 2), lambda: a.row_norms(2),
                 lambda: a.col_norms(1), lambda: a.scale(2.0), lambda: a.scale_dev(2.0, 0, 0, 0, 0), lambda: a.T.reduce("sum", "row")):
        with pytest.raises(dsa.DsaArgumentError):
            call()


@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_helper_sum_matches_the_oracle_product_with_ones(dsa, oracle, sc):
    """expected_reduce("sum") per row is the oracle's A * ones: the same terms v * 1.0 added in ascending key order from 0.0"""
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        return
    m, n = b.size()
    Lr, Lc = b.export_layout(ROWMAJOR), b.export_layout(COLMAJOR)
    out, cells, _, _ = expected_reduce(Lr, m, "sum")
    assert cells.sum() <= b.nnz()
    if m > 0 and n > 0 and _in_size(Lr, n, m) and _in_size(Lc, m, n):          # every stored entry inside size(b): nothing is left out
        assert cells.sum() == b.nnz()
        _same_bits(out, b.mul(np.ones(n)))
        _same_bits(expected_reduce(Lc, n, "sum")[0], b.mul(np.ones(m), transpose=True))


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_reduce_golden_cases(dsa, hip, oracle, sc):
    a = run_scenario(dsa, hip, sc)
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        return
    _check_reduce(dsa, hip, a, b, what=sc["name"])


def _exact_values(rng, k):
    return rng.integers(1, 1 << 20, k) * 2.0 ** -17 * np.where(rng.random(k) < 0.5, -1.0, 1.0)


@pytest.fixture(scope="module")
def random_case():
    """~3000 x 3000 with ~40 k entries, widened to 6500 x 6500 by one row and one column of 6100 cells each; every 97th row and
    column stays empty.  Values k * 2^-17, |k| < 2^20: every sum and squared sum is exact in any order."""
    rng = np.random.default_rng(101)
    dim, base, L = 6500, 3000, 6100
    I, J = rng.integers(1, base + 1, 40000), rng.integers(1, base + 1, 40000)
    free = np.array([k for k in range(1, dim + 1) if k % 97 != 0])
    long_row, long_col = 1234, 2345
    I = np.concatenate([I, np.full(L, long_row), rng.choice(free, L, replace=False)])
    J = np.concatenate([J, rng.choice(free, L, replace=False), np.full(L, long_col)])
    I[I % 97 == 0] += 1
    J[J % 97 == 0] += 1
    V = _exact_values(rng, len(I))
    return dict(I=I, J=J, V=V, dim=dim, long_row=long_row, long_col=long_col, L=L)


def _assert_sums_exact(b):
    """the reference sum alone is exact: per row / column the sum of |term| stays below 2^53 units of the terms' last place"""
    m, n = b.size()
    for o, dim in ((ROWMAJOR, m), (COLMAJOR, n)):
        L = b.export_layout(o)
        v = L["vals"][slot_partitions(L)[0]]
        assert np.array_equal(v * 2.0 ** 17, np.round(v * 2.0 ** 17))
        assert (expected_reduce(L, dim, "abssum")[0] < 2.0 ** (53 - 17)).all()          # terms are multiples of 2^-17
        assert (expected_reduce(L, dim, "sqsum")[0] < 2.0 ** (53 - 34)).all()           # squares are multiples of 2^-34


@pytest.mark.gpu
def test_reduce_random_case_is_exact_after_each_change(dsa, hip, oracle, random_case):
    rc = random_case
    rng = np.random.default_rng(102)
    dim = rc["dim"]
    a, b = (dsa.dynamicsparse(rc["I"], rc["J"], rc["V"], dim, dim, binding=x) for x in (hip, oracle))
    assert a.size() == b.size() == (dim, dim)
    for o, key in ((ROWMAJOR, rc["long_row"]), (COLMAJOR, rc["long_col"])):
        L = b.export_layout(o)
        cell, is_sem, part = slot_partitions(L)
        # the long partition crosses several spans and at least two workgroup tiles
        pid = int(np.nonzero(L["col_keys"][:len(L["semaphores"])] == key)[0][0]) + 1
        slots = np.nonzero(cell & (part == pid))[0]
        assert len(slots) >= rc["L"] and slots[-1] // TILE - slots[0] // TILE >= 2 and slots[-1] // SPAN - slots[0] // SPAN >= 8
        # a row whose cells begin in the span behind its semaphore
        occ = np.nonzero(L["occ"])[0]
        sem_then_cell = is_sem[occ[:-1]] & cell[occ[1:]] & (occ[:-1] // SPAN != occ[1:] // SPAN)
        assert sem_then_cell.any(), "no partition begins in the span behind its semaphore"
        empty = expected_reduce(L, dim, "count")[0] == 0
        assert empty[96::97].all() and empty.sum() >= dim // 97
    _assert_sums_exact(b)

    def check(what):
        _check_reduce(dsa, hip, a, b, exact=True, what=what)
        m, n = a.size()
        _same_bits(a.reduce("sum", "row"), a.matmul(np.ones(n)), what)
        _same_bits(a.T.reduce("sum", "row"), a.T.matmul(np.ones(m)), what)
        r1, r2 = a.reduce("sqsum", "row"), a.reduce("sqsum", "row")
        assert r1.tobytes() == r2.tobytes(), what
        _same_bits(a.row_norms(2), np.sqrt(r1))
        _same_bits(a.col_norms(1), a.reduce("abssum", "column"))
        _same_bits(a.row_norms(np.inf), a.reduce("absmax", "row"))

    check("built")
    # tombstones in both orientations
    for x in (a, b):
        x.deletecolumn(int(rc["J"][0]))
        x.deletecolumn(int(rc["J"][1]))
        x.deleterow(int(rc["I"][2]))
        x.deleterow(rc["long_row"] + 1)
    check("tombstones")
    # new columns, keys in random order
    newc = rng.permutation(np.arange(dim + 1, dim + 61))
    I3, V3 = rng.integers(1, dim + 1, len(newc)), _exact_values(rng, len(newc))
    for x in (a, b):
        x.set_batch(I3, newc, V3)
    assert a.size() == b.size() == (dim, dim + 60)
    check("new columns")
    for x in (a, b):
        x.rebalance_root(ROWMAJOR)
        x.rebalance_root(COLMAJOR)
    _assert_sums_exact(b)
    check("rebalance_root")


@pytest.mark.gpu
def test_reduce_wide_keys(dsa, hip, oracle):
    """a row key above 2^31: the colmajor orientation stores int64 keys; reduce per column walks it (the dense side stays small)"""
    rng = np.random.default_rng(111)
    big = (1 << 31) + 5
    n, nnz = 40, 900
    I = np.concatenate([rng.integers(1, 2000, nnz), [big, big + 3, big + 3]])
    J = np.concatenate([rng.integers(1, n + 1, nnz), [7, 7, n]])
    V = _exact_values(rng, len(I))
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    assert a.size() == b.size() == (big + 3, n)
    L = b.export_layout(COLMAJOR)
    assert L["keys"].max() > (1 << 31)
    for kind in ("count", "absmax", "sum"):
        exp = expected_reduce(L, n, kind)
        for got in _reduce_forms(hip, a, kind, COLMAJOR, n):
            _same_bits(got, exp[0], kind)
    # scale by a scalar and by columns (a row factor would need 2^31 entries): the int64 instantiation of the scale kernels
    alpha, _, c = _factors(rng, 1, n)
    before = _layouts(a)
    a.scale(alpha, None, c)
    after = _layouts(a)
    _assert_layouts_equal(after, before, "wide", vals=False)
    for o in (COLMAJOR, ROWMAJOR):
        occ = before[o]["occ"].astype(bool)
        assert np.array_equal(_bits(after[o]["vals"][occ]), _bits(expected_scaled_vals(before[o], o, alpha, None, c)[occ]))


@pytest.mark.gpu
def test_reduce_edges(dsa, hip, oracle):
    # an empty matrix out of fill mode
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    assert a.size() == (0, 0)
    for kind in KINDS:
        assert a.reduce(kind, "row").shape == (0,) and a.reduce(kind, "column").shape == (0,)
    a.scale(2.0)
    # m = 0 or n = 0
    for m, n in ((5, 0), (0, 4)):
        a = dsa.dynamicsparse(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), m, n, binding=hip)
        assert a.size() == (m, n)
        for kind in KINDS:
            assert (_bits(a.reduce(kind, "row")) == 0).all() and a.reduce(kind, "row").shape == (m,)
            assert (_bits(a.reduce(kind, "column")) == 0).all() and a.reduce(kind, "column").shape == (n,)
        a.scale(3.0, np.ones(m), np.ones(n))
    # a single cell
    a, b = (dsa.dynamicsparse([3], [2], [-1.5], 4, 5, binding=x) for x in (hip, oracle))
    _check_reduce(dsa, hip, a, b, exact=True, what="single")
    assert a.reduce("sqsum", "row").tolist() == [0.0, 0.0, 2.25, 0.0]
    assert a.reduce("absmax", "column").tolist() == [0.0, 1.5, 0.0, 0.0, 0.0]
    # NaN and Inf cells: absmax propagates NaN, count does not care
    I, J = [1, 1, 2, 2, 3, 3, 3], [1, 2, 1, 3, 1, 2, 3]
    V = [1.0, np.nan, -np.inf, 2.0, 3.0, -4.0, 0.5]
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    mx = a.reduce("absmax", "row")
    assert np.isnan(mx[0]) and mx[1] == np.inf and mx[2] == 4.0
    mc = a.reduce("absmax", "column")
    assert mc[0] == np.inf and np.isnan(mc[1]) and mc[2] == 2.0
    assert a.reduce("count", "row").tolist() == [2.0, 2.0, 3.0]
    _check_reduce(dsa, hip, a, b, kinds=("absmax", "count"), exact=True, what="nan")
    # a read right behind single-cell writes sees them (the queue is flushed first)
    a, b = (dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=x) for x in (hip, oracle))
    for x in (a, b):
        x[2, 1] = 4.0
        x[4, 3] = -8.0
    _same_bits(a.reduce("sum", "row"), np.array([1.0, 6.0, 0.0, -8.0]))
    _check_reduce(dsa, hip, a, b, exact=True, what="pending")
    for x in (a, b):
        x[1, 3] = 0.5
    a.scale(2.0)
    assert a[1, 3] == 1.0 and a[4, 3] == -16.0


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_scale_parity_golden_cases(dsa, hip, oracle, sc):
    a = run_scenario(dsa, hip, sc)
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        with pytest.raises(dsa.DsaError) as ei:
            a.scale(2.0)
        assert ei.value.code == EMODE
        return
    rng = np.random.default_rng(121)
    m, n = a.size()
    alpha, r, c = _factors(rng, m, n)
    if not _scale_and_check(dsa, hip, a, b, alpha, r, c, what=sc["name"]):
        return
    _assert_layouts_equal(_layouts(a), _layouts(b), sc["name"] + " (overwritten oracle)")
    _mixed_batch(dsa, rng, a, b, 60, stored_keys=True)
    assert a.size() == b.size()
    _assert_layouts_equal(_layouts(a), _layouts(b), sc["name"] + " (after a mixed batch)")


@pytest.mark.gpu
def test_scale_parity_random_case_every_form(dsa, hip, oracle, random_case):
    rc = random_case
    rng = np.random.default_rng(122)
    dim = rc["dim"]
    a, b = (dsa.dynamicsparse(rc["I"], rc["J"], rc["V"], dim, dim, binding=x) for x in (hip, oracle))
    for what, use, how in (("scalar", (1, 0, 0), "numpy"), ("rows", (0, 1, 0), "numpy"), ("cols", (0, 0, 1), "numpy"),
                           ("all, numpy", (1, 1, 1), "numpy"), ("all, torch", (1, 1, 1), "torch"), ("rows, torch", (0, 1, 0), "torch"),
                           ("all, dev", (1, 1, 1), "dev"), ("cols, dev", (0, 0, 1), "dev")):
        alpha, r, c = _factors(rng, dim, dim)
        assert _scale_and_check(dsa, hip, a, b, alpha if use[0] else 1.0, r if use[1] else None, c if use[2] else None, how, what)
        _assert_layouts_equal(_layouts(a), _layouts(b), what)
    _mixed_batch(dsa, rng, a, b, 3000)
    for x in (a, b):
        x.deletecolumn(rc["long_col"])
    _assert_layouts_equal(_layouts(a), _layouts(b), "after a mixed batch")
    _check_reduce(dsa, hip, a, b, what="after scale and writes")
    # mixing kinds is an error
    import torch
    with pytest.raises(dsa.DsaArgumentError):
        a.scale(1.0, np.ones(dim), torch.ones(dim, dtype=torch.float64, device="cuda"))


@pytest.mark.gpu
def test_scale_by_zero_keeps_every_entry(dsa, hip, oracle):
    rng = np.random.default_rng(131)
    m, n, nnz = 300, 200, 4000
    I, J, V = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz), rng.standard_normal(nnz)
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    Ib, Jb, Vb = _triples(b)
    z = int(Ib[len(Ib) // 2])
    r = rng.random(m) + 0.5
    r[z - 1] = 0.0
    nnz0, cnt_r, cnt_c = a.nnz(), a.reduce("count", "row"), a.reduce("count", "column")
    assert cnt_r[z - 1] > 0
    a.scale(1.0, r, None)
    assert a.nnz() == nnz0
    _same_bits(a.reduce("count", "row"), cnt_r)
    _same_bits(a.reduce("count", "column"), cnt_c)
    for j in Jb[Ib == z][:5]:
        assert a[z, int(j)] == 0.0
    assert (_bits(a.reduce("abssum", "row"))[z - 1] == 0)
    ptr, idx, val = a.to_csr()
    assert ptr[z] - ptr[z - 1] == cnt_r[z - 1] and (val[ptr[z - 1]:ptr[z]] == 0.0).all()
    # the product matches numpy on the scaled triples
    x = rng.standard_normal(n)
    y = np.zeros(m)
    np.add.at(y, Ib - 1, (Vb * r[Ib - 1]) * x[Jb - 1])
    np.testing.assert_allclose(a.mul(x), y, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_scale_drops_the_spmv_plan_and_reduce_keeps_it(dsa, hip):
    """the shape of tests/test_spmv_plan.py: the smallest at which the plan applies"""
    M = N = 420_000
    NNZ = 1_260_000
    rng = np.random.default_rng(141)
    I, J, V = rng.integers(1, M + 1, NNZ), rng.integers(1, N + 1, NNZ), rng.integers(1, 1 << 20, NNZ) * 2.0 ** -17
    a = dsa.dynamicsparse(I, J, V, M, N, binding=hip)
    x = 1.0 + rng.random(N)
    stats = lambda: (a.info(ROWMAJOR)["stat_spmv_plan"], a.info(ROWMAJOR)["stat_spmv_plan_builds"])
    ys = [a.mul(x).copy() for _ in range(3)]
    p0, b0 = stats()
    assert p0 > 0 and b0 == 1
    # a reduce between products: counters and plan untouched, the next product comes from the plan
    cnt = a.reduce("count", "row")
    assert cnt.sum() == a.nnz() and stats() == (p0, b0)
    assert a.mul(x).tobytes() == ys[0].tobytes() and stats() == (p0 + 1, b0)
    ptr, idx, val = a.to_csr()
    Ic, Jc = np.repeat(np.arange(1, M + 1), np.diff(ptr)), idx + 1
    alpha, r, c = 0.75, rng.random(M) + 0.5, rng.random(N) + 0.5
    a.scale(alpha, r, c)
    assert stats() == (p0 + 1, b0)
    zs = [a.mul(x).copy() for _ in range(3)]
    p1, b1 = stats()
    assert b1 == b0 + 1 and p1 == p0 + 2, (p0, b0, p1, b1)
    fresh = dsa.dynamicsparse(Ic, Jc, ((val * alpha) * r[Ic - 1]) * c[Jc - 1], M, N, binding=hip)
    ws = [fresh.mul(x).copy() for _ in range(3)]
    for z, w in zip(zs, ws):
        assert z.tobytes() == w.tobytes()
    assert zs[0].tobytes() != ys[0].tobytes()


@pytest.mark.gpu
def test_scale_reduce_errors(dsa, hip):
    import torch
    # fill mode
    f = dsa.dynamicsparse(binding=hip)
    f.set_batch([1, 2], [1, 2], [1.0, 2.0])
    out = np.full(4, SENTINEL)
    d = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert hip._mat_reduce(f.h, ROWMAJOR, 0, out.ctypes.data_as(P_F64), 2) == EMODE
    assert hip._mat_reduce_dev(f.h, ROWMAJOR, 0, C.c_void_p(d.data_ptr()), 2) == EMODE
    assert hip._mat_scale(f.h, 2.0, None, 0, None, 0) == EMODE
    assert hip._mat_scale_dev(f.h, 2.0, None, 0, None, 0) == EMODE
    # arguments
    a = dsa.dynamicsparse([1, 2, 3], [1, 2, 4], [1.0, 2.0, 3.0], binding=hip)          # 3 x 4
    before = _layouts(a)
    dp = C.c_void_p(d.data_ptr())
    for o, kind, n_out in ((2, 0, 3), (-1, 0, 3), (ROWMAJOR, 5, 3), (ROWMAJOR, -1, 3), (ROWMAJOR, 0, 4), (COLMAJOR, 0, 3), (ROWMAJOR, 0, 2)):
        assert hip._mat_reduce(a.h, o, kind, out.ctypes.data_as(P_F64), n_out) == EARG, (o, kind, n_out)
        assert hip._mat_reduce_dev(a.h, o, kind, dp, n_out) == EARG, (o, kind, n_out)
    assert hip._mat_reduce(a.h, ROWMAJOR, 0, None, 3) == EARG
    assert hip._mat_reduce_dev(a.h, ROWMAJOR, 0, None, 3) == EARG
    ones = np.ones(4)
    op = ones.ctypes.data_as(P_F64)
    for nr, nc in ((2, 4), (4, 4), (3, 3), (3, 5)):
        assert hip._mat_scale(a.h, 2.0, op, nr, op, nc) == EARG, (nr, nc)
        assert hip._mat_scale_dev(a.h, 2.0, dp, nr, dp, nc) == EARG, (nr, nc)
    assert hip._mat_scale(a.h, 2.0, op, 2, None, 4) == EARG and hip._mat_scale(a.h, 2.0, None, 3, op, 3) == EARG
    assert hip._mat_scale(a.h, 1.0, None, 77, None, -1) == 0          # the length of an absent factor is ignored
    with pytest.raises(dsa.DsaArgumentError):
        a.reduce("mean", "row")
    with pytest.raises(dsa.DsaArgumentError):
        a.reduce("sum", "diagonal")
    with pytest.raises(dsa.DsaArgumentError):
        a.row_norms(3)
    with pytest.raises(dsa.DsaArgumentError):
        a.reduce("sum", "row", out=torch.zeros(4, dtype=torch.float64, device="cuda"))
    a.sync()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (d == SENTINEL).all()
    _assert_layouts_equal(_layouts(a), before, "argument errors")
    # explicit m, n smaller than the keys: EBOUNDS from both calls, and a failed scale modifies neither orientation
    I, J, V = [1, 2, 5, 3], [1, 2, 2, 6], [1.0, 2.0, 3.0, 4.0]
    e = dsa.dynamicsparse(I, J, V, 4, 5, binding=hip)
    assert e.size() == (4, 5)
    before = _layouts(e)
    for per in ("row", "column"):
        with pytest.raises(dsa.DsaError) as ei:
            e.reduce("sum", per)
        assert ei.value.code == EBOUNDS, per
    for r, c in ((None, None), (np.full(4, 2.0), np.full(5, 3.0))):
        with pytest.raises(dsa.DsaError) as ei:
            e.scale(2.0, r, c)
        assert ei.value.code == EBOUNDS
        _assert_layouts_equal(_layouts(e), before, "failed scale")
    # only a row key outside: the column reduce still works, scale does not
    e = dsa.dynamicsparse([1, 9], [1, 2], [1.0, -2.0], 4, 5, binding=hip)
    before = _layouts(e)
    _same_bits(e.reduce("sum", "column"), np.array([1.0, -2.0, 0.0, 0.0, 0.0]))
    with pytest.raises(dsa.DsaError) as ei:
        e.reduce("sum", "row")
    assert ei.value.code == EBOUNDS
    with pytest.raises(dsa.DsaError) as ei:
        e.scale(2.0)
    assert ei.value.code == EBOUNDS
    _assert_layouts_equal(_layouts(e), before, "failed scale")
