"""In-place dropzeros! / droptol! (include/dsa.h: dsa_mat_droptol[_dev]; csrc/droptol.hip).

Expected layouts never come from the kernels: `expected_after_drop` is numpy over a layout exported BEFORE the call.  It evaluates the
predicate per cell (|v| <= tol, <= tr[row - 1], <= tc[col - 1]; the owner of a slot from `_owners` of the delete tests), spreads the
survivors — every semaphore among them — by the reference's spread! rule (`spread_slots`), rebuilds `semaphores` and leaves `col_keys`
/ `col_live` as they were.  On the CPU the helper is checked against the oracle: its surviving cell sequence and tables must be those
of the oracle after `b[i, j] = 0` for every dropped cell.  Comparisons are exact: occupancy, keys and tables equal, values bitwise.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode, expected_compressed
from test_delete_batch import _assert_layout, _bits, _clean, _owners, _same_csr, spread_slots

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
SIDES = (COLMAJOR, ROWMAJOR)
EARG, EBOUNDS, EMODE = 1, 2, 5
P_F64, P_I64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
NAMES = ("mat_droptol", "mat_droptol_dev")
METHODS = ("droptol", "dropzeros", "count_droptol", "droptol_dev")
TOLS = ("zero", "median", "inf")
VECS = ("none", "rows", "cols", "both")
INF, NAN = np.inf, np.nan


# ---------------------------------------------------------------------------------------------------------------- helper
def _le(a, t):
    with np.errstate(invalid="ignore"):
        return a <= t                                     # IEEE: False whenever a or t is NaN


def _gather(t, key):
    """t[key - 1] where the key is inside the vector, -1.0 (matches nothing) elsewhere"""
    t = np.asarray(t, dtype=np.float64)
    ok = (key >= 1) & (key <= len(t))
    out = np.full(len(key), -1.0)
    out[ok] = t[key[ok] - 1]
    return out


def drop_mask(L, tol, tr, tc, own_is_col):
    """per slot: the cell is dropped.  own_is_col: L is the colmajor layout (partitions are columns, keys rows)"""
    occ, is_sem, part = _owners(L)
    cell = occ & ~is_sem
    a = np.abs(L["vals"])
    pkey = np.where(part >= 1, L["col_keys"][np.maximum(part, 1) - 1], 0) if len(L["col_keys"]) else np.zeros(len(occ), dtype=np.int64)
    row, col = (L["keys"], pkey) if own_is_col else (pkey, L["keys"])
    drop = _le(a, tol)
    if tr is not None:
        drop = drop | _le(a, _gather(tr, row))
    if tc is not None:
        drop = drop | _le(a, _gather(tc, col))
    return cell & drop


def expected_after_drop(L, tol, tr, tc, own_is_col, drop=None):
    """the layout of one orientation after droptol(tol, tr, tc), from its layout L before; drop: the mask, instead of the predicate"""
    cap, seg = L["info"]["capacity"], L["info"]["segment_capacity"]
    if drop is None:
        drop = drop_mask(L, tol, tr, tc, own_is_col)
    keep = L["occ"].astype(bool) & ~drop
    src = np.nonzero(keep)[0]
    m = len(src)
    dst = src if (cap == seg or not drop.any()) else spread_slots(cap, m)      # a single leaf is not moved; no drop, no move
    occ = np.zeros(cap, dtype=np.uint8)
    k, v = np.zeros(cap, dtype=np.int64), np.zeros(cap)
    occ[dst] = 1
    k[dst], v[dst] = L["keys"][src], L["vals"][src]
    sems = np.zeros(len(L["semaphores"]), dtype=np.int64)
    s = dst[k[dst] == 0]
    sems[v[s].astype(np.int64) - 1] = s + 1
    return dict(keys=k, vals=v, occ=occ, semaphores=sems, col_keys=L["col_keys"].copy(), col_live=L["col_live"].copy(), m=m,
                dropped=int(drop.sum()))


def _cells(L, mask):
    """(i, j) of the masked slots of a COLMAJOR layout"""
    _, _, part = _owners(L)
    s = np.nonzero(mask)[0]
    return L["keys"][s], L["col_keys"][part[s] - 1]


def _cell_sequence(L):
    o = L["occ"].astype(bool)
    return L["keys"][o], _bits(L["vals"][o])


def _cell_abs(L):
    occ, is_sem, _ = _owners(L)
    return np.abs(L["vals"][occ & ~is_sem])


def _tol_of(kind, L):
    if kind == "zero":
        return 0.0
    if kind == "inf":
        return INF
    a = np.sort(_cell_abs(L))
    a = a[~np.isnan(a)]
    return float(a[len(a) // 2]) if len(a) else 1.0        # a stored value: the comparison is <=


def _vectors(kind, L, m, n, seed=0):
    """threshold vectors over the values of the matrix: absent, or per key one of nothing (-1, NaN), zero, a median and +Inf"""
    med = _tol_of("median", L)
    rng = np.random.default_rng(1000 + seed)
    pick = lambda k: rng.choice(np.array([-1.0, NAN, 0.0, med, med, INF]), size=max(int(k), 0))
    return (pick(m) if kind in ("rows", "both") else None), (pick(n) if kind in ("cols", "both") else None)


def _in_bounds(L, m, n):
    occ, is_sem, _ = _owners(L)
    k = L["keys"][occ & ~is_sem]
    pk = L["col_keys"][(L["col_live"] != 0) & (L["semaphores"] != 0)]
    return bool(((k >= 1) & (k <= m)).all() and ((pk >= 1) & (pk <= n)).all())


def _layout_bytes(a):
    out = []
    for o in SIDES:
        L = a.export_layout(o)
        out.append(tuple(L[f].tobytes() for f in ("keys", "vals", "occ", "semaphores", "col_keys", "col_live")))
    return out


def _zero_seq(b, I, J):
    for i, j in zip(I.tolist(), J.tolist()):
        b[i, j] = 0.0


STORED_ZEROS = dict(name="stored_zeros", kind="matrix", steps=[],
                    create=dict(I=[1, 2, 3, 3, 4, 4, 5, 1, 6], J=[1, 1, 2, 2, 2, 3, 3, 4, 4],
                                V=[0.0, 1.5, 2.0, -2.0, -0.0, 3.0, 0.25, 0.0, -4.0]))      # two 0.0, one -0.0, and (3, 2) cancels
CASES = MATRIX_CASES + [STORED_ZEROS]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_droptol_symbols_declared_bound_exported_and_in_julia(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    for meth in METHODS:
        assert hasattr(dsa.DynamicSparseMatrix, meth), meth
    assert callable(dsa.droptol) and callable(dsa.dropzeros)
    jdir = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "julia")
    amd = open(os.path.join(jdir, "DynamicSparseArraysAMD.jl")).read()
    dropin = open(os.path.join(jdir, "DynamicSparseArrays.jl")).read()
    assert "ccall((:dsa_mat_droptol, libdsa)" in amd
    for name in ("dropzeros!", "droptol!"):
        assert re.search(r"SparseArrays\." + re.escape(name) + r"\(a::DynamicSparseMatrix", amd), name
        assert re.search(r"^const " + re.escape(name) + r" = DynamicSparseArraysAMD\." + re.escape(name), dropin, flags=re.M), name
    assert "rows::Union{Nothing,AbstractVector{<:Real}} = nothing" in amd.split("SparseArrays.droptol!(a::DynamicSparseMatrix")[1][:300]


def test_oracle_binding_has_no_droptol(dsa, oracle):
    for name in NAMES:
        assert not oracle.has(name), name
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 0.0], binding=oracle)
    for call in (lambda: a.droptol(0.5), lambda: a.dropzeros(), lambda: a.count_droptol(0.0, rows=[1.0, 1.0]),
                 lambda: a.droptol_dev(0.0, 0, 0, 0, 0), lambda: dsa.droptol(a, 1.0), lambda: dsa.dropzeros(a)):
        with pytest.raises(dsa.DsaArgumentError):
            call()
    assert a.nnz() == 2


def test_stored_zeros_case_holds_stored_zeros(dsa, oracle):
    b = run_scenario(dsa, oracle, STORED_ZEROS)
    L = b.export_layout(COLMAJOR)
    v = L["vals"][L["occ"].astype(bool) & (L["keys"] != 0)]
    assert b.nnz() == 8 and (v == 0.0).sum() == 4           # 0.0, 0.0, -0.0 and the cancelled pair
    assert drop_mask(L, 0.0, None, None, True).sum() == 4
    assert drop_mask(L, -1.0, None, None, True).sum() == 0 and drop_mask(L, NAN, None, None, True).sum() == 0


@pytest.mark.parametrize("sc", CASES, ids=lambda s: s["name"])
def test_helper_survivors_match_sequential_zero_writes_on_the_oracle(dsa, oracle, sc):
    b0 = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b0):
        return
    before = [b0.export_layout(o) for o in SIDES]
    for o in SIDES:                                       # the empty drop set is the identity
        e = expected_after_drop(before[o], -1.0, None, None, o == COLMAJOR)
        assert e["dropped"] == 0
        _assert_layout(before[o], e, (sc["name"], "identity", o))
        assert np.array_equal(e["occ"], before[o]["occ"])
    for kind in TOLS:
        tol = _tol_of(kind, before[COLMAJOR])
        masks = [drop_mask(before[o], tol, None, None, o == COLMAJOR) for o in SIDES]
        assert masks[0].sum() == masks[1].sum()           # the cell leaves both orientations
        # The reference's write cannot address a cell whose inner key is below the semaphore key 0 (matrix_simple_use_A stores
        # A[i, -1]: in rowmajor the key -1 sorts in front of its row's semaphore and the search misses it), so its zero write
        # leaves that cell where it is in that orientation.  droptol drops by value and takes it from both; the oracle is
        # compared on the cells its write reaches.
        reach = [masks[o] & (before[o]["keys"] >= 1) for o in SIDES]
        all_reached = all(np.array_equal(reach[o], masks[o]) for o in SIDES)
        assert all_reached or sc["name"] == "matrix_simple_use_A"
        exp = [expected_after_drop(before[o], tol, None, None, o == COLMAJOR, drop=reach[o]) for o in SIDES]
        I, J = _cells(before[COLMAJOR], masks[COLMAJOR])
        b = run_scenario(dsa, oracle, sc)
        _zero_seq(b, I, J)
        for o in SIDES:
            got = b.export_layout(o)
            ek, ev = _cell_sequence(exp[o])
            gk, gv = _cell_sequence(got)
            assert np.array_equal(ek, gk) and np.array_equal(ev, gv), (sc["name"], kind, o)
            assert got["info"]["table_len"] == before[o]["info"]["table_len"]
            assert np.array_equal(got["col_keys"], exp[o]["col_keys"]) and np.array_equal(got["col_live"], exp[o]["col_live"])
            assert np.array_equal(got["semaphores"] != 0, exp[o]["semaphores"] != 0)
            assert b.nbpartitions(o) == b0.nbpartitions(o)
        assert b.size() == b0.size()
        assert b.nnz() in [b0.nnz() - exp[o]["dropped"] for o in (SIDES if not all_reached else SIDES[:1])]
        if kind == "inf":
            assert masks[0].sum() == b0.nnz() - int(np.isnan(_cell_abs(before[0])).sum())


# ---------------------------------------------------------------------------------------------------------------- GPU
def _drop(a, tol, tr, tc, how="numpy", count_only=False):
    if how == "numpy":
        return (a.count_droptol if count_only else a.droptol)(tol, rows=tr, cols=tc)
    if how == "list":
        f = lambda t: None if t is None else [float(x) for x in t]
        return (a.count_droptol if count_only else a.droptol)(tol, rows=f(tr), cols=f(tc))
    import torch
    f = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to("cuda")
    r, c = f(tr), f(tc)
    if how == "torch":
        return (a.count_droptol if count_only else a.droptol)(tol, rows=r, cols=c)
    torch.cuda.synchronize()
    got = a.droptol_dev(tol, 0 if r is None else r.data_ptr(), 0 if r is None else r.numel(), 0 if c is None else c.data_ptr(),
                        0 if c is None else c.numel(), count_only=count_only)
    a.sync()
    return got


def _apply_and_check(a, tol, tr, tc, what, how="numpy"):
    """droptol on the HIP matrix `a`: the count, both layouts against the helper, counters and the checker"""
    before = [a.export_layout(o) for o in SIDES]
    info0 = [a.info(o) for o in SIDES]
    nnz0, size0, parts0 = a.nnz(), a.size(), [a.nbpartitions(o) for o in SIDES]
    exp = [expected_after_drop(before[o], tol, tr, tc, o == COLMAJOR) for o in SIDES]
    assert exp[0]["dropped"] == exp[1]["dropped"], what
    assert _drop(a, tol, tr, tc, how, count_only=True) == exp[0]["dropped"], what
    dropped = _drop(a, tol, tr, tc, how)
    assert dropped == exp[0]["dropped"], (what, dropped, exp[0]["dropped"])
    for o in SIDES:
        _assert_layout(a.export_layout(o), exp[o], (what, o))
        inf = a.info(o)
        assert inf["nb_elements"] == exp[o]["m"], (what, o)
        for f in ("capacity", "segment_capacity", "height", "table_len", "nb_partitions"):
            assert inf[f] == info0[o][f], (what, o, f)
        assert a.nbpartitions(o) == parts0[o], (what, o)
    assert a.nnz() == nnz0 - dropped and a.size() == size0, what
    _clean(a)
    return dropped


@pytest.mark.gpu
@pytest.mark.parametrize("vec", VECS)
@pytest.mark.parametrize("kind", TOLS)
@pytest.mark.parametrize("sc", CASES, ids=lambda s: s["name"])
def test_golden_scenarios(dsa, hip, oracle, sc, kind, vec):
    a = run_scenario(dsa, hip, sc)
    if _in_fill_mode(dsa, a):
        return
    m, n = a.size()
    L = a.export_layout(COLMAJOR)
    tol = _tol_of(kind, L)
    tr, tc = _vectors(vec, L, m, n)
    if vec != "none" and not _in_bounds(L, m, n):         # matrix_simple_use_A: column -1
        before = _layout_bytes(a)
        with pytest.raises(dsa.DsaBoundsError):
            a.droptol(tol, rows=tr, cols=tc)
        assert _layout_bytes(a) == before
        return
    dropped = _apply_and_check(a, tol, tr, tc, (sc["name"], kind, vec), how=("numpy", "list", "torch", "dev")[VECS.index(vec)])
    R = run_scenario(dsa, oracle, sc).export_layout(ROWMAJOR)
    reached = all((X["keys"][drop_mask(X, tol, None, None, X is L)] >= 1).all() for X in (L, R))
    if vec == "none" and reached:                         # (the reference's own zero write misses A[i, -1] in rowmajor: see the CPU test)
        b = run_scenario(dsa, oracle, sc)
        _zero_seq(b, *_cells(L, drop_mask(L, tol, None, None, True)))
        assert a.nnz() == b.nnz() and a.size() == b.size() and b.nnz() == len(_cell_abs(L)) - dropped
        for o in SIDES:
            assert a.nbpartitions(o) == b.nbpartitions(o)
        _same_csr(dsa, a, b, (sc["name"], kind))


def _rebuild_with_small(dsa, hip, I, J, V, pick):
    """the matrix of (I, J, V) — distinct (i, j), |V| >= 1 — whose cells chosen by pick(colmajor layout) -> slot mask hold 1e-300:
    the layout does not depend on the values, so droptol(1e-200) drops exactly the cells of those slots"""
    L = dsa.dynamicsparse(I, J, V, binding=hip).export_layout(COLMAJOR)
    mask = pick(L)
    i, j = _cells(L, mask)
    small = set(zip(i.tolist(), j.tolist()))
    V2 = np.array([1e-300 if (p, q) in small else v for p, q, v in zip(I.tolist(), J.tolist(), V.tolist())])
    a = dsa.dynamicsparse(I, J, V2, binding=hip)
    L2 = a.export_layout(COLMAJOR)
    assert np.array_equal(L2["occ"], L["occ"]) and np.array_equal(L2["keys"][L["occ"] != 0], L["keys"][L["occ"] != 0])
    return a, mask


def _distinct(rng, m, n, k):
    p = rng.choice(m * n, size=k, replace=False)
    return p // n + 1, p % n + 1, 1.0 + rng.random(k)


def _edge_smallest(dsa, hip):
    """the smallest arrays a matrix has: 4 slots in two leaves of 2.  (A single leaf, capacity == segment_capacity, which the call
    would leave unmoved like the root rebalance, is not a state a matrix reaches: its arrays start with two leaves and never shrink
    below them.  The helper keeps that branch; here it is the smallest array that IS moved.)"""
    a = dsa.dynamicsparse([1], [1], [-0.0], binding=hip)
    assert all(a.info(o)["capacity"] == 4 and a.info(o)["segment_capacity"] == 2 for o in SIDES)
    return a, 0.0, None, None, 1


def _edge_two_small_leaves(dsa, hip):
    a = dsa.dynamicsparse([1, 2, 1], [1, 1, 2], [0.0, 2.0, -0.0], binding=hip)
    assert all(a.info(o)["capacity"] == 8 for o in SIDES)
    return a, 0.0, None, None, 2


def _edge_below_one_span(dsa, hip):
    I, J, V = _distinct(np.random.default_rng(21), 12, 9, 60)
    V[::3] = 0.0
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    inf = [a.info(o) for o in SIDES]
    assert all(64 < i["capacity"] < 512 and i["capacity"] > i["segment_capacity"] for i in inf), inf
    return a, 0.0, None, None, 20


def _edge_span_boundary(dsa, hip):
    """dropped cells in the last slot of one 512-slot span and the first slot of the next"""
    I, J, V = _distinct(np.random.default_rng(22), 90, 70, 5500)

    def pick(L):
        cell = L["occ"].astype(bool) & (L["keys"] != 0)
        s = np.arange(511, len(cell) - 1, 512)
        s = s[cell[s] & cell[s + 1]]
        assert len(s) > 0 and len(cell) >= 4 * 512
        mask = np.zeros(len(cell), dtype=bool)
        mask[s] = mask[s + 1] = True
        return mask
    a, mask = _rebuild_with_small(dsa, hip, I, J, V, pick)
    return a, 1e-200, None, None, int(mask.sum())


def _edge_whole_word(dsa, hip):
    """a 64-slot word whose cells are all dropped (its semaphores stay), beside words that keep everything"""
    I, J, V = _distinct(np.random.default_rng(23), 90, 70, 3000)

    def pick(L):
        cell = L["occ"].astype(bool) & (L["keys"] != 0)
        mask = np.zeros(len(cell), dtype=bool)
        for w in (3, 8, len(cell) // 64 - 1):
            mask[64 * w:64 * w + 64] = cell[64 * w:64 * w + 64]
        assert mask.sum() > 64
        return mask
    a, mask = _rebuild_with_small(dsa, hip, I, J, V, pick)
    return a, 1e-200, None, None, int(mask.sum())


def _edge_only_semaphores(dsa, hip):
    """single deletes have emptied 150 neighbouring columns: words that hold nothing but semaphores; tol = inf takes every cell"""
    J = np.arange(1, 401)
    I = (J * 7) % 50 + 1
    a = dsa.dynamicsparse(I, J, 1.0 + J, binding=hip)
    a.set_batch(I[100:250], J[100:250], np.zeros(150))
    L = a.export_layout(COLMAJOR)
    occ = L["occ"].astype(bool).reshape(-1, 64)
    sem = (occ & (L["keys"] == 0).reshape(-1, 64))
    assert ((occ.sum(1) > 0) & (occ.sum(1) == sem.sum(1))).any()
    return a, INF, None, None, 250


def _edge_long_column(dsa, hip):
    """column 7 and row 5 are longer than a 512-slot span: the owner of most of their cells comes from the carry"""
    rng = np.random.default_rng(24)
    I0, J0, _ = _distinct(rng, 1500, 1500, 3000)
    keep = (J0 != 7) & (I0 != 5)
    I = np.concatenate([np.arange(1, 1501), np.full(1499, 5), I0[keep]])
    J = np.concatenate([np.full(1500, 7), np.setdiff1d(np.arange(1, 1501), [7]), J0[keep]])
    V = 1.0 + rng.random(len(I))
    a = dsa.dynamicsparse(I, J, V, 1500, 1500, binding=hip)
    for o, key in ((COLMAJOR, 7), (ROWMAJOR, 5)):
        L = a.export_layout(o)
        s = np.sort(L["semaphores"][L["semaphores"] != 0])
        at = L["semaphores"][np.nonzero(L["col_keys"] == key)[0][0]]
        assert s[np.searchsorted(s, at) + 1] - at > 2 * 512
    tr, tc = np.full(1500, -1.0), np.full(1500, NAN)
    tc[6], tc[11], tr[4], tr[99] = 1.5, INF, INF, 1.25
    return a, -1.0, tr, tc, None


def _edge_front_of_first_semaphore(dsa, hip):
    """spans that begin inside a partition (cells in front of the span's first semaphore), every column with its own threshold"""
    rng = np.random.default_rng(25)
    I, J, V = _distinct(rng, 300, 25, 4000)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    L = a.export_layout(COLMAJOR)
    occ, is_sem, _ = _owners(L)
    heads = [s0 for s0 in range(512, len(occ), 512) if occ[s0:s0 + 512].any() and not is_sem[s0 + np.argmax(occ[s0:s0 + 512])]]
    assert len(heads) >= 2
    return a, -1.0, None, 1.0 + rng.random(25), None


def _edge_special_values(dsa, hip):
    V = np.array([NAN, INF, -INF, -0.0, 0.0, 5e-324, 2.5, -2.5, np.nextafter(2.5, 3.0), 1e300, -NAN])
    a = dsa.dynamicsparse(np.arange(1, 12), (np.arange(11) % 4) + 1, V, binding=hip)
    return a, 2.5, None, None, 5                          # -0.0, 0.0, the denormal and +-2.5 (<=); NaN and Inf stay


def _edge_special_values_inf(dsa, hip):
    a, _, _, _, _ = _edge_special_values(dsa, hip)
    return a, INF, None, None, 9                          # everything but the two NaN


def _edge_special_vectors(dsa, hip):
    """a value equal to its row threshold; a NaN, a negative and a -0.0 threshold; +Inf against +-Inf"""
    V = np.array([3.0, -3.0, INF, -INF, 0.0, -0.0, 1.0, NAN, 7.0])
    a = dsa.dynamicsparse(np.arange(1, 10), np.full(9, 1), V, 9, 1, binding=hip)
    tr = np.array([3.0, np.nextafter(3.0, 0.0), INF, INF, -0.0, NAN, -1.0, INF, 1e300])
    return a, -INF, tr, np.array([NAN]), 5                # rows 1, 3, 4, 5, 9


def _edge_wide_keys(dsa, hip):
    rng = np.random.default_rng(10)
    big = (1 << 31) + 5
    I = rng.integers(1, 300, 3000) + np.where(rng.random(3000) < 0.5, big, 0)
    J = rng.integers(1, 200, 3000) + np.where(rng.random(3000) < 0.5, big, 0)
    a = dsa.dynamicsparse(I, J, rng.standard_normal(3000), binding=hip)
    assert a.export_layout(COLMAJOR)["keys"].max() > 1 << 31 and a.export_layout(ROWMAJOR)["keys"].max() > 1 << 31
    return a, 0.6, None, None, None


def _edge_tombstones(dsa, hip):
    rng = np.random.default_rng(26)
    I, J, V = _distinct(rng, 200, 150, 5000)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    for c in (4, 70, 71, 150):
        a.deletecolumn(c)
    a.deleterow(9)
    assert a.info(COLMAJOR)["nb_partitions"] < a.info(COLMAJOR)["table_len"]
    tr, tc = _vectors("both", a.export_layout(COLMAJOR), *a.size(), seed=3)
    return a, 1.1, tr, tc, None


EDGES = dict(smallest=_edge_smallest, two_small_leaves=_edge_two_small_leaves, below_one_span=_edge_below_one_span, span_boundary=_edge_span_boundary,
             whole_word=_edge_whole_word, only_semaphores=_edge_only_semaphores, long_column=_edge_long_column,
             front_of_first_semaphore=_edge_front_of_first_semaphore, special_values=_edge_special_values,
             special_values_inf=_edge_special_values_inf, special_vectors=_edge_special_vectors, wide_keys=_edge_wide_keys,
             tombstones=_edge_tombstones)


@pytest.mark.gpu
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_kernel_edges(dsa, hip, edge):
    a, tol, tr, tc, want = EDGES[edge](dsa, hip)
    parts = [a.nbpartitions(o) for o in SIDES]
    dropped = _apply_and_check(a, tol, tr, tc, edge, how="dev" if tr is not None or tc is not None else "numpy")
    assert dropped > 0 and (want is None or dropped == want), (edge, dropped, want)
    if edge == "only_semaphores":
        assert a.nnz() == 0 and [a.nbpartitions(o) for o in SIDES] == parts
        for o in SIDES:
            L = a.export_layout(o)
            assert (L["keys"][L["occ"].astype(bool)] == 0).all() and L["occ"].sum() == parts[o] > 0
            assert np.array_equal(L["col_live"] != 0, L["semaphores"] != 0) and (L["col_live"] != 0).sum() == parts[o]
    # a second call on the result: a layout that came from the spread; whatever is left at or below the threshold is gone already
    before = _layout_bytes(a)
    assert _apply_and_check(a, tol, tr, tc, edge + " (again)") == 0
    assert _layout_bytes(a) == before


def _plan_matrix(dsa, hip, seed):
    """the shape of tests/test_spmv_plan.py: the smallest at which the plan applies"""
    M = N = 420_000
    NNZ = 1_260_000
    rng = np.random.default_rng(seed)
    I, J, V = rng.integers(1, M + 1, NNZ), rng.integers(1, N + 1, NNZ), rng.integers(1, 1 << 20, NNZ) * 2.0 ** -17
    a = dsa.dynamicsparse(I, J, V, M, N, binding=hip)
    x = 1.0 + rng.random(N)
    stats = lambda: (a.info(ROWMAJOR)["stat_spmv_plan"], a.info(ROWMAJOR)["stat_spmv_plan_builds"])
    y0 = [a.mul(x).copy() for _ in range(3)][-1]
    p0, b0 = stats()
    assert p0 > 0 and b0 == 1
    return a, x, y0, stats, M, N


@pytest.mark.gpu
def test_nothing_to_drop_changes_nothing_and_a_drop_rebuilds_the_plan_once(dsa, hip):
    a, x, y0, stats, M, N = _plan_matrix(dsa, hip, 147)
    p0, b0 = stats()
    epochs = lambda: [a.info(o)["stat_rebalances"] for o in SIDES]
    before, e0 = _layout_bytes(a), epochs()
    tr, tc = np.full(M, 2.0 ** -18), np.full(N, NAN)      # every value is a multiple of 2^-17: nothing is at or below 2^-18
    assert a.dropzeros() == 0 and a.droptol(-1.0) == 0 and a.droptol(2.0 ** -18, rows=tr, cols=tc) == 0
    assert a.count_droptol(INF) == a.nnz()                 # count-only: everything would go, nothing does
    assert _layout_bytes(a) == before and epochs() == e0   # unoccupied slots included
    assert stats() == (p0, b0)
    assert a.mul(x).tobytes() == y0.tobytes()
    assert stats() == (p0 + 1, b0)                         # still the plan it had
    # a dropping call: the plan is rebuilt exactly once
    tol = 2.0 ** -6
    nnz0 = a.nnz()
    want = a.count_droptol(tol)
    assert 0 < want < nnz0 and _layout_bytes(a) == before and stats() == (p0 + 1, b0)
    assert a.droptol(tol) == want and a.nnz() == nnz0 - want
    zs = [a.mul(x).copy() for _ in range(3)]
    assert stats()[1] == b0 + 1
    ptr, idx, val = a.to_csr()
    assert len(idx) == a.nnz() and (np.abs(val) > tol).all()
    fresh = dsa.dynamicsparse(np.repeat(np.arange(1, M + 1), np.diff(ptr)), idx + 1, val, M, N, binding=hip)
    w = fresh.mul(x)
    for z in zs:
        assert z.tobytes() == w.tobytes()
    assert zs[0].tobytes() != y0.tobytes()
    _clean(a)


def _random_pair(dsa, rng, bindings, m, n, nnz):
    I, J, V = _distinct(rng, m, n, nnz)
    V = rng.integers(1, 1 << 20, nnz) * 2.0 ** -17        # in (0, 8): positive, so that the products do not cancel
    return [dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in bindings]


@pytest.mark.gpu
def test_same_bits_twice_and_every_form_agrees(dsa, hip):
    rng = np.random.default_rng(31)
    I, J, V = _distinct(rng, 300, 400, 6000)
    V = rng.standard_normal(6000)
    tr, tc = np.where(rng.random(300) < 0.5, 0.3, -1.0), np.where(rng.random(400) < 0.3, 0.7, NAN)
    out, counts = [], []
    for how in ("numpy", "numpy", "list", "torch", "dev"):
        a = dsa.dynamicsparse(I, J, V, 300, 400, binding=hip)
        counts.append(_drop(a, 0.05, tr, tc, how))
        out.append(_layout_bytes(a))
        _clean(a)
    assert counts[0] > 0 and len(set(counts)) == 1
    for o in out[1:]:
        assert o == out[0]


@pytest.mark.gpu
def test_products_after_the_call_are_the_oracles(dsa, hip, oracle):
    rng = np.random.default_rng(33)
    m, n = 900, 700
    a, b = _random_pair(dsa, rng, (hip, oracle), m, n, 9000)
    L = b.export_layout(COLMAJOR)
    tr = np.where(rng.random(m) < 0.2, 4.0, -1.0)
    _apply_and_check(a, 1.0, tr, None, "products", how="torch")
    _zero_seq(b, *_cells(L, drop_mask(L, 1.0, tr, None, True)))
    assert a.nnz() == b.nnz() and 0 < b.nnz() < 9000
    _same_csr(dsa, a, b, "products")
    ptr, idx, val = expected_compressed(b.export_layout(ROWMAJOR), m)
    D = np.zeros((m, n))
    D[np.repeat(np.arange(m), np.diff(ptr)), idx] = val
    for tr_, nx, A in ((False, n, D), (True, m, D.T)):
        x = 1.0 + rng.random(nx)
        np.testing.assert_allclose(a.mul(x, transpose=tr_), b.mul(x, transpose=tr_), rtol=1e-12, atol=0)
        X = 1.0 + rng.random((nx, 3))
        np.testing.assert_allclose(a.matmul(X, transpose=tr_), A @ X, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_life_after_the_call(dsa, hip, oracle):
    """writes behind a droptol behave as behind the sequential zero writes: a few hundred set_batch writes that re-create dropped
    cells and hit emptied columns, content against the oracle twin; and, slot for slot, single writes on the layout the call left,
    imported into a PackedCSC of either library (the matrix itself has no layout import)"""
    rng = np.random.default_rng(35)
    m, n = 400, 300
    a, b = _random_pair(dsa, rng, (hip, oracle), m, n, 6000)
    L = b.export_layout(COLMAJOR)
    tc = np.full(n, -1.0)
    tc[rng.permutation(n)[:40]] = INF                      # 40 columns lose every cell
    mask = drop_mask(L, 1.5, None, tc, True)
    I0, J0 = _cells(L, mask)
    _apply_and_check(a, 1.5, None, tc, "life")
    _zero_seq(b, I0, J0)
    _same_csr(dsa, a, b, "life: before the writes")
    emptied = np.nonzero(tc == INF)[0] + 1
    k = 300
    pick = rng.integers(0, len(I0), k)
    I2, J2, V2 = I0[pick].copy(), J0[pick].copy(), 1.0 + rng.random(k)       # dropped cells again
    I2[:60], J2[:60] = rng.integers(1, m + 1, 60), rng.choice(emptied, 60)   # emptied columns
    V2[200:] = np.where(rng.random(100) < 0.5, 0.0, V2[200:])                # and deletes by zero among them
    for x in (b, a):
        x.set_batch(I2, J2, V2)
    _same_csr(dsa, a, b, "life: after the writes")
    assert a.nnz() == b.nnz()
    _clean(a)
    # slot for slot
    a2, _ = _random_pair(dsa, np.random.default_rng(35), (hip, oracle), m, n, 6000)
    a2.droptol(1.5, cols=tc)
    for o in SIDES:
        S = a2.export_layout(o)
        ps = [dsa.import_packedcsc_layout(S["keys"], S["vals"], S["occ"], S["info"]["segment_capacity"], S["semaphores"], binding=x)
              for x in (hip, oracle)]
        nparts = len(S["semaphores"])
        for t in range(250):
            key, part, v = int(rng.integers(1, 401)), int(rng.integers(1, nparts + 1)), float(rng.integers(0, 3)) * 0.5
            for p in ps:
                p[key, part] = v
        got, exp = ps[0].export_layout(), ps[1].export_layout()
        assert np.array_equal(got[2], exp[2]), ("slots", o)
        occ = exp[2].astype(bool)
        assert np.array_equal(got[0][occ], exp[0][occ]) and np.array_equal(_bits(got[1][occ]), _bits(exp[1][occ])), ("slots", o)
        assert np.array_equal(got[3], exp[3]), ("semaphores", o)


@pytest.mark.gpu
def test_errors_leave_everything_as_it_was(dsa, hip):
    import torch
    got = C.c_int64(-1)
    one = np.ones(4)
    d = torch.ones(4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    # fill mode
    f = dsa.dynamicsparse(binding=hip)
    f.set_batch([1, 2], [1, 2], [1.0, 0.0])
    assert hip._mat_droptol(f.h, 0.0, None, 0, None, 0, 0, C.byref(got)) == EMODE
    assert hip._mat_droptol(f.h, 0.0, one.ctypes.data_as(P_F64), 2, None, 0, 1, C.byref(got)) == EMODE
    assert hip._mat_droptol_dev(f.h, 0.0, None, 0, C.c_void_p(d.data_ptr()), 2, 0, C.byref(got)) == EMODE
    with pytest.raises(dsa.DsaError) as ei:
        f.dropzeros()
    assert ei.value.code == EMODE
    # a stored entry outside size(m): the vector forms refuse, the scalar form works
    sc = [c for c in MATRIX_CASES if c["name"] == "matrix_simple_use_A"][0]
    s = run_scenario(dsa, hip, sc)
    m, n = s.size()
    assert not _in_bounds(s.export_layout(COLMAJOR), m, n)
    before = _layout_bytes(s)
    for kw in (dict(rows=np.ones(m)), dict(cols=np.ones(n)), dict(rows=np.ones(m), cols=np.ones(n))):
        for call in (s.droptol, s.count_droptol):
            with pytest.raises(dsa.DsaBoundsError) as ei:
                call(INF, **kw)
            assert ei.value.code == EBOUNDS
    assert _layout_bytes(s) == before
    assert s.count_droptol(INF) == s.nnz() > 0
    _apply_and_check(s, _tol_of("median", s.export_layout(COLMAJOR)), None, None, "scalar form on column -1")
    # a matrix whose products come from a plan
    a, x, y0, stats, M, N = _plan_matrix(dsa, hip, 149)
    p0, b0 = stats()
    before = _layout_bytes(a)
    big_r, big_c = np.full(M, INF), np.full(N, INF)
    for kw in (dict(tol=NAN), dict(tol=NAN, rows=big_r, cols=big_c), dict(tol=INF, rows=big_r[:-1]), dict(tol=INF, cols=np.ones(N + 1)),
               dict(tol=INF, rows=big_r, cols=big_c[:5]), dict(tol=INF, rows=[]), dict(tol=INF, rows=big_c, cols=big_r[:0])):
        for call in (a.droptol, a.count_droptol):
            with pytest.raises(dsa.DsaArgumentError) as ei:
                call(kw["tol"], rows=kw.get("rows"), cols=kw.get("cols"))
            assert ei.value.code == EARG, kw
    D = torch.full((M,), float("inf"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for args in ((NAN, 0, 0, 0, 0), (INF, D.data_ptr(), M - 1, 0, 0), (INF, 0, 0, D.data_ptr(), N + 3), (NAN, D.data_ptr(), M, D.data_ptr(), N)):
        with pytest.raises(dsa.DsaArgumentError):
            a.droptol_dev(*args)
    with pytest.raises(dsa.DsaArgumentError):
        a.droptol(INF, rows=big_r, cols=D)                 # both of the same kind
    # nothing moved, and the products still come from the plan they had
    assert _layout_bytes(a) == before
    assert stats() == (p0, b0)
    assert a.mul(x).tobytes() == y0.tobytes()
    assert stats() == (p0 + 1, b0)
    _clean(a)
