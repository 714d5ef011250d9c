"""Batched insert of cells that are not stored yet (include/dsa.h: dsa_mat_insert_batch[_dev]; csrc/insert.hip).

Expected layouts never come from the kernels: `expected_after_insert` is numpy over a layout exported BEFORE the call.  It sorts the
ops by (partition, inner key), finds every op's predecessor slot with the reference's own bisection (src/finds.jl:29-57) inside the
partition's slot range, merges old cells and new items in that order, picks the capacity — the current one doubled the fewest times
that lets the merged count fit the root's upper bound floor(t * capacity), t = t_0 + ((t_h - t_0) / height) * height in Float64 with
the reference's thresholds t_h = 0.7, t_0 = 0.92 (src/pma.jl:58), one level more per doubling (src/pma.jl:143-151) — spreads the
merged sequence with `spread_slots` and rebuilds the tables.  On the CPU the helper is checked against the oracle: with an empty
batch it must give the oracle's rebalance_root layout, and for real batches its cell sequence, tables and size() must be those of the
oracle after set_batch of the same triples.  Comparisons are exact: occupancy, keys and tables equal, values bitwise.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode, expected_compressed
from test_delete_batch import _assert_layout, _bits, _clean, _layout_bytes, _owners, _same_csr, spread_slots

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
SIDES = (COLMAJOR, ROWMAJOR)
EARG, EMODE, EASSERT, EKEY = 1, 5, 6, 9
SKIP = 1
P_I64, P_F64, P_U8 = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
NAMES = ("mat_insert_batch", "mat_insert_batch_dev")
METHODS = ("insert_values", "insert_values_dev", "upsert")
KINDS = ("append", "fill", "both")
T_H, T_0 = 0.7, 0.92           # src/pma.jl:58
INS_TILE = 512                 # csrc/insert.h: slots per wave of the rank and merge passes
INS_BLOCK = 256                # ... ops per workgroup of the locate and place passes
BIG = (1 << 31) + 5


# ---------------------------------------------------------------------------------------------------------------- helper
class InsertError(Exception):
    def __init__(self, code, k):
        super().__init__(code, k)
        self.code, self.k = code, k


def root_bound(capacity, height):
    """the largest cell count the root accepts: count / capacity <= t_0 + t_d * height, t_d as _extend! leaves it"""
    t_d = (np.float64(T_H) - np.float64(T_0)) / np.float64(height)
    return int(np.floor((np.float64(T_0) + t_d * np.float64(height)) * np.float64(capacity)))


class _Finder:
    """find(array, key, from, to) of the reference on one exported layout, probe for probe (csrc/find_dev.h: d_find)"""

    def __init__(self, L):
        self.keys = L["keys"]
        pos = np.where(L["occ"].astype(bool), np.arange(1, len(L["occ"]) + 1), 0)
        self.prev = np.concatenate([[0], np.maximum.accumulate(pos)]) if len(pos) else np.zeros(1, dtype=np.int64)

    def _prev_occ(self, pos, lo):
        p = int(self.prev[pos]) if pos >= 1 else 0
        return p if p >= lo else lo - 1

    def find(self, key, frm, to):
        """1-based slot of the cell that holds `key`, else of the cell the new key goes behind"""
        while frm <= to:
            mid = (frm + to) >> 1
            i = self._prev_occ(mid, frm)
            if i < frm:
                frm = mid + 1
            else:
                ck = int(self.keys[i - 1])
                if ck > key:
                    to = i - 1
                elif ck < key:
                    frm = mid + 1
                else:
                    return i
        return self._prev_occ(to, 1) if to >= 1 else 0


def expected_after_insert(L, ops, own):
    """the layout of one orientation after the insert of ops = (I, J, V), from its layout L before.  own: L is the colmajor layout
    (partitions are the ops' columns, inner keys their rows).  Ops whose cell is stored are skipped and reported in `existing`;
    raises InsertError(code, op) for a key below 1, a repeated cell (the later op) and a new partition in the middle of the table"""
    I, J, V = (np.asarray(x).reshape(-1) for x in ops)
    I, J, V = I.astype(np.int64), J.astype(np.int64), V.astype(np.float64)
    n = len(I)
    part, key = (J, I) if own else (I, J)
    inf = L["info"]
    cap, seg, height, tl = inf["capacity"], inf["segment_capacity"], inf["height"], inf["table_len"]
    bad = np.nonzero((I < 1) | (J < 1))[0]
    if len(bad):
        raise InsertError(EKEY, int(bad[0]))
    order = np.lexsort((np.arange(n), key, part))                # stable: equal cells keep their input order
    occ = L["occ"].astype(bool)
    sems, ck, live = L["semaphores"][:tl], L["col_keys"][:tl], L["col_live"][:tl] != 0
    entry = {int(ck[p]): p for p in np.nonzero(live)[0].tolist()}
    s_sorted = np.sort(sems[sems != 0])
    finder = _Finder(L)
    last_occ = int(np.nonzero(occ)[0][-1]) + 1 if occ.any() else 0
    existing = np.zeros(n, dtype=bool)
    it_pred, it_key, it_val = [], [], []                         # the new items in merge order
    new_parts, preds = [], np.zeros(n, dtype=np.int64)
    prev = None
    for k in order.tolist():
        pk, kk = int(part[k]), int(key[k])
        if prev == (pk, kk):
            raise InsertError(EARG, k)
        prev = (pk, kk)
        if pk in entry:
            p = entry[pk]
            lo = int(sems[p])
            assert lo != 0
            nxt = np.searchsorted(s_sorted, lo, side="right")
            hi = int(s_sorted[nxt]) - 1 if nxt < len(s_sorted) else cap
            i = finder.find(kk, lo, hi)
            assert lo <= i <= hi
            preds[k] = i
            if int(L["keys"][i - 1]) == kk and i > lo:
                existing[k] = True
                continue
        else:
            if tl > 0 and not (live[tl - 1] and int(ck[tl - 1]) < pk):
                raise InsertError(EMODE, k)
            i = preds[k] = last_occ
            if not new_parts or new_parts[-1] != pk:
                new_parts.append(pk)
                it_pred.append(i), it_key.append(0), it_val.append(float(tl + len(new_parts)))
        it_pred.append(i), it_key.append(kk), it_val.append(V[k])
    src = np.nonzero(occ)[0]
    items = len(it_pred)
    m = len(src) + items
    # merge: an old cell at its slot, a new item behind its predecessor slot in sorted order
    primary = np.concatenate([src + 1, np.asarray(it_pred, dtype=np.int64)])
    secondary = np.concatenate([np.zeros(len(src), dtype=np.int64), 1 + np.arange(items)])
    mo = np.lexsort((secondary, primary))
    mk = np.concatenate([L["keys"][src], np.asarray(it_key, dtype=np.int64)])[mo]
    mv = np.concatenate([L["vals"][src], np.asarray(it_val, dtype=np.float64)])[mo]
    ncap, nheight = cap, height
    while m > root_bound(ncap, nheight):
        ncap, nheight = 2 * ncap, nheight + 1
    if items == 0 and cap == seg:
        dst = src                                                # a single leaf is not moved by a call that inserts nothing
    else:
        dst = spread_slots(ncap, m)
    o2 = np.zeros(ncap, dtype=np.uint8)
    k2, v2 = np.zeros(ncap, dtype=np.int64), np.zeros(ncap)
    o2[dst] = 1
    k2[dst], v2[dst] = mk, mv
    ntl = tl + len(new_parts)
    sems2 = np.zeros(ntl, dtype=np.int64)
    s = dst[k2[dst] == 0]
    sems2[v2[s].astype(np.int64) - 1] = s + 1
    ck2, live2 = np.zeros(ntl, dtype=np.int64), np.zeros(ntl, dtype=np.uint8)
    ck2[:tl], live2[:tl] = L["col_keys"][:tl], L["col_live"][:tl]
    ck2[tl:ntl], live2[tl:ntl] = np.asarray(new_parts, dtype=np.int64), 1
    return dict(keys=k2, vals=v2, occ=o2, semaphores=sems2, col_keys=ck2, col_live=live2, m=m, items=items, capacity=ncap,
                height=nheight, table_len=ntl, new_parts=len(new_parts), existing=existing, preds=preds, bound0=root_bound(cap, height),
                dst_of_items=dst[np.nonzero(mo >= len(src))[0]])


def _cells_by_partition(L):
    """{partition key: sorted [(key, value bits)]} of the live partitions"""
    occ, is_sem, part = _owners(L)
    live = (L["col_live"] != 0) & (L["semaphores"] != 0)
    out = {int(k): [] for k in L["col_keys"][live].tolist()}
    for s in np.nonzero(occ & ~is_sem & (part >= 1))[0].tolist():
        p = int(part[s]) - 1
        if live[p]:
            out[int(L["col_keys"][p])].append((int(L["keys"][s]), int(_bits(L["vals"][s:s + 1])[0])))
    return {k: sorted(v) for k, v in out.items()}


def _live_keys(L):
    tl = L["info"]["table_len"]
    k = L["col_keys"][:tl][(L["col_live"][:tl] != 0) & (L["semaphores"][:tl] != 0)].astype(np.int64)
    return k[k >= 1]


def _last_entry(L):
    """(key of the last table entry, whether it is live), (0, True) for an empty table"""
    tl = L["info"]["table_len"]
    return (int(L["col_keys"][tl - 1]), bool(L["col_live"][tl - 1])) if tl else (0, True)


def _stored(Lc):
    return {(r, c) for c, cells in _cells_by_partition(Lc).items() for r, _ in cells}


def make_batch(kind, x, seed=0):
    """(I, J, V) for a matrix x, sorted by (column, row): "append" = 3 new columns behind the last, "fill" = new cells inside live
    partitions of both orientations, "both"; None when the matrix has no room for the kind"""
    rng = np.random.default_rng(1000 + seed)
    Lc, Lr = x.export_layout(COLMAJOR), x.export_layout(ROWMAJOR)
    rows, cols = _live_keys(Lr), _live_keys(Lc)
    (lastc, livec), (lastr, liver) = _last_entry(Lc), _last_entry(Lr)
    stored = _stored(Lc)
    I, J = [], []
    if kind in ("append", "both"):
        if not livec:
            return None
        for q in range(1, 4):
            rr = rows[rng.permutation(len(rows))[:4]] if len(rows) else (np.arange(lastr + 1, lastr + 4) if liver else [])
            for r in np.sort(rr).tolist():
                I.append(r), J.append(max(lastc, 0) + q)
    if kind in ("fill", "both"):
        free = [(r, c) for c in cols.tolist() for r in rows.tolist() if (r, c) not in stored]
        for q in rng.permutation(len(free))[:12].tolist():
            I.append(free[q][0]), J.append(free[q][1])
    if not I:
        return None
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    o = np.lexsort((I, J))
    return I[o], J[o], 0.5 + np.arange(len(I), dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_insert_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    assert re.search(r"\bDSA_INS_SKIP_EXISTING\s*=\s*1\b", hdr) and dsa.INS_SKIP_EXISTING == 1
    for meth in METHODS:
        assert hasattr(dsa.DynamicSparseMatrix, meth), meth
    assert hasattr(dsa.Transposed, "insert_values") and hasattr(dsa.Transposed, "upsert")
    assert callable(dsa.insert_values) and callable(dsa.upsert)
    jl = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "julia", "DynamicSparseArraysAMD.jl")).read()
    assert re.search(r"ccall\(\(:dsa_mat_insert_batch, libdsa\), Int32,\s*\(Ptr\{Cvoid\}, Ptr\{Int64\}, Ptr\{Int64\}, Ptr\{Float64\}, Int64, Int32, Ptr\{UInt8\}\)", jl)
    assert "insert_values!" in jl and "upsert!" in jl


def test_oracle_binding_has_no_insert(dsa, oracle):
    for name in NAMES:
        assert not oracle.has(name), name
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    for call in (lambda: a.insert_values([3], [3], [1.0]), lambda: a.insert_values_dev(0, 0, 0, 0), lambda: a.upsert([1], [1], [2.0]),
                 lambda: dsa.insert_values(a, [3], [3], [1.0]), lambda: a.T.insert_values([3], [3], [1.0])):
        with pytest.raises(dsa.DsaArgumentError):
            call()


def test_root_bound_by_hand():
    """t_h = 0.7 at the root up to the rounding of t_0 + t_d * height: 0.7 * 256 = 179.2"""
    assert root_bound(256, 5) == 179 and root_bound(512, 6) == 358 and root_bound(8, 1) == 5


@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_helper_with_an_empty_batch_is_the_oracle_root_rebalance(dsa, oracle, sc):
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        return
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    for o in SIDES:
        L = b.export_layout(o)
        exp = expected_after_insert(L, none, o == COLMAJOR)
        assert exp["items"] == 0 and exp["capacity"] == L["info"]["capacity"] and exp["table_len"] == L["info"]["table_len"]
        c = run_scenario(dsa, oracle, sc)
        c.rebalance_root(o)
        _assert_layout(c.export_layout(o), exp, (sc["name"], o))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_helper_content_matches_set_batch_on_the_oracle(dsa, oracle, sc, kind):
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        return
    batch = make_batch(kind, b)
    if batch is None:
        return
    before = [b.export_layout(o) for o in SIDES]
    b.set_batch(*batch)
    for o in SIDES:
        exp, got = expected_after_insert(before[o], batch, o == COLMAJOR), b.export_layout(o)
        assert not exp["existing"].any() and exp["items"] == len(batch[0]) + exp["new_parts"]
        eo, go = exp["occ"].astype(bool), got["occ"].astype(bool)
        assert np.array_equal(exp["keys"][eo], got["keys"][go]), (sc["name"], kind, o, "cell sequence")
        assert np.array_equal(_bits(exp["vals"][eo]), _bits(got["vals"][go])), (sc["name"], kind, o, "cell sequence")
        L2 = dict(exp, info=dict(table_len=exp["table_len"]))
        assert _cells_by_partition(L2) == _cells_by_partition(got), (sc["name"], kind, o, "tables")
        assert exp["table_len"] == got["info"]["table_len"] and exp["m"] == got["info"]["nb_elements"]
        assert exp["capacity"] >= got["info"]["capacity"] or exp["m"] <= root_bound(exp["capacity"], exp["height"])
        # the helper's geometry is one the oracle takes, and its density one the oracle's next write accepts
        if (exp["semaphores"][:exp["table_len"]] != 0).all():
            p = dsa.import_packedcsc_layout(exp["keys"], exp["vals"], exp["occ"], before[o]["info"]["segment_capacity"], exp["semaphores"],
                                            binding=oracle)
            pi = p.info()
            assert (pi["capacity"], pi["height"], pi["nb_elements"]) == (exp["capacity"], exp["height"], exp["m"])
            assert exp["m"] <= root_bound(pi["capacity"], pi["height"])
            k2, v2, o2, s2 = p.export_layout()
            assert np.array_equal(o2, exp["occ"]) and np.array_equal(s2, exp["semaphores"][:exp["table_len"]])
    size0 = run_scenario(dsa, oracle, sc).size()
    assert b.size() == (max(size0[0], int(batch[0].max())), max(size0[1], int(batch[1].max())))


def test_helper_refuses_what_the_call_refuses(dsa, oracle):
    a = dsa.dynamicsparse([1, 2, 3, 2], [1, 2, 5, 5], [1.0, 2.0, 3.0, 4.0], binding=oracle)
    L = a.export_layout(COLMAJOR)
    for ops, code, k in ((([1, 0], [1, 2], [1.0, 1.0]), EKEY, 1), (([3, 1, 3], [6, 6, 6], [1.0, 2.0, 3.0]), EARG, 2),
                         (([1], [3], [1.0]), EMODE, 0)):
        with pytest.raises(InsertError) as ei:
            expected_after_insert(L, ops, True)
        assert (ei.value.code, ei.value.k) == (code, k)
    exp = expected_after_insert(L, ([1, 3, 1], [1, 5, 2], [9.0, 9.0, 9.0]), True)
    assert exp["existing"].tolist() == [True, True, False] and exp["items"] == 1


# ---------------------------------------------------------------------------------------------------------------- GPU
def _insert(a, I, J, V, how, skip=False):
    """-> the mask of skipped ops (None without skip)"""
    I, J, V = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64), np.asarray(V, dtype=np.float64)
    ex = "skip" if skip else "error"
    if how == "numpy":
        return a.insert_values(I, J, V, existing=ex)
    if how == "list":
        return a.insert_values(I.tolist(), J.tolist(), V.tolist(), existing=ex)
    if how == "transposed":
        return a.T.insert_values(J, I, V, existing=ex)
    import torch
    ti, tj, tv = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in (I, J, V))
    if how == "torch":
        r = a.insert_values(ti, tj, tv, existing=ex)
        return r.cpu().numpy() if skip else None
    mask = torch.full((max(len(I), 1),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.insert_values_dev(ti.data_ptr(), tj.data_ptr(), tv.data_ptr(), len(I), SKIP if skip else 0, d_existing=mask.data_ptr() if skip else None)
    return mask.cpu().numpy()[:len(I)].astype(bool) if skip else None


def _insert_and_check(a, I, J, V, what, how="numpy", skip=False):
    """the insert on the HIP matrix `a`: both layouts slot for slot against the helper, counters, size and the checker"""
    I, J, V = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64), np.asarray(V, dtype=np.float64)
    before = [a.export_layout(o) for o in SIDES]
    nnz0, size0 = a.nnz(), a.size()
    exp = [expected_after_insert(before[o], (I, J, V), o == COLMAJOR) for o in SIDES]
    assert np.array_equal(exp[0]["existing"], exp[1]["existing"]), what
    assert skip or not exp[0]["existing"].any(), what
    mask = _insert(a, I, J, V, how, skip)
    if skip:
        assert np.array_equal(mask, exp[0]["existing"]), what
    ins = int((~exp[0]["existing"]).sum())
    for o in SIDES:
        got = a.export_layout(o)
        inf = got["info"]
        assert inf["capacity"] == exp[o]["capacity"], (what, o, inf["capacity"], exp[o]["capacity"])
        _assert_layout(got, exp[o], (what, o))
        assert (inf["nb_elements"], inf["height"], inf["table_len"]) == (exp[o]["m"], exp[o]["height"], exp[o]["table_len"]), (what, o)
        assert inf["segment_capacity"] == before[o]["info"]["segment_capacity"], (what, o)
        assert a.nbpartitions(o) == before[o]["info"]["nb_partitions"] + exp[o]["new_parts"], (what, o)
    assert a.nnz() == nnz0 + ins, what
    keep = ~exp[0]["existing"]
    if keep.any():
        assert a.size() == (max(size0[0], int(I.max())), max(size0[1], int(J.max()))), what
    else:
        assert a.size() == size0
    _clean(a)
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_scenarios(dsa, hip, oracle, sc):
    a0 = run_scenario(dsa, hip, sc)
    if _in_fill_mode(dsa, a0):
        return
    for kind, how in zip(KINDS, ("numpy", "dev", "torch")):
        a, b = run_scenario(dsa, hip, sc), run_scenario(dsa, oracle, sc)
        batch = make_batch(kind, b)
        if batch is None:
            continue
        _insert_and_check(a, *batch, (sc["name"], kind), how)
        b.set_batch(*batch)
        assert a.nnz() == b.nnz() and a.size() == b.size()
        for o in SIDES:
            assert a.nbpartitions(o) == b.nbpartitions(o)
            assert _cells_by_partition(a.export_layout(o)) == _cells_by_partition(b.export_layout(o)), (sc["name"], kind, o)
        _same_csr(dsa, a, b, (sc["name"], kind))


def _matrix(seed, nrows=200, ncols=40, nnz=1500):
    """random triples; every row of 1 .. 3 exists, and column 1 has no cell in them: there is room in front of its first cell"""
    rng = np.random.default_rng(seed)
    I, J = rng.integers(1, nrows + 1, nnz), rng.integers(1, ncols + 1, nnz)
    keep = ~((J == 1) & (I <= 3))
    I, J = np.concatenate([I[keep], [1, 2, 3, 4]]), np.concatenate([J[keep], [2, 2, 2, 1]])
    return I, J, rng.standard_normal(len(I))


def _free_cells(a, count, rng):
    """`count` cells that are not stored, in live rows and live columns, sorted by (column, row)"""
    Lc, Lr = a.export_layout(COLMAJOR), a.export_layout(ROWMAJOR)
    rows, cols = _live_keys(Lr), _live_keys(Lc)
    stored = _stored(Lc)
    free = [(r, c) for c in cols.tolist() for r in rows.tolist() if (r, c) not in stored]
    assert len(free) >= count, (len(free), count)
    pick = sorted(free[q] for q in rng.permutation(len(free))[:count].tolist())
    I, J = np.asarray([p[0] for p in pick], dtype=np.int64), np.asarray([p[1] for p in pick], dtype=np.int64)
    o = np.lexsort((I, J))
    return I[o], J[o]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ("numpy", "dev"))
def test_edge_single_op_and_empty_matrix(dsa, hip, how):
    a = dsa.dynamicsparse(*_matrix(1), binding=hip)
    i1, j1 = _free_cells(a, 1, np.random.default_rng(1))
    exp = _insert_and_check(a, i1, j1, [-0.0], "n = 1", how)
    assert exp[0]["items"] == 1 and exp[1]["items"] == 1
    assert _bits(a.get_batch(i1, j1))[0] == 1 << 63               # -0.0 keeps its sign
    e = dsa.dynamicsparse(fill_mode=False, binding=hip)
    assert e.nnz() == 0 and e.info(COLMAJOR)["table_len"] == 0
    rng = np.random.default_rng(2)
    pairs = np.unique(rng.integers(1, 40, (300, 2)), axis=0)
    nan = np.float64(np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), dtype=np.float64)[0])
    V = rng.standard_normal(len(pairs))
    V[0], V[1] = nan, 0.0
    exp = _insert_and_check(e, pairs[:, 0], pairs[:, 1], V, "empty matrix", how)
    assert exp[0]["new_parts"] == len(np.unique(pairs[:, 1])) and (exp[0]["preds"] == 0).all()
    assert e.nnz() == len(pairs)                                 # the stored zero counts
    Lc = e.export_layout(COLMAJOR)
    assert int(_bits(np.asarray([nan]))[0]) in _bits(Lc["vals"][Lc["occ"].astype(bool)]).tolist()
    e.dropzeros()
    assert e.nnz() == len(pairs) - 1


@pytest.mark.gpu
def test_edge_first_semaphore_last_cell_and_only_new_partitions(dsa, hip):
    I, J, V = _matrix(3)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    L = a.export_layout(COLMAJOR)
    first = int(np.nonzero(L["occ"])[0][0]) + 1
    assert L["semaphores"][0] == first and int(_live_keys(L)[0]) == 1 and min(r for r, _ in _cells_by_partition(L)[1]) == 4
    exp = _insert_and_check(a, [2], [1], [1.25], "in front of the first cell", "dev")
    assert exp[0]["preds"][0] == first
    L = a.export_layout(COLMAJOR)
    cl = int(_live_keys(L)[-1])
    last = int(np.nonzero(L["occ"])[0][-1]) + 1
    exp = _insert_and_check(a, [int(I.max()) + 7], [cl], [2.5], "behind the last cell", "numpy")
    assert exp[0]["preds"][0] == last and exp[0]["new_parts"] == 0 and exp[1]["new_parts"] == 1
    r0, c0 = a.size()
    In, Jn = np.repeat(np.arange(r0 + 1, r0 + 6), 4), np.tile(np.arange(c0 + 1, c0 + 5), 5)
    exp = _insert_and_check(a, In, Jn, np.arange(20.0), "only new partitions", "torch")
    assert exp[0]["new_parts"] == 4 and exp[1]["new_parts"] == 5 and exp[0]["items"] == 24 and exp[1]["items"] == 25


def _column_ending_a_tile(L):
    """(slot, column) of a colmajor layout: the last cell of the column (or the semaphore of an empty one) in the last slot of a tile"""
    occ, is_sem, part = _owners(L)
    at = np.nonzero(occ)[0]
    for q, s0 in enumerate(at.tolist()):
        if (s0 + 1) % INS_TILE == 0 and part[s0] >= 1 and (q + 1 == len(at) or is_sem[at[q + 1]]):
            return s0 + 1, int(L["col_keys"][part[s0] - 1])
    raise AssertionError("no column ends in the last slot of a tile")


TILE_END_SEED = 5      # a seed at which a column ends in the last slot of a tile (asserted below)


@pytest.mark.gpu
def test_edge_runs_and_tiles(dsa, hip):
    # a predecessor in the last slot of a tile; its run of 700 items passes the tile's destination range.  The new cells lie in new
    # rows behind the last one: behind the last cell of their column, and 700 appended partitions in rowmajor
    I, J, V = _matrix(TILE_END_SEED, nrows=300, ncols=400, nnz=4000)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    L = a.export_layout(COLMAJOR)
    assert L["info"]["capacity"] >= 4 * INS_TILE
    s1, col = _column_ending_a_tile(L)
    rows = int(I.max()) + 1 + np.arange(700)
    exp = _insert_and_check(a, rows, np.full(700, col), np.arange(700.0), "tile end", "dev")
    assert (exp[0]["preds"] == s1).all() and s1 % INS_TILE == 0 and exp[1]["new_parts"] == 700
    # a run whose last item lands on the last slot of a destination tile
    I, J, V = _matrix(5, nrows=300, ncols=400, nnz=4000)
    b0 = dsa.dynamicsparse(I, J, V, binding=hip)
    L = b0.export_layout(COLMAJOR)
    col = int(_live_keys(L)[len(_live_keys(L)) // 2])
    rows = int(I.max()) + 1 + np.arange(600)
    hit = None
    for length in range(1, 601):
        e = expected_after_insert(L, (rows[:length], np.full(length, col), np.zeros(length)), True)
        if (int(e["dst_of_items"][-1]) + 1) % INS_TILE == 0:
            hit = length
            break
    assert hit is not None
    _insert_and_check(b0, rows[:hit], np.full(hit, col), np.arange(float(hit)), "run ends at a tile boundary", "numpy")
    # 3000 ops behind one predecessor: more than a wave, a workgroup and a tile of destination; two doublings
    I, J, V = _matrix(6, nrows=300, ncols=30, nnz=1150)
    c = dsa.dynamicsparse(I, J, V, binding=hip)
    Lc = c.export_layout(COLMAJOR)
    cap0 = Lc["info"]["capacity"]
    col = int(_live_keys(Lc)[3])
    rows = int(I.max()) + 1 + np.arange(3000)
    exp = _insert_and_check(c, rows, np.full(3000, col), np.arange(3000.0), "3000 behind one predecessor", "dev")
    assert len(np.unique(exp[0]["preds"])) == 1 and exp[0]["capacity"] == 4 * cap0, (cap0, exp[0]["capacity"])


@pytest.mark.gpu
def test_edge_capacity_rule_and_idempotence(dsa, hip):
    rng = np.random.default_rng(7)
    a = dsa.dynamicsparse(*_matrix(8, nrows=300, ncols=60, nnz=2500), binding=hip)
    inf = a.info(COLMAJOR)
    room = root_bound(inf["capacity"], inf["height"]) - inf["nb_elements"]
    assert room > 40 and inf["capacity"] > inf["segment_capacity"]
    I, J = _free_cells(a, 40, rng)
    exp = _insert_and_check(a, I, J, rng.standard_normal(40), "fits without growth", "dev")
    assert exp[0]["capacity"] == inf["capacity"] == a.info(COLMAJOR)["capacity"]
    # idempotence: the layout is the root rebalance's own
    for o in SIDES:
        if exp[o]["capacity"] != a.info(o)["segment_capacity"]:
            L0 = a.export_layout(o)
            a.rebalance_root(o)
            _assert_layout(a.export_layout(o), L0, ("idempotent", o))
    # exactly one doubling: one cell more than the root takes at the old capacity
    inf = a.info(COLMAJOR)
    bound = root_bound(inf["capacity"], inf["height"])
    need = bound - inf["nb_elements"] + 1
    I, J = _free_cells(a, need, rng)
    exp = _insert_and_check(a, I, J, rng.standard_normal(need), "one doubling", "numpy")
    assert exp[0]["bound0"] == bound and exp[0]["m"] == bound + 1 and exp[0]["capacity"] == 2 * inf["capacity"]
    assert a.info(COLMAJOR)["capacity"] == 2 * inf["capacity"] and a.info(COLMAJOR)["stat_extends"] == inf["stat_extends"] + 1


@pytest.mark.gpu
@pytest.mark.parametrize("side", SIDES, ids=("rows", "columns"))
def test_edge_wide_keys(dsa, hip, side):
    I, J, V = _matrix(9 + side, nnz=800)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    assert a.export_layout(COLMAJOR)["keys"].max() < 1 << 31 and a.export_layout(ROWMAJOR)["keys"].max() < 1 << 31
    cols, rows = np.unique(J), np.unique(I)
    fi, fj = _free_cells(a, 1, np.random.default_rng(side))
    if side == COLMAJOR:      # a row key beyond Int32: the colmajor keys widen, the rowmajor table takes a new row
        In, Jn = np.array([BIG, BIG, fi[0]]), np.array([cols[0], cols[3], fj[0]])
    else:
        In, Jn = np.array([rows[0], rows[5], fi[0]]), np.array([BIG, BIG, fj[0]])
    o = np.lexsort((In, Jn))
    In, Jn = In[o], Jn[o]
    _insert_and_check(a, In, Jn, [1.0, 2.0, 3.0], ("wide", side), "dev")
    assert a.export_layout(side)["keys"].max() == BIG
    assert a.get_batch(In, Jn).tolist() == [1.0, 2.0, 3.0]
    more = (np.array([BIG + 1]), cols[:1]) if side == COLMAJOR else (rows[:1], np.array([BIG + 1]))
    _insert_and_check(a, more[0], more[1], [4.0], ("wide, second batch", side), "numpy")


@pytest.mark.gpu
@pytest.mark.parametrize("side", SIDES, ids=("delete_columns", "delete_rows"))
def test_edge_tombstones_and_appended_partitions(dsa, hip, oracle, side):
    I, J, V = _matrix(11 + side, nnz=1200)
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    keys = np.unique(J if side == COLMAJOR else I)
    dead = keys[[len(keys) // 3, len(keys) // 2]]
    (a.delete_columns if side == COLMAJOR else a.delete_rows)(dead)
    for k in dead.tolist():
        (b.deletecolumn if side == COLMAJOR else b.deleterow)(k)
    assert a.nbpartitions(side) == a.info(side)["table_len"] - 2
    m, n = a.size()
    rows = np.unique(I)
    rows = rows[~np.isin(rows, dead)] if side == ROWMAJOR else rows
    In = np.concatenate([rows[:5], rows[2:7], [m + 1, m + 2]])
    Jn = np.concatenate([np.full(5, n + 1), np.full(5, n + 2), [n + 1, n + 3]])
    o = np.lexsort((In, Jn))
    In, Jn = In[o], Jn[o]
    exp = _insert_and_check(a, In, Jn, np.arange(1.0, 13.0), ("tombstones", side), "dev")
    assert exp[0]["new_parts"] == 3 and exp[1]["new_parts"] == 2
    assert a.nbpartitions(side) == a.info(side)["table_len"] - 2
    b.set_batch(In, Jn, np.arange(1.0, 13.0))
    _same_csr(dsa, a, b, ("tombstones", side))


@pytest.mark.gpu
def test_same_bits_twice(dsa, hip):
    I, J, V = _matrix(13, nrows=300, ncols=60, nnz=3000)
    rng = np.random.default_rng(14)
    out = []
    for _ in range(2):
        a = dsa.dynamicsparse(I, J, V, binding=hip)
        In, Jn = _free_cells(a, 900, np.random.default_rng(15))
        a.insert_values(In, Jn, np.arange(900.0))
        m, n = a.size()
        a.insert_values(np.tile(np.unique(I)[:50], 3), np.repeat([n + 1, n + 2, n + 3], 50), np.arange(150.0))
        out.append([a.export_layout(o) for o in SIDES])
    for o in SIDES:
        assert out[0][o]["occ"].tobytes() == out[1][o]["occ"].tobytes()
        _assert_layout(out[0][o], out[1][o], ("twice", o))


def _plan_matrix(dsa, hip, seed):
    """the shape of tests/test_spmv_plan.py: the smallest at which the plan applies"""
    M = N = 420_000
    NNZ = 1_260_000
    rng = np.random.default_rng(seed)
    I, J, V = rng.integers(1, M + 1, NNZ), rng.integers(1, N + 1, NNZ), rng.integers(1, 1 << 20, NNZ) * 2.0 ** -17
    return dsa.dynamicsparse(I, J, V, M, N, binding=hip), I, J, 1.0 + rng.random(N), M, N


def _raises(dsa, a, I, J, V, how, skip=False):
    with pytest.raises(dsa.DsaError) as ei:
        _insert(a, I, J, V, how, skip)
    return ei.value


@pytest.mark.gpu
def test_errors_and_skipped_batches_leave_everything_as_it_was(dsa, hip):
    import torch
    # fill mode
    f = dsa.dynamicsparse(binding=hip)
    f.set_batch([1, 2], [1, 2], [1.0, 2.0])
    for how in ("numpy", "dev"):
        assert _raises(dsa, f, [3], [3], [1.0], how).code == EMODE
    # a new partition in the middle of a table WITHOUT tombstones: ids would shift
    s = dsa.dynamicsparse([1, 2, 3, 9], [1, 2, 5, 5], [1.0, 2.0, 3.0, 4.0], binding=hip)
    sb, si = _layout_bytes(s), [s.info(o) for o in SIDES]
    for how in ("numpy", "dev"):
        e = _raises(dsa, s, [1, 2], [6, 3], [1.0, 1.0], how)
        assert e.code == EMODE and "use set_batch" in str(e) and "op 1 " in str(e)
        e = _raises(dsa, s, [5, 10], [1, 1], [1.0, 1.0], how)          # row 5 between rows 3 and 9
        assert e.code == EMODE and "use set_batch" in str(e) and "op 0 " in str(e)
    assert _layout_bytes(s) == sb and [s.info(o) for o in SIDES] == si and s.size() == (9, 5)
    # the shape at which products come from a plan
    a, I, J, x, M, N = _plan_matrix(dsa, hip, 147)
    cols, rows = np.unique(J), np.unique(I)
    a.deletecolumn(int(cols[10]))
    y0 = [a.mul(x).copy() for _ in range(3)][-1]
    stats = lambda: (a.info(ROWMAJOR)["stat_spmv_plan"], a.info(ROWMAJOR)["stat_spmv_plan_builds"])
    counters = lambda: [{k: v for k, v in a.info(o).items() if k != "hbm_bytes"} for o in SIDES]
    p0, b0 = stats()
    assert p0 > 0
    before, info0, size0, nnz0 = _layout_bytes(a), counters(), a.size(), a.nnz()
    absent_col = int(np.setdiff1d(np.arange(1, N + 1), cols)[0])
    r = int(rows[0])
    cases = [("stored", [r, I[5], rows[1]], [N + 1, J[5], N + 1], EARG, 1),
             ("duplicate", [r, rows[1], r], [N + 1, N + 2, N + 1], EARG, 2),
             ("key 0", [r, 0], [N + 1, N + 1], EKEY, None),
             ("column 0", [r, r], [N + 1, 0], EKEY, None),
             ("middle, tombstones", [r, rows[1]], [N + 1, absent_col], EMODE, 1),
             ("the deleted key", [r], [int(cols[10])], EMODE, 0)]
    for what, Ie, Je, code, op in cases:
        for how in ("numpy", "dev"):
            e = _raises(dsa, a, Ie, Je, np.ones(len(Ie)), how)
            assert e.code == code, (what, how, e.code, str(e))
            assert op is None or ("op %d " % op) in str(e), (what, how, str(e))
            assert code != EMODE or "use set_batch" in str(e)
    d = torch.ones(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert hip._mat_insert_batch_dev(a.h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), -1, 0, None) == EARG
    assert hip._mat_insert_batch_dev(a.h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), 1, 2, None) == EARG
    assert hip._mat_insert_batch_dev(a.h, None, None, None, 1, 0, None) == EARG
    # n = 0 and a batch that is skipped entirely: success, nothing happens
    assert hip._mat_insert_batch_dev(a.h, None, None, None, 0, 0, None) == 0
    assert a.insert_values([], [], []) is None
    for how in ("numpy", "dev", "torch"):
        mask = _insert(a, I[:300], J[:300], np.zeros(300), how, skip=True)
        assert mask.all() == (not np.isin(J[:300], cols[10]).any()) and mask.sum() == int((J[:300] != cols[10]).sum())
    # nothing moved, no counter changed, and the products still come from the plan they had
    assert _layout_bytes(a) == before and counters() == info0 and a.size() == size0 and a.nnz() == nnz0
    assert stats() == (p0, b0)
    assert a.mul(x).tobytes() == y0.tobytes()
    assert stats() == (p0 + 1, b0)
    _clean(a)
    # a batch that inserts drops the plan exactly once
    Ii, Ji = np.concatenate([rows[:400], rows[100:300]]), np.concatenate([np.full(400, N + 1), np.full(200, N + 3)])
    a.insert_values(Ii, Ji, np.full(600, 0.5))
    assert stats() == (p0 + 1, b0) and a.size() == (M, N + 3) and a.nnz() == nnz0 + 600
    x2 = np.concatenate([x, [1.5, 2.5, 3.5]])
    zs = [a.mul(x2).copy() for _ in range(3)]
    assert stats()[1] == b0 + 1
    ptr, idx, val = a.to_csr()
    fresh = dsa.dynamicsparse(np.repeat(np.arange(1, M + 1), np.diff(ptr)), idx + 1, val, M, N + 3, binding=hip)
    w = fresh.mul(x2)
    for z in zs:
        assert z.tobytes() == w.tobytes()
    _clean(a)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ("numpy", "dev", "transposed"))
def test_existing_skip(dsa, hip, how):
    I, J, V = _matrix(16, nnz=2000)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    rng = np.random.default_rng(17)
    fi, fj, _ = a.findnz()
    In, Jn = _free_cells(a, 150, rng)
    pick = rng.permutation(len(fi))[:100]
    Ib, Jb = np.concatenate([In, fi[pick]]), np.concatenate([Jn, fj[pick]])
    sh = rng.permutation(len(Ib))
    Ib, Jb = Ib[sh], Jb[sh]
    pairs = lambda i, j: np.asarray(i, dtype=np.int64) * (1 << 20) + np.asarray(j, dtype=np.int64)
    want = np.isin(pairs(Ib, Jb), pairs(fi, fj))
    assert want.sum() == 100
    exp = _insert_and_check(a, Ib, Jb, 1.0 + np.arange(len(Ib)), "skip", how, skip=True)
    assert np.array_equal(exp[0]["existing"], want)
    assert np.array_equal(a.get_batch(Ib[~want], Jb[~want]), (1.0 + np.arange(len(Ib)))[~want])
    e = _raises(dsa, a, Ib, Jb, np.ones(len(Ib)), "numpy")
    assert e.code == EARG and "op 0 " in str(e)


def _life_ops(rng, b, k):
    m, n = b.size()
    ptr, idx, _ = expected_compressed(b.export_layout(COLMAJOR), n)
    Jc = np.repeat(np.arange(1, n + 1), np.diff(ptr))
    pick = rng.integers(0, len(idx), k)
    I2, J2 = idx[pick] + 1, Jc[pick].copy()
    V2 = np.where(rng.random(k) < 0.35, 0.0, rng.standard_normal(k))
    new = rng.random(k) < 0.15
    J2[new] = n + 1 + rng.integers(0, 20, int(new.sum()))
    V2[new] = 1.0 + rng.random(int(new.sum()))
    return I2, J2, V2


@pytest.mark.gpu
@pytest.mark.parametrize("k", (200, 4000), ids=("small", "shrinks"))
def test_life_after_the_call(dsa, hip, oracle, k):
    """writes, deletes, updates and droptol behind an insert behave as behind the set_batch of the same triples"""
    rng = np.random.default_rng(19 + k)
    I, J = rng.integers(1, 401, 6000), rng.integers(1, 301, 6000)
    V = rng.integers(1, 1 << 20, 6000) * 2.0 ** -17
    a, b = (dsa.dynamicsparse(I, J, V, 400, 300, binding=x) for x in (hip, oracle))
    In, Jn = _free_cells(b, 500, rng)
    In, Jn = np.concatenate([In, np.arange(1, 41)]), np.concatenate([Jn, np.repeat([301, 302], 20)])
    Vn = 1.0 + rng.random(len(In))
    _insert_and_check(a, In, Jn, Vn, "life", "dev")
    b.set_batch(In, Jn, Vn)
    _same_csr(dsa, a, b, "life: after the insert")
    I2, J2, V2 = _life_ops(rng, b, k)
    if k > 1000:
        V2 = np.where(rng.random(k) < 0.95, 0.0, V2)
    for x in (b, a):
        x.set_batch(I2, J2, V2)
        x.deletecolumn(301)
        x.deletecolumn(int(Jn[0]))
    a.delete_rows([3, 4])
    b.deleterow(3), b.deleterow(4)
    _same_csr(dsa, a, b, "life: after the writes and deletes")
    fi, fj, fv = a.findnz()
    a.update_values(fi[:50], fj[:50], fv[:50] * 2.0)
    b.set_batch(fi[:50], fj[:50], fv[:50] * 2.0)
    tol = float(np.median(np.abs(fv)))
    a.droptol(tol)
    # the oracle's droptol: every small entry set to zero, which deletes it
    bptr, bidx, bval = expected_compressed(b.export_layout(COLMAJOR), b.size()[1])
    bJ = np.repeat(np.arange(1, b.size()[1] + 1), np.diff(bptr))
    small = np.abs(bval) <= tol
    b.set_batch(bidx[small] + 1, bJ[small], np.zeros(int(small.sum())))
    _same_csr(dsa, a, b, "life: after update_values and droptol")
    assert a.nnz() == b.nnz()
    _clean(a)


@pytest.mark.gpu
def test_products_after_the_call_are_the_oracles(dsa, hip, oracle):
    rng = np.random.default_rng(23)
    m, n = 900, 700
    I, J = rng.integers(1, m + 1, 9000), rng.integers(1, n + 1, 9000)
    V = rng.integers(1, 1 << 20, 9000) * 2.0 ** -17
    a, b = (dsa.dynamicsparse(I, J, V, m, n, binding=x) for x in (hip, oracle))
    In, Jn = _free_cells(b, 800, rng)
    In, Jn = np.concatenate([In, np.arange(1, 201)]), np.concatenate([Jn, n + 1 + (np.arange(200) // 20)])
    Vn = rng.integers(1, 1 << 20, len(In)) * 2.0 ** -17
    _insert_and_check(a, In, Jn, Vn, "products", "torch")
    b.set_batch(In, Jn, Vn)
    assert a.size() == b.size() == (m, n + 10)
    for tr, nx in ((False, n + 10), (True, m)):
        x = 1.0 + rng.random(nx)
        ya, yb = a.mul(x, transpose=tr), b.mul(x, transpose=tr)
        assert np.array_equal(_bits(ya), _bits(yb)), tr
    xi = np.sort(rng.permutation(n + 10)[:60] + 1)
    xv = 1.0 + rng.random(60)
    ra, rb = a.mul((xi, xv)), b.mul((xi, xv))
    # positive terms, at most 60 per row: the two summation orders differ by less than 60 roundings of the sum
    assert np.array_equal(np.asarray(ra[0]), np.asarray(rb[0])) and np.allclose(ra[1], rb[1], rtol=60 * 2.0 ** -53, atol=0.0)
    _same_csr(dsa, a, b, "products")


@pytest.mark.gpu
def test_upsert_is_set_batch_of_nonzero_values(dsa, hip, oracle):
    rng = np.random.default_rng(29)
    I, J = rng.integers(1, 201, 3000), rng.integers(1, 151, 3000)
    V = rng.standard_normal(3000)
    a, b = (dsa.dynamicsparse(I, J, V, 200, 150, binding=x) for x in (hip, oracle))
    fi, fj, _ = a.findnz()
    In, Jn = _free_cells(b, 300, rng)
    pick = rng.permutation(len(fi))[:250]
    Iu = np.concatenate([In, fi[pick], [7, 9]])
    Ju = np.concatenate([Jn, fj[pick], [151, 152]])
    sh = rng.permutation(len(Iu))
    Iu, Ju = Iu[sh], Ju[sh]
    Vu = 1.0 + rng.random(len(Iu))
    updated, inserted = a.upsert(Iu, Ju, Vu)
    assert (updated, inserted) == (250, 302)
    b.set_batch(Iu, Ju, Vu)
    assert a.nnz() == b.nnz() and a.size() == b.size()
    _same_csr(dsa, a, b, "upsert")
    assert dsa.upsert(a, Iu[:5], Ju[:5], Vu[:5] + 1.0) == (5, 0)
    _clean(a)
