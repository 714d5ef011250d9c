"""The general write from triples (include/dsa.h: dsa_mat_assemble[_dev]; csrc/assemble.hip): any triples folded to distinct cells,
the stored ones written in place, the others inserted.

Expected layouts never come from the kernels.  `fold_triples` is a plain Python left fold per cell; `expected_after_assemble` works on
layouts exported BEFORE the call: fold, split by what is stored, write the hits' values into both layouts (stored + s, or the
folded value), then `expected_after_insert` of tests/test_insert_batch.py on the misses per orientation.  On the CPU the model is
checked against the oracle: the ADD fold against dynamicsparse(I, J, V), SET against set_batch of the raw triples, ADD on dyadic
values against dynamicsparse of findnz(A) followed by the triples.  Comparisons are exact: occupancy, keys and tables equal, values
bitwise.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode
from test_delete_batch import _assert_layout, _bits, _clean, _layout_bytes, _owners
from test_insert_batch import (InsertError, _cells_by_partition, _free_cells, _live_keys, _matrix, _plan_matrix, _stored,
                               expected_after_insert, make_batch)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
SIDES = (COLMAJOR, ROWMAJOR)
EARG, EMODE, EASSERT, EKEY = 1, 5, 6, 9
SET, ADD = 0, 1
NAMES = ("mat_assemble", "mat_assemble_dev")
ASM_TILE = 1024                # csrc/assemble.h: sorted positions per workgroup of the flag, fold and scatter kernels
ASM_FOLD_INLINE = 64           # ... ops of one cell folded by the lane of the run's head
PAIR_SORT_TILE = 4096          # csrc/pairsort.h: elements per workgroup of a radix pass
BIG = (1 << 31) + 5
HOWS = ("numpy", "dev", "torch")
OPS = ("set", "add")


# ---------------------------------------------------------------------------------------------------------------- model
def _triples(I, J, V):
    I, J, V = (np.asarray(x).reshape(-1) for x in (I, J, V))
    return I.astype(np.int64), J.astype(np.int64), V.astype(np.float64)


def fold_triples(I, J, V, op):
    """(I', J', V', last) of the distinct cells in (column, row) order: "add" sums a cell's values one after the other in the order
    of the batch, "set" keeps the last; last = the index of the cell's last op.  A cell with one op keeps the bits of its V."""
    I, J, V = _triples(I, J, V)
    acc, last = {}, {}
    for k in range(len(I)):
        c = (int(J[k]), int(I[k]))
        if c in acc and op == "add":
            acc[c] = acc[c] + V[k]                                # one IEEE add on float64 scalars
        else:
            acc[c] = V[k]
        last[c] = k
    cells = sorted(acc)
    lk = np.asarray([last[c] for c in cells], dtype=np.int64)
    fv = V[lk].copy() if len(cells) else np.zeros(0)              # the bits of the last op: all of "set", the single ops of "add"
    if op == "add":
        for q, c in enumerate(cells):
            fv[q] = acc[c]
    return (np.asarray([c[1] for c in cells], dtype=np.int64), np.asarray([c[0] for c in cells], dtype=np.int64), fv, lk)


def _cell_slots(L, pk, kk):
    """0-based slot of the cell (partition key pk[q], inner key kk[q]) of layout L, -1 where it is not stored"""
    pk, kk = np.asarray(pk, dtype=np.int64), np.asarray(kk, dtype=np.int64)
    occ, is_sem, part = _owners(L)
    tl = L["info"]["table_len"]
    live = (L["col_live"][:tl] != 0) & (L["semaphores"][:tl] != 0)
    none = np.full(len(pk), -1, dtype=np.int64)
    s = np.nonzero(occ & ~is_sem & (part >= 1))[0]
    s = s[live[part[s] - 1]] if len(s) else s
    ids = np.nonzero(live)[0]
    if not len(s) or not len(pk):
        return none
    comp = (part[s].astype(np.int64) << 32) | L["keys"][s].astype(np.int64)      # (entry, key): keys are below 2^32 in this suite
    o = np.argsort(comp, kind="stable")
    comp, s = comp[o], s[o]
    lk = L["col_keys"][:tl][ids].astype(np.int64)
    oo = np.argsort(lk, kind="stable")
    pos = np.minimum(np.searchsorted(lk[oo], pk), len(lk) - 1)
    ok = (lk[oo][pos] == pk) & (kk >= 1) & (kk < (1 << 32))
    q = ((ids[oo][pos] + 1).astype(np.int64) << 32) | np.where(ok, kk, 0)
    at = np.minimum(np.searchsorted(comp, q), len(comp) - 1)
    return np.where(ok & (comp[at] == q), s[at], -1)


def expected_after_assemble(Lc, Lr, ops, op):
    """([colmajor, rowmajor] layouts, counts) after assemble(ops, op) from the layouts before.  Raises InsertError for a key below 1
    (the first such op) and for what the insert of the misses refuses (k: an index into the misses)"""
    I, J, V = _triples(*ops)
    bad = np.nonzero((I < 1) | (J < 1))[0]
    if len(bad):
        raise InsertError(EKEY, int(bad[0]))
    fI, fJ, fV, _ = fold_triples(I, J, V, op)
    sc, sr = _cell_slots(Lc, fJ, fI), _cell_slots(Lr, fI, fJ)
    hit = sc >= 0
    assert np.array_equal(hit, sr >= 0)
    out = []
    new = None
    for L, s in ((Lc, sc), (Lr, sr)):
        vals = L["vals"].copy()
        if hit.any():
            if new is None:
                new = vals[s[hit]] + fV[hit] if op == "add" else fV[hit]      # stored + s: one more IEEE add
            else:
                assert np.array_equal(_bits(L["vals"][s[hit]]), _bits(Lc["vals"][sc[hit]]))
            vals[s[hit]] = new
        out.append(dict(L, vals=vals))
    miss = ~hit
    counts = dict(distinct=len(fI), updated=int(hit.sum()), inserted=int(miss.sum()))
    if miss.any():
        out = [expected_after_insert(out[o], (fI[miss], fJ[miss], fV[miss]), o == COLMAJOR) for o in SIDES]
        for e in out:
            assert not e["existing"].any()
    return out, counts


def _content(L, own):
    """{(row, column): value bits} of an exported or expected layout"""
    if "info" not in L:
        L = dict(L, info=dict(table_len=L["table_len"]))
    return {((k, p) if own else (p, k)): b for p, cells in _cells_by_partition(L).items() for k, b in cells}


def _stored_cells(x):
    """the stored cells (row, column) of x with keys a batch may name (matrix_simple_use_A has a column -1), sorted"""
    return sorted(c for c in _stored(x.export_layout(COLMAJOR)) if c[0] >= 1 and c[1] >= 1)


def _hits_and_misses(x, rng, nh, nm, new_cols=0, new_rows=0):
    """cells of the matrix x in (column, row) order: nh stored ones, nm free ones inside live partitions, then new_cols / new_rows
    cells in columns / rows behind the tables"""
    Lc = x.export_layout(COLMAJOR)
    st = _stored_cells(x)
    assert len(st) >= nh
    pick = [st[q] for q in rng.permutation(len(st))[:nh].tolist()]
    fi, fj = _free_cells(x, nm, rng) if nm else (np.zeros(0, dtype=np.int64),) * 2
    m, n = x.size()
    rows = _live_keys(x.export_layout(ROWMAJOR))
    cells = pick + list(zip(fi.tolist(), fj.tolist()))
    cells += [(int(rows[q % len(rows)]), n + 1 + q // 3) for q in range(new_cols)]
    cells += [(m + 1 + q // 2, int(_live_keys(Lc)[q % 5])) for q in range(new_rows)]
    I, J = np.asarray([c[0] for c in cells], dtype=np.int64), np.asarray([c[1] for c in cells], dtype=np.int64)
    o = np.lexsort((I, J))
    return I[o], J[o]


def _with_runs(I, J, lengths, rng, op, shuffle=True):
    """the batch in which cell q (cells in (column, row) order) is addressed lengths[q] times: position p of the sorted order belongs
    to the cell whose run covers p.  "set" values encode k — the last op wins, and an unstable sort shows; "add" values are
    standard normal"""
    rep = np.repeat(np.arange(len(I)), lengths)
    if shuffle:
        rep = rep[rng.permutation(len(rep))]
    V = 0.5 + np.arange(len(rep), dtype=np.float64) if op == "set" else rng.standard_normal(len(rep))
    return I[rep], J[rep], V


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_assemble_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    for meth in ("assemble", "assemble_dev"):
        assert hasattr(dsa.DynamicSparseMatrix, meth), meth
    assert hasattr(dsa.Transposed, "assemble") and callable(dsa.assemble)
    jl = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "julia", "DynamicSparseArraysAMD.jl")).read()
    assert re.search(r"ccall\(\(:dsa_mat_assemble, libdsa\), Int32,\s*\(Ptr\{Cvoid\}, Int32, Ptr\{Int64\}, Ptr\{Int64\}, Ptr\{Float64\}, Int64, "
                     r"Ref\{Int64\}, Ref\{Int64\}, Ref\{Int64\}\)", jl)
    assert "assemble!" in jl and 'throw(ArgumentError("assemble!: op must be + or :set"))' in jl


def test_oracle_binding_has_no_assemble(dsa, oracle):
    for name in NAMES:
        assert not oracle.has(name), name
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    for call in (lambda: a.assemble([3], [3], [1.0]), lambda: a.assemble_dev(0, 0, 0, 0), lambda: dsa.assemble(a, [1], [1], [2.0]),
                 lambda: a.T.assemble([3], [3], [1.0], op="set")):
        with pytest.raises(dsa.DsaArgumentError):
            call()


def test_constants_are_those_of_the_header():
    csrc = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc")
    txt = open(os.path.join(csrc, "assemble.h")).read()
    assert int(re.search(r"constexpr int64_t ASM_TILE = (\d+);", txt).group(1)) == ASM_TILE
    assert int(re.search(r"constexpr int ASM_FOLD_INLINE = (\d+);", txt).group(1)) == ASM_FOLD_INLINE
    assert int(re.search(r"constexpr int64_t PAIR_SORT_TILE = (\d+);", open(os.path.join(csrc, "pairsort.h")).read()).group(1)) == PAIR_SORT_TILE


def test_add_fold_is_the_oracles_dynamicsparse(dsa, oracle):
    rng = np.random.default_rng(31)
    I, J, V = rng.integers(1, 30, 2000), rng.integers(1, 12, 2000), rng.standard_normal(2000)
    I[:300], J[:300] = 7, 3                                       # one long run
    fI, fJ, fV, _ = fold_triples(I, J, V, "add")
    assert len(fI) < 400
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    got = _content(b.export_layout(COLMAJOR), True)
    assert got == {(int(i), int(j)): int(x) for i, j, x in zip(fI, fJ, _bits(fV))}
    # by hand: the order of the batch decides
    assert fold_triples([1] * 4, [1] * 4, [1e16, 1.0, -1e16, 1.0], "add")[2].tolist() == [1.0]
    sI, sJ, sV, sl = fold_triples([2, 1, 2], [1, 1, 1], [1.0, -0.0, 3.0], "set")
    assert (sI.tolist(), sJ.tolist(), sl.tolist()) == ([1, 2], [1, 1], [1, 2]) and _bits(sV).tolist() == [1 << 63, _bits([3.0])[0]]


def _raw_set_batch(b, kind, rng):
    """raw triples for SET on the matrix b: the cells of make_batch in order, stored cells, and repeats of both with other values"""
    batch = make_batch(kind, b)
    if batch is None:
        return None
    I, J, _ = batch
    st = _stored_cells(b)
    hits = [st[q] for q in rng.permutation(len(st))[:6].tolist()]
    I = np.concatenate([I, np.asarray([h[0] for h in hits], dtype=np.int64)])
    J = np.concatenate([J, np.asarray([h[1] for h in hits], dtype=np.int64)])
    again = rng.integers(0, len(I), 2 * len(I))
    I, J = np.concatenate([I, I[again]]), np.concatenate([J, J[again]])
    return I, J, 1.0 + rng.random(len(I))


@pytest.mark.parametrize("kind", ("append", "fill"))
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_helper_set_matches_set_batch_on_the_oracle(dsa, oracle, sc, kind):
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        return
    raw = _raw_set_batch(b, kind, np.random.default_rng(37))
    if raw is None:
        return
    size0 = b.size()
    exp, counts = expected_after_assemble(b.export_layout(COLMAJOR), b.export_layout(ROWMAJOR), raw, "set")
    assert counts["distinct"] == counts["updated"] + counts["inserted"] and counts["inserted"] > 0
    nnz0 = b.nnz()
    b.set_batch(*raw)
    for o in SIDES:
        assert _content(exp[o], o == COLMAJOR) == _content(b.export_layout(o), o == COLMAJOR), (sc["name"], kind, o)
    assert b.nnz() == nnz0 + counts["inserted"]
    assert b.size() == (max(size0[0], int(raw[0].max())), max(size0[1], int(raw[1].max())))


def _dyadic(rng, n):
    return rng.integers(1, 513, n) / 8.0                           # multiples of 1/8 in (0, 64]: every summation order is exact


def test_helper_add_on_dyadic_values_is_the_oracles_dynamicsparse(dsa, oracle):
    rng = np.random.default_rng(41)
    I0, J0, _ = _matrix(41)
    b = dsa.dynamicsparse(I0, J0, _dyadic(rng, len(I0)), binding=oracle)
    I, J = _hits_and_misses(b, rng, 80, 60, new_cols=9, new_rows=6)
    I, J, _ = _with_runs(I, J, rng.integers(1, 5, len(I)), rng, "add")
    V = _dyadic(rng, len(I))
    exp, counts = expected_after_assemble(b.export_layout(COLMAJOR), b.export_layout(ROWMAJOR), (I, J, V), "add")
    assert counts["updated"] == 80 and counts["inserted"] == 75
    before = _content(b.export_layout(COLMAJOR), True)
    fi = np.asarray([c[0] for c in before], dtype=np.int64)
    fj = np.asarray([c[1] for c in before], dtype=np.int64)
    fv = np.asarray([before[c] for c in before], dtype=np.uint64).view(np.float64)
    want = dsa.dynamicsparse(np.concatenate([fi, I]), np.concatenate([fj, J]), np.concatenate([fv, V]), binding=oracle)
    for o in SIDES:
        assert _content(exp[o], o == COLMAJOR) == _content(want.export_layout(o), o == COLMAJOR), o
    # the vectorised lookup of the model finds what _stored finds
    Lc = b.export_layout(COLMAJOR)
    st = _stored(Lc)
    assert all(((int(i), int(j)) in st) == (s >= 0) for i, j, s in zip(I, J, _cell_slots(Lc, J, I)))


def test_helper_refuses_what_the_call_refuses(dsa, oracle):
    a = dsa.dynamicsparse([1, 2, 3, 2], [1, 2, 5, 5], [1.0, 2.0, 3.0, 4.0], binding=oracle)
    Lc, Lr = a.export_layout(COLMAJOR), a.export_layout(ROWMAJOR)
    for ops, code, k in ((([1, 0, 1], [1, 2, 2], [1.0, 1.0, 1.0]), EKEY, 1), (([1, 2], [1, -3], [1.0, 1.0]), EKEY, 1),
                         (([1, 1], [1, 3], [1.0, 1.0]), EMODE, 0)):
        for op in OPS:
            with pytest.raises(InsertError) as ei:
                expected_after_assemble(Lc, Lr, ops, op)
            assert (ei.value.code, ei.value.k) == (code, k)
    exp, counts = expected_after_assemble(Lc, Lr, ([1, 3, 1, 1], [1, 5, 2, 1], [9.0, 9.0, 9.0, 1.0]), "add")
    assert counts == dict(distinct=3, updated=2, inserted=1)
    assert _content(exp[0], True)[(1, 1)] == _bits([1.0 + (9.0 + 1.0)])[0]


# ---------------------------------------------------------------------------------------------------------------- GPU
def _call(a, I, J, V, op, how):
    I, J, V = _triples(I, J, V)
    if how == "numpy":
        return a.assemble(I, J, V, op=op)
    if how == "list":
        return a.assemble(I.tolist(), J.tolist(), V.tolist(), op=op)
    if how == "transposed":
        return a.T.assemble(J, I, V, op=op)
    import torch
    ti, tj, tv = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in (I, J, V))
    if how == "torch":
        return a.assemble(ti, tj, tv, op=op)
    torch.cuda.synchronize()
    out = a.assemble_dev(ti.data_ptr(), tj.data_ptr(), tv.data_ptr(), len(I), ADD if op == "add" else SET)
    a.sync()
    return out


def _assemble_and_check(a, I, J, V, op, what, how="numpy"):
    """assemble on the HIP matrix `a`: both layouts slot for slot against the model, the counts, counters, size and the checker"""
    I, J, V = _triples(I, J, V)
    before = [a.export_layout(o) for o in SIDES]
    nnz0, size0 = a.nnz(), a.size()
    exp, counts = expected_after_assemble(before[0], before[1], (I, J, V), op)
    got = _call(a, I, J, V, op, how)
    assert got == (counts["distinct"], counts["updated"], counts["inserted"]), (what, got, counts)
    for o in SIDES:
        L = a.export_layout(o)
        inf = L["info"]
        _assert_layout(L, exp[o], (what, o))
        if counts["inserted"]:
            assert (inf["capacity"], inf["nb_elements"], inf["height"], inf["table_len"]) == \
                (exp[o]["capacity"], exp[o]["m"], exp[o]["height"], exp[o]["table_len"]), (what, o)
            assert a.nbpartitions(o) == before[o]["info"]["nb_partitions"] + exp[o]["new_parts"], (what, o)
        else:
            assert {k: v for k, v in inf.items() if k != "hbm_bytes"} == {k: v for k, v in before[o]["info"].items() if k != "hbm_bytes"}, (what, o)
    assert a.nnz() == nnz0 + counts["inserted"], what
    want = (max(size0[0], int(I.max())), max(size0[1], int(J.max()))) if len(I) else size0
    assert a.size() == want, (what, a.size(), size0, want)
    _clean(a)
    return exp, counts


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_scenarios(dsa, hip, oracle, sc):
    a0 = run_scenario(dsa, hip, sc)
    if _in_fill_mode(dsa, a0):
        return
    rng = np.random.default_rng(43)
    for how, op, kind in zip(HOWS + HOWS, OPS * 3, ("append", "fill", "both") * 2):
        a = run_scenario(dsa, hip, sc)
        raw = _raw_set_batch(a, kind, rng)
        if raw is None:
            continue
        _, counts = _assemble_and_check(a, *raw, op, (sc["name"], how, op), how)
        # a second batch through the transposed view: stored cells, some of them twice
        st = _stored_cells(a)
        pick = rng.integers(0, len(st), 40)
        I2, J2 = (np.asarray([st[q][t] for q in pick.tolist()], dtype=np.int64) for t in (0, 1))
        V2 = rng.standard_normal(40)
        before = [a.export_layout(o) for o in SIDES]
        exp, c2 = expected_after_assemble(before[0], before[1], (I2, J2, V2), op)
        assert a.T.assemble(J2, I2, V2, op=op) == (c2["distinct"], c2["updated"], 0)
        for o in SIDES:
            _assert_layout(a.export_layout(o), exp[o], (sc["name"], "transposed", o))
        _clean(a)


RUNS = (1, 2, 63, 64, 65, 128, 129, 200)


def _run_case(name, rng):
    """(hits, misses, lengths builder) of the run-length cases: lengths[q] per cell q of the (column, row) order"""
    if name.startswith("len"):
        R = int(name[3:])
        return 3, 2, lambda c: np.where(np.arange(c) == 2, R, 1)
    if name == "all":
        return 10, 6, lambda c: np.concatenate([RUNS, RUNS])
    at = {"wave": 64, "tile": ASM_TILE, "sort": PAIR_SORT_TILE}.get(name)
    if at is not None:                  # a run of 10 over positions at - 4 .. at + 5, and one of 100 that starts at at + 60
        return 300, at - 4 + 60, lambda c: np.where(np.arange(c) == at - 4, 10, np.where(np.arange(c) == at - 4 + 1 + 54, 100, 1))
    if name == "run_last":
        return 40, 30, lambda c: np.where(np.arange(c) == c - 1, 70, 1)
    if name == "head_last":
        return 40, 30, lambda c: np.where(np.arange(c) == c - 2, 66, 1)
    raise AssertionError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["len%d" % r for r in RUNS] + ["all", "wave", "tile", "sort", "run_last", "head_last"])
def test_run_lengths_and_their_places(dsa, hip, name, op):
    rng = np.random.default_rng(sum(map(ord, name)))
    a = dsa.dynamicsparse(*_matrix(47), binding=hip)
    nh, nm, lengths = _run_case(name, rng)
    I, J = _hits_and_misses(a, rng, nh, nm)
    L = lengths(len(I))
    assert len(L) == len(I) and L.min() >= 1
    Ib, Jb, Vb = _with_runs(I, J, L, rng, op)
    # where the runs lie in the sorted order
    start = np.concatenate([[0], np.cumsum(L)[:-1]])
    if name in ("wave", "tile", "sort"):
        at = {"wave": 64, "tile": ASM_TILE, "sort": PAIR_SORT_TILE}[name]
        assert ((start < at) & (start + L > at) & (L > 1)).any()
    if name == "run_last":
        assert start[-1] + L[-1] == len(Ib) and L[-1] > ASM_FOLD_INLINE
    if name == "head_last":
        assert L[-1] == 1 and start[-1] == len(Ib) - 1 and L[-2] > ASM_FOLD_INLINE
    _, counts = _assemble_and_check(a, Ib, Jb, Vb, op, (name, op), "dev")
    assert counts == dict(distinct=len(I), updated=nh, inserted=nm)
    if op == "set":                     # the last op of every cell, whatever the order of the batch
        got = a.get_batch(Ib, Jb)
        last = {}
        for k, c in enumerate(zip(Ib.tolist(), Jb.tolist())):
            last[c] = Vb[k]
        assert got.tolist() == [last[c] for c in zip(Ib.tolist(), Jb.tolist())]


@pytest.mark.gpu
@pytest.mark.parametrize("n", (ASM_TILE - 1, ASM_TILE, ASM_TILE + 1, PAIR_SORT_TILE - 1, PAIR_SORT_TILE, PAIR_SORT_TILE + 1))
def test_batch_sizes_at_the_tile_edges(dsa, hip, n):
    rng = np.random.default_rng(n)
    a = dsa.dynamicsparse(*_matrix(53), binding=hip)
    cells = n - 3 * 9                    # nine runs of 4, the rest single ops
    I, J = _hits_and_misses(a, rng, 500, cells - 500)
    L = np.ones(cells, dtype=np.int64)
    L[rng.permutation(cells)[:9]] = 4
    assert L.sum() == n
    op = OPS[n % 2]
    Ib, Jb, Vb = _with_runs(I, J, L, rng, op)
    _, counts = _assemble_and_check(a, Ib, Jb, Vb, op, ("size", n), "dev" if n % 2 else "numpy")
    assert counts == dict(distinct=cells, updated=500, inserted=cells - 500)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ("numpy", "dev"))
def test_summation_order(dsa, hip, how):
    a = dsa.dynamicsparse([1, 2, 3], [1, 1, 2], [0.5, 2.0, 3.0], binding=hip)
    V = [1e16, 1.0, -1e16, 1.0]
    # a new cell (3, 1) and the stored cell (1, 1), interleaved: ((1e16 + 1.0) - 1e16) + 1.0 == 1.0; a pairwise or reversed sum gives 0.0
    I = [3, 1, 3, 1, 3, 1, 3, 1]
    exp, counts = _assemble_and_check(a, I, [1] * 8, np.repeat(V, 2), "add", "order", how)
    assert counts == dict(distinct=2, updated=1, inserted=1)
    assert a.get_batch([3, 1], [1, 1]).tolist() == [1.0, 0.5 + 1.0]


@pytest.mark.gpu
def test_degenerate_shapes(dsa, hip):
    rng = np.random.default_rng(59)
    nan = np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), dtype=np.float64)[0]
    for op in OPS:
        a = dsa.dynamicsparse(*_matrix(59), binding=hip)
        fi, fj, _ = a.findnz()
        mi, mj = _free_cells(a, 1, rng)
        _, c = _assemble_and_check(a, mi, mj, [2.5], op, "n = 1, a miss", "dev")
        assert c == dict(distinct=1, updated=0, inserted=1)
        _, c = _assemble_and_check(a, fi[:1], fj[:1], [-1.5], op, "n = 1, a hit", "dev")
        assert c == dict(distinct=1, updated=1, inserted=0)
        _, c = _assemble_and_check(a, np.full(500, fi[7]), np.full(500, fj[7]), rng.standard_normal(500), op, "one cell, a hit", "numpy")
        assert c == dict(distinct=1, updated=1, inserted=0)
        mi, mj = _free_cells(a, 1, rng)
        _, c = _assemble_and_check(a, np.full(300, mi[0]), np.full(300, mj[0]), rng.standard_normal(300), op, "one cell, a miss", "dev")
        assert c == dict(distinct=1, updated=0, inserted=1)
        I, J = _hits_and_misses(a, rng, 200, 150, new_cols=6)
        sh = rng.permutation(len(I))
        _, c = _assemble_and_check(a, I[sh], J[sh], rng.standard_normal(len(I)), op, "all distinct", "torch")
        assert c == dict(distinct=356, updated=200, inserted=156)
        # hits only: nothing but values changes (the model's layouts are the old ones with other values; counters compared inside)
        lb = _layout_bytes(a)
        pick = rng.integers(0, len(fi), 700)
        _, c = _assemble_and_check(a, fi[pick], fj[pick], rng.standard_normal(700), op, "hits only", "dev")
        assert c["inserted"] == 0 and c["updated"] == len(np.unique(pick))
        la = _layout_bytes(a)
        for o in SIDES:
            assert [x == y for x, y in zip(lb[o], la[o])] == [True, False, True, True, True, True]
        mi, mj = _free_cells(a, 400, rng)
        rep = rng.integers(0, 400, 900)
        _, c = _assemble_and_check(a, mi[rep], mj[rep], rng.standard_normal(900), op, "misses only", "numpy")
        assert c["updated"] == 0 and c["inserted"] == len(np.unique(rep))
    # an empty matrix
    for op in OPS:
        e = dsa.dynamicsparse(fill_mode=False, binding=hip)
        pairs = rng.integers(1, 25, (300, 2))
        assert len(np.unique(pairs, axis=0)) < 300
        _, c = _assemble_and_check(e, pairs[:, 0], pairs[:, 1], rng.standard_normal(300), op, "empty matrix", "dev")
        assert c["updated"] == 0 and e.nnz() == c["inserted"] == len(np.unique(pairs, axis=0))
    # bits under SET: -0.0 and a NaN payload, on a hit and on a miss, each behind an op that it overrides
    a = dsa.dynamicsparse(*_matrix(61), binding=hip)
    fi, fj, _ = a.findnz()
    mi, mj = _free_cells(a, 2, rng)
    I, J = np.asarray([fi[0], mi[0], fi[1], mi[1]] * 2), np.asarray([fj[0], mj[0], fj[1], mj[1]] * 2)
    V = np.asarray([1.0, 2.0, 3.0, 4.0, -0.0, -0.0, nan, nan])
    _assemble_and_check(a, I, J, V, "set", "bits", "dev")
    assert _bits(a.get_batch(I[:4], J[:4])).tolist() == [1 << 63, 1 << 63, 0x7FF8000000000123, 0x7FF8000000000123]
    # a cancelling sum is a stored zero, on a new cell and on a stored one
    a = dsa.dynamicsparse([1, 2], [1, 2], [4.0, 5.0], binding=hip)
    _, c = _assemble_and_check(a, [2, 1, 2, 1], [1, 1, 1, 1], [1.5, -1.0, -1.5, -3.0], "add", "cancel", "numpy")
    assert c == dict(distinct=2, updated=1, inserted=1) and a.nnz() == 3
    assert a.get_batch([1, 2], [1, 1]).tolist() == [0.0, 0.0]
    assert a.dropzeros() == 2 and a.nnz() == 1
    _clean(a)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_mixed_batch(dsa, hip, op):
    rng = np.random.default_rng(67)
    a = dsa.dynamicsparse(*_matrix(67), binding=hip)
    m, n = a.size()
    I, J = _hits_and_misses(a, rng, 300, 200, new_cols=12, new_rows=8)
    rows, cols = _live_keys(a.export_layout(ROWMAJOR)), _live_keys(a.export_layout(COLMAJOR))
    # one key beyond Int32, once as a row (in a live column) and once as a column (in a live row)
    I, J = np.concatenate([I, [BIG, rows[3]]]), np.concatenate([J, [cols[2], BIG]])
    o = np.lexsort((I, J))
    I, J = I[o], J[o]
    L = rng.integers(1, 4, len(I))
    L[[0, len(I) // 2, len(I) - 1]] = 70
    Ib, Jb, Vb = _with_runs(I, J, L, rng, op)
    exp, counts = _assemble_and_check(a, Ib, Jb, Vb, op, "mixed", "dev")
    assert counts == dict(distinct=522, updated=300, inserted=222)
    assert exp[0]["new_parts"] == 5 and exp[1]["new_parts"] == 5 and a.size() == (BIG, BIG)
    assert a.export_layout(COLMAJOR)["keys"].max() == BIG and a.export_layout(ROWMAJOR)["keys"].max() == BIG


def _raises(dsa, a, I, J, V, op, how):
    with pytest.raises(dsa.DsaError) as ei:
        _call(a, I, J, V, op, how)
    return ei.value


@pytest.mark.gpu
def test_errors_leave_everything_as_it_was_and_writes_drop_the_plan(dsa, hip):
    import torch
    f = dsa.dynamicsparse(binding=hip)
    f.set_batch([1, 2], [1, 2], [1.0, 2.0])
    for how in ("numpy", "dev"):
        assert _raises(dsa, f, [3], [3], [1.0], "add", how).code == EMODE
    a, I, J, x, M, N = _plan_matrix(dsa, hip, 149)
    cols, rows = np.unique(J), np.unique(I)
    y0 = [a.mul(x).copy() for _ in range(3)][-1]
    stats = lambda: (a.info(ROWMAJOR)["stat_spmv_plan"], a.info(ROWMAJOR)["stat_spmv_plan_builds"])
    counters = lambda: [{k: v for k, v in a.info(o).items() if k != "hbm_bytes"} for o in SIDES]
    p0, b0 = stats()
    assert p0 > 0
    before, info0, size0, nnz0 = _layout_bytes(a), counters(), a.size(), a.nnz()
    absent_col = int(np.setdiff1d(np.arange(1, N + 1), cols)[0])
    r = int(rows[0])
    cases = [("key 0, overridden", [0, I[5], 0], [J[5], J[5], J[5]], EKEY, None),
             ("column 0", [r, r], [N + 1, 0], EKEY, None),
             ("a negative key", [r, -4], [N + 1, N + 1], EKEY, None),
             ("middle, with hits", [I[5], r, I[6], r], [J[5], absent_col, J[6], absent_col], EMODE, 3)]
    for what, Ie, Je, code, last in cases:
        for how in ("numpy", "dev"):
            for op in OPS:
                e = _raises(dsa, a, Ie, Je, np.ones(len(Ie)), op, how)
                assert e.code == code, (what, how, e.code, str(e))
                if code == EMODE:      # the message names an op of THIS batch and the cell, never a folded index
                    assert "use set_batch" in str(e) and ("op %d " % last) in str(e) and ("(%d, %d)" % (r, absent_col)) in str(e), str(e)
    d = torch.ones(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p = C.c_void_p(d.data_ptr())
    assert hip._mat_assemble_dev(a.h, 2, p, p, p, 1, None, None, None) == EARG
    assert hip._mat_assemble_dev(a.h, -1, p, p, p, 1, None, None, None) == EARG
    assert hip._mat_assemble_dev(a.h, ADD, p, p, p, -1, None, None, None) == EARG
    assert hip._mat_assemble_dev(a.h, ADD, None, p, p, 1, None, None, None) == EARG
    assert hip._mat_assemble_dev(a.h, ADD, p, p, None, 1, None, None, None) == EARG
    with pytest.raises(dsa.DsaArgumentError):
        a.assemble([1], [1], [1.0], op="mul")
    # n = 0: success, nothing happens
    assert hip._mat_assemble_dev(a.h, SET, None, None, None, 0, None, None, None) == 0
    assert a.assemble([], [], []) == (0, 0, 0)
    assert _layout_bytes(a) == before and counters() == info0 and a.size() == size0 and a.nnz() == nnz0
    assert stats() == (p0, b0)
    assert a.mul(x).tobytes() == y0.tobytes()                    # ... from the plan it had
    assert stats() == (p0 + 1, b0)
    _clean(a)
    # a call that writes drops the plan: hits, duplicates and two new columns in one batch
    Ii = np.concatenate([I[:300], I[:300], rows[:200], rows[100:200]])
    Ji = np.concatenate([J[:300], J[:300], np.full(200, N + 1), np.full(100, N + 3)])
    Vi = np.random.default_rng(150).integers(1, 1 << 20, len(Ii)) * 2.0 ** -17
    Lc, Lr = a.export_layout(COLMAJOR), a.export_layout(ROWMAJOR)
    exp, counts = expected_after_assemble(Lc, Lr, (Ii, Ji, Vi), "add")
    assert a.assemble(Ii, Ji, Vi) == (counts["distinct"], counts["updated"], counts["inserted"]) and counts["inserted"] == 300
    assert stats() == (p0 + 1, b0) and a.size() == (M, N + 3) and a.nnz() == nnz0 + 300
    for o in SIDES:
        _assert_layout(a.export_layout(o), exp[o], ("plan", o))
    x2 = np.concatenate([x, [1.5, 2.5, 3.5]])
    zs = [a.mul(x2).copy() for _ in range(3)]
    assert stats()[1] == b0 + 1
    E = exp[0]
    occ, is_sem, part = _owners(E)
    cell = occ & ~is_sem
    y = np.bincount(E["keys"][cell] - 1, weights=E["vals"][cell] * x2[E["col_keys"][part[cell] - 1] - 1], minlength=M)
    for z in zs:
        np.testing.assert_allclose(z, y, rtol=1e-12, atol=0)
    # hits only drop it too (the content epoch moves), and nothing else changes
    p1, b1 = stats()
    assert a.assemble(I[:50], J[:50], np.ones(50), op="set")[2] == 0
    zs = [a.mul(x2).copy() for _ in range(3)]
    assert stats()[1] == b1 + 1
    _clean(a)


@pytest.mark.gpu
def test_same_bits_twice(dsa, hip):
    I, J, V = _matrix(71, nrows=300, ncols=60, nnz=3000)
    out = []
    for _ in range(2):
        rng = np.random.default_rng(72)
        a = dsa.dynamicsparse(I, J, V, binding=hip)
        Ic, Jc = _hits_and_misses(a, rng, 600, 700, new_cols=30)
        Ib, Jb, Vb = _with_runs(Ic, Jc, rng.integers(1, 90, len(Ic)), rng, "add")
        a.assemble(Ib, Jb, Vb)
        out.append(_layout_bytes(a))
    assert out[0] == out[1]


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_life_after_the_call(dsa, hip, oracle, op):
    """single writes, a deletecolumn, a set_batch and a second assemble behind an assemble: the content is the oracle's, driven
    with the folded triples (ADD on dyadic values: with get + set)"""
    rng = np.random.default_rng(73)
    I0, J0, _ = _matrix(73)
    V0 = _dyadic(rng, len(I0))
    a, b = (dsa.dynamicsparse(I0, J0, V0, binding=x) for x in (hip, oracle))

    def both(new_cols):
        I, J = _hits_and_misses(b, rng, 150, 100, new_cols=new_cols)
        Ib, Jb, _ = _with_runs(I, J, rng.integers(1, 6, len(I)), rng, op)
        Vb = _dyadic(rng, len(Ib))
        _assemble_and_check(a, Ib, Jb, Vb, op, ("life", op), "dev")
        fI, fJ, fV, _ = fold_triples(Ib, Jb, Vb, op)
        b.set_batch(fI, fJ, fV + b.get_batch(fI, fJ) if op == "add" else fV)

    def same():
        assert a.nnz() == b.nnz() and a.size() == b.size()
        for o in SIDES:
            assert _content(a.export_layout(o), o == COLMAJOR) == _content(b.export_layout(o), o == COLMAJOR), o

    both(9)
    same()
    m, n = b.size()
    for _ in range(200):
        i, j, v = int(rng.integers(1, m + 1)), int(rng.integers(1, n + 3)), float(_dyadic(rng, 1)[0])
        a[i, j] = v
        b[i, j] = v
    for x in (a, b):
        x.deletecolumn(int(J0[0]))
    Is, Js, Vs = rng.integers(1, m + 1, 300), rng.integers(1, n + 1, 300), _dyadic(rng, 300)
    keep = Js != int(J0[0])
    for x in (a, b):
        x.set_batch(Is[keep], Js[keep], Vs[keep])
    same()
    both(0)
    same()
    _clean(a)
