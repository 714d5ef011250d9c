"""In-place update of stored values and the batched read that stays in HBM (include/dsa.h: dsa_mat_update_values[_dev],
dsa_mat_get_batch_dev; csrc/update.hip).

Expected state never comes from the kernels: `model` is a Python dict over the two layouts exported BEFORE the call — (row, column) ->
slot per orientation, the ops applied one after the other — and gives the values of both slot arrays, the number of cells written and
the mask of the ops without a stored cell.  After the call keys, occupancy, semaphores, col_keys, col_live and the info() counters
must be byte-identical to the layout before, the values must be the model's bit for bit in EVERY slot, the checker must be clean and
to_csc / to_csr / get_batch must agree with a numpy walk over the new layout.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode, expected_compressed
from test_delete_batch import _bits, _clean, _owners

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
SIDES = (COLMAJOR, ROWMAJOR)
EARG, EMODE, EASSERT, EKEY = 1, 5, 6, 9
SET, ADD, SKIP = 0, 1, 1
NAMES = ("mat_update_values", "mat_update_values_dev", "mat_get_batch_dev")
METHODS = ("update_values", "add_values", "update_values_dev", "get_batch_dev")
FIELDS = ("keys", "occ", "semaphores", "col_keys", "col_live")

# ---- the constants of csrc/update.h
WAVE = 64                      # ops per wave of the locate kernel (one lane per op)
UPD_BLOCK = 256                # ops per workgroup
UPD_K_BITS = 32                # claim word = slot << 32 | k
PHI = 0x9E3779B97F4A7C15


def table_cap(n):
    c = 2
    while c < 2 * n:
        c <<= 1
    return c


def bucket(slot1, cap):
    """first bucket of the 1-based colmajor slot in a claim table of `cap` words"""
    return ((int(slot1) * PHI) & ((1 << 64) - 1)) >> (64 - (cap.bit_length() - 1))


N_EDGES = [0, 1, WAVE - 1, WAVE, WAVE + 1, UPD_BLOCK - 1, UPD_BLOCK, UPD_BLOCK + 1, 512, 513]      # 512 -> 1024 buckets, 513 -> 2048


# ---------------------------------------------------------------------------------------------------------------- model
def cell_slots(L, colmajor):
    """{(row, column): 0-based slot} of the cells of the live partitions of one orientation"""
    occ, is_sem, part = _owners(L)
    out = {}
    live = (L["col_live"] != 0) & (L["semaphores"] != 0)
    for s in np.nonzero(occ & ~is_sem & (part >= 1))[0].tolist():
        p = int(part[s]) - 1
        if not live[p]:
            continue
        key, pk = int(L["keys"][s]), int(L["col_keys"][p])
        out[(key, pk) if colmajor else (pk, key)] = s
    return out


class ModelError(Exception):
    def __init__(self, code, k):
        super().__init__(code, k)
        self.code, self.k = code, k


class Lookup:
    """the lookup of dsa_mat_get_batch on one exported layout, probe for probe (the reference's find, src/finds.jl:29-57, inside the
    partition's slot range): a cell is STORED iff this finds it.  On a partition whose keys ascend it is the dict of cell_slots; it is
    spelled out because a key below the semaphore's (matrix_simple_use_A stores A[i, -1]) sits in front of its row's semaphore, in the
    range of the row before, whose bisection it can mislead."""

    def __init__(self, L):
        self.keys, self.cap = L["keys"], L["info"]["capacity"]
        pos = np.where(L["occ"].astype(bool), np.arange(1, len(L["occ"]) + 1), 0)
        self.prev = np.concatenate([[0], np.maximum.accumulate(pos)]) if len(pos) else np.zeros(1, dtype=np.int64)
        sems = L["semaphores"]
        live = np.nonzero((L["col_live"] != 0))[0]
        self.part = {int(L["col_keys"][p]): p for p in live.tolist()}
        self.sems = sems
        nxt, self.end = 0, np.zeros(len(sems), dtype=np.int64)
        for p in range(len(sems) - 1, -1, -1):                # slot in front of the next live semaphore, or the capacity
            self.end[p] = nxt - 1 if nxt else self.cap
            if sems[p] != 0:
                nxt = int(sems[p])

    def _prev_occ(self, pos, lo):
        p = int(self.prev[pos]) if pos >= 1 else 0
        return p if p >= lo else lo - 1

    def slot(self, key, part):
        """1-based slot of (key, part), 0 if the lookup does not find it"""
        p = self.part.get(part)
        if p is None or self.sems[p] == 0:
            return 0
        lo, hi = int(self.sems[p]), int(self.end[p])
        frm, to = lo, hi
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
                    return i if lo < i <= hi else 0
        i = self._prev_occ(to, 1) if to >= 1 else 0           # the reference's fallback cell; it counts only inside the partition
        return i if i > 0 and int(self.keys[i - 1]) == key and lo < i <= hi else 0


def locate(before, I, J):
    """per orientation the 1-based slots of the ops, 0 where the lookup misses"""
    look = [Lookup(before[o]) for o in SIDES]
    I, J = np.asarray(I).reshape(-1).tolist(), np.asarray(J).reshape(-1).tolist()
    return [np.array([look[0].slot(i, j) for i, j in zip(I, J)], dtype=np.int64),
            np.array([look[1].slot(j, i) for i, j in zip(I, J)], dtype=np.int64)]


def model(before, I, J, V, op, skip):
    """the ops one after the other on the layouts `before`; raises ModelError(code, the op the call names) where it must fail"""
    I, J, V = (np.asarray(x).reshape(-1).tolist() for x in (I, J, np.asarray(V, dtype=np.float64)))
    for k, (i, j) in enumerate(zip(I, J)):
        if i == 0 or j == 0:
            raise ModelError(EKEY, k)
    slots = locate(before, I, J)
    stored = (slots[0] != 0).tolist()
    for k in range(len(I)):
        if stored[k] != bool(slots[1][k] != 0):
            raise ModelError(EASSERT, k)
    if not skip and not all(stored):
        raise ModelError(EARG, stored.index(False))
    last, losers = {}, []
    for k in range(len(I)):
        if stored[k]:
            s = int(slots[0][k])
            if s in last:
                losers.append(last[s])
            last[s] = k
    if op == ADD and losers:
        raise ModelError(EARG, min(losers))                   # the first op that a later one addresses again
    vals = [before[o]["vals"].copy() for o in SIDES]
    V = np.asarray(V, dtype=np.float64)                       # assigned element by element: the bits of V, NaN payloads included
    with np.errstate(invalid="ignore"):
        for k in last.values():
            for o in SIDES:
                s = int(slots[o][k]) - 1
                vals[o][s] = V[k] if op == SET else before[o]["vals"][s] + V[k]
    return dict(vals=vals, updated=len(last), missing=~np.array(stored, dtype=bool), slots=slots)


def _layouts(a):
    return [a.export_layout(o) for o in SIDES]


def _layout_bytes(a):
    return [tuple(L[f].tobytes() for f in ("keys", "vals", "occ", "semaphores", "col_keys", "col_live")) for L in _layouts(a)]


def _call(a, I, J, V, op, skip, how):
    """-> (updated, missing mask or None)"""
    I, J, V = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64), np.asarray(V, dtype=np.float64)
    name = "set" if op == SET else "add"
    if how in ("numpy", "list"):
        f = (lambda x: x) if how == "numpy" else (lambda x: x.tolist())
        if op == ADD and not skip:
            return a.add_values(f(I), f(J), f(V)), None
        r = a.update_values(f(I), f(J), f(V), op=name, missing="skip" if skip else "error")
        return r if skip else (r, None)
    import torch
    ti, tj, tv = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in (I, J, V))
    if how == "torch":
        r = a.update_values(ti, tj, tv, op=name, missing="skip" if skip else "error")
        return (r[0], r[1].cpu().numpy()) if skip else (r, None)
    mask = torch.full((max(len(I), 1),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    upd, mis = a.update_values_dev(ti.data_ptr(), tj.data_ptr(), tv.data_ptr(), len(I), op, SKIP if skip else 0,
                                   d_missing=mask.data_ptr() if skip else None)
    a.sync()
    got = mask.cpu().numpy()[:len(I)].astype(bool) if skip and len(I) else (np.zeros(0, dtype=bool) if skip else None)
    assert not skip or mis == int(got.sum())
    return upd, got


def _agree(dsa, a, after, I, J, exp):
    """to_csc / to_csr against a numpy walk over the new layouts, get_batch against the model's cells"""
    m, n = a.size()
    try:
        for o, export, dim in ((COLMAJOR, a.to_csc, n), (ROWMAJOR, a.to_csr, m)):
            if dim > 1 << 24:                                 # a pointer array per key of a wide dimension: 8 * 2^31 bytes
                continue
            got = export()
            e = expected_compressed(after[o], dim)
            assert np.array_equal(np.asarray(got[0], dtype=np.int64), e[0]) and np.array_equal(np.asarray(got[1], dtype=np.int64), e[1])
            assert np.array_equal(_bits(got[2]), _bits(e[2]))
    except dsa.DsaBoundsError:
        pass                                              # an entry outside size(m): no compressed form
    if len(I):
        got = a.get_batch(I, J)
        sc = exp["slots"][0]
        want = np.where(sc != 0, after[0]["vals"][np.maximum(sc, 1) - 1], 0.0)
        assert np.array_equal(_bits(got), _bits(want))


def apply_and_check(dsa, a, I, J, V, op=SET, skip=False, how="numpy", what=""):
    before = _layouts(a)
    info0 = [a.info(o) for o in SIDES]
    nnz0, size0 = a.nnz(), a.size()
    exp = model(before, I, J, V, op, skip)
    updated, missing = _call(a, I, J, V, op, skip, how)
    info1 = [a.info(o) for o in SIDES]
    after = _layouts(a)
    assert updated == exp["updated"], (what, updated, exp["updated"])
    if skip:
        assert np.array_equal(missing, exp["missing"]), what
    for o in SIDES:
        for f in FIELDS:
            assert after[o][f].tobytes() == before[o][f].tobytes(), (what, o, f)
        assert info1[o] == info0[o], (what, o)
        gb, eb = _bits(after[o]["vals"]), _bits(exp["vals"][o])
        # the sign and payload of a NaN that an ADD generates (Inf + -Inf) are not fixed by IEEE 754: NaN against NaN there
        same = (gb == eb) | (np.isnan(after[o]["vals"]) & np.isnan(exp["vals"][o]) if op == ADD else False)
        assert same.all(), (what, o, np.nonzero(~same)[0][:8])
    sc, sr = exp["slots"]
    hit = sc != 0                                             # both orientations hold identical bits in every addressed cell
    assert np.array_equal(_bits(after[0]["vals"][sc[hit] - 1]), _bits(after[1]["vals"][sr[hit] - 1])), what
    assert a.nnz() == nnz0 and a.size() == size0, what
    _clean(a)
    _agree(dsa, a, after, I, J, exp)
    return exp


def expect_error(dsa, a, I, J, V, op, skip, code, how="numpy"):
    """the call fails with `code`, names the model's op and leaves every byte where it was"""
    before = _layout_bytes(a)
    with pytest.raises(ModelError) as me:
        model(_layouts(a), I, J, V, op, skip)
    assert me.value.code == code
    with pytest.raises(dsa.DsaError) as ei:
        _call(a, I, J, V, op, skip, how)
    assert ei.value.code == code, ei.value
    assert "op %d " % me.value.k in str(ei.value), (me.value.k, str(ei.value))
    assert _layout_bytes(a) == before


def _distinct(rng, m, n, nnz):
    lin = rng.choice(m * n, size=nnz, replace=False)
    return lin // n + 1, lin % n + 1


def _random_matrix(dsa, b, seed=5, m=200, n=200, nnz=3000):
    rng = np.random.default_rng(seed)
    I, J = _distinct(rng, m, n, nnz)
    return dsa.dynamicsparse(I, J, rng.standard_normal(nnz), m, n, binding=b), rng


def _stored(a):
    """(I, J) of the stored cells with both keys >= 1, in colmajor slot order"""
    c = [ij for ij in cell_slots(a.export_layout(COLMAJOR), True) if ij[0] >= 1 and ij[1] >= 1]
    return np.array([x[0] for x in c], dtype=np.int64), np.array([x[1] for x in c], dtype=np.int64)


def probe_ops(a, rng, repeats=0.3):
    """every stored cell (both keys >= 1) — the first cell behind each semaphore, the last in front of the next, the last occupied
    slot, every one-cell partition — and misses of every kind: per live column a row below its first, above its last and in a gap;
    column and row keys below the first table entry, between entries and above the last; in random order with ~30 % repeats"""
    L = a.export_layout(COLMAJOR)
    have = cell_slots(L, True)
    I, J = _stored(a)
    ops = list(zip(I.tolist(), J.tolist()))
    cols = sorted({j for _, j in have})
    rows = sorted({i for i, _ in have})
    for j in cols:
        r = sorted(i for i, jj in have if jj == j)
        cand = [r[0] - 1, r[-1] + 1] + [x + 1 for x in r[:-1] if x + 1 not in r][:1]
        ops += [(i, j) for i in cand if i >= 1 and j >= 1]
    for keys, mk in ((cols, lambda k: (rows[0] if rows else 1, k)), (rows, lambda k: (k, cols[0] if cols else 1))):
        if keys:
            gaps = [k + 1 for k in keys[:-1] if k + 1 not in keys][:3]
            ops += [mk(k) for k in [keys[0] - 1, keys[-1] + 1, keys[-1] + 1000] + gaps if k >= 1]
    ops = [x for x in ops if x[0] >= 1 and x[1] >= 1]
    if not ops:
        ops = [(1, 1)]
    extra = [ops[t] for t in rng.integers(0, len(ops), int(len(ops) * repeats))]
    ops = ops + extra
    order = rng.permutation(len(ops))
    I = np.array([ops[t][0] for t in order], dtype=np.int64)
    J = np.array([ops[t][1] for t in order], dtype=np.int64)
    return I, J, rng.standard_normal(len(I))


def lookups(dsa, a, rng, what, hows=("numpy",)):
    """SET with skips over the probe ops, then ADD over the same ops made distinct"""
    I, J, V = probe_ops(a, rng)
    sc, sr = locate(_layouts(a), I, J)
    bad = (sc != 0) != (sr != 0)
    if bad.any():                                             # a cell the lookup finds in one orientation only (see Lookup)
        expect_error(dsa, a, I, J, V, SET, True, EASSERT)
        I, J, V = I[~bad], J[~bad], V[~bad]
    for how in hows:
        exp = apply_and_check(dsa, a, I, J, V, SET, True, how, what)
    _, first = np.unique(np.stack([I, J]), axis=1, return_index=True)
    first.sort()
    apply_and_check(dsa, a, I[first], J[first], V[first], ADD, True, hows[-1], what + " add")
    hit = ~exp["missing"]
    if hit.any():
        apply_and_check(dsa, a, I[hit], J[hit], V[hit] * 2.0, SET, False, hows[0], what + " strict")
    return exp


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_update_symbols_declared_bound_exported_and_in_julia(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    for const in ("DSA_UPD_SET = 0", "DSA_UPD_ADD = 1", "DSA_UPD_SKIP_MISSING = 1"):
        assert const in hdr, const
    assert (dsa.UPD_SET, dsa.UPD_ADD, dsa.UPD_SKIP_MISSING) == (0, 1, 1)
    for meth in METHODS:
        assert hasattr(dsa.DynamicSparseMatrix, meth), meth
    assert hasattr(dsa.Transposed, "update_values") and hasattr(dsa.Transposed, "add_values")
    jdir = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "julia")
    amd = open(os.path.join(jdir, "DynamicSparseArraysAMD.jl")).read()
    assert "ccall((:dsa_mat_update_values, libdsa)" in amd and "ccall((:dsa_mat_get_batch_dev, libdsa)" in amd
    for name in ("update_values!", "add_values!", "getstored"):
        assert re.search(r"^(?:function )?" + re.escape(name) + r"\(a::DynamicSparseMatrix", amd, flags=re.M), name
        assert re.search(r"\b" + re.escape(name) + r"(?:,|\s*$)", amd.split("const libdsa")[0], flags=re.M), name      # exported
    # the mirrored constants are the header's
    h = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "update.h")).read()
    assert "UPD_BLOCK = %d;" % UPD_BLOCK in h and "UPD_K_BITS = %d;" % UPD_K_BITS in h and "0x%X" % PHI in h
    assert [table_cap(n) for n in (0, 1, 2, 3, 512, 513)] == [2, 2, 4, 8, 1024, 2048]


def test_oracle_binding_has_no_update_values(dsa, oracle):
    for name in NAMES:
        assert not oracle.has(name), name
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    for call in (lambda: a.update_values([1], [1], [3.0]), lambda: a.add_values([1], [1], [3.0]),
                 lambda: a.update_values([1], [1], [3.0], op="add", missing="skip"), lambda: a.T.update_values([1], [1], [3.0]),
                 lambda: a.T.add_values([1], [1], [3.0]), lambda: a.update_values_dev(0, 0, 0, 0), lambda: a.get_batch_dev(0, 0, 0, 0)):
        with pytest.raises(dsa.DsaArgumentError) as ei:
            call()
        assert "need the HIP product library" in str(ei.value)
    assert a[1, 1] == 1.0 and a.nnz() == 2


def _oracle_triples(rng, I, J, k):
    t = rng.integers(0, len(I), k)
    return I[t], J[t], rng.integers(1, 1 << 20, k) * 2.0 ** -10 * rng.choice([-1.0, 1.0], k)       # nonzero


def test_oracle_set_batch_of_nonzero_values_onto_stored_cells_moves_no_slot(dsa, oracle):
    """the precondition of test_set_is_the_oracles_set_batch_slot_for_slot: such a set_batch only overwrites values, so the oracle's
    layout afterwards is the expectation of a SET; and the model gives exactly that layout"""
    b, rng = _random_matrix(dsa, oracle, seed=9)
    I, J = _stored(b)
    before = _layouts(b)
    info0 = [b.info(o) for o in SIDES]
    ti, tj, tv = _oracle_triples(rng, I, J, 2000)
    assert len(set(zip(ti.tolist(), tj.tolist()))) < 2000     # with repeats
    b.set_batch(ti, tj, tv)
    exp = model(before, ti, tj, tv, SET, False)
    for o, L in zip(SIDES, _layouts(b)):
        for f in FIELDS:
            assert L[f].tobytes() == before[o][f].tobytes(), (o, f)
        assert b.info(o) == info0[o]
        assert np.array_equal(_bits(L["vals"]), _bits(exp["vals"][o])), o


def test_model_orders_errors_and_duplicates(dsa, oracle):
    b = dsa.dynamicsparse([1, 2, 2], [1, 1, 3], [1.0, 2.0, 3.0], binding=oracle)
    L = _layouts(b)
    e = model(L, [2, 9, 2, 2], [1, 1, 1, 3], [5.0, 6.0, 7.0, -0.0], SET, True)
    assert e["updated"] == 2 and e["missing"].tolist() == [False, True, False, False]
    maps = [cell_slots(L[o], o == COLMAJOR) for o in SIDES]
    for o in SIDES:                                           # the spelled-out lookup is the dict of the cells
        assert e["slots"][o].tolist() == [maps[o][(2, 1)] + 1, 0, maps[o][(2, 1)] + 1, maps[o][(2, 3)] + 1]
        assert e["vals"][o][maps[o][(2, 1)]] == 7.0 and np.signbit(e["vals"][o][maps[o][(2, 3)]]) and e["vals"][o][maps[o][(1, 1)]] == 1.0
    for args, code, k in ((([2, 9], [1, 1], [1.0, 1.0], SET, False), EARG, 1), (([2, 0], [1, 1], [1.0, 1.0], SET, True), EKEY, 1),
                          (([2, 1, 2], [1, 1, 1], [1.0] * 3, ADD, False), EARG, 0), (([9, 9], [1, 1], [1.0] * 2, ADD, True), None, None)):
        if code is None:
            assert model(L, *args)["updated"] == 0
            continue
        with pytest.raises(ModelError) as me:
            model(L, *args)
        assert (me.value.code, me.value.k) == (code, k)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["numpy", "dev"])
def test_wave_workgroup_and_table_edges(dsa, hip, how):
    a, rng = _random_matrix(dsa, hip)
    I, J = _stored(a)
    for n in N_EDGES:
        t = rng.permutation(len(I))[:n]
        i, j, v = I[t].copy(), J[t].copy(), rng.standard_normal(n)
        if n >= 3:
            i[n // 2] = 201                                   # one miss in the middle, one at the end
            j[n - 1] = 5000
        exp = apply_and_check(dsa, a, i, j, v, SET, True, how, "n=%d" % n)
        assert exp["updated"] == n - (2 if n >= 3 else 0)
        if n:
            apply_and_check(dsa, a, i, j, v, ADD, True, how, "add n=%d" % n)


@pytest.mark.gpu
def test_claim_table_collisions_and_wrap(dsa, hip):
    """ops whose colmajor slots share one first bucket (a probe chain as long as the op list), and ops that start in the last
    bucket so that the probes wrap to bucket 0 — built from the hash of csrc/update.h over the exported layout"""
    a, rng = _random_matrix(dsa, hip)
    slots = cell_slots(a.export_layout(COLMAJOR), True)
    for n, which in ((8, "chain"), (8, "wrap"), (24, "wrap"), (24, "chain")):
        cap = table_cap(n)
        by = {}
        for ij, s in slots.items():
            by.setdefault(bucket(s + 1, cap), []).append(ij)
        if which == "chain":
            b0 = max(by, key=lambda k: len(by[k]))
            pick = by[b0][:n]
        else:
            pick = by[cap - 1][:n // 2] + by[cap - 2][:n - n // 2]
            assert len(by[cap - 1]) >= 2
        assert len(pick) == n, (n, which)                     # 3000 cells over <= 64 buckets: every bucket holds enough
        if which == "chain":
            assert len({bucket(slots[ij] + 1, cap) for ij in pick}) == 1
        i = np.array([x[0] for x in pick], dtype=np.int64)
        j = np.array([x[1] for x in pick], dtype=np.int64)
        apply_and_check(dsa, a, i, j, rng.standard_normal(n), SET, False, "numpy", which)
        # the same slots addressed twice each, in another order, inside the same table size
        h = n // 2
        i2, j2 = np.concatenate([i[:h], i[:h][::-1]]), np.concatenate([j[:h], j[:h][::-1]])
        assert table_cap(len(i2)) == cap
        apply_and_check(dsa, a, i2, j2, rng.standard_normal(len(i2)), SET, False, "dev", which + " twice")


@pytest.mark.gpu
def test_duplicates_last_wins_across_waves_and_workgroups(dsa, hip):
    out = []
    for _ in range(2):
        a, rng = _random_matrix(dsa, hip)
        I, J = _stored(a)
        n = 3 * UPD_BLOCK
        i, j, v = I[:n].copy(), J[:n].copy(), rng.standard_normal(n)
        where = [3, WAVE + 6, 2 * UPD_BLOCK + 44]             # first wave, second wave, third workgroup
        for k in where:
            i[k], j[k] = I[n], J[n]
        exp = apply_and_check(dsa, a, i, j, v, SET, False, "dev", "duplicates")
        assert exp["updated"] == n - 2
        assert a[int(I[n]), int(J[n])] == v[where[-1]]
        # and with the winner in the FIRST wave of the list's first workgroup being overtaken by a later workgroup only
        apply_and_check(dsa, a, i[::-1].copy(), j[::-1].copy(), v, SET, False, "numpy", "duplicates reversed")
        out.append(_layout_bytes(a))
    assert out[0] == out[1]                                   # the same input gives the same bits
    # ADD: a repeated stored cell is an error, a repeated miss is not
    expect_error(dsa, a, i, j, v, ADD, False, EARG)
    expect_error(dsa, a, i, j, v, ADD, True, EARG, how="dev")
    i2, j2 = I[:n].copy(), J[:n].copy()
    i2[where], j2[where] = 777, 5                             # the same absent cell three times
    exp = apply_and_check(dsa, a, i2, j2, v, ADD, True, "dev", "repeated miss")
    assert exp["missing"].sum() == 3 and exp["updated"] == n - 3
    expect_error(dsa, a, i2, j2, v, ADD, False, EARG)         # strict: the miss


def _edges_matrix(dsa, b):
    """column 1: one cell; column 2: 150 cells (crosses 64-slot words); columns 5, 9: a few; column 40: the last, one cell"""
    I = [7] + list(range(3, 303, 2)) + [1, 2, 300] + [5, 6] + [300]
    J = [1] + [2] * 150 + [5, 5, 5] + [9, 9] + [40]
    return dsa.dynamicsparse(I, J, np.arange(1, len(I) + 1) * 0.5, 300, 40, binding=b)


@pytest.mark.gpu
def test_lookup_edges_on_a_crafted_matrix(dsa, hip):
    a = _edges_matrix(dsa, hip)
    L = a.export_layout(COLMAJOR)
    occ, is_sem, part = _owners(L)
    s2 = np.nonzero(occ & ~is_sem & (part == 2))[0]
    assert len(s2) == 150 and s2[0] // 64 != s2[-1] // 64     # a partition that crosses a bitmap word
    assert (part[occ & ~is_sem] == 1).sum() == 1              # a one-cell partition
    last = np.nonzero(occ)[0][-1]
    assert not is_sem[last] and L["keys"][last] == 300        # the last occupied slot is a cell
    exp = lookups(dsa, a, np.random.default_rng(3), "crafted", hows=("numpy", "torch", "dev"))
    assert exp["missing"].any() and (~exp["missing"]).sum() >= 157


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_lookups_on_the_golden_scenarios(dsa, hip, sc):
    a = run_scenario(dsa, hip, sc)
    if _in_fill_mode(dsa, a):
        with pytest.raises(dsa.DsaError) as ei:
            a.update_values([1], [1], [1.0])
        assert ei.value.code == EMODE
        return
    lookups(dsa, a, np.random.default_rng(11), sc["name"])


@pytest.mark.gpu
def test_random_matrix_5000_ops(dsa, hip):
    a, rng = _random_matrix(dsa, hip, seed=21)
    I, J = _stored(a)
    t = rng.integers(0, len(I), 5000)
    t[3500:] = t[rng.integers(0, 3500, 1500)]                 # 30 % repeats of earlier ops
    i, j = I[t].copy(), J[t].copy()
    miss = rng.random(5000) < 0.2
    j[miss] = rng.integers(201, 260, int(miss.sum()))         # columns that do not exist
    i[miss & (rng.random(5000) < 0.5)] += 200                 # ... and rows that do not
    exp = None
    for how in ("numpy", "torch", "dev"):
        exp = apply_and_check(dsa, a, i, j, rng.standard_normal(5000), SET, True, how, "random " + how)
    assert 700 < exp["missing"].sum() < 1300 and exp["updated"] < (~exp["missing"]).sum()
    lookups(dsa, a, rng, "random probes")
    # the transpose addresses the same cells with the sides swapped
    before = _layouts(a)
    v = rng.standard_normal(5000)
    e = model(before, i, j, v, SET, True)
    got = a.T.update_values(j, i, v, missing="skip")
    assert got[0] == e["updated"] and np.array_equal(got[1], e["missing"])
    for o, L in zip(SIDES, _layouts(a)):
        assert np.array_equal(_bits(L["vals"]), _bits(e["vals"][o]))


@pytest.mark.gpu
def test_states_after_deletes_droptol_extension_and_a_queued_write(dsa, hip):
    a, rng = _random_matrix(dsa, hip, seed=8)
    I0, J0 = _stored(a)
    # tombstones: a deleted key misses, a key behind tombstones hits
    a.delete_columns([3, 4, 5, 120])
    a.delete_rows([1, 2, 77])
    assert a.info(COLMAJOR)["nb_partitions"] < a.info(COLMAJOR)["table_len"]
    exp = apply_and_check(dsa, a, I0, J0, rng.standard_normal(len(I0)), SET, True, "dev", "after deletes")
    gone = np.isin(J0, [3, 4, 5, 120]) | np.isin(I0, [1, 2, 77])
    assert np.array_equal(exp["missing"], gone) and gone.any() and (~gone & (J0 > 120)).any()
    lookups(dsa, a, rng, "after deletes")
    # an empty live partition: every cell of column 10 dropped, the column stays
    i10 = I0[(J0 == 10) & ~gone]
    a.update_values(i10, np.full(len(i10), 10), np.zeros(len(i10)))
    nb = a.nbpartitions(COLMAJOR)
    assert a.dropzeros() == len(i10) > 0 and a.nbpartitions(COLMAJOR) == nb
    exp = apply_and_check(dsa, a, I0, J0, rng.standard_normal(len(I0)), SET, True, "numpy", "after droptol")
    assert exp["missing"][J0 == 10].all()
    _clean(a)
    # a set_batch that extended the array (on a matrix without tombstones: the reference's write asserts behind one)
    a, rng = _random_matrix(dsa, hip, seed=8)
    cap0 = a.info(COLMAJOR)["capacity"]
    I2, J2 = _distinct(rng, 400, 400, 6000)
    a.set_batch(I2, J2, rng.standard_normal(6000))
    assert a.info(COLMAJOR)["capacity"] > cap0
    lookups(dsa, a, rng, "after extension", hows=("dev",))
    # a queued single write is applied first: the update lands on the new cell
    a[399, 7] = 4.5
    assert a.update_values([399], [7], [-1.25]) == 1
    assert a[399, 7] == -1.25
    a[398, 9] = 2.0
    assert a.add_values([398], [9], [0.5]) == 1 and a[398, 9] == 2.5
    _clean(a)


@pytest.mark.gpu
def test_wide_keys_take_the_64_bit_key_path(dsa, hip):
    big = (1 << 31) + 5
    I = np.array([1, 2, 3, 3, 4], dtype=np.int64)
    J = np.array([1, 7, 2, big, big], dtype=np.int64)
    a = dsa.dynamicsparse(I, J, np.array([1.5, -2.0, 3.25, 4.0, 0.125]), binding=hip)
    i = np.array([3, 4, 2, 3, 4, 1, 3], dtype=np.int64)
    j = np.array([big, big, big, 2, big - 1, 1, big], dtype=np.int64)
    for how in ("numpy", "dev"):
        exp = apply_and_check(dsa, a, i, j, np.arange(7) + 0.5, SET, True, how, "wide " + how)
        assert exp["missing"].tolist() == [False, False, True, False, True, False, False] and exp["updated"] == 4
    apply_and_check(dsa, a, i[[1, 3, 6]], j[[1, 3, 6]], [1.0, 2.0, 3.0], ADD, False, "dev", "wide add")
    # wide ROW keys: the 64-bit path of the colmajor slot array
    b = dsa.dynamicsparse(J, I, np.array([1.5, -2.0, 3.25, 4.0, 0.125]), binding=hip)
    apply_and_check(dsa, b, j, i, np.arange(7) + 0.5, SET, True, "dev", "wide rows")


@pytest.mark.gpu
def test_values_by_bits(dsa, hip):
    a, rng = _random_matrix(dsa, hip)
    I, J = _stored(a)
    special = np.array([0x7FF8DEADBEEF0001, 0xFFF0000000000000, 0x7FF0000000000000, 0x8000000000000000, 0x7FF0000000000001,
                        0xFFFFFFFFFFFFFFFF, 0x0000000000000001], dtype=np.uint64).view(np.float64)
    n = len(special)
    for how in ("numpy", "dev"):
        apply_and_check(dsa, a, I[:n], J[:n], special, SET, False, how, "special " + how)
        L = a.export_layout(COLMAJOR)
        m = cell_slots(L, True)
        got = np.array([L["vals"][m[(i, j)]] for i, j in zip(I[:n].tolist(), J[:n].tolist())])
        assert np.array_equal(_bits(got), _bits(special))     # NaN payloads, +-Inf, -0.0, a denormal: the bits of V
    # ADD: +0.0 + -0.0 = +0.0, Inf + -Inf = NaN, -0.0 + -0.0 = -0.0
    base = np.array([0.0, np.inf, -0.0, 1.0])
    add = np.array([-0.0, -np.inf, -0.0, 2.0 ** -60])
    apply_and_check(dsa, a, I[10:14], J[10:14], base, SET, False, "numpy", "base")
    apply_and_check(dsa, a, I[10:14], J[10:14], add, ADD, False, "dev", "ieee add")
    got = a.get_batch(I[10:14], J[10:14])
    assert _bits(got[:1])[0] == 0 and np.isnan(got[1]) and np.signbit(got[2]) and got[2] == 0.0 and got[3] == 1.0 + 2.0 ** -60
    # SET of 0.0 keeps nnz, and the cell is still exported
    nnz0 = a.nnz()
    assert a.update_values(I[20:25], J[20:25], np.zeros(5)) == 5
    assert a.nnz() == nnz0
    ri, ci, vi = a.findnz()
    at = {(int(r), int(c)): v for r, c, v in zip(ri, ci, vi)}
    assert all(at[(int(i), int(j))] == 0.0 for i, j in zip(I[20:25], J[20:25]))
    zeros = int((vi == 0.0).sum())                            # these five, the -0.0 of the SET and the two zero sums of the ADD
    assert zeros == 8 and a.dropzeros() == zeros and a.nnz() == nnz0 - zeros      # ... until dropzeros


@pytest.mark.gpu
def test_set_is_the_oracles_set_batch_slot_for_slot(dsa, hip, oracle):
    a, rng = _random_matrix(dsa, hip, seed=9)
    b, _ = _random_matrix(dsa, oracle, seed=9)
    I, J = _stored(b)
    ti, tj, tv = _oracle_triples(rng, I, J, 2000)
    assert a.update_values(ti, tj, tv) == len(set(zip(ti.tolist(), tj.tolist())))
    b.set_batch(ti, tj, tv)
    for o in SIDES:
        La, Lb = a.export_layout(o), b.export_layout(o)
        for f in FIELDS:
            assert La[f].tobytes() == Lb[f].tobytes(), (o, f)
        assert np.array_equal(_bits(La["vals"]), _bits(Lb["vals"])), o


def _plan_matrix(dsa, hip, seed):
    """the shape of tests/test_spmv_plan.py: the smallest at which the plan applies (as in tests/test_droptol.py)"""
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
    return a, x, y0, stats, (int(I[0]), int(J[0]))


@pytest.mark.gpu
def test_errors_and_no_ops_keep_bytes_and_plan_and_one_write_rebuilds_it_once(dsa, hip):
    import torch
    a, x, y0, stats, (ci, cj) = _plan_matrix(dsa, hip, 151)
    p0, b0 = stats()
    before = _layout_bytes(a)
    P_I64, P_F64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    one_i, one_f = np.array([ci], dtype=np.int64), np.array([1.0])
    d = torch.ones(4, dtype=torch.int64, device="cuda")
    dv = torch.ones(4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    upd, mis = C.c_int64(-1), C.c_int64(-1)
    raw = lambda *args: hip._mat_update_values_dev(a.h, *args, C.byref(upd), C.byref(mis))
    vp = lambda t: C.c_void_p(t.data_ptr())
    failing = [
        (lambda: a.update_values([ci, 420_001], [cj, 1], [1.0, 2.0]), EARG),                     # a strict miss
        (lambda: a.update_values([ci, 0], [cj, 1], [1.0, 2.0], missing="skip"), EKEY),           # a zero key, in both forms
        (lambda: a.update_values([ci, 5], [cj, 0], [1.0, 2.0]), EKEY),
        (lambda: a.add_values([ci, ci], [cj, cj], [1.0, 2.0], missing="skip"), EARG),            # ADD onto one cell twice
    ]
    for call, code in failing:
        with pytest.raises(dsa.DsaError) as ei:
            call()
        assert ei.value.code == code, ei.value
    assert "op 1 " in str(ei.value) or "op 0 " in str(ei.value)
    for args, code in (((SET, 0, vp(d), vp(d), vp(dv), -1, None), EARG), ((SET, 0, None, vp(d), vp(dv), 4, None), EARG),
                       ((SET, 0, vp(d), vp(d), None, 4, None), EARG), ((2, 0, vp(d), vp(d), vp(dv), 4, None), EARG),
                       ((ADD, 2, vp(d), vp(d), vp(dv), 4, None), EARG), ((SET, 4, vp(d), vp(d), vp(dv), 4, None), EARG)):
        assert raw(*args) == code, args
    assert hip._mat_update_values(a.h, SET, 0, None, one_i.ctypes.data_as(P_I64), one_f.ctypes.data_as(P_F64), 1, None,
                                  C.byref(upd), C.byref(mis)) == EARG
    assert hip._mat_get_batch_dev(a.h, vp(d), vp(d), -1, vp(dv), None) == EARG
    assert hip._mat_get_batch_dev(a.h, vp(d), vp(d), 4, None, None) == EARG
    f = dsa.dynamicsparse(binding=hip)                        # fill mode
    f[1, 1] = 2.0
    assert hip._mat_update_values_dev(f.h, SET, 0, vp(d), vp(d), vp(dv), 4, None, C.byref(upd), C.byref(mis)) == EMODE
    assert hip._mat_update_values(f.h, SET, SKIP, one_i.ctypes.data_as(P_I64), one_i.ctypes.data_as(P_I64),
                                  one_f.ctypes.data_as(P_F64), 1, None, C.byref(upd), C.byref(mis)) == EMODE
    assert hip._mat_get_batch_dev(f.h, vp(d), vp(d), 4, vp(dv), None) == EMODE
    # n = 0 and a skip-mode call whose ops all miss: nothing is written
    assert a.update_values([], [], []) == 0
    assert raw(SET, 0, None, None, None, 0, None) == 0 and (upd.value, mis.value) == (0, 0)
    got = a.update_values([420_001, ci], [1, 420_002], [1.0, 2.0], missing="skip")
    assert got[0] == 0 and got[1].tolist() == [True, True]
    got = a.add_values([420_001, 420_001], [1, 1], [1.0, 2.0], missing="skip")
    assert got[0] == 0
    assert _layout_bytes(a) == before and stats() == (p0, b0)
    assert a.mul(x).tobytes() == y0.tobytes()
    assert stats() == (p0 + 1, b0)                            # still the plan it had
    # one cell written: the plan is rebuilt exactly once, and the product is that of a freshly built matrix
    assert a.update_values([ci], [cj], [-3.5]) == 1
    zs = [a.mul(x).copy() for _ in range(3)]
    assert stats()[1] == b0 + 1
    ptr, idx, val = a.to_csr()
    M = len(ptr) - 1
    fresh = dsa.dynamicsparse(np.repeat(np.arange(1, M + 1), np.diff(ptr)), idx + 1, val, M, len(x), binding=hip)
    w = fresh.mul(x)
    for z in zs:
        assert z.tobytes() == w.tobytes()
    assert zs[0].tobytes() != y0.tobytes()
    _clean(a)


@pytest.mark.gpu
def test_get_batch_dev_is_get_batch(dsa, hip):
    import torch
    a, rng = _random_matrix(dsa, hip, seed=4)
    I, J = _stored(a)
    a.delete_columns([9])
    a.update_values(I[J == 20], J[J == 20], np.zeros(int((J == 20).sum())))          # stored zeros
    i11 = I[J == 11]
    a.set_batch(i11, np.full(len(i11), 11), np.zeros(len(i11)))                      # deleted by the write planner: column 11 is empty and live
    have = cell_slots(a.export_layout(COLMAJOR), True)
    for n in N_EDGES:
        t = rng.integers(0, len(I), n)
        i, j = I[t].copy(), J[t].copy()
        if n >= 8:
            i[0], j[0] = I[J == 20][0], 20                    # a stored zero
            i[1], j[1] = I[J == 9][0], 9                      # a tombstoned column
            i[2], j[2] = i11[0], 11                           # an empty live column
            i[3], j[3] = 201, j[3]                            # a present column, an absent row
            i[4], j[4] = i[4], 999                            # above the last column
            i[5], j[5] = i[5], 9                              # the tombstone again, another row
        ti, tj = torch.from_numpy(i).to("cuda"), torch.from_numpy(j).to("cuda")
        out = torch.full((max(n, 1),), 7.0, dtype=torch.float64, device="cuda")
        found = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
        out2 = out.clone()
        torch.cuda.synchronize()
        a.get_batch_dev(ti.data_ptr(), tj.data_ptr(), n, out.data_ptr(), found.data_ptr())
        a.get_batch_dev(ti.data_ptr(), tj.data_ptr(), n, out2.data_ptr())           # found is optional
        a.sync()
        want = a.get_batch(i, j)
        assert np.array_equal(_bits(out.cpu().numpy()[:n]), _bits(want)), n
        assert np.array_equal(_bits(out2.cpu().numpy()[:n]), _bits(want)), n
        stored = np.array([(x, y) in have for x, y in zip(i.tolist(), j.tolist())], dtype=bool)
        assert np.array_equal(found.cpu().numpy()[:n].astype(bool), stored), n
        if n >= 8:
            assert stored[0] and want[0] == 0.0 and not stored[1:6].any()
        if n == 0:
            assert float(out[0]) == 7.0 and int(found[0]) == 7
