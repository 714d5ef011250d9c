"""The read paths at their edges: the device-side invariant checker (csrc/read.hip: k_check_slots, k_check_table; pma_host.hip:
pma_check), the one-launch view k_view_small with its host side (view_small, read_range, view_dev, pack_small), the general K-pack
(csrc/rebalance.hip: k_tile_count, k_tile_scan, k_compact) and the lookups k_get_small / k_get_batch.  Every comparison is exact:
keys with array_equal, values bit for bit, counts equal — values are copied, never computed.

1. `reference_check` restates report words 0-5 of the checker in numpy.  On the CPU it is run on layouts the oracle built (words 2-5
   zero) and on tiny literal arrays with hand-counted answers; on the GPU layouts with PLANTED violations go into the HIP library
   through dsa_vec_import_layout / dsa_pcsc_import_layout (which do not validate key order) and check()[0:6] must equal
   reference_check word for word.  The expected numbers come from reference_check and from counting by hand, never from the device.
   report[4] (a table entry that does not point back) and report[5] (occupancy bits beyond the capacity) stay UNREACHED: the import
   rejects such a table with DSA_EARG (asserted here) and builds the occupancy words from exactly `capacity` bytes.
   report[6] compares report[0] with nb_elements and report[1] with the live table entries.  The import takes nb_elements from the
   occupancy bytes and the live count from the non-zero table entries, so report[6] is 0 on every plant but the two with a stray
   semaphore cell: that cell is one semaphore cell more than the table has live entries, report[6] must be 1 there.
2. k_view_small through nonzeros() of imported vectors, where the range is [1, capacity] and so exact: 65536 slots is exactly
   VIEW_SMALL_SLOTS (1024 words, one per thread), 131072 the first general K-pack; the 512 cells that travel through pinned memory
   against the rest fetched by a copy (counts 511 / 512 / 513); first and last word, first and last slot; narrow and wide keys.
   A range of 65536 slots that starts inside a word (1025 words, two per thread) needs a partition of exactly that span and is not
   reachable through a vector.  filter / == / + run pack_small and both branches of read_range at the same counts.
3. The general K-pack at the edges of its 4096-slot tiles and 16-tile count workgroups: 2^17, 2^18, 2^20 slots are 32, 64, 256 tiles,
   2, 4, 16 count workgroups.  The next edge of k_tile_scan, a second round beyond 4096 tiles, needs 2^24 slots and is out of scope.
4. Matrix views, device views and slices of partitions on both sides of 65536 slots (asserted on the oracle's layout), of 511 / 512 /
   513 cells, of an absent key and of a deleted column.
5. Lookups of 1, 63, 64, 65 and 129 queries: k_get_small up to 64, k_get_batch above; the error word and sequence number of the pinned
   landing area after a failed call."""
import numpy as np
import pytest

from rawhooks import to_arrays
from test_hip_parity import assert_vec_equal
from util import layouts_equal

COLMAJOR, ROWMAJOR = 0, 1
W40 = 1 << 40
SEG = 16


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


# ================================================================== 1. the checker
def reference_check(keys, vals, occ, sems=None, table_len=0):
    """report[0..5] of the device checker (csrc/read.hip, above k_check_slots) for the slot array keys / vals / occ of len(keys) slots
    (occ may be longer: the bits past the capacity) and, for a partitioned array, the semaphore table sems[:table_len].
    [0] occupied cells, [1] semaphore cells (key 0), [2] semaphore cells whose table entry does not point back at them, [3] key-order
    violations: an occupied non-semaphore cell whose previous occupied cell is not a semaphore cell and holds a key that is not
    smaller (equal keys are a violation; the cell right behind a semaphore cell is exempt; a semaphore cell is not compared with the
    cell in front of it, so order is not compared across a semaphore), [4] non-zero table entries that do not point at an occupied
    cell (0, id), [5] occupancy bits at or beyond the capacity.  A plain vector (sems None) has no semaphore cells: key 0 is a key."""
    keys = np.asarray(keys, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    cap = len(keys)
    o = np.asarray(occ).astype(bool)
    inside = o[:cap]
    pos = np.flatnonzero(inside)
    k = keys[pos]
    r = np.zeros(6, dtype=np.int64)
    r[0] = len(pos)
    r[5] = int(o[cap:].sum())
    if sems is None:
        r[3] = int((k[:-1] >= k[1:]).sum())
        return r
    table = np.asarray(sems, dtype=np.int64)[:table_len]
    is_sem = k == 0
    r[1] = int(is_sem.sum())
    ids = np.trunc(vals[pos][is_sem]).astype(np.int64)
    at = pos[is_sem] + 1
    known = (ids >= 1) & (ids <= table_len)
    back = np.zeros(len(ids), dtype=bool)
    back[known] = table[ids[known] - 1] == at[known]
    r[2] = int((~back).sum())
    r[3] = int((~is_sem[1:] & ~is_sem[:-1] & (k[:-1] >= k[1:])).sum())
    for i, p in enumerate(table.tolist()):
        if p != 0 and not (1 <= p <= cap and inside[p - 1] and keys[p - 1] == 0 and vals[p - 1] == float(i + 1)):
            r[4] += 1
    return r


def counts_disagree(ref, sems=None):
    """report[6] of an IMPORTED layout: nb_elements is the number of occupancy bytes set, the live partitions are the non-zero table
    entries"""
    live = 0 if sems is None else int(np.count_nonzero(sems))
    return int(ref[1] != live)


def ascending(occ, step=10):
    """keys step, 2 step, ... and distinct values in the occupied slots"""
    o = np.asarray(occ).astype(np.uint8)
    m = o.astype(bool)
    n = int(m.sum())
    k = np.zeros(len(o), dtype=np.int64)
    v = np.zeros(len(o), dtype=np.float64)
    k[m] = np.arange(1, n + 1, dtype=np.int64) * step
    v[m] = np.arange(1, n + 1) + 0.25
    return k, v, o


def widen(k, o):
    """the largest stored key moves beyond 2^40: the array is stored with 64-bit keys, the order of the keys is unchanged"""
    m = np.asarray(o).astype(bool)
    p = np.flatnonzero(m)[np.argmax(k[m])]
    k[p] += W40


VECTOR_PLANTS = ("clean", "in_word", "word_edge", "gap", "ends", "duplicate", "run130")
VECTOR_CAPS = (4096, 1 << 18)


def vector_plant(name, cap, wide):
    """(keys, vals, occ, violations counted by hand).  The slots the plant needs are occupied (or emptied) before the ascending keys
    are handed out, then the keys of the plant are exchanged."""
    rng = np.random.default_rng(cap)
    occ = rng.random(cap) < 0.5
    occ[-1] = True
    # the empty stretch behind the last slot of a word: 5000 slots where the array has them, 3000 in the 4096-slot array
    gap = 5000 if cap > 8192 else 3000
    a = b = None
    if name == "in_word":
        a, b = 64 * 7 + 20, 64 * 7 + 21
    elif name == "word_edge":
        a, b = 63, 64
    elif name == "gap":
        a = 64 * 2 + 63
        b = a + gap
        occ[a:b + 1] = False
    elif name == "ends":
        a, b = 0, cap - 1
        occ[:] = False
    elif name == "duplicate":
        a, b = 64 * 9 + 5, 64 * 9 + 6
    elif name == "run130":
        a = 256 * 3 + 60                       # slots 828 .. 957: three waves of the fourth 256-slot workgroup
        b = a + 130
        occ[a:b] = True
    if name in ("in_word", "word_edge", "gap", "ends", "duplicate"):
        occ[a] = occ[b] = True
    k, v, o = ascending(occ)
    want = 0
    if name in ("in_word", "word_edge", "gap", "ends"):
        k[a], k[b] = k[b], k[a]
        want = 1
    elif name == "duplicate":
        k[b] = k[a]
        want = 1
    elif name == "run130":
        k[a:b] = k[a:b][::-1].copy()
        want = 129
    if wide:
        widen(k, o)
    return k, v, o, want


BASE_PARTS = [[5, 9, 14, 20, 33, 47, 58, 60],          # id 1
              [-7, 3, 9, 12],                          # id 2: a negative key right behind the semaphore (0 is not smaller than it)
              [20, 40, 60, 80, 100],                   # id 3
              [],                                      # id 4: an empty partition
              None,                                    # id 5: a deleted partition (table entry 0, no cell)
              [100, 200, 300, 400, 500, 600, 700],     # id 6
              [1, 2, 3] + list(range(10, 40))]         # id 7
PCSC_CAP = 512
PCSC_PLANTS = ("clean", "mid_inversion", "across_semaphore", "behind_semaphore", "second_semaphore", "unknown_semaphore")


def pcsc_layout(parts, cap, seed, wide=False):
    """PackedCSC slot array of the partitions `parts` (key lists; None: deleted) at random ascending slots.  Returns keys, vals, occ,
    sems and where[(id, j)] = 0-based slot of the j-th cell of partition id (j = -1: its semaphore cell)."""
    cells = []
    for pid, ks in enumerate(parts, start=1):
        if ks is None:
            continue
        cells.append((pid, -1, 0, float(pid)))
        cells += [(pid, j, key, 1000.0 * pid + j + 0.5) for j, key in enumerate(ks)]
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(cap, size=len(cells), replace=False))
    k = np.zeros(cap, dtype=np.int64)
    v = np.zeros(cap, dtype=np.float64)
    o = np.zeros(cap, dtype=np.uint8)
    sems = np.zeros(len(parts), dtype=np.int64)
    where = {}
    for s, (pid, j, key, val) in zip(pos.tolist(), cells):
        k[s], v[s], o[s] = key, val, 1
        where[(pid, j)] = s
        if j < 0:
            sems[pid - 1] = s + 1
    if wide:
        k[where[(6, 6)]] += W40
    return k, v, o, sems, where


def pcsc_plant(name, wide=False):
    """(keys, vals, occ, sems, (bad semaphore cells, order violations) counted by hand)"""
    k, v, o, sems, at = pcsc_layout(BASE_PARTS, PCSC_CAP, 3, wide)
    want = (0, 0)
    if name == "mid_inversion":
        a, b = at[(1, 3)], at[(1, 4)]
        k[a], k[b] = k[b], k[a]
        want = (0, 1)
    elif name == "across_semaphore":            # 900 | semaphore of 3 | 2: descending, not compared
        k[at[(2, 3)]] = 900
        k[at[(3, 0)]] = 2
    elif name == "behind_semaphore":            # semaphore of 3 | 50 | 40: the second cell of the pair is compared
        k[at[(3, 0)]] = 50
        want = (0, 1)
    elif name == "second_semaphore":            # a second cell (0, 2): the table entry of 2 points at the first
        s = at[(7, 5)]
        k[s], v[s] = 0, 2.0
        want = (1, 0)
    elif name == "unknown_semaphore":           # a cell (0, id) behind the end of the table
        s = at[(7, 5)]
        k[s], v[s] = 0, float(len(sems) + 1)
        want = (1, 0)
    return k, v, o, sems, want


# ------------------------------------------------------------------ CPU: the reference checker alone
def test_reference_check_on_literal_arrays():
    N = None
    k, v, o = to_arrays([[1, 1.0], N, [3, 1.0], [2, 1.0], N, [2, 1.0], [9, 1.0], N])
    assert reference_check(k, v, o).tolist() == [5, 0, 0, 2, 0, 0]                # 3 > 2 and 2 == 2
    k, v, o = to_arrays([[0, 1.0], [7, 1.0], N, [0, 1.0]])
    assert reference_check(k, v, o).tolist() == [3, 0, 0, 1, 0, 0]                # a plain vector: 0 is a key like any other
    # semaphore of 1 | 5 3 (violation) | semaphore of 2 | 1 (exempt: behind the semaphore) 7 7 (violation) | a cell (0, 3) the table has no entry for
    slots = [[0, 1.0], [5, 1.0], [3, 1.0], N, [0, 2.0], [1, 1.0], [7, 1.0], [7, 2.0], [0, 3.0], N]
    k, v, o = to_arrays(slots)
    assert reference_check(k, v, o, np.array([1, 5, 0]), 3).tolist() == [8, 3, 1, 2, 0, 0]
    # the table entry of 2 points at the cell (1, 1.0): the entry is bad, and the semaphore cell of 2 is not pointed back at
    assert reference_check(k, v, o, np.array([1, 6, 0]), 3).tolist() == [8, 3, 2, 2, 1, 0]
    # a table of two entries: the cell (0, 3) is behind its end all the same
    assert reference_check(k, v, o, np.array([1, 5, 0]), 2).tolist() == [8, 3, 1, 2, 0, 0]
    # descending across a semaphore: not compared; descending right behind it: compared; a negative key right behind it: in order
    k, v, o = to_arrays([[0, 1.0], [50, 1.0], [0, 2.0], [10, 1.0]])
    assert reference_check(k, v, o, np.array([1, 3]), 2).tolist() == [4, 2, 0, 0, 0, 0]
    k, v, o = to_arrays([[0, 1.0], [50, 1.0], [10, 1.0]])
    assert reference_check(k, v, o, np.array([1]), 1).tolist() == [3, 1, 0, 1, 0, 0]
    k, v, o = to_arrays([[0, 1.0], N, [-7, 1.0], [3, 1.0]])
    assert reference_check(k, v, o, np.array([1]), 1).tolist() == [3, 1, 0, 0, 0, 0]
    # occupancy longer than the slot array: the bits behind the capacity
    k, v, o = to_arrays([[1, 1.0], [2, 1.0]])
    assert reference_check(k, v, np.array([1, 1, 0, 1, 1], dtype=np.uint8)).tolist() == [2, 0, 0, 0, 0, 2]


def test_reference_check_counts_the_plants_as_counted_by_hand():
    """the planted layouts of the GPU tests: reference_check sees exactly the violations the plant was built to hold"""
    for cap in VECTOR_CAPS:
        for wide in (False, True):
            for name in VECTOR_PLANTS:
                k, v, o, want = vector_plant(name, cap, wide)
                ref = reference_check(k, v, o)
                assert ref.tolist() == [int(o.sum()), 0, 0, want, 0, 0], (name, cap, wide)
                assert (int(k.max()) >= W40) is wide
                if name == "gap":
                    p = np.flatnonzero(o)
                    a = 64 * 2 + 63
                    assert p[np.searchsorted(p, a) + 1] - a == (5000 if cap > 8192 else 3000) and k[a] > k[p[np.searchsorted(p, a) + 1]]
                if name == "ends":
                    assert np.flatnonzero(o).tolist() == [0, cap - 1]
    for wide in (False, True):
        for name in PCSC_PLANTS:
            k, v, o, sems, want = pcsc_plant(name, wide)
            ref = reference_check(k, v, o, sems, len(sems))
            stray = want[0]
            assert ref.tolist() == [int(o.sum()), 6 + stray, want[0], want[1], 0, 0], (name, wide)
            assert counts_disagree(ref, sems) == stray


def test_reference_check_is_clean_on_oracle_built_layouts(dsa, oracle):
    """words 2-5 are zero on what the oracle builds, among them the layouts test_hip_raw_primitives.py imports"""
    rng = np.random.default_rng(5)
    keys = np.sort(rng.choice(10 ** 6, size=20000, replace=False)) + 1
    src = dsa.dynamicsparsevec(keys, rng.random(20000) + 1.0, binding=oracle)
    src.set_batch(rng.choice(10 ** 6, size=5000) + 1, np.where(rng.random(5000) < 0.2, 0.0, 2.0))
    k, v, o = src.export_layout()
    assert reference_check(k, v, o).tolist() == [src.nnz(), 0, 0, 0, 0, 0]
    # the skewed layouts: everything on one side, dense clumps between empty stretches; as built and after the oracle's root rebalance
    cap, m = 1 << 18, 150000
    for shape in ("left", "right", "clumps"):
        occ = np.zeros(cap, dtype=np.uint8)
        if shape == "left":
            occ[:m] = 1
        elif shape == "right":
            occ[cap - m:] = 1
        else:
            for s in np.sort(np.random.default_rng(9).choice(cap // 4096, size=m // 3000, replace=False)) * 4096:
                occ[s:s + 3000] = 1
        k, v, o = ascending(occ, step=7)
        n = int(o.sum())
        assert reference_check(k, v, o).tolist() == [n, 0, 0, 0, 0, 0]
        b = dsa.import_vector_layout(k, v, o, 16, binding=oracle)
        b.rebalance_root()
        assert reference_check(*b.export_layout()).tolist() == [n, 0, 0, 0, 0, 0]
    # a PackedCSC with a deleted partition and a partition appended by a write
    rng = np.random.default_rng(11)
    rows = [np.sort(rng.choice(5000, size=int(rng.integers(0, 60)), replace=False)) + 1 for _ in range(300)]
    p = dsa.packedcsc(rows, [rng.random(len(r)) + 1.0 for r in rows], binding=oracle)
    p.deletepartition(17)
    p[5, 300] = 2.5
    k, v, o, s = p.export_layout()
    assert reference_check(k, v, o, s, len(s)).tolist() == [p.nnz() + p.nbpartitions(), p.nbpartitions(), 0, 0, 0, 0]
    assert counts_disagree(reference_check(k, v, o, s, len(s)), s) == 0
    # both orientations of a matrix after deletions
    I, J = rng.integers(1, 400, 6000), rng.integers(1, 300, 6000)
    a = dsa.dynamicsparse(I, J, rng.random(6000) + 1.0, binding=oracle)
    a.deletecolumn(7)
    a.deleterow(9)
    for orientation in (COLMAJOR, ROWMAJOR):
        L = a.export_layout(orientation)
        ref = reference_check(L["keys"], L["vals"], L["occ"], L["semaphores"], len(L["semaphores"]))
        assert ref.tolist() == [a.nnz() + a.nbpartitions(orientation), a.nbpartitions(orientation), 0, 0, 0, 0]


# ------------------------------------------------------------------ GPU: planted violations
@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["keys32", "keys64"])
@pytest.mark.parametrize("cap", VECTOR_CAPS)
@pytest.mark.parametrize("name", VECTOR_PLANTS)
def test_checker_reports_planted_vector_violations(dsa, hip, name, cap, wide):
    k, v, o, want = vector_plant(name, cap, wide)
    ref = reference_check(k, v, o)
    assert ref[3] == want
    x = dsa.import_vector_layout(k, v, o, SEG, binding=hip)
    got = x.check()
    assert got[0:6].tolist() == ref.tolist()
    assert got[6] == 0                                        # the counts agree: only the order is wrong
    if name == "clean":
        assert got.sum() == got[0] == int(o.sum())            # nothing but the cell count


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["keys32", "keys64"])
@pytest.mark.parametrize("name", PCSC_PLANTS)
def test_checker_reports_planted_packedcsc_violations(dsa, hip, name, wide):
    k, v, o, sems, want = pcsc_plant(name, wide)
    ref = reference_check(k, v, o, sems, len(sems))
    assert (ref[2], ref[3]) == want
    p = dsa.import_packedcsc_layout(k, v, o, SEG, sems, binding=hip)
    got = p.check()
    assert got[0:6].tolist() == ref.tolist()
    # a stray semaphore cell is one more than the table has live entries: the counts disagree there, and only there
    assert got[6] == counts_disagree(ref, sems) == want[0]
    if name == "clean":
        assert got[2:8].sum() == 0 and got[0] == int(o.sum()) and got[1] == 6


@pytest.mark.gpu
def test_import_rejects_a_table_that_does_not_point_back(dsa, hip):
    """report[4] cannot be planted: dsa_pcsc_import_layout refuses the table with DSA_EARG"""
    k, v, o, sems, at = pcsc_layout(BASE_PARTS, PCSC_CAP, 3)
    for entry, slot in ((2, at[(3, 1)]),        # at a cell that is no semaphore cell
                        (2, at[(6, -1)]),       # at the semaphore cell of another id
                        (4, at[(7, 0)] + 1),    # the entry of the deleted partition at a slot that may be empty
                        (0, PCSC_CAP)):         # behind the capacity (1-based: PCSC_CAP + 1)
        bad = sems.copy()
        bad[entry] = slot + 1
        if entry == 4:
            o2 = o.copy()
            o2[slot] = 0
        else:
            o2 = o
        with pytest.raises(dsa.DsaArgumentError) as ei:
            dsa.import_packedcsc_layout(k, v, o2, SEG, bad, binding=hip)
        assert ei.value.code == dsa.binding.EARG
    # the handle-less failures left nothing behind: the same arrays with the good table import and check clean
    assert dsa.import_packedcsc_layout(k, v, o, SEG, sems, binding=hip).check()[2:7].sum() == 0


# ================================================================== 2. k_view_small through vectors
def cells_layout(occ, wide, seed):
    """ascending keys and random values (a -0.0 among them) in the slots `occ`"""
    k, _, o = ascending(occ, step=3)
    m = o.astype(bool)
    v = np.zeros(len(o), dtype=np.float64)
    v[m] = np.random.default_rng(seed).standard_normal(int(m.sum()))
    v[np.flatnonzero(m)[0]] = -0.0
    if wide:
        widen(k, o)
    return k, v, o


def place(cap, count, how, seed):
    rng = np.random.default_rng(seed)
    occ = np.zeros(cap, dtype=bool)
    nw = cap // 64
    if how == "word0":
        occ[rng.choice(64, size=count, replace=False)] = True
    elif how == "last_word":
        occ[cap - 64 + rng.choice(64, size=count, replace=False)] = True
    elif how == "ends":
        occ[0] = occ[cap - 1] = True
    elif how == "per_word":                     # one cell per word, `count` words from the first to the last, another lane in each
        w = np.linspace(0, nw - 1, count).astype(np.int64) if count > 1 else np.array([nw - 1])
        assert len(np.unique(w)) == count
        occ[w * 64 + (w * 7) % 64] = True
    else:
        occ[rng.choice(cap, size=count, replace=False)] = True
    assert int(occ.sum()) == count
    return occ


VIEW_COUNTS = {128: (1, 2, 64, 100), 65536: (1, 2, 511, 512, 513, 1024, 1025, 60000), 131072: (1, 2, 511, 512, 513, 2048, 100000)}


def view_cases(cap):
    """(count, placement): every placement at every count that fits it"""
    out = []
    for count in VIEW_COUNTS[cap]:
        if count <= 64:
            out += [(count, "word0"), (count, "last_word")]
        if count == 2:
            out.append((count, "ends"))
        if count <= cap // 64:
            out.append((count, "per_word"))
        out.append((count, "random"))
    return out


def assert_reads_back(x, k, v, o, what):
    """nonzeros() are the imported cells in slot order; the structure checks clean and is the imported one afterwards (the view packs
    into the alternate buffer and must not disturb the current one)"""
    m = o.astype(bool)
    gk, gv = x.nonzeros()
    assert len(gk) == int(m.sum()), what
    assert np.array_equal(gk, k[m]), what
    assert np.array_equal(bits(gv), bits(v[m])), what
    r = x.check()
    assert r[0] == int(m.sum()) and r[2:7].sum() == 0, (what, r)
    assert layouts_equal(x.export_layout(), (k, v, o)), what


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["keys32", "keys64"])
@pytest.mark.parametrize("cap", sorted(VIEW_COUNTS))
def test_vector_nonzeros_at_the_view_small_edges(dsa, hip, cap, wide):
    cases = view_cases(cap)
    assert {c for c, _ in cases} == set(VIEW_COUNTS[cap])
    for i, (count, how) in enumerate(cases):
        k, v, o = cells_layout(place(cap, count, how, 100 + i), wide, i)
        x = dsa.import_vector_layout(k, v, o, SEG, binding=hip)
        assert_reads_back(x, k, v, o, (cap, count, how))
        assert_reads_back(x, k, v, o, (cap, count, how, "again"))          # the landing area and its sequence number are reused


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["keys32", "keys64"])
@pytest.mark.parametrize("count", [511, 512, 513])
@pytest.mark.parametrize("cap", [65536, 131072])
def test_vector_filter_equal_add_at_the_pinned_cell_count(dsa, hip, oracle, cap, count, wide):
    """filter reads through read_range (k_view_small at 65536 slots, the general K-pack at 131072); == and + pack both operands and,
    for +, the merged stream through pack_small.  Same imported layouts on both libraries."""
    k, v, o = cells_layout(place(cap, count, "random", count), wide, 1)
    k2, v2, o2 = k.copy(), v.copy(), np.zeros(cap, dtype=np.uint8)              # the same cells in other slots
    m = o.astype(bool)
    p2 = np.flatnonzero(place(cap, count, "random", count + 7))
    k2[:] = 0
    v2[:] = 0
    k2[p2], v2[p2], o2[p2] = k[m], v[m], 1
    k3, v3, o3 = k2.copy(), v2.copy(), o2.copy()                                # one value differs in the last cell
    v3[p2[-1]] += 1.0
    k4, v4, o4 = cells_layout(place(cap, count, "random", count + 9), False, 2)  # other keys, every second one shared with k
    k4[o4.astype(bool)] = np.arange(1, count + 1, dtype=np.int64) * 6
    res = []
    for b in (hip, oracle):
        x, y, z, w = (dsa.import_vector_layout(kk, vv, oo, SEG, n=int(max(k.max(), 6 * count)), binding=b)
                      for kk, vv, oo in ((k, v, o), (k2, v2, o2), (k3, v3, o3), (k4, v4, o4)))
        f = x.filter(lambda e: e[0] % 2 == 0)
        res.append(dict(f=f, eq=(x == y, y == x, x == z, x == w), add=x + w, sub=x - y, self=x + x, x=x))
    g, e = res
    assert g["eq"] == e["eq"] == (True, True, False, False)
    assert_vec_equal(g["f"], e["f"])
    assert g["f"].nnz() == int((k[m] % 2 == 0).sum())
    for op in ("add", "sub", "self"):
        assert np.array_equal(g[op][0], e[op][0]), op
        assert np.array_equal(bits(g[op][1]), bits(e[op][1])), op
    assert len(g["add"][0]) == len(np.union1d(k[m], k4[o4.astype(bool)]))
    assert_reads_back(g["x"], k, v, o, (cap, count, "after the operations"))


# ================================================================== 3. the general K-pack at tile edges
TILE = 4096


def tile_place(cap, how, seed):
    rng = np.random.default_rng(seed)
    occ = np.zeros(cap, dtype=bool)
    nt = cap // TILE
    if how == "last_tile":
        occ[cap - TILE + rng.choice(TILE, size=1500, replace=False)] = True
        occ[cap - 1] = True
    elif how == "tile0":
        occ[rng.choice(TILE, size=1500, replace=False)] = True
        occ[0] = True
    elif how == "tile_edges":                   # the last slot of every tile and the first of the next
        t = np.arange(nt - 1) * TILE
        occ[t + TILE - 1] = True
        occ[t + TILE] = True
    elif how == "empty_middle":
        occ[:] = rng.random(cap) < 0.6
        occ[(nt // 4) * TILE:(3 * nt // 4) * TILE] = False
    else:
        occ[:] = rng.random(cap) < 0.9
    return occ


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["keys32", "keys64"])
@pytest.mark.parametrize("how", ["last_tile", "tile0", "tile_edges", "empty_middle", "dense"])
@pytest.mark.parametrize("cap", [1 << 17, 1 << 18, 1 << 20])
def test_vector_nonzeros_through_the_general_pack(dsa, hip, cap, how, wide):
    k, v, o = cells_layout(tile_place(cap, how, cap % 1000 + len(how)), wide, 3)
    x = dsa.import_vector_layout(k, v, o, SEG, binding=hip)
    assert_reads_back(x, k, v, o, (cap, how))


# ================================================================== 4. matrix views on both sides of 65536 slots
LONG_COLS = {3100: 20000, 3101: 24000, 3102: 30000, 3103: 45000, 3104: 60000, 3105: 70000}
LONG_ROW = 3201
EDGE_COLS = {3301: 511, 3302: 512, 3303: 513}
EDGE_ROWS = {3401: 511, 3402: 512, 3403: 513}
DELETED_COL, DELETED_ROW, ABSENT = 17, 23, 4000
PUSHED_COL = 3104
WIDE_ROW = W40 + 9
DIM = 80000


def matrix_triples(wide):
    """about 3000 x 3000 with 30 k random entries; long columns and one long row whose other keys lie in 5001 .. DIM, away from the
    partitions of 511 / 512 / 513 cells, whose other keys lie in 101 .. 3000.  wide: one long column alone, a row key >= 2^40 in it."""
    rng = np.random.default_rng(4)
    I, J = [rng.integers(1, 3001, 30000)], [rng.integers(1, 3001, 30000)]
    far = lambda n: np.sort(rng.choice(DIM - 5000, size=n, replace=False)) + 5001
    near = lambda n: np.sort(rng.choice(2900, size=n, replace=False)) + 101            # (not the deleted keys)
    if wide:
        rows = far(60000)
        rows[-1] = WIDE_ROW
        I.append(rows)
        J.append(np.full(60000, 3104))
    else:
        for key, n in LONG_COLS.items():
            I.append(far(n))
            J.append(np.full(n, key))
        I.append(np.full(70000, LONG_ROW))
        J.append(far(70000))
        for key, n in EDGE_COLS.items():
            I.append(near(n))
            J.append(np.full(n, key))
        for key, n in EDGE_ROWS.items():
            I.append(np.full(n, key))
            J.append(near(n))
    I, J = np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)
    return I, J, rng.integers(1, 1000, len(I)).astype(np.float64)


def build_matrix(dsa, binding, wide):
    """the bulk build spreads the cells evenly (no two of them in neighbouring slots at these densities); single writes into one long
    column and the long row afterwards push cells together, so that a rank that is wrong among neighbours shows in their views"""
    a = dsa.dynamicsparse(*matrix_triples(wide), binding=binding)
    a.deletecolumn(DELETED_COL)
    a.deleterow(DELETED_ROW)
    rng = np.random.default_rng(6)
    more = rng.choice(DIM - 5000, size=3000, replace=False) + 5001
    a.set_batch(more, np.full(3000, PUSHED_COL), np.full(3000, 7.0))
    if not wide:
        a.set_batch(np.full(3000, LONG_ROW), more, np.full(3000, 9.0))
    return a


def partition_spans(L):
    """{partition key: slots of its range [semaphore + 1, next live semaphore - 1]} from an exported layout and its tables"""
    live = L["col_live"].astype(bool)
    at = L["semaphores"][live]
    assert np.all(np.diff(at) > 0)
    end = np.concatenate([at[1:] - 1, [L["info"]["capacity"]]])
    return dict(zip(L["col_keys"][live].tolist(), (end - at).tolist()))


def neighbours_in(L, key):
    """pairs of occupied neighbouring slots inside the range of partition `key`"""
    live = L["col_live"].astype(bool)
    at = L["semaphores"][live]
    i = L["col_keys"][live].tolist().index(key)
    o = L["occ"][at[i]:at[i] + partition_spans(L)[key]].astype(bool)
    return int((o[:-1] & o[1:]).sum())


_matrices = {}


def oracle_matrix(dsa, oracle, wide):
    """built once, never modified"""
    if wide not in _matrices:
        _matrices[wide] = build_matrix(dsa, oracle, wide)
    return _matrices[wide]


def view_keys(wide):
    if wide:
        return [3104, 1, ABSENT], [WIDE_ROW, 1]
    return (list(LONG_COLS) + list(EDGE_COLS) + [ABSENT, DELETED_COL, 1, 2999, DIM],
            [LONG_ROW] + list(EDGE_ROWS) + [ABSENT, DELETED_ROW, 1, 2999, DIM])


def test_long_partitions_lie_on_both_sides_of_the_small_view(dsa, oracle):
    """on the oracle's layout, which is the HIP library's slot for slot: long columns with a slot range of at most 65536 slots (one
    k_view_small launch) and of more (tile counts, scan, K-pack); the long row is on the far side; the partitions of 511 / 512 / 513
    cells hold exactly that many"""
    b = oracle_matrix(dsa, oracle, False)
    cols, rows = partition_spans(b.export_layout(COLMAJOR)), partition_spans(b.export_layout(ROWMAJOR))
    spans = [cols[key] for key in LONG_COLS]
    assert min(spans) <= 65536 < max(spans), spans
    assert sum(s <= 65536 for s in spans) >= 1 and sum(s > 65536 for s in spans) >= 1
    assert all(cols[key] >= n for key, n in LONG_COLS.items())
    assert rows[LONG_ROW] > 65536
    for key, n in EDGE_COLS.items():
        assert len(b.col_view(key)) == n
    for key, n in EDGE_ROWS.items():
        assert len(b.row_view(key)) == n
    assert len(b.col_view(3105)) == 70000 and len(b.row_view(LONG_ROW)) > 70000 and len(b.col_view(PUSHED_COL)) > 60000
    Lc, Lr = b.export_layout(COLMAJOR), b.export_layout(ROWMAJOR)
    assert cols[PUSHED_COL] > 65536 and neighbours_in(Lc, PUSHED_COL) > 100 and neighbours_in(Lr, LONG_ROW) > 100
    assert b.col_view(ABSENT) == [] and b.col_view(DELETED_COL) == [] and b.row_view(DELETED_ROW) == []
    assert DELETED_COL not in cols and DELETED_ROW not in rows
    bw = oracle_matrix(dsa, oracle, True)
    assert bw.col_view(3104)[-1][0] == WIDE_ROW and len(bw.row_view(WIDE_ROW)) == 1
    assert neighbours_in(bw.export_layout(COLMAJOR), 3104) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["keys32", "keys64"])
def test_matrix_views_device_views_and_slices(dsa, hip, oracle, wide):
    import torch
    b = oracle_matrix(dsa, oracle, wide)
    a = build_matrix(dsa, hip, wide)
    cols, rows = view_keys(wide)
    for orientation, keys in ((COLMAJOR, cols), (ROWMAJOR, rows)):
        col = orientation == COLMAJOR
        for key in keys:
            want = (b.col_view if col else b.row_view)(key)
            wk = np.array([c[0] for c in want], dtype=np.int64)
            wv = np.array([c[1] for c in want], dtype=np.float64)
            got = (a.col_view if col else a.row_view)(key)
            assert np.array_equal(np.array([c[0] for c in got], dtype=np.int64), wk), (orientation, key)
            assert np.array_equal(bits([c[1] for c in got]), bits(wv)), (orientation, key)
            view_dev = a.col_view_dev if col else a.row_view_dev
            dk = torch.empty(len(want) + 1, dtype=torch.int64, device="cuda")           # the arrays hold what the call may write
            dv = torch.empty(len(want) + 1, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            n = view_dev(key, dk.data_ptr(), dv.data_ptr(), len(want))
            a.sync()
            assert n == len(want), (orientation, key)
            assert np.array_equal(dk[:n].cpu().numpy(), wk) and np.array_equal(bits(dv[:n].cpu().numpy()), bits(wv)), (orientation, key)
            if len(want) > 0:
                with pytest.raises(dsa.DsaError) as ei:
                    view_dev(key, dk.data_ptr(), dv.data_ptr(), len(want) - 1)
                assert ei.value.code == dsa.binding.ECAP, (orientation, key)
            assert_vec_equal((a.col_slice if col else a.row_slice)(key), (b.col_slice if col else b.row_slice)(key))
        assert a.check(orientation)[2:7].sum() == 0


# ================================================================== 5. lookups at the 64 / 65 switch
GET_SIZES = (1, 63, 64, 65, 129)


def half_and_half(rng, present, absent, n):
    """n queries, present and absent ones alternating (the odd one is present)"""
    q = np.empty(n, dtype=np.int64)
    q[0::2] = rng.choice(present, size=len(q[0::2]))
    q[1::2] = rng.choice(absent, size=len(q[1::2]))
    return q


@pytest.mark.gpu
def test_vector_lookups_on_both_sides_of_the_switch(dsa, hip, oracle):
    rng = np.random.default_rng(8)
    keys = np.arange(1, 5001, dtype=np.int64) * 3
    vals = rng.standard_normal(5000)
    x, y = (dsa.dynamicsparsevec(keys, vals, binding=b) for b in (hip, oracle))
    for n in GET_SIZES:
        q = half_and_half(rng, keys, keys + 1, n)
        got, want = x.get_batch(q), y.get_batch(q)
        assert np.array_equal(bits(got), bits(want)), n
        assert np.array_equal(bits(got[0::2]), bits(vals[q[0::2] // 3 - 1])) and np.all(bits(got[1::2]) == 0), n
    q = keys[:64] + 1                                        # present in lanes 0 and 63 only
    q[0], q[63] = keys[10], keys[4999]
    got = x.get_batch(q)
    assert np.array_equal(bits(got), bits(y.get_batch(q)))
    assert np.all(bits(got[1:63]) == 0) and bits(got[[0, 63]]).tolist() == bits(vals[[10, 4999]]).tolist()
    assert x[int(keys[7])] == vals[7] and x[int(keys[7]) + 1] == 0.0


@pytest.mark.gpu
def test_packedcsc_lookups_and_the_error_word(dsa, hip, oracle):
    rng = np.random.default_rng(9)
    rows = [np.sort(rng.choice(500, size=int(rng.integers(1, 40)), replace=False)) + 1 for _ in range(40)]
    vals = [rng.standard_normal(len(r)) for r in rows]
    p, o = (dsa.packedcsc(rows, vals, binding=b) for b in (hip, oracle))
    table_len = p.info()["table_len"]
    assert table_len == 40

    def valid(n):
        part = rng.integers(1, 41, size=n)
        key = np.array([rng.choice(rows[j - 1]) if i % 2 == 0 else 501 + i for i, j in enumerate(part.tolist())], dtype=np.int64)
        got = np.array([p[int(k), int(j)] for k, j in zip(key, part)])
        want = np.array([o[int(k), int(j)] for k, j in zip(key, part)])
        assert np.array_equal(bits(got), bits(want)), n
        assert np.all(bits(got[1::2]) == 0) and np.all(got[0::2] != 0.0)

    for n in GET_SIZES:
        valid(n)
    for bad in (0, table_len + 1):
        with pytest.raises(dsa.DsaBoundsError) as ei:
            p[int(rows[0][0]), bad]
        assert ei.value.code == dsa.binding.EBOUNDS
        # the same handle right after the error: the error word and the sequence number of its landing area are reused
        assert bits([p[int(rows[0][0]), 1]]).tolist() == bits([vals[0][0]]).tolist()
        valid(3)
    assert p.check()[2:7].sum() == 0


@pytest.mark.gpu
def test_matrix_lookups_on_both_sides_of_the_switch(dsa, hip, oracle):
    rng = np.random.default_rng(10)
    I, J = rng.integers(1, 301, 4000), rng.integers(1, 201, 4000) * 2          # even columns only: an odd column is absent
    V = rng.integers(1, 1000, 4000).astype(np.float64)
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    for n in GET_SIZES:
        pick = rng.integers(0, 4000, size=n)
        qi, qj = I[pick].copy(), J[pick].copy()
        qj[1::2] += 1                                        # an absent column: 0.0, not an error
        got, want = a.get_batch(qi, qj), b.get_batch(qi, qj)
        assert np.array_equal(bits(got), bits(want)), n
        assert np.all(got[0::2] != 0.0) and np.all(bits(got[1::2]) == 0), n
    qi, qj = np.full(64, 5, dtype=np.int64), np.arange(64, dtype=np.int64) * 2 + 1001      # columns behind the last one
    qi[0], qj[0], qi[63], qj[63] = I[0], J[0], I[1], J[1]
    got = a.get_batch(qi, qj)
    assert np.array_equal(bits(got), bits(b.get_batch(qi, qj)))
    assert np.all(bits(got[1:63]) == 0) and got[0] != 0.0 and got[63] != 0.0
    # a row the present column does not hold, and keys below 1: answers, not errors, and the next call is served
    for qi, qj in (([100000], [int(J[0])]), ([int(I[0])], [-3]), ([int(I[0])], [0])):
        assert np.array_equal(bits(a.get_batch(qi, qj)), bits(b.get_batch(qi, qj)))
    assert a[int(I[0]), int(J[0])] == b[int(I[0]), int(J[0])] != 0.0
