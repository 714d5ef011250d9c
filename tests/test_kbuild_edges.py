"""K-build (csrc/build.hip, csrc/build_host.hip) at its branch points: the derived twin and its threshold, the bit-width switches of
build_prepare, duplicate runs placed on wave-row / wave-block / tile edges and at both ends of the sorted stream, speculative buffers
handed back, the one-launch small vector and its hand-over, PackedCSC semaphores on all three sort paths, the fill buffer's running key
ranges across uploaded pieces, and the scan kernels' items-per-thread switch.

Two references: the CPU oracle, slot for slot (assert_mat_equal / assert_vec_equal / layouts_equal), and fold_reference below — numpy
and Python only, no project code — bit for bit, so that a mistake shared by the oracle and the kernels does not pass.
Every docstring names the constant or branch its test aims at (file:symbol): when that constant moves, the test moves with it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import assert_mat_equal, layouts_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

COMBINES = ("+", "*", "last")
TWIN_MIN = 1 << 16            # matwrite_host.hip:mat_build_major_dev — from this many triples on the rowmajor twin is derived
WAVE_ROW, WAVE_BLOCK, TILE = 64, 1024, 4096      # build.hip: 64 lanes, RS_PER_WAVE, RS_TILE
SMALL_VEC_MAX = 1024          # host.h:VIEW_AREA_CELLS == build.hip:BSV_MAX


# ------------------------------------------------------------------------------------------------------------------------------------
# the plain reference
# ------------------------------------------------------------------------------------------------------------------------------------
def fold_reference(I, J, V, combine):
    """Distinct cells sorted by (column, row); each value the left fold of the cell's duplicates in input order, starting from the
    first value (not from 0.0: -0.0 survives).  J = None: a vector.  Returns (rows, columns, values)."""
    I = np.asarray(I, dtype=np.int64)
    n = len(I)
    J = np.zeros(n, dtype=np.int64) if J is None else np.asarray(J, dtype=np.int64)
    V = np.asarray(V, dtype=np.float64)
    if n == 0:
        return I, J, V
    order = np.lexsort((I, J))                     # stable: equal (column, row) pairs stay in input order
    si, sj, sv = I[order], J[order], V[order].tolist()
    head = np.ones(n, dtype=bool)
    head[1:] = (si[1:] != si[:-1]) | (sj[1:] != sj[:-1])
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    out = np.empty(len(starts), dtype=np.float64)
    for c, (s, e) in enumerate(zip(starts.tolist(), ends.tolist())):
        acc = sv[s]
        if combine == "+":
            for t in range(s + 1, e):
                acc = acc + sv[t]
        elif combine == "*":
            for t in range(s + 1, e):
                acc = acc * sv[t]
        else:
            acc = sv[e - 1]
        out[c] = acc
    return si[starts], sj[starts], out


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def bit_width(x):
    return int(x).bit_length()


def clean(report):
    return not np.asarray(report)[2:7].any()


# ------------------------------------------------------------------------------------------------------------------------------------
# what a structure stores, read from its exported layout (works for any key range, unlike findnz)
# ------------------------------------------------------------------------------------------------------------------------------------
def _cells_of_layout(keys, vals, occ, part_keys=None):
    m = np.asarray(occ).astype(bool)
    k, v = keys[m], vals[m]
    sem = k == 0
    ids = v[sem].astype(np.int64)                           # semaphore cells hold their partition id
    which = np.cumsum(sem) - 1                              # index of the semaphore in front of every slot
    assert len(k) == 0 or sem[0]                            # every entry has a semaphore in front of it
    pid = ids[which[~sem]] if len(ids) else np.zeros(0, dtype=np.int64)
    part = pid if part_keys is None else np.asarray(part_keys)[pid - 1]
    return part, k[~sem], v[~sem]


def matrix_cells(mat, orientation):
    """(partition keys, keys, values) of one orientation in slot order"""
    L = mat.export_layout(orientation)
    return _cells_of_layout(L["keys"], L["vals"], L["occ"], L["col_keys"])


def pcsc_cells(p):
    k, v, o, _ = p.export_layout()
    return _cells_of_layout(k, v, o)


def assert_vec_equal(a, b):
    ia, ib = a.info(), b.info()
    for k in ("capacity", "segment_capacity", "nb_segments", "nb_elements", "height"):
        assert ia[k] == ib[k], (k, ia, ib)
    assert len(a) == len(b)
    assert layouts_equal(a.export_layout(), b.export_layout())


def assert_matrix_is_fold(mat, I, J, V):
    """both orientations of a HIP matrix against fold_reference, bit for bit"""
    rows, cols, vals = fold_reference(I, J, V, "+")
    pc, kr, v0 = matrix_cells(mat, 0)                       # colmajor: partitions = columns, keys = rows
    assert np.array_equal(pc, cols) and np.array_equal(kr, rows)
    assert bits_equal(v0, vals)
    cols_t, rows_t, vals_t = fold_reference(J, I, V, "+")   # rowmajor: the same cells sorted by (row, column)
    pr, kc, v1 = matrix_cells(mat, 1)
    assert np.array_equal(pr, rows_t) and np.array_equal(kc, cols_t)
    assert bits_equal(v1, vals_t)


def check_matrix(dsa, hip, oracle, I, J, V, findnz=False):
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    assert_mat_equal(a, b)
    assert_matrix_is_fold(a, I, J, V)
    if findnz:                                              # (keys 1..m / 1..n only)
        rows, cols, vals = fold_reference(I, J, V, "+")
        fi, fj, fv = a.findnz()
        assert np.array_equal(fi, rows) and np.array_equal(fj, cols) and bits_equal(fv, vals)
    assert clean(a.check(0)) and clean(a.check(1))
    return a, b


def check_vector(dsa, hip, oracle, K, V, combine):
    a = dsa.dynamicsparsevec(K, V, combine, binding=hip)
    b = dsa.dynamicsparsevec(K, V, combine, binding=oracle)
    assert_vec_equal(a, b)
    keys, _, vals = fold_reference(K, None, V, combine)
    nk, nv = a.nonzeros()
    assert np.array_equal(nk, keys) and bits_equal(nv, vals), combine
    assert clean(a.check())
    return a, b


def check_pcsc(dsa, hip, oracle, rows, vals, combine):
    a = dsa.packedcsc(rows, vals, combine, binding=hip)
    b = dsa.packedcsc(rows, vals, combine, binding=oracle)
    la, lb = a.export_layout(), b.export_layout()
    assert layouts_equal(la[:3], lb[:3]) and np.array_equal(la[3], lb[3])
    assert a.nnz() == b.nnz() and a.nbpartitions() == b.nbpartitions() == len(rows)
    part = np.concatenate([np.full(len(r), p + 1, dtype=np.int64) for p, r in enumerate(rows)] + [np.zeros(0, dtype=np.int64)])
    keys = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, dtype=np.int64)])
    flat = np.concatenate([np.asarray(v, dtype=np.float64) for v in vals] + [np.zeros(0)])
    rk, rp, rv = fold_reference(keys, part, flat, combine)
    hp, hk, hv = pcsc_cells(a)
    assert np.array_equal(hp, rp) and np.array_equal(hk, rk) and bits_equal(hv, rv), combine
    assert clean(a.check())
    return a, b


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs: values that make the fold order visible, the special cells, key ranges with both ends forced in
# ------------------------------------------------------------------------------------------------------------------------------------
def mixed_values(g, n, combine="+"):
    """'+' / 'last': magnitudes 1e10 and 1e-3 mixed (a sum in another order rounds differently); '*': factors around 1 (a long product
    neither overflows nor underflows, and still rounds differently in another order)"""
    if combine == "*":
        return 1.0 + (g.random(n) - 0.5) * 1e-3
    return (0.5 + g.random(n)) * np.where(g.random(n) < 0.5, 1e10, 1e-3)


CANCEL_RUN = (1e10, 2.5, -1e10, -2.5)      # left fold with '+': exactly +0.0, a stored zero


def set_cell_values(V, where, values):
    """values of one cell's duplicates, in input order"""
    where = np.sort(np.asarray(where))
    assert len(where) == len(values)
    V[where] = values


def decorate(g, I, J, V):
    """four special cells from four cells that occur once: a -0.0, a NaN, a run [Inf, 1.0] and the run CANCEL_RUN.  Adds four triples
    (coordinates that exist already: the key ranges stay what they were)."""
    J0 = np.zeros(len(I), dtype=np.int64) if J is None else J
    order = np.lexsort((I, J0))
    si, sj = I[order], J0[order]
    head = np.ones(len(I), dtype=bool)
    head[1:] = (si[1:] != si[:-1]) | (sj[1:] != sj[:-1])
    starts = np.flatnonzero(head)
    single = order[starts[np.diff(np.append(starts, len(I))) == 1]]
    assert len(single) >= 4
    c = np.sort(g.choice(single, 4, replace=False))
    V = V.copy()
    V[c[0]], V[c[1]], V[c[2]], V[c[3]] = -0.0, np.nan, np.inf, CANCEL_RUN[0]
    extra = np.array([c[2], c[3], c[3], c[3]])
    I2 = np.concatenate([I, I[extra]])
    J2 = None if J is None else np.concatenate([J, J[extra]])
    V2 = np.concatenate([V, [1.0, CANCEL_RUN[1], CANCEL_RUN[2], CANCEL_RUN[3]]])
    return I2, J2, V2


def ranged(g, n, lo, hi):
    """n keys in [lo, hi], never the reserved key 0"""
    k = g.integers(lo, hi, n, endpoint=True, dtype=np.int64)
    k[k == 0] = 1 if lo <= 1 <= hi else lo
    return k


def gen_triples(seed, nnz, rows, cols, dup=0.1, combine="+"):
    """nnz triples with rows in [rows[0], rows[1]] and columns in [cols[0], cols[1]], all four ends forced into the data, about `dup` of
    the triples repeating an earlier cell, the special cells of decorate() among them, in random input order"""
    g = np.random.default_rng(seed)
    n = nnz - 4
    nb = n - int(n * dup)
    I, J = ranged(g, nb, *rows), ranged(g, nb, *cols)
    I[0], I[1], J[2], J[3] = rows[0], rows[1], cols[0], cols[1]
    again = g.integers(0, nb, n - nb)
    I, J = np.concatenate([I, I[again]]), np.concatenate([J, J[again]])
    perm = g.permutation(n)
    I, J = I[perm], J[perm]
    I, J, V = decorate(g, I, J, mixed_values(g, n, combine))
    assert len(I) == nnz and I.min() == rows[0] and I.max() == rows[1] and J.min() == cols[0] and J.max() == cols[1]
    assert not (I == 0).any() and not (J == 0).any()
    return I, J, V


def composite_bits(I, J, nnz):
    """(row bits, column bits, index bits) as build.hip:build_prepare computes them for the colmajor orientation"""
    kbits = max(1, bit_width(int(I.max()) - int(I.min())))
    pbits = bit_width(int(J.max()) - int(J.min()))
    return kbits, pbits, max(1, bit_width(nnz - 1))


# case 1: rows < 300, columns < 70 000, about 10 % duplicates
def twin_case(nnz):
    return gen_triples(1000 + nnz, nnz, (1, 299), (1, 69999))


def single_column_case():
    I, _, V = gen_triples(11, TWIN_MIN, (1, 100000), (12, 12))
    return I, np.full(len(I), 12, dtype=np.int64), V


def single_row_case():
    _, J, V = gen_triples(12, TWIN_MIN, (-3, -3), (1, 100000))
    return np.full(len(J), -3, dtype=np.int64), J, V


# case 2: 24 + 24 bits of keys
SPAN24 = (1 << 24) - 1
BOUNDARY = {"negative_rows": (-(1 << 23), 7), "offset_columns": (5, (1 << 40) - 12345)}


def boundary_case(variant, nnz):
    r0, c0 = BOUNDARY[variant]
    return gen_triples(2000 + nnz, nnz, (r0, r0 + SPAN24), (c0, c0 + SPAN24))


# case 3: 32 + 32 bits, keys that still fit 32-bit storage
def full64_case():
    return gen_triples(3, TWIN_MIN, (-(1 << 31), (1 << 31) - 1), (-(1 << 31), (1 << 31) - 1))


# case 4: 33 + 32 bits
def general_case(nnz):
    return gen_triples(4000 + nnz, nnz, (1, 1 << 33), (-(1 << 31), (1 << 31) - 1))


def path_cases():
    """what test_mat_build_major_reports_the_intended_path builds in its child process"""
    yield "twin_65535", twin_case(TWIN_MIN - 1)
    yield "twin_65536", twin_case(TWIN_MIN)
    yield "boundary_65536", boundary_case("negative_rows", TWIN_MIN)
    yield "boundary_65537", boundary_case("offset_columns", TWIN_MIN + 1)
    yield "general_65536", general_case(TWIN_MIN)
    yield "general_30000", general_case(30000)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. threshold of the derived twin
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [TWIN_MIN - 1, TWIN_MIN])
def test_twin_threshold(dsa, hip, oracle, nnz):
    """matwrite_host.hip:mat_build_major_dev `nnz >= (1 << 16)`: 65535 triples are two independent builds, 65536 one sort and a twin
    derived from der_comp / der_val (build_host.hip:mat_build_both_dev, build.hip:build_derived_sort).  Same generator on both sides."""
    I, J, V = twin_case(nnz)
    kbits, pbits, ibits = composite_bits(I, J, nnz)
    assert kbits + pbits + ibits <= 64                       # index-in-word sort
    ncells = len(fold_reference(I, J, V, "+")[0])
    assert 0.05 * nnz < nnz - ncells < 0.15 * nnz            # about 10 % duplicates
    check_matrix(dsa, hip, oracle, I, J, V, findnz=True)


def test_twin_of_a_single_column_and_of_a_single_row(dsa, hip, oracle):
    """build_host.hip:mat_build_both_dev passes the sibling's pbits as the twin's kbits: a single column is pbits = 0, so the twin runs
    build.hip:k_bf_emit / bf_flags with kbits = 0 (kmask = 0); a single row is kbits = max(1, 0) = 1 in build.hip:build_prepare and a
    twin with pbits = 1 (one radix pass over one bit)."""
    I, J, V = single_column_case()
    assert len(I) == TWIN_MIN and composite_bits(I, J, len(I))[1] == 0
    check_matrix(dsa, hip, oracle, I, J, V, findnz=True)
    I, J, V = single_row_case()
    assert len(I) == TWIN_MIN and composite_bits(I, J, len(I))[0] == 1
    check_matrix(dsa, hip, oracle, I, J, V)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. - 4. the bit-width switches of build_prepare
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(BOUNDARY))
@pytest.mark.parametrize("nnz,total", [(TWIN_MIN, 64), (TWIN_MIN + 1, 65)])
def test_index_in_word_against_payload_sort(dsa, hip, oracle, variant, nnz, total):
    """build.hip:build_prepare `s.ibits = total_bits + ibits_need <= 64 ? ibits_need : 0`: 24 + 24 bits of keys and 16 bits of input
    index are exactly one word (8-byte sort, values gathered at the emit); one triple more is 17 index bits: the payload sort
    (k_rs_scatter<true>), still one composite and still a derived twin.  Negative rows / columns near 2^40: the stored keys are wide
    on one side only."""
    I, J, V = boundary_case(variant, nnz)
    kbits, pbits, ibits = composite_bits(I, J, nnz)
    assert (kbits, pbits) == (24, 24) and ibits == bit_width(nnz - 1) and kbits + pbits + ibits == total
    assert nnz >= TWIN_MIN
    check_matrix(dsa, hip, oracle, I, J, V)


def test_64_bit_composite_with_narrow_stored_keys(dsa, hip, oracle):
    """build.hip:build_prepare `s.kbits + s.pbits > 64` is false at exactly 64: 8 radix passes fill all 8 rows of ghist, payload path,
    kmask of k_bf_emit at kbits = 32; the twin (build.hip:build_derived_sort) sorts at shifts kbits + 8 * pass = 32 ... 56.  Both key
    ranges end at the ends of Int32, so host.h:needs_wide stays false: 32-bit keys in HBM."""
    I, J, V = full64_case()
    nnz = len(I)
    kbits, pbits, ibits = composite_bits(I, J, nnz)
    assert (kbits, pbits) == (32, 32) and kbits + pbits == 64 and kbits + pbits + ibits > 64 and nnz == TWIN_MIN
    assert np.abs(I).max() <= 1 << 31 and np.abs(J).max() <= 1 << 31
    check_matrix(dsa, hip, oracle, I, J, V)


@pytest.mark.parametrize("nnz", [30000, TWIN_MIN])
def test_smallest_general_path(dsa, hip, oracle, nnz):
    """build.hip:build_prepare `s.kbits + s.pbits > 64` at 33 + 32 = 65: prepare_wide / emit_wide.  At 65536 triples
    build_host.hip:mat_build_both_dev returns false and matwrite_host.hip:mat_build_major_dev builds B with pma_build_dev (`!both`);
    at 30 000 both orientations go through pma_build_dev side by side."""
    I, J, V = general_case(nnz)
    kbits, pbits, _ = composite_bits(I, J, nnz)
    assert (kbits, pbits) == (33, 32) and kbits + pbits == 65
    check_matrix(dsa, hip, oracle, I, J, V)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. duplicate runs at known positions of the sorted stream
# ------------------------------------------------------------------------------------------------------------------------------------
PLACED_N = 70000
PLACED_RUNS = (                                   # (sorted index of the first duplicate, length)
    (0, 70),                                      # the first elements of the stream
    (127, 65),                                    # starts in lane 63 of a wave row
    (WAVE_BLOCK - 50, 129),                       # crosses a wave's block of 1024
    (TILE - 100, 200),                            # crosses a tile
    (4301, 64), (4403, 65), (4517, 128), (4711, 129),
    (2 * TILE - 300, 5000),                       # covers tile 2 entirely
    (13000, 2), (13100, 4),                       # the [Inf, 1.0] and CANCEL_RUN cells
    (PLACED_N - 70, 70),                          # the last elements: the largest composite
)
PLACED_SINGLE = {"negzero": 200, "nan": 300}      # sorted indices of two cells that occur once


def placed_cells(seed):
    """cell number (= rank of the cell in sorted order) of every triple, shuffled, and the cell at every sorted index"""
    mult, pos = [], 0
    for start, length in PLACED_RUNS:
        assert start >= pos
        mult += [1] * (start - pos) + [length]
        pos = start + length
    assert pos == PLACED_N
    mult = np.array(mult)
    sorted_cells = np.repeat(np.arange(len(mult)), mult)
    g = np.random.default_rng(seed)
    return g, sorted_cells[g.permutation(PLACED_N)], sorted_cells


def placed_values(g, cell, sorted_cells, combine):
    V = mixed_values(g, len(cell), combine)
    set_cell_values(V, np.flatnonzero(cell == sorted_cells[PLACED_SINGLE["negzero"]]), [-0.0])
    set_cell_values(V, np.flatnonzero(cell == sorted_cells[PLACED_SINGLE["nan"]]), [np.nan])
    set_cell_values(V, np.flatnonzero(cell == sorted_cells[13000]), [np.inf, 1.0])
    set_cell_values(V, np.flatnonzero(cell == sorted_cells[13100]), CANCEL_RUN)
    return V


def assert_placement(I, J):
    """the runs of equal (J, I) in the order a stable sort leaves are where PLACED_RUNS says — recomputed from the triples"""
    n = len(I)
    J = np.zeros(n, dtype=np.int64) if J is None else J
    order = np.lexsort((I, J))
    si, sj = I[order], J[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (si[1:] != si[:-1]) | (sj[1:] != sj[:-1])
    starts = np.flatnonzero(head)
    length = dict(zip(starts.tolist(), np.diff(np.append(starts, n)).tolist()))
    assert n == PLACED_N >= TWIN_MIN
    for start, ln in PLACED_RUNS:
        assert length[start] == ln, (start, ln)
    assert sorted(v for v in length.values() if v > 1) == sorted(ln for _, ln in PLACED_RUNS)
    crosses = lambda s, ln, unit: s // unit != (s + ln - 1) // unit and s % unit != 0
    assert length[127] == 65 and 127 % WAVE_ROW == 63
    s, ln = PLACED_RUNS[2]
    assert ln == 129 and crosses(s, ln, WAVE_BLOCK)
    s, ln = PLACED_RUNS[3]
    assert ln == 200 and crosses(s, ln, TILE)
    assert {64, 65, 128, 129} <= set(length.values())
    s, ln = PLACED_RUNS[8]
    assert ln == 5000 and s <= 2 * TILE and 3 * TILE <= s + ln
    assert length[0] == 70 and length[n - 70] == 70
    for p in PLACED_SINGLE.values():
        assert length[p] == 1


PLACED_ROWS = 257


def placed_matrix():
    g, cell, sorted_cells = placed_cells(5)
    I = (cell % PLACED_ROWS) * 2 - 101                     # odd: never the reserved key 0; (column, row) order = cell order
    J = (cell // PLACED_ROWS) * 3 - 50
    return g, cell, sorted_cells, I, J


def test_placed_duplicate_runs_matrix(dsa, hip, oracle):
    """build.hip:FOLD_INLINE (64) and the hand-over to k_fold_long, with `der_val[lr.dpos]` for the twin; bf_flags' lane-0 / lane-63
    neighbour loads at wave rows (64), RS_PER_WAVE (1024) and RS_TILE (4096); k_bf_emit's `nxt` and k_fold_long's `i < n` guards for a
    run that ends the stream.  70 000 triples: the derived path."""
    g, cell, sorted_cells, I, J = placed_matrix()
    assert_placement(I, J)
    V = placed_values(g, cell, sorted_cells, "+")
    check_matrix(dsa, hip, oracle, I, J, V)


@pytest.mark.parametrize("combine", COMBINES)
def test_placed_duplicate_runs_vector(dsa, hip, oracle, combine):
    """the placements of test_placed_duplicate_runs_matrix in mode 1 (build_host.hip:pma_build_dev, no partitions) above
    host.h:VIEW_AREA_CELLS pairs, with each build.hip:bld_combine"""
    g, cell, sorted_cells = placed_cells(6)
    K = cell * 3 - 1000                                    # (1000 is no multiple of 3: never key 0)
    assert len(K) > SMALL_VEC_MAX
    assert_placement(K, None)
    V = placed_values(g, cell, sorted_cells, combine)
    check_vector(dsa, hip, oracle, K, V, combine)


@pytest.mark.parametrize("combine", COMBINES)
def test_placed_duplicate_runs_packedcsc(dsa, hip, oracle, combine):
    """the placements of test_placed_duplicate_runs_matrix in mode 2 (explicit partition ids; build.hip:k_bf_emit writes scell for
    k_emit_sems), with each build.hip:bld_combine"""
    g, cell, sorted_cells = placed_cells(7)
    key = (cell % PLACED_ROWS) * 2 - 101
    part = cell // PLACED_ROWS + 1
    assert_placement(key, part)
    V = placed_values(g, cell, sorted_cells, combine)
    order = np.argsort(part, kind="stable")                # the constructor takes one list per partition: input order inside each
    cuts = np.cumsum(np.bincount(part, minlength=part.max() + 1)[1:])[:-1]
    rows, vals = np.split(key[order], cuts), np.split(V[order], cuts)
    assert len(rows) == part.max()
    check_pcsc(dsa, hip, oracle, rows, vals, combine)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. speculative buffers handed back
# ------------------------------------------------------------------------------------------------------------------------------------
def capacity_for(n):
    """pma_host.hip:capacity_for — the power of two at or above n / 0.7"""
    return 1 << (int(np.ceil(n / 0.7)) - 1).bit_length()


@pytest.mark.parametrize("combine", COMBINES)
def test_speculative_buffers_handed_back(dsa, hip, oracle, combine):
    """build_host.hip:pma_build_dev `release_prealloc` — `P.cap_alloc > 8 * capacity_for(n) && P.cap_alloc > (1 << 20)`: the buffers
    sized under the sort are 2 * capacity_for(380 000) = 2 * 2^20 = 2^21 slots, which is > 2^20 and > 8 * capacity_for(40) = 8 * 64;
    they go back and the vector is sized for its 40 entries.  It must then take writes (growing from the small buffers) like the
    oracle's."""
    nnz, nkeys = 380000, 40
    assert capacity_for(nnz) == 1 << 20 and capacity_for(nkeys) == 64
    assert 2 * capacity_for(nnz) == 1 << 21 > 1 << 20 and 2 * capacity_for(nnz) > 8 * capacity_for(nkeys)
    g = np.random.default_rng(60)
    heavy = g.integers(1, 37, nnz - 8) * 1000003 - 20000000    # 36 keys with about 10 555 duplicates each, some negative
    K = np.concatenate([heavy, [37000] * 1, [38000] * 1, [39000] * 2, [40000] * 4])
    V = np.concatenate([mixed_values(g, nnz - 8, combine), [-0.0, np.nan, np.inf, 1.0], CANCEL_RUN])
    assert len(K) == nnz and len(np.unique(K)) == nkeys
    a, b = check_vector(dsa, hip, oracle, K, V, combine)
    assert a.info()["capacity"] == b.info()["capacity"] == capacity_for(nkeys)
    k2 = g.permutation(np.arange(50001, 53001))
    v2 = mixed_values(g, len(k2))
    for v in (a, b):
        v[37000] = 4.5
        v.set_batch(k2, v2)
    assert_vec_equal(a, b)
    assert clean(a.check())


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. the one-launch small vector and its hand-over to the general builder
# ------------------------------------------------------------------------------------------------------------------------------------
SMALL_PATTERNS = ("equal", "descending", "half", "wide")


def small_vector(pattern, n, combine, seed=0):
    g = np.random.default_rng(7000 + 10 * n + seed)
    V = mixed_values(g, n, combine)
    if pattern == "equal":
        K = np.full(n, 17, dtype=np.int64)
    elif pattern == "descending":
        K = np.arange(n, 0, -1, dtype=np.int64) * 5
    elif pattern == "half":
        K = g.permutation(np.arange(n, dtype=np.int64) // 2 + 1)
    else:                                                      # one key beyond 2^31 and a negative one: 64-bit keys in HBM
        K = g.permutation(np.arange(1, n + 1, dtype=np.int64))
        K[0] = (1 << 31) + 5
        if n >= 2:
            K[1] = -7
    if pattern != "equal" and n >= 64:                         # (in one long run a NaN would hide the order of everything behind it)
        for key, special in zip(np.unique(K)[:3], (-0.0, np.nan, np.inf)):
            V[np.flatnonzero(K == key)[0]] = special
    return K, V


@pytest.mark.parametrize("n", [1, 2, 64, 65, 1023, 1024, 1025])
def test_small_vector_launch(dsa, hip, oracle, n):
    """build_host.hip:pma_build_from_host `nnz <= VIEW_AREA_CELLS` (1024): up to there build.hip:k_build_small_vec — one 1024-thread
    workgroup, ranks with the `j < i` tie-break, ballots per 64 lanes — and from 1025 on the general builder."""
    for pattern in SMALL_PATTERNS:
        for combine in COMBINES:
            K, V = small_vector(pattern, n, combine)
            check_vector(dsa, hip, oracle, K, V, combine)


@pytest.mark.parametrize("pattern", SMALL_PATTERNS)
def test_small_vector_handover_agrees_across_the_threshold(dsa, hip, pattern):
    """host.h:VIEW_AREA_CELLS: 1024 pairs through build.hip:k_build_small_vec and the same pairs plus one with a new key through the
    general builder store the same entries for the shared input, bit for bit"""
    for combine in COMBINES:
        K, V = small_vector(pattern, SMALL_VEC_MAX, combine)
        new_key = int(K.max()) + 1
        K2, V2 = np.append(K, new_key), np.append(V, 3.25)
        assert len(K) == SMALL_VEC_MAX and len(K2) == SMALL_VEC_MAX + 1 and new_key not in K
        ka, va = dsa.dynamicsparsevec(K, V, combine, binding=hip).nonzeros()
        kb, vb = dsa.dynamicsparsevec(K2, V2, combine, binding=hip).nonzeros()
        keep = kb != new_key
        assert keep.sum() == len(kb) - 1 and vb[~keep][0] == 3.25
        assert np.array_equal(ka, kb[keep]) and bits_equal(va, vb[keep]), combine


# ------------------------------------------------------------------------------------------------------------------------------------
# 8. PackedCSC semaphores
# ------------------------------------------------------------------------------------------------------------------------------------
def pcsc_input(g, lens, lo, hi, combine):
    """one key list per partition: a dozen candidate keys from [lo, hi] (both ends among them), drawn with repetition, unsorted"""
    cand = np.unique(np.concatenate([ranged(g, 10, lo, hi), [lo, hi]]))
    rows = [g.choice(cand, int(c)) for c in lens]
    filled = [p for p, c in enumerate(lens) if c > 0]
    rows[filled[0]][0], rows[filled[-1]][-1] = lo, hi
    vals = [mixed_values(g, len(r), combine) for r in rows]
    return rows, vals


def pcsc_lens(g, nparts, kind, per):
    if kind == "one":                                          # all empty but one
        lens = np.zeros(nparts, dtype=np.int64)
        lens[nparts // 2] = 2 * per
        return lens
    lens = g.integers(1, 2 * per, nparts)
    if nparts > 1:
        lens[0] = lens[-1] = 0                                 # empty first and last
    if nparts >= 30:
        lens[nparts // 2: nparts // 2 + 10] = 0                # ten empty partitions in a row
    return lens


@pytest.mark.parametrize("nparts", [1, 255, 256, 257, 600])
def test_packedcsc_semaphores_at_block_edges(dsa, hip, oracle, nparts):
    """build.hip:k_emit_sems — one thread per partition in blocks of 256 (`p > nparts` guard), a binary search for the first cell of
    each partition: empty partitions first, last, ten in a row, and all empty but one.  nparts = 1 is pbits = 0
    (build_host.hip:pma_build_from_host sets the partition range to [1, nparts])."""
    g = np.random.default_rng(800 + nparts)
    for kind in ("edges", "one"):
        for combine in COMBINES:
            lens = pcsc_lens(g, nparts, kind, 4)
            rows, vals = pcsc_input(g, lens, -40, 5000, combine)
            nnz = int(lens.sum())
            assert bit_width(5040) + bit_width(nparts - 1) + bit_width(nnz - 1) <= 64          # composite path, index in word
            a, _ = check_pcsc(dsa, hip, oracle, rows, vals, combine)
            assert a.nbpartitions() == nparts


def test_packedcsc_without_entries(dsa, hip, oracle):
    """build_host.hip:pma_build_dev `nnz == 0` with mode 2: only the semaphore cells of the 5 partitions"""
    rows, vals = [[] for _ in range(5)], [[] for _ in range(5)]
    a, _ = check_pcsc(dsa, hip, oracle, rows, vals, "+")
    assert a.nbpartitions() == 5 and a.nnz() == 0


@pytest.mark.parametrize("combine", COMBINES)
def test_packedcsc_semaphores_on_the_general_path(dsa, hip, oracle, combine):
    """build.hip:k_emit_sems_wide (emit_wide, mode 2): row keys spanning more than 2^56 need 57 bits, 257 partitions 9 bits — 66 > 64,
    the general path of build.hip:build_prepare; 257 partitions are two blocks of k_emit_sems_wide"""
    nparts, lo, hi = 257, -(1 << 55) - 3, (1 << 55) + 11
    assert hi - lo > 1 << 56 and bit_width(hi - lo) + bit_width(nparts - 1) == 66
    g = np.random.default_rng(81)
    for kind in ("edges", "one"):
        rows, vals = pcsc_input(g, pcsc_lens(g, nparts, kind, 4), lo, hi, combine)
        check_pcsc(dsa, hip, oracle, rows, vals, combine)


@pytest.mark.parametrize("combine", COMBINES)
def test_packedcsc_semaphores_on_the_payload_path(dsa, hip, oracle, combine):
    """build.hip:build_prepare `s.ibits = 0` in mode 2: 30 000 entries (15 index bits), row keys spanning about 2^50 (50 bits) and 600
    partitions (10 bits) are 75 bits with the index, 60 without — one composite, values sorted as payload; k_emit_sems shifts by
    ibits = 0"""
    nparts, lo, hi, nnz = 600, -(1 << 49), (1 << 49) - 7, 30000
    g = np.random.default_rng(82)
    lens = pcsc_lens(g, nparts, "edges", 4)
    live = np.flatnonzero(lens)
    lens[live] = nnz // len(live)
    lens[live[0]] += nnz - lens.sum()
    kbits, pbits, ibits = bit_width(hi - lo), bit_width(nparts - 1), bit_width(nnz - 1)
    assert lens.sum() == nnz and (kbits, pbits, ibits) == (50, 10, 15) and kbits + pbits <= 64 < kbits + pbits + ibits
    rows, vals = pcsc_input(g, lens, lo, hi, combine)
    check_pcsc(dsa, hip, oracle, rows, vals, combine)


# ------------------------------------------------------------------------------------------------------------------------------------
# 9. the fill buffer's running key ranges across uploaded pieces
# ------------------------------------------------------------------------------------------------------------------------------------
FILL_PIECE = 1 << 18          # host.h:FillBuffer::PIECE


@pytest.mark.parametrize("extremes", ["last_batch", "first_batch"])
def test_fill_mode_key_ranges_across_pieces(dsa, hip, oracle, extremes):
    """fill_host.hip:fill_upload_chunk folds every uploaded piece (host.h:FillBuffer::PIECE = 2^18 triples, EAGER = 2^16) into the
    running ranges with build.hip:k_minmax_acc, and fill_host.hip:fill_drain hands them to the build as the composite's kmin / pmin and
    bit counts.  2^18 + 5 triples are one full piece and a rest that stays staged; the only negative row and the only column above
    2^33 arrive either in the last batch (a range that stops at an earlier piece loses them) or in the first piece only (a range of
    the last piece alone loses them) — either way `key - kmin` would spill into the partition bits without any error."""
    n1 = FILL_PIECE + 5
    I1, J1, V1 = gen_triples(90, n1, (1, 2000), (1, 2000))
    g = np.random.default_rng(91)
    I4, J4, V4 = ranged(g, 100, 1, 2000), ranged(g, 100, 1, 2000), mixed_values(g, 100)
    far_row, far_col = -5, (1 << 33) + 9
    if extremes == "last_batch":
        I4[40], J4[60] = far_row, far_col
    else:
        I1[10], J1[FILL_PIECE - 20] = far_row, far_col
    singles = [(int(I1[t]), int(J1[t]), float(v)) for t, v in zip(g.integers(0, n1, 20), mixed_values(g, 20))]      # cells of batch 1 again
    row_cols, row_vals = np.array([7, 1999, 3, 400]), np.array([1.5, -2.5, 1e10, 1e-3])
    mats = []
    for bnd in (hip, oracle):
        m = dsa.dynamicsparse(fill_mode=True, binding=bnd)
        m.set_batch(I1, J1, V1)
        m.addrow(2001, row_cols, row_vals)
        for i, j, v in singles:
            m[i, j] = v
        m.set_batch(I4, J4, V4)
        m.closefillmode()
        mats.append(m)
    a, b = mats
    assert_mat_equal(a, b)
    I = np.concatenate([I1, np.full(4, 2001), [s[0] for s in singles], I4])
    J = np.concatenate([J1, row_cols, [s[1] for s in singles], J4])
    V = np.concatenate([V1, row_vals, [s[2] for s in singles], V4])
    assert len(I) >= TWIN_MIN and I.min() == far_row and J.max() == far_col
    assert (I < 0).sum() == 1 and (J > 1 << 33).sum() == 1
    assert_matrix_is_fold(a, I, J, V)
    assert clean(a.check(0)) and clean(a.check(1))


# ------------------------------------------------------------------------------------------------------------------------------------
# 10. the scan kernels' items-per-thread switch
# ------------------------------------------------------------------------------------------------------------------------------------
def test_scan_items_per_thread_switch(dsa, hip, oracle):
    """build.hip:k_rs_scan `ipt = (nblocks + RS_BLOCK - 1) / RS_BLOCK`: 256 * 4096 + 1 triples are 257 tiles, the first size at which
    a thread of the histogram scan owns two tiles (and the last threads none)"""
    nnz = 256 * TILE + 1
    assert (nnz + TILE - 1) // TILE == 257
    I, J, V = gen_triples(10, nnz, (1, 299), (1, 69999))
    check_matrix(dsa, hip, oracle, I, J, V)


# ------------------------------------------------------------------------------------------------------------------------------------
# which path ran
# ------------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import dsa_loader
import test_kbuild_edges as T
dsa = dsa_loader.load(); hip = dsa.product()
for name, (I, J, V) in T.path_cases():
    sys.stderr.write("\nCASE %s %d\n" % (name, len(I))); sys.stderr.flush()
    dsa.dynamicsparse(I, J, V, binding=hip).close()
sys.stderr.write("\nCASE end 0\n"); sys.stderr.flush()
print("ok")
"""


def test_mat_build_major_reports_the_intended_path(dsa, hip):
    """matwrite_host.hip:mat_build_major_dev prints which way it went under DSA_DEV=1 DSA_DBG_TIME=1: `twin derived` from 65536 triples
    on (cases 1 and 2), two orientations timed side by side below, `general path` for the 65-bit composite of case 4.  If the
    threshold or a bit-width switch moves, this test says so and the cases above have to move with it."""
    env = dict(os.environ, DSA_DEV="1", DSA_DBG_TIME="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = (int(line.split()[2]), [])
        elif name is not None and line.startswith("[mat_build_major] nnz="):
            seen[name][1].append(line)
    expect = {"twin_65535": "colmajor", "twin_65536": "(twin derived)", "boundary_65536": "(twin derived)",
              "boundary_65537": "(twin derived)", "general_65536": "(general path)", "general_30000": "colmajor"}
    for case, word in expect.items():
        nnz, lines = seen[case]
        assert len(lines) == 1 and lines[0].startswith("[mat_build_major] nnz=%d " % nnz), (case, lines)
        assert word in lines[0], (case, lines)
        if word == "colmajor":
            assert "rowmajor" in lines[0] and "both orientations" not in lines[0], (case, lines)
