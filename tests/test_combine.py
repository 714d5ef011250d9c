"""Combine on the device (include/dsa.h: dsa_mat_combine; csrc/combine.hip): alpha * A + beta * shift(B) as a new matrix, and what is
built on it: copy, +, -, unary -, scalar *, hcat, vcat, blockdiag.

Expected matrices never come from the library under test.  `_triples` walks the ORACLE's exported colmajor layout of an operand in
slot order (the findnz order) to (i, j, v); `_expected` scales and shifts in numpy (one IEEE multiply per cell, as on the device),
concatenates and hands the list to the oracle's dynamicsparse(I, J, V, m, n).  Both orientations are then compared slot for slot
(assert_mat_equal); values are bit-equal, except that a NaN matches any NaN (0 * Inf carries the other sign bit on the device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _expect, _in_fill_mode, _in_size
from test_hip_parity import assert_mat_equal
from util import MAT_INFO_KEYS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
EARG, EBOUNDS, EMODE, EKEY = 1, 2, 5, 9
TILE = 2048               # slots per wave of the combine pass (csrc/export_dev.h: EX_TILE_SHIFT)
I64_MAX = (1 << 63) - 1
LAYOUT_ARRAYS = ("keys", "vals", "occ", "semaphores", "col_keys", "col_live")


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_combine_symbol_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    assert re.search(r"\bdsa_mat_combine\s*\(", hdr)
    assert "mat_combine" in dsa.Binding.declared_symbols()
    assert hasattr(lib, "dsa_mat_combine")
    jl = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "julia", "DynamicSparseArraysAMD.jl")).read()
    assert ":dsa_mat_combine" in jl
    for method in ("Base.copy(", "Base.:+(", "Base.:-(", "Base.:*(", "Base.hcat(", "Base.vcat(", "SparseArrays.blockdiag("):
        assert method in jl, method
    hdr = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "export_dev.h")).read()
    assert 1 << int(re.search(r"EX_TILE_SHIFT\s*=\s*(\d+)", hdr).group(1)) == TILE


def test_combine_python_names_are_callable(dsa):
    for name in ("hcat", "vcat", "blockdiag"):
        assert callable(getattr(dsa, name)), name
    for name in ("combine", "copy", "__add__", "__sub__", "__neg__", "__mul__", "__rmul__"):
        assert callable(getattr(dsa.DynamicSparseMatrix, name)), name


def test_combine_needs_the_product_library(dsa, oracle):
    assert not oracle.has("mat_combine")
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    for call in (a.copy, a.combine, lambda: a + a, lambda: a - a, lambda: -a, lambda: 2.0 * a, lambda: a * 2.0,
                 lambda: dsa.hcat(a, a), lambda: dsa.vcat(a, a), lambda: dsa.blockdiag(a, a)):
        with pytest.raises(dsa.DsaArgumentError, match="needs the HIP product library"):
            call()


def test_golden_set_is_large_enough_for_both_groups(dsa, oracle):
    """what test_golden_scenarios asserts about its own coverage, shown on the oracle: at least half of MATRIX_CASES end out of fill
    mode (the unshifted forms), and at least half end with every cell inside size() (the shifted forms)"""
    plain = shifted = 0
    for sc in MATRIX_CASES:
        b = run_scenario(dsa, oracle, sc)
        if _in_fill_mode(dsa, b):
            continue
        plain += 1
        shifted += _all_inside(b)
    assert 2 * plain >= len(MATRIX_CASES) and 2 * shifted >= len(MATRIX_CASES), (plain, shifted, len(MATRIX_CASES))


# ---------------------------------------------------------------------------------------------------------------- helpers
def _all_inside(b):
    m, n = b.size()
    return _in_size(_expect(b, COLMAJOR), m) and _in_size(_expect(b, ROWMAJOR), n)


def _triples(ora):
    """(I, J, V) of the stored cells of an oracle matrix in the slot order of its colmajor orientation"""
    L = ora.export_layout(COLMAJOR)
    occ = L["occ"].astype(bool)
    keys, vals = L["keys"][occ], L["vals"][occ]
    if len(keys) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    is_sem = keys == 0
    assert is_sem[0], "a cell in front of the first semaphore"
    pid = vals[is_sem].astype(np.int64)                     # semaphore value = partition id (1-based)
    part = pid[np.cumsum(is_sem) - 1]
    cell = ~is_sem
    return keys[cell].astype(np.int64), L["col_keys"][part[cell] - 1].astype(np.int64), vals[cell].copy()


def _expected(dsa, oracle, A, alpha=1.0, B=None, beta=1.0, row_off=0, col_off=0, m=None, n=None):
    """the oracle's dynamicsparse of the scaled, shifted, concatenated triples; A / B are ORACLE matrices"""
    I, J, V = _triples(A)
    with np.errstate(invalid="ignore"):                    # (0 * Inf)
        V = alpha * V
    ma, na = A.size()
    if B is not None:
        Ib, Jb, Vb = _triples(B)
        with np.errstate(invalid="ignore"):
            Vb = beta * Vb
        I, J, V = np.concatenate((I, Ib + row_off)), np.concatenate((J, Jb + col_off)), np.concatenate((V, Vb))
        mb, nb = B.size()
        ma, na = max(ma, mb + row_off), max(na, nb + col_off)
    return dsa.dynamicsparse(I, J, V, ma if m is None else m, na if n is None else n, binding=oracle)


def _same(got, ref):
    """assert_mat_equal; with NaNs in the expected values the same checks, a NaN matching any NaN"""
    nan = any(np.isnan(ref.export_layout(o)["vals"][ref.export_layout(o)["occ"].astype(bool)]).any() for o in (0, 1))
    if not nan:
        assert_mat_equal(got, ref)
        return
    assert got.size() == ref.size()
    for o in (0, 1):
        La, Lb = got.export_layout(o), ref.export_layout(o)
        for k in MAT_INFO_KEYS:
            assert La["info"][k] == Lb["info"][k], (o, k)
        for k in ("occ", "semaphores", "col_keys", "col_live"):
            assert np.array_equal(La[k], Lb[k]), (o, k)
        occ = La["occ"].astype(bool)
        assert np.array_equal(La["keys"][occ], Lb["keys"][occ]), o
        va, vb = La["vals"][occ], Lb["vals"][occ]
        both = np.isnan(va) & np.isnan(vb)
        assert np.array_equal(va[~both].view(np.uint64), vb[~both].view(np.uint64)), o


def _pair(dsa, hip, oracle, I, J, V, m=None, n=None, then=None):
    """the same matrix on the HIP library and on the oracle; `then(x)` is applied to both"""
    out = []
    for b in (hip, oracle):
        x = dsa.dynamicsparse(np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64), np.asarray(V, dtype=np.float64), m, n, binding=b)
        if then is not None:
            then(x)
        out.append(x)
    return out


def _columns(lens, scale=1.0):
    """columns 1 .. len(lens), column j holding rows 1 .. lens[j - 1]; distinct values"""
    I = np.concatenate([np.arange(1, l + 1) for l in lens]).astype(np.int64)
    J = np.repeat(np.arange(1, len(lens) + 1), lens).astype(np.int64)
    return I, J, scale * np.arange(1, len(I) + 1, dtype=np.float64)


def _sem_slots(a):
    """0-based slots of the live semaphores of the colmajor orientation, ascending, and its capacity"""
    L = a.export_layout(COLMAJOR)
    s = L["semaphores"]
    return np.sort(s[s != 0] - 1), L["info"]["capacity"]


def _snapshot(a):
    return [a.export_layout(o) for o in (0, 1)]


def _unchanged(a, before):
    for o in (0, 1):
        after = a.export_layout(o)
        assert after["info"] == before[o]["info"], o
        for k in LAYOUT_ARRAYS:
            assert np.array_equal(after[k].view(np.uint8), before[o][k].view(np.uint8)), (o, k)


def _check_plain(dsa, oracle, a, b, a2, b2):
    """every unshifted form of (a, a2), matrices on the HIP library; b, b2 are their oracle twins"""
    _same(a.copy(), _expected(dsa, oracle, b))
    _same(2.5 * a, _expected(dsa, oracle, b, 2.5))
    _same(a + a, _expected(dsa, oracle, b, 1.0, b, 1.0))
    z = a - a
    _same(z, _expected(dsa, oracle, b, 1.0, b, -1.0))
    assert z.nnz() == a.nnz()
    L = z.export_layout(COLMAJOR)
    cells = L["occ"].astype(bool) & (L["keys"] != 0)
    assert cells.sum() == a.nnz() and not np.any(L["vals"][cells])              # every cell a stored zero
    _same(a + a2, _expected(dsa, oracle, b, 1.0, b2, 1.0))


def _check_shifted(dsa, oracle, a, b, a2, b2):
    """hcat / vcat / blockdiag of (a, a2), both inside their size; m / n padded through the explicit m, n where they differ"""
    (ma, na), (mb, nb) = b.size(), b2.size()
    _same(a.combine(a2, col_off=na, m=max(ma, mb)), _expected(dsa, oracle, b, 1.0, b2, 1.0, 0, na, m=max(ma, mb)))
    _same(a.combine(a2, row_off=ma, n=max(na, nb)), _expected(dsa, oracle, b, 1.0, b2, 1.0, ma, 0, n=max(na, nb)))
    _same(dsa.blockdiag(a, a2), _expected(dsa, oracle, b, 1.0, b2, 1.0, ma, na))
    if ma == mb:
        _same(dsa.hcat(a, a2), _expected(dsa, oracle, b, 1.0, b2, 1.0, 0, na))
    if na == nb:
        _same(dsa.vcat(a, a2), _expected(dsa, oracle, b, 1.0, b2, 1.0, ma, 0))


def _check_forms(dsa, oracle, a, b, a2, b2):
    _check_plain(dsa, oracle, a, b, a2, b2)
    _check_shifted(dsa, oracle, a, b, a2, b2)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_golden_scenarios(dsa, hip, oracle):
    """every golden matrix scenario out of fill mode: copy, 2.5 * A, A + A, A - A, A + (the next scenario); those with every cell inside
    size() also hcat / vcat / blockdiag with the next such scenario, m / n padded through the explicit m, n.  14 scenarios, none in
    fill mode at its end, 12 inside their size (test_golden_set_is_large_enough_for_both_groups)."""
    pairs = []
    for sc in MATRIX_CASES:
        b = run_scenario(dsa, oracle, sc)
        if _in_fill_mode(dsa, b):
            continue
        pairs.append((run_scenario(dsa, hip, sc), b, _all_inside(b)))
    inside = [p for p in pairs if p[2]]
    assert 2 * len(pairs) >= len(MATRIX_CASES) and 2 * len(inside) >= len(MATRIX_CASES), (len(pairs), len(inside))
    for k, (a, b, ins) in enumerate(pairs):
        a2, b2, _ = pairs[(k + 1) % len(pairs)]
        _check_plain(dsa, oracle, a, b, a2, b2)
    for k, (a, b, _) in enumerate(inside):
        a2, b2, _ = inside[(k + 1) % len(inside)]
        _check_shifted(dsa, oracle, a, b, a2, b2)


# lens of the columns of the tile-edge matrices; the conditions are asserted from the layout of the matrix under test
TILE_SHAPES = {
    "below_one_tile": [3, 40, 1, 17],                       # capacity < 2048
    "column_over_three_tiles": [3, 5000, 4],                # semaphores in tiles 0, 0, 3: tiles 1 and 2 take their owner from the carry
    "semaphores_on_tile_edges": [1599, 799, 800],           # semaphores in slots 1, 4096 (first of tile 2) and 6143 (last of tile 2)
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(TILE_SHAPES))
def test_tile_edges(dsa, hip, oracle, shape):
    a, b = _pair(dsa, hip, oracle, *_columns(TILE_SHAPES[shape]))
    a2, b2 = _pair(dsa, hip, oracle, *_columns([5, 0, 7, 2], scale=-0.5))
    sems, cap = _sem_slots(a)
    tiles = sems // TILE
    if shape == "below_one_tile":
        assert cap < TILE
    elif shape == "column_over_three_tiles":
        gaps = np.nonzero(np.diff(tiles) >= 3)[0]
        assert len(gaps) > 0                                 # two tiles without a semaphore between this column's and the next one's
        occ = a.export_layout(COLMAJOR)["occ"]
        t = int(tiles[gaps[0]]) + 1
        assert occ[t * TILE:(t + 1) * TILE].any() and occ[(t + 1) * TILE:(t + 2) * TILE].any()
    else:
        assert np.any(sems % TILE == TILE - 1) and np.any((sems % TILE == 0) & (sems > 0))
    _check_forms(dsa, oracle, a, b, a2, b2)
    _check_forms(dsa, oracle, a2, b2, a, b)


@pytest.mark.gpu
def test_tables_with_tombstones_and_empty_columns(dsa, hip, oracle):
    I, J, V = _columns([4, 6, 3, 5, 2, 7])
    other = _pair(dsa, hip, oracle, *_columns([2, 2, 9], scale=0.25))

    def drop_middle_and_last(x):
        x.deletecolumn(3)
        x.deletecolumn(6)
    a, b = _pair(dsa, hip, oracle, I, J, V, then=drop_middle_and_last)
    L = a.export_layout(COLMAJOR)
    assert L["info"]["table_len"] == 6 and L["semaphores"][2] == 0 and L["semaphores"][5] == 0       # tombstones, one at the end
    _check_forms(dsa, oracle, a, b, other[0], other[1])
    _check_forms(dsa, oracle, other[0], other[1], a, b)

    # an emptied but live column: droptol of all its cells (on the oracle: each of them set to 0)
    a, b = _pair(dsa, hip, oracle, I, J, np.where(J == 4, 1e-9, V))
    assert a.droptol(1e-6) == 5
    for i in range(1, 6):
        b[i, 4] = 0.0
    L = a.export_layout(COLMAJOR)
    s4 = L["semaphores"][3]
    assert s4 != 0 and L["col_live"][3] != 0
    nxt = s4 + np.nonzero(L["occ"][s4:])[0][0]               # the next occupied slot behind column 4's semaphore: another semaphore
    assert L["keys"][nxt] == 0
    assert np.array_equal(np.stack(a.findnz()[:2]), np.stack(_triples(b)[:2]))
    _check_forms(dsa, oracle, a, b, other[0], other[1])
    _check_forms(dsa, oracle, other[0], other[1], a, b)


@pytest.mark.gpu
def test_empty_operands_and_no_second_operand(dsa, hip, oracle):
    a, b = _pair(dsa, hip, oracle, *_columns([4, 6, 3]))
    e, eb = _pair(dsa, hip, oracle, [], [], [], 3, 2)
    assert e.nnz() == 0
    _same(a + e, _expected(dsa, oracle, b, 1.0, eb))
    _same(e + a, _expected(dsa, oracle, eb, 1.0, b))
    _same(e + e, _expected(dsa, oracle, eb, 1.0, eb))
    _same(e.copy(), _expected(dsa, oracle, eb))
    _same(dsa.blockdiag(e, a), _expected(dsa, oracle, eb, 1.0, b, 1.0, 3, 2))
    _same(dsa.blockdiag(e, e), _expected(dsa, oracle, eb, 1.0, eb, 1.0, 3, 2))
    assert dsa.blockdiag(e, e).size() == (6, 4)
    for x in (a.combine(None, alpha=-3.0), a.combine(alpha=-3.0, beta=7.0, row_off=5, col_off=9)):       # without b the rest is ignored
        _same(x, _expected(dsa, oracle, b, -3.0))
    _same(-a, _expected(dsa, oracle, b, -1.0))
    _same(a * 4, _expected(dsa, oracle, b, 4.0))
    # stored zeros of an operand stay stored; Inf * 0 is a NaN on both sides
    z, zb = _pair(dsa, hip, oracle, [1, 2, 2, 3], [1, 2, 2, 1], [0.0, 1.5, -1.5, np.inf])
    assert z.nnz() == 3
    _same(z.copy(), _expected(dsa, oracle, zb))
    _same(0.0 * z, _expected(dsa, oracle, zb, 0.0))
    _same(z - z, _expected(dsa, oracle, zb, 1.0, zb, -1.0))


@pytest.mark.gpu
def test_wide_and_negative_keys(dsa, hip, oracle):
    big = (1 << 40) + 5
    w, wb = _pair(dsa, hip, oracle, [1, big, 7, 2, big], [1, 1, 3, big, big], [1.5, -2.0, 3.25, 4.0, 0.125])
    n_, nb = _pair(dsa, hip, oracle, *_columns([4, 6, 3]))
    assert w.size() == (big, big)
    _same(w.copy(), _expected(dsa, oracle, wb))
    _same(w + n_, _expected(dsa, oracle, wb, 1.0, nb))
    _same(n_ - w, _expected(dsa, oracle, nb, 1.0, wb, -1.0))
    _same(dsa.blockdiag(n_, w), _expected(dsa, oracle, nb, 1.0, wb, 1.0, 6, 3))
    _same(n_.combine(w, row_off=1 << 41), _expected(dsa, oracle, nb, 1.0, wb, 1.0, 1 << 41, 0))        # narrow keys shifted into wide ones
    # negative and out-of-size keys, zero offsets: nothing is bounds-checked
    g, gb = _pair(dsa, hip, oracle, [-3, 2, 5, -1, 9], [1, -2, -2, 4, 4], [1.0, 2.0, 3.0, 4.0, 5.0], 4, 3)
    assert g.size() == (4, 3)
    _same(g.copy(), _expected(dsa, oracle, gb))
    _same(g + n_, _expected(dsa, oracle, gb, 1.0, nb))
    _same(n_.combine(g, beta=0.5, m=2, n=2), _expected(dsa, oracle, nb, 1.0, gb, 0.5, m=2, n=2))       # m, n below the key range


@pytest.mark.gpu
def test_errors_leave_operands_and_out_untouched(dsa, hip, oracle):
    a, b = _pair(dsa, hip, oracle, *_columns([4, 6, 3]))                       # 6 x 3
    c, cb = _pair(dsa, hip, oracle, [3, 1, 5], [1, 2, 2], [1.0, 2.0, 3.0])     # 5 x 2, holds row key 3
    out_a, _ = _pair(dsa, hip, oracle, [1, 2, 9], [1, 7, 2], [1.0, 2.0, 3.0], 9, 4)      # column 7 beyond n = 4
    out_r, _ = _pair(dsa, hip, oracle, [1, 8, 2], [1, 2, 3], [1.0, 2.0, 3.0], 5, 3)      # row 8 beyond m = 5
    fill = dsa.dynamicsparse(fill_mode=True, binding=hip)

    def raw(x, y, row_off=0, col_off=0, m=-1, n=-1):
        h = C.c_void_p(0xdead)
        rc = hip._mat_combine(x.h, 1.0, None if y is None else y.h, 1.0, row_off, col_off, m, n, C.byref(h))
        assert rc == 0 or h.value == 0xdead                  # *out is untouched on an error
        if rc == 0:
            dsa.DynamicSparseMatrix(hip, h).close()
        return rc

    def good():
        _same(a + c, _expected(dsa, oracle, b, 1.0, cb))
        _same(dsa.blockdiag(a, c), _expected(dsa, oracle, b, 1.0, cb, 1.0, 6, 3))

    cases = [
        (EKEY, a, c, dict(row_off=-3)),                       # row key 3 of c -> 0
        (EKEY, a, c, dict(col_off=-2)),                       # column key 2 of c -> 0
        (EBOUNDS, out_a, c, dict(col_off=4)),                 # a holds a column beyond its n
        (EBOUNDS, a, out_a, dict(col_off=3)),                 # b does
        (EBOUNDS, out_r, c, dict(row_off=5)),                 # the same for rows
        (EBOUNDS, a, out_r, dict(row_off=6)),
        (EARG, a, c, dict(row_off=I64_MAX - 2, m=10, n=10)),  # 3 + off leaves int64
        (EARG, a, c, dict(col_off=I64_MAX, m=10, n=10)),
        (EARG, a, c, dict(row_off=I64_MAX - 2)),              # ... and so does the default m
        (EMODE, fill, a, {}),
        (EMODE, a, fill, {}),
        (EMODE, fill, None, {}),
    ]
    good()
    for code, x, y, kw in cases:
        before = [(z, _snapshot(z)) for z in (x, y) if z is not None and z is not fill]
        assert raw(x, y, **kw) == code, (code, kw)
        for z, snap in before:
            _unchanged(z, snap)
        good()
    assert raw(out_a, c) == 0 and raw(a, out_r) == 0          # the same operands with zero offsets: nothing is bounds-checked
    with pytest.raises(dsa.DsaArgumentError) as ei:
        a.combine(c, row_off=-3)
    assert ei.value.code == EKEY
    with pytest.raises(dsa.DsaBoundsError):
        dsa.hcat(out_a, out_a)
    with pytest.raises(dsa.DsaErrorException) as ei:
        fill.copy()
    assert ei.value.code == EMODE
    good()


@pytest.mark.gpu
def test_operands_are_only_read_and_results_repeat(dsa, hip, oracle):
    """the smallest shape the SpMV plan applies to (x beyond 3 MB, as in test_spmv_plan; ~1200 tiles, the builder's twin-build path): the
    cached plan of `a` survives copy and A + A, the layouts of `a` keep their bytes, and two calls give the same bits"""
    rng = np.random.default_rng(17)
    m = n = 420_000
    nnz = 1_260_000
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.random(nnz) + 0.5
    a, b = _pair(dsa, hip, oracle, I, J, V)
    x = rng.random(n) + 0.5
    for _ in range(3):
        a.mul(x)                                             # the plan is built on the second product
    y0 = a.mul(x)
    before, info0 = _snapshot(a), [a.info(o) for o in (0, 1)]
    assert info0[ROWMAJOR]["stat_spmv_plan"] > 0 and info0[ROWMAJOR]["stat_spmv_plan_builds"] == 1
    c1, c2, s1 = a.copy(), a.copy(), a + a
    ref = _expected(dsa, oracle, b)
    _same(c1, ref)
    assert s1.nnz() == c1.nnz() == ref.nnz()
    for o in (0, 1):
        L1, L2 = c1.export_layout(o), c2.export_layout(o)
        for k in LAYOUT_ARRAYS:
            assert np.array_equal(L1[k].view(np.uint8), L2[k].view(np.uint8)), (o, k)
    _unchanged(a, before)
    assert [a.info(o) for o in (0, 1)] == info0              # no plan build, no rebalance, no product counted
    y1 = a.mul(x)
    i1 = a.info(ROWMAJOR)
    assert i1["stat_spmv_plan_builds"] == 1 and i1["stat_spmv_plan"] == info0[ROWMAJOR]["stat_spmv_plan"] + 1
    assert np.array_equal(np.asarray(y1).view(np.uint64), np.asarray(y0).view(np.uint64))
    # 2 * a and a + a hold the same bits (x + x == 2 x in IEEE), in the same slots
    d1 = 2.0 * a
    for o in (0, 1):
        L1, L2 = s1.export_layout(o), d1.export_layout(o)
        for k in LAYOUT_ARRAYS:
            assert np.array_equal(L1[k].view(np.uint8), L2[k].view(np.uint8)), (o, k)


@pytest.mark.gpu
def test_size_arithmetic(dsa, hip, oracle):
    a, b = _pair(dsa, hip, oracle, *_columns([4, 6, 3]), 8, 5)                 # 8 x 5
    c, cb = _pair(dsa, hip, oracle, *_columns([2, 7], scale=2.0), 8, 2)        # 8 x 2
    d, db = _pair(dsa, hip, oracle, *_columns([1, 2, 3, 4, 5], scale=3.0), 6, 5)       # 6 x 5
    assert dsa.hcat(a, c).size() == (8, 7)
    _same(dsa.hcat(a, c), _expected(dsa, oracle, b, 1.0, cb, 1.0, 0, 5))
    assert dsa.vcat(a, d).size() == (14, 5)
    _same(dsa.vcat(a, d), _expected(dsa, oracle, b, 1.0, db, 1.0, 8, 0))
    assert dsa.blockdiag(a, c).size() == (16, 7)
    _same(dsa.blockdiag(a, c), _expected(dsa, oracle, b, 1.0, cb, 1.0, 8, 5))
    assert (d + a).size() == (8, 5) and (a - d).size() == (8, 5) and (2 * d).size() == (6, 5) and d.copy().size() == (6, 5)
    s = a.combine(d, m=3, n=2)                                # smaller than the key range: allowed, as in dynamicsparse
    assert s.size() == (3, 2)
    _same(s, _expected(dsa, oracle, b, 1.0, db, 1.0, m=3, n=2))
    calls = []
    real = hip._mat_combine
    hip._mat_combine = lambda *args: calls.append(args) or real(*args)
    try:
        with pytest.raises(dsa.DsaArgumentError):
            dsa.hcat(a, d)                                    # 8 and 6 rows
        with pytest.raises(dsa.DsaArgumentError):
            dsa.vcat(a, c)                                    # 5 and 2 columns
    finally:
        hip._mat_combine = real
    assert calls == []
