"""The batched sparse-x product Y = A S / A' S (include/dsa.h: dsa_mat_spgemm_csc[_dev]; csrc/spgemm.hip, csrc/spgemm_host.hip).

Expected values never come from the library.  Column j of Y is `model_mul` of tests/test_sparse_x.py (a numpy walk over the ORACLE's
exported layout, products added in slot order from +0.0) on column j of S; the CPU half shows that this helper and the oracle's own
mul((xi, xv), transpose) agree bit for bit on every input the GPU half uses.  Values of A and S are standard normal, so a wrong
summation order shows.  Every comparison is bitwise (uint64 views) and there is no tolerance anywhere; the one exception is the payload
of a NaN, which IEEE 754 leaves open (0 * Inf gives another sign bit on the host than on the device): a NaN matches a NaN.

A CASE is a function of mk(I, J, V, m, n) -> matrix that returns a list of (matrix, columns, transpose, pick): columns = [(xi, xv)]
with 1-based ascending keys, pick = None or the indices of the columns S is made of (k = 65537 columns out of 50 distinct ones).
Outputs are pre-filled with a sentinel; nothing beyond `total` may change.  The edges follow the four constants of csrc/spgemm.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _in_fill_mode
from test_sparse_x import model_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLMAJOR, ROWMAJOR = 0, 1
EARG, EBOUNDS, EMODE, EASSERT, ECAP = 1, 2, 5, 6, 8
NAMES = ("mat_spgemm_csc", "mat_spgemm_csc_dev")

with open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "spgemm.h")) as _f:
    _H = _f.read()
SPG = {name: int(re.search(r"constexpr\s+int64_t\s+" + name + r"\s*=\s*(\d+)\s*;", _H).group(1))
       for name in ("SPG_SMALL_MAX", "SPG_TABLE_SLOTS", "SPG_MAX_SLABS", "SPG_SLAB_BYTES_MAX")}
SMALL, SLOTS, MAX_SLABS = SPG["SPG_SMALL_MAX"], SPG["SPG_TABLE_SLOTS"], SPG["SPG_MAX_SLABS"]


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


# ---- the expected CSC ---------------------------------------------------------------------------------------------------------------
def csc_of(cols, pick=None):
    """0-based CSC arrays (xptr, xidx, xval) of the columns [(xi, xv)] (1-based keys), in the order of `pick`"""
    order = range(len(cols)) if pick is None else pick
    if len(cols) == 0 or len(order) == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    lens = np.array([len(cols[j][0]) for j in range(len(cols))], dtype=np.int64)
    order = np.asarray(list(order), dtype=np.int64)
    ptr = np.concatenate(([0], np.cumsum(lens[order]))).astype(np.int64)
    idx = np.concatenate([i64(cols[j][0]) - 1 for j in order]) if ptr[-1] else np.zeros(0, dtype=np.int64)
    val = np.concatenate([np.asarray(cols[j][1], dtype=np.float64) for j in order]) if ptr[-1] else np.zeros(0)
    return ptr, i64(idx), np.ascontiguousarray(val, dtype=np.float64)


def expected_csc(L, cols, pick=None):
    """(ptr, idx, val) of Y, 0-based, from the oracle's layout `L` of the walked orientation: model_mul per column"""
    per = [model_mul(L, i64(xi), np.asarray(xv, dtype=np.float64))[:2] for xi, xv in cols]
    return csc_of([(r, v) for r, v in per], pick)


def in_size(exp, ny):
    return bool(np.all((exp[1] >= 0) & (exp[1] < ny)))


def same_bits(got, exp):
    g, e = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    return g.shape == e.shape and bool(np.all((g.view(np.uint64) == e.view(np.uint64)) | (np.isnan(g) & np.isnan(e))))


def assert_same(got, exp, base, what):
    assert np.array_equal(np.asarray(got[0], dtype=np.int64), exp[0] + base), what
    assert np.array_equal(np.asarray(got[1], dtype=np.int64), exp[1] + base), what
    assert same_bits(got[2], exp[2]), what


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------
def normal_matrix(seed, m, n, cnt):
    rng = np.random.default_rng(seed)
    IJ = np.unique(np.stack([rng.integers(1, m + 1, cnt), rng.integers(1, n + 1, cnt)], axis=1), axis=0)
    return i64(IJ[:, 0]), i64(IJ[:, 1]), rng.standard_normal(len(IJ))


def random_columns(seed, dim, k, per):
    """k columns of up to `per` keys out of 1..dim + 5 (inside and beyond the size), standard-normal values, a stored zero in every
    third column, an empty column in the middle"""
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(k):
        cnt = 0 if j == k // 2 else int(rng.integers(1, per + 1))
        xi = np.unique(rng.integers(1, dim + 6, cnt)) if cnt else np.zeros(0, dtype=np.int64)
        xv = rng.standard_normal(len(xi))
        if j % 3 == 0 and len(xv):
            xv[len(xv) // 2] = 0.0
        cols.append((i64(xi), xv))
    return cols


def column_matrix(seed, m, lens):
    """an m-row matrix whose column c (1-based) holds lens[c - 1] cells in random rows, standard-normal values"""
    rng = np.random.default_rng(seed)
    I = np.concatenate([np.sort(rng.choice(m, size=c, replace=False)) + 1 for c in lens])
    J = np.concatenate([np.full(c, j + 1) for j, c in enumerate(lens)])
    return i64(I), i64(J), rng.standard_normal(len(I)), m, len(lens)


def nrm(seed, n):
    return np.random.default_rng(seed).standard_normal(n)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def both(mk, I, J, V, m, n, cols, pick=None):
    """the case on the colmajor orientation (A, transpose = 0) and, with rows and columns swapped, on the rowmajor one (A', transpose = 1):
    the same partitions, the same columns of S"""
    return [(mk(I, J, V, m, n), cols, False, pick), (mk(J, I, V, n, m), cols, True, pick)]


def c_degenerate(mk):
    m, n = 200, 150
    I, J, V = normal_matrix(11, m, n, 1500)
    keep = J != 9                                                    # column 9 is never written
    a = mk(I[keep], J[keep], V[keep], m, n)
    a.deletecolumn(7)
    e = (np.zeros(0, dtype=np.int64), np.zeros(0))
    some = (i64([3, 20, 21, 150]), nrm(1, 4))
    cols_sets = [[],                                                  # k = 0
                 [e, e, e],                                           # nnzx = 0
                 [e, some, e, e, (i64([5]), nrm(2, 1)), e],           # empty columns between the others
                 [(i64([9, n + 1, n + 2, n + 400]), nrm(3, 4)), some],  # no key of the column has a partition
                 [(i64([7]), nrm(4, 1)), (i64([6, 7, 8]), nrm(5, 3))]]  # a deleted column alone and between two live ones
    out = [(a, cols, False, None) for cols in cols_sets]
    rows = [(i64([2, 3, 199, 200, 201]), nrm(6, 5)), e, (i64([m + 7]), nrm(7, 1))]
    return out + [(a, rows, True, None)]


def nonfinite_matrix():
    """6 x 8: rows 2 and 3 hold nothing but +Inf / NaN in column 5; finite cells elsewhere"""
    I = i64([1, 4, 5, 6, 1, 4, 2, 3, 5, 6, 1])
    J = i64([1, 1, 2, 2, 3, 3, 5, 5, 6, 7, 8])
    V = nrm(21, len(I))
    V[6], V[7] = np.inf, np.nan
    return I, J, V, 6, 8


def c_nonfinite(mk):
    a = mk(*nonfinite_matrix())
    cols = [(i64([1, 5]), np.array([1.5, 0.0])),                    # Inf / NaN under a stored zero: NaN in rows 2 and 3
            (i64([1, 5, 6]), np.array([1.5, 2.0, -1.0])),           # under a stored value: Inf and NaN
            (i64([1, 2, 3, 6]), nrm(22, 4)),                        # column 5 not stored: rows 2 and 3 untouched
            (i64([1, 3]), np.array([0.0, 0.0])),                    # stored zeros keep their rows touched
            (i64([2, 7]), np.array([-0.0, 1.0]))]
    rows = [(i64([1, 2, 3]), np.array([1.0, 0.0, 2.0])), (i64([1, 4, 5, 6]), nrm(23, 4))]
    return [(a, cols, False, None), (a, rows, True, None)]


def c_ub_edges(mk):
    """columns of S whose products visit SPG_SMALL_MAX - 1, SPG_SMALL_MAX and SPG_SMALL_MAX + 1 cells (the last one takes a slab), with
    rows in common so that the order of the additions matters"""
    lens = [SMALL - 424, 423, 1, 1, 40]
    cols = [(i64([1, 2]), nrm(32, 2)), (i64([1, 2, 3]), nrm(33, 3)), (i64([1, 2, 3, 4]), nrm(34, 4)), (i64([5]), nrm(35, 1))]
    return both(mk, *column_matrix(31, 3000, lens), cols)


def c_congruent(mk):
    """touched rows all congruent modulo SPG_TABLE_SLOTS"""
    rows = 1 + SLOTS * np.arange(40, dtype=np.int64)
    I = np.concatenate([rows, rows[::2], rows[5:30]])
    J = np.concatenate([np.full(40, 1), np.full(20, 2), np.full(25, 3)])
    return both(mk, i64(I), i64(J), nrm(41, len(I)), int(rows[-1]) + 3, 3, [(i64([1, 2, 3]), nrm(42, 3)), (i64([2]), nrm(43, 1))])


HUGE = 1 << 40


def huge_matrix():
    """m = 2^40: row keys above 2^32, int64 keys; columns 1..3 of 400 cells each (together a slab-path column), 4 and 5 short"""
    rng = np.random.default_rng(51)
    lens = [400, 400, 400, 30, 7]
    I = np.concatenate([np.sort(rng.choice(1 << 20, size=c, replace=False)).astype(np.int64) * 1000003 + (1 << 32) + 1 for c in lens])
    J = np.concatenate([np.full(c, j + 1) for j, c in enumerate(lens)])
    I[-1] = HUGE
    return i64(I), i64(J), rng.standard_normal(len(I)), HUGE, 5


HUGE_COLS = [(i64([4, 5]), nrm(52, 2)), (i64([1, 4]), nrm(53, 2)), (i64([2, 3]), nrm(54, 2))]
HUGE_LONG = [(i64([4]), np.ones(1)), (i64([1, 2, 3]), np.ones(3))]      # the second column visits 1200 cells: the slab path


def c_huge_rows(mk):
    return both(mk, *huge_matrix(), HUGE_COLS)


def c_spans(mk):
    """a span longer than 64 slots in the LDS path, one longer than 2048 slots in the slab path (the CPU test checks both lengths on
    the oracle's layout), and a row touched by every entry of a 300-entry column of S"""
    m = 4000
    I, J, V, _, _ = column_matrix(61, m, [100, 2500, 900])
    I = np.concatenate([I, np.full(300, 7), np.arange(1, 301) * 5])
    J = np.concatenate([J, np.arange(4, 304), np.arange(4, 304)])
    V = np.concatenate([V, nrm(62, 600)])
    cols = [(i64([1]), nrm(63, 1)), (i64([2]), nrm(64, 1)), (i64([1, 3]), nrm(65, 2)), (i64(np.arange(4, 304)), nrm(66, 300))]
    out = both(mk, i64(I), i64(J), V, m, 303, cols)
    return out + [(out[0][0], [(i64([7]), nrm(67, 1)), (i64([7, 10, 15]), nrm(68, 3))], True, None)]


def c_slabs(mk):
    """SPG_MAX_SLABS + 1 long columns in one call (the owners reuse slabs), short ones between them"""
    lens = [SMALL + 6] + [3] * (MAX_SLABS + 2)
    cols = []
    for j in range(MAX_SLABS + 1):
        cols.append((i64([1, 2 + j]), nrm(72 + j, 2)))
        if j % 3 == 0:
            cols.append((i64([2 + j, 3 + j]), nrm(172 + j, 2)))
    return both(mk, *column_matrix(71, 3000, lens), cols)


GRID_K = 65537


def c_grid(mk):
    """k = 65537 single-entry columns out of 50 distinct ones"""
    I, J, V = normal_matrix(81, 60, 50, 150)
    cols = [(i64([c]), nrm(82 + c, 1)) for c in range(1, 51)]
    return both(mk, I, J, V, 60, 50, cols, np.arange(GRID_K, dtype=np.int64) * 7 % 50)


def c_protocol(mk):
    I, J, V = normal_matrix(91, 300, 200, 2500)
    a = mk(I, J, V, 300, 200)
    cols = [(xi, np.where(xv == 0.0, 1.0, xv)) for xi, xv in random_columns(92, 200, 9, 30)]      # no stored zero: the round trip keeps every entry
    rows = random_columns(93, 300, 5, 12)
    return [(a, cols, False, None), (a, rows, True, None)]


CASES = dict(degenerate=c_degenerate, nonfinite=c_nonfinite, ub_edges=c_ub_edges, congruent=c_congruent, huge_rows=c_huge_rows,
             spans=c_spans, slabs=c_slabs, grid=c_grid, protocol=c_protocol)


def maker(dsa, binding):
    return lambda I, J, V, m, n: dsa.dynamicsparse(I, J, V, m, n, binding=binding)


def layout_of(b, tr):
    return b.export_layout(ROWMAJOR if tr else COLMAJOR)


def cells_visited(L, xi):
    """stored cells the column with keys xi visits (ub of csrc/spgemm.hip)"""
    return sum(len(model_mul(L, i64([key]), np.ones(1))[0]) for key in xi.tolist())


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
def test_spgemm_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name


def test_api_has_the_product(dsa):
    for cls, names in ((dsa.DynamicSparseMatrix, ("matmul_sparse", "matmul_sparse_dev", "_require_spgemm")), (dsa.Transposed, ("matmul_sparse",))):
        for name in names:
            assert callable(getattr(cls, name, None)), (cls.__name__, name)


def test_constants_are_consistent():
    assert SLOTS >= 2 * SMALL and SLOTS & (SLOTS - 1) == 0 and MAX_SLABS >= 1
    assert SPG["SPG_SLAB_BYTES_MAX"] < HUGE * 8                     # the m = 2^40 matrix cannot get a slab


def test_oracle_binding_does_not_have_them(dsa, oracle):
    assert oracle.prefix == "ora"
    for name in NAMES:
        assert not oracle.has(name)
        assert name not in dsa.Binding.SIGNATURES
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    S = (i64([0, 1]), i64([0]), np.ones(1))
    for call in (lambda: a.matmul_sparse(S), lambda: a.T.matmul_sparse(S), lambda: a.matmul_sparse_dev(0, 0, 0, 0, 0, 0, 0, 0, 0)):
        with pytest.raises(dsa.DsaArgumentError):
            call()


def oracle_mul(b, xi, xv, tr, cap):
    """ora_mat_spmv_sparse with a result buffer of `cap` pairs (the API's mul sizes it by size(m), which is 2^40 in one case)"""
    P64, PF = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    xi, xv = i64(xi), np.ascontiguousarray(xv, dtype=np.float64)
    yi, yv, k = np.empty(cap, dtype=np.int64), np.empty(cap), C.c_int64()
    b.b.call("mat_spmv_sparse", b.h, 1 if tr else 0, xi.ctypes.data_as(P64), xv.ctypes.data_as(PF), len(xi), yi.ctypes.data_as(P64),
             yv.ctypes.data_as(PF), cap, C.byref(k))
    return yi[:k.value], yv[:k.value]


def _helper_against_oracle(b, cols, tr, what):
    L = layout_of(b, tr)
    m, n = b.size()
    ny = n if tr else m
    exp = expected_csc(L, cols)
    for j, (xi, xv) in enumerate(cols):
        rows, vals = exp[1][exp[0][j]:exp[0][j + 1]] + 1, exp[2][exp[0][j]:exp[0][j + 1]]
        if len(rows) and (rows.min() < 1 or rows.max() > ny):
            continue                                                 # the oracle throws for a row outside size(m); so does the product
        ie, ve = oracle_mul(b, xi, xv, tr, len(rows) + 8)
        assert np.array_equal(rows, ie), (what, j)
        assert same_bits(vals, ve), (what, j)
        assert np.all(np.diff(rows) > 0)
    return L, exp


@pytest.mark.parametrize("name", sorted(CASES))
def test_helper_matches_the_oracle_on_every_case(dsa, oracle, name):
    items = CASES[name](maker(dsa, oracle))
    assert {tr for _, _, tr, _ in items} == {False, True}, "every case runs both transposes"
    for q, (b, cols, tr, pick) in enumerate(items):
        for xi, _ in cols:
            assert np.all(np.diff(xi) > 0), "the keys of a column must ascend strictly"
        L, exp = _helper_against_oracle(b, cols, tr, (name, q))
        ub = [cells_visited(L, xi) for xi, _ in cols] if name in ("ub_edges", "slabs", "huge_rows", "spans") else []
        if name == "ub_edges":
            assert ub[:3] == [SMALL - 1, SMALL, SMALL + 1]
        if name == "slabs":
            assert sum(u > SMALL for u in ub) == MAX_SLABS + 1 and any(u <= SMALL for u in ub) and sum(ub) <= 20000
        if name == "huge_rows":
            assert max(ub) <= SMALL and exp[1].min() >= 1 << 32 and exp[1].max() == HUGE - 1
        if name == "congruent":
            assert len(set((exp[1] % SLOTS).tolist())) == 1 and len(exp[1]) > 40
        if name == "spans" and len(cols) == 4:                       # (both orientations)
            sem = L["semaphores"]
            span = np.diff(np.append(sem, len(L["occ"]) + 1)) - 1     # slots of each partition (the table has no tombstone here)
            assert span[0] > 64 and ub[0] <= SMALL and span[1] > 2048 and ub[1] > SMALL and ub[3] >= 600
            row7 = exp[1][exp[0][3]:exp[0][4]].tolist().index(6)
            assert np.isfinite(exp[2][exp[0][3] + row7])
        if name == "nonfinite" and not tr:
            col = lambda j: dict(zip((exp[1][exp[0][j]:exp[0][j + 1]] + 1).tolist(), exp[2][exp[0][j]:exp[0][j + 1]].tolist()))
            assert np.isnan(col(0)[2]) and np.isnan(col(0)[3]) and col(1)[2] == np.inf and np.isnan(col(1)[3])
            assert 2 not in col(2) and 3 not in col(2)
            assert sorted(col(3)) == [1, 4] and all(v == 0.0 for v in col(3).values())


def test_the_huge_matrix_has_a_slab_path_column(dsa, oracle):
    for b, _, tr, _ in c_huge_rows(maker(dsa, oracle)):
        ub = [cells_visited(layout_of(b, tr), xi) for xi, _ in HUGE_LONG]
        assert ub[0] <= SMALL < ub[1], (tr, ub)
        assert b.size()[1 if tr else 0] == HUGE


@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_helper_matches_the_oracle_on_the_golden_layouts(dsa, oracle, sc):
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        return
    m, n = b.size()
    for tr in (False, True):
        _helper_against_oracle(b, random_columns(len(sc["name"]), m if tr else n, 6, 8), tr, (sc["name"], tr))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def _t(arr, dt, dev="cuda"):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev).to(dt)
    return t if t.numel() else torch.zeros(1, dtype=dt, device=dev)


def run_dev(a, S, tr, bits=64, base=0, protocol=True):
    """dsa_mat_spgemm_csc_dev on torch tensors: the count-only call, cap = total - 1 (DSA_ECAP: yptr valid, yidx / yval untouched),
    then cap = total into buffers three entries longer.  Returns numpy (ptr, idx, val)."""
    import torch
    dt = torch.int32 if bits == 32 else torch.int64
    xptr, xidx, xval = S
    k, nnzx = len(xptr) - 1, len(xidx)
    d_xptr, d_xidx, d_xval = _t(xptr + base, dt), _t(xidx + base, dt), _t(xval, torch.float64)
    yptr = torch.full((k + 1,), -7, dtype=dt, device="cuda")
    torch.cuda.synchronize()

    def call(d_yidx, d_yval, cap):
        r = a.matmul_sparse_dev(d_xptr.data_ptr(), d_xidx.data_ptr(), d_xval.data_ptr(), k, nnzx, yptr.data_ptr(), d_yidx, d_yval, cap,
                                index_bits=bits, base=base, transpose=tr)
        a.sync()
        return r
    total, fits = call(0, 0, 0)
    assert fits == (total == 0)
    ptr0 = yptr.cpu().numpy().astype(np.int64)
    assert ptr0[0] == base and ptr0[-1] == base + total and np.all(np.diff(ptr0) >= 0)
    yidx = torch.full((total + 3,), -7, dtype=dt, device="cuda")
    yval = torch.full((total + 3,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if protocol and total > 0:
        yptr.fill_(-7)
        torch.cuda.synchronize()
        got, fits = call(yidx.data_ptr(), yval.data_ptr(), total - 1)
        assert not fits and got == total
        assert np.array_equal(yptr.cpu().numpy().astype(np.int64), ptr0)
        assert bool((yidx == -7).all()) and bool((yval == -7.0).all())
    yptr.fill_(-7)
    torch.cuda.synchronize()
    got, fits = call(yidx.data_ptr(), yval.data_ptr(), total)
    assert fits and got == total
    assert np.array_equal(yptr.cpu().numpy().astype(np.int64), ptr0)          # the count-only call leaves the same yptr
    assert bool((yidx[total:] == -7).all()) and bool((yval[total:] == -7.0).all())
    return ptr0, yidx[:total].cpu().numpy().astype(np.int64), yval[:total].cpu().numpy()


def run_host(a, S, tr, base=0):
    return a.matmul_sparse((S[0] + base, S[1] + base, S[2]), transpose=tr, base=base)


def check_case(dsa, a, b, cols, tr, pick, what, bits=(64,), bases=(0,), protocol=True):
    m, n = b.size()
    exp = expected_csc(layout_of(b, tr), cols, pick)
    S = csc_of(cols, pick)
    if not in_size(exp, n if tr else m):
        with pytest.raises(dsa.DsaBoundsError):
            run_dev(a, S, tr)
        with pytest.raises(dsa.DsaBoundsError):
            run_host(a, S, tr)
        return exp
    for base in bases:
        for nb in bits:
            assert_same(run_dev(a, S, tr, nb, base, protocol), exp, base, (what, "dev", nb, base))
        assert_same(run_host(a, S, tr, base), exp, base, (what, "host", base))
    return exp


def run_cases(dsa, hip, oracle, name, **kw):
    for q, ((a, cols, tr, pick), (b, _, _, _)) in enumerate(zip(CASES[name](maker(dsa, hip)), CASES[name](maker(dsa, oracle)))):
        check_case(dsa, a, b, cols, tr, pick, (name, q), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_layouts(dsa, hip, oracle, sc):
    """tombstones, deleted partitions, sparse tables: random columns with keys inside and beyond the size, both transposes"""
    a, b = run_scenario(dsa, hip, sc), run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        for call in (lambda: a.matmul_sparse_dev(0, 0, 0, 0, 0, 0, 0, 0, 0), lambda: a.matmul_sparse((i64([0]), i64([]), np.zeros(0)))):
            with pytest.raises(dsa.DsaError) as ei:
                call()
            assert ei.value.code == EMODE
        return
    m, n = b.size()
    for tr in (False, True):
        check_case(dsa, a, b, random_columns(len(sc["name"]), m if tr else n, 6, 8), tr, None, (sc["name"], tr), bits=(32, 64), bases=(0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("degenerate", "nonfinite", "ub_edges", "congruent", "spans", "slabs"))
def test_shapes_values_and_both_paths(dsa, hip, oracle, name):
    run_cases(dsa, hip, oracle, name, bits=(32, 64))


@pytest.mark.gpu
def test_k_zero_gives_the_base(dsa, hip):
    a = maker(dsa, hip)(*nonfinite_matrix())
    for base in (0, 1):
        for nb in (32, 64):
            ptr, idx, val = run_dev(a, csc_of([]), False, nb, base)
            assert ptr.tolist() == [base] and len(idx) == 0
        ptr, idx, val = run_host(a, csc_of([]), True, base)
        assert ptr.tolist() == [base] and len(idx) == 0 and len(val) == 0


@pytest.mark.gpu
def test_row_keys_above_2_to_32_and_the_slab_limit(dsa, hip, oracle):
    """m = 2^40, int64 keys: the LDS path carries the full key; a column that needs a slab of 2^40 doubles is the documented DSA_EARG
    (nothing of that size is allocated: the pool holds no more afterwards), and the next call is right"""
    for (a, cols, tr, pick), (b, _, _, _) in zip(c_huge_rows(maker(dsa, hip)), c_huge_rows(maker(dsa, oracle))):
        exp = check_case(dsa, a, b, cols, tr, pick, ("huge", tr), bases=(0, 1))
        assert exp[1].max() == HUGE - 1
        idle = dsa.pool_idle_bytes(hip)
        for fn in (run_dev, run_host):
            with pytest.raises(dsa.DsaArgumentError) as ei:
                fn(a, csc_of(HUGE_LONG), tr)
            assert ei.value.code == EARG and "SPG_SLAB_BYTES_MAX" in str(ei.value)
        with pytest.raises(dsa.DsaArgumentError):                    # 32-bit indices cannot hold the rows
            run_dev(a, csc_of(cols), tr, bits=32)
        assert dsa.pool_idle_bytes(hip) <= idle + (1 << 24)
        check_case(dsa, a, b, cols, tr, pick, ("huge after EARG", tr))


@pytest.mark.gpu
def test_grid_arithmetic(dsa, hip, oracle):
    run_cases(dsa, hip, oracle, "grid", bits=(32,), protocol=False)


@pytest.mark.gpu
def test_protocol_formats_round_trip_and_repeatability(dsa, hip, oracle):
    import torch
    run_cases(dsa, hip, oracle, "protocol", bits=(32, 64), bases=(0, 1))
    (a, cols, tr, _), _ = c_protocol(maker(dsa, hip))
    S = csc_of(cols)
    first = run_dev(a, S, tr)
    again = run_dev(a, S, tr)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert np.array_equal(first[2].view(np.uint64), again[2].view(np.uint64))
    # the result goes straight into the device import, and the export of that matrix is the result
    m, n = a.size()
    k, total = len(S[0]) - 1, len(first[1])
    d = [torch.from_numpy(x).to("cuda") for x in first]
    torch.cuda.synchronize()
    y = dsa.dynamicsparse_compressed_dev(COLMAJOR, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), k, m, total, binding=hip)
    assert y.size() == (m, k) and y.nnz() == total
    back = y.to_csc()
    assert np.array_equal(back[0], first[0]) and np.array_equal(back[1], first[1])
    assert np.array_equal(back[2].view(np.uint64), first[2].view(np.uint64))


@pytest.mark.gpu
def test_torch_sparse_csc(dsa, hip, oracle):
    import torch
    for (a, cols, tr, _), (b, _, _, _) in zip(c_protocol(maker(dsa, hip)), c_protocol(maker(dsa, oracle))):
        m, n = b.size()
        nx, ny = (m, n) if tr else (n, m)
        cols = [(xi[xi <= nx], xv[xi <= nx]) for xi, xv in cols]      # torch checks the indices against the shape
        exp = expected_csc(layout_of(b, tr), cols)
        S = csc_of(cols)
        dense = np.zeros((ny, len(cols)))
        for j in range(len(cols)):
            dense[exp[1][exp[0][j]:exp[0][j + 1]], j] = exp[2][exp[0][j]:exp[0][j + 1]]
        for dt in (torch.int32, torch.int64):
            St = torch.sparse_csc_tensor(_t(S[0], dt), _t(S[1], dt)[:len(S[1])], _t(S[2], torch.float64)[:len(S[1])], size=(nx, len(cols)))
            Y = (a.T.matmul_sparse(St) if tr else a.matmul_sparse(St))
            assert Y.layout == torch.sparse_csc and tuple(Y.shape) == (ny, len(cols)) and Y.ccol_indices().dtype == dt
            assert same_bits(Y.to_dense().cpu().numpy(), dense)


def broken_inputs(S):
    """(what, S') for every clause of the input contract, made from the valid S"""
    xptr, xidx, xval = S
    lens = np.diff(xptr)
    j = int(np.nonzero(lens >= 3)[0][0])                             # a column with three entries or more
    lo, hi = int(xptr[j]), int(xptr[j + 1])
    q = int(np.nonzero(xptr[:-1] >= 1)[0][0])                        # a column that does not start at 0
    swapped = xidx.copy(); swapped[lo], swapped[lo + 1] = xidx[lo + 1], xidx[lo]
    repeated = xidx.copy(); repeated[hi - 1] = repeated[hi - 2]
    falling = xptr.copy(); falling[q + 1] = falling[q] - 1
    short = xptr.copy(); short[-1] -= 1
    shifted = xptr.copy(); shifted[0] = 1
    return [("descending", (xptr, swapped, xval)), ("repeated", (xptr, repeated, xval)), ("ptr decreases", (falling, xidx, xval)),
            ("ptr[k] - base != nnzx", (short, xidx, xval)), ("ptr[0] != base", (shifted, xidx, xval))]


@pytest.mark.gpu
def test_errors_end_as_status_codes_and_the_next_call_is_right(dsa, hip, oracle):
    import torch
    # fill mode
    f = dsa.dynamicsparse(binding=hip)
    f.addrow(1, [1, 2], [1.0, 2.0])
    for tr in (False, True):
        with pytest.raises(dsa.DsaError) as ei:
            run_dev(f, csc_of([(i64([1]), np.ones(1))]), tr)
        assert ei.value.code == EMODE
    for (a, cols, tr, _), (b, _, _, _) in zip(c_protocol(maker(dsa, hip)), c_protocol(maker(dsa, oracle))):
        S = csc_of(cols)
        good = lambda: check_case(dsa, a, b, cols, tr, None, ("after an error", tr), protocol=False)
        good()
        # the input contract
        for what, bad in broken_inputs(S):
            for base in (0, 1):
                with pytest.raises(dsa.DsaError) as ei:
                    run_dev(a, bad, tr, 64, base)
                assert ei.value.code == EARG, (what, base, tr)
            good()
        for what, bad in broken_inputs(S)[:3]:                       # (the host form takes nnzx from xptr[k])
            with pytest.raises(dsa.DsaError) as ei:
                run_host(a, bad, tr)
            assert ei.value.code == EARG, (what, tr)
        good()
        # arguments
        buf = torch.zeros(64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        p = buf.data_ptr()
        ok = dict(d_xptr=p, d_xidx=p, d_xval=p, k=2, nnzx=0, d_yptr=p + 256, d_yidx=p, d_yval=p, cap=8, index_bits=64, base=0, transpose=tr)
        assert a.matmul_sparse_dev(**ok) == (0, True)
        for change in (dict(index_bits=16), dict(base=2), dict(base=-1), dict(transpose=2), dict(k=-1), dict(k=1 << 31), dict(nnzx=-1),
                       dict(nnzx=1 << 31), dict(d_xptr=0), dict(d_yptr=0), dict(d_yidx=0), dict(d_yval=0), dict(cap=-1),
                       dict(nnzx=1, d_xidx=0), dict(nnzx=1, d_xval=0)):
            with pytest.raises(dsa.DsaError) as ei:
                args = dict(ok, **change)
                a.b.call("mat_spgemm_csc_dev", a.h, int(args["transpose"]), args["index_bits"], args["base"], C.c_void_p(args["d_xptr"]),
                         C.c_void_p(args["d_xidx"]), C.c_void_p(args["d_xval"]), args["k"], args["nnzx"], C.c_void_p(args["d_yptr"]),
                         C.c_void_p(args["d_yidx"]), C.c_void_p(args["d_yval"]), args["cap"], C.byref(C.c_int64()))
            assert ei.value.code == EARG, (change, tr)
        a.sync()
        good()
    # a stored key beyond size(m): an explicit size below the largest key, as a row key (A S) and as a column key (A' S)
    bad_cols, ok_cols = [(i64([1]), np.ones(1)), (i64([2, 3]), np.ones(2))], [(i64([1, 3]), nrm(1, 2)), (i64([3]), nrm(2, 1))]
    for tr in (False, True):
        I, J = ([1, 2, 3], [1, 5, 2]) if tr else ([1, 5, 2], [1, 2, 3])
        c, d = (dsa.dynamicsparse(I, J, [1.0, 2.0, 3.0], m=3, n=3, binding=x) for x in (hip, oracle))
        with pytest.raises(dsa.DsaError):
            d.mul(bad_cols[1], transpose=tr)
        for fn in (run_dev, run_host):
            with pytest.raises(dsa.DsaError) as ei:
                fn(c, csc_of(bad_cols), tr)
            assert ei.value.code == EBOUNDS, tr
            check_case(dsa, c, d, ok_cols, tr, None, ("after EBOUNDS", tr))
