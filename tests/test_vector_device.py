"""DynamicSparseVector as a device operand (csrc/vecops.hip, csrc/vecops_host.hip): nonzeros_dev / to_torch, dynamicsparsevec_dev,
axpby_vec, mul_vec (plain and transposed), reduce / sum / norm, dot (sparse and dense) and to_dense_dev.

Models.  Plain numpy / Python, nothing of the library: `model_axpby` (as in test_vector_algebra.py, restated), `model_fold` (the
builder's stable sort + left fold, stored zeros kept: src/vector.jl:10-36), `model_mul` (the touched rows of mat * x over the stored
entries of x), `exact` (a sum of doubles as a Fraction).  The CPU half runs them on literals and against the oracle's axpby / mul /
dynamicsparsevec on the very inputs the GPU half uses, so the inputs are qualified before the GPU sees them.

GPU half.  Keys, occupancy, lengths and capacities are compared exactly.  Layout comparisons (`same_layout`) are bitwise on the
occupied slots.  Every case asserts the regime it claims on the structure at hand first:
* the pack switch: capacity against VIEW_SMALL_SLOTS = 65536 (a range of exactly 65536 slots is still packed by the one launch).
  40 000 entries build into 65 536 slots and stay on the one-launch side; 46 000 entries build into 131 072 slots and are the
  case that crosses it.  Both sizes are run wherever a size is asked for.
* the physical key width: nothing reports it; a vector that holds a key >= 2^31 cannot keep 32-bit keys, one built from keys below
  2^31 keeps them (csrc/build_host.hip: KeyScan) — the cases assert the keys they hold.
* the strategy of the sparse-x product: nothing reports it; the rule is csrc/sparsex_host.hip: spx_xdriven, 8 nx < ncols is driven by
  x, anything else gathers — unless the first key of x is below 1, which only the x-driven kernel can address.

Values.  axpby_vec, dynamicsparsevec_dev, nonzeros_dev and to_dense_dev move or merge values: bitwise.  mul_vec with small-integer
values: every sum is exact in any order, bitwise.  mul_vec with standard-normal values: tests/test_sparse_x.py applies NO tolerance
to this product (it demands equality on inputs that sum exactly), so there is none to take from it; both sides here are sums of the
same n separately rounded products in two unknown orders (fp64 atomics), each within gamma_n * sum|p| of the exact sum, and the test
bounds their difference by 2 * gamma_n * sum|p| per row, gamma_n = n u / (1 - n u), u = 2^-53.  reduce / dot: |got - exact| <=
gamma_n * sum|term| with exact and sum|term| as Fractions (n = the terms that are not +0.0 by construction: adding +0.0 is exact),
and bitwise equality wherever the issue states one (twice, across layouts, dot(a, a) against the sum of squares)."""
import ctypes as C
import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 65536                      # VIEW_SMALL_SLOTS
W31, W40 = 1 << 31, 1 << 40
A3, B7 = 1.0 / 3.0, 0.7
U = F(1, 2 ** 53)
VO_FIN_THREADS = 1024              # csrc/vecops.h, asserted in test_stage2_constants
VO_PASS_CELLS = VO_FIN_THREADS * 64
ECAP = 8


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def same_values(got, want):
    """bitwise, but a NaN matches a NaN of any payload"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


# ================================================================== the models
def model_axpby(xk, xv, alpha, yk, yv, beta):
    xk, yk = np.asarray(xk, dtype=np.int64), np.asarray(yk, dtype=np.int64)
    xv, yv = np.asarray(xv, dtype=np.float64), np.asarray(yv, dtype=np.float64)
    assert np.all(xk[1:] > xk[:-1]) and np.all(yk[1:] > yk[:-1])
    keys = np.union1d(xk, yk).astype(np.int64)
    ix, iy = np.searchsorted(keys, xk), np.searchsorted(keys, yk)
    inx, iny = np.zeros(len(keys), dtype=bool), np.zeros(len(keys), dtype=bool)
    inx[ix] = True
    iny[iy] = True
    ax, by = np.zeros(len(keys)), np.zeros(len(keys))
    with np.errstate(all="ignore"):
        ax[ix] = np.float64(alpha) * xv
        by[iy] = np.float64(beta) * yv
        both = inx & iny
        out = np.where(inx, ax, by)
        out[both] = (ax + by)[both]
    keep = ~(both & (out == 0.0))
    return keys[keep], out[keep]


def model_fold(keys, vals, combine):
    """_prepare_keys_vals! (src/vector.jl:10-36): stable sort by key, duplicates folded left to right in input order, zeros kept"""
    keys, vals = np.asarray(keys, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    op = {"+": lambda a, b: a + b, "*": lambda a, b: a * b, "last": lambda a, b: b}[combine]
    order = np.argsort(keys, kind="stable")
    ok, ov = [], []
    for q in order.tolist():
        if ok and ok[-1] == keys[q]:
            ov[-1] = op(ov[-1], vals[q])
        else:
            ok.append(int(keys[q]))
            ov.append(vals[q])
    return np.array(ok, dtype=np.int64), np.array(ov, dtype=np.float64)


def model_mul(I, J, V, xk, xv, transpose):
    """the touched rows of mat * x (src/operations.jl:62-135) for DISTINCT cells (I, J, V): a row is touched by every stored entry of
    x whose key is the column of one of its cells; returns (rows ascending, sums in cell order, per row the products)"""
    if transpose:
        I, J = J, I
    pos = {int(k): float(v) for k, v in zip(np.asarray(xk).tolist(), np.asarray(xv).tolist())}
    prods = {}
    with np.errstate(invalid="ignore"):
        for i, j, a in zip(I.tolist(), J.tolist(), V.tolist()):
            if j in pos:
                prods.setdefault(i, []).append(np.float64(pos[j]) * np.float64(a))
    rows = np.array(sorted(prods), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        vals = np.array([np.sum(np.array(prods[r])) for r in rows.tolist()], dtype=np.float64)
    return rows, vals, prods


def exact(terms):
    """(sum, sum of |.|) of finite doubles as Fractions"""
    s = a = 0
    for t in np.asarray(terms, dtype=np.float64).tolist():
        n, d = t.as_integer_ratio()                   # d is a power of two <= 2^1074
        n *= (1 << 1074) // d
        s += n
        a += abs(n)
    return F(s, 1 << 1074), F(a, 1 << 1074)


def gamma(n):
    return n * U / (1 - n * U)


def within_bound(got, terms):
    """|got - exact| <= gamma_n * sum|term| over the terms that are not zero by construction"""
    s, a = exact(terms)
    n = len(terms)
    return abs(F(float(got)) - s) <= gamma(n) * a if n else (float(got) == 0.0 and not math.copysign(1.0, got) < 0)


# ================================================================== seeded inputs, shared by the CPU and the GPU half
def vec_input(n, seed, step=3, first=1, ints=False):
    rng = np.random.default_rng(seed)
    k = first + step * np.arange(n, dtype=np.int64)
    v = rng.integers(-9, 10, n).astype(np.float64) if ints else rng.standard_normal(n)
    if ints:
        v[v == 0.0] = 1.0
    return k, v


def fold_cases():
    rng = np.random.default_rng(4102)
    out = {}
    k = rng.permutation(5 * np.arange(1, 301, dtype=np.int64))
    out["unsorted"] = (k, rng.standard_normal(300), "+", None)
    k = rng.integers(1, 120, 400)
    out["duplicates_add"] = (k, rng.standard_normal(400), "+", None)
    out["duplicates_mul"] = (k, rng.standard_normal(400), "*", None)
    out["duplicates_last"] = (k, rng.standard_normal(400), "last", 500)
    out["cancel_to_zero"] = (np.array([7, 3, 7, 9]), np.array([1.5, 2.0, -1.5, 0.0]), "+", None)      # stored zeros are kept
    out["empty"] = (np.zeros(0, dtype=np.int64), np.zeros(0), "+", None)
    out["empty_len"] = (np.zeros(0, dtype=np.int64), np.zeros(0), "+", 17)
    k = np.concatenate([rng.permutation(np.arange(1, 60, dtype=np.int64)), [W31 + 5]])
    out["wide_key"] = (k, rng.standard_normal(60), "+", None)
    out["len_given"] = (np.array([4, 2, 9]), np.array([1.0, 2.0, 3.0]), "+", 1000)
    k = rng.integers(1, 2500, 3000)                   # more than 1024 pairs: the host form takes the general builder as well
    out["long_duplicates"] = (k, rng.standard_normal(3000), "+", None)
    return out


def axpby_cases():
    """name -> (a, b, alpha, beta); a / b = (keys, values, len or None); b None: b is a"""
    rng = np.random.default_rng(4103)
    out = {}
    ak, av = vec_input(300, 1, step=2)
    bk, bv = vec_input(280, 2, step=3)
    out["small"] = ((ak, av, None), (bk, bv, 2000), A3, B7)
    out["b_is_a"] = ((ak, av, None), None, A3, B7)
    out["cancel"] = ((ak, av, None), (ak, av.copy(), None), 1.0, -1.0)
    big = vec_input(46000, 3, step=2)
    out["operand_large"] = ((big[0], big[1], None), (bk, bv, None), A3, B7)
    h1, h2 = vec_input(35000, 4, step=2), vec_input(35000, 5, step=2, first=20001)
    out["merged_large"] = ((h1[0], h1[1], None), (h2[0], h2[1], None), A3, B7)
    wk = np.concatenate([ak[::2], W31 + 3 * np.arange(50), W40 + np.arange(1, 51)])
    out["mixed_widths"] = ((ak, av, None), (wk, rng.standard_normal(len(wk)), None), A3, B7)
    out["wide_first"] = ((wk, rng.standard_normal(len(wk)), None), (ak, av, None), B7, A3)
    none = (np.zeros(0, dtype=np.int64), np.zeros(0), 7)
    out["a_empty"] = (none, (bk, bv, None), A3, B7)
    out["b_empty"] = ((ak, av, None), none, A3, B7)
    out["empty_both"] = ((np.zeros(0, dtype=np.int64), np.zeros(0), 5), (np.zeros(0, dtype=np.int64), np.zeros(0), 9), A3, B7)
    return out


M_ROWS, M_COLS = 300, 200
EMPTY_COLS = (141, 170)            # no cell in these columns
EMPTY_ROWS = (231, 275)            # ... nor in these rows (the columns of the transposed product)


def matrix_input(ints=True, seed=4104):
    """about 2000 distinct cells of a 300 x 200 matrix; columns 141..170 and rows 231..275 stay empty"""
    rng = np.random.default_rng(seed)
    cell = rng.choice(M_ROWS * M_COLS, 2600, replace=False)
    I, J = cell // M_COLS + 1, cell % M_COLS + 1
    keep = ~((J >= EMPTY_COLS[0]) & (J <= EMPTY_COLS[1])) & ~((I >= EMPTY_ROWS[0]) & (I <= EMPTY_ROWS[1]))
    I, J = I[keep].astype(np.int64), J[keep].astype(np.int64)
    if ints:
        V = rng.integers(-8, 9, len(I)).astype(np.float64)
        V[V == 0.0] = 3.0
    else:
        V = rng.standard_normal(len(I))
    return I, J, V


def x_cases(transpose, ints=True):
    """name -> (keys, values, forced) for a product over `ncols` columns; forced: the first key is below 1"""
    ncols = M_ROWS if transpose else M_COLS
    lo, hi = EMPTY_ROWS if transpose else EMPTY_COLS
    edge = (ncols - 1) // 8                           # 8 * edge < ncols <= 8 * (edge + 1)
    rng = np.random.default_rng(4105 + transpose)

    def vals(n):
        if ints:
            v = rng.integers(-6, 7, n).astype(np.float64)
            v[::7] = 0.0                              # stored zeros of x still touch their rows
            return v
        return rng.standard_normal(n)

    def keys(n, among=None):
        pool = np.arange(1, ncols + 1) if among is None else among
        return np.sort(rng.choice(pool, n, replace=False)).astype(np.int64)

    live = np.setdiff1d(np.arange(1, ncols + 1), np.arange(lo, hi + 1))
    out = {}
    out["xdriven_edge"] = (keys(edge, live), vals(edge), False)
    out["gather_edge"] = (keys(edge + 1, live), vals(edge + 1), False)
    out["empty"] = (np.zeros(0, dtype=np.int64), np.zeros(0), False)
    out["all_miss_xdriven"] = (np.arange(lo, lo + 5, dtype=np.int64), vals(5), False)
    out["all_miss_gather"] = (np.arange(lo, hi + 1, dtype=np.int64)[:edge + 2], vals(edge + 2), False)
    k = np.concatenate([[-3], keys(10, live), [ncols + 50]])
    out["outside_xdriven"] = (k, vals(len(k)), True)
    k = np.concatenate([[-7, -3], keys(edge + 5, live), [ncols + 1, ncols + 50]])
    out["outside_gather_forced"] = (k, vals(len(k)), True)
    k = np.concatenate([keys(edge + 5, live), [ncols + 1, W31 + 9]])
    out["wide_keys_gather"] = (k, vals(len(k)), False)
    k = np.concatenate([keys(6, live), [W40]])
    out["wide_keys_xdriven"] = (k, vals(len(k)), False)
    out["dense_x"] = (np.arange(1, ncols + 1, dtype=np.int64), vals(ncols), False)
    return out


def rule_xdriven(nx, ncols, forced):
    return nx * 8 < max(ncols, 1) or forced


# ================================================================== CPU half
def test_models_on_literals():
    k, v = model_axpby([1, 3, 5], [1.0, 2.0, -0.0], 2.0, [3, 4, 5], [-4.0, 0.5, 0.0], 1.0)
    assert k.tolist() == [1, 4] and v.tolist() == [2.0, 0.5]
    k, v = model_fold([5, 2, 5, 2, 9], [1.0, 2.0, 3.0, -2.0, 0.0], "+")
    assert k.tolist() == [2, 5, 9] and v.tolist() == [0.0, 4.0, 0.0]          # zeros stay stored
    assert model_fold([5, 2, 5], [2.0, 7.0, 3.0], "*")[1].tolist() == [7.0, 6.0]
    assert model_fold([5, 2, 5], [2.0, 7.0, 3.0], "last")[1].tolist() == [7.0, 3.0]
    I, J, V = np.array([1, 1, 2, 3]), np.array([1, 2, 2, 3]), np.array([2.0, 3.0, 4.0, np.inf])
    r, s, _ = model_mul(I, J, V, [1, 2], [10.0, 0.0], False)
    assert r.tolist() == [1, 2] and s.tolist() == [20.0, 0.0]                 # a stored zero of x touches row 2; column 3 is never read
    r, s, _ = model_mul(I, J, V, [3], [0.0], False)
    assert r.tolist() == [3] and np.isnan(s[0])                               # 0 * Inf through a column x stores
    r, s, _ = model_mul(I, J, V, [1], [1.0], True)
    assert r.tolist() == [1, 2] and s.tolist() == [2.0, 3.0]
    s, a = exact([0.1, -0.1, 2.0 ** -1074])
    assert s == F(1, 1 << 1074) and a == 2 * F(0.1) + F(1, 1 << 1074)
    assert gamma(1) == U / (1 - U) and gamma(0) == 0
    assert within_bound(0.1 + 0.2, [0.1, 0.2]) and not within_bound(0.4, [0.1, 0.2])
    assert within_bound(0.0, []) and not within_bound(-0.0, []) and not within_bound(1e-300, [])
    assert same_values([np.nan, 1.0], [-np.nan, 1.0]) and not same_values([0.0], [-0.0])
    assert rule_xdriven(24, 200, False) and not rule_xdriven(25, 200, False) and rule_xdriven(25, 200, True)


def test_stage2_constants():
    """the lengths the reductions are tested at come from csrc/vecops.h: one pass of stage 2 covers VO_FIN_THREADS partials of 64 cells"""
    txt = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "vecops.h")).read()
    assert int(re.search(r"constexpr int VO_FIN_THREADS = (\d+);", txt).group(1)) == VO_FIN_THREADS
    assert re.search(r"constexpr int64_t VO_PASS_CELLS = \(int64_t\)VO_FIN_THREADS \* 64;", txt)
    assert int(re.search(r"constexpr int VO_BLOCK = (\d+);", txt).group(1)) % 64 == 0


def test_inputs_qualified_on_oracle(dsa, oracle):
    """the models against the oracle's dynamicsparsevec / axpby / mul on the inputs of the GPU half"""
    for name, (k, v, combine, n) in fold_cases().items():
        vec = dsa.dynamicsparsevec(k, v, combine=combine, n=n, binding=oracle)
        wk, wv = model_fold(k, v, combine)
        gk, gv = vec.nonzeros()
        assert np.array_equal(gk, wk) and same_values(gv, wv), name
        assert len(vec) == (n if n is not None else max(0, int(k.max()) if len(k) else 0)), name
    for name, (a, b, alpha, beta) in axpby_cases().items():
        va = dsa.dynamicsparsevec(a[0], a[1], n=a[2], binding=oracle)
        vb = va if b is None else dsa.dynamicsparsevec(b[0], b[1], n=b[2], binding=oracle)
        bb = a if b is None else b
        gk, gv = va.axpby(alpha, vb, beta)
        wk, wv = model_axpby(a[0], a[1], alpha, bb[0], bb[1], beta)
        assert np.array_equal(gk, wk) and same_values(gv, wv), name
        if name == "cancel":
            assert len(wk) == 0
    I, J, V = matrix_input()
    A = dsa.dynamicsparse(I, J, V, M_ROWS, M_COLS, binding=oracle)
    for tr in (False, True):
        for name, (xk, xv, _) in x_cases(tr).items():
            gr, gs = A.mul((xk, xv), transpose=tr)
            wr, ws, _ = model_mul(I, J, V, xk, xv, tr)
            assert np.array_equal(gr, wr) and same_values(gs, ws), (tr, name)
            if name.startswith("all_miss") or name == "empty":
                assert len(wr) == 0


def test_device_calls_need_the_product_library(dsa, oracle):
    """the new calls are HIP library only: on another binding they raise, they do not fall back"""
    v = dsa.dynamicsparsevec([1, 2], [1.0, 2.0], binding=oracle)
    A = dsa.dynamicsparse([1], [1], [1.0], 2, 2, binding=oracle)
    for call in (lambda: v.dot(v), lambda: v.sum(), lambda: v.norm(1), lambda: v.axpby_vec(1.0, v, 1.0), lambda: v.to_torch(),
                 lambda: v.nonzeros_dev(0, 0, 0), lambda: v.to_dense_dev(0, 0), lambda: A.mul_vec(v), lambda: A.T.mul_vec(v),
                 lambda: dsa.dynamicsparsevec_dev(0, 0, 0, binding=oracle)):
        with pytest.raises(dsa.DsaArgumentError):
            call()
    for name in ("vec_nonzeros_dev", "vec_create_dev", "mat_mul_vec", "vec_axpby_vec", "vec_reduce", "vec_dot", "vec_dot_dense_dev",
                 "vec_to_dense_dev"):
        assert name in dsa.Binding.PRODUCT_SIGNATURES and name not in dsa.Binding.SIGNATURES


# ================================================================== GPU half: helpers
def dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).to("cuda")


def clean(vec):
    r = vec.check()
    return not np.any(r[2:7])


def same_layout(got, want):
    """slot for slot: capacity, occupancy, and keys / values of the occupied slots bitwise; the lengths agree"""
    gk, gv, go = got.export_layout()
    wk, wv, wo = want.export_layout()
    gi, wi = got.info(), want.info()
    assert gi["capacity"] == wi["capacity"] and gi["segment_capacity"] == wi["segment_capacity"], (gi, wi)
    assert gi["nb_elements"] == wi["nb_elements"]
    assert np.array_equal(go, wo)
    m = wo.astype(bool)
    assert np.array_equal(gk[m], wk[m])
    assert same_values(gv[m], wv[m])
    assert len(got) == len(want)
    return True


def mkvec(dsa, hip, k, v, n=None):
    return dsa.dynamicsparsevec(np.asarray(k, dtype=np.int64), np.asarray(v, dtype=np.float64), n=n, binding=hip)


# ================================================================== nonzeros_dev / to_torch
@pytest.mark.gpu
def test_nonzeros_dev_and_to_torch(dsa, hip):
    import torch
    cases = {}
    cases["n100"] = mkvec(dsa, hip, *vec_input(100, 11))
    cases["n40000"] = mkvec(dsa, hip, *vec_input(40000, 12))
    cases["n46000"] = mkvec(dsa, hip, *vec_input(46000, 13))
    k, v = vec_input(200, 14)
    cases["wide"] = mkvec(dsa, hip, np.concatenate([k, [W31, W40 + 1]]), np.concatenate([v, [1.5, -2.5]]))
    cases["empty"] = mkvec(dsa, hip, [], [])
    q = mkvec(dsa, hip, *vec_input(50, 15))
    q[2] = 7.25                                       # queued single writes: a new key, an overwrite, a delete
    q[1] = -1.0
    q[4] = 0.0
    cases["queued"] = q
    assert cases["n100"].info()["capacity"] <= SMALL and cases["n40000"].info()["capacity"] == SMALL
    assert cases["n46000"].info()["capacity"] == 2 * SMALL                      # the tile kernels pack this one
    assert cases["wide"].nonzeros()[0].max() >= W31 and cases["n100"].nonzeros()[0].max() < W31
    for name, vec in cases.items():
        tk, tv = vec.to_torch()
        wk, wv = vec.nonzeros()
        assert tk.dtype == torch.int64 and tv.dtype == torch.float64 and tk.is_cuda and tv.is_cuda, name
        assert np.array_equal(tk.cpu().numpy(), wk) and np.array_equal(bits(tv.cpu().numpy()), bits(wv)), name
        assert np.all(wk[1:] > wk[:-1]) and len(wk) == vec.nnz(), name
        assert clean(vec), name
    assert cases["queued"].nonzeros()[0][:3].tolist() == [1, 2, 7] and cases["queued"].nnz() == 50
    # cap one too small: DSA_ECAP, the count is reported and nothing is written; cap exact: the count comes back
    for name in ("n100", "n46000"):
        vec = cases[name]
        n = vec.nnz()
        dk = torch.full((n,), -77, dtype=torch.int64, device="cuda")
        dv = torch.full((n,), -77.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        got = C.c_int64(-1)
        with pytest.raises(dsa.DsaError) as e:
            hip.call("vec_nonzeros_dev", vec.h, C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr()), n - 1, C.byref(got))
        assert e.value.code == ECAP and got.value == n
        vec.sync()
        assert bool((dk == -77).all()) and bool((dv == -77.5).all()), name
        assert vec.nonzeros_dev(dk.data_ptr(), dv.data_ptr(), n) == n
        vec.sync()
        assert np.array_equal(dk.cpu().numpy(), vec.nonzeros()[0])


# ================================================================== dynamicsparsevec_dev
@pytest.mark.gpu
def test_dynamicsparsevec_dev_builds_the_host_layout(dsa, hip):
    for name, (k, v, combine, n) in fold_cases().items():
        want = dsa.dynamicsparsevec(k, v, combine=combine, n=n, binding=hip)
        got = dsa.dynamicsparsevec_dev(dev(k, np.int64), dev(v, np.float64), combine=combine, len=n, binding=hip)
        assert same_layout(got, want), name
        wk, wv = model_fold(k, v, combine)
        gk, gv = got.nonzeros()
        assert np.array_equal(gk, wk) and same_values(gv, wv), name
        assert len(got) == (n if n is not None else max(0, int(k.max()) if len(k) else 0)), name
        assert clean(got), name
        if name == "wide_key":
            assert gk.max() >= W31
    # device addresses and a count instead of tensors; a prefix of longer arrays
    k, v, _, _ = fold_cases()["unsorted"]
    tk, tv = dev(k, np.int64), dev(v, np.float64)
    import torch
    torch.cuda.synchronize()
    got = dsa.dynamicsparsevec_dev(tk.data_ptr(), tv.data_ptr(), 100, binding=hip)
    assert same_layout(got, dsa.dynamicsparsevec(k[:100], v[:100], binding=hip))
    # the vector is a full citizen: writes, reads and == work on it
    got[1] = 4.0
    assert got[1] == 4.0 and clean(got)


# ================================================================== axpby_vec
@pytest.mark.gpu
def test_axpby_vec_builds_the_vector_of_axpby(dsa, hip):
    for name, (a, b, alpha, beta) in axpby_cases().items():
        va = mkvec(dsa, hip, *a)
        vb = va if b is None else mkvec(dsa, hip, *b)
        bb = a if b is None else b
        if name == "operand_large":
            assert va.info()["capacity"] > SMALL and vb.info()["capacity"] <= SMALL
        elif name == "merged_large":
            assert va.info()["capacity"] <= SMALL and vb.info()["capacity"] <= SMALL and va.nnz() + vb.nnz() > SMALL
        elif name not in ("mixed_widths", "wide_first"):
            assert va.info()["capacity"] <= SMALL and va.nnz() + vb.nnz() <= SMALL
        if name in ("mixed_widths", "wide_first"):
            ka, kb = (a[0], bb[0]) if name == "mixed_widths" else (bb[0], a[0])
            assert ka.max() < W31 <= kb.max()
        pk, pv = va.axpby(alpha, vb, beta)
        wk, wv = model_axpby(a[0], a[1], alpha, bb[0], bb[1], beta)
        assert np.array_equal(pk, wk) and same_values(pv, wv), name
        want = dsa.dynamicsparsevec(pk, pv, n=max(len(va), len(vb)), binding=hip)
        got = va.axpby_vec(alpha, vb, beta)
        assert same_layout(got, want), name
        assert len(got) == max(len(va), len(vb)), name
        if name == "cancel":
            assert got.nnz() == 0 and va.nnz() == 300
        assert clean(got) and clean(va) and clean(vb), name
        # the operands are untouched and still writable: the alternate buffers were handed back in order
        va[int(a[0][0]) if len(a[0]) else 1] = 123.0
        assert va[int(a[0][0]) if len(a[0]) else 1] == 123.0 and clean(va), name


# ================================================================== mul_vec
@pytest.fixture(scope="module")
def int_matrix():
    return matrix_input(ints=True)


def expected_product(dsa, hip, A, xk, xv, tr):
    """dynamicsparsevec(*A.mul((xk, xv)), n=size): today's route through host pairs"""
    yi, yv = A.mul((xk, xv), transpose=tr)
    m, n = A.size()
    return dsa.dynamicsparsevec(yi, yv, n=(n if tr else m), binding=hip), yi, yv


@pytest.mark.gpu
@pytest.mark.parametrize("tr", [False, True], ids=["plain", "transposed"])
def test_mul_vec_small_integers_bitwise(dsa, hip, int_matrix, tr):
    I, J, V = int_matrix
    A = dsa.dynamicsparse(I, J, V, M_ROWS, M_COLS, binding=hip)
    ncols = M_ROWS if tr else M_COLS
    seen = set()
    for name, (xk, xv, forced) in x_cases(tr).items():
        if name == "xdriven_edge":
            assert len(xk) * 8 < ncols <= (len(xk) + 1) * 8 and (tr or len(xk) == 24)
        if name == "gather_edge":
            assert (len(xk) - 1) * 8 < ncols <= len(xk) * 8 and (tr or len(xk) == 25)
        xd = rule_xdriven(len(xk), ncols, forced)
        assert xd == (not ("gather" in name or name == "dense_x") or "forced" in name), name
        seen.add((xd, forced))
        if "wide" in name:
            assert xk.max() >= W31
        if forced:
            assert xk.min() < 1 and xk.max() > ncols
        x = mkvec(dsa, hip, xk, xv)
        assert np.array_equal(x.nonzeros()[0], xk)
        want, yi, yv = expected_product(dsa, hip, A, xk, xv, tr)
        wr, ws, _ = model_mul(I, J, V, xk, xv, tr)
        assert np.array_equal(yi, wr) and same_values(yv, ws), name            # integers: one sum in any order
        got = (A.T if tr else A).mul_vec(x)
        assert same_layout(got, want), name
        assert len(got) == (M_COLS if tr else M_ROWS), name
        if name.startswith("all_miss") or name == "empty":
            assert got.nnz() == 0
        assert clean(x) and clean(got), name
        # x was only read, and its alternate buffer is its own again: a write, then the pairs
        x[5000] = 2.5
        k2, v2 = x.nonzeros()
        i = np.searchsorted(k2, 5000)
        assert k2[i] == 5000 and v2[i] == 2.5 and len(k2) == len(np.union1d(xk, [5000])), name
        assert np.array_equal(np.delete(k2, i), xk[xk != 5000]), name
    assert seen == {(True, False), (False, False), (True, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("tr", [False, True], ids=["plain", "transposed"])
def test_mul_vec_queued_writes_fill_mode_and_nonfinite(dsa, hip, int_matrix, tr):
    I, J, V = int_matrix
    ncols = M_ROWS if tr else M_COLS
    cases = x_cases(tr)
    # queued single writes on x and on the matrix, never flushed by a read in between
    for which in ("xdriven_edge", "gather_edge"):
        xk, xv, _ = cases[which]
        A = dsa.dynamicsparse(I, J, V, M_ROWS, M_COLS, binding=hip)
        x = mkvec(dsa, hip, xk[:-3], xv[:-3])
        for k, v in zip(xk[-3:].tolist(), xv[-3:].tolist()):
            x[k] = v if v != 0.0 else 1.0
        xv2 = xv.copy()
        xv2[-3:][xv2[-3:] == 0.0] = 1.0
        A[int(I[0]), int(J[0])] = 0.0                 # a queued delete and two queued inserts
        A[M_ROWS, M_COLS] = 5.0
        A[1, 1] = -2.0
        got = (A.T if tr else A).mul_vec(x)
        want, _, _ = expected_product(dsa, hip, A, xk, xv2, tr)
        assert same_layout(got, want), which
        I2, J2, V2 = A.findnz()
        wr, ws, _ = model_mul(np.asarray(I2), np.asarray(J2), np.asarray(V2), xk, xv2, tr)
        gk, gv = got.nonzeros()
        assert np.array_equal(gk, wr) and same_values(gv, ws), which
        assert clean(got) and clean(x)
    # fill mode
    Fm = dsa.dynamicsparse(binding=hip)
    Fm.addrow(1, [1, 2], [1.0, 2.0])
    x = mkvec(dsa, hip, [1], [1.0])
    with pytest.raises(dsa.DsaError) as e:
        (Fm.T if tr else Fm).mul_vec(x)
    assert e.value.code == 5                          # DSA_EMODE
    # a stored Inf of A in a column x stores (0 * Inf = NaN, Inf * 2 = Inf) and in one it does not (never read): both strategies
    live = np.setdiff1d(np.arange(1, ncols + 1), np.arange(*(EMPTY_ROWS if tr else EMPTY_COLS)) )
    c_in, c_zero, c_out = int(live[3]), int(live[10]), int(live[20])
    extra = [(7, c_in, np.inf), (8, c_zero, -np.inf), (9, c_out, np.inf), (7, c_out, np.nan)]
    cells = {(int(i), int(j)): float(v) for i, j, v in zip(I, J, V)}
    for r, c, v in extra:
        cells[(c, r) if tr else (r, c)] = v
    Ii = np.array([k[0] for k in cells], dtype=np.int64)
    Jj = np.array([k[1] for k in cells], dtype=np.int64)
    Vv = np.array(list(cells.values()))
    A = dsa.dynamicsparse(Ii, Jj, Vv, M_ROWS, M_COLS, binding=hip)
    for nx in ((ncols - 1) // 8 - 2, (ncols - 1) // 8 + 6):
        others = np.setdiff1d(live, [c_in, c_zero, c_out])[5:5 + nx]
        xk = np.sort(np.concatenate([others, [c_in, c_zero]])).astype(np.int64)
        xv = np.full(len(xk), 2.0)
        xv[xk == c_zero] = 0.0
        assert rule_xdriven(len(xk), ncols, False) == (nx < (ncols - 1) // 8)
        x = mkvec(dsa, hip, xk, xv)
        got = (A.T if tr else A).mul_vec(x)
        want, yi, yv = expected_product(dsa, hip, A, xk, xv, tr)
        wr, ws, _ = model_mul(Ii, Jj, Vv, xk, xv, tr)
        assert np.array_equal(yi, wr) and same_values(yv, ws)
        assert same_layout(got, want)
        gk, gv = got.nonzeros()
        assert np.isposinf(gv[gk == 7][0]) and np.isnan(gv[gk == 8][0])
        assert 9 not in gk.tolist() or np.isfinite(gv[gk == 9][0])            # row 9 is touched only through finite cells, if at all


@pytest.mark.gpu
@pytest.mark.parametrize("tr", [False, True], ids=["plain", "transposed"])
def test_mul_vec_normal_values_within_the_rounding_bound(dsa, hip, tr):
    I, J, V = matrix_input(ints=False, seed=4106)
    A = dsa.dynamicsparse(I, J, V, M_ROWS, M_COLS, binding=hip)
    for name, (xk, xv, forced) in x_cases(tr, ints=False).items():
        x = mkvec(dsa, hip, xk, xv)
        got = (A.T if tr else A).mul_vec(x)
        want, yi, yv = expected_product(dsa, hip, A, xk, xv, tr)
        gk, gv, go = got.export_layout()
        wk, wv, wo = want.export_layout()
        assert got.info()["capacity"] == want.info()["capacity"] and np.array_equal(go, wo), name
        m = wo.astype(bool)
        assert np.array_equal(gk[m], wk[m]) and len(got) == len(want), name
        wr, _, prods = model_mul(I, J, V, xk, xv, tr)
        assert np.array_equal(gk[m], wr), name
        worst = F(0)
        for r, a, b in zip(wr.tolist(), gv[m].tolist(), wv[m].tolist()):
            s, mag = exact(prods[r])
            n = len(prods[r])
            assert abs(F(a) - s) <= gamma(n) * mag and abs(F(b) - s) <= gamma(n) * mag, (name, r)
            assert abs(F(a) - F(b)) <= 2 * gamma(n) * mag, (name, r)
            if mag:
                worst = max(worst, abs(F(a) - F(b)) / (2 * gamma(n) * mag))
        print("%s %s: %d rows, largest |mul_vec - mul| / bound = %.3g" % ("transposed" if tr else "plain", name, len(wr), float(worst)))


# ================================================================== reduce / dot
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, VO_PASS_CELLS + 1, 40000, 46000]


def reduce_models(v):
    v = np.asarray(v, dtype=np.float64)
    return {"sum": v, "abssum": np.abs(v), "sqsum": v * v}


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_reduce_and_dot_by_length(dsa, hip, n):
    """sum, sum |v|, sum v*v, max |v|, dot with itself, with a longer and with a shorter operand, at every length of the driving
    operand that changes the shape of a stage: accuracy against the exact value, the same bits twice, dot(a, a) == sqsum"""
    k, v = vec_input(n, 500 + n % 97)
    a = mkvec(dsa, hip, k, v)
    cap = a.info()["capacity"]
    assert (cap > SMALL) == (n in (VO_PASS_CELLS + 1, 46000)) and (n != 40000 or cap == SMALL)
    for kind, terms in reduce_models(v).items():
        got = a.reduce(kind)
        assert within_bound(got, terms), (kind, n)
        assert bits([a.reduce(kind)])[0] == bits([got])[0], (kind, n)
    assert a.reduce("absmax") == (np.max(np.abs(v)) if n else 0.0)
    assert a.sum() == a.reduce("sum") and a.norm(1) == a.reduce("abssum") and a.norm(np.inf) == a.reduce("absmax")
    assert a.norm(2) == float(np.sqrt(a.reduce("sqsum")))
    assert bits([a.dot(a)])[0] == bits([a.reduce("sqsum")])[0], n               # one shape
    if n == 0:
        assert a.sum() == 0.0 and not np.signbit(a.sum()) and a.dot(a) == 0.0
    # the other operand: every key of a and as many in between (longer), every second key of a (shorter)
    rng = np.random.default_rng(900 + n % 89)
    lk = np.union1d(k, k + 1).astype(np.int64)
    longer = mkvec(dsa, hip, lk, rng.standard_normal(len(lk)))
    sk = k[::2]
    shorter = mkvec(dsa, hip, sk, rng.standard_normal(len(sk)))
    for other, ok_, name in ((longer, lk, "longer"), (shorter, sk, "shorter")):
        ov = other.nonzeros()[1]
        common, ia, ib = np.intersect1d(k, ok_, return_indices=True)
        terms = v[ia] * ov[ib]
        d1, d2 = a.dot(other), other.dot(a)
        assert within_bound(d1, terms) and within_bound(d2, terms), (name, n)
        # the driving operand is the shorter one whichever way round it is given: the same lanes, the same bits
        if len(k) != len(ok_):
            assert bits([d1])[0] == bits([d2])[0], (name, n)
        assert bits([a.dot(other)])[0] == bits([d1])[0], (name, n)


@pytest.mark.gpu
def test_dot_match_positions_roles_and_widths(dsa, hip):
    rng = np.random.default_rng(4201)
    n = 300
    k, v = vec_input(n, 31, step=4)
    a = mkvec(dsa, hip, k, v)

    def other(keys):
        keys = np.asarray(keys, dtype=np.int64)
        vals = rng.standard_normal(len(keys))
        return mkvec(dsa, hip, keys, vals), keys, vals

    between = k[:-1] + 2                              # keys a does not store
    shapes = {
        "first_only": np.concatenate([[k[0]], between[:200]]),
        "last_only": np.concatenate([between[:200], [k[-1]]]),
        "first_and_last": np.concatenate([[k[0]], between[:150], [k[-1]]]),
        "none": between,
        "all": k,
        "b_below_a": np.arange(-400, 0),
        "b_above_a": k[-1] + np.arange(1, 50),
    }
    for name, keys in shapes.items():
        b, bk, bv = other(np.sort(keys))
        common, ia, ib = np.intersect1d(k, bk, return_indices=True)
        assert len(common) == {"first_only": 1, "last_only": 1, "first_and_last": 2, "none": 0, "all": n, "b_below_a": 0, "b_above_a": 0}[name]
        terms = v[ia] * bv[ib]
        d = a.dot(b)
        assert within_bound(d, terms), name
        assert bits([b.dot(a)])[0] == bits([d])[0] or len(bk) == n, name
        if len(common) == 0:
            assert d == 0.0 and not np.signbit(d), name
        if len(common) == 1:
            assert d == terms[0], name
    # the tie rule: equal lengths drive from a.  dot(a, b) sums fl(a_k b_k) over a's lanes, dot(b, a) over b's lanes: with keys that
    # sit at other packed positions in the two operands the two orders differ, and each equals its own model of the lane tree
    bk = np.concatenate([k[:100], k[100:] + 1])       # 100 matches, all at a's and b's first positions -> same lanes either way
    b, bk, bv = other(bk)
    assert len(bk) == n
    assert bits([a.dot(b)])[0] == bits([b.dot(a)])[0]
    shifted = np.concatenate([np.arange(-50, 0), k[:n - 50]])                   # the matches sit 50 positions further right in b
    b2, b2k, b2v = other(shifted)
    common, ia, ib = np.intersect1d(k, b2k, return_indices=True)
    terms = v[ia] * b2v[ib]
    dab, dba = a.dot(b2), b2.dot(a)
    assert within_bound(dab, terms) and within_bound(dba, terms)
    assert bits([dab])[0] == bits([lane_tree_sum(place(terms, ia, n))])[0]       # driven by a: term i at a's position ia[i]
    assert bits([dba])[0] == bits([lane_tree_sum(place(terms, ib, n))])[0]       # driven by b2 when b2 is the first operand
    # mixed physical key widths, either role
    wk = np.concatenate([k[::3], [W31 + 1, W40]])
    w, wk, wv = other(wk)
    assert wk.max() >= W31 > k.max()
    common, ia, ib = np.intersect1d(k, wk, return_indices=True)
    terms = v[ia] * wv[ib]
    assert within_bound(a.dot(w), terms) and bits([a.dot(w)])[0] == bits([w.dot(a)])[0]
    assert within_bound(w.reduce("sum"), wv)
    # small integers: exact equality with numpy
    ik, iv = vec_input(1000, 32, ints=True)
    jk, jv = vec_input(700, 33, step=6, ints=True)
    vi, vj = mkvec(dsa, hip, ik, iv), mkvec(dsa, hip, jk, jv)
    common, ia, ib = np.intersect1d(ik, jk, return_indices=True)
    assert len(common) > 100
    assert vi.dot(vj) == float(np.dot(iv[ia], jv[ib])) == vj.dot(vi)
    assert vi.sum() == float(iv.sum()) and vi.norm(1) == float(np.abs(iv).sum()) and vi.reduce("sqsum") == float((iv * iv).sum())
    assert vi.norm(np.inf) == float(np.abs(iv).max())


def place(terms, positions, n):
    out = np.zeros(((n + 63) // 64) * 64)
    out[np.asarray(positions)] = terms
    return out


def lane_tree_sum(t):
    """the documented order of the reduction for up to VO_PASS_CELLS terms (csrc/vecops.hip): per 64 terms the xor butterfly
    o = 32 .. 1, the partials one per stage-2 thread, the 64 threads of a stage-2 wave by the same butterfly, the 16 wave words again"""
    def butterfly(w):
        w = np.array(w, dtype=np.float64)
        o = 32
        while o:
            w = w + w[np.arange(64) ^ o]
            o >>= 1
        return w[0]
    t = np.asarray(t, dtype=np.float64)
    assert len(t) % 64 == 0 and len(t) <= VO_PASS_CELLS
    partial = np.zeros(VO_FIN_THREADS)
    for p in range(len(t) // 64):
        partial[p] = 0.0 + butterfly(t[64 * p:64 * p + 64])
    waves = np.zeros(64)
    for w in range(VO_FIN_THREADS // 64):
        waves[w] = butterfly(partial[64 * w:64 * w + 64])
    return butterfly(waves)


@pytest.mark.gpu
def test_reduce_same_bits_across_layouts(dsa, hip):
    rng = np.random.default_rng(4202)
    for n in (777, 46000):
        k, v = vec_input(n, 41)
        a = mkvec(dsa, hip, k, v)
        b = mkvec(dsa, hip, k[::2], rng.standard_normal(len(k[::2])))
        kinds = ("sum", "abssum", "sqsum", "absmax")
        ref = {q: bits([a.reduce(q)])[0] for q in kinds}
        ref["dot"], ref["dot_r"] = bits([a.dot(b)])[0], bits([b.dot(a)])[0]

        def same(vec, what):
            lay = vec.export_layout()
            for q in kinds:
                assert bits([vec.reduce(q)])[0] == ref[q], (what, q, n)
            assert bits([vec.dot(b)])[0] == ref["dot"] and bits([b.dot(vec)])[0] == ref["dot_r"], (what, n)
            return lay

        base = same(a, "as built")
        # the same content in another insertion order: batches of single writes in a shuffled order leave another slot layout
        p = rng.permutation(n)
        other = mkvec(dsa, hip, k[p[:n // 2]], v[p[:n // 2]], n=int(k.max()))
        other.set_batch(k[p[n // 2:]], v[p[n // 2:]])
        assert other == a
        lay = same(other, "other insertion order")
        assert not np.array_equal(lay[2], base[2]) or n == 777               # (a small one may land on the same slots)
        a.b.call("vec_dev_relayout", a.h, 1)                                   # all cells packed to the left
        lay = same(a, "relayout 1")
        assert not np.array_equal(lay[2], base[2])
        a.rebalance_root()
        same(a, "rebalance_root")
        a.b.call("vec_dev_relayout", a.h, 3)                                   # capacity doubled
        assert a.info()["capacity"] == 2 * len(base[2])
        same(a, "relayout 3")


@pytest.mark.gpu
def test_reduce_special_values(dsa, hip):
    k = np.arange(1, 201, dtype=np.int64)
    base = np.random.default_rng(4203).standard_normal(200)
    for special, at in ((np.nan, 0), (np.nan, 199), (np.inf, 77), (-np.inf, 130)):
        v = base.copy()
        v[at] = special
        a = mkvec(dsa, hip, k, v)
        one = mkvec(dsa, hip, k, np.ones(200))
        with np.errstate(invalid="ignore"):
            assert same_values([a.sum()], [np.sum(v)]) and same_values([a.norm(1)], [np.sum(np.abs(v))])
            assert same_values([a.norm(np.inf)], [np.max(np.abs(v))])          # NaN propagates in max |v|, Inf is the maximum
            assert same_values([a.reduce("sqsum")], [np.sum(v * v)])
            assert same_values([a.dot(one)], [np.sum(v)]) and same_values([one.dot(a)], [np.sum(v)])
    # Inf - Inf, and NaN beside Inf in max |v|
    a = mkvec(dsa, hip, [1, 2, 3], [np.inf, -np.inf, 1.0])
    assert np.isnan(a.sum()) and a.norm(np.inf) == np.inf and a.norm(1) == np.inf
    a = mkvec(dsa, hip, [1, 2, 3], [np.inf, np.nan, 1.0])
    assert np.isnan(a.norm(np.inf))
    # negative zeros: every sum starts at +0.0 and every wave is padded with +0.0
    z = mkvec(dsa, hip, [4, 8, 9], [0.0, 0.0, 0.0])
    z.set_batch([4, 8], [5.0, 6.0])
    nz = dsa.dynamicsparsevec_dev(dev([4, 8], np.int64), dev([-0.0, -0.0], np.float64), binding=hip)
    assert np.all(np.signbit(nz.nonzeros()[1])) and nz.nnz() == 2
    for q in ("sum", "abssum", "sqsum", "absmax"):
        r = nz.reduce(q)
        assert r == 0.0 and not np.signbit(r), q
    d = nz.dot(z)
    assert d == 0.0 and not np.signbit(d)
    m = dsa.dynamicsparsevec_dev(dev([1, 2], np.int64), dev([-0.0, 3.0], np.float64), binding=hip)
    assert m.sum() == 3.0 and m.norm(np.inf) == 3.0
    with pytest.raises(dsa.DsaArgumentError):
        hip.call("vec_reduce", m.h, 4, C.byref(C.c_double()))                 # the count kind: nnz() exists
    with pytest.raises(dsa.DsaArgumentError):
        m.reduce("count")


@pytest.mark.gpu
def test_dot_dense_and_to_dense(dsa, hip):
    import torch
    rng = np.random.default_rng(4204)
    for n, nx in ((0, 10), (1, 1), (300, 900), (46000, 3 * 46000)):
        k, v = vec_input(n, 51)
        a = mkvec(dsa, hip, k, v)
        if n:
            a[nx] = 1.25                              # a key at nx; vec_input starts at key 1
            k, v = a.nonzeros()
            assert k[0] == 1 and k[-1] == nx
        xh = rng.standard_normal(nx)
        x = dev(xh, np.float64)
        got = a.dot(x)
        assert within_bound(got, v * xh[k - 1]), n
        assert bits([a.dot(x)])[0] == bits([got])[0]
        ones = torch.ones(nx, dtype=torch.float64, device="cuda")
        assert bits([a.dot(ones)])[0] == bits([a.sum()])[0], n                 # v_k * 1.0 is v_k: the same terms in the same lanes
        dense = torch.full((nx + 2,), -5.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        a.to_dense_dev(dense.data_ptr() + 8, nx)
        a.sync()
        want = np.zeros(nx)
        want[k - 1] = v
        h = dense.cpu().numpy()
        assert h[0] == -5.5 and h[-1] == -5.5 and np.array_equal(bits(h[1:-1]), bits(want)), n
    # keys outside 1..nx: at nx + 1 and at 0 (or below): DSA_EBOUNDS, the destination untouched
    for bad in ([1, 5, 101], [-2, 5, 100], [0, 5, 100]):
        a = dsa.dynamicsparsevec_dev(dev(bad, np.int64), dev([1.0, 2.0, 3.0], np.float64), binding=hip)
        x = torch.ones(100, dtype=torch.float64, device="cuda")
        with pytest.raises(dsa.DsaBoundsError):
            a.dot(x)
        dense = torch.full((100,), -5.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(dsa.DsaBoundsError):
            a.to_dense_dev(dense.data_ptr(), 100)
        a.sync()
        assert bool((dense == -5.5).all()), bad
    ok = dsa.dynamicsparsevec_dev(dev([1, 5, 100], np.int64), dev([1.0, 2.0, 3.0], np.float64), binding=hip)
    assert ok.dot(torch.ones(100, dtype=torch.float64, device="cuda")) == 6.0
    # mixed into a product: mat @ densified x equals mul_vec(x) densified
    I, J, V = matrix_input(ints=True)
    A = dsa.dynamicsparse(I, J, V, M_ROWS, M_COLS, binding=hip)
    xk, xv, _ = x_cases(False)["gather_edge"]
    xs = mkvec(dsa, hip, xk, xv)
    xd = torch.empty(M_COLS, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    xs.to_dense_dev(xd.data_ptr(), M_COLS)
    xs.sync()
    y = A.matmul(xd)
    yd = torch.empty(M_ROWS, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    yv = A.mul_vec(xs)
    yv.to_dense_dev(yd.data_ptr(), M_ROWS)
    yv.sync()
    assert np.array_equal(y.cpu().numpy(), yd.cpu().numpy())                   # small integers: exact in any order
