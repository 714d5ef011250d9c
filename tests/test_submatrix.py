"""Submatrix export A[I, J]: both key lists selected and renumbered on the device (include/dsa.h: dsa_mat_submatrix_compressed[_dev];
csrc/submatrix.hip).

Expected arrays never come from the kernels under test: the ORACLE matrix goes through the same operations, `Expect(...).select(outer)`
(test_select.py) gives the selected partitions of its full CSC / CSR, and numpy filters and renumbers their cells with a dict from
inner key to position.  Comparisons are exact: ptr and idx equal, values equal as uint64 bit patterns.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_select import (COLMAJOR, EARG, EBOUNDS, ECAP, EMODE, LONG_COLS, MATRIX_CASES, OWNER_LENGTHS, ROOT, ROWMAJOR, Expect, _assert_same,
                         _in_fill_mode, long_case, owner_search_selections)  # noqa: F401  (long_case: the module-scoped fixture,
#                                                                              instantiated once more for this module)

NAMES = ("mat_submatrix_compressed", "mat_submatrix_compressed_dev")


def expect_sub(E, outer, inner):
    """A[inner, outer] / A[outer, inner] of the oracle matrix at base 0: the selected partitions, filtered and renumbered in numpy"""
    ptr, idx, val = E.select(outer)
    pos = {int(k): p for p, k in enumerate(np.asarray(inner, dtype=np.int64).tolist())}
    assert len(pos) == len(inner)
    new = np.fromiter((pos.get(k, -1) for k in (idx + 1).tolist()), dtype=np.int64, count=len(idx))
    keep = new >= 0
    kept_before = np.concatenate(([0], np.cumsum(keep))).astype(np.int64)
    return kept_before[ptr], new[keep], val[keep].copy()


def with_base(exp, base):
    return exp[0] + base, exp[1] + base, exp[2]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_submatrix_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NAMES:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name


def test_oracle_binding_does_not_have_them(dsa, oracle):
    assert oracle.prefix == "ora"
    for name in NAMES:
        assert not oracle.has(name)
        assert name not in dsa.Binding.SIGNATURES


def test_submatrix_needs_the_product_library(dsa, oracle):
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    for call in (lambda: a.submatrix([1], [1]), lambda: a.submatrix([1], [2], layout="csc"), lambda: a.count_submatrix([1], [1], "csr"),
                 lambda: a.submatrix_compressed_dev(COLMAJOR, 0, 0, 0, 0, 0, 0, 0, 0)):
        with pytest.raises(dsa.DsaArgumentError):
            call()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _sub_dev(a, o, outer, inner, bits, base):
    """dsa_mat_submatrix_compressed_dev into torch tensors (the count-only call, then the one that fits), back to numpy"""
    import torch
    dt = torch.int32 if bits == 32 else torch.int64
    d_out = torch.from_numpy(np.ascontiguousarray(outer, dtype=np.int64)).to("cuda")
    d_in = torch.from_numpy(np.ascontiguousarray(inner, dtype=np.int64)).to("cuda")
    no, ni = d_out.numel(), d_in.numel()
    ptr = torch.full((no + 1,), -7, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    total, fits = a.submatrix_compressed_dev(o, d_out.data_ptr(), no, d_in.data_ptr(), ni, ptr.data_ptr(), 0, 0, 0, index_bits=bits, base=base)
    a.sync()
    assert fits == (total == 0)
    ptr0 = ptr.cpu().numpy()
    idx = torch.full((max(total, 1),), -7, dtype=dt, device="cuda")
    val = torch.full((max(total, 1),), -7.0, dtype=torch.float64, device="cuda")
    ptr.fill_(-7)
    torch.cuda.synchronize()
    got, fits = a.submatrix_compressed_dev(o, d_out.data_ptr(), no, d_in.data_ptr(), ni, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(),
                                           total, index_bits=bits, base=base)
    a.sync()
    assert fits and got == total
    assert np.array_equal(ptr.cpu().numpy(), ptr0)          # the count-only call leaves the same ptr
    return ptr0, idx[:got].cpu().numpy(), val[:got].cpu().numpy()


def _sub_host(a, o, outer, inner, base):
    if o == COLMAJOR:
        return a.submatrix(inner, outer, layout="csc", base=base)
    return a.submatrix(outer, inner, layout="csr", base=base)


def _check(dsa, a, E, o, outer, inner, bits=(32, 64), bases=(0, 1)):
    """every combination of index width and base through the _dev entry, every base through the host entry"""
    outer, inner = np.asarray(outer, dtype=np.int64), np.asarray(inner, dtype=np.int64)
    if not E.in_size(outer):
        for call in (lambda: _sub_dev(a, o, outer, inner, 64, 0), lambda: _sub_host(a, o, outer, inner, 0)):
            with pytest.raises(dsa.DsaBoundsError):
                call()
        return None
    exp = expect_sub(E, outer, inner)
    for base in bases:
        for b in bits:
            _assert_same(_sub_dev(a, o, outer, inner, b, base), with_base(exp, base))
        _assert_same(_sub_host(a, o, outer, inner, base), with_base(exp, base))
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_cases_exact(dsa, hip, oracle, sc):
    a = run_scenario(dsa, hip, sc)
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        for o in (COLMAJOR, ROWMAJOR):
            with pytest.raises(dsa.DsaError) as ei:
                a.submatrix_compressed_dev(o, 0, 0, 0, 0, 0, 0, 0, 0)
            assert ei.value.code == EMODE
            with pytest.raises(dsa.DsaError) as ei:
                a.submatrix([1], [1], layout="csc" if o == COLMAJOR else "csr")
            assert ei.value.code == EMODE
        return
    for o in (COLMAJOR, ROWMAJOR):
        E = Expect(b, o)
        outer = np.arange(1, E.dim_out + 1, dtype=np.int64)
        inner = np.arange(1, E.dim_in + 1, dtype=np.int64)
        exp = _check(dsa, a, E, o, outer, inner)
        if exp is not None:                                 # every key of both sides, in order: the full export of size(m)
            _assert_same(exp, E.select(outer))
        _check(dsa, a, E, o, outer, inner[::-1])
        _check(dsa, a, E, o, outer[::2], inner[::2])


def _inner_lists(E, long_key, dim_in, dead, rng, pow2):
    """the inner lists of the long-partition test for one orientation; `long_key` is the outer key whose keys give the percentiles"""
    keys = E.select([long_key])[1] + 1
    p10, p90 = np.percentile(keys, 10), np.percentile(keys, 90)
    every = np.arange(1, dim_in + 1, dtype=np.int64)
    used = np.zeros(dim_in + 1, dtype=bool)
    used[E.idx + 1] = True
    unused = every[~used[1:]]                               # keys of the inner side that no cell uses
    unused = unused[unused != dead]
    assert len(unused) >= 1
    return {
        "all": every,
        "tails": every[(every < p10) | (every > p90)],
        "single": keys[len(keys) // 2:len(keys) // 2 + 1],
        "absent": np.array([dead, unused[0]], dtype=np.int64),
        "random_permuted": rng.permutation(dim_in)[:dim_in // 2] + 1,
        "multiples_of_64": every[every % 64 == 0],
        "power_of_two": rng.permutation(dim_in)[:pow2] + 1,
    }


@pytest.mark.gpu
def test_long_partition_and_edge_keys(dsa, long_case):
    a, E, dead_row = long_case
    assert E[COLMAJOR].counts(LONG_COLS).tolist() == [5004, 38, 28, 0, 0, 5004, 25, 19, 38]      # the input is the one the cases were chosen on
    rng = np.random.default_rng(31)
    # colmajor: column 150 spans several 2048-slot work items; "tails" leaves its middle items without a kept cell
    lists = _inner_lists(E[COLMAJOR], 150, 6000, dead_row, rng, 2048)
    assert len(lists["random_permuted"]) == 3000 and len(lists["power_of_two"]) == 2048
    for name, inner in lists.items():
        exp = _check(dsa, a, E[COLMAJOR], COLMAJOR, LONG_COLS, inner)
        if name == "all":
            _assert_same(exp, E[COLMAJOR].select(LONG_COLS))
        if name == "absent":
            assert len(exp[1]) == 0 and not exp[0].any()
        if name == "single":
            assert len(exp[1]) >= 2                         # column 150 is listed twice
        assert np.array_equal(a.count_submatrix(inner, LONG_COLS, "csc"), np.diff(exp[0])), name
    # rowmajor: the same kinds of lists over the 300 columns (40 is a deleted column, 17 was never written; 256 keys for the power
    # of two); rows with repeats, the deleted row, first and last row
    rows = np.concatenate(([6000, 1, dead_row, 77, 77, 3], rng.integers(1, 6001, 300)))
    busiest = int(np.argmax(np.diff(E[ROWMAJOR].ptr))) + 1
    lists = _inner_lists(E[ROWMAJOR], busiest, 300, 40, rng, 256)
    assert lists["absent"].tolist() == [40, 17]
    for name, inner in lists.items():
        exp = _check(dsa, a, E[ROWMAJOR], ROWMAJOR, rows, inner)
        if name == "absent":
            assert len(exp[1]) == 0
        assert np.array_equal(a.count_submatrix(rows, inner, "csr"), np.diff(exp[0])), name


@pytest.mark.gpu
def test_empty_lists_and_scan_carry(dsa, long_case):
    a, E, _ = long_case
    none = np.zeros(0, dtype=np.int64)
    some_rows = np.arange(1, 6001, 7, dtype=np.int64)
    for o, outer, inner in ((COLMAJOR, LONG_COLS, some_rows), (ROWMAJOR, [6000, 77, 77, 3], [150, 1, 300])):
        for out_l, in_l in ((none, inner), (outer, none), (none, none)):
            exp = _check(dsa, a, E[o], o, out_l, in_l)
            assert len(exp[1]) == 0 and len(exp[0]) == len(out_l) + 1
    assert len(a.count_submatrix([], [1, 2], "csr")) == 0
    # more than one 8192-entry step of the scan over the outer keys (20000 of them); column 150 comes about 67 times, 3 work items each
    outer = np.random.default_rng(22).integers(1, 301, 20000)
    inner = np.random.default_rng(31).permutation(6000)[:3000] + 1
    _check(dsa, a, E[COLMAJOR], COLMAJOR, outer, inner, bits=(32, 64), bases=(1,))
    for k in (8192, 8193):                                  # one full step of the prefix loop, and one entry more
        _check(dsa, a, E[COLMAJOR], COLMAJOR, outer[:k], inner, bits=(64,), bases=(0,))


@pytest.mark.gpu
def test_owner_search_boundaries(dsa, long_case):
    """the outer lists of test_select.py's case of this name (the owner search is the same function), the inner list every other row"""
    a, E, _ = long_case
    inner = np.arange(1, 6001, 2, dtype=np.int64)
    for n in OWNER_LENGTHS:
        for outer in owner_search_selections(E[COLMAJOR], n):
            _check(dsa, a, E[COLMAJOR], COLMAJOR, outer, inner, bits=(32, 64), bases=(0,))


@pytest.mark.gpu
def test_wide_inner_keys(dsa, hip, oracle):
    big = (1 << 31) + 5
    I = np.array([1, 2, 3, 3, 4], dtype=np.int64)
    J = np.array([1, 7, 2, big, big], dtype=np.int64)
    V = np.array([1.5, -2.0, 3.25, 4.0, 0.125])
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    E = Expect(b, ROWMAJOR)
    outer, inner = [3, 4, 1, 3, 2], [big, 2, 7]
    exp = _check(dsa, a, E, ROWMAJOR, outer, inner)         # index_bits 32 included: only ninner must fit, not n
    assert exp[0].tolist() == [0, 2, 3, 3, 5, 6]
    assert exp[1].tolist() == [1, 0, 0, 1, 0, 2]
    assert exp[2].tolist() == [3.25, 4.0, 0.125, 3.25, 4.0, -2.0]
    with pytest.raises(dsa.DsaBoundsError):
        _sub_dev(a, ROWMAJOR, outer, [big + 1, 2], 64, 0)


def _raw_dev(hip, a, o, outer, inner, cap, with_arrays, base=0):
    """the entry point itself: (rc, nnz_out, ptr, idx, val) with -7 sentinels in every output"""
    import torch
    d_out = torch.from_numpy(np.ascontiguousarray(outer, dtype=np.int64)).to("cuda")
    d_in = torch.from_numpy(np.ascontiguousarray(inner, dtype=np.int64)).to("cuda")
    ptr = torch.full((len(outer) + 1,), -7, dtype=torch.int64, device="cuda")
    idx = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
    val = torch.full((max(cap, 1),), -7.0, dtype=torch.float64, device="cuda")
    got = C.c_int64(-1)
    torch.cuda.synchronize()
    rc = hip._mat_submatrix_compressed_dev(a.h, o, 64, base, C.c_void_p(d_out.data_ptr()), len(outer), C.c_void_p(d_in.data_ptr()),
                                           len(inner), C.c_void_p(ptr.data_ptr()), C.c_void_p(idx.data_ptr() if with_arrays else None),
                                           C.c_void_p(val.data_ptr() if with_arrays else None), cap, C.byref(got))
    a.sync()
    torch.cuda.synchronize()
    return rc, got.value, ptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()


@pytest.mark.gpu
def test_capacity_protocol(dsa, hip, long_case):
    a, E, dead_row = long_case
    inner = np.random.default_rng(31).permutation(6000)[:3000] + 1
    exp = with_base(expect_sub(E[COLMAJOR], LONG_COLS, inner), 1)
    total = len(exp[1])
    assert total > 2048
    rc, got, ptr, idx, val = _raw_dev(hip, a, COLMAJOR, LONG_COLS, inner, total - 1, True, base=1)
    assert rc == ECAP and got == total
    assert np.array_equal(ptr, exp[0]) and (idx == -7).all() and (val == -7.0).all()
    rc, got, ptr, idx, val = _raw_dev(hip, a, COLMAJOR, LONG_COLS, inner, 0, False, base=1)
    assert rc == ECAP and got == total
    assert np.array_equal(ptr, exp[0]) and (idx == -7).all() and (val == -7.0).all()
    rc, got, ptr, idx, val = _raw_dev(hip, a, COLMAJOR, LONG_COLS, [dead_row], 0, False, base=1)      # nothing kept: DSA_OK
    assert rc == 0 and got == 0 and np.array_equal(ptr, np.ones(len(LONG_COLS) + 1, dtype=np.int64))
    rc, got, ptr, idx, val = _raw_dev(hip, a, COLMAJOR, LONG_COLS, inner, total, True, base=1)        # exactly enough
    assert rc == 0 and got == total
    _assert_same((ptr, idx, val), exp)
    # the host form: ptr filled with DSA_ECAP as well
    outer = np.asarray(LONG_COLS, dtype=np.int64)
    inner = np.ascontiguousarray(inner, dtype=np.int64)
    hptr = np.full(len(outer) + 1, -7, dtype=np.int64)
    hidx = np.full(total, -7, dtype=np.int64)
    hval = np.full(total, -7.0)
    n_out = C.c_int64(-1)
    P64, PF = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    rc = hip._mat_submatrix_compressed(a.h, COLMAJOR, 1, outer.ctypes.data_as(P64), len(outer), inner.ctypes.data_as(P64), len(inner),
                                       hptr.ctypes.data_as(P64), hidx.ctypes.data_as(P64), hval.ctypes.data_as(PF), total - 1,
                                       C.byref(n_out))
    assert rc == ECAP and n_out.value == total
    assert np.array_equal(hptr, exp[0]) and (hidx == -7).all() and (hval == -7.0).all()


@pytest.mark.gpu
def test_bounds_and_arguments(dsa, hip, oracle, long_case):
    rng = np.random.default_rng(3)
    m, n = 50, 40
    I, J = rng.integers(1, m + 1, 300), rng.integers(1, n + 1, 300)
    I[0], J[0] = m, n
    V = rng.random(300) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    assert a.size() == b.size() == (m, n)
    _check(dsa, a, Expect(b, COLMAJOR), COLMAJOR, [n, 1, 2, 1], [m, 3, 1])

    def code_of(call):
        with pytest.raises(dsa.DsaError) as ei:
            call()
        return ei.value.code

    # a repeated inner key: next to each other, and far apart (another workgroup of the table fill)
    for inner in ([4, 4], [1, 9, 9, 3], [9, 1, 2, 3, 9]):
        assert code_of(lambda: _sub_dev(a, COLMAJOR, [1, 2], inner, 64, 0)) == EARG, inner
        assert code_of(lambda: a.submatrix(inner, [1, 2], layout="csc")) == EARG, inner
        assert code_of(lambda: a.submatrix([1, 2], inner, layout="csr")) == EARG, inner
    la, lE, _ = long_case
    far = np.random.default_rng(31).permutation(6000)[:3000] + 1
    far[-1] = far[0]
    assert code_of(lambda: _sub_dev(la, COLMAJOR, LONG_COLS, far, 32, 1)) == EARG
    assert code_of(lambda: la.count_submatrix(far, LONG_COLS, "csc")) == EARG
    # keys outside size(m)
    for bad in (0, m + 1, -3):
        assert code_of(lambda: _sub_dev(a, COLMAJOR, [1, 2], [1, bad, 2], 64, 0)) == EBOUNDS, bad
        assert code_of(lambda: a.submatrix([bad], [1, 2], layout="csc")) == EBOUNDS, bad
    assert code_of(lambda: a.submatrix([1], [n + 1], layout="csr")) == EBOUNDS
    for bad in (0, n + 1):
        assert code_of(lambda: _sub_dev(a, COLMAJOR, [1, bad, 2], [1, 2], 64, 0)) == EBOUNDS, bad
        assert code_of(lambda: a.submatrix([1, 2], [bad], layout="csc")) == EBOUNDS, bad
    assert code_of(lambda: a.submatrix([m + 1], [1], layout="csr")) == EBOUNDS
    import torch
    d_out = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    d_in = torch.tensor([3, 1, 2], dtype=torch.int64, device="cuda")
    ptr = torch.zeros(3, dtype=torch.int64, device="cuda")
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    good = dict(orientation=COLMAJOR, d_outer=d_out.data_ptr(), nouter=2, d_inner=d_in.data_ptr(), ninner=3, d_ptr=ptr.data_ptr(),
                d_idx=buf.data_ptr(), d_vals=buf.data_ptr(), cap=64, index_bits=64, base=0)
    assert a.submatrix_compressed_dev(**good)[1]
    for change in (dict(index_bits=16), dict(base=2), dict(base=-1), dict(orientation=2), dict(nouter=-1), dict(nouter=1 << 31),
                   dict(ninner=-1), dict(ninner=1 << 31), dict(d_ptr=0), dict(d_outer=0), dict(d_inner=0), dict(d_idx=0), dict(d_vals=0),
                   dict(cap=-1)):
        with pytest.raises(dsa.DsaArgumentError) as ei:
            a.submatrix_compressed_dev(**dict(good, **change))
        assert ei.value.code == EARG, change
    a.sync()
    # explicit m below the largest row key: a selection that takes the column holding that row is out of bounds, listed or not
    c, d = (dsa.dynamicsparse([1, 5, 2], [1, 2, 3], [1.0, 2.0, 3.0], m=3, n=3, binding=x) for x in (hip, oracle))
    assert c.size() == (3, 3)
    E = Expect(d, COLMAJOR)
    assert not E.in_size([2]) and E.in_size([3, 1])
    assert code_of(lambda: _sub_dev(c, COLMAJOR, [1, 2, 3], [1, 2, 3], 64, 0)) == EBOUNDS
    assert code_of(lambda: c.submatrix([1, 2], [2], layout="csc")) == EBOUNDS
    assert code_of(lambda: c.submatrix([5], [2], layout="csc")) == EBOUNDS          # the inner key itself lies outside 1..m
    _check(dsa, c, E, COLMAJOR, [3, 1, 3], [2, 1])


@pytest.mark.gpu
def test_read_only_layout_and_plan_untouched(dsa, hip, oracle):
    rng = np.random.default_rng(13)
    m = n = 20000
    I, J = rng.integers(1, m + 1, 200000), rng.integers(1, n + 1, 200000)
    V = rng.random(200000) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    x = rng.random(n) + 0.5
    for _ in range(3):
        a.mul(x)                                # the plan is built on the second product
    before = [a.export_layout(o) for o in (COLMAJOR, ROWMAJOR)]
    builds = a.info(ROWMAJOR)["stat_spmv_plan_builds"]
    for o in (COLMAJOR, ROWMAJOR):
        E = Expect(b, o)
        outer = rng.integers(1, E.dim_out + 1, 3000)
        inner = rng.permutation(E.dim_in)[:5000] + 1
        _check(dsa, a, E, o, outer, inner, bits=(32,), bases=(0,))
    for o in (COLMAJOR, ROWMAJOR):
        after = a.export_layout(o)
        for k in ("keys", "vals", "occ", "semaphores", "col_keys", "col_live"):
            assert np.array_equal(after[k].view(np.uint8), before[o][k].view(np.uint8)), (o, k)
    y = a.mul(x)
    assert a.info(ROWMAJOR)["stat_spmv_plan_builds"] == builds
    np.testing.assert_allclose(y, b.mul(x), rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_submatrix_torch_arrays_and_product(dsa, hip, oracle):
    import torch
    rng = np.random.default_rng(5)
    m, n, nnz = 3000, 2000, 40000
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.random(nnz) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    rows_sorted = np.sort(rng.permutation(m)[:700] + 1)
    cols_sorted = np.sort(rng.permutation(n)[:257] + 1)
    for layout, o in ((torch.sparse_csc, COLMAJOR), (torch.sparse_csr, ROWMAJOR)):
        E = Expect(b, o)
        # the outer side in any order, the inner side ascending
        rows = rows_sorted if o == COLMAJOR else rng.permutation(rows_sorted)
        cols = rng.permutation(cols_sorted) if o == COLMAJOR else cols_sorted
        outer, inner = (cols, rows) if o == COLMAJOR else (rows, cols)
        exp = expect_sub(E, outer, inner)
        for dt, as_given in ((torch.int32, lambda k: k.tolist()), (torch.int64, lambda k: torch.from_numpy(k).to("cuda"))):
            t = a.submatrix_torch(layout, as_given(rows), as_given(cols), index_dtype=dt)
            assert t.layout == layout and tuple(t.shape) == (len(rows), len(cols))
            comp, plain = (t.ccol_indices(), t.row_indices()) if o == COLMAJOR else (t.crow_indices(), t.col_indices())
            assert comp.dtype == dt and plain.dtype == dt and t.values().dtype == torch.float64
            _assert_same((comp.cpu().numpy(), plain.cpu().numpy(), t.values().cpu().numpy()), exp)
            ones = torch.ones((t.shape[1], 1), dtype=torch.float64, device="cuda")
            y = (t @ ones).squeeze(1).cpu().numpy()
            # the numpy product of the expected arrays with a vector of ones: the sum of each row of the submatrix
            ref = np.zeros(len(rows))
            if o == COLMAJOR:
                np.add.at(ref, exp[1], exp[2])
            else:
                np.add.at(ref, np.repeat(np.arange(len(rows)), np.diff(exp[0])), exp[2])
            np.testing.assert_allclose(y, ref, rtol=1e-12, atol=0)
        # torch expects sorted indices: an inner list that does not ascend strictly is refused
        for bad in (inner[::-1], np.concatenate((inner[:3], inner[2:5]))):
            with pytest.raises(dsa.DsaArgumentError):
                if o == COLMAJOR:
                    a.submatrix_torch(layout, bad, cols)
                else:
                    a.submatrix_torch(layout, rows, bad)
    t = a.submatrix_torch(torch.sparse_csc, [], [])
    assert tuple(t.shape) == (0, 0) and t.values().numel() == 0
    t = a.submatrix_torch(torch.sparse_csr, [5, 5, 1], [])
    assert tuple(t.shape) == (3, 0) and t.values().numel() == 0


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes(dsa, long_case):
    a, E, _ = long_case
    inner = np.random.default_rng(31).permutation(6000)[:3000] + 1
    outer = np.random.default_rng(22).integers(1, 301, 2000)
    first = _sub_dev(a, COLMAJOR, outer, inner, 64, 0)
    a.submatrix(inner[:100], [150], layout="csc")          # another table in the same scratch in between
    second = _sub_dev(a, COLMAJOR, outer, inner, 64, 0)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    _assert_same(first, expect_sub(E[COLMAJOR], outer, inner))
