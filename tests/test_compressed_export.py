"""Compressed export of a matrix (include/dsa.h: dsa_mat_to_compressed[_dev]; csrc/compress.hip).

Expected arrays come from `expected_compressed`, a numpy walk over the ORACLE's exported slot array (cut at semaphores, tombstones
skipped, partition ids mapped to their keys): it does not use the kernel.  Comparisons are exact: indices equal, values bitwise.
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from scenario import run_scenario

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "reference_cases.json")) as f:
    MATRIX_CASES = [c for c in json.load(f)["scenarios"] if c["kind"] == "matrix"]

COLMAJOR, ROWMAJOR = 0, 1


def expected_compressed(L, dim_out, base=0):
    """(ptr, idx, val) of one orientation from its exported layout: the cells of every live partition in slot order, the partition's
    key as the outer index, the cell's key - 1 + base as the inner one; ptr[k] = base + cells whose outer key is <= k."""
    occ = L["occ"].astype(bool)
    keys, vals = L["keys"][occ], L["vals"][occ]
    sems, col_keys = L["semaphores"], L["col_keys"]
    live = (sems != 0) & (L["col_live"] != 0)
    is_sem = keys == 0
    assert not occ.any() or is_sem[0], "a cell in front of the first semaphore"
    pid = vals[is_sem].astype(np.int64)                     # semaphore value = partition id (1-based)
    part = pid[np.cumsum(is_sem) - 1]                       # partition of every occupied slot
    cell = ~is_sem & live[part - 1]
    outer = col_keys[part[cell] - 1]
    assert np.all(np.diff(outer) >= 0)
    ptr = base + np.searchsorted(outer, np.arange(dim_out + 1), side="right").astype(np.int64)
    return ptr, keys[cell].astype(np.int64) - 1 + base, vals[cell].copy()


def _in_size(exp, dim_in, base=0):
    """whether every stored entry lies inside size(m) (otherwise the export fails with EBOUNDS)"""
    ptr, idx, _ = exp
    return ptr[0] == base and ptr[-1] == base + len(idx) and bool(np.all((idx >= base) & (idx < base + dim_in)))


def _assert_same(got, exp):
    assert np.array_equal(np.asarray(got[0], dtype=np.int64), exp[0])
    assert np.array_equal(np.asarray(got[1], dtype=np.int64), exp[1])
    assert np.array_equal(np.asarray(got[2], dtype=np.float64).view(np.uint64), exp[2].view(np.uint64))


def _expect(ora, o, base=0):
    m, n = ora.size()
    return expected_compressed(ora.export_layout(o), m if o == ROWMAJOR else n, base)


def _in_fill_mode(dsa, a):
    try:
        a.export_layout(0)
    except dsa.DsaError as e:
        if e.code == 5:        # EMODE
            return True
        raise
    return False


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_export_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in ("mat_to_compressed", "mat_to_compressed_dev"):
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name


def test_oracle_fixture_still_binds(oracle):
    assert oracle.prefix == "ora"
    assert not oracle.has("mat_to_compressed") and not oracle.has("mat_to_compressed_dev")


@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_helper_matches_the_views_on_the_oracle(dsa, oracle, sc):
    """the helper against the reference's own iteration (src/views.jl:15-40): CSC == col_view(1..n), CSR == row_view(1..m)"""
    a = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, a):
        return
    m, n = a.size()
    for o, dim, view in ((COLMAJOR, n, a.col_view), (ROWMAJOR, m, a.row_view)):
        ptr, idx, val = _expect(a, o)
        assert len(ptr) == dim + 1 and len(idx) == a.nnz()
        assert ptr[-1] - ptr[0] == sum(len(view(k)) for k in range(1, dim + 1))
        for k in range(1, dim + 1):
            cells = view(k)
            got = list(zip((idx[ptr[k - 1]:ptr[k]] + 1).tolist(), val[ptr[k - 1]:ptr[k]].tolist()))
            assert got == cells, (o, k, got, cells)


def test_export_needs_the_product_library(dsa, oracle):
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    with pytest.raises(dsa.DsaArgumentError):
        a.to_csr()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _export_dev(a, o, bits, base):
    """dsa_mat_to_compressed_dev into torch tensors, back to numpy"""
    import torch
    m, n = a.size()
    outer = m if o == ROWMAJOR else n
    nnz = a.nnz()
    dt = torch.int32 if bits == 32 else torch.int64
    ptr = torch.full((outer + 1,), -7, dtype=dt, device="cuda")
    idx = torch.full((max(nnz, 1),), -7, dtype=dt, device="cuda")
    val = torch.full((max(nnz, 1),), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    got = a.to_compressed_dev(o, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz, index_bits=bits, base=base)
    a.sync()
    assert got == nnz
    return ptr.cpu().numpy(), idx[:got].cpu().numpy(), val[:got].cpu().numpy()


def _check_all(dsa, a, ora, bits=(32, 64), bases=(0, 1)):
    m, n = ora.size()
    for o in (COLMAJOR, ROWMAJOR):
        dim_in = n if o == ROWMAJOR else m
        for base in bases:
            exp = _expect(ora, o, base)
            for b in bits:
                if _in_size(exp, dim_in, base):
                    _assert_same(_export_dev(a, o, b, base), exp)
                else:
                    with pytest.raises(dsa.DsaBoundsError):
                        _export_dev(a, o, b, base)
        exp = _expect(ora, o, 0)
        if _in_size(exp, dim_in):
            _assert_same(a.to_csc() if o == COLMAJOR else a.to_csr(), exp)
        else:
            with pytest.raises(dsa.DsaBoundsError):
                a.to_csc() if o == COLMAJOR else a.to_csr()


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_cases_exact(dsa, hip, oracle, sc):
    a = run_scenario(dsa, hip, sc)
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        for o in (COLMAJOR, ROWMAJOR):
            with pytest.raises(dsa.DsaError) as ei:
                a.to_compressed_dev(o, 0, 0, 0, 0)
            assert ei.value.code == 5           # EMODE
        return
    _check_all(dsa, a, b)


@pytest.mark.gpu
def test_random_matrix_after_each_change(dsa, hip, oracle):
    rng = np.random.default_rng(11)
    m, n, nnz = 700, 500, 6000
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.integers(1, 1 << 20, nnz) * 2.0 ** -9
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    _check_all(dsa, a, b)
    # mixed writes, a quarter of them zeros (deletions)
    I2, J2 = rng.integers(1, m + 1, 3000), rng.integers(1, n + 1, 3000)
    V2 = np.where(rng.random(3000) < 0.25, 0.0, rng.integers(1, 100, 3000) * 0.5)
    for x in (a, b):
        x.set_batch(I2, J2, V2)
    _check_all(dsa, a, b)
    # tombstones in both orientations
    c1, c2 = (int(c) for c in np.unique(J[:20])[:2])
    for x in (a, b):
        x.deletecolumn(c1)
        x.deletecolumn(c2)
        x.deleterow(int(I[5]))
    _check_all(dsa, a, b)
    # new columns, keys in random order
    newc = rng.permutation(np.arange(n + 1, n + 41))
    I3 = rng.integers(1, m + 1, len(newc))
    for x in (a, b):
        x.set_batch(I3, newc, np.full(len(newc), 2.5))
    assert a.size() == b.size() == (m, n + 40)
    _check_all(dsa, a, b)
    # a zero written beyond size(m, 2): an empty partition outside the size
    for x in (a, b):
        x[3, n + 100] = 0.0
    assert a.size() == b.size()
    assert a.size()[1] < n + 100
    _check_all(dsa, a, b)


@pytest.mark.gpu
def test_wide_column_key_csr(dsa, hip, oracle):
    big = (1 << 31) + 5
    I = np.array([1, 2, 3, 3, 4], dtype=np.int64)
    J = np.array([1, 7, 2, big, big], dtype=np.int64)
    V = np.array([1.5, -2.0, 3.25, 4.0, 0.125])
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    exp = _expect(b, ROWMAJOR, 0)
    assert exp[1].max() == big - 1
    _assert_same(_export_dev(a, ROWMAJOR, 64, 0), exp)
    _assert_same(_export_dev(a, ROWMAJOR, 64, 1), _expect(b, ROWMAJOR, 1))
    _assert_same(a.to_csr(), exp)
    with pytest.raises(dsa.DsaError) as ei:
        _export_dev(a, ROWMAJOR, 32, 0)
    assert ei.value.code == 1                   # EARG: n does not fit 32-bit indices


@pytest.mark.gpu
def test_capacity_and_bounds_errors(dsa, hip):
    import torch
    a = dsa.dynamicsparse([1, 2, 3], [1, 2, 3], [1.0, 2.0, 3.0], binding=hip)
    ptr = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    idx = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    val = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    got = C.c_int64(-1)
    rc = hip._mat_to_compressed_dev(a.h, COLMAJOR, 64, 0, C.c_void_p(ptr.data_ptr()), C.c_void_p(idx.data_ptr()),
                                    C.c_void_p(val.data_ptr()), 2, C.byref(got))
    assert rc == 8 and got.value == 3           # ECAP, nnz reported
    torch.cuda.synchronize()
    assert (ptr == -7).all() and (idx == -7).all() and (val == -7.0).all()
    # explicit m below the largest row: CSC sees a row key outside 1..m, CSR a row partition outside 1..m
    c = dsa.dynamicsparse([1, 5, 2], [1, 2, 3], [1.0, 2.0, 3.0], m=3, n=3, binding=hip)
    assert c.size() == (3, 3)
    for o in (COLMAJOR, ROWMAJOR):
        with pytest.raises(dsa.DsaBoundsError):
            _export_dev(c, o, 64, 0)
        with pytest.raises(dsa.DsaBoundsError):
            c.to_csr() if o == ROWMAJOR else c.to_csc()


@pytest.mark.gpu
def test_c3_full_size_exact_layout_and_plan_untouched(dsa, hip, oracle):
    sys.path.insert(0, ROOT)
    import bench
    import torch
    I, J, V = bench.c3_triplets(1_000_000, 1_000_000, 10, 0, seed_rows=5, seed_vals=6)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    x = bench.unit12(9, 1_000_000)
    for _ in range(3):
        a.mul(x)                                # the plan is built on the second product
    builds = a.info(ROWMAJOR)["stat_spmv_plan_builds"]
    before = [a.export_layout(o) for o in (COLMAJOR, ROWMAJOR)]
    for o in (COLMAJOR, ROWMAJOR):
        exp = _expect(b, o, 0)
        for bits in (32, 64):
            _assert_same(_export_dev(a, o, bits, 0), exp)
    for o in (COLMAJOR, ROWMAJOR):
        after = a.export_layout(o)
        for k in ("keys", "vals", "occ", "semaphores", "col_keys", "col_live"):
            assert np.array_equal(after[k].view(np.uint8), before[o][k].view(np.uint8)), (o, k)
    y = a.mul(x)
    assert a.info(ROWMAJOR)["stat_spmv_plan_builds"] == builds
    np.testing.assert_allclose(y, b.mul(x), rtol=1e-12, atol=0)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_to_torch_csr_product_and_arrays(dsa, hip, oracle):
    import torch
    rng = np.random.default_rng(5)
    m, n, nnz = 3000, 2000, 40000
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.random(nnz) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    x = rng.random(n)
    exp = _expect(b, ROWMAJOR, 0)
    for dt in (torch.int32, torch.int64):
        t = a.to_torch(torch.sparse_csr, index_dtype=dt)
        assert t.layout == torch.sparse_csr and tuple(t.shape) == (m, n) and t.crow_indices().dtype == dt
        _assert_same((t.crow_indices().cpu().numpy(), t.col_indices().cpu().numpy(), t.values().cpu().numpy()), exp)
        y = (t @ torch.from_numpy(x).to("cuda").unsqueeze(1)).squeeze(1).cpu().numpy()
        np.testing.assert_allclose(y, a.mul(x), rtol=1e-12, atol=0)
    t = a.to_torch(torch.sparse_csc)
    assert t.layout == torch.sparse_csc and tuple(t.shape) == (m, n)
    _assert_same((t.ccol_indices().cpu().numpy(), t.row_indices().cpu().numpy(), t.values().cpu().numpy()), _expect(b, COLMAJOR, 0))


@pytest.mark.gpu
def test_export_right_after_a_batch_sees_it(dsa, hip, oracle):
    rng = np.random.default_rng(8)
    m = n = 4000
    I, J = rng.integers(1, m + 1, 30000), rng.integers(1, n + 1, 30000)
    a, b = (dsa.dynamicsparse(I, J, np.ones(30000), binding=x) for x in (hip, oracle))
    for step in range(3):
        I2, J2 = rng.integers(1, m + 1, 5000), rng.integers(1, n + 1, 5000)
        V2 = np.where(rng.random(5000) < 0.3, 0.0, rng.random(5000))
        for x in (a, b):
            x.set_batch(I2, J2, V2)
        _assert_same(_export_dev(a, step % 2, 64, 0), _expect(b, step % 2, 0))     # no sync between the batch and the export
    I, J, V = a.findnz()
    Ib, Jb, Vb = [], [], []
    for j in range(1, n + 1):
        for i, v in b.col_view(j):
            Ib.append(i); Jb.append(j); Vb.append(v)
    assert np.array_equal(I, Ib) and np.array_equal(J, Jb) and np.array_equal(V, Vb)
