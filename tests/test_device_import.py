"""Import from device memory (include/dsa.h: dsa_mat_create_from_coo_dev / dsa_mat_create_from_compressed_dev; csrc/ingest.hip): a
matrix built from COO / CSR / CSC arrays that are already in HBM is, slot for slot, the matrix the ORACLE's dynamicsparse(I, J, V, m, n)
builds from the same 1-based triples in the same order.  Expected values never come from the library under test."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import MATRIX_CASES, _assert_same, _expect, _in_fill_mode, _in_size, expected_compressed
from test_hip_parity import assert_mat_equal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLMAJOR, ROWMAJOR = 0, 1
EARG, EBOUNDS, EKEY = 1, 2, 9
IN_ITEM = 2048            # entries per work item of k_in_expand (csrc/ingest.h)
NEW_SYMBOLS = ("mat_create_from_coo_dev", "mat_create_from_compressed_dev")


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_import_symbols_declared_bound_and_exported(dsa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsa.h")).read(), flags=re.S)
    syms = dsa.Binding.declared_symbols()
    lib = C.CDLL(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bdsa_" + name + r"\s*\(", hdr), name
        assert name in syms, name
        assert hasattr(lib, "dsa_" + name), name
    for name in ("dynamicsparse_dev", "dynamicsparse_compressed_dev", "from_torch"):
        assert callable(getattr(dsa, name)), name
    hdr = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "ingest.h")).read()
    assert int(re.search(r"IN_ITEM\s*=\s*(\d+)", hdr).group(1)) == IN_ITEM


def test_import_needs_the_product_library(dsa, oracle):
    for name in NEW_SYMBOLS:
        assert not oracle.has(name)
    with pytest.raises(dsa.DsaArgumentError, match="needs the HIP product library"):
        dsa.dynamicsparse_dev(0, 0, 0, 0, binding=oracle)
    with pytest.raises(dsa.DsaArgumentError, match="needs the HIP product library"):
        dsa.dynamicsparse_compressed_dev(ROWMAJOR, 0, 0, 0, 0, 0, 0, binding=oracle)
    with pytest.raises(dsa.DsaArgumentError, match="needs the HIP product library"):
        dsa.from_torch(None, binding=oracle)


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _dev(a, bits=None):
    """numpy array -> torch tensor in HBM (indices as int32 / int64, values as float64)"""
    import torch
    if bits is None:
        return torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda")
    return torch.from_numpy(np.array(a, dtype=np.int32 if bits == 32 else np.int64)).to("cuda")


def _import_compressed(dsa, hip, o, ptr0, idx0, val, outer, inner, bits, base, keep=None):
    """0-based host arrays -> device arrays of `bits` counted from `base` -> dsa_mat_create_from_compressed_dev"""
    import torch
    tp, ti, tv = _dev(np.asarray(ptr0) + base, bits), _dev(np.asarray(idx0) + base, bits), _dev(val)
    torch.cuda.synchronize()
    a = dsa.dynamicsparse_compressed_dev(o, tp.data_ptr(), ti.data_ptr(), tv.data_ptr(), outer, inner, len(val), index_bits=bits,
                                         index_base=base, binding=hip)
    if keep is not None:
        keep.extend((tp, ti, tv))
    return a


def _import_coo(dsa, hip, I1, J1, val, m, n, bits, base, keep=None):
    """1-based host triples -> device arrays of `bits` counted from `base` -> dsa_mat_create_from_coo_dev"""
    import torch
    ti, tj, tv = _dev(np.asarray(I1) - 1 + base, bits), _dev(np.asarray(J1) - 1 + base, bits), _dev(val)
    torch.cuda.synchronize()
    a = dsa.dynamicsparse_dev(ti.data_ptr(), tj.data_ptr(), tv.data_ptr(), len(val), m, n, index_bits=bits, index_base=base, binding=hip)
    if keep is not None:
        keep.extend((ti, tj, tv))
    return a


def _outer_keys(ptr0):
    return np.repeat(np.arange(1, len(ptr0), dtype=np.int64), np.diff(ptr0))


def _csr_of(I, J, V, m):
    """CSR (0-based ptr, idx, val) of 1-based triples, the entries of a row in input order (unsorted columns, duplicates kept)"""
    order = np.argsort(I, kind="stable")
    ptr = np.searchsorted(I[order], np.arange(m + 1), side="right").astype(np.int64)
    return ptr, (J[order] - 1).astype(np.int64), V[order]


@functools.lru_cache(maxsize=None)
def _random_triples(nnz):
    rng = np.random.default_rng(1000 + nnz)
    m, n = 400, 300                         # 120 000 cells: both sizes hold many duplicates
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.standard_normal(nnz)
    for x in (I, J, V):
        x.setflags(write=False)
    return m, n, I, J, V


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_golden_round_trip(dsa, hip, oracle):
    """every golden matrix scenario that ends with all cells inside size(m): its CSC and CSR (from the oracle's layout) imported as CSC,
    CSR and COO, 32 / 64 bits, base 0 / 1, against the oracle built from those triples in that order"""
    ran = 0
    for sc in MATRIX_CASES:
        b = run_scenario(dsa, oracle, sc)
        if _in_fill_mode(dsa, b):
            continue
        m, n = b.size()
        csc, csr = _expect(b, COLMAJOR), _expect(b, ROWMAJOR)
        if not (_in_size(csc, m) and _in_size(csr, n)):
            continue
        ran += 1
        for o, (ptr, idx, val), outer, inner in ((COLMAJOR, csc, n, m), (ROWMAJOR, csr, m, n)):
            ko, ki = _outer_keys(ptr), idx + 1
            I, J = (ko, ki) if o == ROWMAJOR else (ki, ko)
            ref = dsa.dynamicsparse(I, J, val, m, n, binding=oracle)
            if o == COLMAJOR:
                _assert_same(_expect(ref, COLMAJOR), csc)           # (the fresh build from the CSC-order triples reproduces the CSC)
            for bits in (32, 64):
                for base in (0, 1):
                    assert_mat_equal(_import_compressed(dsa, hip, o, ptr, idx, val, outer, inner, bits, base), ref)
                    assert_mat_equal(_import_coo(dsa, hip, I, J, val, m, n, bits, base), ref)
    assert ran >= 12, ran


def _expansion_breaker(rng):
    """one CSR that stresses the expansion (see the test below); returns 0-based (ptr, idx, val), outer, inner"""
    inner = 150
    lens = [0, 0,                   # empty slices at the front
            5,                      # duplicates, one pair cancelling to 0.0
            0,                      # empty in the middle (1)
            11,
            2 * IN_ITEM + 3,        # longer than two work items
            0, 0, 0,                # empty in the middle (2)
            IN_ITEM - 19,           # ends exactly on an item boundary: 5 + 11 + 2 * IN_ITEM + 3 + IN_ITEM - 19 = 3 * IN_ITEM
            7,                      # holds the explicit 0.0
            0, 0]                   # empty slices at the end
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    assert ptr[10] == 3 * IN_ITEM
    nnz = int(ptr[-1])
    idx = rng.integers(0, inner, nnz).astype(np.int64)          # unsorted, with duplicates inside the long slices
    val = rng.standard_normal(nnz)
    idx[0:5] = [4, 9, 4, 2, 9]
    val[0], val[2] = 1.5, -1.5                                   # (row 3, column 5) cancels to a stored 0.0
    p = int(ptr[10])
    idx[p:p + 7] = [140, 3, 77, 12, 149, 0, 60]
    val[p + 2] = 0.0                                             # an explicit 0.0
    return ptr, idx, val, len(lens), inner


@pytest.mark.gpu
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("base", (0, 1))
def test_shapes_that_break_an_expansion(dsa, hip, oracle, bits, base):
    rng = np.random.default_rng(21)
    ptr, idx, val, outer, inner = _expansion_breaker(rng)
    ref = dsa.dynamicsparse(_outer_keys(ptr), idx + 1, val, outer, inner, binding=oracle)
    assert ref[3, 5] == 0.0 and ref.nnz() < len(val)
    a = _import_compressed(dsa, hip, ROWMAJOR, ptr, idx, val, outer, inner, bits, base)
    assert_mat_equal(a, ref)
    x = rng.standard_normal(inner)
    assert np.array_equal(np.asarray(a.mul(x)).view(np.uint64), np.asarray(ref.mul(x)).view(np.uint64))
    # all slices empty
    e = _import_compressed(dsa, hip, ROWMAJOR, np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), 5, 4, bits, base)
    eref = dsa.dynamicsparse(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), 5, 4, binding=oracle)
    assert e.nnz() == 0
    assert_mat_equal(e, eref)


@pytest.mark.gpu
def test_stored_zeros_are_kept(dsa, hip, oracle):
    I, J, V = np.array([1, 2, 2, 3, 3]), np.array([1, 2, 2, 1, 4]), np.array([0.0, 1.5, -1.5, 2.0, 3.0])
    ref = dsa.dynamicsparse(I, J, V, binding=oracle)
    a = _import_coo(dsa, hip, I, J, V, None, None, 64, 1)
    assert a.nnz() == 4 == ref.nnz()
    assert_mat_equal(a, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("nnz", (60_000, 70_000))          # below / above the 1 << 16 twin-build threshold of mat_build_major_dev
def test_both_build_paths(dsa, hip, oracle, nnz):
    m, n, I, J, V = _random_triples(nnz)
    assert_mat_equal(_import_coo(dsa, hip, I, J, V, m, n, 64, 1), dsa.dynamicsparse(I, J, V, m, n, binding=oracle))
    assert_mat_equal(_import_coo(dsa, hip, I, J, V, m, n, 32, 0), dsa.dynamicsparse(I, J, V, m, n, binding=oracle))
    ptr, idx, val = _csr_of(I, J, V, m)
    ref = dsa.dynamicsparse(_outer_keys(ptr), idx + 1, val, m, n, binding=oracle)
    assert_mat_equal(_import_compressed(dsa, hip, ROWMAJOR, ptr, idx, val, m, n, 32, 0), ref)
    assert_mat_equal(_import_compressed(dsa, hip, ROWMAJOR, ptr, idx, val, m, n, 64, 1), ref)


@pytest.mark.gpu
def test_wide_keys(dsa, hip, oracle):
    big = (1 << 40) + 5
    I = np.array([1, 2, -3, 3, 4], dtype=np.int64)
    J = np.array([1, 7, 2, big, big], dtype=np.int64)
    V = np.array([1.5, -2.0, 3.25, 4.0, 0.125])
    ref = dsa.dynamicsparse(I, J, V, binding=oracle)
    a = _import_coo(dsa, hip, I, J, V, None, None, 64, 1)
    assert a.size() == ref.size() == (4, big)
    assert_mat_equal(a, ref)
    # the same column as the outer dimension of a CSC with 32-bit indices: refused before anything is read
    tp, ti, tv = _dev(np.zeros(2), 32), _dev(np.zeros(1), 32), _dev(np.ones(1))
    with pytest.raises(dsa.DsaError) as ei:
        dsa.dynamicsparse_compressed_dev(COLMAJOR, tp.data_ptr(), ti.data_ptr(), tv.data_ptr(), big, 4, 1, index_bits=32, binding=hip)
    assert ei.value.code == EARG


@pytest.mark.gpu
def test_errors_one_fault_at_a_time(dsa, hip, oracle):
    """a well-formed 20-entry CSR with one fault each: the status code, no handle, and a correct import right behind it"""
    import torch
    rng = np.random.default_rng(33)
    outer, inner, nnz = 6, 8, 20
    lens = [3, 0, 6, 4, 5, 2]
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    idx = rng.integers(0, inner, nnz).astype(np.int64)
    val = rng.standard_normal(nnz)
    ref = dsa.dynamicsparse(_outer_keys(ptr), idx + 1, val, outer, inner, binding=oracle)

    def raw(o, bits, base, p, i, v, nnz_arg=nnz, null_ptr=False):
        tp, ti, tv = _dev(p, 32 if bits == 32 else 64), _dev(i, 32 if bits == 32 else 64), _dev(v)
        torch.cuda.synchronize()
        h = C.c_void_p(0xdead)
        rc = hip._mat_create_from_compressed_dev(o, bits, base, C.c_void_p(0 if null_ptr else tp.data_ptr()), C.c_void_p(ti.data_ptr()),
                                                 C.c_void_p(tv.data_ptr()), outer, inner, nnz_arg, C.byref(h))
        assert h.value == 0xdead                     # *out is untouched on an error
        return rc

    def good():
        assert_mat_equal(_import_compressed(dsa, hip, ROWMAJOR, ptr, idx, val, outer, inner, 64, 0), ref)

    good()
    for base in (0, 1):
        for bits in (32, 64):
            p, i = ptr + base, idx + base
            q = p.copy(); q[0] = base + 1
            assert raw(ROWMAJOR, bits, base, q, i, val) == EARG; good()
            q = p.copy(); q[outer] = base + nnz - 1
            assert raw(ROWMAJOR, bits, base, q, i, val) == EARG; good()
            q = p.copy(); q[3] = q[2] - 1                                # one decreasing step
            assert raw(ROWMAJOR, bits, base, q, i, val) == EARG; good()
            j = i.copy(); j[7] = base + inner
            assert raw(ROWMAJOR, bits, base, p, j, val) == EBOUNDS; good()
            j = i.copy(); j[11] = base - 1
            assert raw(ROWMAJOR, bits, base, p, j, val) == EBOUNDS; good()
    assert raw(ROWMAJOR, 16, 0, ptr, idx, val) == EARG; good()
    assert raw(ROWMAJOR, 64, 2, ptr, idx, val) == EARG; good()
    assert raw(2, 64, 0, ptr, idx, val) == EARG; good()
    assert raw(ROWMAJOR, 64, 0, ptr, idx, val, nnz_arg=-1) == EARG; good()
    assert raw(ROWMAJOR, 64, 0, ptr, idx, val, null_ptr=True) == EARG; good()
    # COO, base 0, an index -1: the key 0
    I0, J0 = _outer_keys(ptr) - 1, idx.copy()
    J0[4] = -1
    for bits in (32, 64):
        ti, tj, tv = _dev(I0, bits), _dev(J0, bits), _dev(val)
        torch.cuda.synchronize()
        h = C.c_void_p(0xdead)
        rc = hip._mat_create_from_coo_dev(C.c_void_p(ti.data_ptr()), C.c_void_p(tj.data_ptr()), C.c_void_p(tv.data_ptr()), nnz, bits, 0,
                                          outer, inner, C.byref(h))
        assert rc == EKEY and h.value == 0xdead
        good()
    with pytest.raises(dsa.DsaError) as ei:
        dsa.dynamicsparse_dev(0, 0, 0, 3, binding=hip)                   # NULL arrays of a non-empty shape
    assert ei.value.code == EARG
    good()


@pytest.mark.gpu
def test_from_torch(dsa, hip, oracle):
    import torch
    rng = np.random.default_rng(44)
    m, n, nnz = 300, 200, 3000
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.standard_normal(nnz)
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    b = dsa.dynamicsparse(I, J, V, m, n, binding=oracle)
    cases = [(torch.sparse_csr, torch.int64), (torch.sparse_csc, torch.int32), (torch.sparse_csc, torch.int64)]
    for layout, dt in cases:
        o = ROWMAJOR if layout == torch.sparse_csr else COLMAJOR
        ptr, idx, val = _expect(b, o)                                    # what the export must hold: the oracle's compressed form
        ko, ki = _outer_keys(ptr), idx + 1
        ref = dsa.dynamicsparse(*((ko, ki) if o == ROWMAJOR else (ki, ko)), val, m, n, binding=oracle)
        t = a.to_torch(layout, index_dtype=dt)
        c = dsa.from_torch(t, binding=hip)
        assert_mat_equal(c, ref)
        t2 = c.to_torch(layout, index_dtype=dt)
        for get in ((lambda z: z.crow_indices(), lambda z: z.col_indices()) if o == ROWMAJOR else (lambda z: z.ccol_indices(), lambda z: z.row_indices())):
            assert get(t2).dtype == dt and torch.equal(get(t2), get(t))
        assert torch.equal(t2.values().view(torch.int64), t.values().view(torch.int64))
        _assert_same(tuple(x.cpu().numpy() for x in ((t2.crow_indices(), t2.col_indices()) if o == ROWMAJOR else
                                                     (t2.ccol_indices(), t2.row_indices())) + (t2.values(),)), (ptr, idx, val))
    # uncoalesced COO with duplicates, in the order of the triples
    ind = torch.from_numpy(np.stack([I - 1, J - 1]).astype(np.int64)).to("cuda")
    coo = torch.sparse_coo_tensor(ind, torch.from_numpy(V).to("cuda"), size=(m, n))
    assert not coo.is_coalesced() and len(np.unique(I * 1000 + J)) < nnz
    assert_mat_equal(dsa.from_torch(coo, binding=hip), b)
    # float32 values are widened on the device
    V32 = V.astype(np.float32)
    coo32 = torch.sparse_coo_tensor(ind, torch.from_numpy(V32).to("cuda"), size=(m, n))
    assert_mat_equal(dsa.from_torch(coo32, binding=hip), dsa.dynamicsparse(I, J, V32.astype(np.float64), m, n, binding=oracle))
    with pytest.raises(dsa.DsaArgumentError):
        dsa.from_torch(coo.cpu(), binding=hip)
    with pytest.raises(dsa.DsaArgumentError):
        dsa.from_torch(torch.zeros(3, 3, device="cuda"), binding=hip)


@pytest.mark.gpu
def test_callers_arrays_are_free_on_return(dsa, hip, oracle):
    """the tensors are overwritten with garbage right behind the call, without any sync of the library: the layout is the oracle's"""
    import torch
    m, n, I, J, V = _random_triples(70_000)
    ptr, idx, val = _csr_of(I, J, V, m)
    ref_csr = dsa.dynamicsparse(_outer_keys(ptr), idx + 1, val, m, n, binding=oracle)
    ref_coo = dsa.dynamicsparse(I, J, V, m, n, binding=oracle)
    built = []
    for make, ref in ((lambda k: _import_compressed(dsa, hip, ROWMAJOR, ptr, idx, val, m, n, 32, 0, keep=k), ref_csr),
                      (lambda k: _import_coo(dsa, hip, I, J, V, m, n, 64, 1, keep=k), ref_coo),        # (read in place by the builder)
                      (lambda k: _import_coo(dsa, hip, I, J, V, m, n, 32, 0, keep=k), ref_coo)):
        keep = []
        a = make(keep)
        keep[0].fill_(-7); keep[1].fill_(1 << 20); keep[2].fill_(float("nan"))
        built.append((a, ref))
    torch.cuda.synchronize()
    for a, ref in built:
        assert_mat_equal(a, ref)
