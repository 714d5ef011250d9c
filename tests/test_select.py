"""Selected export of a matrix: A[:, J] / A[I, :] for a key list (include/dsa.h: dsa_mat_select_compressed[_dev]; csrc/select.hip).

Expected arrays never come from the kernels under test: the ORACLE matrix goes through the same operations, `expected_compressed`
(test_compressed_export.py, pinned there against the reference's own col_view / row_view iteration) gives its full CSC / CSR, and slice k
of it is idx[ptr[k-1]:ptr[k]].  Comparisons are exact: ptr and idx equal, values equal as uint64 bit patterns.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from scenario import run_scenario
from test_compressed_export import expected_compressed

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "reference_cases.json")) as f:
    MATRIX_CASES = [c for c in json.load(f)["scenarios"] if c["kind"] == "matrix"]

COLMAJOR, ROWMAJOR = 0, 1
EARG, EBOUNDS, EMODE, ECAP = 1, 2, 5, 8
NAMES = ("mat_select_compressed", "mat_select_compressed_dev")


class Expect:
    """the full compressed form of one orientation of the oracle matrix, sliced per key on demand"""

    def __init__(self, ora, o):
        m, n = ora.size()
        self.dim_out, self.dim_in = (m, n) if o == ROWMAJOR else (n, m)
        self.ptr, self.idx, self.val = expected_compressed(ora.export_layout(o), self.dim_out, 0)

    def counts(self, sel):
        sel = np.asarray(sel, dtype=np.int64)
        return self.ptr[sel] - self.ptr[sel - 1]

    def select(self, sel, base=0):
        sel = np.asarray(sel, dtype=np.int64)
        assert np.all((sel >= 1) & (sel <= self.dim_out))
        ptr = base + np.concatenate(([0], np.cumsum(self.counts(sel)))).astype(np.int64)
        parts = [np.arange(self.ptr[k - 1], self.ptr[k]) for k in sel]
        take = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
        return ptr, self.idx[take] + base, self.val[take].copy()

    def in_size(self, sel):
        """whether every cell of the selected partitions lies inside size(m) (otherwise: EBOUNDS)"""
        idx = self.select(sel)[1]
        return bool(np.all((idx >= 0) & (idx < self.dim_in)))


def _assert_same(got, exp):
    assert np.array_equal(np.asarray(got[0], dtype=np.int64), exp[0])
    assert np.array_equal(np.asarray(got[1], dtype=np.int64), exp[1])
    assert np.array_equal(np.ascontiguousarray(got[2], dtype=np.float64).view(np.uint64), exp[2].view(np.uint64))


def _in_fill_mode(dsa, a):
    try:
        a.export_layout(0)
    except dsa.DsaError as e:
        if e.code == EMODE:
            return True
        raise
    return False


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_select_symbols_declared_bound_and_exported(dsa):
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


def test_select_needs_the_product_library(dsa, oracle):
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=oracle)
    for call in (lambda: a.select_columns([1]), lambda: a.select_rows([1]), lambda: a.count_columns([1]), lambda: a.count_rows([2]),
                 lambda: a.select_compressed_dev(COLMAJOR, 0, 0, 0, 0, 0, 0)):
        with pytest.raises(dsa.DsaArgumentError):
            call()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _select_dev(a, o, sel, bits, base):
    """dsa_mat_select_compressed_dev into torch tensors (the count-only call, then the one that fits), back to numpy"""
    import torch
    dt = torch.int32 if bits == 32 else torch.int64
    d_sel = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int64)).to("cuda")
    nsel = d_sel.numel()
    ptr = torch.full((nsel + 1,), -7, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    total, fits = a.select_compressed_dev(o, d_sel.data_ptr(), nsel, ptr.data_ptr(), 0, 0, 0, index_bits=bits, base=base)
    a.sync()
    assert fits == (total == 0)
    ptr0 = ptr.cpu().numpy()
    idx = torch.full((max(total, 1),), -7, dtype=dt, device="cuda")
    val = torch.full((max(total, 1),), -7.0, dtype=torch.float64, device="cuda")
    ptr.fill_(-7)
    torch.cuda.synchronize()
    got, fits = a.select_compressed_dev(o, d_sel.data_ptr(), nsel, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), total,
                                        index_bits=bits, base=base)
    a.sync()
    assert fits and got == total
    assert np.array_equal(ptr.cpu().numpy(), ptr0)          # the count-only call leaves the same ptr
    return ptr0, idx[:got].cpu().numpy(), val[:got].cpu().numpy()


def _check_dev(dsa, a, E, o, sel, bits=(32, 64), bases=(0, 1)):
    for base in bases:
        for b in bits:
            if E.in_size(sel):
                _assert_same(_select_dev(a, o, sel, b, base), E.select(sel, base))
            else:
                with pytest.raises(dsa.DsaBoundsError):
                    _select_dev(a, o, sel, b, base)


def _check_host(dsa, a, E, o, sel, bases=(0, 1)):
    fn = a.select_columns if o == COLMAJOR else a.select_rows
    for base in bases:
        if E.in_size(sel):
            _assert_same(fn(sel, base=base), E.select(sel, base))
        else:
            with pytest.raises(dsa.DsaBoundsError):
                fn(sel, base=base)


@pytest.mark.gpu
@pytest.mark.parametrize("sc", MATRIX_CASES, ids=lambda s: s["name"])
def test_golden_cases_exact(dsa, hip, oracle, sc):
    a = run_scenario(dsa, hip, sc)
    b = run_scenario(dsa, oracle, sc)
    if _in_fill_mode(dsa, b):
        for o in (COLMAJOR, ROWMAJOR):
            with pytest.raises(dsa.DsaError) as ei:
                a.select_compressed_dev(o, 0, 0, 0, 0, 0, 0)
            assert ei.value.code == EMODE
            with pytest.raises(dsa.DsaError) as ei:
                a.select_columns([1]) if o == COLMAJOR else a.select_rows([1])
            assert ei.value.code == EMODE
        return
    for o in (COLMAJOR, ROWMAJOR):
        E = Expect(b, o)
        every = np.arange(1, E.dim_out + 1, dtype=np.int64)
        for sel in (every, every[::-1], every[::2]):
            _check_dev(dsa, a, E, o, sel)
        _check_host(dsa, a, E, o, every[::-1], bases=(0,))


LONG_COLS = [150, 1, 300, 17, 40, 150, 299, 2, 1]


@pytest.fixture(scope="module")
def long_case(dsa, hip, oracle):
    """6000 x 300, one column of 5000 cells among short ones, two column tombstones, two columns never written, one row deleted; the
    product matrix, the expected full forms of the oracle matrix (left unchanged by every test), and the deleted row's key"""
    rng = np.random.default_rng(21)
    m, n = 6000, 300
    I, J = rng.integers(1, m + 1, 9000), rng.integers(1, n + 1, 9000)
    V = rng.integers(1, 1 << 20, 9000) * 2.0 ** -9
    keep = (J != 17) & (J != 18)
    I, J, V = I[keep], J[keep], V[keep]
    rows = rng.choice(m, 5000, replace=False) + 1
    I = np.concatenate((I, rows))
    J = np.concatenate((J, np.full(5000, 150)))
    V = np.concatenate((V, rng.integers(1, 1 << 20, 5000) * 2.0 ** -9))
    mats = [dsa.dynamicsparse(I, J, V, m=m, n=n, binding=x) for x in (hip, oracle)]
    for x in mats:
        x.deletecolumn(40)
        x.deletecolumn(41)
        x.deleterow(int(I[5]))
    assert mats[0].size() == mats[1].size() == (m, n)
    return mats[0], {o: Expect(mats[1], o) for o in (COLMAJOR, ROWMAJOR)}, int(I[5])


@pytest.mark.gpu
def test_long_column_tombstones_absent_keys_and_repeats(dsa, long_case):
    a, E, dead_row = long_case
    assert E[COLMAJOR].counts(LONG_COLS).tolist() == [5004, 38, 28, 0, 0, 5004, 25, 19, 38]      # the input is the one the cases were chosen on
    rows = [6000, 1, dead_row, 77, 77, 3]
    assert E[ROWMAJOR].counts(rows)[2] == 0
    for o, sel in ((COLMAJOR, LONG_COLS), (ROWMAJOR, rows)):
        assert E[o].in_size(sel)
        _check_dev(dsa, a, E[o], o, sel)
        _check_host(dsa, a, E[o], o, sel)
    assert np.array_equal(a.count_columns(LONG_COLS), np.diff(E[COLMAJOR].select(LONG_COLS)[0]))
    assert np.array_equal(a.count_rows(rows), np.diff(E[ROWMAJOR].select(rows)[0]))


@pytest.mark.gpu
def test_scan_carry_and_tiny_selections(dsa, long_case):
    a, E, _ = long_case
    sel = np.random.default_rng(22).integers(1, 301, 20000)          # more than one 8192-entry step of the scan loop
    _check_dev(dsa, a, E[COLMAJOR], COLMAJOR, sel, bits=(32, 64), bases=(1,))
    _check_host(dsa, a, E[COLMAJOR], COLMAJOR, sel, bases=(0,))
    for k in (8192, 8193):                                           # one full step of the prefix loop, and one entry more
        _check_dev(dsa, a, E[COLMAJOR], COLMAJOR, sel[:k], bits=(64,), bases=(0,))
    for o in (COLMAJOR, ROWMAJOR):
        for sel in (np.zeros(0, dtype=np.int64), np.array([150]), np.array([17]), np.array([2])):
            _check_dev(dsa, a, E[o], o, sel)
            _check_host(dsa, a, E[o], o, sel)
    assert len(a.count_columns([])) == 0


OWNER_LENGTHS = (63, 64, 65, 4096, 4097)          # no narrowing round of the 64-ary owner search, the first round, the step past one round


def owner_search_selections(E, n):
    """column selections of `long_case` with n keys for the work-item owner search (export_dev.h: item_owner): short columns with
    cells everywhere but at one position, which in turn holds the long column 150 first, in the middle and last (an owner of several
    work items at either end) and an absent key first and last (tied item prefixes at both ends)"""
    every = np.arange(1, E.dim_out + 1, dtype=np.int64)
    short = every[(E.counts(every) > 0) & (every != 150)]
    fill = np.random.default_rng(n).choice(short, n)
    for pos, key in ((0, 150), (n // 2, 150), (n - 1, 150), (0, 17), (n - 1, 40)):
        sel = fill.copy()
        sel[pos] = key
        yield sel


@pytest.mark.gpu
def test_owner_search_boundaries(dsa, long_case):
    a, E, _ = long_case
    assert E[COLMAJOR].counts([150, 17, 40]).tolist() == [5004, 0, 0]
    for n in OWNER_LENGTHS:
        for sel in owner_search_selections(E[COLMAJOR], n):
            _check_dev(dsa, a, E[COLMAJOR], COLMAJOR, sel, bits=(32, 64), bases=(0,))


@pytest.mark.gpu
def test_selection_right_after_a_batch_sees_it(dsa, hip, oracle):
    rng = np.random.default_rng(8)
    m = n = 4000
    I, J = rng.integers(1, m + 1, 30000), rng.integers(1, n + 1, 30000)
    a, b = (dsa.dynamicsparse(I, J, np.ones(30000), binding=x) for x in (hip, oracle))
    for step in range(3):
        I2, J2 = rng.integers(1, m + 1, 5000), rng.integers(1, n + 1, 5000)
        V2 = np.where(rng.random(5000) < 0.3, 0.0, rng.random(5000))
        for x in (a, b):
            x.set_batch(I2, J2, V2)
        o = step % 2
        E = Expect(b, o)
        sel = rng.integers(1, E.dim_out + 1, 500)
        _assert_same(_select_dev(a, o, sel, 64, 0), E.select(sel))         # no sync between the batch and the selection
    # new columns, keys in random order; old and new keys mixed
    newc = rng.permutation(np.arange(n + 1, n + 41))
    I3 = rng.integers(1, m + 1, len(newc))
    for x in (a, b):
        x.set_batch(I3, newc, np.full(len(newc), 2.5))
    assert a.size() == b.size() == (m, n + 40)
    E = Expect(b, COLMAJOR)
    sel = rng.permutation(np.concatenate((newc, rng.integers(1, n + 1, 60), [n + 40, n + 1, 1])))
    assert E.counts(newc).min() >= 1
    _check_dev(dsa, a, E, COLMAJOR, sel)
    _check_host(dsa, a, E, COLMAJOR, sel, bases=(1,))
    E = Expect(b, ROWMAJOR)
    sel = np.concatenate((I3[:20], rng.integers(1, m + 1, 50)))
    _check_dev(dsa, a, E, ROWMAJOR, sel, bits=(32,), bases=(0,))


def _raw_dev(hip, a, o, sel, cap, with_arrays, base=0):
    """the entry point itself: (rc, nnz_out, ptr, idx, val) with -7 sentinels in every output"""
    import torch
    d_sel = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int64)).to("cuda")
    ptr = torch.full((len(sel) + 1,), -7, dtype=torch.int64, device="cuda")
    idx = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
    val = torch.full((max(cap, 1),), -7.0, dtype=torch.float64, device="cuda")
    got = C.c_int64(-1)
    torch.cuda.synchronize()
    rc = hip._mat_select_compressed_dev(a.h, o, 64, base, C.c_void_p(d_sel.data_ptr()), len(sel), C.c_void_p(ptr.data_ptr()),
                                        C.c_void_p(idx.data_ptr() if with_arrays else None),
                                        C.c_void_p(val.data_ptr() if with_arrays else None), cap, C.byref(got))
    a.sync()
    torch.cuda.synchronize()
    return rc, got.value, ptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()


@pytest.mark.gpu
def test_capacity_protocol(dsa, hip, long_case):
    a, E, _ = long_case
    exp = E[COLMAJOR].select(LONG_COLS, 1)
    total = len(exp[1])
    rc, got, ptr, idx, val = _raw_dev(hip, a, COLMAJOR, LONG_COLS, total - 1, True, base=1)
    assert rc == ECAP and got == total
    assert np.array_equal(ptr, exp[0]) and (idx == -7).all() and (val == -7.0).all()
    rc, got, ptr, idx, val = _raw_dev(hip, a, COLMAJOR, LONG_COLS, 0, False, base=1)
    assert rc == ECAP and got == total
    assert np.array_equal(ptr, exp[0]) and (idx == -7).all() and (val == -7.0).all()
    rc, got, ptr, idx, val = _raw_dev(hip, a, COLMAJOR, [17, 40, 41, 18], 0, False, base=1)      # nothing there: DSA_OK
    assert rc == 0 and got == 0 and np.array_equal(ptr, np.ones(5, dtype=np.int64))
    # the host form: ptr filled with DSA_ECAP as well
    sel = np.asarray(LONG_COLS, dtype=np.int64)
    hptr = np.full(len(sel) + 1, -7, dtype=np.int64)
    hidx = np.full(total, -7, dtype=np.int64)
    hval = np.full(total, -7.0)
    n_out = C.c_int64(-1)
    P64, PF = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    rc = hip._mat_select_compressed(a.h, COLMAJOR, 1, sel.ctypes.data_as(P64), len(sel), hptr.ctypes.data_as(P64),
                                    hidx.ctypes.data_as(P64), hval.ctypes.data_as(PF), total - 1, C.byref(n_out))
    assert rc == ECAP and n_out.value == total
    assert np.array_equal(hptr, exp[0]) and (hidx == -7).all() and (hval == -7.0).all()


@pytest.mark.gpu
def test_bounds_and_arguments(dsa, hip, oracle):
    rng = np.random.default_rng(3)
    m, n = 50, 40
    I, J = rng.integers(1, m + 1, 300), rng.integers(1, n + 1, 300)
    I[0], J[0] = m, n
    V = rng.random(300) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    for x in (a, b):
        x[3, n + 100] = 0.0                     # an empty partition beyond size(m, 2)
    assert a.size() == b.size() == (m, n)
    for bad in (0, n + 1, n + 100):
        with pytest.raises(dsa.DsaBoundsError):
            _select_dev(a, COLMAJOR, [1, bad, 2], 64, 0)
        with pytest.raises(dsa.DsaBoundsError):
            a.select_columns([bad])
    with pytest.raises(dsa.DsaBoundsError):
        a.select_rows([m + 1])
    _check_dev(dsa, a, Expect(b, COLMAJOR), COLMAJOR, [n, 1, 2])
    import torch
    d_sel = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    ptr = torch.zeros(3, dtype=torch.int64, device="cuda")
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    good = dict(orientation=COLMAJOR, d_sel=d_sel.data_ptr(), nsel=2, d_ptr=ptr.data_ptr(), d_idx=buf.data_ptr(), d_vals=buf.data_ptr(),
                cap=64, index_bits=64, base=0)
    assert a.select_compressed_dev(**good)[1]
    for change in (dict(index_bits=16), dict(base=2), dict(base=-1), dict(orientation=2), dict(nsel=-1), dict(nsel=1 << 31),
                   dict(d_ptr=0), dict(d_sel=0), dict(d_idx=0), dict(d_vals=0), dict(cap=-1)):
        with pytest.raises(dsa.DsaArgumentError) as ei:
            a.select_compressed_dev(**dict(good, **change))
        assert ei.value.code == EARG, change
    a.sync()
    # explicit m below the largest row key: only the column that holds that row is out of bounds
    c, d = (dsa.dynamicsparse([1, 5, 2], [1, 2, 3], [1.0, 2.0, 3.0], m=3, n=3, binding=x) for x in (hip, oracle))
    assert c.size() == (3, 3)
    with pytest.raises(dsa.DsaBoundsError):
        _select_dev(c, COLMAJOR, [1, 2, 3], 64, 0)
    with pytest.raises(dsa.DsaBoundsError):
        c.select_columns([2])
    E = Expect(d, COLMAJOR)
    assert not E.in_size([2]) and E.in_size([3, 1])
    _check_dev(dsa, c, E, COLMAJOR, [3, 1, 3])
    _check_host(dsa, c, E, COLMAJOR, [3, 1, 3])
    with pytest.raises(dsa.DsaBoundsError):
        c.select_rows([5])                      # the row partition itself lies outside 1..m


@pytest.mark.gpu
def test_wide_inner_key_rowmajor(dsa, hip, oracle):
    big = (1 << 31) + 5
    I = np.array([1, 2, 3, 3, 4], dtype=np.int64)
    J = np.array([1, 7, 2, big, big], dtype=np.int64)
    V = np.array([1.5, -2.0, 3.25, 4.0, 0.125])
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    E = Expect(b, ROWMAJOR)
    sel = [3, 4, 1, 3]
    assert E.select(sel)[1].max() == big - 1
    _check_dev(dsa, a, E, ROWMAJOR, sel, bits=(64,))
    _check_host(dsa, a, E, ROWMAJOR, sel)
    with pytest.raises(dsa.DsaError) as ei:
        _select_dev(a, ROWMAJOR, sel, 32, 0)
    assert ei.value.code == EARG                # n does not fit 32-bit indices


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
        sel = rng.integers(1, E.dim_out + 1, 3000)
        _assert_same(_select_dev(a, o, sel, 32, 0), E.select(sel))
        _assert_same(a.select_columns(sel[:100]) if o == COLMAJOR else a.select_rows(sel[:100]), E.select(sel[:100]))
    for o in (COLMAJOR, ROWMAJOR):
        after = a.export_layout(o)
        for k in ("keys", "vals", "occ", "semaphores", "col_keys", "col_live"):
            assert np.array_equal(after[k].view(np.uint8), before[o][k].view(np.uint8)), (o, k)
    y = a.mul(x)
    assert a.info(ROWMAJOR)["stat_spmv_plan_builds"] == builds
    np.testing.assert_allclose(y, b.mul(x), rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_select_torch_arrays_and_product(dsa, hip, oracle):
    import torch
    rng = np.random.default_rng(5)
    m, n, nnz = 3000, 2000, 40000
    I, J = rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz)
    V = rng.random(nnz) + 0.5
    a, b = (dsa.dynamicsparse(I, J, V, binding=x) for x in (hip, oracle))
    for layout, o, dim in ((torch.sparse_csc, COLMAJOR, n), (torch.sparse_csr, ROWMAJOR, m)):
        E = Expect(b, o)
        keys = rng.permutation(dim)[:257] + 1
        exp = E.select(keys)
        for dt, given in ((torch.int32, keys.tolist()), (torch.int64, torch.from_numpy(keys).to("cuda"))):
            t = a.select_torch(layout, given, index_dtype=dt)
            assert t.layout == layout
            if o == COLMAJOR:
                assert tuple(t.shape) == (m, len(keys))
                comp, plain = t.ccol_indices(), t.row_indices()
            else:
                assert tuple(t.shape) == (len(keys), n)
                comp, plain = t.crow_indices(), t.col_indices()
            assert comp.dtype == dt and plain.dtype == dt
            _assert_same((comp.cpu().numpy(), plain.cpu().numpy(), t.values().cpu().numpy()), exp)
            ones = torch.ones((t.shape[1], 1), dtype=torch.float64, device="cuda")
            y = (t @ ones).squeeze(1).cpu().numpy()
            # the numpy product of the expected slices with a vector of ones
            if o == COLMAJOR:
                ref = np.zeros(m)
                np.add.at(ref, exp[1], exp[2])
            else:
                ref = np.add.reduceat(np.concatenate((exp[2], [0.0])), np.minimum(exp[0][:-1], len(exp[2])))
                ref[np.diff(exp[0]) == 0] = 0.0
            np.testing.assert_allclose(y, ref, rtol=1e-12, atol=0)
    t = a.select_torch(torch.sparse_csc, [])
    assert tuple(t.shape) == (m, 0) and t.values().numel() == 0
