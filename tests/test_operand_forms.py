"""The helpers of api.py that turn an operand — a device address, a (rows, cols) factor pair, an (I, J, V) triple — into the form a
library call takes.  No GPU and no library call: host arrays, lists and CPU tensors only.  The message strings are the ones scale,
droptol, update_values and insert_values have always raised."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

BOTH_KINDS = "rows and cols must both be numpy arrays or both be tensors on the GPU"
FACTOR_TENSORS = "rows and cols must be 1-D float64 tensors on the GPU"
ALL_KINDS = "I, J and V must all be numpy arrays or all be tensors on the GPU"
TRIPLE_TENSORS = "I, J, V must be 1-D int64, int64, float64 tensors of one length on the GPU"
SAME_LENGTH = "rows, columns, and nonzeros do not have same length."


@pytest.fixture(scope="module")
def api(dsa):
    from dsa_amd import api
    return api


def raises(dsa, text):
    return pytest.raises(dsa.DsaArgumentError, match="^EARG: " + re.escape(text) + "$")


def address(p):
    return C.cast(p, C.c_void_p).value


def test_device_address(api):
    assert api._dptr(0) is None and api._dptr(None) is None
    p = api._dptr(0x7F0000001000)
    assert isinstance(p, C.c_void_p) and p.value == 0x7F0000001000
    assert api._dptr(np.int64(4096)).value == 4096


def test_is_tensor(api):
    assert api._is_tensor(torch.zeros(2))
    assert not any(api._is_tensor(x) for x in (np.zeros(2), [1.0, 2.0], (1, 2), None, 3.0))


def test_factor_pair_host(api):
    r = np.array([1.0, 2.0, 3.0])
    dev, (rp, nr, cp, nc), keep = api._factor_pair(r, [4, 5])
    assert dev is False and (nr, nc) == (3, 2)
    assert address(rp) == r.ctypes.data                     # a contiguous float64 array is used where it is
    assert [rp[k] for k in range(3)] == [1.0, 2.0, 3.0] and [cp[k] for k in range(2)] == [4.0, 5.0]
    # None is NULL; a factor of length 0 is "given": a non-NULL pointer
    dev, (rp, nr, cp, nc), keep = api._factor_pair(None, np.zeros(0))
    assert dev is False and rp is None and (nr, nc) == (0, 0) and address(cp)
    dev, (rp, nr, cp, nc), keep = api._factor_pair([], None)
    assert address(rp) and cp is None and (nr, nc) == (0, 0)
    assert api._factor_pair(None, None)[:2] == (False, (None, 0, None, 0))
    # a strided view is copied, not read with the wrong stride
    dev, (rp, nr, cp, nc), keep = api._factor_pair(np.arange(6.0)[::2], None)
    assert nr == 3 and [rp[k] for k in range(3)] == [0.0, 2.0, 4.0]


def test_factor_pair_errors(api, dsa):
    t = torch.ones(3, dtype=torch.float64)
    for rows, cols in ((t, np.ones(3)), ([1.0], t)):
        with raises(dsa, BOTH_KINDS):
            api._factor_pair(rows, cols)
    for bad in (t,                                                   # not on the GPU
                torch.ones(3, dtype=torch.float32),                  # wrong dtype
                torch.ones(3, 1, dtype=torch.float64)):              # 2-D
        for rows, cols in ((bad, None), (None, bad), (bad, bad)):
            with raises(dsa, FACTOR_TENSORS):
                api._factor_pair(rows, cols)


def test_triple_host(api):
    i = np.array([1, 2, 3], dtype=np.int64)
    dev, (ip, jp, vp, n, mp), mask, keep = api._triple(i, [4, 5, 6], (0.5, 1.5, 2.5), False)
    assert dev is False and n == 3 and mp is None and mask is None
    assert address(ip) == i.ctypes.data
    assert [(ip[k], jp[k], vp[k]) for k in range(3)] == [(1, 4, 0.5), (2, 5, 1.5), (3, 6, 2.5)]
    dev, (ip, jp, vp, n, mp), mask, keep = api._triple(i.reshape(3, 1), i, i, True)      # flattened; the mask is one byte per op
    assert n == 3 and mask.dtype == np.uint8 and mask.shape == (3,) and not mask.any() and address(mp) == mask.ctypes.data
    dev, (ip, jp, vp, n, mp), mask, keep = api._triple([], [], [], True)
    assert dev is False and n == 0 and mask.shape == (0,)
    hi, hj, hv = api._host_triple([1, 2], np.array([3, 4], dtype=np.int32), [5, 6])
    assert (hi.dtype, hj.dtype, hv.dtype) == (np.int64, np.int64, np.float64) and hv.tolist() == [5.0, 6.0]


def test_triple_errors(api, dsa):
    ti, tv = torch.tensor([1, 2]), torch.tensor([1.0, 2.0], dtype=torch.float64)
    for ops in ((ti, [1, 2], [1.0, 2.0]), (np.array([1, 2]), np.array([1, 2]), tv), (ti, ti, [1.0, 2.0])):
        with raises(dsa, ALL_KINDS):
            api._triple(*ops, False)
    for ops in ((ti, ti, tv),                                        # not on the GPU
                (ti.to(torch.int32), ti, tv),                        # wrong dtype
                (ti, ti, tv.to(torch.float32)),
                (ti.reshape(2, 1), ti.reshape(2, 1), tv.reshape(2, 1)),      # 2-D
                (ti, ti[:1], tv)):                                   # unequal lengths
        with raises(dsa, TRIPLE_TENSORS):
            api._triple(*ops, True)
    for ops in (([1, 2], [1], [1.0, 2.0]), ([1], [1], []), (np.zeros((2, 2)), [1, 2], [1.0, 2.0])):
        with raises(dsa, SAME_LENGTH):
            api._triple(*ops, False)
        with raises(dsa, SAME_LENGTH):
            api._host_triple(*ops)


# ---- the read-only side: dense right-hand sides, key tensors, the count-then-emit protocol --------------------------------------
X_DIMS = "X must have one or two dimensions"
X_KIND = "X must be a numpy array or a torch tensor"
X_TENSOR = "X must be a 1-D or 2-D float64 tensor on the GPU"
KEY_TENSOR = "a key tensor must be a one-dimensional int64 CUDA tensor"


def test_dense_operand_numpy(api, dsa):
    dev, p, nx, k, ldx, one_d, device, keep = api._dense_operand(np.array([1.0, 2.0, 3.0]))
    assert dev is False and device is None and (nx, k, ldx, one_d) == (3, 1, 1, True)
    assert [p[i] for i in range(3)] == [1.0, 2.0, 3.0]
    x = np.arange(12.0).reshape(4, 3)
    dev, p, nx, k, ldx, one_d, device, keep = api._dense_operand(x)
    assert (nx, k, ldx, one_d) == (4, 3, 3, False) and address(p) == x.ctypes.data       # C-contiguous float64: used where it is
    for other in (np.asfortranarray(x), x.astype(np.int32)):                             # copied into row-major float64
        dev, p, nx, k, ldx, one_d, device, keep = api._dense_operand(other)
        assert (nx, k, ldx, one_d) == (4, 3, 3, False) and address(p) != other.ctypes.data
        assert [p[i] for i in range(12)] == x.reshape(-1).tolist()
    with raises(dsa, X_DIMS):
        api._dense_operand(np.zeros((2, 2, 2)))
    dev, p, nx, k, ldx, one_d, device, keep = api._dense_operand(np.zeros((0, 3)))
    assert (nx, k, one_d) == (0, 3, False)
    assert api._dense_operand(np.zeros((3, 0)))[2:4] == (3, 0)                           # no columns: left to the library


def test_dense_operand_tensor_errors(api, dsa):
    for bad in (torch.ones(3, 2, dtype=torch.float64),                   # not on the GPU
                torch.ones(3, 2, dtype=torch.float32),                   # wrong dtype
                torch.ones(2, 2, 2, dtype=torch.float64)):               # 3-D
        with raises(dsa, X_TENSOR):
            api._dense_operand(bad)
    with raises(dsa, X_KIND):
        api._dense_operand([[1.0, 2.0], [3.0, 4.0]])


def test_key_tensor_errors(api, dsa):
    for bad in (torch.tensor([1, 2]),                                    # int64, but not on the GPU
                torch.tensor([1, 2], dtype=torch.int32),
                torch.tensor([[1, 2]])):                                 # 2-D
        with raises(dsa, KEY_TENSOR):
            api._key_tensor(bad, "cpu")


class FakeLibrary:
    """Stands in for a Binding under one matrix handle: an export whose total is `total` at the count-only call and `later` (default:
    the same) afterwards.  It writes the total, fills what fits, and answers DSA_ECAP where the library would; the calls are recorded
    as (name, cap)."""

    def __init__(self, dsa, total, later=None):
        self.dsa, self.totals, self.calls = dsa, [total, total if later is None else later], []

    def has(self, name):
        return True

    def call(self, name, h, *args):
        if name in ("mat_destroy", "mat_sync"):
            return
        *_, idx, val, cap, got = args
        total = self.totals[min(len(self.calls), 1)]
        self.calls.append((name, cap))
        got._obj.value = total
        if cap < total:
            raise self.dsa.DsaErrorException(self.dsa.binding.ECAP, "the arrays are too short")
        for k in range(total):
            idx[k], val[k] = k + 1, 0.5 * k


def test_two_calls_count_then_emit(api, dsa):
    lib = FakeLibrary(dsa, 0)
    ptr, idx, val = api.DynamicSparseMatrix(lib, 1)._two_calls("export", (7,), 3, False)
    assert lib.calls == [("export", 0)] and ptr.shape == (4,) and ptr.dtype == np.int64
    assert (idx.dtype, idx.shape, val.dtype, val.shape) == (np.int64, (0,), np.float64, (0,))
    lib = FakeLibrary(dsa, 5)
    ptr, idx, val = api.DynamicSparseMatrix(lib, 1)._two_calls("export", (7,), 3, False)
    assert lib.calls == [("export", 0), ("export", 5)]
    assert idx.tolist() == [1, 2, 3, 4, 5] and val.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    lib = FakeLibrary(dsa, 5, later=3)                                   # fewer at the emit: sliced to what was delivered
    ptr, idx, val = api.DynamicSparseMatrix(lib, 1)._two_calls("export", (), 3, False)
    assert idx.tolist() == [1, 2, 3] and val.shape == (3,)
    lib = FakeLibrary(dsa, 5, later=6)                                   # more at the emit: the library's own error
    with pytest.raises(dsa.DsaErrorException, match="^ECAP: the arrays are too short$") as e:
        api.DynamicSparseMatrix(lib, 1)._two_calls("export", (), 3, False)
    assert e.value.code == dsa.binding.ECAP and lib.calls == [("export", 0), ("export", 5)]
    lib = FakeLibrary(dsa, 5)
    ptr, idx, val = api.DynamicSparseMatrix(lib, 1)._two_calls("export", (), 3, True)
    assert lib.calls == [("export", 0)] and ptr.shape == (4,) and idx is None and val is None
    lib = FakeLibrary(dsa, 0)                                            # count_only with a total that fits: the empty arrays
    ptr, idx, val = api.DynamicSparseMatrix(lib, 1)._two_calls("export", (), 3, True)
    assert lib.calls == [("export", 0)] and idx.shape == (0,) and val.shape == (0,)


def test_torch_arrays_count_then_emit(api, dsa, monkeypatch):
    """the device helper on CPU tensors: only the hand-over to the library, which needs a GPU, is replaced — and counted"""
    waits = []
    monkeypatch.setattr(api, "_to_library", waits.append)
    a = api.DynamicSparseMatrix(FakeLibrary(dsa, 0), 1)
    totals, caps = [], []

    def call(d_ptr, d_idx, d_vals, cap):
        caps.append((cap, bool(d_idx), bool(d_vals)))
        total = totals.pop(0)
        return total, cap >= total

    totals[:] = [0]
    ptr, idx, val = a._torch_arrays("cpu", torch.int32, 3, call, "thing")
    assert caps == [(0, False, False)] and len(waits) == 1
    assert ptr.dtype == torch.int32 and ptr.shape == (4,) and idx.dtype == torch.int32 and idx.shape == (0,) and val.shape == (0,)
    del caps[:], waits[:]
    totals[:] = [5, 5]
    ptr, idx, val = a._torch_arrays("cpu", torch.int64, 3, call, "thing")
    assert caps == [(0, False, False), (5, True, True)] and len(waits) == 2      # each call behind a hand-over of its own
    assert idx.dtype == torch.int64 and idx.shape == (5,) and val.dtype == torch.float64 and val.shape == (5,)
    del caps[:], waits[:]
    totals[:] = [5]                                                      # the total is known: the emit alone
    ptr, idx, val = a._torch_arrays("cpu", torch.int64, 3, call, "thing", total=5)
    assert caps == [(5, True, True)] and len(waits) == 1 and idx.shape == (5,)
    del caps[:], waits[:]
    totals[:] = [5, 6]
    with pytest.raises(dsa.DsaErrorException, match="^ECAP: the product grew between the count and the emit$"):
        a._torch_arrays("cpu", torch.int64, 3, call, "product")
    assert caps == [(0, False, False), (5, True, True)]
