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
