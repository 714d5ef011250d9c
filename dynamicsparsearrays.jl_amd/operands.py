"""The forms an operand or a result of api.py takes on its way to the library: a device address, a dense right-hand side, a key list,
a (rows, cols) factor pair, an (I, J, V) triple, each as host arrays or as tensors on the GPU — and the hand-over between torch's
stream and the library's.  Private to api.py, which imports every name; nothing here calls the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding as B
from .binding import P_F64, P_I64, P_U8, _f64, _i64


def _dptr(x):
    """a device address as a C argument: 0 and None are NULL"""
    return C.c_void_p(int(x)) if x else None


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _to_library(dev):
    """The hand-over of tensors on `dev` to the library, which works on streams of its own and knows nothing of torch's.  Before the
    call, here: torch's pending work on the operands and on the freshly allocated result blocks must be over, and the operands must
    stay as they are until the call has finished.  After a call that only enqueues, the owner's sync() lets torch's consumers of the
    result start behind it; a call that blocks by itself (dot, the builds, the factor and triple mutators) has no such second half."""
    import torch
    torch.cuda.current_stream(dev).synchronize()


def _dense_tensor_device(X):
    """the device of a dense right-hand side that is no numpy array: it must be a float64 tensor on the GPU"""
    import torch
    if not isinstance(X, torch.Tensor):
        raise B.DsaArgumentError(B.EARG, "X must be a numpy array or a torch tensor")
    if X.dtype != torch.float64 or not X.is_cuda or X.dim() not in (1, 2):
        raise B.DsaArgumentError(B.EARG, "X must be a 1-D or 2-D float64 tensor on the GPU")
    return X.device


def _dense_operand(X, device=None):
    """A dense right-hand side X (n x k, or 1-D: n x 1) in the row-major form the products take it: (True, address, nx, k, ldx, one_d,
    device, xx) for a float64 tensor on the GPU, used where it is unless its rows overlap or are not contiguous, else (False,
    pointer, nx, k, k, one_d, None, xx) for a numpy array, as float64 in C order.  `xx` is what the address points into.  A tensor
    without columns is refused here; an array without them by the library.  `device`: that of a tensor whose kind the caller has
    judged already (_dense_tensor_device), as matmul_selected does to look at its keys before the shape of X."""
    if isinstance(X, np.ndarray):
        one_d = X.ndim == 1
        xx = np.ascontiguousarray(X.reshape(-1, 1) if one_d else X, dtype=np.float64)
        if xx.ndim != 2:
            raise B.DsaArgumentError(B.EARG, "X must have one or two dimensions")
        nx, k = xx.shape
        return False, xx.ctypes.data_as(P_F64), nx, k, k, one_d, None, xx
    if device is None:
        device = _dense_tensor_device(X)
    one_d = X.dim() == 1
    xx = X.unsqueeze(1) if one_d else X
    nx, k = xx.shape
    if k < 1:
        raise B.DsaArgumentError(B.EARG, "X has no columns")
    if xx.stride(1) != 1 or (nx > 1 and xx.stride(0) < k):
        xx = xx.contiguous()
    return True, xx.data_ptr(), nx, k, (xx.stride(0) if nx > 1 else k), one_d, device, xx


def _key_tensor(keys, dev):
    """a key list as a contiguous one-dimensional int64 CUDA tensor: a tensor is used in place, a list or an array goes to `dev`"""
    import torch
    if isinstance(keys, torch.Tensor):
        if keys.dtype != torch.int64 or not keys.is_cuda or keys.dim() != 1:
            raise B.DsaArgumentError(B.EARG, "a key tensor must be a one-dimensional int64 CUDA tensor")
        return keys.contiguous()
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)).to(dev)


def _factor_pair(rows, cols):
    """A (rows, cols) factor pair, None = absent, in the form the library takes it: (True, (d_r, nr, d_c, nc), keep) for float64
    tensors on the GPU (device addresses of contiguous tensors, 0 = absent; torch's current stream synchronised), else
    (False, (r, nr, c, nc), keep) with pointers to float64 host arrays.  `keep` holds what the addresses point into."""
    ops = [x for x in (rows, cols) if x is not None]
    is_t = [_is_tensor(x) for x in ops]
    if any(is_t):
        import torch
        if not all(is_t):
            raise B.DsaArgumentError(B.EARG, "rows and cols must both be numpy arrays or both be tensors on the GPU")
        for x in ops:
            if x.dtype != torch.float64 or not x.is_cuda or x.dim() != 1:
                raise B.DsaArgumentError(B.EARG, "rows and cols must be 1-D float64 tensors on the GPU")
        keep = [None if x is None else x.contiguous() for x in (rows, cols)]
        _to_library(ops[0].device)
        (r, nr), (c, nc) = ((0, 0) if x is None else (x.data_ptr(), x.numel()) for x in keep)
        return True, (r, nr, c, nc), keep
    keep = [np.zeros(1, dtype=np.float64)]
    args = []
    for x in (rows, cols):
        a, p = (None, None) if x is None else _f64(np.asarray(x, dtype=np.float64))
        # a factor of length 0 is still "given": a non-NULL pointer that is never read
        if a is not None and len(a) == 0:
            p = keep[0].ctypes.data_as(P_F64)
        keep.append(a)
        args += [p, 0 if a is None else len(a)]
    return False, tuple(args), keep


def _host_triple(I, J, V):
    """(I, J, V) as flat contiguous int64, int64, float64 arrays of one length"""
    i, j = (_i64(np.asarray(x, dtype=np.int64).reshape(-1))[0] for x in (I, J))
    v = _f64(np.asarray(V, dtype=np.float64).reshape(-1))[0]
    if not (len(i) == len(j) == len(v)):
        raise B.DsaArgumentError(B.EARG, "rows, columns, and nonzeros do not have same length.")
    return i, j, v


def _triple(I, J, V, want_mask):
    """An (I, J, V) triple in the form the library takes it, with a uint8 mask of one byte per op if one is wanted:
    (True, (d_I, d_J, d_V, n, d_mask), mask, keep) for int64, int64, float64 tensors on the GPU (device addresses of contiguous
    tensors; torch's current stream synchronised), else (False, (I, J, V, n, mask), mask, keep) with pointers to host arrays.
    An absent mask, and the device mask of an empty batch, is None.  `keep` holds what the addresses point into."""
    ops = (I, J, V)
    is_t = [_is_tensor(x) for x in ops]
    if any(is_t):
        import torch
        if not all(is_t):
            raise B.DsaArgumentError(B.EARG, "I, J and V must all be numpy arrays or all be tensors on the GPU")
        for x, dt in zip(ops, (torch.int64, torch.int64, torch.float64)):
            if x.dtype != dt or not x.is_cuda or x.dim() != 1 or x.numel() != I.numel():
                raise B.DsaArgumentError(B.EARG, "I, J, V must be 1-D int64, int64, float64 tensors of one length on the GPU")
        keep = [x.contiguous() for x in ops]
        n = keep[0].numel()
        mask = torch.zeros(n, dtype=torch.uint8, device=keep[0].device) if want_mask else None
        _to_library(keep[0].device)
        return True, (*(x.data_ptr() for x in keep), n, mask.data_ptr() if want_mask and n else None), mask, keep
    i, j, v = keep = _host_triple(I, J, V)
    mask = np.zeros(len(i), dtype=np.uint8) if want_mask else None
    return False, (i.ctypes.data_as(P_I64), j.ctypes.data_as(P_I64), v.ctypes.data_as(P_F64), len(i),
                   mask.ctypes.data_as(P_U8) if want_mask else None), mask, keep
