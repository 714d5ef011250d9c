"""Host-side mirror of the reference's public surface (src/DynamicSparseArrays.jl:5-16)
over the C ABI of include/dsa.h.

The reference is a Julia package and there is no Julia toolchain in the build image,
so this Python module plays the role of the Julia wrapper for testing: same names
(`dynamicsparsevec`, `dynamicsparse`, `deletecolumn`, `deleterow`, `addrow`,
`closefillmode`, `shrink_size`, `nbpartitions`, `nnz`, indexing with ``[]``), same
argument meaning, same error behaviour (ArgumentError -> ValueError subclass,
BoundsError -> IndexError subclass, ErrorException -> RuntimeError subclass).
The Julia wrapper a maintainer would ship is in INTEGRATION.md / julia/.

Every object takes the `Binding` it runs on; by default that is the HIP product
library (`binding.product()`), which raises if it is not built.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding as B
from .binding import Binding, INFO, INFO_COUNT, P_F64, P_I64, P_U8, VP, _f64, _i64
from .operands import (  # noqa: F401
    _dense_operand, _dense_tensor_device, _dptr, _factor_pair, _host_triple, _is_tensor, _key_tensor, _to_library, _triple,
)

COMBINE = {"+": 0, "add": 0, "*": 1, "mul": 1, "last": 2}
COLMAJOR, ROWMAJOR = 0, 1
UPD_SET, UPD_ADD = 0, 1                  # DSA_UPD_*: the op of update_values_dev
INS_SKIP_EXISTING = 1                    # DSA_INS_SKIP_EXISTING: the flag of insert_values_dev
UPD_SKIP_MISSING = 1                     # ... and its flag


def _bind(b):
    return b if b is not None else B.product()


class _Handle:
    _destroy = None

    def __init__(self, b: Binding, h):
        self.b = b
        self.h = h

    def close(self):
        if self.h is not None:
            self.b.call(self._destroy, self.h)
            self.h = None

    def _require(self, symbol, message):
        """DsaArgumentError(message) on a binding that does not have `symbol`"""
        if not self.b.has(symbol):
            raise B.DsaArgumentError(B.EARG, message)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DynamicSparseVector(_Handle):
    """DynamicSparseVector{Int64,Float64}  (src/vector.jl:1-4)."""
    _destroy = "vec_destroy"

    def __getitem__(self, key):                       # src/vector.jl:73
        out = C.c_double()
        self.b.call("vec_get", self.h, int(key), C.byref(out))
        return out.value

    def __setitem__(self, key, value):                # src/vector.jl:76-81
        self.b.call("vec_set", self.h, int(key), float(value))

    def get_batch(self, keys):
        k, kp = _i64(keys)
        out = np.empty(len(k), dtype=np.float64)
        self.b.call("vec_get_batch", self.h, kp, len(k), out.ctypes.data_as(P_F64))
        return out

    def set_batch(self, keys, vals):
        k, kp = _i64(keys)
        v, vp = _f64(vals)
        assert len(k) == len(v)
        self.b.call("vec_set_batch", self.h, kp, vp, len(k))

    def __len__(self):                                # length(v)  src/vector.jl:69
        out = C.c_int64()
        self.b.call("vec_len", self.h, C.byref(out))
        return out.value

    def nnz(self):                                    # src/vector.jl:88
        out = C.c_int64()
        self.b.call("vec_nnz", self.h, C.byref(out))
        return out.value

    def shrink_size(self):                            # shrink_size!  src/vector.jl:64
        self.b.call("vec_shrink_size", self.h)

    def info(self):
        a = np.zeros(INFO_COUNT, dtype=np.int64)
        self.b.call("vec_info", self.h, a.ctypes.data_as(P_I64))
        return {k: int(a[i]) for k, i in INFO.items()}

    def nonzeros(self):
        """(keys, values) of the stored entries in iteration (slot) order  src/vector.jl:71,93-109."""
        n = self.nnz()
        k = np.empty(max(n, 1), dtype=np.int64)
        v = np.empty(max(n, 1), dtype=np.float64)
        out = C.c_int64()
        self.b.call("vec_nonzeros", self.h, k.ctypes.data_as(P_I64), v.ctypes.data_as(P_F64), len(k), C.byref(out))
        return k[:out.value], v[:out.value]

    def __iter__(self):
        k, v = self.nonzeros()
        return iter(zip(k.tolist(), v.tolist()))

    def export_layout(self):
        cap = self.info()["capacity"]
        k = np.empty(cap, dtype=np.int64)
        v = np.empty(cap, dtype=np.float64)
        o = np.empty(cap, dtype=np.uint8)
        self.b.call("vec_export_layout", self.h, k.ctypes.data_as(P_I64), v.ctypes.data_as(P_F64),
                    o.ctypes.data_as(P_U8), cap)
        return k, v, o

    def rebalance_root(self):
        self.b.call("vec_rebalance_root", self.h)

    def check(self):
        """device-side invariant checker (HIP library only): report[2..6] must be 0."""
        r = np.zeros(8, dtype=np.int64)
        self.b.call("vec_check", self.h, r.ctypes.data_as(P_I64))
        return r

    def set_wait_policy(self, policy):
        """0 (DSA_WAIT_SPIN): blocking calls poll pinned memory; 1 (DSA_WAIT_BLOCK): they park in hipStreamSynchronize first."""
        self.b.call("vec_set_wait_policy", self.h, int(policy))

    def __eq__(self, other):                          # src/vector.jl:85-87, src/pma.jl:236-266
        if not isinstance(other, DynamicSparseVector):
            return NotImplemented
        if other.b is not self.b:
            raise B.DsaArgumentError(B.EARG, "vectors of two different libraries")
        out = C.c_int32()
        self.b.call("vec_equal", self.h, other.h, C.byref(out))
        return bool(out.value)

    def axpby(self, alpha, other, beta):
        """alpha*self + beta*other as ascending (keys, values): the SparseVector of v1 + v2 / v1 - v2 / -v
        (AbstractSparseVector fallbacks over src/vector.jl:93-109; test/functional/math.jl:53-94)."""
        if other.b is not self.b:
            raise B.DsaArgumentError(B.EARG, "vectors of two different libraries")
        cap = max(self.nnz() + other.nnz(), 1)
        k = np.empty(cap, dtype=np.int64)
        v = np.empty(cap, dtype=np.float64)
        out = C.c_int64()
        self.b.call("vec_axpby", self.h, float(alpha), other.h, float(beta), k.ctypes.data_as(P_I64), v.ctypes.data_as(P_F64),
                    cap, C.byref(out))
        return k[:out.value], v[:out.value]

    def __add__(self, other):
        return self.axpby(1.0, other, 1.0)

    def __sub__(self, other):
        return self.axpby(1.0, other, -1.0)

    def __neg__(self):
        k, v = self.nonzeros()
        return k, -v

    def filter(self, f):
        """filter(f, v)  src/vector.jl:83 -> src/pma.jl:224-234: a NEW dynamic vector of the stored (key, value) pairs e with f(e)."""
        k, v = self.nonzeros()
        sel = np.fromiter((bool(f((int(a), float(b)))) for a, b in zip(k, v)), dtype=bool, count=len(k))
        return dynamicsparsevec(k[sel], v[sel], binding=self.b)

    # ---- the vector as a device operand (include/dsa.h: dsa_vec_*_dev, dsa_vec_reduce, dsa_vec_dot, dsa_vec_axpby_vec; HIP library only) ----
    _DEV_NEEDS = "dynamic vectors as device operands need the HIP product library"
    RED_KINDS = {"sum": 0, "abssum": 1, "sqsum": 2, "absmax": 3}

    def sync(self):                                   # dsa_vec_sync: everything enqueued on the vector's stream has finished
        self.b.call("vec_sync", self.h)

    def nonzeros_dev(self, d_keys, d_vals, cap):
        """the stored (key, value) pairs in ascending key order into device memory (addresses of `cap` int64 / float64 entries); returns
        their number.  More than `cap` pairs: DsaErrorException with code ECAP, nothing written.  Stream-ordered on the vector's
        stream (sync())."""
        self._require("vec_nonzeros_dev", self._DEV_NEEDS)
        out = C.c_int64()
        self.b.call("vec_nonzeros_dev", self.h, _dptr(d_keys), _dptr(d_vals), int(cap), C.byref(out))
        return out.value

    def to_torch(self, device=None):
        """(int64 tensor of the keys, float64 tensor of the values) of the stored pairs, ascending, on the GPU: they never leave HBM"""
        self._require("vec_nonzeros_dev", self._DEV_NEEDS)
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        n = self.nnz()
        k = torch.empty(n, dtype=torch.int64, device=dev)
        v = torch.empty(n, dtype=torch.float64, device=dev)
        _to_library(dev)
        got = self.nonzeros_dev(k.data_ptr(), v.data_ptr(), n)
        self.sync()
        return k[:got], v[:got]

    def to_dense_dev(self, d_x, nx):
        """d_x[0:nx] = 0, then d_x[key - 1] = value for every stored pair (device address of nx doubles): the vector as an operand of
        matmul_dev and of torch.  DsaBoundsError, with d_x untouched, when a stored key lies outside 1..nx.  Stream-ordered (sync())."""
        self._require("vec_to_dense_dev", self._DEV_NEEDS)
        self.b.call("vec_to_dense_dev", self.h, _dptr(d_x), int(nx))

    def reduce(self, kind):
        """"sum", "abssum" (sum of |v|), "sqsum" (sum of v * v) or "absmax" (max |v|, NaN propagates) over the stored values; an empty
        vector gives 0.0.  The bits depend on the stored pairs only, not on the layout."""
        self._require("vec_reduce", self._DEV_NEEDS)
        if kind not in self.RED_KINDS:
            raise B.DsaArgumentError(B.EARG, "kind must be one of %s" % ", ".join(sorted(self.RED_KINDS)))
        out = C.c_double()
        self.b.call("vec_reduce", self.h, self.RED_KINDS[kind], C.byref(out))
        return out.value

    def sum(self):
        return self.reduce("sum")

    def norm(self, p=2):
        """the p-norm of the stored values, p in {1, 2, inf} (the 2-norm is sqrt of the "sqsum" reduction, taken here)"""
        if p == 1:
            return self.reduce("abssum")
        if p == 2:
            return float(np.sqrt(self.reduce("sqsum")))
        if p in (np.inf, "inf"):
            return self.reduce("absmax")
        raise B.DsaArgumentError(B.EARG, "p must be 1, 2 or inf")

    def dot(self, other):
        """dot(v, w): `other` is a DynamicSparseVector (the sum over the keys both store) or a 1-D float64 tensor on the GPU (the sum
        of v[k] * other[k - 1]; DsaBoundsError when a stored key lies outside 1..len(other)).  Only the scalar leaves HBM."""
        self._require("vec_dot", self._DEV_NEEDS)
        out = C.c_double()
        if isinstance(other, DynamicSparseVector):
            if other.b is not self.b:
                raise B.DsaArgumentError(B.EARG, "vectors of two different libraries")
            self.b.call("vec_dot", self.h, other.h, C.byref(out))
            return out.value
        if not _is_tensor(other):
            raise B.DsaArgumentError(B.EARG, "other must be a DynamicSparseVector or a float64 tensor on the GPU")
        import torch
        if other.dtype != torch.float64 or not other.is_cuda or other.dim() != 1:
            raise B.DsaArgumentError(B.EARG, "other must be a 1-D float64 tensor on the GPU")
        x = other.contiguous()
        _to_library(x.device)
        self.b.call("vec_dot_dense_dev", self.h, _dptr(x.data_ptr()), x.numel(), C.byref(out))
        return out.value

    def axpby_vec(self, alpha, other, beta):
        """alpha*self + beta*other as a NEW DynamicSparseVector of length max(len(self), len(other)): the pairs of axpby, built on the
        device (they never leave HBM).  `other` may be `self`."""
        self._require("vec_axpby_vec", self._DEV_NEEDS)
        if other.b is not self.b:
            raise B.DsaArgumentError(B.EARG, "vectors of two different libraries")
        h = VP()
        self.b.call("vec_axpby_vec", self.h, float(alpha), other.h, float(beta), C.byref(h))
        return DynamicSparseVector(self.b, h)

    __hash__ = None


def dynamicsparsevec_dev(d_keys, d_vals, n=None, combine="+", len=None, binding: Binding | None = None) -> DynamicSparseVector:
    """dynamicsparsevec(I, V, [combine, n]) with I and V in HBM: device addresses of `n` int64 keys / float64 values (e.g.
    tensor.data_ptr()), or 1-D int64 / float64 tensors on the GPU (then n defaults to their length).  Any order, duplicates folded by
    `combine`; `len` = length of the vector (None: the largest key).  The arrays must be complete at the call (torch's current stream
    is synchronised for tensors) and are the caller's again when it returns."""
    b = _bind(binding)
    if not b.has("vec_create_dev"):
        raise B.DsaArgumentError(B.EARG, DynamicSparseVector._DEV_NEEDS)
    keep = None
    if _is_tensor(d_keys) or _is_tensor(d_vals):
        import torch
        if not (_is_tensor(d_keys) and _is_tensor(d_vals)):
            raise B.DsaArgumentError(B.EARG, "keys and values must both be device addresses or both be tensors on the GPU")
        if d_keys.dtype != torch.int64 or d_vals.dtype != torch.float64 or not d_keys.is_cuda or not d_vals.is_cuda or \
                d_keys.dim() != 1 or d_vals.dim() != 1:
            raise B.DsaArgumentError(B.EARG, "keys and values must be 1-D int64 / float64 tensors on the GPU")
        if d_keys.numel() != d_vals.numel():
            raise B.DsaArgumentError(B.EARG, "keys & nonzeros vectors must have same length.")
        keep = (d_keys.contiguous(), d_vals.contiguous())
        if n is None:
            n = keep[0].numel()
        if int(n) > keep[0].numel():
            raise B.DsaArgumentError(B.EARG, "n exceeds the length of the tensors")
        _to_library(keep[0].device)
        d_keys, d_vals = keep[0].data_ptr(), keep[1].data_ptr()
    if n is None:
        raise B.DsaArgumentError(B.EARG, "n is required with device addresses")
    h = VP()
    b.call("vec_create_dev", _dptr(d_keys), _dptr(d_vals), int(n), COMBINE[combine], -1 if len is None else int(len), C.byref(h))
    return DynamicSparseVector(b, h)


def dynamicsparsevec(I, V, combine="+", n=None, binding: Binding | None = None) -> DynamicSparseVector:
    """dynamicsparsevec(I, V, [combine, n])  src/vector.jl:44-62."""
    b = _bind(binding)
    if len(I) != len(V):
        raise B.DsaArgumentError(B.EARG, "keys & nonzeros vectors must have same length.")
    k, kp = _i64(I)
    v, vp = _f64(V)
    h = VP()
    b.call("vec_create", kp, vp, len(k), COMBINE[combine], -1 if n is None else int(n), C.byref(h))
    return DynamicSparseVector(b, h)


def import_vector_layout(keys, vals, occ, segment_capacity, n=None, binding: Binding | None = None) -> DynamicSparseVector:
    """A vector restored from an exported layout (`DynamicSparseVector.export_layout` + its segment capacity): snapshot / restore,
    and the way a test puts a structure into an arbitrary state.  No reference counterpart (include/dsa.h: dsa_vec_import_layout)."""
    b = _bind(binding)
    k, kp = _i64(keys)
    v, vp = _f64(vals)
    o = np.ascontiguousarray(occ, dtype=np.uint8)
    assert len(k) == len(v) == len(o)
    if n is None:
        n = int(k[o.astype(bool)].max()) if o.any() else 0
    h = VP()
    b.call("vec_import_layout", kp, vp, o.ctypes.data_as(P_U8), len(o), int(segment_capacity), int(n), C.byref(h))
    return DynamicSparseVector(b, h)


class PackedCSC(_Handle):
    """PackedCSC{Int64,Float64}  (src/pcsr.jl:4-9)."""
    _destroy = "pcsc_destroy"

    def __getitem__(self, idx):                       # src/pcsr.jl:228-232
        key, partition = idx
        out = C.c_double()
        self.b.call("pcsc_get", self.h, int(key), int(partition), C.byref(out))
        return out.value

    def __setitem__(self, idx, value):                # src/pcsr.jl:294-310
        key, partition = idx
        self.b.call("pcsc_set", self.h, float(value), int(key), int(partition))

    def deletepartition(self, partition):             # src/pcsr.jl:188-204
        self.b.call("pcsc_deletepartition", self.h, int(partition))

    def nnz(self):
        out = C.c_int64()
        self.b.call("pcsc_nnz", self.h, C.byref(out))
        return out.value

    def nbpartitions(self):
        out = C.c_int64()
        self.b.call("pcsc_nbpartitions", self.h, C.byref(out))
        return out.value

    def info(self):
        a = np.zeros(INFO_COUNT, dtype=np.int64)
        self.b.call("pcsc_info", self.h, a.ctypes.data_as(P_I64))
        return {k: int(a[i]) for k, i in INFO.items()}

    def export_layout(self):
        inf = self.info()
        cap, tl = inf["capacity"], max(inf["table_len"], 1)
        k = np.empty(cap, dtype=np.int64)
        v = np.empty(cap, dtype=np.float64)
        o = np.empty(cap, dtype=np.uint8)
        s = np.zeros(tl, dtype=np.int64)
        self.b.call("pcsc_export_layout", self.h, k.ctypes.data_as(P_I64), v.ctypes.data_as(P_F64),
                    o.ctypes.data_as(P_U8), cap, s.ctypes.data_as(P_I64), tl)
        return k, v, o, s[:inf["table_len"]]

    def check(self):
        """device-side invariant checker (HIP library only): report[2..6] must be 0."""
        r = np.zeros(8, dtype=np.int64)
        self.b.call("pcsc_check", self.h, r.ctypes.data_as(P_I64))
        return r


def packedcsc(row_keys, values, combine="+", binding: Binding | None = None) -> PackedCSC:
    """PackedCSC(row_keys::Vector{Vector}, values::Vector{Vector}, combine)  src/pcsr.jl:26-63."""
    b = _bind(binding)
    assert len(row_keys) == len(values)
    colptr = np.zeros(len(row_keys) + 1, dtype=np.int64)
    for p, r in enumerate(row_keys):
        assert len(r) == len(values[p])
        colptr[p + 1] = colptr[p] + len(r)
    rk = np.array([x for r in row_keys for x in r], dtype=np.int64)
    vv = np.array([x for r in values for x in r], dtype=np.float64)
    if len(rk) == 0:
        rk = np.zeros(1, dtype=np.int64)
        vv = np.zeros(1, dtype=np.float64)
    h = VP()
    b.call("pcsc_create", colptr.ctypes.data_as(P_I64), len(row_keys), rk.ctypes.data_as(P_I64),
           vv.ctypes.data_as(P_F64), COMBINE[combine], C.byref(h))
    return PackedCSC(b, h)


def import_packedcsc_layout(keys, vals, occ, segment_capacity, semaphores, binding: Binding | None = None) -> PackedCSC:
    """A PackedCSC restored from an exported layout (include/dsa.h: dsa_pcsc_import_layout)."""
    b = _bind(binding)
    k, kp = _i64(keys)
    v, vp = _f64(vals)
    o = np.ascontiguousarray(occ, dtype=np.uint8)
    s, sp = _i64(semaphores if len(semaphores) else [0])
    h = VP()
    b.call("pcsc_import_layout", kp, vp, o.ctypes.data_as(P_U8), len(o), int(segment_capacity), sp, len(semaphores), C.byref(h))
    return PackedCSC(b, h)


def packedcsc_empty(binding: Binding | None = None) -> PackedCSC:
    b = _bind(binding)
    h = VP()
    b.call("pcsc_create_empty", C.byref(h))
    return PackedCSC(b, h)


class Transposed:
    """transpose(mat)  src/operations.jl:1-9."""

    def __init__(self, mat):
        self.array = mat

    def __getitem__(self, idx):
        r, c = idx
        return self.array[c, r]

    def __setitem__(self, idx, val):
        r, c = idx
        self.array[c, r] = val

    def size(self):
        m, n = self.array.size()
        return (n, m)

    def mul(self, x, **kw):
        return self.array.mul(x, transpose=True, **kw)

    def mul_vec(self, x):
        return self.array.mul_vec(x, transpose=True)

    def matmul(self, X):
        return self.array.matmul(X, transpose=True)

    def __matmul__(self, X):
        return self.array.matmul(X, transpose=True)

    def matmul_selected(self, keys, X):
        """rows `keys` of transpose(mat) * X: mat[:, keys]' * X"""
        return self.array.matmul_selected(keys, X, transpose=True)

    def matmul_sparse(self, S):
        """transpose(mat) * S for a sparse S (CSC triple or torch.sparse_csc tensor): see DynamicSparseMatrix.matmul_sparse"""
        return self.array.matmul_sparse(S, transpose=True)

    def reduce(self, kind, per, out=None):
        """the reduction per row / column of the transpose: per column / row of the matrix"""
        if per not in ("row", "column"):
            raise B.DsaArgumentError(B.EARG, "per must be 'row' or 'column'")
        return self.array.reduce(kind, "column" if per == "row" else "row", out=out)

    def update_values(self, I, J, V, op="set", missing="error"):
        """transpose(mat)[I[k], J[k]] = V[k] on stored cells: update_values of the matrix with the sides swapped"""
        return self.array.update_values(J, I, V, op=op, missing=missing)

    def add_values(self, I, J, V, missing="error"):
        return self.array.update_values(J, I, V, op="add", missing=missing)

    def insert_values(self, I, J, V, existing="error"):
        """transpose(mat)[I[k], J[k]] created with V[k]: insert_values of the matrix with the sides swapped"""
        return self.array.insert_values(J, I, V, existing=existing)

    def upsert(self, I, J, V):
        return self.array.upsert(J, I, V)

    def assemble(self, I, J, V, op="add"):
        """transpose(mat)[I[k], J[k]] += V[k] (or = V[k]) for any triples: assemble of the matrix with the sides swapped"""
        return self.array.assemble(J, I, V, op=op)


class DynamicSparseMatrix(_Handle):
    """DynamicSparseMatrix{Int64,Int64,Float64}  (src/matrix.jl:1-8)."""
    _destroy = "mat_destroy"

    def __setitem__(self, idx, val):                  # src/matrix.jl:43-62
        row, col = idx
        self.b.call("mat_set", self.h, float(val), int(row), int(col))

    def __getitem__(self, idx):                       # src/matrix.jl:64-68
        row, col = idx
        out = C.c_double()
        self.b.call("mat_get", self.h, int(row), int(col), C.byref(out))
        return out.value

    def set_batch(self, I, J, V):
        i, ip = _i64(I)
        j, jp = _i64(J)
        v, vp = _f64(V)
        assert len(i) == len(j) == len(v)
        self.b.call("mat_set_batch", self.h, ip, jp, vp, len(i))

    def get_batch(self, I, J):
        i, ip = _i64(I)
        j, jp = _i64(J)
        out = np.empty(len(i), dtype=np.float64)
        self.b.call("mat_get_batch", self.h, ip, jp, len(i), out.ctypes.data_as(P_F64))
        return out

    def addrow(self, row, colids, vals):              # addrow!  src/matrix.jl:113-124
        c, cp = _i64(colids)
        v, vp = _f64(vals)
        assert len(c) == len(v)
        self.b.call("mat_addrow", self.h, int(row), cp, vp, len(c))

    def closefillmode(self):                          # closefillmode!  src/matrix.jl:126-134
        self.b.call("mat_closefillmode", self.h)

    def deletecolumn(self, col):                      # deletecolumn!  src/matrix.jl:95-102
        self.b.call("mat_deletecolumn", self.h, int(col))

    def deleterow(self, row):                         # deleterow!  src/matrix.jl:104-111
        self.b.call("mat_deleterow", self.h, int(row))

    def _view(self, name, key):
        cap = 64
        while True:
            k = np.empty(cap, dtype=np.int64)
            v = np.empty(cap, dtype=np.float64)
            n = C.c_int64()
            try:
                self.b.call(name, self.h, int(key), k.ctypes.data_as(P_I64), v.ctypes.data_as(P_F64), cap, C.byref(n))
            except B.DsaError as e:
                if e.code == B.ECAP:
                    cap *= 8
                    continue
                raise
            return list(zip(k[:n.value].tolist(), v[:n.value].tolist()))

    def col_view(self, col):                          # @view m[:, col]  src/matrix.jl:83-88
        return self._view("mat_col_view", col)

    def row_view(self, row):                          # @view m[row, :]  src/matrix.jl:70-81
        return self._view("mat_row_view", row)

    def _view_dev(self, name, key, d_keys, d_vals, cap):
        """the view delivered into HBM: d_keys / d_vals are device addresses (int64 / float64 arrays of cap entries, e.g.
        tensor.data_ptr()); returns the number of cells; the copy is enqueued on the orientation's stream (sync())"""
        n = C.c_int64()
        self.b.call(name, self.h, int(key), _dptr(d_keys), _dptr(d_vals), int(cap), C.byref(n))
        return n.value

    def sync(self):                                   # dsa_mat_sync: everything enqueued on the handle's streams has finished
        self.b.call("mat_sync", self.h)

    def col_view_dev(self, col, d_rows, d_vals, cap):  # @view m[:, col] into device memory
        return self._view_dev("mat_col_view_dev", col, d_rows, d_vals, cap)

    def row_view_dev(self, row, d_cols, d_vals, cap):  # @view m[row, :] into device memory
        return self._view_dev("mat_row_view_dev", row, d_cols, d_vals, cap)

    def col_slice(self, col):                         # m[:, col]  src/pcsr.jl:285-291
        h = VP()
        self.b.call("mat_col_slice", self.h, int(col), C.byref(h))
        return DynamicSparseVector(self.b, h)

    def row_slice(self, row):                         # m[row, :]  src/pcsr.jl:269-283
        h = VP()
        self.b.call("mat_row_slice", self.h, int(row), C.byref(h))
        return DynamicSparseVector(self.b, h)

    def nnz(self):
        out = C.c_int64()
        self.b.call("mat_nnz", self.h, C.byref(out))
        return out.value

    def size(self):
        m, n = C.c_int64(), C.c_int64()
        self.b.call("mat_size", self.h, C.byref(m), C.byref(n))
        return (m.value, n.value)

    def nbpartitions(self, orientation):
        out = C.c_int64()
        self.b.call("mat_nbpartitions", self.h, orientation, C.byref(out))
        return out.value

    def info(self, orientation):
        a = np.zeros(INFO_COUNT, dtype=np.int64)
        self.b.call("mat_info", self.h, orientation, a.ctypes.data_as(P_I64))
        return {k: int(a[i]) for k, i in INFO.items()}

    def export_layout(self, orientation):
        inf = self.info(orientation)
        cap, tl = inf["capacity"], max(inf["table_len"], 1)
        k = np.empty(cap, dtype=np.int64)
        v = np.empty(cap, dtype=np.float64)
        o = np.empty(cap, dtype=np.uint8)
        s = np.zeros(tl, dtype=np.int64)
        ck = np.zeros(tl, dtype=np.int64)
        cl = np.zeros(tl, dtype=np.uint8)
        self.b.call("mat_export_layout", self.h, orientation, k.ctypes.data_as(P_I64), v.ctypes.data_as(P_F64),
                    o.ctypes.data_as(P_U8), cap, s.ctypes.data_as(P_I64), ck.ctypes.data_as(P_I64),
                    cl.ctypes.data_as(P_U8), tl)
        n = inf["table_len"]
        return dict(keys=k, vals=v, occ=o, semaphores=s[:n], col_keys=ck[:n], col_live=cl[:n], info=inf)

    def rebalance_root(self, orientation):
        self.b.call("mat_rebalance_root", self.h, orientation)

    # ---- what the HIP-only calls below share ---------------------------------------------------------------------------------------
    def _fits(self, name, *args):
        """`name`(h, *args, &total) -> (total, fits): with DSA_ECAP the total is known and the arrays of `cap` entries are untouched"""
        got = C.c_int64()
        try:
            self.b.call(name, self.h, *args, C.byref(got))
        except B.DsaError as e:
            if e.code != B.ECAP:
                raise
            return got.value, False
        return got.value, True

    def _two_calls(self, name, head, nouter, count_only):
        """the host form `name`(h, *head, ptr, idx, vals, cap, &total) of a key-list export or sparse product: the count-only call,
        then, if it said DSA_ECAP, the one into arrays of `total` entries, whose errors are the caller's"""
        ptr = np.empty(nouter + 1, dtype=np.int64)
        total, fits = self._fits(name, *head, ptr.ctypes.data_as(P_I64), None, None, 0)
        if count_only and not fits:
            return ptr, None, None
        idx, val = np.empty(total, dtype=np.int64), np.empty(total, dtype=np.float64)
        if not fits:
            got = C.c_int64()
            self.b.call(name, self.h, *head, ptr.ctypes.data_as(P_I64), idx.ctypes.data_as(P_I64), val.ctypes.data_as(P_F64), total, C.byref(got))
            total = got.value
        return ptr, idx[:total], val[:total]

    # the torch forms of the three exports: the arrays never leave HBM
    @staticmethod
    def _torch_format(layout, index_dtype):
        """(orientation, index dtype, index bits, the current device) of a torch export"""
        import torch
        if index_dtype is None:
            index_dtype = torch.int64
        if layout not in (torch.sparse_csr, torch.sparse_csc):
            raise B.DsaArgumentError(B.EARG, "layout must be torch.sparse_csr or torch.sparse_csc")
        if index_dtype not in (torch.int32, torch.int64):
            raise B.DsaArgumentError(B.EARG, "index_dtype must be torch.int32 or torch.int64")
        return (ROWMAJOR if layout == torch.sparse_csr else COLMAJOR, index_dtype, 32 if index_dtype == torch.int32 else 64,
                torch.device("cuda", torch.cuda.current_device()))

    def _torch_arrays(self, dev, index_dtype, nouter, call, what, total=None):
        """(ptr[nouter + 1], idx, vals) of a device export or sparse product `what` as tensors.  call(d_ptr, d_idx, d_vals, cap) ->
        (total, fits): the count-only call (cap = 0, 0 for idx / vals) unless the total is given, then the call into arrays of `total`
        entries, each behind a hand-over of its own, for each has fresh blocks"""
        import torch
        ptr = torch.empty(nouter + 1, dtype=index_dtype, device=dev)
        fits = False
        if total is None:
            _to_library(dev)
            total, fits = call(ptr.data_ptr(), 0, 0, 0)
        idx = torch.empty(max(total, 1), dtype=index_dtype, device=dev)
        val = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
        if not fits:
            _to_library(dev)
            total, fits = call(ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), total)
            if not fits:
                raise B.DsaErrorException(B.ECAP, "the %s grew between the count and the emit" % what)
        self.sync()
        return ptr, idx[:total], val[:total]

    @staticmethod
    def _torch_tensor(orientation, arrays, nouter, ninner):
        import torch
        if orientation == ROWMAJOR:
            return torch.sparse_csr_tensor(*arrays, size=(nouter, ninner))
        return torch.sparse_csc_tensor(*arrays, size=(ninner, nouter))

    # ---- compressed export (include/dsa.h: dsa_mat_to_compressed[_dev]; HIP library only) ----------------------------------------
    def _compressed(self, orientation, base):
        self._require("mat_to_compressed", "compressed export needs the HIP product library")
        m, n = self.size()
        outer = m if orientation == ROWMAJOR else n
        cap = self.nnz()
        ptr = np.empty(outer + 1, dtype=np.int64)
        idx = np.empty(max(cap, 1), dtype=np.int64)
        val = np.empty(max(cap, 1), dtype=np.float64)
        got = C.c_int64()
        self.b.call("mat_to_compressed", self.h, orientation, int(base), ptr.ctypes.data_as(P_I64), idx.ctypes.data_as(P_I64),
                    val.ctypes.data_as(P_F64), cap, C.byref(got))
        return ptr, idx[:got.value], val[:got.value]

    def to_csr(self, base=0):
        """scipy-style (indptr, indices, data) of the rows 1..m, int64 indices counted from `base` (0 or 1)"""
        return self._compressed(ROWMAJOR, base)

    def to_csc(self, base=0):
        """scipy-style (indptr, indices, data) of the columns 1..n, int64 indices counted from `base` (0 or 1)"""
        return self._compressed(COLMAJOR, base)

    def findnz(self):
        """findnz(m): 1-based (I, J, V) of the stored entries in column-major order (SparseArrays.findnz)"""
        ptr, rows, vals = self.to_csc(base=1)
        cols = np.repeat(np.arange(1, len(ptr), dtype=np.int64), np.diff(ptr))
        return rows, cols, vals

    def to_compressed_dev(self, orientation, d_ptr, d_idx, d_vals, cap, index_bits=64, base=0):
        """the compressed form into device memory (device addresses, e.g. tensor.data_ptr()); enqueued on the orientation's stream
        (sync()); returns nnz"""
        self._require("mat_to_compressed", "compressed export needs the HIP product library")
        got = C.c_int64()
        self.b.call("mat_to_compressed_dev", self.h, int(orientation), int(index_bits), int(base), _dptr(d_ptr),
                    _dptr(d_idx), _dptr(d_vals), int(cap), C.byref(got))
        return got.value

    def to_torch(self, layout, index_dtype=None):
        """torch.sparse_csr_tensor (layout torch.sparse_csr, from rowmajor) or torch.sparse_csc_tensor (torch.sparse_csc, from
        colmajor) of size(m) on the current device; the arrays never leave HBM"""
        self._require("mat_to_compressed", "compressed export needs the HIP product library")
        orientation, index_dtype, bits, dev = self._torch_format(layout, index_dtype)
        m, n = self.size()
        outer, inner = (m, n) if orientation == ROWMAJOR else (n, m)
        arrays = self._torch_arrays(dev, index_dtype, outer, what="matrix", total=self.nnz(), call=lambda d_ptr, d_idx, d_vals, cap: (
            self.to_compressed_dev(orientation, d_ptr, d_idx, d_vals, cap, index_bits=bits), True))
        return self._torch_tensor(orientation, arrays, outer, inner)

    # ---- selected export (include/dsa.h: dsa_mat_select_compressed[_dev]; HIP library only) --------------------------------------
    def select_compressed_dev(self, orientation, d_sel, nsel, d_ptr, d_idx, d_vals, cap, index_bits=64, base=0):
        """A[:, sel] (COLMAJOR) / A[sel, :] (ROWMAJOR) in compressed form into device memory: d_sel = nsel int64 outer keys (1-based,
        any order, repeats allowed), d_ptr = nsel + 1 indices, d_idx / d_vals = cap entries (device addresses, e.g. tensor.data_ptr();
        0 for idx / vals with cap = 0: the count-only call).  Enqueued on the orientation's stream (sync()).  Returns (total, fits):
        the number of selected cells and whether they were delivered; with fits False (cap < total) only ptr has been written."""
        self._require("mat_select_compressed", "the selected export needs the HIP product library")
        return self._fits("mat_select_compressed_dev", int(orientation), int(index_bits), int(base), _dptr(d_sel), int(nsel),
                          _dptr(d_ptr), _dptr(d_idx), _dptr(d_vals), int(cap))

    def _select(self, orientation, keys, base, count_only=False):
        self._require("mat_select_compressed", "the selected export needs the HIP product library")
        sel, sp = _i64(keys)
        if sel.ndim != 1:
            raise B.DsaArgumentError(B.EARG, "the selection must be one-dimensional")
        return self._two_calls("mat_select_compressed", (int(orientation), int(base), sp, len(sel)), len(sel), count_only)

    def select_columns(self, cols, base=0):
        """A[:, cols] as scipy-style CSC arrays (indptr, indices, data) with len(cols) columns: int64 indices counted from `base`"""
        return self._select(COLMAJOR, cols, base)

    def select_rows(self, rows, base=0):
        """A[rows, :] as scipy-style CSR arrays (indptr, indices, data) with len(rows) rows: int64 indices counted from `base`"""
        return self._select(ROWMAJOR, rows, base)

    def count_columns(self, cols):
        """stored entries of each of the columns `cols` (0 for a column that is not there)"""
        return np.diff(self._select(COLMAJOR, cols, 0, count_only=True)[0])

    def count_rows(self, rows):
        """stored entries of each of the rows `rows` (0 for a row that is not there)"""
        return np.diff(self._select(ROWMAJOR, rows, 0, count_only=True)[0])

    def select_torch(self, layout, keys, index_dtype=None):
        """A[:, keys] as torch.sparse_csc_tensor of shape (m, len(keys)) (layout torch.sparse_csc) or A[keys, :] as
        torch.sparse_csr_tensor of shape (len(keys), n) (torch.sparse_csr) on the current device.  `keys`: a list, a numpy array, or
        an int64 CUDA tensor (used in place); the arrays never leave HBM."""
        self._require("mat_select_compressed", "the selected export needs the HIP product library")
        orientation, index_dtype, bits, dev = self._torch_format(layout, index_dtype)
        sel = _key_tensor(keys, dev)
        nsel = sel.numel()
        m, n = self.size()
        arrays = self._torch_arrays(dev, index_dtype, nsel, what="selection", call=lambda d_ptr, d_idx, d_vals, cap: (
            self.select_compressed_dev(orientation, sel.data_ptr(), nsel, d_ptr, d_idx, d_vals, cap, index_bits=bits)))
        return self._torch_tensor(orientation, arrays, nsel, n if orientation == ROWMAJOR else m)

    # ---- submatrix export (include/dsa.h: dsa_mat_submatrix_compressed[_dev]; HIP library only) ----------------------------------
    def submatrix_compressed_dev(self, orientation, d_outer, nouter, d_inner, ninner, d_ptr, d_idx, d_vals, cap, index_bits=64, base=0):
        """A[inner, outer] as CSC (COLMAJOR: outer = column keys, inner = row keys) / A[outer, inner] as CSR (ROWMAJOR) into device
        memory: d_outer = nouter int64 outer keys (1-based, any order, repeats allowed), d_inner = ninner DISTINCT int64 inner keys
        (1-based, any order), d_ptr = nouter + 1 indices, d_idx / d_vals = cap entries (device addresses; 0 for idx / vals with
        cap = 0: the count-only call).  A delivered cell's index is the position of its key in the inner list + base.  Enqueued on the
        orientation's stream (sync()).  Returns (total, fits) like select_compressed_dev."""
        self._require("mat_submatrix_compressed", "the submatrix export needs the HIP product library")
        return self._fits("mat_submatrix_compressed_dev", int(orientation), int(index_bits), int(base), _dptr(d_outer), int(nouter),
                          _dptr(d_inner), int(ninner), _dptr(d_ptr), _dptr(d_idx), _dptr(d_vals),
                          int(cap))

    @staticmethod
    def _submatrix_sides(rows, cols, layout):
        if layout not in ("csr", "csc"):
            raise B.DsaArgumentError(B.EARG, "layout must be 'csr' or 'csc'")
        return (ROWMAJOR, rows, cols) if layout == "csr" else (COLMAJOR, cols, rows)

    def _submatrix(self, rows, cols, layout, base, count_only=False):
        self._require("mat_submatrix_compressed", "the submatrix export needs the HIP product library")
        orientation, outer, inner = self._submatrix_sides(rows, cols, layout)
        out, op = _i64(outer)
        inn, ip = _i64(inner)
        if out.ndim != 1 or inn.ndim != 1:
            raise B.DsaArgumentError(B.EARG, "the key lists must be one-dimensional")
        return self._two_calls("mat_submatrix_compressed", (int(orientation), int(base), op, len(out), ip, len(inn)), len(out), count_only)

    def submatrix(self, rows, cols, layout="csr", base=0):
        """A[rows, cols] as scipy-style arrays (indptr, indices, data) of a len(rows) x len(cols) matrix: CSR (layout "csr": one slice
        per entry of `rows`, which may repeat; `cols` distinct) or CSC ("csc": one slice per entry of `cols`; `rows` distinct).  int64
        indices = position in the other list + `base`; they ascend within a slice iff that list ascends."""
        return self._submatrix(rows, cols, layout, base)

    def count_submatrix(self, rows, cols, layout="csr"):
        """entries of A[rows, cols] per row of `rows` (layout "csr") or per column of `cols` ("csc")"""
        return np.diff(self._submatrix(rows, cols, layout, 0, count_only=True)[0])

    def submatrix_torch(self, layout, rows, cols, index_dtype=None):
        """A[rows, cols] as torch.sparse_csr_tensor / torch.sparse_csc_tensor of shape (len(rows), len(cols)) on the current device.
        `rows`, `cols`: lists, numpy arrays, or int64 CUDA tensors (used in place); the arrays never leave HBM.  The inner list (cols
        for CSR, rows for CSC) must ascend strictly, because torch expects sorted indices within a slice."""
        self._require("mat_submatrix_compressed", "the submatrix export needs the HIP product library")
        orientation, index_dtype, bits, dev = self._torch_format(layout, index_dtype)
        d_rows, d_cols = _key_tensor(rows, dev), _key_tensor(cols, dev)
        outer, inner = (d_rows, d_cols) if orientation == ROWMAJOR else (d_cols, d_rows)
        nouter, ninner = outer.numel(), inner.numel()
        if ninner > 1 and not bool((inner[1:] > inner[:-1]).all()):
            raise B.DsaArgumentError(B.EARG, "the inner key list must ascend strictly (torch expects sorted indices)")
        arrays = self._torch_arrays(dev, index_dtype, nouter, what="submatrix", call=lambda d_ptr, d_idx, d_vals, cap: (
            self.submatrix_compressed_dev(orientation, outer.data_ptr(), nouter, inner.data_ptr(), ninner, d_ptr, d_idx, d_vals, cap,
                                          index_bits=bits)))
        return self._torch_tensor(orientation, arrays, nouter, ninner)

    # ---- combine (include/dsa.h: dsa_mat_combine; HIP library only) ---------------------------------------------------------------
    def combine(self, other=None, alpha=1.0, beta=1.0, row_off=0, col_off=0, m=None, n=None):
        """alpha * self + beta * other as a NEW matrix, built on the device; `other`'s keys are shifted by (row_off, col_off).  It is
        the matrix dynamicsparse(I, J, V, m, n) builds from the stored cells of self in findnz order, scaled by alpha, followed by
        those of other, shifted and scaled by beta: a cell present in both is their sum (a stored zero when it cancels: dropzeros()).
        other=None: a scaled copy.  m, n: size of the result (default: the smallest that holds both operands).  A non-zero offset
        needs both operands inside their size() in that dimension (DsaBoundsError).  The operands are only read."""
        self._require("mat_combine", "combining matrices needs the HIP product library")
        if other is not None:
            if not isinstance(other, DynamicSparseMatrix):
                raise B.DsaArgumentError(B.EARG, "the second operand must be a DynamicSparseMatrix")
            if other.b is not self.b:
                raise B.DsaArgumentError(B.EARG, "matrices of two different libraries")
        h = VP()
        self.b.call("mat_combine", self.h, float(alpha), None if other is None else other.h, float(beta), int(row_off), int(col_off),
                    -1 if m is None else int(m), -1 if n is None else int(n), C.byref(h))
        return DynamicSparseMatrix(self.b, h)

    def copy(self):
        """an independent matrix with the same stored cells and size (a fresh build: the layout is that of dynamicsparse(findnz(A)...))"""
        return self.combine()

    def __add__(self, other):
        if not isinstance(other, DynamicSparseMatrix):
            return NotImplemented
        return self.combine(other)

    def __sub__(self, other):
        if not isinstance(other, DynamicSparseMatrix):
            return NotImplemented
        return self.combine(other, beta=-1.0)

    def __neg__(self):
        return self.combine(alpha=-1.0)

    def __mul__(self, alpha):
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)):
            return NotImplemented
        return self.combine(alpha=float(alpha))

    __rmul__ = __mul__

    def check(self, orientation):
        """device-side invariant checker (HIP library only): report[2..6] must be 0."""
        r = np.zeros(8, dtype=np.int64)
        self.b.call("mat_check", self.h, orientation, r.ctypes.data_as(P_I64))
        return r

    def set_wait_policy(self, policy):
        """0 (DSA_WAIT_SPIN): blocking calls poll pinned memory; 1 (DSA_WAIT_BLOCK): they park in hipStreamSynchronize first."""
        self.b.call("mat_set_wait_policy", self.h, int(policy))

    def transpose(self):
        return Transposed(self)

    @property
    def T(self):
        return Transposed(self)

    def mul(self, x, transpose=False, dense_out=None, out=None):
        """mat * v / transpose(mat) * v  (src/operations.jl:14-36).

        `x` is a DynamicSparseVector, a (indices, values) pair of the stored entries
        (ascending indices), or a dense numpy array.  Sparse inputs return
        (indices, values) of the touched rows, ascending — the `_mul_output` shape;
        a dense array returns a dense array of length size(mat, 1 | 2).
        `out` = (int64 array, float64 array) the caller keeps across products (each at least as long as the result): the
        result is fetched into them and views are returned — a long result does not pay for fresh pages every time.
        """
        if isinstance(x, np.ndarray):
            m, n = self.size()
            ny = (n if transpose else m) if dense_out is None else dense_out
            xx, xp = _f64(x)
            y = np.empty(max(ny, 1), dtype=np.float64)
            self.b.call("mat_spmv_dense", self.h, 1 if transpose else 0, xp, len(xx), y.ctypes.data_as(P_F64), ny)
            return y[:ny]
        if isinstance(x, DynamicSparseVector):
            xi, xv = x.nonzeros()
        else:
            xi, xv = x
        xi, xip = _i64(xi)
        xv, xvp = _f64(xv)
        tr = 1 if transpose else 0
        n_out = C.c_int64()
        if "mat_spmv_sparse_begin" in self.b.SIGNATURES:
            # compute, learn the number of touched rows, allocate exactly that, fetch (one product, whatever the result size)
            self.b.call("mat_spmv_sparse_begin", self.h, tr, xip, xvp, len(xi), C.byref(n_out))
            cnt = n_out.value
            if out is not None and len(out[0]) >= cnt and len(out[1]) >= cnt:
                yi, yv = out[0][:cnt], out[1][:cnt]
            else:
                yi = np.empty(cnt, dtype=np.int64)
                yv = np.empty(cnt, dtype=np.float64)
            if cnt:
                self.b.call("mat_spmv_sparse_fetch", self.h, yi.ctypes.data_as(P_I64), yv.ctypes.data_as(P_F64), cnt, C.byref(n_out))
            return yi, yv
        m, n = self.size()
        cap = max(n if transpose else m, 1)                # the touched rows are at most all rows
        yi = np.empty(cap, dtype=np.int64)
        yv = np.empty(cap, dtype=np.float64)
        self.b.call("mat_spmv_sparse", self.h, tr, xip, xvp, len(xi), yi.ctypes.data_as(P_I64), yv.ctypes.data_as(P_F64), cap, C.byref(n_out))
        return yi[:n_out.value].copy(), yv[:n_out.value].copy()

    def mul_vec(self, x, transpose=False):
        """mat * v / transpose(mat) * v for a DynamicSparseVector, as a NEW DynamicSparseVector of length size(mat, 1 | 2): the vector
        dynamicsparsevec(*mul(x), n=size) would build, with x, the product and the result never leaving HBM."""
        self._require("mat_mul_vec", "mul_vec needs the HIP product library")
        if not isinstance(x, DynamicSparseVector):
            raise B.DsaArgumentError(B.EARG, "x must be a DynamicSparseVector (mul takes pairs and dense arrays)")
        if x.b is not self.b:
            raise B.DsaArgumentError(B.EARG, "operands of two different libraries")
        h = VP()
        self.b.call("mat_mul_vec", self.h, 1 if transpose else 0, x.h, C.byref(h))
        return DynamicSparseVector(self.b, h)

    def mul_dev(self, d_xi, d_xv, nx, d_yi, d_yv, cap, d_count, transpose=False):
        """the sparse product with every operand in HBM (device addresses, e.g. tensor.data_ptr()); stream-ordered, no host wait"""
        self.b.call("mat_spmv_sparse_dev", self.h, 1 if transpose else 0, _dptr(d_xi), _dptr(d_xv), int(nx),
                    _dptr(d_yi), _dptr(d_yv), int(cap), _dptr(d_count))

    # ---- dense multi-vector product (include/dsa.h: dsa_mat_spmm_dense[_dev]; HIP library only) ------------------------------------
    def matmul(self, X, transpose=False):
        """mat * X / transpose(mat) * X for k right-hand sides: column j of the result is mul(X[:, j]).

        A 2-D float64 numpy array returns a new (size(mat, 1 | 2), k) array; a 2-D float64 torch tensor on the GPU returns a new
        tensor on the same device (the operands never leave HBM); a 1-D input returns the 1-D product.  Inputs that are not
        row-contiguous are copied into that form first."""
        self._require("mat_spmm_dense", "the multi-vector product needs the HIP product library")
        tr = 1 if transpose else 0
        m, n = self.size()
        ny = n if transpose else m
        dev, xp, nx, k, ldx, one_d, device, xx = _dense_operand(X)
        y = xx.new_empty((ny, k)) if dev else np.empty((ny, k), dtype=np.float64)
        if dev:
            _to_library(device)
            self.matmul_dev(xp, nx, k, y.data_ptr(), ny, ldx=ldx, ldy=k, transpose=transpose)
            self.sync()
        else:
            self.b.call("mat_spmm_dense", self.h, tr, xp, nx, k, ldx, y.ctypes.data_as(P_F64), ny, k)
        return y[:, 0] if one_d else y

    def __matmul__(self, X):
        return self.matmul(X)

    def matmul_dev(self, d_x, nx, k, d_y, ny, ldx=None, ldy=None, transpose=False):
        """the multi-vector product with both operands in HBM (device addresses, e.g. tensor.data_ptr()), row-major with leading
        dimensions ldx / ldy (default k); stream-ordered on the orientation's stream, no host wait (sync())"""
        self._require("mat_spmm_dense", "the multi-vector product needs the HIP product library")
        self.b.call("mat_spmm_dense_dev", self.h, 1 if transpose else 0, _dptr(d_x), int(nx), int(k),
                    int(k if ldx is None else ldx), _dptr(d_y), int(ny), int(k if ldy is None else ldy))

    # ---- selected-key product (include/dsa.h: dsa_mat_spmm_selected[_dev]; HIP library only) -------------------------------------
    def matmul_selected(self, keys, X, transpose=False):
        """mat[keys, :] * X / mat[:, keys]' * X (transpose=True): row j of the result is row keys[j] - 1 of matmul(X), bit for bit, at a
        cost that follows the selected rows / columns only.  Keys are 1-based, in any order, repeats allowed; a key that owns no row /
        column gives a zero row.

        A float64 numpy X takes a list or array of keys and returns a new (len(keys), k) array.  A float64 torch tensor on the GPU
        takes a list, an array, or an int64 CUDA tensor (used in place) and returns a new tensor on the same device (nothing leaves
        HBM).  A 1-D X returns the 1-D product.  Inputs that are not row-contiguous are handled as in matmul."""
        self._require("mat_spmm_selected", "the selected-key product needs the HIP product library")
        tr = 1 if transpose else 0
        if isinstance(X, np.ndarray):
            sel, sp = _i64(keys)
            if sel.ndim != 1:
                raise B.DsaArgumentError(B.EARG, "the selection must be one-dimensional")
            nsel, device = len(sel), None
        else:
            device = _dense_tensor_device(X)                     # the keys are judged after the kind of X and before its shape
            sel = _key_tensor(keys, device)
            nsel = sel.numel()
        dev, xp, nx, k, ldx, one_d, device, xx = _dense_operand(X, device)
        y = xx.new_empty((nsel, k)) if dev else np.empty((nsel, k), dtype=np.float64)
        if dev:
            _to_library(device)
            self.matmul_selected_dev(sel.data_ptr(), nsel, xp, nx, k, y.data_ptr(), ldx=ldx, ldy=k, transpose=transpose)
            self.sync()
        else:
            self.b.call("mat_spmm_selected", self.h, tr, sp, nsel, xp, nx, k, ldx, y.ctypes.data_as(P_F64), k)
        return y[:, 0] if one_d else y

    def matmul_selected_dev(self, d_sel, nsel, d_x, nx, k, d_y, ldx=None, ldy=None, transpose=False):
        """the selected-key product with keys (nsel int64) and both operands in HBM (device addresses, e.g. tensor.data_ptr()), X and
        Y row-major with leading dimensions ldx / ldy (default k); stream-ordered on the orientation's stream, no host wait (sync()).
        A key without a row / column (0 and negative keys included) gives a zero row: nothing is reported."""
        self._require("mat_spmm_selected", "the selected-key product needs the HIP product library")
        self.b.call("mat_spmm_selected_dev", self.h, 1 if transpose else 0, _dptr(d_sel), int(nsel), _dptr(d_x),
                    int(nx), int(k), int(k if ldx is None else ldx), _dptr(d_y), int(k if ldy is None else ldy))

    # ---- batched sparse-x product (include/dsa.h: dsa_mat_spgemm_csc[_dev]; HIP library only) ---------------------------------------
    def _require_spgemm(self):
        self._require("mat_spgemm_csc", "the batched sparse-x product needs the HIP product library")

    def matmul_sparse_dev(self, d_xptr, d_xidx, d_xval, k, nnzx, d_yptr, d_yidx, d_yval, cap, index_bits=64, base=0, transpose=False):
        """mat * S / transpose(mat) * S for k sparse columns, S and the result CSC in device memory (device addresses, e.g.
        tensor.data_ptr()): d_xptr = k + 1 indices, d_xidx / d_xval = nnzx entries (indices ascending strictly within a column),
        d_yptr = k + 1 indices, d_yidx / d_yval = cap entries (0 for both with cap = 0: the count-only call).  Column j of the result
        is mul() of column j of S, bit for bit.  Enqueued on the stream of the orientation that is walked (sync()).  Returns
        (total, fits) like select_compressed_dev: with fits False (cap < total) only yptr has been written."""
        self._require_spgemm()
        return self._fits("mat_spgemm_csc_dev", 1 if transpose else 0, int(index_bits), int(base), _dptr(d_xptr),
                          _dptr(d_xidx), _dptr(d_xval), int(k), int(nnzx), _dptr(d_yptr),
                          _dptr(d_yidx), _dptr(d_yval), int(cap))

    def matmul_sparse(self, S, transpose=False, base=0):
        """mat * S / transpose(mat) * S for a sparse S with k columns: column j of the result is mul() of column j of S (the touched
        rows only, ascending, stored zeros kept), bit for bit and the same on every call.

        S = (indptr, indices, data), scipy-style CSC counted from `base` (0 or 1), indices ascending strictly within a column: returns
        the same triple with int64 indices.  A float64 torch.sparse_csc tensor on the GPU with int32 or int64 indices returns a
        torch.sparse_csc_tensor of shape (size(mat, 1 | 2), k) with the same index dtype; nothing leaves HBM."""
        self._require_spgemm()
        tr = 1 if transpose else 0
        m, n = self.size()
        ny = n if transpose else m
        if isinstance(S, (tuple, list)):
            if len(S) != 3:
                raise B.DsaArgumentError(B.EARG, "S must be (indptr, indices, data)")
            xptr, xpp = _i64(S[0])
            xidx, xip = _i64(S[1])
            xval, xvp = _f64(S[2])
            if xptr.ndim != 1 or len(xptr) < 1 or xidx.ndim != 1 or xval.ndim != 1 or len(xidx) != len(xval):
                raise B.DsaArgumentError(B.EARG, "S must be (indptr[k + 1], indices[nnz], data[nnz])")
            k = len(xptr) - 1
            if int(xptr[k]) - int(base) != len(xidx):
                raise B.DsaArgumentError(B.EARG, "indptr[k] - base must be the number of stored entries")
            return self._two_calls("mat_spgemm_csc", (tr, int(base), xpp, xip, xvp, k), k, False)
        import torch
        if not isinstance(S, torch.Tensor) or S.layout != torch.sparse_csc:
            raise B.DsaArgumentError(B.EARG, "S must be a CSC triple or a torch.sparse_csc tensor")
        if S.dtype != torch.float64 or not S.is_cuda or S.dim() != 2:
            raise B.DsaArgumentError(B.EARG, "S must be a 2-D float64 sparse_csc tensor on the GPU")
        xptr, xidx, xval = S.ccol_indices().contiguous(), S.row_indices().contiguous(), S.values().contiguous()
        if xptr.dtype != xidx.dtype or xptr.dtype not in (torch.int32, torch.int64):
            raise B.DsaArgumentError(B.EARG, "the indices of S must be int32 or int64")
        bits = 32 if xptr.dtype == torch.int32 else 64
        k, nnzx = S.shape[1], xidx.numel()
        arrays = self._torch_arrays(S.device, xptr.dtype, k, what="product", call=lambda d_ptr, d_idx, d_vals, cap: (
            self.matmul_sparse_dev(xptr.data_ptr(), xidx.data_ptr(), xval.data_ptr(), k, nnzx, d_ptr, d_idx, d_vals, cap, index_bits=bits,
                                   transpose=transpose)))
        return self._torch_tensor(COLMAJOR, arrays, k, ny)

    # ---- reductions per row / column and in-place scaling (include/dsa.h: dsa_mat_reduce[_dev], dsa_mat_scale[_dev]; HIP library only)
    RED_KINDS = {"sum": 0, "abssum": 1, "sqsum": 2, "absmax": 3, "count": 4}

    def _reduce_args(self, kind, per):
        self._require("mat_reduce", "reduce and scale need the HIP product library")
        if kind not in self.RED_KINDS:
            raise B.DsaArgumentError(B.EARG, "kind must be one of %s" % ", ".join(sorted(self.RED_KINDS)))
        if per not in ("row", "column"):
            raise B.DsaArgumentError(B.EARG, "per must be 'row' or 'column'")
        return self.RED_KINDS[kind], (ROWMAJOR if per == "row" else COLMAJOR)

    def reduce(self, kind, per, out=None):
        """One value per row (per="row") or column (per="column") over the STORED cells: kind "sum", "abssum" (sum of |v|), "sqsum"
        (sum of v * v), "absmax" (max |v|, NaN propagates) or "count" (stored cells, stored zeros included).  Keys without cells give
        0.0.  Returns a numpy array; with out= a float64 tensor on the GPU of the right length the result is written there (it never
        leaves HBM) and out is returned."""
        k, o = self._reduce_args(kind, per)
        self.sync()                                   # size() after the queued single writes
        m, n = self.size()
        cnt = m if o == ROWMAJOR else n
        if out is None:
            y = np.empty(max(cnt, 1), dtype=np.float64)
            self.b.call("mat_reduce", self.h, o, k, y.ctypes.data_as(P_F64), cnt)
            return y[:cnt]
        import torch
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_cuda or out.dim() != 1 or \
                not out.is_contiguous() or out.numel() != cnt:
            raise B.DsaArgumentError(B.EARG, "out must be a contiguous 1-D float64 tensor on the GPU with one element per %s" % per)
        _to_library(out.device)
        self.reduce_dev(kind, per, out.data_ptr(), cnt)
        self.sync()
        return out

    def reduce_dev(self, kind, per, d_out, n):
        """reduce with the result in HBM (device address of n doubles); stream-ordered on the orientation's stream (sync())"""
        k, o = self._reduce_args(kind, per)
        self.b.call("mat_reduce_dev", self.h, o, k, _dptr(d_out), int(n))

    def _norms(self, p, per):
        if p == 1:
            return self.reduce("abssum", per)
        if p == 2:
            return np.sqrt(self.reduce("sqsum", per))
        if p in (np.inf, "inf"):
            return self.reduce("absmax", per)
        raise B.DsaArgumentError(B.EARG, "p must be 1, 2 or inf")

    def row_norms(self, p=2):
        """the p-norm of every row, p in {1, 2, inf} (the 2-norm is sqrt of the "sqsum" reduction, taken here)"""
        return self._norms(p, "row")

    def col_norms(self, p=2):
        return self._norms(p, "column")

    def scale(self, alpha=1.0, rows=None, cols=None):
        """A <- diag(rows) * (alpha * A) * diag(cols) in place: every stored value v becomes ((v * alpha) * rows[i]) * cols[j].
        Structure is preserved: a zero factor leaves stored zeros (nnz unchanged).  rows / cols: numpy arrays (or sequences), or
        float64 tensors on the GPU (any stride; made contiguous first) — both of the same kind; None = factor absent."""
        self._require("mat_reduce", "reduce and scale need the HIP product library")
        dev, (r, nr, c, nc), _keep = _factor_pair(rows, cols)
        if dev:
            self.scale_dev(alpha, r, nr, c, nc)
            self.sync()
        else:
            self.b.call("mat_scale", self.h, float(alpha), r, nr, c, nc)
        return self

    def scale_dev(self, alpha, d_r, nr, d_c, nc):
        """scale with the factors in HBM (device addresses, 0 = factor absent): they are read on both orientations' streams and
        must stay valid and unchanged until sync()"""
        self._require("mat_reduce", "reduce and scale need the HIP product library")
        self.b.call("mat_scale_dev", self.h, float(alpha), _dptr(d_r), int(nr),
                    _dptr(d_c), int(nc))

    # ---- batched delete (include/dsa.h: dsa_mat_delete_batch[_dev]; HIP library only) --------------------------------------------
    def _delete_batch(self, orientation, keys):
        self._require("mat_delete_batch", "the batched delete needs the HIP product library")
        if _is_tensor(keys):
            import torch
            if keys.dtype != torch.int64 or keys.dim() != 1:
                raise B.DsaArgumentError(B.EARG, "a key tensor must be a one-dimensional int64 tensor")
            if keys.is_cuda:
                k = keys.contiguous()
                _to_library(k.device)
                return self.delete_batch_dev(orientation, k.data_ptr(), k.numel())
            keys = keys.numpy()
        k, kp = _i64(np.asarray(keys, dtype=np.int64).reshape(-1))
        got = C.c_int64()
        self.b.call("mat_delete_batch", self.h, int(orientation), kp, len(k), C.byref(got))
        return got.value

    def delete_columns(self, cols):
        """deletecolumn! for every key of cols in one device pass (any order, distinct keys, each a live column).  cols: a sequence, a
        numpy array or an int64 tensor (one on the GPU is used where it is).  Content and tables are those of the single deletes one
        after the other; the survivors of both orientations are spread evenly as by rebalance_root.  Every error leaves the matrix
        untouched.  Returns the number of entries removed.  For one or two keys deletecolumn is the cheaper call."""
        return self._delete_batch(COLMAJOR, cols)

    def delete_rows(self, rows):
        """deleterow! for every key of rows in one device pass (see delete_columns)"""
        return self._delete_batch(ROWMAJOR, rows)

    def delete_batch_dev(self, orientation, d_keys, n):
        """the batched delete with the key list in HBM (device address of n int64 keys, complete at the call): COLMAJOR deletes
        columns, ROWMAJOR rows; returns the number of entries removed"""
        self._require("mat_delete_batch", "the batched delete needs the HIP product library")
        got = C.c_int64()
        self.b.call("mat_delete_batch_dev", self.h, int(orientation), _dptr(d_keys), int(n), C.byref(got))
        return got.value

    # ---- dropzeros! / droptol! (include/dsa.h: dsa_mat_droptol[_dev]; HIP library only) -------------------------------------------
    def _droptol(self, tol, rows, cols, count_only):
        self._require("mat_droptol", "dropzeros and droptol need the HIP product library")
        dev, (r, nr, c, nc), _keep = _factor_pair(rows, cols)
        if dev:
            got = self.droptol_dev(tol, r, nr, c, nc, count_only=count_only)
            self.sync()
            return got
        got = C.c_int64()
        self.b.call("mat_droptol", self.h, float(tol), r, nr, c, nc, 1 if count_only else 0, C.byref(got))
        return got.value

    def droptol(self, tol, rows=None, cols=None):
        """SparseArrays' droptol! in place on the device: the stored cell (i, j) with value v is dropped iff |v| <= tol, or
        |v| <= rows[i - 1], or |v| <= cols[j - 1] (IEEE: a NaN value is never dropped, a NaN or negative threshold matches nothing;
        a negative tol gives purely relative dropping, e.g. A.droptol(-1, rows=eps * A.row_norms(np.inf))).  Content and tables are
        those of A[i, j] = 0 for every dropped cell; an emptied column or row stays as an empty partition; the survivors of both
        orientations are spread evenly as by rebalance_root.  When nothing is dropped nothing changes (cached SpMV plans survive), and
        every error leaves the matrix untouched.  rows / cols: numpy arrays (or sequences), or float64 tensors on the GPU — both of
        the same kind; None = vector absent.  Returns the number of entries dropped."""
        return self._droptol(tol, rows, cols, False)

    def dropzeros(self):
        """SparseArrays' dropzeros!: every stored 0.0 / -0.0 leaves the matrix (droptol(0.0)).  Returns the number dropped."""
        return self._droptol(0.0, None, None, False)

    def count_droptol(self, tol, rows=None, cols=None):
        """the number of entries droptol(tol, rows, cols) would drop; modifies nothing"""
        return self._droptol(tol, rows, cols, True)

    def droptol_dev(self, tol, d_r, nr, d_c, nc, count_only=False):
        """droptol with the threshold vectors in HBM (device addresses, 0 = vector absent): they are read on both orientations'
        streams and must be complete at the call; returns the number of entries dropped (count_only: that would be dropped)"""
        self._require("mat_droptol", "dropzeros and droptol need the HIP product library")
        got = C.c_int64()
        self.b.call("mat_droptol_dev", self.h, float(tol), _dptr(d_r), int(nr),
                    _dptr(d_c), int(nc), 1 if count_only else 0, C.byref(got))
        return got.value

    # ---- update of stored values in place (include/dsa.h: dsa_mat_update_values[_dev], dsa_mat_get_batch_dev; HIP library only) ---
    _UPDATE_NEEDS = "update_values, add_values and get_batch_dev need the HIP product library"

    @staticmethod
    def _update_op(op):
        try:
            return {"set": UPD_SET, "add": UPD_ADD, UPD_SET: UPD_SET, UPD_ADD: UPD_ADD}[op]
        except (KeyError, TypeError):
            raise B.DsaArgumentError(B.EARG, "op must be 'set' or 'add'") from None

    def update_values(self, I, J, V, op="set", missing="error"):
        """A[I[k], J[k]] = V[k] (op "set") or += V[k] ("add") for cells that are ALREADY STORED, in place on the device: no cell is
        created, deleted or moved, so the call does not go through the write planner of set_batch.  "set" keeps the bits of V
        (a 0.0 leaves a stored zero: dropzeros() removes it); a cell addressed more than once ends with the last value; "add"
        must address a cell at most once.  missing="error": a cell that is not stored raises DsaArgumentError and nothing is
        modified; "skip": such ops are skipped and the call returns (updated, missing_mask) — send the masked triples through
        set_batch.  Otherwise returns the number of cells written.  I, J, V: sequences or numpy arrays, or tensors on the GPU
        (int64, int64, float64; all three of the same kind), which are used where they are.  Cached SpMV plans are dropped only
        when a value is written."""
        self._require("mat_update_values", self._UPDATE_NEEDS)
        opc = self._update_op(op)
        if missing not in ("error", "skip"):
            raise B.DsaArgumentError(B.EARG, "missing must be 'error' or 'skip'")
        skip = missing == "skip"
        flags = UPD_SKIP_MISSING if skip else 0
        dev, (i, j, v, n, mp), mask, _keep = _triple(I, J, V, skip)
        if dev:
            updated, _ = self.update_values_dev(i, j, v, n, opc, flags, d_missing=mp)
            self.sync()
            return (updated, mask.bool()) if skip else updated
        upd, mis = C.c_int64(), C.c_int64()
        self.b.call("mat_update_values", self.h, opc, flags, i, j, v, n, mp, C.byref(upd), C.byref(mis))
        return (upd.value, mask.astype(bool)) if skip else upd.value

    def add_values(self, I, J, V, missing="error"):
        """A[I[k], J[k]] += V[k] on stored cells: update_values(I, J, V, op="add")"""
        return self.update_values(I, J, V, op="add", missing=missing)

    def update_values_dev(self, d_I, d_J, d_V, n, op=UPD_SET, flags=0, d_missing=None):
        """update_values with the triples in HBM (device addresses of n int64, int64, float64 entries, complete at the call and
        unchanged until sync()); op UPD_SET | UPD_ADD, flags 0 | UPD_SKIP_MISSING, d_missing: device address of n bytes that receive
        1 for an op without a stored cell, or None.  The host waits for the verdict only: the stores are enqueued on the two
        streams (sync()).  Returns (updated, missing): cells written and ops without a stored cell."""
        self._require("mat_update_values", self._UPDATE_NEEDS)
        upd, mis = C.c_int64(), C.c_int64()
        self.b.call("mat_update_values_dev", self.h, int(op), int(flags), _dptr(d_I),
                    _dptr(d_J), _dptr(d_V), int(n),
                    _dptr(d_missing), C.byref(upd), C.byref(mis))
        return upd.value, mis.value

    def get_batch_dev(self, d_I, d_J, n, d_out, d_found=None):
        """get_batch with everything in HBM: d_out[k] = A[d_I[k], d_J[k]] (0.0 when the cell is not stored), d_found[k] (n bytes,
        optional) = 1 iff it is stored.  Device addresses; enqueued on the colmajor stream, no host wait (sync())."""
        self._require("mat_update_values", self._UPDATE_NEEDS)
        self.b.call("mat_get_batch_dev", self.h, _dptr(d_I), _dptr(d_J), int(n),
                    _dptr(d_out), _dptr(d_found))

    # ---- insert of cells that are not stored yet, in place (include/dsa.h: dsa_mat_insert_batch[_dev]; HIP library only) ---------
    _INSERT_NEEDS = "insert_values and upsert need the HIP product library"

    def insert_values(self, I, J, V, existing="error"):
        """Creates the cells (I[k], J[k]) with the values V[k] in place on the device, in both orientations: the back end of
        update_values(..., missing="skip").  The cells must not be stored yet and must be distinct.  Content, nnz and size() end
        as after set_batch of the same nonzero triples; the LAYOUT is the merged cell sequence spread by the root rebalance (as
        after delete_columns), with the capacity doubled as often as the merged count needs, never shrunk.  V keeps its bits; a 0.0
        creates a stored zero (dropzeros() removes it).  New columns / rows must lie behind the last entry of their table, which
        must be live: one that would land in the middle raises DsaErrorException with code EMODE (use set_batch).  existing="error": a cell that is
        already stored raises DsaArgumentError and nothing is modified; "skip": such ops are skipped and the call returns their
        boolean mask.  I, J, V: sequences or numpy arrays, or tensors on the GPU (int64, int64, float64; all three of the same
        kind), which are used where they are.  An error, an empty batch and a batch that is skipped entirely change nothing and
        keep the cached SpMV plans."""
        self._require("mat_insert_batch", self._INSERT_NEEDS)
        if existing not in ("error", "skip"):
            raise B.DsaArgumentError(B.EARG, "existing must be 'error' or 'skip'")
        skip = existing == "skip"
        flags = INS_SKIP_EXISTING if skip else 0
        dev, (i, j, v, n, mp), mask, _keep = _triple(I, J, V, skip)
        if dev:
            self.insert_values_dev(i, j, v, n, flags, d_existing=mp)
            return mask.bool() if skip else None
        self.b.call("mat_insert_batch", self.h, i, j, v, n, flags, mp)
        return mask.astype(bool) if skip else None

    def insert_values_dev(self, d_I, d_J, d_V, n, flags=0, d_existing=None):
        """insert_values with the triples in HBM (device addresses of n int64, int64, float64 entries, complete at the call); flags
        0 | INS_SKIP_EXISTING, d_existing: device address of n bytes that receive 1 for an op whose cell is already stored, or
        None.  Returns with both streams drained."""
        self._require("mat_insert_batch", self._INSERT_NEEDS)
        self.b.call("mat_insert_batch_dev", self.h, _dptr(d_I), _dptr(d_J),
                    _dptr(d_V), int(n), int(flags), _dptr(d_existing))

    def upsert(self, I, J, V):
        """A[I[k], J[k]] = V[k] whether the cell is stored or not, for DISTINCT cells and host arrays: update_values(...,
        missing="skip"), then insert_values of the ops it reports missing — the general write for nonzero values composed of its
        two halves (a 0.0 leaves or creates a stored zero).  Returns (updated, inserted)."""
        self._require("mat_insert_batch", self._INSERT_NEEDS)
        i, j, v = _host_triple(I, J, V)
        updated, miss = self.update_values(i, j, v, missing="skip")
        if miss.any():
            self.insert_values(i[miss], j[miss], v[miss])
        return updated, int(miss.sum())

    # ---- the general write from triples, in place (include/dsa.h: dsa_mat_assemble[_dev]; HIP library only) -------------------------
    _ASSEMBLE_NEEDS = "assemble needs the HIP product library"

    def assemble(self, I, J, V, op="add"):
        """A[I[k], J[k]] += V[k] (op "add") or = V[k] ("set") for ANY triples — cells stored or not, repeated or not, in any order —
        in place on the device.  The ops are folded to distinct cells first: "add" sums a cell's values one after the other in the
        order of the batch (the left fold of dynamicsparse over duplicates), "set" keeps the last, bit for bit.  Stored cells are
        then written as by update_values ("add": stored + sum), the others created as by insert_values, with its layout and its
        limit: a new column / row must lie behind the last live entry of its table, else DsaErrorException with code EMODE (use
        set_batch).  A zero, or a sum that cancels, is a stored zero (dropzeros() removes it).  "add" is A + sparse(I, J, V) in
        place.  I, J, V: sequences or numpy arrays, or tensors on the GPU (int64, int64, float64; all three of the same kind), which
        are used where they are.  An error and an empty batch change nothing and keep the cached SpMV plans.  Returns (distinct,
        updated, inserted): the distinct cells, those written in place, those created."""
        self._require("mat_assemble", self._ASSEMBLE_NEEDS)
        opc = self._update_op(op)
        dev, (i, j, v, n, _), _mask, _keep = _triple(I, J, V, False)
        if dev:
            out = self.assemble_dev(i, j, v, n, opc)
            self.sync()
            return out
        d, u, ins = C.c_int64(), C.c_int64(), C.c_int64()
        self.b.call("mat_assemble", self.h, opc, i, j, v, n, C.byref(d), C.byref(u), C.byref(ins))
        return d.value, u.value, ins.value

    def assemble_dev(self, d_I, d_J, d_V, n, op=UPD_ADD):
        """assemble with the triples in HBM (device addresses of n int64, int64, float64 entries, complete at the call and unchanged
        until it returns); op UPD_SET | UPD_ADD.  When only stored cells are written the stores may still be enqueued (sync());
        when cells are created the call returns with both streams drained.  Returns (distinct, updated, inserted)."""
        self._require("mat_assemble", self._ASSEMBLE_NEEDS)
        d, u, ins = C.c_int64(), C.c_int64(), C.c_int64()
        self.b.call("mat_assemble_dev", self.h, int(op), _dptr(d_I), _dptr(d_J), _dptr(d_V), int(n),
                    C.byref(d), C.byref(u), C.byref(ins))
        return d.value, u.value, ins.value


def dynamicsparse(I=None, J=None, V=None, m=None, n=None, fill_mode=True,
                  binding: Binding | None = None) -> DynamicSparseMatrix:
    """dynamicsparse(I, J, V, [m, n])  src/matrix.jl:15-19  /  dynamicsparse(Ti,Tj,Tv; fill_mode)  :31-41."""
    b = _bind(binding)
    h = VP()
    if I is None:
        b.call("mat_create_empty", 1 if fill_mode else 0, C.byref(h))
        return DynamicSparseMatrix(b, h)
    if not (len(I) == len(J) == len(V)):
        raise B.DsaArgumentError(B.EARG, "rows, columns, and nonzeros do not have same length.")
    i, ip = _i64(I)
    j, jp = _i64(J)
    v, vp = _f64(V)
    b.call("mat_create_from_coo", ip, jp, vp, len(i), -1 if m is None else int(m), -1 if n is None else int(n),
           C.byref(h))
    return DynamicSparseMatrix(b, h)


# ---- import from device memory (include/dsa.h: dsa_mat_create_from_coo_dev / _compressed_dev; HIP library only) ------------------
def _require_import(b):
    if not b.has("mat_create_from_coo_dev"):
        raise B.DsaArgumentError(B.EARG, "the device import needs the HIP product library")


def dynamicsparse_dev(d_I, d_J, d_V, nnz, m=None, n=None, index_bits=64, index_base=1,
                      binding: Binding | None = None) -> DynamicSparseMatrix:
    """dynamicsparse(I, J, V, [m, n]) with the triples in HBM (device addresses, e.g. tensor.data_ptr()): indices of `index_bits`
    counted from `index_base`, float64 values.  The arrays must be complete at the call and are the caller's again when it returns."""
    b = _bind(binding)
    _require_import(b)
    h = VP()
    b.call("mat_create_from_coo_dev", _dptr(d_I), _dptr(d_J), _dptr(d_V), int(nnz), int(index_bits),
           int(index_base), -1 if m is None else int(m), -1 if n is None else int(n), C.byref(h))
    return DynamicSparseMatrix(b, h)


def dynamicsparse_compressed_dev(orientation, d_ptr, d_idx, d_vals, outer, inner, nnz, index_bits=64, index_base=0,
                                 binding: Binding | None = None) -> DynamicSparseMatrix:
    """the matrix of a CSR (orientation ROWMAJOR, outer = rows) or CSC (COLMAJOR, outer = columns) form in HBM: the conventions of
    to_compressed_dev, so an export can be fed straight back; size = (outer, inner) for CSR, (inner, outer) for CSC"""
    b = _bind(binding)
    _require_import(b)
    h = VP()
    b.call("mat_create_from_compressed_dev", int(orientation), int(index_bits), int(index_base), _dptr(d_ptr),
           _dptr(d_idx), _dptr(d_vals), int(outer), int(inner), int(nnz), C.byref(h))
    return DynamicSparseMatrix(b, h)


def from_torch(t, binding: Binding | None = None) -> DynamicSparseMatrix:
    """DynamicSparseMatrix of a 2-d torch.sparse_coo (coalesced or not: duplicates are summed), torch.sparse_csr or torch.sparse_csc
    tensor on the GPU, int32 or int64 indices; size = t.shape.  The arrays never leave HBM."""
    import torch
    b = _bind(binding)
    _require_import(b)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise B.DsaArgumentError(B.EARG, "from_torch needs a sparse tensor on the GPU")
    if t.layout not in (torch.sparse_coo, torch.sparse_csr, torch.sparse_csc):
        raise B.DsaArgumentError(B.EARG, "layout must be torch.sparse_coo, torch.sparse_csr or torch.sparse_csc")
    if t.layout == torch.sparse_coo:
        unsupported = t.sparse_dim() != 2 or t.dense_dim() != 0
    else:
        unsupported = t.dim() != 2 or t.values().dim() != 1
    if unsupported:
        raise B.DsaArgumentError(B.EARG, "batched and hybrid sparse tensors are not supported")
    m, n = (int(s) for s in t.shape)
    if t.layout == torch.sparse_coo:
        ind = t._indices()
        val = t._values()
        ptr, idx = ind[0].contiguous(), ind[1].contiguous()          # (row indices, column indices)
    elif t.layout == torch.sparse_csr:
        ptr, idx, val = t.crow_indices().contiguous(), t.col_indices().contiguous(), t.values()
    else:
        ptr, idx, val = t.ccol_indices().contiguous(), t.row_indices().contiguous(), t.values()
    if ptr.dtype not in (torch.int32, torch.int64) or idx.dtype != ptr.dtype:
        raise B.DsaArgumentError(B.EARG, "indices must be int32 or int64")
    val = val.to(torch.float64).contiguous()
    bits = 32 if ptr.dtype == torch.int32 else 64
    nnz = int(val.numel())
    _to_library(t.device)
    if t.layout == torch.sparse_coo:
        return dynamicsparse_dev(ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz, m, n, index_bits=bits, index_base=0, binding=b)
    if t.layout == torch.sparse_csr:
        return dynamicsparse_compressed_dev(ROWMAJOR, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), m, n, nnz, index_bits=bits,
                                            index_base=0, binding=b)
    return dynamicsparse_compressed_dev(COLMAJOR, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), n, m, nnz, index_bits=bits,
                                        index_base=0, binding=b)


# ---- concatenation (dsa_mat_combine with an offset; HIP library only) ---------------------------------------------------------------
def _arg_error(msg):
    return B.DsaArgumentError(B.EARG, msg)


def _concat_operands(lhs, rhs):
    for x in (lhs, rhs):
        if not isinstance(x, DynamicSparseMatrix):
            raise _arg_error("both operands must be DynamicSparseMatrix")
    lhs._require("mat_combine", "combining matrices needs the HIP product library")
    return lhs.size(), rhs.size()


def hcat(A, B):
    """[A B]: the columns of B appended behind those of A (col_off = A.n); both need the same number of rows"""
    (ma, na), (mb, _) = _concat_operands(A, B)
    if ma != mb:
        raise _arg_error(f"hcat: the operands have {ma} and {mb} rows")
    return A.combine(B, col_off=na)


def vcat(A, B):
    """[A; B]: the rows of B appended below those of A (row_off = A.m); both need the same number of columns"""
    (ma, na), (_, nb) = _concat_operands(A, B)
    if na != nb:
        raise _arg_error(f"vcat: the operands have {na} and {nb} columns")
    return A.combine(B, row_off=ma)


def blockdiag(A, B):
    """[A 0; 0 B]"""
    (ma, na), _ = _concat_operands(A, B)
    return A.combine(B, row_off=ma, col_off=na)


# free-function spellings of the exported names (src/DynamicSparseArrays.jl:5-16)
def deletecolumn(mat, col):
    mat.deletecolumn(col)
    return True


def deleterow(mat, row):
    mat.deleterow(row)
    return True


def deletecolumns(mat, cols):
    return mat.delete_columns(cols)


def deleterows(mat, rows):
    return mat.delete_rows(rows)


def insert_values(mat, I, J, V, existing="error"):
    """insert_values!(A, I, J, V): cells that are not stored yet created in place (DynamicSparseMatrix.insert_values)"""
    return mat.insert_values(I, J, V, existing=existing)


def upsert(mat, I, J, V):
    return mat.upsert(I, J, V)


def assemble(mat, I, J, V, op="add"):
    """assemble!(A, I, J, V; op): any triples folded, stored cells written, the others created (DynamicSparseMatrix.assemble)"""
    return mat.assemble(I, J, V, op=op)


def droptol(mat, tol, rows=None, cols=None):
    """droptol!(A, tol; rows, cols): returns the matrix, like SparseArrays"""
    mat.droptol(tol, rows=rows, cols=cols)
    return mat


def dropzeros(mat):
    mat.dropzeros()
    return mat


def addrow(mat, row, colids, vals):
    mat.addrow(row, colids, vals)
    return True


def closefillmode(mat):
    mat.closefillmode()
    return True


def shrink_size(vec):
    vec.shrink_size()


def nbpartitions(obj, orientation=None):
    return obj.nbpartitions() if orientation is None else obj.nbpartitions(orientation)


def deletepartition(pcsc, partition):
    pcsc.deletepartition(partition)


def nnz(obj):
    return obj.nnz()


def pool_idle_bytes(binding: Binding | None = None) -> int:
    """idle HBM the library's caching allocator holds for reuse (dsa_pool_idle_bytes)"""
    out = C.c_int64()
    _bind(binding).call("pool_idle_bytes", C.byref(out))
    return out.value


def pool_trim(keep_bytes=0, binding: Binding | None = None):
    """release idle HBM blocks until at most keep_bytes remain (dsa_pool_trim)"""
    _bind(binding).call("pool_trim", int(keep_bytes))


def dev_switches(binding: Binding | None = None):
    """(names, enabled): the library's table of development switches and whether this process honours them
    (only with DSA_DEV=1 in the environment: a release process ignores them — dsa_dev_switches)"""
    buf = C.create_string_buffer(2048)
    on = C.c_int32()
    _bind(binding).call("dev_switches", buf, 2048, C.byref(on))
    return buf.value.decode().split(), bool(on.value)
