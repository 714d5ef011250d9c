"""The numpy and the torch form of matmul, matmul_selected and matmul_sparse on one tiny matrix, at the operand shapes the larger suites
(test_spmm.py, test_selected_product.py, test_spgemm.py) do not reach: a transposed view, a single row, an empty key list, an
empty product.  What is pinned is the way an operand reaches the library — view or copy, leading dimension, key upload, count then
emit, the 1-D tail — through the documented identities, bit for bit.  Every value is a small dyadic rational, so every product and
every sum is exact in float64 and the bits cannot depend on the order or the fusing of the adds, which is the kernels' business."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N = 5, 4
# six cells; row 5 and column 2 are empty
CELLS = [(1, 1, 1.5), (1, 3, -2.0), (2, 3, 0.25), (3, 1, 3.0), (3, 4, -0.75), (4, 4, 2.5)]
BASE = (np.arange(24.0).reshape(4, 6) - 7.0) / 8.0
# name -> (the view of the 4 x 6 base, whether the tensor is used in place, the leading dimension that reaches the library)
VIEWS = {
    "row-strided": (lambda b: b[:, :3], True, 6),          # stride (6, 1): in place
    "transposed": (lambda b: b.T, False, 4),               # 6 x 4 with stride(1) != 1: copied
    "one row": (lambda b: b[:1, :3], True, 3),             # a single row has no row stride to honour: ldx = k
    "1-D": (lambda b: b[:, 0], True, 6),                   # n x 1 over the first column
}
KEYS = ([2, 2, 5, 1], [])                                  # a repeat and the empty row; nothing


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def case(dsa, hip):
    """(the matrix, the base as a CUDA tensor, {view name: matmul of its numpy form}): built once, only read"""
    import torch
    I, J, V = (np.array(x) for x in zip(*CELLS))
    a = dsa.dynamicsparse(I.astype(np.int64), J.astype(np.int64), V.astype(np.float64), M, N, binding=hip)
    assert a.size() == (M, N) and a.nnz() == len(CELLS)
    full = {name: a.matmul(view(BASE)) for name, (view, _, _) in VIEWS.items()}
    return a, torch.from_numpy(BASE).to("cuda"), full


@pytest.mark.parametrize("name", VIEWS)
def test_matmul_columns_and_forms(dsa, case, name):
    from dsa_amd import api
    a, base_d, full = case
    view, in_place, ldx = VIEWS[name]
    X, Xd, Y = view(BASE), view(base_d), full[name]
    assert isinstance(Y, np.ndarray) and Y.shape == ((M,) if X.ndim == 1 else (M, X.shape[1]))
    X2, Y2 = X.reshape(len(X), -1), Y.reshape(M, -1)
    if len(X) >= N:
        for j in range(X2.shape[1]):                                     # column j of matmul(X) is mul(X[:, j])
            assert same_bits(Y2[:, j], a.mul(X2[:, j].copy())), (name, j)
    else:                                                                # cells beyond the rows of X contribute nothing
        assert same_bits(Y, a.matmul(np.vstack([X, np.zeros((N - len(X), X.shape[1]))])))
    dev, addr, nx, k, ld, one_d, device, keep = api._dense_operand(Xd)
    assert dev is True and device == base_d.device and (nx, k, one_d) == (X2.shape[0], X2.shape[1], X.ndim == 1)
    assert (addr == base_d.data_ptr()) == in_place and ld == ldx
    Yd = a.matmul(Xd)
    assert Yd.is_cuda and Yd.device == base_d.device
    assert same_bits(Yd.cpu().numpy(), Y)                                # the torch form is the numpy form


@pytest.mark.parametrize("name", VIEWS)
def test_matmul_selected_rows_and_forms(dsa, case, name):
    import torch
    a, base_d, full = case
    view = VIEWS[name][0]
    X, Xd, Y = view(BASE), view(base_d), full[name]
    for keys in KEYS:
        exp = Y[np.array(keys, dtype=np.int64) - 1]                      # row j is row keys[j] - 1 of matmul(X)
        assert exp.shape == ((len(keys),) if X.ndim == 1 else (len(keys), X.shape[1]))
        for k in (keys, np.array(keys, dtype=np.int64)):
            got = a.matmul_selected(k, X)
            assert isinstance(got, np.ndarray) and same_bits(got, exp), (name, keys)
        for k in (keys, torch.tensor(keys, dtype=torch.int64, device="cuda")):
            got = a.matmul_selected(k, Xd)
            assert got.is_cuda and got.device == base_d.device and same_bits(got.cpu().numpy(), exp), (name, keys)


# S has k = 2 columns over the 4 columns of the matrix; (indptr, indices, data) counted from 0
SPARSE = {
    "one empty column": ([0, 2, 2], [0, 3], [2.0, -0.5]),
    "empty product": ([0, 1, 1], [1], [4.0]),              # only the matrix's empty column 2 is addressed: nothing is touched
}


@pytest.mark.parametrize("name", SPARSE)
def test_matmul_sparse_columns_and_forms(dsa, case, name):
    import torch
    a = case[0]
    xptr, xidx, xval = (np.array(x, dtype=dt) for x, dt in zip(SPARSE[name], (np.int64, np.int64, np.float64)))
    k = len(xptr) - 1
    yptr, yidx, yval = a.matmul_sparse((xptr, xidx, xval))
    assert (yptr.dtype, yidx.dtype, yval.dtype) == (np.int64, np.int64, np.float64) and yptr.shape == (k + 1,)
    assert yptr[0] == 0 and yptr[k] == len(yidx) == len(yval)
    for j in range(k):                                                   # column j is mul of column j of S
        lo, hi = xptr[j], xptr[j + 1]
        ei, ev = a.mul((xidx[lo:hi] + 1, xval[lo:hi])) if hi > lo else (np.zeros(0, dtype=np.int64), np.zeros(0))
        assert np.array_equal(yidx[yptr[j]:yptr[j + 1]], ei - 1) and same_bits(yval[yptr[j]:yptr[j + 1]], ev), (name, j)
    assert (len(yidx) == 0) == (name == "empty product")
    bptr, bidx, bval = a.matmul_sparse((xptr + 1, xidx + 1, xval), base=1)
    assert np.array_equal(bptr, yptr + 1) and np.array_equal(bidx, yidx + 1) and same_bits(bval, yval)
    for dt in (torch.int32, torch.int64):                                # the torch form is the numpy form, in S's index dtype
        S = torch.sparse_csc_tensor(torch.tensor(xptr, dtype=dt, device="cuda"), torch.tensor(xidx, dtype=dt, device="cuda"),
                                    torch.tensor(xval, dtype=torch.float64, device="cuda"), size=(N, k))
        Y = a.matmul_sparse(S)
        assert Y.layout == torch.sparse_csc and tuple(Y.shape) == (M, k) and Y.is_cuda
        assert Y.ccol_indices().dtype == dt and Y.row_indices().dtype == dt
        assert np.array_equal(Y.ccol_indices().cpu().numpy(), yptr) and np.array_equal(Y.row_indices().cpu().numpy(), yidx)
        assert same_bits(Y.values().cpu().numpy(), yval)
