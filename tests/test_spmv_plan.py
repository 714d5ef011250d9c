"""The column-swept SpMV plan (csrc/spmv.hip: k_spmv_plan).

A dense product over the gather orientation whose x does not fit an XCD's L2 builds the plan on the second product at one content
epoch and computes from it from the third one on.  Every test checks stat_spmv_plan > 0, so that none of them can pass on
k_spmv_gather alone.  y from the plan is compared byte for byte with y from k_spmv_gather (the first product of the same handle:
same left-to-right sums), and with the CPU oracle.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

RTOL = 1e-12
M = N = 420_000          # 8 * N bytes of x > 3 MB: the non-temporal regime, where the plan applies
NNZ = 1_260_000

pytestmark = pytest.mark.gpu


def _triplets(seed, m=M, n=N, nnz=NNZ):
    rng = np.random.default_rng(seed)
    return rng.integers(1, m + 1, nnz), rng.integers(1, n + 1, nnz), rng.integers(1, 1 << 20, nnz) * 2.0 ** -17


def _x(seed, n=N):
    return 1.0 + np.random.default_rng(seed).random(n)


def _stats(a):
    i = a.info(1)        # ROWMAJOR: the orientation mat * v gathers over
    return i["stat_spmv_plan"], i["stat_spmv_plan_builds"], i["hbm_bytes"]


def _three_products(a, x, **kw):
    """product, product (the plan is built behind it), product (from the plan)."""
    ys = [a.mul(x, **kw).copy() for _ in range(3)]
    assert ys[0].tobytes() == ys[1].tobytes()
    return ys


def test_plan_bit_identical_to_gather_and_matches_oracle(dsa, hip, oracle):
    I, J, V = _triplets(1)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    x = _x(2)
    p0, b0, _ = _stats(a)
    y1, _, y3 = _three_products(a, x)
    p1, b1, _ = _stats(a)
    assert b1 == b0 + 1 and p1 == p0 + 1, (p0, b0, p1, b1)
    assert y3.tobytes() == y1.tobytes()
    np.testing.assert_allclose(y3, b.mul(x), rtol=RTOL, atol=0)
    y4 = a.mul(x)
    assert _stats(a)[0] == p1 + 1 and y4.tobytes() == y1.tobytes()


def _writes():
    rng = np.random.default_rng(7)
    I, J, V = _triplets(3)
    k = rng.integers(0, NNZ, 50)
    In, Jn = rng.integers(1, M + 1, 2000), rng.integers(1, N + 1, 2000)
    return [
        ("set_overwrite", lambda m: m.__setitem__((int(I[k[0]]), int(J[k[0]])), 3.25)),       # value-only: no slot moves
        ("set_batch_overwrite", lambda m: m.set_batch(I[k], J[k], np.full(len(k), -0.5))),
        ("set_batch_new", lambda m: m.set_batch(In, Jn, np.full(2000, 1.5))),
        ("addrow", lambda m: m.addrow(M - 7, np.array([11, 4_000, 399_999]), np.array([2.0, 3.0, 4.0]))),
        ("rebalance_root", lambda m: m.rebalance_root(1)),
        ("deletecolumn", lambda m: m.deletecolumn(int(J[k[1]]))),
        ("deleterow", lambda m: m.deleterow(int(I[k[2]]))),      # last: a deleted row leaves a tombstone, and the plan needs none
    ]


def test_plan_dropped_by_every_write(dsa, hip, oracle):
    I, J, V = _triplets(3)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    x = _x(4)
    _three_products(a, x)
    assert _stats(a)[0] == 1
    for name, w in _writes():
        p0, b0, _ = _stats(a)
        w(a)
        w(b)
        yo = b.mul(x)
        y1 = a.mul(x)             # the first product after the write: never the stale plan
        assert _stats(a)[0] == p0, name
        np.testing.assert_allclose(y1, yo, rtol=RTOL, atol=0, err_msg=name)
        a.mul(x)                  # the second one builds the plan again ...
        y3 = a.mul(x)             # ... and the third one uses it
        p1, b1, _ = _stats(a)
        if name != "deleterow":   # (a deleted row leaves a tombstone in the row table: no plan then)
            assert b1 == b0 + 1 and p1 == p0 + 1, (name, p0, b0, p1, b1)
        assert y3.tobytes() == y1.tobytes(), name
        np.testing.assert_allclose(y3, yo, rtol=RTOL, atol=0, err_msg=name)


def test_plan_after_closefillmode(dsa, hip, oracle):
    I, J, V = _triplets(5)
    a = dsa.dynamicsparse(binding=hip)
    b = dsa.dynamicsparse(binding=oracle)
    for m in (a, b):
        m.set_batch(I, J, V)
        m.closefillmode()
    x = _x(6)
    y1, _, y3 = _three_products(a, x)
    assert _stats(a)[0] >= 1
    assert y3.tobytes() == y1.tobytes()
    np.testing.assert_allclose(y3, b.mul(x), rtol=RTOL, atol=0)


def test_plan_follows_nx_ny(dsa, hip, oracle):
    I, J, V = _triplets(8)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    x = _x(9)
    yref = b.mul(x)
    _, _, y3 = _three_products(a, x)
    np.testing.assert_allclose(y3, yref, rtol=RTOL, atol=0)
    p0, b0, _ = _stats(a)
    # a longer x (nx changes) and a longer y (ny changes: the rows behind the last one are zeroed by the plan)
    x2 = np.concatenate([x, _x(10, 5000)])
    _, _, y3b = _three_products(a, x2)
    np.testing.assert_allclose(y3b, yref, rtol=RTOL, atol=0)
    _, _, y3c = _three_products(a, x, dense_out=M + 3000)
    assert np.all(y3c[M:] == 0.0)
    np.testing.assert_allclose(y3c[:M], yref, rtol=RTOL, atol=0)
    p1, b1, _ = _stats(a)
    assert b1 == b0 + 2 and p1 == p0 + 2, (p0, b0, p1, b1)


def test_plan_memory_returned(dsa, hip):
    I, J, V = _triplets(11)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    x = _x(12)
    a.mul(x)
    _, _, h0 = _stats(a)
    _three_products(a, x)
    p, _, h1 = _stats(a)
    assert p >= 1
    cells = a.nnz()
    assert h1 - h0 >= 12 * cells, (h0, h1, cells)          # 12 B per stored cell (+ the offset table)
    a[1, 1] = 2.0                                          # invalidation returns it
    _, _, h2 = _stats(a)
    assert h1 - h2 >= 12 * cells, (h1, h2)
    _three_products(a, x)
    _, _, h3 = _stats(a)
    assert h3 - h2 >= 12 * cells, (h2, h3)
    idle = C.c_int64()
    hip.call("pool_idle_bytes", C.byref(idle))
    idle0 = idle.value
    a.close()
    hip.call("pool_idle_bytes", C.byref(idle))
    assert idle.value >= idle0 + 12 * cells                # the plan's blocks are back in the pool after destroy


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import dsa_loader, test_spmv_plan as t
dsa = dsa_loader.load(); hip = dsa.product()
I, J, V = t._triplets(1)
a = dsa.dynamicsparse(I, J, V, binding=hip)
ys = [a.mul(t._x(2)) for _ in range(3)]
assert a.info(1)["stat_spmv_plan"] == 0 and a.info(1)["stat_spmv_plan_builds"] == 0
np.save(sys.argv[3], ys[2])
"""


def test_dev_switch_off_gives_the_same_y(dsa, hip, tmp_path):
    """DSA_SPMV_PLAN=0 (development switch): no plan is built or used, and y is the plan's, byte for byte."""
    I, J, V = _triplets(1)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    _, _, y3 = _three_products(a, _x(2))
    assert _stats(a)[0] >= 1
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "y_off.npy")
    env = dict(os.environ, DSA_DEV="1", DSA_SPMV_PLAN="0")
    subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(here), here, out], env=env, check=True, timeout=600)
    assert np.load(out).tobytes() == y3.tobytes()
