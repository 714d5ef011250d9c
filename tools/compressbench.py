#!/usr/bin/env python3
"""Compressed export of the C3 matrix (1M x 1M, 10M nnz, 2^24-slot orientations): CSR and CSC, int32 and int64 indices, HIP events on
the orientation's stream, median of 20; dsa_mat_rebalance_root of the same orientation in the same process as the comparator.  Prints
one JSON line.  Physical bytes of an export: (kb + 8) * capacity + capacity / 8 + 17 * table_len + (ib + 8) * nnz + ib * (dim + 1).
Usage: python tools/compressbench.py [reps]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import dsa_loader  # noqa: E402

PEAK = 8e12
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dsa = dsa_loader.load()
hip = dsa.product()
m = n = 1_000_000
I, J, V = bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6)
a = dsa.dynamicsparse(I, J, V, binding=hip)
stream = torch.cuda.current_stream()
hip.call("mat_set_stream", a.h, C.c_void_p(stream.cuda_stream))
nnz = a.nnz()


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


out = dict(workload="C3 compressed export (1M x 1M, %d nnz)" % nnz, reps=reps, peak_bytes_per_s=PEAK, exports={}, rebalance_root={})
for o, name in ((1, "csr"), (0, "csc")):
    inf = a.info(o)
    cap, tl = inf["capacity"], inf["table_len"]
    kb = 4                                                     # C3 keys fit 32 bits
    for ib in (4, 8):
        dt = torch.int32 if ib == 4 else torch.int64
        ptr = torch.empty(m + 1, dtype=dt, device="cuda")
        idx = torch.empty(nnz, dtype=dt, device="cuda")
        val = torch.empty(nnz, dtype=torch.float64, device="cuda")
        us = timed(lambda: a.to_compressed_dev(o, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz, index_bits=8 * ib))
        phys = (kb + 8) * cap + cap // 8 + 17 * tl + (ib + 8) * nnz + ib * (m + 1)
        out["exports"]["%s_int%d" % (name, 8 * ib)] = dict(us=round(us, 2), physical_bytes=phys, frac_peak=round(phys / (us * 1e-6) / PEAK, 4))
    us = timed(lambda: a.rebalance_root(o))
    phys = 2 * (kb + 8) * cap + cap // 4
    out["rebalance_root"][name] = dict(us=round(us, 2), physical_bytes=phys, frac_peak=round(phys / (us * 1e-6) / PEAK, 4))
for k, e in out["exports"].items():
    e["no_slower_than_rebalance_root"] = e["us"] <= out["rebalance_root"][k.split("_")[0]]["us"]
print(json.dumps(out))
