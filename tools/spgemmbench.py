#!/usr/bin/env python3
"""The batched sparse-x product against k single sparse-x products, on the config-3 matrix (1 M x 1 M, 10 M nnz, built as bench.py
builds it).

For k in {1, 8, 64, 512} columns of S with 10, 100 and 10 000 stored entries each (random column keys, standard-normal values),
operands in HBM and every buffer sized beforehand, in one process:
  (batched) one dsa_mat_spgemm_csc_dev (count and emit in one call: cap = the total a count-only call reported);
  (single)  k calls of dsa_mat_spmv_sparse_dev (mul_dev), one per column of S, on the same columns.
Each form is timed on the host clock from the call to the end of dsa_mat_sync (the batched call waits for its hand-overs itself), after
one warm-up of both, three times, the two forms alternating; the JSON holds the three times, their median and
ratio = median(single) / median(batched): above 1 the batched call is the faster one.  `long_columns` says how many columns of S visit
more than SPG_SMALL_MAX cells (the slab path); the others are summed in LDS.  The touched rows of the first column are asserted to be
those of the single product (the values differ in the last bits by design: the single product adds with fp64 atomics).

  python tools/spgemmbench.py [--out profiles/spgemm_c3.json] [--ks 1 8 64 512] [--entries 10 100 10000]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = N = 1_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 8, 64, 512])
    ap.add_argument("--entries", type=int, nargs="*", default=[10, 100, 10000])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm_c3.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import dsa_loader
    dsa = dsa_loader.load()
    hip = dsa.product()
    with open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "spgemm.h")) as fh:
        small_max = int(re.search(r"SPG_SMALL_MAX\s*=\s*(\d+)", fh.read()).group(1))
    I, J, V = bench.c3_triplets(M, N, 10, 0, seed_rows=5, seed_vals=6)
    A = dsa.dynamicsparse(I, J, V, M, N, binding=hip)
    per_col = np.bincount(np.asarray(J, dtype=np.int64), minlength=N + 1)
    rng = np.random.default_rng(23)
    d_yi = torch.empty(M, dtype=torch.int64, device="cuda")
    d_yv = torch.empty(M, dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    res = dict(shape="config 3: %d x %d, %d nnz" % (M, N, len(I)), runs=a.runs, warmup=1, small_max=small_max,
               timing="host clock from the call to the end of dsa_mat_sync, the two forms alternating; batched = one "
                      "dsa_mat_spgemm_csc_dev (cap = the counted total), single = k calls of dsa_mat_spmv_sparse_dev on the same columns; "
                      "ratio = median(single) / median(batched)", points=[])
    for per in a.entries:
        for k in a.ks:
            cols = [np.sort(rng.choice(N, per, replace=False)).astype(np.int64) for _ in range(k)]
            xptr = np.arange(k + 1, dtype=np.int64) * per
            xidx = np.concatenate(cols)
            xval = rng.standard_normal(k * per)
            long_columns = int(sum(int(per_col[c + 1].sum()) > small_max for c in cols))
            t_xptr, t_xidx, t_xval = (torch.from_numpy(x).to("cuda") for x in (xptr, xidx, xval))
            t_keys = t_xidx + 1                                        # mul_dev takes 1-based keys
            yptr = torch.empty(k + 1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            args = (t_xptr.data_ptr(), t_xidx.data_ptr(), t_xval.data_ptr(), k, k * per, yptr.data_ptr())
            total, _ = A.matmul_sparse_dev(*args, 0, 0, 0)
            yidx = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
            yval = torch.empty(max(total, 1), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()

            def batched():
                t0 = time.perf_counter()
                got, fits = A.matmul_sparse_dev(*args, yidx.data_ptr(), yval.data_ptr(), total)
                A.sync()
                assert fits and got == total
                return (time.perf_counter() - t0) * 1e6

            def single():
                t0 = time.perf_counter()
                for j in range(k):
                    A.mul_dev(t_keys.data_ptr() + 8 * j * per, t_xval.data_ptr() + 8 * j * per, per, d_yi.data_ptr(), d_yv.data_ptr(), M,
                              d_cnt.data_ptr())
                A.sync()
                return (time.perf_counter() - t0) * 1e6

            batched(); single()
            # the last single product is column k - 1: its touched rows are those of the batched result
            n_last = int(d_cnt.item())
            p = yptr[-2:].cpu().numpy()
            assert n_last == p[1] - p[0] and torch.equal(d_yi[:n_last] - 1, yidx[p[0]:p[1]]), (k, per)
            tb, ts = [], []
            for _ in range(a.runs):
                tb.append(batched())
                ts.append(single())
            point = dict(k=k, entries_per_column=per, nnzx=k * per, total=int(total), long_columns=long_columns, batched_us=tb, single_us=ts,
                         batched_us_median=statistics.median(tb), single_us_median=statistics.median(ts),
                         ratio=statistics.median(ts) / statistics.median(tb))
            res["points"].append(point)
            print(json.dumps(point), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
