#!/usr/bin/env python3
"""The batched delete against the per-key loop on the config-3 matrix (1 M x 1 M, 10 M nnz, 2^24 slots, built as bench.py builds it).

Two identically built matrices in one process: on A every list goes through dsa_mat_delete_batch_dev (the keys already in HBM), on
B the same keys go through k calls of dsa_mat_deletecolumn / dsa_mat_deleterow.  A delete cannot be repeated on the same keys, so
every run takes the next k keys of one random permutation of the live columns (rows); both matrices see the same lists in the same
order and stay in step (about 19 000 of 10^6 columns and as many rows are gone at the end).  Per k = 1, 8, 64, 512, 4096: one
warm-up run, then the median of three, host wall time around the blocking call(s) with both streams drained before and after.
The crossover is the smallest k from which the batched call is the faster one at every measured k.

  python tools/deletebench.py [--out profiles/delete_c3.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = N = 1_000_000
KS = (1, 8, 64, 512, 4096)
RUNS, WARMUP = 3, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delete_c3.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import dsa_loader
    dsa = dsa_loader.load()
    hip = dsa.product()

    I, J, V = bench.c3_triplets(M, N, 10, 0, seed_rows=5, seed_vals=6)
    A = dsa.dynamicsparse(I, J, V, M, N, binding=hip)
    B = dsa.dynamicsparse(I, J, V, M, N, binding=hip)
    rng = np.random.default_rng(9)
    res = dict(shape="config 3: %d x %d, %d nnz" % (M, N, A.nnz()), runs=RUNS, warmup=WARMUP, ks=list(KS),
               timing="host wall time around the blocking call(s), both streams drained before and after; median of the runs; "
                      "every run deletes the next k keys of one random permutation, the same keys on both matrices")

    def timed(fn, X):
        X.sync()
        t0 = time.perf_counter()
        fn()
        X.sync()
        return (time.perf_counter() - t0) * 1e6

    for side, name, keys, single in ((dsa.COLMAJOR, "columns", np.unique(J), "mat_deletecolumn"),
                                     (dsa.ROWMAJOR, "rows", np.unique(I), "mat_deleterow")):
        pool = rng.permutation(keys).astype(np.int64)
        at = 0
        out = {}
        for k in KS:
            tb, ts, removed = [], [], 0
            for run in range(WARMUP + RUNS):
                ks = pool[at:at + k]
                at += k
                d = torch.from_numpy(ks).to("cuda")
                torch.cuda.synchronize()
                got = []
                b_us = timed(lambda: got.append(A.delete_batch_dev(side, d.data_ptr(), k)), A)
                s_us = timed(lambda: [hip.call(single, B.h, int(q)) for q in ks], B)
                assert A.nnz() == B.nnz(), (name, k, run, A.nnz(), B.nnz())
                if run >= WARMUP:
                    tb.append(b_us)
                    ts.append(s_us)
                    removed += got[0]
            out[str(k)] = dict(batched_us=statistics.median(tb), per_key_loop_us=statistics.median(ts),
                               batched_runs_us=tb, per_key_loop_runs_us=ts, entries_removed_per_run=removed / RUNS,
                               speedup=statistics.median(ts) / statistics.median(tb))
        wins = [k for k in KS if out[str(k)]["speedup"] > 1.0]
        cross = None
        for k in KS:
            if all(q in wins for q in KS if q >= k):
                cross = k
                break
        out["batched_wins_from_k"] = cross
        inf = A.info(1 - side)
        out["twin_capacity"], out["twin_model_bytes"] = inf["capacity"], 4.125 * inf["capacity"]
        res[name] = out
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        assert not A.check(o)[2:7].any() and not B.check(o)[2:7].any()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
