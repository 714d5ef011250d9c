#!/usr/bin/env python3
"""insert_values_dev against the routes that exist without it, on the config-3 matrix (1 M x 1 M, 10 M nnz, built as bench.py
builds it; 2^24 slots per orientation).

Per k in 1, 8, 64, 512, 4096, 65536, two kinds of batch, the triples in HBM:

  columns  k new columns behind the last, 10 cells each, in rows the matrix has
  fill     10 k cells that are not stored, in rows and columns the matrix has

and per kind

  insert   insert_values_dev of the triples
  set      set_batch of the same triples from host arrays on an identically built matrix in the same process
  hcat     (columns only) hcat with a block built by dynamicsparse_dev from the triples, build included: a new handle

and once the floor an insert is built from: two rebalance_root, one orientation after the other.  Every run uses a freshly built
matrix (the triples stay in HBM, dynamicsparse_dev builds it).  Host wall time around the blocking call, both streams drained
before and after; one warm-up run, then the median of three.

  python tools/insertbench.py [--out profiles/insert_c3.json]
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
SIZES = (1, 8, 64, 512, 4096, 65536)
RUNS, WARMUP = 3, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insert_c3.json"))
    ap.add_argument("--per", type=int, default=10, help="entries per column (10: config 3)")
    ap.add_argument("--size", type=int, default=M, help="rows = columns (10^6: config 3)")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import dsa_loader
    dsa = dsa_loader.load()
    hip = dsa.product()
    m = n = a.size

    I, J, V = bench.c3_triplets(m, n, a.per, 0, seed_rows=5, seed_vals=6)
    dI, dJ, dV = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in (I, J, V))
    torch.cuda.synchronize()
    nnz0 = len(I)
    stored = np.sort(I * np.int64(n + 1) + J)
    rows_live, cols_live = np.unique(I), np.unique(J)
    assert cols_live[-1] == n
    rng = np.random.default_rng(11)

    def fresh():
        x = dsa.dynamicsparse_dev(dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), nnz0, m, n, binding=hip)
        x.sync()
        return x

    def timed(fn, X):
        X.sync()
        t0 = time.perf_counter()
        out = fn(X)
        (out if out is not None else X).sync()
        return (time.perf_counter() - t0) * 1e6

    def median_of(fn):
        t = [timed(fn, fresh()) for _ in range(WARMUP + RUNS)][WARMUP:]
        return statistics.median(t), t

    def batch(kind, k):
        if kind == "columns":
            bj = np.repeat(np.arange(n + 1, n + 1 + k, dtype=np.int64), a.per)
            bi = np.concatenate([np.sort(rows_live[rng.choice(len(rows_live), a.per, replace=False)]) for _ in range(k)])
        else:
            want, bi, bj = a.per * k, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
            while len(bi) < want:
                ci = rows_live[rng.integers(0, len(rows_live), 2 * want)]
                cj = cols_live[rng.integers(0, len(cols_live), 2 * want)]
                key = ci * np.int64(n + 1) + cj
                ok = ~np.isin(key, stored)
                key, first = np.unique(np.concatenate([bi * np.int64(n + 1) + bj, key[ok]]), return_index=True)
                bi, bj = key // np.int64(n + 1), key % np.int64(n + 1)
            pick = rng.permutation(len(bi))[:want]
            bi, bj = bi[pick], bj[pick]
        return np.ascontiguousarray(bi), np.ascontiguousarray(bj), 1.0 + rng.random(len(bi))

    x0 = fresh()
    inf = x0.info(dsa.COLMAJOR)
    res = dict(shape="%d x %d, %d nnz, %d slots per orientation" % (m, n, x0.nnz(), inf["capacity"]), runs=RUNS, warmup=WARMUP,
               timing="host wall time around the blocking call on a freshly built matrix, both streams drained before and after; median of the runs",
               by_kind={})
    del x0

    def two_root_rebalances(X):
        X.rebalance_root(dsa.COLMAJOR)
        X.rebalance_root(dsa.ROWMAJOR)

    fl, fl_runs = median_of(two_root_rebalances)
    res["two_root_rebalances_us"], res["two_root_rebalances_runs_us"] = fl, fl_runs
    print("floor: %.1f us" % fl, file=sys.stderr, flush=True)
    for kind in ("columns", "fill"):
        res["by_kind"][kind] = {}
        for k in a.sizes:
            hi, hj, hv = batch(kind, k)
            cnt = len(hi)
            di, dj, dv = (torch.from_numpy(x).to("cuda") for x in (hi, hj, hv))
            torch.cuda.synchronize()
            checked = []

            def do_insert(X):
                X.insert_values_dev(di.data_ptr(), dj.data_ptr(), dv.data_ptr(), cnt)
                if not checked:
                    checked.append(X.nnz())

            ins, ins_runs = median_of(do_insert)
            assert checked[0] == nnz0 + cnt, (checked, nnz0, cnt)
            st, st_runs = median_of(lambda X: X.set_batch(hi, hj, hv))
            e = dict(cells=cnt, insert_values_dev_us=ins, insert_runs_us=ins_runs, set_batch_us=st, set_batch_runs_us=st_runs,
                     set_batch_over_insert=st / ins, insert_over_floor=ins / fl, insert_cells_per_s=cnt / (ins * 1e-6),
                     set_batch_cells_per_s=cnt / (st * 1e-6))
            if kind == "columns":
                djl = dj - n

                def do_hcat(X):
                    blk = dsa.dynamicsparse_dev(di.data_ptr(), djl.data_ptr(), dv.data_ptr(), cnt, m, k, binding=hip)
                    return dsa.hcat(X, blk)

                hc, hc_runs = median_of(do_hcat)
                e.update(hcat_us=hc, hcat_runs_us=hc_runs, hcat_over_insert=hc / ins)
            res["by_kind"][kind][str(k)] = e
            print("%s k = %d: %s" % (kind, k, json.dumps(e)), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
