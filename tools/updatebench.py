#!/usr/bin/env python3
"""update_values_dev and get_batch_dev against the routes that exist without them, on the config-3 matrix (1 M x 1 M, 10 M nnz, built
as bench.py builds it; one cell per (i, j)).

Per size k in 10^3 .. 10^7, k distinct stored cells are drawn from findnz and kept in HBM with new nonzero values:

  update   update_values_dev (SET, strict) of the k triples in HBM, then sync()
  set      dsa_mat_set_batch of the same triples from host arrays on an identically built matrix in the same process — the route
           that exists today; a nonzero value on a stored cell moves no slot, so both matrices keep their layout from run to run
  get      get_batch_dev of the k cells into HBM, then sync(), against get_batch from and to host arrays

and once, for all cells, update_values_dev against scale_dev(alpha), the streaming floor of a value-only pass.  Host wall time around
the blocking call, both streams drained before and after; one warm-up run, then the median of three.

  python tools/updatebench.py [--out profiles/update_c3.json]
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
SIZES = (10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7)
RUNS, WARMUP = 3, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_c3.json"))
    ap.add_argument("--per", type=int, default=10, help="entries per column (10: config 3)")
    ap.add_argument("--size", type=int, default=M, help="rows = columns (10^6: config 3)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import dsa_loader
    dsa = dsa_loader.load()
    hip = dsa.product()
    m = n = a.size

    I, J, V = bench.c3_triplets(m, n, a.per, 0, seed_rows=5, seed_vals=6)
    A = dsa.dynamicsparse(I, J, V, m, n, binding=hip)         # update_values_dev / get_batch_dev
    B = dsa.dynamicsparse(I, J, V, m, n, binding=hip)         # set_batch / get_batch
    nnz = A.nnz()
    fi, fj, _ = A.findnz()
    assert len(fi) == nnz
    rng = np.random.default_rng(7)

    def timed(fn, X):
        X.sync()
        t0 = time.perf_counter()
        fn()
        X.sync()
        return (time.perf_counter() - t0) * 1e6

    def median_of(fn, X):
        t = [timed(fn, X) for _ in range(WARMUP + RUNS)][WARMUP:]
        return statistics.median(t), t

    inf = A.info(dsa.COLMAJOR)
    res = dict(shape="%d x %d, %d nnz, %d slots per orientation" % (m, n, nnz, inf["capacity"]), runs=RUNS, warmup=WARMUP,
               timing="host wall time around the blocking call, both streams drained before and after; median of the runs",
               by_size={})
    for k in SIZES:
        k = min(k, nnz)
        t = rng.choice(nnz, size=k, replace=False) if k < nnz else np.arange(nnz)
        hi, hj = np.ascontiguousarray(fi[t]), np.ascontiguousarray(fj[t])
        hv = 1.0 + rng.random(k)
        di, dj, dv = (torch.from_numpy(x).to("cuda") for x in (hi, hj, hv))
        dout = torch.empty(k, dtype=torch.float64, device="cuda")
        dfound = torch.empty(k, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        got = []
        upd, upd_runs = median_of(lambda: got.append(A.update_values_dev(di.data_ptr(), dj.data_ptr(), dv.data_ptr(), k)), A)
        assert all(g == (k, 0) for g in got), got
        st, st_runs = median_of(lambda: B.set_batch(hi, hj, hv), B)
        gd, gd_runs = median_of(lambda: A.get_batch_dev(di.data_ptr(), dj.data_ptr(), k, dout.data_ptr(), dfound.data_ptr()), A)
        outs = []
        gh, gh_runs = median_of(lambda: outs.append(B.get_batch(hi, hj)), B)
        assert np.array_equal(dout.cpu().numpy(), hv) and np.array_equal(outs[-1], hv) and bool(dfound.all())
        e = dict(update_values_dev_us=upd, update_runs_us=upd_runs, set_batch_us=st, set_batch_runs_us=st_runs,
                 set_batch_over_update=st / upd, update_cells_per_s=k / (upd * 1e-6), set_batch_cells_per_s=k / (st * 1e-6),
                 get_batch_dev_us=gd, get_batch_dev_runs_us=gd_runs, get_batch_us=gh, get_batch_runs_us=gh_runs,
                 get_batch_over_dev=gh / gd)
        if k == nnz:
            sc, sc_runs = median_of(lambda: A.scale_dev(1.0000001, 0, 0, 0, 0), A)
            e.update(scale_dev_us=sc, scale_runs_us=sc_runs, update_over_scale=upd / sc)
        res["by_size"][str(k)] = e
        print("k = %d: %s" % (k, json.dumps(e)), file=sys.stderr, flush=True)
    assert A.nnz() == nnz == B.nnz()
    for X in (A, B):
        for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
            assert not X.check(o)[2:7].any()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
