#!/usr/bin/env python3
"""droptol against its floor and against the zero writes it replaces, on the config-3 matrix (1 M x 1 M, 10 M nnz, 2^24 slots,
built as bench.py builds it; its values are distinct and lie in [1, 2), one cell per (i, j)).

Per fraction f in {0, 0.1 %, 1 %, 10 %, 50 %} the threshold is the order statistic of |v| that drops round(f * nnz) cells (f = 0:
a threshold below every value).  A droptol cannot be repeated on the matrix it changed, so every run builds the matrix again — the
same triples, so the same layout — and times one call on it: host wall time around the blocking call, both streams drained before
and after.  One warm-up run, then the median of three.  Two references are measured the same way in the same process:

  floor      what the call is built from, per orientation one after the other: one reduce("absmax") pass (the same slot stream:
             occupancy, keys and values once) plus one dsa_mat_rebalance_root.  droptol runs its two orientations concurrently and
             rebalances only when something is dropped, so it may come in below this sum.
  set_batch  what a user does today: the same cells written with 0.0 through set_batch on an identically built matrix.  Only the
             set_batch call is timed — the export and the host-side search for the cells, which that way also needs, are not — and
             a fraction is skipped once the one before it took longer than --skip-after seconds.

  python tools/dropbench.py [--out profiles/drop_c3.json]
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
FRACTIONS = (0.0, 0.001, 0.01, 0.1, 0.5)
RUNS, WARMUP = 3, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_c3.json"))
    ap.add_argument("--skip-after", type=float, default=20.0)
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
    absv = np.sort(np.abs(V))
    build = lambda: dsa.dynamicsparse(I, J, V, m, n, binding=hip)

    def timed(fn, X):
        X.sync()
        t0 = time.perf_counter()
        fn()
        X.sync()
        return (time.perf_counter() - t0) * 1e6

    A = build()
    nnz = A.nnz()
    inf = [A.info(o) for o in (dsa.COLMAJOR, dsa.ROWMAJOR)]
    slots = sum(i["capacity"] for i in inf)
    res = dict(shape="%d x %d, %d nnz, %d + %d slots" % (m, n, nnz, inf[0]["capacity"], inf[1]["capacity"]), runs=RUNS, warmup=WARMUP,
               fractions=list(FRACTIONS),
               timing="host wall time around the blocking call(s), both streams drained before and after; median of the runs; every "
                      "droptol and set_batch run is on a freshly built matrix",
               model_bytes_pass1=12.125 * slots)

    # ---- the floor: on one matrix, it changes nothing the next run would see differently
    out_r = torch.empty(m, dtype=torch.float64, device="cuda")
    out_c = torch.empty(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    red, reb = [], []
    for run in range(WARMUP + RUNS):
        t_red = timed(lambda: (A.reduce_dev("absmax", "row", out_r.data_ptr(), m), A.reduce_dev("absmax", "column", out_c.data_ptr(), n)), A)
        t_reb = timed(lambda: (A.rebalance_root(dsa.COLMAJOR), A.rebalance_root(dsa.ROWMAJOR)), A)
        if run >= WARMUP:
            red.append(t_red)
            reb.append(t_reb)
    floor = dict(reduce_absmax_both_us=statistics.median(red), rebalance_root_both_us=statistics.median(reb),
                 reduce_runs_us=red, rebalance_runs_us=reb)
    floor["total_us"] = floor["reduce_absmax_both_us"] + floor["rebalance_root_both_us"]
    res["floor"] = floor
    del A

    skip_set = False
    res["by_fraction"] = {}
    for f in FRACTIONS:
        k = int(round(f * nnz))
        tol = float(absv[k - 1]) if k > 0 else float(absv[0]) / 2
        sel = np.abs(V) <= tol
        k = int(sel.sum())
        td, ts = [], []
        for run in range(WARMUP + RUNS):
            X = build()
            got = []
            us = timed(lambda: got.append(X.droptol(tol)), X)
            assert got[0] == k and X.nnz() == nnz - k, (f, got, k)
            if run == 0:
                for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
                    assert not X.check(o)[2:7].any()
            del X
            if run >= WARMUP:
                td.append(us)
        if k > 0 and not skip_set:
            Is, Js, Zs = I[sel], J[sel], np.zeros(k)
            for run in range(WARMUP + RUNS):
                Y = build()
                us = timed(lambda: Y.set_batch(Is, Js, Zs), Y)
                assert Y.nnz() == nnz - k, (f, Y.nnz())
                del Y
                if run >= WARMUP:
                    ts.append(us)
                if us > a.skip_after * 1e6:
                    skip_set = True
                    break
        e = dict(tol=tol, dropped=k, droptol_us=statistics.median(td), droptol_runs_us=td,
                 over_floor=statistics.median(td) / floor["total_us"],
                 over_read_pass=statistics.median(td) / floor["reduce_absmax_both_us"])
        if ts:
            e.update(set_batch_us=statistics.median(ts), set_batch_runs_us=ts, speedup_over_set_batch=statistics.median(ts) / statistics.median(td),
                     set_batch_writes_per_s=k / (statistics.median(ts) * 1e-6))
        res["by_fraction"]["%g" % f] = e
        print("f = %g: %s" % (f, json.dumps(e)), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
