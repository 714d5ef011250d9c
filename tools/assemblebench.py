#!/usr/bin/env python3
"""assemble_dev against the routes that exist without it and against the floor it is built from, on the config-3 matrix (1 M x 1 M,
10 M nnz, built as bench.py builds it; 2^24 slots per orientation).

Per n in 10^4, 10^5, 10^6, 10^7 triples:

  add    "add" of n triples on stored cells, 1 and 4 ops per cell, the triples in HBM, against
           combine     A + dynamicsparse_dev(I, J, V): a new matrix, the only device route without the call
           add_values  add_values of triples folded on the host (numpy), the fold and the upload counted
           floor       update_values_dev ("add") of the distinct cells, folded beforehand, in HBM
  set    "set" of n distinct cells, 90 % stored and 10 % in new columns behind the last, against
           set_batch   set_batch of the same triples from host arrays
           upsert      upsert of the same (distinct) triples from host arrays
           floor       update_values_dev of the stored ones + insert_values_dev of the others, split beforehand, in HBM

Every timed run is on a freshly built matrix (dynamicsparse_dev from triples that stay in HBM); the calls of one comparison
alternate in one process.  Host wall time around the blocking call, both streams drained before and after; one warm-up run, then
the median of three.

  python tools/assemblebench.py [--out profiles/assemble_c3.json]
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
SIZES = (10_000, 100_000, 1_000_000, 10_000_000)
RUNS, WARMUP = 3, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_c3.json"))
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
    rows_live = np.unique(I)
    rng = np.random.default_rng(13)
    dev = lambda *xs: tuple(torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in xs)
    ptr = lambda t: t.data_ptr()

    def fresh():
        x = dsa.dynamicsparse_dev(dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), nnz0, m, n, binding=hip)
        x.sync()
        return x

    def timed(fn, X):
        X.sync()
        t0 = time.perf_counter()
        out = fn(X)
        (out if hasattr(out, "sync") else X).sync()      # a new handle (combine) is drained itself
        return (time.perf_counter() - t0) * 1e6

    def compare(fns):
        """{name: (median, runs)} of the calls of one comparison, alternating, each run on a fresh matrix"""
        t = {k: [] for k in fns}
        for _ in range(WARMUP + RUNS):
            for k, fn in fns.items():
                t[k].append(timed(fn, fresh()))
        return {k: (statistics.median(v[WARMUP:]), v[WARMUP:]) for k, v in t.items()}

    x0 = fresh()
    res = dict(shape="%d x %d, %d nnz, %d slots per orientation" % (m, n, x0.nnz(), x0.info(dsa.COLMAJOR)["capacity"]), runs=RUNS, warmup=WARMUP,
               timing="host wall time around the blocking call on a freshly built matrix, both streams drained before and after; median of the "
                      "runs; the calls of one comparison alternate",
               add={}, set={})
    del x0

    def entry(cnt, r, ours, floor):
        e = dict(ops=cnt)
        for k, (med, runs) in r.items():
            e[k + "_us"], e[k + "_runs_us"] = med, runs
            if k != ours:
                e[k + "_over_" + ours] = med / r[ours][0]
        e[ours + "_over_" + floor] = r[ours][0] / r[floor][0]
        e[ours + "_ops_per_s"] = cnt / (r[ours][0] * 1e-6)
        return e

    for cnt in a.sizes:
        for per_cell in (1, 4):
            cells = max(cnt // per_cell, 1)
            pick = rng.choice(nnz0, min(cells, nnz0), replace=False)
            rep = rng.permutation(np.repeat(pick, per_cell))
            hi, hj, hv = np.ascontiguousarray(I[rep]), np.ascontiguousarray(J[rep]), 1.0 + rng.random(len(rep))
            di, dj, dv = dev(hi, hj, hv)
            # the distinct cells with their sums, for the floor (any summation order: the floor is about time)
            key, inv = np.unique(hi * np.int64(n + 1) + hj, return_inverse=True)
            fi, fj, fv = dev(key // np.int64(n + 1), key % np.int64(n + 1), np.bincount(inv, weights=hv))
            torch.cuda.synchronize()
            got = []

            def do_assemble(X):
                out = X.assemble_dev(ptr(di), ptr(dj), ptr(dv), len(hi), dsa.UPD_ADD)
                if not got:
                    got.append(out)

            def do_combine(X):
                return X + dsa.dynamicsparse_dev(ptr(di), ptr(dj), ptr(dv), len(hi), m, n, binding=hip)

            def do_add_values(X):
                k2, iv = np.unique(hi * np.int64(n + 1) + hj, return_inverse=True)
                X.add_values(k2 // np.int64(n + 1), k2 % np.int64(n + 1), np.bincount(iv, weights=hv))

            r = compare(dict(assemble=do_assemble, combine=do_combine, add_values=do_add_values,
                             floor=lambda X: X.update_values_dev(ptr(fi), ptr(fj), ptr(fv), len(key), dsa.UPD_ADD)))
            assert got[0] == (len(key), len(key), 0), (got, len(key))
            e = entry(len(hi), r, "assemble", "floor")
            e["distinct"] = len(key)
            res["add"]["%d x %d" % (len(hi), per_cell)] = e
            print("add n = %d, %d per cell: %s" % (len(hi), per_cell, json.dumps(e)), file=sys.stderr, flush=True)
        # set: 90 % stored cells, 10 % cells in new columns (a.per cells each, in rows the matrix has)
        nh = min(cnt - cnt // 10, nnz0)
        nm = cnt - nh
        pick = rng.choice(nnz0, nh, replace=False)
        kcols = (nm + a.per - 1) // a.per
        mj = np.repeat(np.arange(n + 1, n + 1 + kcols, dtype=np.int64), a.per)[:nm]
        # per column a.per distinct rows, ascending: sorted draws plus 0, 1, 2, ...
        mi = rows_live[np.sort(rng.integers(0, len(rows_live) - a.per, (kcols, a.per)), axis=1) + np.arange(a.per)].reshape(-1)[:nm]
        mv = 1.0 + rng.random(nm)
        # shuffled hits in front, the new columns in key order behind them: set_batch takes new columns in any order, but slowly
        sh = rng.permutation(nh)
        hi, hj = np.concatenate([I[pick][sh], mi]), np.concatenate([J[pick][sh], mj])
        hv = np.concatenate([1.0 + rng.random(nh), mv])
        hi, hj = np.ascontiguousarray(hi), np.ascontiguousarray(hj)
        di, dj, dv = dev(hi, hj, hv)
        ui, uj, uv = dev(hi[:nh], hj[:nh], hv[:nh])
        ni, nj, nv = dev(mi, mj, mv)
        torch.cuda.synchronize()
        got = []

        def do_assemble_set(X):
            out = X.assemble_dev(ptr(di), ptr(dj), ptr(dv), cnt, dsa.UPD_SET)
            if not got:
                got.append(out)

        def do_floor(X):
            X.update_values_dev(ptr(ui), ptr(uj), ptr(uv), nh, dsa.UPD_SET)
            X.insert_values_dev(ptr(ni), ptr(nj), ptr(nv), nm)

        r = compare(dict(assemble=do_assemble_set, set_batch=lambda X: X.set_batch(hi, hj, hv), upsert=lambda X: X.upsert(hi, hj, hv),
                         floor=do_floor))
        assert got[0] == (cnt, nh, nm), (got, cnt, nh, nm)
        e = entry(cnt, r, "assemble", "floor")
        e.update(hits=nh, new_cells=nm, new_columns=kcols)
        res["set"][str(cnt)] = e
        print("set n = %d: %s" % (cnt, json.dumps(e)), file=sys.stderr, flush=True)
        # partial results survive a run that is cut short
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
