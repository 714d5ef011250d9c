#!/usr/bin/env python3
"""Dynamic vectors as device operands on config 3 (1M x 1M, 10M nnz), for x with 100, 10 000 and 394 000 stored entries:
  mul_vec  A.mul_vec(x) (dsa_mat_mul_vec: pack, widen, sparse-x product, builder, all in HBM) against the route that existed before it,
           dynamicsparsevec(*A.mul(x), n=m) with x a vector handle (nonzeros() down, the pairs up again, the result down, the pairs up);
  dot      v.dot(w) (dsa_vec_dot) for two such vectors that share about half of their keys against nonzeros() of both +
           numpy.intersect1d + numpy.dot.
Every run is a blocking call chain: host wall time, the result handle created and destroyed, median of three runs after a warm-up, the
compared calls alternating in one process.  The two products are compared once per size: keys and occupancy must agree, the largest
|difference| of a value is recorded (its bound per row is checked in tests/test_vector_device.py, not here).  Model
bytes of dot: (kb + 8) * min(na, nb) for the driving operand + the bisection, ceil(log2(max + 1)) dependent key loads per driving
cell.  No ratio is fixed in advance: the tool records both times and new / old.  Writes profiles/vec_c3.json and prints it as one JSON line.
Usage: python tools/vecbench.py [reps]"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
m = n = 1_000_000
SIZES = (100, 10_000, 394_000)


def sparse_keys(rng, count, upto):
    return np.sort(rng.choice(upto, count, replace=False).astype(np.int64) + 1)


def timed(reps, fns):
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for key, fn in fns.items():
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            if hasattr(r, "close"):
                r.close()
            ts[key].append(dt * 1e3)
    return ts


def main():
    import bench
    import dsa_loader
    reps = max(int(sys.argv[1]) if len(sys.argv) > 1 else 3, 3)
    dsa = dsa_loader.load()
    hip = dsa.product()
    A = dsa.dynamicsparse(*bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6), m, n, binding=hip)
    rng = np.random.default_rng(77)
    out = dict(workload="C3 (1M x 1M, 10M nnz): mul_vec and dot with dynamic vectors of nx stored entries, host wall ms per blocking "
                        "call chain, result handle created and destroyed", reps=reps, sizes={})
    for nx in SIZES:
        xk = sparse_keys(rng, nx, n)
        x = dsa.dynamicsparsevec(xk, rng.standard_normal(nx), n=n, binding=hip)
        wk = np.union1d(xk[::2], sparse_keys(rng, nx // 2, n))[:nx]
        w = dsa.dynamicsparsevec(wk, rng.standard_normal(len(wk)), n=n, binding=hip)

        def new_mul():
            return A.mul_vec(x)

        def old_mul():
            return dsa.dynamicsparsevec(*A.mul(x), n=m, binding=hip)

        def new_dot():
            return x.dot(w)

        def old_dot():
            (ak, av), (bk, bv) = x.nonzeros(), w.nonzeros()
            _, ia, ib = np.intersect1d(ak, bk, assume_unique=True, return_indices=True)
            return float(np.dot(av[ia], bv[ib]))

        # warm-up of every route (pool, streams, scratch) and the cross-check
        y1, y0 = new_mul(), old_mul()
        (k1, v1, o1), (k0, v0, o0) = y1.export_layout(), y0.export_layout()
        same_slots = bool(len(o1) == len(o0) and np.array_equal(o1, o0) and np.array_equal(k1[o1.astype(bool)], k0[o0.astype(bool)]))
        max_diff = float(np.max(np.abs(v1[o1.astype(bool)] - v0[o0.astype(bool)]))) if same_slots and o1.any() else 0.0
        touched = y1.nnz()
        y1.close(); y0.close()
        d1, d0 = new_dot(), old_dot()
        ts = timed(reps, dict(mul_vec=new_mul, mul_rebuild=old_mul, dot=new_dot, dot_host=old_dot))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        common = len(np.intersect1d(xk, wk, assume_unique=True))
        out["sizes"][str(nx)] = dict(
            x_entries=nx, w_entries=len(wk), common_keys=common, touched_rows=touched,
            strategy="x-driven" if nx * 8 < n else "gather",
            same_keys_and_occupancy_as_rebuild=same_slots, max_abs_value_difference=max_diff,
            mul_vec_ms=round(med["mul_vec"], 3), mul_rebuild_ms=round(med["mul_rebuild"], 3),
            ratio_mul_vec_over_rebuild=round(med["mul_vec"] / med["mul_rebuild"], 3),
            dot_ms=round(med["dot"], 3), dot_host_ms=round(med["dot_host"], 3),
            ratio_dot_over_host=round(med["dot"] / med["dot_host"], 3),
            dot_value=d1, dot_host_value=d0,
            dot_model_bytes=12 * min(nx, len(wk)), dot_dependent_loads_per_cell=math.ceil(math.log2(max(nx, len(wk)) + 1)),
            all_ms={k: [round(t, 3) for t in v] for k, v in ts.items()})
        x.close(); w.close()
    with open(os.path.join(ROOT, "profiles", "vec_c3.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if not all(s["same_keys_and_occupancy_as_rebuild"] for s in out["sizes"].values()):
        raise SystemExit("a mul_vec result stores other rows than the rebuilt product")


if __name__ == "__main__":
    main()
