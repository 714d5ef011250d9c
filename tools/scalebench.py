#!/usr/bin/env python3
"""Reduce and scale against their yardsticks on the config-3 matrix (1 M x 1 M, 10 M nnz, 2^24 slots, built as bench.py builds it).

Everything is timed with HIP events on the matrix's stream (both orientations are put on it), one event pair per repetition after a
warm-up, the median over the repetitions, all in one process:
  per orientation  each reduce kind (dsa_mat_reduce_dev; the event pair includes the hand-over of the bounds word);
                   dsa_mat_spmm_dense_dev at k = 1 with X = ones — the same slot stream plus the gathers of X: reduce's yardstick;
                   dsa_mat_rebalance_root — reads and writes the slot array once: scale's yardstick;
  both at once     dsa_mat_scale_dev with alpha, r and c (the call covers both orientations: compare with the SUM of the two
                   rebalances), and the same split into its check pass and the rest by a scale with alpha alone.
The long-row case is a 1000 x 1 000 000 matrix whose row 1 holds 10^6 cells: reduce per row and the k = 1 product over it.
Bytes per slot are the model of csrc/scale.hip (int32 keys): reduce 12.1, scale 4.1 (check) + 12.1 + 8 * fill (apply).

  python tools/scalebench.py [--reps 30] [--warmup 5] [--out profiles/scale_c3.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12
M = N = 1_000_000
KINDS = ("sum", "abssum", "sqsum", "absmax", "count")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_c3.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    import numpy as np
    import torch

    import bench
    import dsa_loader
    dsa = dsa_loader.load()
    hip = dsa.product()
    vp = C.c_void_p
    stream = torch.cuda.current_stream()

    def median_us(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        t = [x.elapsed_time(y) * 1e3 for x, y in ev]
        return dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t))

    def measure(A, m, n, kinds, with_scale):
        hip.call("mat_set_stream", A.h, vp(stream.cuda_stream))
        out = {}
        ones = torch.ones(max(m, n), dtype=torch.float64, device="cuda")
        y = torch.zeros(max(m, n), dtype=torch.float64, device="cuda")
        for o, per, dim, nx in ((dsa.ROWMAJOR, "row", m, n), (dsa.COLMAJOR, "column", n, m)):
            inf = A.info(o)
            r = dict(capacity=inf["capacity"], cells=inf["nb_elements"] - inf["nb_partitions"], partitions=inf["nb_partitions"])
            for kind in kinds:
                r["reduce_" + kind] = median_us(lambda: A.reduce_dev(kind, per, y.data_ptr(), dim))
            tr = 1 if o == dsa.COLMAJOR else 0
            r["spmm_k1_ones"] = median_us(lambda: hip.call("mat_spmm_dense_dev", A.h, tr, vp(ones.data_ptr()), nx, 1, 1, vp(y.data_ptr()), dim, 1))
            r["rebalance_root"] = median_us(lambda: A.rebalance_root(o))
            bytes_reduce = 12.125 * inf["capacity"]
            r["reduce_sum_fraction_of_peak"] = bytes_reduce / (r["reduce_sum"]["median_us"] * 1e-6) / PEAK_BYTES_PER_S
            out[per] = r
        if with_scale:
            rng = np.random.default_rng(7)
            fr = torch.from_numpy(1.0 + 0.001 * (rng.random(m) - 0.5)).to("cuda")
            fc = torch.from_numpy(1.0 + 0.001 * (rng.random(n) - 0.5)).to("cuda")
            torch.cuda.synchronize()
            s = dict(all_three=median_us(lambda: A.scale_dev(1.0009765625, fr.data_ptr(), m, fc.data_ptr(), n)),
                     alpha_only=median_us(lambda: A.scale_dev(1.0, 0, 0, 0, 0)))
            s["rebalance_root_both"] = out["row"]["rebalance_root"]["median_us"] + out["column"]["rebalance_root"]["median_us"]
            cap = out["row"]["capacity"] + out["column"]["capacity"]
            cells = out["row"]["cells"] + out["column"]["cells"]
            s["model_bytes"] = (4.125 + 12.125) * cap + 8 * cells
            s["fraction_of_peak"] = s["model_bytes"] / (s["all_three"]["median_us"] * 1e-6) / PEAK_BYTES_PER_S
            out["scale_both_orientations"] = s
        hip.call("mat_sync", A.h)
        return out

    I, J, V = bench.c3_triplets(M, N, 10, 0, seed_rows=5, seed_vals=6)
    A = dsa.dynamicsparse(I, J, V, M, N, binding=hip)
    res = dict(shape="config 3: %d x %d, %d nnz" % (M, N, len(I)), reps=a.reps, warmup=a.warmup,
               timing="HIP events on the matrix's stream, one pair per repetition, median over the repetitions, one process",
               peak_bytes_per_s=PEAK_BYTES_PER_S, c3=measure(A, M, N, KINDS, True))
    del A
    # the long-row case: one partition of 10^6 cells among 30 000 ordinary cells
    rng = np.random.default_rng(8)
    m2, n2, L = 1000, 1_000_000, 1_000_000
    I2 = np.concatenate([np.ones(L, dtype=np.int64), rng.integers(2, m2 + 1, 30_000)])
    J2 = np.concatenate([np.arange(1, L + 1), rng.integers(1, n2 + 1, 30_000)])
    B = dsa.dynamicsparse(I2, J2, rng.random(len(I2)) + 0.5, m2, n2, binding=hip)
    res["long_row"] = dict(shape="%d x %d, row 1 holds %d cells" % (m2, n2, L), **measure(B, m2, n2, ("sum",), False))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
