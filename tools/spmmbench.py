#!/usr/bin/env python3
"""SpMM against the loop of single products on the config-3 matrix (1 M x 1 M, 10 M nnz, built as bench.py builds it).

For k in {2, 4, 8, 16}, timed with HIP events on the matrix's stream after a warm-up, one event pair per repetition, the two
forms alternating:
  (a) one dsa_mat_spmm_dense_dev on a row-major X (nx x k);
  (b) k back-to-back dsa_mat_spmv_dense_dev(algo = 0) on the k columns stored contiguously per column, the column-swept plan
      warmed — the fastest existing way to the same Y.
The default mode runs three fresh child processes and writes profiles/spmm_c3.json: per k the min / median / max over the runs of
each run's median, their ratio, the model bytes 12 * capacity + 64 * ceil(k / 8) * nnz + 8 * k * (nx + ny) and the fraction of the
8 TB/s peak that the model bytes over the measured SpMM time come to.

  python tools/spmmbench.py [--runs 3] [--reps 30] [--out profiles/spmm_c3.json]
  python tools/spmmbench.py --child [--ks 8] [--reps 30]        one process, one JSON line on stdout (what a profiler wraps)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12
M = N = 1_000_000


def child(ks, reps, warm):
    import numpy as np
    import torch

    import bench
    import dsa_loader
    dsa = dsa_loader.load()
    hip = dsa.product()
    I, J, V = bench.c3_triplets(M, N, 10, 0, seed_rows=5, seed_vals=6)
    A = dsa.dynamicsparse(I, J, V, M, N, binding=hip)
    stream = torch.cuda.current_stream()
    hip.call("mat_set_stream", A.h, C.c_void_p(stream.cuda_stream))
    inf = A.info(dsa.ROWMAJOR)
    out = dict(capacity=inf["capacity"], nnz=int(len(I)), nx=N, ny=M, reps=reps, warmup=warm, k={})
    vp = C.c_void_p

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    for k in ks:
        xc = torch.from_numpy(bench.unit12(70 + k, N * k).reshape(k, N)).to("cuda")      # (b): one contiguous column per row
        xr = xc.t().contiguous()                                                          # (a): row-major nx x k
        yc = torch.zeros((k, M), dtype=torch.float64, device="cuda")
        yr = torch.zeros((M, k), dtype=torch.float64, device="cuda")

        def spmm():
            hip.call("mat_spmm_dense_dev", A.h, 0, vp(xr.data_ptr()), N, k, k, vp(yr.data_ptr()), M, k)

        def loop():
            for j in range(k):
                hip.call("mat_spmv_dense_dev", A.h, 0, 0, vp(xc[j].data_ptr()), N, vp(yc[j].data_ptr()), M)

        for _ in range(warm):        # the plan of (b) is built on the second product and used from the third on
            spmm()
            loop()
        torch.cuda.synchronize()
        plan_products = A.info(dsa.ROWMAJOR)["stat_spmv_plan"]
        ev = [(timed(spmm), timed(loop)) for _ in range(reps)]
        torch.cuda.synchronize()
        ta = [a[0].elapsed_time(a[1]) * 1e3 for a, _ in ev]
        tb = [b[0].elapsed_time(b[1]) * 1e3 for _, b in ev]
        err = float(((yr.t() - yc).abs() / yc.abs().clamp_min(1e-300)).max())
        assert err <= 1e-12, err                                                          # the two forms computed the same Y
        out["k"][str(k)] = dict(spmm_us=statistics.median(ta), loop_us=statistics.median(tb), spmm_us_min=min(ta), loop_us_min=min(tb),
                                max_rel_diff=err, loop_used_plan=A.info(dsa.ROWMAJOR)["stat_spmv_plan"] > plan_products)
        del xc, xr, yc, yr
    print(json.dumps(out), flush=True)


def mmm(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ks", type=int, nargs="*", default=[2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_c3.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    if a.child:
        return child(a.ks, a.reps, a.warmup)
    runs = []
    for r in range(a.runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup), "--ks"]
                           + [str(k) for k in a.ks], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("run %d failed with status %d" % (r, p.returncode))
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print("run %d: %s" % (r, {k: (round(v["spmm_us"], 1), round(v["loop_us"], 1)) for k, v in runs[-1]["k"].items()}), flush=True)
    cap, nnz, nx, ny = (runs[0][f] for f in ("capacity", "nnz", "nx", "ny"))
    res = dict(shape="config 3: %d x %d, %d nnz, capacity %d slots (rowmajor)" % (ny, nx, nnz, cap), runs=len(runs), reps=a.reps, warmup=a.warmup,
               timing="HIP events on the matrix's stream, one pair per repetition, (a) and (b) alternating; per run the median over the repetitions",
               peak_bytes_per_s=PEAK_BYTES_PER_S, k={})
    for k in a.ks:
        sa = [r["k"][str(k)]["spmm_us"] for r in runs]
        sb = [r["k"][str(k)]["loop_us"] for r in runs]
        model = 12 * cap + 64 * -(-k // 8) * nnz + 8 * k * (nx + ny)
        res["k"][str(k)] = dict(spmm_us=mmm(sa), spmv_loop_us=mmm(sb), ratio_loop_over_spmm=statistics.median(sb) / statistics.median(sa),
                                slowest_spmm_below_fastest_loop=max(sa) < min(sb), model_bytes=model,
                                fraction_of_peak=model / (statistics.median(sa) * 1e-6) / PEAK_BYTES_PER_S,
                                loop_used_plan=all(r["k"][str(k)]["loop_used_plan"] for r in runs),
                                max_rel_diff=max(r["k"][str(k)]["max_rel_diff"] for r in runs))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["k"], indent=1))


if __name__ == "__main__":
    main()
