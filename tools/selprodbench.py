#!/usr/bin/env python3
"""Selected-key product against the full multi-vector product and the selected export, on the config-3 matrix (1 M x 1 M, 10 M nnz,
built as bench.py builds it).

For k in {1, 8}, for random selections of 0.1 %, 1 %, 10 % and 100 % of the rows (transpose = 0) and of the columns (transpose = 1),
and for one selection that holds a row of 20 000 cells (written into the matrix for this purpose: 1000 random rows and the long one),
timed with HIP events on the matrix's stream after a warm-up, one event pair per repetition, the three forms alternating:
  (sel) one dsa_mat_spmm_selected_dev;
  (a)   the full dsa_mat_spmm_dense_dev at the same k and the gather of the selected rows of its Y (torch.index_select);
  (b)   dsa_mat_select_compressed_dev of the same keys into buffers sized beforehand: what reading the same spans costs — exporting
        the selection and multiplying it outside the library can be no faster than this.
The result of (sel) is asserted to be bit-identical to the gathered rows of (a).  The default mode runs three fresh child processes
(each GPU step under its own time limit, the first failure ends the tool) and writes profiles/selprod_c3.json: per case the
min / median / max over the runs of each run's median, the ratios against (a) and (b), the model bytes of the kernel's header comment
and, per k and orientation, the smallest measured fraction at which (a) is the faster call.

  python tools/selprodbench.py [--runs 3] [--reps 20] [--out profiles/selprod_c3.json]
  python tools/selprodbench.py --child [--ks 8] [--reps 20]        one process, one JSON line on stdout (what a profiler wraps)
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = N = 1_000_000
FRACTIONS = (0.001, 0.01, 0.1, 1.0)
LONG_CELLS = 20_000


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
    rng = np.random.default_rng(17)
    vp = C.c_void_p
    out = dict(nnz=int(len(I)), m=M, n=N, reps=reps, warmup=warm, cases=[])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    def case(name, transpose, keys, k):
        tr = 1 if transpose else 0
        orientation = dsa.COLMAJOR if transpose else dsa.ROWMAJOR
        inf = A.info(orientation)
        nx, ny = (M, N) if transpose else (N, M)
        nsel = len(keys)
        sel = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64)).to("cuda")
        gat = sel - 1
        x = torch.from_numpy(bench.unit12(70 + k, nx * k).reshape(nx, k)).to("cuda")
        ys = torch.full((nsel, k), -7.25, dtype=torch.float64, device="cuda")
        yf = torch.zeros((ny, k), dtype=torch.float64, device="cuda")
        yg = torch.empty((nsel, k), dtype=torch.float64, device="cuda")
        ptr = torch.empty(nsel + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        cells, _ = A.select_compressed_dev(orientation, sel.data_ptr(), nsel, ptr.data_ptr(), 0, 0, 0)
        idx = torch.empty(max(cells, 1), dtype=torch.int64, device="cuda")
        val = torch.empty(max(cells, 1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def selected():
            hip.call("mat_spmm_selected_dev", A.h, tr, vp(sel.data_ptr()), nsel, vp(x.data_ptr()), nx, k, k, vp(ys.data_ptr()), k)

        def full():
            hip.call("mat_spmm_dense_dev", A.h, tr, vp(x.data_ptr()), nx, k, k, vp(yf.data_ptr()), ny, k)
            torch.index_select(yf, 0, gat, out=yg)

        def export():
            A.select_compressed_dev(orientation, sel.data_ptr(), nsel, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), cells)

        for _ in range(warm):
            selected()
            full()
            export()
        torch.cuda.synchronize()
        ev = [(timed(selected), timed(full), timed(export)) for _ in range(reps)]
        torch.cuda.synchronize()
        t = [[e[q][0].elapsed_time(e[q][1]) * 1e3 for e in ev] for q in range(3)]
        assert torch.equal(ys.view(torch.int64), yg.view(torch.int64)), name      # bit-identical to the rows of the full product
        out["cases"].append(dict(name=name, transpose=tr, k=k, nsel=nsel, cells=int(cells), capacity=int(inf["capacity"]),
                                 table_len=int(inf["table_len"]), nb_elements=int(inf["nb_elements"]),
                                 selected_us=statistics.median(t[0]), full_us=statistics.median(t[1]), export_us=statistics.median(t[2]),
                                 selected_us_min=min(t[0]), full_us_min=min(t[1]), export_us_min=min(t[2])))

    for k in ks:
        for transpose, dim in ((False, M), (True, N)):
            for f in FRACTIONS:
                keys = rng.permutation(dim)[:max(1, int(round(dim * f)))] + 1
                case("%s %g%%" % ("cols" if transpose else "rows", 100 * f), transpose, keys, k)
    # a row of 20 000 cells among 1000 ordinary ones (written last: the cases above see the matrix bench.py builds)
    long_row = 123_457
    cols = rng.choice(N, LONG_CELLS, replace=False) + 1
    A.set_batch(np.full(LONG_CELLS, long_row), cols, 0.5 + rng.random(LONG_CELLS))
    keys = np.concatenate([rng.permutation(M)[:500] + 1, [long_row], rng.permutation(M)[:500] + 1])
    for k in ks:
        case("1000 rows and one of %d cells" % LONG_CELLS, False, keys, k)
    print(json.dumps(out), flush=True)


def mmm(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=360, help="time limit of one child process in seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selprod_c3.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    if a.child:
        return child(a.ks, a.reps, a.warmup)
    runs = []
    for r in range(a.runs):
        # a fresh process per run, under its own time limit; the first one that fails ends the tool (nothing more is started)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup), "--ks"]
                               + [str(k) for k in a.ks], capture_output=True, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("run %d exceeded its time limit of %d s" % (r, a.child_timeout))
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("run %d failed with status %d" % (r, p.returncode))
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print("run %d: %s" % (r, {"%s k=%d" % (c["name"], c["k"]): (round(c["selected_us"], 1), round(c["full_us"], 1), round(c["export_us"], 1))
                                  for c in runs[-1]["cases"]}), flush=True)
    res = dict(shape="config 3: %d x %d, %d nnz" % (runs[0]["m"], runs[0]["n"], runs[0]["nnz"]), runs=len(runs), reps=a.reps, warmup=a.warmup,
               timing="HIP events on the matrix's stream, one pair per repetition, the three forms alternating; per run the median over "
                      "the repetitions; selected = dsa_mat_spmm_selected_dev, full = dsa_mat_spmm_dense_dev + gather of the selected "
                      "rows, export = dsa_mat_select_compressed_dev of the same keys",
               bitwise_agreement_with_full="asserted in every case of every run", cases=[], crossover={})
    for i, c0 in enumerate(runs[0]["cases"]):
        s, f, e = ([r["cases"][i][q] for r in runs] for q in ("selected_us", "full_us", "export_us"))
        k, nsel, cells = c0["k"], c0["nsel"], c0["cells"]
        # the slots of the selected spans are not known exactly without walking them: cells (and their semaphores) over the
        # structure's density (occupied slots, semaphores included, over the capacity); every other term is exact.  Config 3 fits
        # 32-bit keys: kb = 4
        slots = (cells + nsel) * c0["capacity"] / c0["nb_elements"]
        model = 8 * nsel + 8 * math.log2(max(c0["table_len"], 2)) * nsel + (4 + 8 + 1 / 8) * slots \
            + 64 * -(-k // 8) * cells + 8 * k * nsel
        res["cases"].append(dict(name=c0["name"], transpose=c0["transpose"], k=k, nsel=nsel, cells=cells, selected_us=mmm(s), full_us=mmm(f),
                                 export_us=mmm(e), ratio_full_over_selected=statistics.median(f) / statistics.median(s),
                                 ratio_export_over_selected=statistics.median(e) / statistics.median(s),
                                 selected_faster_than_full=max(s) < min(f), model_bytes=int(model),
                                 model_bytes_per_s=model / (statistics.median(s) * 1e-6)))
    for k in a.ks:
        for tr, what in ((0, "rows"), (1, "cols")):
            mine = [c for c in res["cases"] if c["k"] == k and c["transpose"] == tr and c["name"].startswith(what)]
            slower = [c["nsel"] / runs[0]["m" if tr == 0 else "n"] for c in mine if c["ratio_full_over_selected"] < 1.0]
            res["crossover"]["%s k=%d" % (what, k)] = dict(
                smallest_measured_fraction_where_full_is_faster=min(slower) if slower else None,
                largest_measured_fraction_where_selected_is_faster=max(
                    [c["nsel"] / runs[0]["m" if tr == 0 else "n"] for c in mine if c["ratio_full_over_selected"] >= 1.0], default=None))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(cases=[(c["name"], c["k"], round(c["selected_us"]["median"], 1), round(c["full_us"]["median"], 1),
                                  round(c["export_us"]["median"], 1)) for c in res["cases"]], crossover=res["crossover"]), indent=1))


if __name__ == "__main__":
    main()
