#!/usr/bin/env python3
"""Device import on config 3 (1M x 1M, 10M nnz): the matrix built from a device CSR (int32 and int64 indices) and from device COO
(int64 1-based, read in place; int32 0-based) through dsa_mat_create_from_compressed_dev / dsa_mat_create_from_coo_dev, alternating in
the same process with dsa_mat_create_from_coo on the SAME triples from host arrays (the yardstick: 240 MB over PCIe first).  Every
build is a blocking call: wall time per build, handle creation included, the handle destroyed before the next one.  Model bytes of
the ingest launches, compressed with ib-byte indices: in ib * (outer + 1) + ib * nnz, out 16 * nnz.  The split into expand / keys /
build comes from the library's DSA_DBG_TIME line of one build per form in a child process (DSA_DEV=1; its extra wait between expand
and keys is why the child is not timed).  Writes profiles/import_c3.json and prints it as one JSON line.
Usage: python tools/importbench.py [reps]"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWMAJOR = 1
m = n = 1_000_000


def triples():
    import bench
    I, J, V = bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6)
    order = np.argsort(I, kind="stable")                     # CSR storage order: every form below holds the same triples in this order
    I, J, V = np.ascontiguousarray(I[order]), np.ascontiguousarray(J[order]), np.ascontiguousarray(V[order])
    ptr = np.searchsorted(I, np.arange(m + 1), side="right").astype(np.int64)
    return I, J, V, ptr


def forms(dsa, hip, I, J, V, ptr):
    import torch
    nnz = len(V)
    d = dict(v=torch.from_numpy(V).to("cuda"))
    for bits, dt in ((32, torch.int32), (64, torch.int64)):
        d["ptr%d" % bits] = torch.from_numpy(ptr).to("cuda").to(dt)
        d["idx%d" % bits] = torch.from_numpy(J - 1).to("cuda").to(dt)
    d["i64"], d["j64"] = torch.from_numpy(I).to("cuda"), torch.from_numpy(J).to("cuda")
    d["i32"], d["j32"] = (d["i64"] - 1).to(torch.int32), (d["j64"] - 1).to(torch.int32)
    torch.cuda.synchronize()
    P = {k: t.data_ptr() for k, t in d.items()}
    return d, {
        "host_coo": lambda: dsa.dynamicsparse(I, J, V, m, n, binding=hip),
        "dev_csr_int32": lambda: dsa.dynamicsparse_compressed_dev(ROWMAJOR, P["ptr32"], P["idx32"], P["v"], m, n, nnz, index_bits=32, binding=hip),
        "dev_csr_int64": lambda: dsa.dynamicsparse_compressed_dev(ROWMAJOR, P["ptr64"], P["idx64"], P["v"], m, n, nnz, index_bits=64, binding=hip),
        "dev_coo_int64_base1": lambda: dsa.dynamicsparse_dev(P["i64"], P["j64"], P["v"], nnz, m, n, binding=hip),
        "dev_coo_int32_base0": lambda: dsa.dynamicsparse_dev(P["i32"], P["j32"], P["v"], nnz, m, n, index_bits=32, index_base=0, binding=hip),
    }


def main():
    import dsa_loader
    child = len(sys.argv) > 1 and sys.argv[1] == "--split"
    reps = 2 if child else max(int(sys.argv[1]) if len(sys.argv) > 1 else 7, 3)
    split = {}
    if not child:
        # the child first: one GPU process at a time does the work
        env = dict(os.environ, DSA_DEV="1", DSA_DBG_TIME="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--split"], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("split child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        for mm in re.finditer(r"\[ingest\] (\w+) nnz=\d+ bits=(\d+) base=(\d+): expand ([\d.]+) ms  keys ([\d.]+) ms  build ([\d.]+) ms", r.stderr):
            split["dev_%s_int%s%s" % (mm.group(1), mm.group(2), "_base" + mm.group(3) if mm.group(1) == "coo" else "")] = dict(
                expand_ms=float(mm.group(4)), keys_ms=float(mm.group(5)), build_ms=float(mm.group(6)))
    dsa = dsa_loader.load()
    hip = dsa.product()
    I, J, V, ptr = triples()
    keep, fns = forms(dsa, hip, I, J, V, ptr)
    names = list(fns)
    ts = {k: [] for k in names}
    for rep in range(reps + (0 if child else 2)):              # two warm rounds (pool, streams, first-launch costs), then alternating
        for k in names:
            if child and k == "host_coo":
                continue
            t0 = time.perf_counter()
            a = fns[k]()
            dt = time.perf_counter() - t0
            a.close()
            if child or rep >= 2:
                ts[k].append(dt * 1e3)
    if child:
        return
    nnz = len(V)
    out = dict(workload="C3 import (1M x 1M, %d triples in CSR order), wall ms per blocking build" % nnz, reps=reps, builds={}, split_ms=split)
    for k in names:
        out["builds"][k] = dict(median_ms=round(float(np.median(ts[k])), 3), min_ms=round(float(np.min(ts[k])), 3),
                                all_ms=[round(float(t), 3) for t in ts[k]])
    for bits in (32, 64):
        ib = bits // 8
        out["builds"]["dev_csr_int%d" % bits]["ingest_model_bytes"] = ib * (m + 1) + ib * nnz + 16 * nnz
    host = out["builds"]["host_coo"]["median_ms"]
    out["ratio_vs_host"] = {k: round(out["builds"][k]["median_ms"] / host, 3) for k in names if k != "host_coo"}
    with open(os.path.join(ROOT, "profiles", "import_c3.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
