#!/usr/bin/env python3
"""Combine on config 3 (1M x 1M, 10M nnz): copy(A), A + B (B a second 10M-nnz build on the same shape) and hcat(A, B) with B = 1 % new
columns (10 000 columns of 10 entries) through dsa_mat_combine, each alternating in the same process with the route that existed before
it: to_compressed_dev of each operand (CSC, int64, base 1), the expansion of ptr to column keys and torch.cat in HBM, dynamicsparse_dev.
Every run is a blocking call chain: host wall time with the result handle created and destroyed, median of three runs after a warm-up.
Both routes feed the builder the same triples in the same order, so the two results are compared slot for slot once per operation.
Model bytes of the combine passes per operand: (kb + 8) * capacity + capacity / 8 in, 24 * nnz out (then the builder).  No ratio is fixed
in advance: the tool records both times and new / old.  Writes profiles/combine_c3.json and prints it as one JSON line.
Usage: python tools/combinebench.py [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLMAJOR = 0
m = n = 1_000_000
NEW_COLS = n // 100
ARRAYS = ("keys", "vals", "occ", "semaphores", "col_keys", "col_live")


def export_triples(a, col_off=0):
    """findnz(a) in HBM the old way: the CSC export, then ptr expanded to column keys (one torch kernel chain, no host copy)"""
    import torch
    rows, cols = a.size()
    nnz = a.nnz()
    ptr = torch.empty(cols + 1, dtype=torch.int64, device="cuda")
    idx = torch.empty(max(nnz, 1), dtype=torch.int64, device="cuda")
    val = torch.empty(max(nnz, 1), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                                 # the library writes on its own stream
    got = a.to_compressed_dev(COLMAJOR, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz, index_bits=64, base=1)
    a.sync()
    assert got == nnz
    keys = torch.arange(1 + col_off, cols + 1 + col_off, dtype=torch.int64, device="cuda")
    J = torch.repeat_interleave(keys, ptr[1:] - ptr[:-1], output_size=nnz)
    return idx[:nnz], J, val[:nnz]


def old_route(dsa, hip, operands, rows, cols):
    """operands: (matrix, column offset); the concatenated triples imported as they are"""
    import torch
    parts = [export_triples(a, off) for a, off in operands]
    I, J, V = (torch.cat([p[k] for p in parts]).contiguous() for k in range(3))
    torch.cuda.synchronize()                                 # the library reads on streams of its own
    return dsa.dynamicsparse_dev(I.data_ptr(), J.data_ptr(), V.data_ptr(), int(V.numel()), rows, cols, binding=hip)


def same_layout(x, y):
    if x.size() != y.size():
        return False
    for o in (0, 1):
        Lx, Ly = x.export_layout(o), y.export_layout(o)
        if Lx["info"]["capacity"] != Ly["info"]["capacity"]:
            return False
        if any(not np.array_equal(Lx[k].view(np.uint8), Ly[k].view(np.uint8)) for k in ARRAYS):
            return False
    return True


def pass_bytes(a):
    info = a.info(COLMAJOR)
    cap, nnz = info["capacity"], a.nnz()
    kb = 4 if max(a.size()) < 2 ** 31 else 8
    return (kb + 8) * cap + cap // 8, 24 * nnz


def main():
    import bench
    import dsa_loader
    reps = max(int(sys.argv[1]) if len(sys.argv) > 1 else 3, 3)
    dsa = dsa_loader.load()
    hip = dsa.product()
    A = dsa.dynamicsparse(*bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6), m, n, binding=hip)
    B = dsa.dynamicsparse(*bench.c3_triplets(m, n, 10, 0, seed_rows=15, seed_vals=16), m, n, binding=hip)
    Ih, Jh, Vh = bench.c3_triplets(m, NEW_COLS, 10, 0, seed_rows=25, seed_vals=26)
    H = dsa.dynamicsparse(Ih, Jh, Vh, m, NEW_COLS, binding=hip)
    ops = {
        "copy": (lambda: A.copy(), lambda: old_route(dsa, hip, [(A, 0)], m, n), [A]),
        "add": (lambda: A + B, lambda: old_route(dsa, hip, [(A, 0), (B, 0)], m, n), [A, B]),
        "hcat_1pct": (lambda: dsa.hcat(A, H), lambda: old_route(dsa, hip, [(A, 0), (H, n)], m, n + NEW_COLS), [A, H]),
    }
    out = dict(workload="C3 combine (1M x 1M, 10M nnz per full operand; hcat adds %d columns of 10), host wall ms per blocking call, "
                        "result handle created and destroyed" % NEW_COLS, reps=reps, ops={})
    for name, (new, old, operands) in ops.items():
        x, y = new(), old()                                  # warm-up of both routes (pool, streams, scratch), and the cross-check
        same = same_layout(x, y)
        nnz_out = x.nnz()
        x.close(); y.close()
        ts = dict(combine=[], export_import=[])
        for _ in range(reps):
            for key, fn in (("combine", new), ("export_import", old)):
                t0 = time.perf_counter()
                r = fn()
                dt = time.perf_counter() - t0
                r.close()
                ts[key].append(dt * 1e3)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        bytes_in, bytes_out = (sum(p[k] for p in map(pass_bytes, operands)) for k in (0, 1))
        out["ops"][name] = dict(result_nnz=nnz_out, same_layout_as_export_import=bool(same),
                                combine_ms=round(med["combine"], 3), export_import_ms=round(med["export_import"], 3),
                                ratio_combine_over_export_import=round(med["combine"] / med["export_import"], 3),
                                combine_all_ms=[round(t, 3) for t in ts["combine"]],
                                export_import_all_ms=[round(t, 3) for t in ts["export_import"]],
                                pass_model_bytes_in=bytes_in, pass_model_bytes_out=bytes_out)
    with open(os.path.join(ROOT, "profiles", "combine_c3.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if not all(o["same_layout_as_export_import"] for o in out["ops"].values()):
        raise SystemExit("a combine result differs from the export / import route")


if __name__ == "__main__":
    main()
