#!/usr/bin/env python3
"""Submatrix export on the C3 matrix (1M x 1M, 10M nnz, 2^24-slot orientations): A[I, J] as CSC with int32 indices for a random outer
list J of 1 %, 10 % and all of the columns and random inner lists I of 1 %, 10 % and 50 % of the rows (distinct, in random order).
Every shape is warmed, then timed by HIP events on the orientation's stream (bracketed by a synchronise), alternating in the same
process with dsa_mat_select_compressed_dev on the SAME outer list (A[:, J], every row: the yardstick, and what a caller had to export
and filter before).  Both calls are the fitting ones: for the submatrix the table fill, both counts and the emit with their three
host waits, for the selection count and emit with their two.  Model bytes of a submatrix call:
  in   8 * (nouter + ninner) + 8 * log2(table_len) * nouter + 2 * (kb + 8) * cells_in_spans + 2 * span_slots / 8 + 12 * kept
  out  12 * table_capacity + (ib + 8) * kept + ib * (nouter + 1)
(cells_in_spans: every cell of the selected partitions has its key read and one 8-byte table entry probed, in the count and in the
emit; kept: value and position are read for kept cells only).  The file records, per shape, both medians and the
submatrix-to-select ratio.  Writes profiles/submatrix_c3.json and prints it as one JSON line.
Usage: python tools/submatrixbench.py [reps]"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import dsa_loader  # noqa: E402

COLMAJOR = 0
reps = max(int(sys.argv[1]) if len(sys.argv) > 1 else 20, 20)
dsa = dsa_loader.load()
hip = dsa.product()
m = n = 1_000_000
I, J, V = bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6)
a = dsa.dynamicsparse(I, J, V, binding=hip)
stream = torch.cuda.current_stream()
hip.call("mat_set_stream", a.h, C.c_void_p(stream.cuda_stream))
nnz = a.nnz()
L = a.export_layout(COLMAJOR)
cap, tl = L["info"]["capacity"], L["info"]["table_len"]
live = np.flatnonzero(L["semaphores"] != 0)
sem = L["semaphores"][live]
span_of_key = np.zeros(n + 2, dtype=np.int64)              # slots behind the semaphore of column key k up to the next live one
keys_live = L["col_keys"][live]
inside = (keys_live >= 1) & (keys_live <= n)
span_of_key[keys_live[inside]] = (np.append(sem[1:] - 1, cap) - sem)[inside]
del L
kb, ib = 4, 4                                               # C3 keys fit 32 bits; int32 indices


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(ts):
    return dict(median_us=round(float(np.median(ts)), 2), min_us=round(float(np.min(ts)), 2), all_us=[round(float(t), 2) for t in ts])


out = dict(workload="C3 submatrix export, colmajor, int32 (1M x 1M, %d nnz, %d slots)" % (nnz, cap), reps=reps, shapes={})
rng = np.random.default_rng(23)
for ofrac, olabel in ((0.01, "1%"), (0.1, "10%"), (1.0, "100%")):
    no = int(round(n * ofrac))
    outer = (rng.permutation(n)[:no] + 1).astype(np.int64)
    d_outer = torch.from_numpy(outer).to("cuda")
    ptr = torch.empty(no + 1, dtype=torch.int32, device="cuda")
    sptr = torch.empty(no + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cells, _ = a.select_compressed_dev(COLMAJOR, d_outer.data_ptr(), no, sptr.data_ptr(), 0, 0, 0, index_bits=32)
    sidx = torch.empty(max(cells, 1), dtype=torch.int32, device="cuda")
    sval = torch.empty(max(cells, 1), dtype=torch.float64, device="cuda")
    slots = int(span_of_key[outer].sum())

    def select():
        a.select_compressed_dev(COLMAJOR, d_outer.data_ptr(), no, sptr.data_ptr(), sidx.data_ptr(), sval.data_ptr(), cells, index_bits=32)

    for ifrac, ilabel in ((0.01, "1%"), (0.1, "10%"), (0.5, "50%")):
        ni = int(round(m * ifrac))
        inner = (rng.permutation(m)[:ni] + 1).astype(np.int64)
        d_inner = torch.from_numpy(inner).to("cuda")
        torch.cuda.synchronize()
        kept, _ = a.submatrix_compressed_dev(COLMAJOR, d_outer.data_ptr(), no, d_inner.data_ptr(), ni, ptr.data_ptr(), 0, 0, 0, index_bits=32)
        idx = torch.empty(max(kept, 1), dtype=torch.int32, device="cuda")
        val = torch.empty(max(kept, 1), dtype=torch.float64, device="cuda")

        def submatrix():
            a.submatrix_compressed_dev(COLMAJOR, d_outer.data_ptr(), no, d_inner.data_ptr(), ni, ptr.data_ptr(), idx.data_ptr(),
                                       val.data_ptr(), kept, index_bits=32)

        for _ in range(3):
            submatrix()
            select()
        ts, ss = [], []
        for _ in range(reps):                               # alternating with the yardstick
            ts.append(one(submatrix))
            ss.append(one(select))
        tcap = 2
        while tcap < 2 * ni:
            tcap *= 2
        model = (8 * (no + ni) + int(8 * math.log2(max(tl, 2)) * no) + 2 * (kb + 8) * cells + 2 * (slots // 8) + 12 * kept
                 + 12 * tcap + (ib + 8) * kept + ib * (no + 1))
        e = dict(nouter=no, ninner=ni, cells_in_spans=int(cells), kept=int(kept), span_slots=slots, table_capacity=tcap, model_bytes=model,
                 submatrix=stats(ts), select_same_outer=stats(ss))
        e["gb_per_s"] = round(model / (e["submatrix"]["median_us"] * 1e-6) / 1e9, 1)
        e["ratio_submatrix_vs_select"] = round(e["submatrix"]["median_us"] / e["select_same_outer"]["median_us"], 3)
        out["shapes"]["outer_%s_inner_%s" % (olabel, ilabel)] = e
with open(os.path.join(ROOT, "profiles", "submatrix_c3.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
