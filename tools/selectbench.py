#!/usr/bin/env python3
"""Selected export on the C3 matrix (1M x 1M, 10M nnz, 2^24-slot orientations): A[:, J] as CSC with int32 indices for 0.1 %, 1 %, 10 %
and 100 % of the columns, ascending and in random order.  Every shape is warmed, then timed by HIP events on the orientation's stream
(bracketed by a synchronise), alternating with dsa_mat_to_compressed_dev of the whole matrix in the same process (the yardstick); a loop
of dsa_mat_col_view_dev over the 0.1 % selection is what the selection replaces.  Model bytes of a selection:
  in   8 * nsel + 8 * log2(table_len) * nsel + (kb + 8) * span_slots + 2 * span_slots / 8
  out  (ib + 8) * total + ib * (nsel + 1)
with span_slots = the slots between the selected partitions' semaphores and the next live ones.  Writes profiles/select_c3.json and
prints it as one JSON line.  Usage: python tools/selectbench.py [reps]"""
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

PEAK = 8e12
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


full_ptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
full_idx = torch.empty(nnz, dtype=torch.int32, device="cuda")
full_val = torch.empty(nnz, dtype=torch.float64, device="cuda")


def full_export():
    a.to_compressed_dev(COLMAJOR, full_ptr.data_ptr(), full_idx.data_ptr(), full_val.data_ptr(), nnz, index_bits=32)


full_bytes = (kb + 8) * cap + cap // 8 + 17 * tl + (ib + 8) * nnz + ib * (n + 1)
out = dict(workload="C3 selected export, colmajor, int32 (1M x 1M, %d nnz, %d slots)" % (nnz, cap), reps=reps, peak_bytes_per_s=PEAK,
           selections={}, full_export={}, col_view_loop={})
rng = np.random.default_rng(17)
full_ts = []
for frac, label in ((0.001, "0.1%"), (0.01, "1%"), (0.1, "10%"), (1.0, "100%")):
    k = int(round(n * frac))
    asc = np.sort(rng.permutation(n)[:k] + 1).astype(np.int64)
    for order, sel in (("ascending", asc), ("random", rng.permutation(asc))):
        d_sel = torch.from_numpy(sel).to("cuda")
        ptr = torch.empty(k + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        total, _ = a.select_compressed_dev(COLMAJOR, d_sel.data_ptr(), k, ptr.data_ptr(), 0, 0, 0, index_bits=32)
        idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        val = torch.empty(max(total, 1), dtype=torch.float64, device="cuda")

        def select():
            a.select_compressed_dev(COLMAJOR, d_sel.data_ptr(), k, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), total, index_bits=32)

        for _ in range(3):
            select()
            full_export()
        ts = []
        for _ in range(reps):                               # alternating with the yardstick
            ts.append(one(select))
            full_ts.append(one(full_export))
        slots = int(span_of_key[sel].sum())
        model = 8 * k + int(8 * math.log2(max(tl, 2)) * k) + (kb + 8) * slots + 2 * (slots // 8) + (ib + 8) * total + ib * (k + 1)
        e = stats(ts)
        e.update(nsel=k, cells=int(total), span_slots=slots, model_bytes=model, gb_per_s=round(model / (e["median_us"] * 1e-6) / 1e9, 1))
        out["selections"]["%s_%s" % (label, order)] = e
        if frac == 0.001 and order == "ascending":
            keys = torch.empty(4096, dtype=torch.int64, device="cuda")
            vals = torch.empty(4096, dtype=torch.float64, device="cuda")

            def loop():
                for c in sel:
                    a.col_view_dev(int(c), keys.data_ptr(), vals.data_ptr(), 4096)

            loop()
            e = stats([one(loop) for _ in range(reps)])
            e.update(nsel=k)
            out["col_view_loop"] = e
e = stats(full_ts)
e.update(physical_bytes=full_bytes, gb_per_s=round(full_bytes / (e["median_us"] * 1e-6) / 1e9, 1))
e.pop("all_us")
out["full_export"] = e
out["ratio_0.1%_ascending_vs_col_view_loop"] = round(out["selections"]["0.1%_ascending"]["median_us"] / out["col_view_loop"]["median_us"], 4)
out["ratio_100%_ascending_vs_full_export"] = round(out["selections"]["100%_ascending"]["median_us"] / out["full_export"]["median_us"], 3)
with open(os.path.join(ROOT, "profiles", "select_c3.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
