"""Child process of tests/test_append_models.py: append-run scenarios on the product library and the CPU oracle, side by side.
The parent sets DSA_DEV=1 DSA_DBG_RUN=1 (and DSA_MODEL5=2 for the generic-epoch child): the library then prints one
`[append model ...]` line per model launch to stderr.  This script prints one JSON line per batch, flushed, so that on a shared
pipe the model lines of a batch stand in front of its JSON line.

Usage: python tests/append_models_child.py SCENARIO...      (APPEND_MODELS_SELF=1: oracle against oracle, no GPU)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dsa_loader  # noqa: E402
import oracle_binding  # noqa: E402
from util import MAT_INFO_KEYS, SplitMix64, layouts_equal, unit12_array  # noqa: E402

dsa = dsa_loader.load()
ora = oracle_binding.load(dsa)
hip = ora if os.environ.get("APPEND_MODELS_SELF") == "1" else dsa.product()
STATS = ("capacity", "stat_extends", "stat_rebalances", "stat_window_slots")


def report(scenario, batch, equal, info, ops, cells):
    sys.stderr.flush()
    print(json.dumps({"scenario": scenario, "batch": batch, "equal": bool(equal), "capacity": int(info["capacity"]),
                      "segment": int(info["segment_capacity"]), "height": int(info["height"]),
                      "stat_extends": int(info["stat_extends"]), "ops": int(ops), "cells": int(cells)}), flush=True)


def vec_equal(a, b):
    ia, ib = a.info(), b.info()
    return layouts_equal(a.export_layout(), b.export_layout()) and all(ia[k] == ib[k] for k in STATS)


def mat_equal(a, b):
    if a.size() != b.size():
        return False
    for o in (0, 1):
        La, Lb = a.export_layout(o), b.export_layout(o)
        ia, ib = a.info(o), b.info(o)
        if any(La["info"][k] != Lb["info"][k] for k in MAT_INFO_KEYS) or any(ia[k] != ib[k] for k in STATS):
            return False
        if not layouts_equal((La["keys"], La["vals"], La["occ"]), (Lb["keys"], Lb["vals"], Lb["occ"])):
            return False
        if not all(np.array_equal(La[k], Lb[k]) for k in ("semaphores", "col_live", "col_keys")):
            return False
    return True


def vector_runs(name, a, b, nxt, runs):
    """append runs of consecutive keys from `nxt` on; batch 0 reports the vector as it was built"""
    report(name, 0, vec_equal(a, b), b.info(), 0, 0)
    for r_i, r in enumerate(runs, start=1):
        ks = np.arange(nxt, nxt + r, dtype=np.int64)
        nxt += r
        vs = unit12_array(20 + r_i, r)
        a.set_batch(ks, vs); b.set_batch(ks, vs)
        report(name, r_i, vec_equal(a, b), b.info(), r, r)


def build_vec(n_first, total):
    keys = np.arange(1, total + 1, dtype=np.int64) * 2
    pair = [dsa.dynamicsparsevec(keys[:n_first], unit12_array(9, n_first), binding=x) for x in (hip, ora)]
    if total > n_first:
        for v in pair:
            v.set_batch(keys[n_first:], unit12_array(10, total - n_first))
    return pair[0], pair[1], int(keys[-1]) + 1


def scenario_vec16():
    a, b, nxt = build_vec(30000, 30000)
    vector_runs("vec16", a, b, nxt, [511, 512, 513, 3000, 8000, 8000])


def scenario_vec_small():
    for n_first in (3, 150):
        a, b, nxt = build_vec(n_first, 36000)
        vector_runs("vec_small%d" % n_first, a, b, nxt, [512, 3000, 8000])


def columns(g, col, ncols, nrows, maxlen):
    """`ncols` new columns behind `col`: 1 + next % maxlen draws of 1 + next % nrows each, de-duplicated and sorted"""
    I, J = [], []
    for _ in range(ncols):
        col += 1
        rows = sorted({1 + g.next() % nrows for _ in range(1 + g.next() % maxlen)})
        I += rows
        J += [col] * len(rows)
    return I, J, col


def matrix_batches(name, a, b, g, col, nrows, batches):
    report(name, 0, mat_equal(a, b), b.info(0), 0, 0)
    for r_i, (ncols, maxlen) in enumerate(batches, start=1):
        I, J, col = columns(g, col, ncols, nrows, maxlen)
        V = unit12_array(50 + r_i, len(I))
        a.set_batch(I, J, V); b.set_batch(I, J, V)
        report(name, r_i, mat_equal(a, b), b.info(0), len(I), len(I) + ncols)


def scenario_typed16():
    g = SplitMix64(4242)
    I0, J0, col = columns(g, 0, 6000, 4000, 6)
    V0 = unit12_array(7, len(I0))
    a, b = (dsa.dynamicsparse(I0, J0, V0, binding=x) for x in (hip, ora))
    matrix_batches("typed16", a, b, g, col, 4000, [(n, 6) for n in (100, 150, 200, 1500, 4000)])


# (columns, longest column) per batch.  The first 20 columns come in two batches below the model's 64-op minimum: a run on the
# EMPTY matrix is launched and refused (no tail in the last leaf: scenario_refusal), so the first launch here finds cells
M5_BATCHES = [(10, 9), (10, 9), (13, 9), (14, 9), (16, 9), (40, 9), (64, 1), (63, 1), (300, 9), (900, 9), (2500, 9), (2500, 9), (8200, 1), (8193, 1)]


def scenario_m5():
    a, b = (dsa.dynamicsparse(fill_mode=False, binding=x) for x in (hip, ora))
    matrix_batches("m5", a, b, SplitMix64(77), 0, 5000, M5_BATCHES)


def scenario_refusal():
    """the first 20 columns of the same stream as ONE batch: the last leaf of an empty matrix holds no tail"""
    a, b = (dsa.dynamicsparse(fill_mode=False, binding=x) for x in (hip, ora))
    matrix_batches("refusal", a, b, SplitMix64(77), 0, 5000, [(20, 9)])


if __name__ == "__main__":
    for s in sys.argv[1:]:
        globals()["scenario_" + s]()
