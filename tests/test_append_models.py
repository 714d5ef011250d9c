"""What the append-replay models (csrc/appendmodel.hip) CONSUME.  A model that refuses a run writes {0, 0, reason} and the per-op
replay (csrc/appendrun.hip) takes all of it: the layout is the oracle's either way, so the layout tests cannot tell a model that
works from one that always refuses.  Here the eight result words are read back through the library's own trace line
(DSA_DEV=1 DSA_DBG_RUN=1, csrc/writes_host.hip):

    [append model v3|v5 (typed epochs)] run of R ops: placed P status S reason W | events above the tables E, table levels L | ...

One child process per library setting (the development switches are read once per process): tests/append_models_child.py runs the
scenarios on the product and on the oracle and prints a JSON line per batch behind the model lines of that batch.  The shapes are
the smallest the host launches a model on (512 ops / 65536 slots for the count-only model, 64 ops / 256 slots for the typed
epochs); the expectations come from the kernels' text: the count-only model consumes a whole run up to the op in front of an
_extend! (status 2), the epoch model whole leaf epochs (at most 9 cells each: only the trailing partial one is left).

Recorded when the file was written, (R, placed, status, reason, table levels) per line — the kernels were then rewritten as stage
sequences with the same lines:  vector, 16 slots, second 8000-op run: (8000, 3885, 2, 0, 11) (4114, 4114, 1, 0, 9);  segments of 2:
(8000, 6844, 2, 0, 14) (1155, 1155, 1, 0, 12);  of 8: (8000, 6556, 2, 0, 12) (1443, 1443, 1, 0, 10);  built matrix, 14 085 ops:
(14085, 10511, 2, 0, 10) (5918, 7573, 1, 0, 9);  grown matrix: 68 ops (68, 82, 1, 0, 6);  100: (100, 69, 1, 0, 6);  64: (64, 54, 1, 0, 7);
1469: (1469, 520, 1, 0, 8) (1030, 1246, 1, 0, 9);  4466: (4466, 210, ..) (4290, 2875, ..) (1894, 2278, 1, 0, 9);  12 592: (12592, 3466, ..)
(9699, 11507, ..) (95, 114, 1, 0, 9);  12 251: (12251, 14751, 1, 0, 9);  8200: (8200, 8048, ..) (4175, 8350, 1, 0, 9);  8193: (8193, 16382,
1, 0, 9);  the empty matrix: (114, 0, 0, 4, 0).  A 600-key run on the 30 000-cell vector after its highest 16 keys were deleted is NOT
refused (600, 600, 1, 0, 10), so the refusal case is the empty matrix, and the grown-matrix scenario starts below the 64-op minimum."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"\[append model (v3|v5 \(typed epochs\))\] run of (\d+) ops: placed (-?\d+) status (-?\d+) reason (-?\d+) \| "
                  r"events above the tables (-?\d+), table levels (-?\d+) \|")


def run_child(scenarios, **switches):
    """{scenario: [batch dict with its model lines under "lines"]}, batches in order"""
    env = dict(os.environ, DSA_DEV="1", DSA_DBG_RUN="1", **switches)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "append_models_child.py")] + scenarios, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out, lines = {}, []
    for text in r.stdout.splitlines():
        m = LINE.search(text)
        if m:
            lines.append({"kind": "v3" if m.group(1) == "v3" else "v5", "R": int(m.group(2)), "placed": int(m.group(3)), "status": int(m.group(4)),
                          "reason": int(m.group(5)), "events": int(m.group(6)), "levels": int(m.group(7))})
        elif text.startswith("{"):
            b = json.loads(text)
            b["lines"], lines = lines, []
            out.setdefault(b["scenario"], []).append(b)
            print(b["scenario"], b["batch"], "ops", b["ops"], "cells", b["cells"], "capacity", b["capacity"], "extends", b["stat_extends"],
                  [(ln["kind"], ln["R"], ln["placed"], ln["status"], ln["reason"], ln["levels"]) for ln in b["lines"]])
    assert not lines, lines
    return out


@pytest.fixture(scope="module")
def default_child():
    return run_child(["vec16", "vec_small", "refusal", "typed16", "m5"])


@pytest.fixture(scope="module")
def generic_child():
    return run_child(["m5"], DSA_MODEL5="2")


def check_oracle(batches, capacities, extends):
    """every batch slot for slot the oracle's (layout, capacity, stat_extends, stat_rebalances, stat_window_slots), on the geometry the
    scenario was chosen for.  Returns per batch (index from 1) whether the oracle extended in it."""
    assert [b["batch"] for b in batches] == list(range(len(capacities)))
    assert all(b["equal"] for b in batches), [b["batch"] for b in batches if not b["equal"]]
    assert [b["capacity"] for b in batches] == capacities
    assert [b["stat_extends"] - batches[0]["stat_extends"] for b in batches] == extends
    return [None] + [b["stat_extends"] != a["stat_extends"] for a, b in zip(batches, batches[1:])]


def whole_run(b, kind, placed):
    """exactly one line of `kind`: the model took the batch as one run and consumed `placed` cells of it"""
    assert [ln["kind"] for ln in b["lines"]] == [kind], b
    ln = b["lines"][0]
    assert ln["R"] == b["ops"] and (ln["placed"], ln["status"], ln["reason"]) == (placed, 1, 0), b


def up_to_the_extend(b, kind):
    """the first line of a batch the oracle extends in: everything in front of the op that extends, status 2"""
    assert b["lines"] and all(ln["kind"] == kind for ln in b["lines"]), b
    ln = b["lines"][0]
    assert ln["R"] == b["ops"] and ln["status"] == 2 and ln["reason"] == 0 and 0 < ln["placed"] < ln["R"], b


def test_count_only_model_takes_vector_runs_on_16_slot_segments(default_child):
    bs = default_child["vec16"]
    assert (bs[0]["segment"], bs[0]["height"]) == (16, 12)
    ext = check_oracle(bs, [65536] * 6 + [131072], [0] * 6 + [1])
    assert ext[1:] == [False] * 5 + [True]
    assert bs[1]["ops"] == 511 and bs[1]["lines"] == []              # below the host's minimum of 512 ops: no launch
    for b, r in zip(bs[2:6], (512, 513, 3000, 8000)):
        assert b["ops"] == r
        whole_run(b, "v3", r)
    up_to_the_extend(bs[6], "v3")


@pytest.mark.parametrize("n_first,segment", [(3, 2), (150, 8)])
def test_count_only_model_takes_vector_runs_on_small_segments(default_child, n_first, segment):
    bs = default_child["vec_small%d" % n_first]
    assert bs[0]["segment"] == segment
    check_oracle(bs, [65536] * 3 + [131072], [0, 0, 0, 1])
    whole_run(bs[1], "v3", 512)
    whole_run(bs[2], "v3", 3000)
    up_to_the_extend(bs[3], "v3")


def test_count_only_model_takes_typed_runs_on_a_built_matrix(default_child):
    bs = default_child["typed16"]
    assert bs[0]["segment"] == 16
    check_oracle(bs, [65536] * 5 + [131072], [0] * 5 + [1])
    assert [b["ops"] for b in bs[1:]] == [346, 529, 688, 5166, 14085]
    assert bs[1]["lines"] == []
    for b in bs[2:5]:
        whole_run(b, "v3", b["cells"])                               # cells of the run: its ops plus its new columns (semaphores)
    up_to_the_extend(bs[5], "v3")


M5_OPS = [57, 57, 61, 68, 100, 231, 64, 63, 1469, 4466, 12592, 12251, 8200, 8193]
M5_CAPACITY = [256, 256, 256, 512, 512, 1024, 1024, 2048, 2048, 4096, 16384, 65536, 65536, 131072, 131072]
M5_EXTENDS = [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 6, 8, 8, 9, 9]


def check_m5(bs):
    assert bs[0]["segment"] == 8
    ext = check_oracle(bs, M5_CAPACITY, M5_EXTENDS)
    assert [b["ops"] for b in bs[1:]] == M5_OPS
    for i, b in enumerate(bs[1:], start=1):
        # (the count-only model is never tried on typed runs over 8-slot segments: the host does not launch it there)
        assert all(ln["kind"] == "v5" for ln in b["lines"]), b
        if b["ops"] < 64:
            assert b["lines"] == [], b
        elif i == 14:
            # 8193 columns of one element: semaphores on the even cells, the 8192nd on cell 2 * 8191 — the list holds no more
            assert b["lines"][0]["status"] == 1 and b["lines"][0]["reason"] == 0 and 0 < b["lines"][0]["placed"] <= 2 * 8191, b
        elif not ext[i]:
            assert len(b["lines"]) == 1, b
            ln = b["lines"][0]
            assert ln["R"] == b["ops"] and ln["status"] == 1 and ln["reason"] == 0 and b["cells"] - 9 < ln["placed"] <= b["cells"], b
        else:
            assert b["lines"] and b["lines"][0]["status"] == 1, b
            assert all(0 <= ln["reason"] <= 9 for ln in b["lines"]), b
            assert sum(ln["placed"] for ln in b["lines"]) <= b["cells"], b
    for b in bs[11:13]:                                           # capacity 65536: events wider than the table rows
        assert b["height"] == 13 and all(ln["levels"] < 13 for ln in b["lines"]), b


def test_epoch_model_takes_typed_runs_on_a_grown_matrix(default_child):
    check_m5(default_child["m5"])


def test_generic_epoch_path_is_the_hand_scheduled_block(default_child, generic_child):
    """DSA_MODEL5=2: every epoch through the C++ epoch — two writings of one function"""
    check_m5(generic_child["m5"])
    key = lambda bs: [[(ln["R"], ln["placed"], ln["status"], ln["reason"]) for ln in b["lines"]] for b in bs]      # noqa: E731
    assert key(generic_child["m5"]) == key(default_child["m5"])


def test_a_refused_run_is_replayed_per_op(default_child):
    """114 ops on the EMPTY grown matrix: the last leaf holds no cell, so no tail (reason 4 of the epoch model: it commits nothing),
    and the whole run is the per-op replay's — the layout is the oracle's all the same"""
    bs = default_child["refusal"]
    check_oracle(bs, [256, 256], [0, 0])
    assert [ln["kind"] for ln in bs[1]["lines"]] == ["v5"], bs[1]
    ln = bs[1]["lines"][0]
    assert (ln["R"], ln["placed"], ln["status"], ln["reason"]) == (114, 0, 0, 4), bs[1]
