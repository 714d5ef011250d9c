"""GPU parity tests (run on a real MI355X with `-m gpu`): the HIP library, called through the C ABI,
against (1) the reference's own golden vectors, (2) the survey digests and (3) the CPU oracle slot for
slot on seeded inputs.  Integer keys, slot positions, semaphore tables: bit-exact.  Float64 SpMV
accumulations: relative 1e-12 (north_star tolerance)."""
import json
import os
import sys

import numpy as np
import pytest

import ka
from scenario import run_scenario
from util import (SplitMix64, assert_mat_equal, check_key_order, check_semaphores, layouts_equal, orientation_equal, splitmix_array,
                  unit12_array)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "reference_cases.json")) as f:
    CASES = json.load(f)
with open(os.path.join(HERE, "golden", "survey_known_answers.json")) as f:
    KA = json.load(f)

RTOL = 1e-12


def subset_equal(got, exp, path=""):
    for k, v in exp.items():
        if k.startswith("_"):
            continue
        assert k in got, path + k
        if isinstance(v, dict):
            subset_equal(got[k], v, path + k + ".")
        else:
            assert got[k] == v, (path + k, got[k], v)


def assert_vec_equal(a, b):
    ia, ib = a.info(), b.info()
    for k in ("capacity", "segment_capacity", "nb_segments", "nb_elements", "height"):
        assert ia[k] == ib[k], (k, ia, ib)
    assert len(a) == len(b)
    assert layouts_equal(a.export_layout(), b.export_layout())


# ---------------------------------------------------------------- golden vectors of the reference
@pytest.mark.parametrize("sc", CASES["scenarios"], ids=lambda s: s["name"])
def test_reference_scenarios_on_hip(dsa, hip, sc):
    run_scenario(dsa, hip, sc)


def test_survey_known_answers_on_hip(dsa, hip):
    subset_equal(ka.ka4(dsa, hip), KA["ka4"])
    subset_equal(ka.ka5(dsa, hip), KA["ka5"])
    exp = json.loads(json.dumps(KA["ka6"]))
    exp["c"].pop("shrinks")
    subset_equal(ka.ka6(dsa, hip, batch=True), exp)
    got = ka.ka7_9(dsa, hip, batch=True)
    y4 = got["ka7"].pop("y4")
    exp7 = {k: json.loads(json.dumps(KA[k])) for k in ("ka7", "ka8", "ka9")}
    y4_exp = exp7["ka7"].pop("y4")
    subset_equal(got, exp7)
    for a, e in zip(y4, y4_exp):
        assert abs(float.fromhex(a) - float.fromhex(e)) <= RTOL * abs(float.fromhex(e))


# ---------------------------------------------------------------- full-window rebalance (pack + spread)
FP_EDGE = [(64, 15), (128, 25), (128, 21), (64, 1), (64, 63), (64, 64), (64, 0), (2, 1), (4, 3), (8, 8), (16, 1)]


@pytest.mark.parametrize("cap,m", FP_EDGE + [(1 << 10, 1), (1 << 12, 2867), (1 << 14, 11468), (1 << 15, 9830),
                                             (1 << 16, 45875), (1 << 18, 100000), (1 << 20, 734003)])
def test_bulk_spread_matches_oracle(dsa, hip, oracle, cap, m):
    """dynamicsparsevec of n keys -> capacity rule + one full-array spread (src/pma.jl:42-55,69-84).
    (W, E) pairs of SURVEY App. A.3 where floor(fl(k*fl(W/E))) != floor(kW/E) are included via n."""
    # choose n so that capacity_for(n) == cap when possible, else just use m keys
    n = m if m > 0 else 0
    keys = (np.arange(1, n + 1) * 3).astype(np.int64)
    vals = unit12_array(11, n) if n else np.zeros(0)
    a = dsa.dynamicsparsevec(keys, vals, binding=hip)
    b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
    assert_vec_equal(a, b)


@pytest.mark.parametrize("n", [5, 45, 100, 1000, 5000, 70000, 300000, 1000003])
def test_rebalance_root_idempotent_and_equal(dsa, hip, oracle, n):
    keys = np.cumsum(1 + (splitmix_array(3, n) % np.uint64(5)).astype(np.int64))
    vals = unit12_array(4, n)
    a = dsa.dynamicsparsevec(keys, vals, binding=hip)
    b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
    assert_vec_equal(a, b)
    # punch holes (deletes that do not trigger a rebalance are fine too), then rebalance the root window
    dele = keys[:: 7][: min(2000, n // 7)]
    a.set_batch(dele, np.zeros(len(dele)))
    b.set_batch(dele, np.zeros(len(dele)))
    assert_vec_equal(a, b)
    a.rebalance_root()
    b.rebalance_root()
    assert_vec_equal(a, b)
    a.rebalance_root()
    assert_vec_equal(a, b)


# ---------------------------------------------------------------- batched writes through the device sequencer
@pytest.mark.parametrize("seed,n0,nops,keyspace", [(1, 0, 3000, 10 ** 6), (2, 1000, 5000, 5000), (3, 10000, 20000, 10 ** 7),
                                                   (4, 50, 4000, 300)])
def test_vec_mixed_batch_matches_oracle(dsa, hip, oracle, seed, n0, nops, keyspace):
    g = SplitMix64(seed)
    keys0 = sorted({1 + g.next() % keyspace for _ in range(n0)})
    vals0 = [g.unit12() for _ in keys0]
    a = dsa.dynamicsparsevec(keys0, vals0, binding=hip)
    b = dsa.dynamicsparsevec(keys0, vals0, binding=oracle)
    ks, vs = [], []
    for _ in range(nops):
        r = g.next() % 10
        k = 1 + g.next() % keyspace
        ks.append(k)
        vs.append(0.0 if r < 3 else g.unit12())
    a.set_batch(ks, vs)
    b.set_batch(ks, vs)
    assert_vec_equal(a, b)
    q = [1 + g.next() % keyspace for _ in range(500)] + ks[:500]
    assert np.array_equal(a.get_batch(q), b.get_batch(q))
    assert a.nnz() == b.nnz()


def test_c1_plumbing_vector_10k_plus_1k_ops(dsa, hip, oracle):
    """BASELINE config 1: 10k-nnz vector + 1k mixed setindex! (70% new / 20% overwrite / 10% delete)."""
    g = SplitMix64(1)
    seen, keys = set(), []
    while len(keys) < 10000:
        k = 1 + g.next() % 10 ** 7
        if k not in seen:
            seen.add(k)
            keys.append(k)
    g6 = SplitMix64(6)
    vals = [g6.unit12() for _ in keys]
    a = dsa.dynamicsparsevec(keys, vals, binding=hip)
    b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
    assert a.info()["capacity"] == 1 << 14
    g2 = SplitMix64(2)
    ks, vs = [], []
    for _ in range(1000):
        r = g2.next() % 10
        if r < 7:
            ks.append(1 + g2.next() % 10 ** 7); vs.append(g2.unit12())
        elif r < 9:
            ks.append(keys[g2.next() % len(keys)]); vs.append(g2.unit12())
        else:
            ks.append(keys[g2.next() % len(keys)]); vs.append(0.0)
    for k, v in zip(ks[:200], vs[:200]):      # single-op entry point
        a[k] = v
        b[k] = v
    a.set_batch(ks[200:], vs[200:])
    b.set_batch(ks[200:], vs[200:])
    assert_vec_equal(a, b)


@pytest.mark.parametrize("n0,napp", [(700, 300), (44000, 6000), (175000, 40000)])
def test_ascending_appends_trigger_big_windows_and_extend(dsa, hip, oracle, n0, napp):
    """The append pattern of BASELINE config 2 (scaled): escalates through every window level, the
    grid-wide rebalance kernel (windows > 8192 slots) and _extend!."""
    keys0 = np.arange(1, n0 + 1, dtype=np.int64) * 2
    vals0 = unit12_array(3, n0)
    a = dsa.dynamicsparsevec(keys0, vals0, binding=hip)
    b = dsa.dynamicsparsevec(keys0, vals0, binding=oracle)
    app = np.arange(2 * n0 + 1, 2 * n0 + 1 + napp, dtype=np.int64)
    vapp = unit12_array(5, napp)
    a.set_batch(app, vapp)
    b.set_batch(app, vapp)
    assert_vec_equal(a, b)
    ia, ib = a.info(), b.info()
    assert ia["stat_extends"] == ib["stat_extends"] and ia["stat_window_slots"] == ib["stat_window_slots"]
    assert ia["stat_rebalances"] == ib["stat_rebalances"]
    # descending deletes: shrink path
    a.set_batch(app[::-1], np.zeros(napp))
    b.set_batch(app[::-1], np.zeros(napp))
    assert_vec_equal(a, b)


@pytest.mark.parametrize("n0,runs,seed", [(1, [64, 65, 200], 1), (3, [5000], 2), (100, [63, 64, 1000, 70, 3000], 3),
                                           (5000, [20000, 100, 64], 4), (70000, [150000], 5), (20, [70] * 12, 6)])
def test_append_runs_simulated_on_the_bitmap_match_oracle(dsa, hip, oracle, n0, runs, seed):
    """Ascending append runs (>= 64 ops) take the bitmap-only path of the sequencer (insert + density scan + spread!
    replayed on occupancy words, cells moved once by K-permute).  Runs of many lengths, from tiny capacities (leaf-only
    arrays, segment < 64 slots) through several _extend!s, separated by ops that break a run: an update of an existing key,
    a delete, an insert in the middle, a descending key, an explicit zero."""
    rng = np.random.default_rng(seed)
    keys0 = np.arange(1, n0 + 1, dtype=np.int64) * 3
    a = dsa.dynamicsparsevec(keys0, unit12_array(seed, n0), binding=hip)
    b = dsa.dynamicsparsevec(keys0, unit12_array(seed, n0), binding=oracle)
    top = int(keys0[-1])
    for r_i, r in enumerate(runs):
        steps = rng.integers(1, 4, size=r).astype(np.int64)
        app = top + np.cumsum(steps)
        top = int(app[-1])
        vals = unit12_array(seed * 100 + r_i, r)
        # one batch = breaker ops + the run + breaker ops, so that the run is detected in the middle of a batch
        pre_k = np.array([keys0[0], app[0] - 1 if steps[0] > 1 else keys0[-1], keys0[n0 // 2]], dtype=np.int64)
        pre_v = np.array([1.5, 0.0, 0.0 if r_i % 2 else 2.5])
        post_k = np.array([app[-1], app[r // 2], app[-1] + 5, app[-1] + 2], dtype=np.int64)   # update, update, append, descending
        post_v = np.array([9.0, 0.0, 1.0, 2.0])
        top += 5
        ks = np.concatenate([pre_k, app, post_k]); vs = np.concatenate([pre_v, vals, post_v])
        a.set_batch(ks, vs)
        b.set_batch(ks, vs)
        assert_vec_equal(a, b)
        ia, ib = a.info(), b.info()
        for k in ("stat_extends", "stat_shrinks", "stat_rebalances", "stat_window_slots"):
            assert ia[k] == ib[k], (k, r_i, ia, ib)
    rep = a.check()
    assert rep[0] == a.nnz() and not rep[2:7].any(), rep
    q = np.concatenate([keys0[:50], np.arange(top - 200, top + 3, dtype=np.int64)])
    assert np.array_equal(a.get_batch(q), b.get_batch(q))


def test_c2_full_scale_batches(dsa, hip, oracle):
    """BASELINE config 2 at full size: 2^20-slot PMA (700k keys), batch A = 100k ascending appends
    (one 2^20-slot root rebalance + one extend to 2^21), batch B = 100k uniform odd keys."""
    n0 = 700000
    keys0 = np.arange(1, n0 + 1, dtype=np.int64) * 2
    a = dsa.dynamicsparsevec(keys0, unit12_array(3, n0), binding=hip)
    b = dsa.dynamicsparsevec(keys0, unit12_array(3, n0), binding=oracle)
    assert a.info()["capacity"] == 1 << 20 and a.info()["segment_capacity"] == 16 and a.info()["height"] == 16
    app = np.arange(1400001, 1500001, dtype=np.int64)
    va = unit12_array(3, 100000)
    a.set_batch(app, va)
    b.set_batch(app, va)
    assert_vec_equal(a, b)
    ia = a.info()
    assert ia["capacity"] == 1 << 21 and ia["stat_extends"] == 1
    assert ia["stat_window_slots"] == b.info()["stat_window_slots"]
    odd = np.unique(1 + 2 * (splitmix_array(4, 120000) % np.uint64(700000)).astype(np.int64))[:100000]
    rng = np.random.default_rng(4)
    rng.shuffle(odd)
    vb = unit12_array(4, len(odd))
    a.set_batch(odd, vb)
    b.set_batch(odd, vb)
    assert_vec_equal(a, b)
    rep = a.check()                       # device-side invariant checker on the 2^21-slot array
    assert rep[0] == a.nnz() and not rep[2:7].any(), rep


# ---------------------------------------------------------------- PackedCSC / matrix writes
def rand_matrix_ops(seed, nrow, ncol, nops, pzero=0.25):
    g = SplitMix64(seed)
    I, J, V = [], [], []
    for _ in range(nops):
        I.append(1 + g.next() % nrow)
        J.append(1 + g.next() % ncol)
        V.append(0.0 if g.next() % 100 < pzero * 100 else float(1 + g.next() % 9))
    return I, J, V


@pytest.mark.parametrize("seed,nrow,ncol,nnz0,nops", [(11, 40, 60, 1, 2500), (12, 300, 200, 5000, 6000),
                                                      (13, 2000, 3000, 60000, 30000), (14, 7, 5, 10, 800)])
def test_matrix_random_writes_match_oracle(dsa, hip, oracle, seed, nrow, ncol, nnz0, nops):
    I0, J0, V0 = rand_matrix_ops(seed, nrow, ncol, nnz0, pzero=0.0)
    a = dsa.dynamicsparse(I0, J0, V0, binding=hip)
    b = dsa.dynamicsparse(I0, J0, V0, binding=oracle)
    assert_mat_equal(a, b)
    I, J, V = rand_matrix_ops(seed + 100, nrow + 10, ncol + 10, nops)
    a.set_batch(I, J, V)
    b.set_batch(I, J, V)
    assert_mat_equal(a, b)
    L = a.export_layout(0)
    check_semaphores(L["keys"], L["vals"], L["occ"], L["semaphores"])
    check_key_order(L["keys"], L["occ"])
    for o in (0, 1):
        rep = a.check(o)
        assert not rep[2:7].any(), (o, rep)
    q = rand_matrix_ops(seed + 200, nrow + 10, ncol + 10, 1000)
    assert np.array_equal(a.get_batch(q[0], q[1]), b.get_batch(q[0], q[1]))
    assert a.nnz() == b.nnz()
    # column / row deletion (tombstones), then more writes that avoid the documented crash paths
    cols = sorted({1 + (s % ncol) for s in range(3, 40, 7)})
    for c in cols:
        for m_ in (a, b):
            try:
                m_.deletecolumn(c)
            except dsa.DsaArgumentError:
                pass
    assert_mat_equal(a, b)
    x = unit12_array(seed, max(a.size()) + 5)
    ya = a.mul(x[: a.size()[1]])
    yb = b.mul(x[: b.size()[1]])
    np.testing.assert_allclose(ya, yb, rtol=RTOL, atol=0)
    yta = a.mul(x[: a.size()[0]], transpose=True)
    ytb = b.mul(x[: b.size()[0]], transpose=True)
    np.testing.assert_allclose(yta, ytb, rtol=RTOL, atol=0)


def test_matrix_from_empty_streaming_columns_c5_scaled(dsa, hip, oracle):
    """BASELINE config 5 (scaled): stream new columns element by element into an empty matrix,
    SpMV every few hundred columns, compared with the oracle."""
    m_rows, ncols, per = 500, 600, 8
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    g = SplitMix64(11)
    gv = SplitMix64(12)
    x = unit12_array(13, ncols)
    for start in range(0, ncols, 150):
        I, J, V = [], [], []
        for j in range(start + 1, min(start + 150, ncols) + 1):
            rows = set()
            while len(rows) < per:
                rows.add(1 + g.next() % m_rows)
            for r in sorted(rows):
                I.append(r); J.append(j); V.append(gv.unit12())
        a.set_batch(I, J, V)
        b.set_batch(I, J, V)
        assert_mat_equal(a, b)
        ya = a.mul(x[: a.size()[1]])
        yb = b.mul(x[: b.size()[1]])
        np.testing.assert_allclose(ya, yb, rtol=RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["column_at_a_time", "row_at_a_time", "mixed"])
def test_small_matrix_batches_match_oracle(dsa, hip, oracle, shape):
    """Batches of 8..127 writes (a column or a row that arrives on its own, src/matrix.jl:43-62 once per element): the orientation in
    which the writes fall into many partitions runs through the local rounds, the other through its sequencer, side by side
    (mat_apply_sets); mixed batches keep the two sequencers.  State after every batch against the oracle, both orientations."""
    g = SplitMix64(91)
    gv = SplitMix64(92)
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    for step in range(60):
        n = 8 + g.next() % 100
        I, J, V = [], [], []
        if shape == "column_at_a_time":
            j = 1 + step if step % 5 else 1 + g.next() % 40            # a new column, now and then an old one again
            rows = sorted({1 + g.next() % 300 for _ in range(n)})
            I = rows; J = [j] * len(rows)
        elif shape == "row_at_a_time":
            i = 1 + step if step % 4 else 1 + g.next() % 30
            cols = sorted({1 + g.next() % 300 for _ in range(n)})
            J = cols; I = [i] * len(cols)
        else:
            for _ in range(n):
                I.append(1 + g.next() % 25); J.append(1 + g.next() % 25)
        V = [0.0 if gv.next() % 9 == 0 else gv.unit12() for _ in I]     # some deletes (zero writes) among them
        a.set_batch(I, J, V)
        b.set_batch(I, J, V)
        assert_mat_equal(a, b)
    n = a.size()[1]
    x = unit12_array(93, max(n, 1))
    np.testing.assert_allclose(a.mul(x[:n]), b.mul(x[:n]), rtol=RTOL, atol=0)


@pytest.mark.gpu
def test_kbuild_buffers_sized_for_the_upper_bound_then_duplicates_fold(dsa, hip, oracle):
    """K-build allocates tables and slot buffers while its sort runs, for the UPPER bounds (every triple a cell of its own, every key of the
    partition range a partition: csrc/build_host.hip, pma_build_dev) — the exact counts are known only after the sort.  When most triples are
    duplicates, and when the partition keys are few but far apart, the structure ends up far smaller than its buffers: geometry, layout and
    tables must still be the reference's (capacity from the FOLDED count, src/pma.jl:42-55), and the structure must keep working (writes,
    _extend!, product) in buffers it did not size itself."""
    g = np.random.default_rng(2025)
    base_i = g.integers(1, 400, 3000)
    base_j = g.integers(1, 300, 3000) * 100003                     # 300 distinct column keys spread over a range of 3 * 10^7
    I = np.tile(base_i, 40)                                           # every (i, j) forty times: 120 000 triples, <= 3 000 cells
    J = np.tile(base_j, 40)
    V = 1.0 + g.random(len(I))
    perm = g.permutation(len(I))
    I, J, V = I[perm], J[perm], V[perm]
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    assert_mat_equal(a, b)
    for o in (0, 1):
        assert a.info(o)["capacity"] == b.info(o)["capacity"] <= 8192      # (the upper bound would have been 2^18 slots)
    I2 = g.integers(1, 2000, 20000)
    J2 = g.integers(1, 300, 20000) * 100003 + g.integers(0, 2, 20000)
    V2 = np.where(g.random(20000) < 0.2, 0.0, 1.0 + g.random(20000))
    for m_ in (a, b):
        m_.set_batch(I2, J2, V2)
    assert_mat_equal(a, b)
    assert a.info(0)["stat_extends"] == b.info(0)["stat_extends"] >= 1
    x = 1.0 + g.random(a.size()[1])
    np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=RTOL, atol=0)
    # the same through fill mode (closefillmode! -> the same builder on the device-resident buffer)
    c = dsa.dynamicsparse(fill_mode=True, binding=hip)
    d = dsa.dynamicsparse(fill_mode=True, binding=oracle)
    for m_ in (c, d):
        m_.set_batch(I, J, V)
        m_.closefillmode()
    assert_mat_equal(c, d)


@pytest.mark.gpu
def test_column_generation_with_deletions_matches_oracle(dsa, hip, oracle):
    """Column generation with deletions (Coluna's pattern: new columns get new, larger ids while old ones are deleted): batches of new
    columns streamed into a matrix whose colmajor tables hold tombstones.  A batch whose column keys never decrease and start at or
    behind the last LIVE table entry cannot fail, so both orientations are updated side by side (matwrite_host.hip: mat_apply_sets, cannot_fail); deleting
    the last column, writing to an older column, or a deleted row make the batch take the reference's statement order instead — same
    state and same error codes as the oracle either way."""
    m_rows, per, step = 400, 6, 60              # 360 element writes per batch (>= 128: the batch-parallel branch)
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    g = SplitMix64(71)
    gv = SplitMix64(72)

    def both(fn):
        ea = eb = None
        try:
            fn(a)
        except dsa.DsaError as e:
            ea = e.code
        try:
            fn(b)
        except dsa.DsaError as e:
            eb = e.code
        assert ea == eb, (ea, eb)
        return ea

    next_col = 1
    for rnd in range(9):
        I, J, V = [], [], []
        for j in range(next_col, next_col + step):
            rows = set()
            while len(rows) < per:
                rows.add(1 + g.next() % m_rows)
            for r in sorted(rows):
                I.append(r); J.append(j); V.append(gv.unit12())
        if rnd == 2:                            # one write to an older column in front: keys decrease -> the sequential orientation order
            I.insert(0, 7); J.insert(0, next_col - 10); V.insert(0, 3.25)
        if rnd == 4:                            # a zero-valued write creates an (empty) column too: appended like the others
            I.append(3); J.append(next_col + step); V.append(0.0)
        err = both(lambda mtx: mtx.set_batch(I, J, V))
        if err is not None:
            assert rnd == 7, rnd                # the reference's crash path after deleting the LAST column (round 6): same code on both sides;
            return                              # the state behind it is a documented divergence
        assert_mat_equal(a, b)
        next_col += step + (1 if rnd == 4 else 0)
        # deletions between the batches: old columns, sometimes the LAST one (then the next batch must not take the side-by-side branch),
        # once a row (a tombstone in the rowmajor tables)
        for j in range(next_col - step, next_col - 1, 7):
            both(lambda mtx: mtx.deletecolumn(j))
        if rnd == 6:
            both(lambda mtx: mtx.deletecolumn(next_col - 1))
        if rnd == 3:
            both(lambda mtx: mtx.deleterow(11))
        assert_mat_equal(a, b)
        if rnd == 5:
            n = a.size()[1]
            x = unit12_array(73, max(n, 1))
            np.testing.assert_allclose(a.mul(x[:n]), b.mul(x[:n]), rtol=RTOL, atol=0)
    raise AssertionError("the batch behind a deleted last column was expected to take the reference's error path")


@pytest.mark.parametrize("seed,nkeys,batch,span", [(31, 3000, 3000, 10**6), (32, 2500, 700, 5000), (33, 400, 90, 600)])
def test_new_columns_in_random_key_order_deferred_table_inserts(dsa, hip, oracle, seed, nkeys, batch, span):
    """Writes that create rows AND columns in random key order (middle inserts of addpartition!, src/pcsr.jl:114-146): the
    device keeps new partitions at the end of the tables inside a launch and merges them once (more than 1024 new keys
    in a batch: several merges); negative keys, overwrites, deletes of entries, and a deletecolumn! / deleterow! in the
    middle (tombstones: the literal reference path).  Tables, semaphore ids and slot layout must equal the oracle's."""
    g = SplitMix64(seed)
    gv = SplitMix64(seed + 100)
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    done = 0
    while done < nkeys:
        I, J, V = [], [], []
        for _ in range(min(batch, nkeys - done)):
            i = int(g.next() % (2 * span)) - span
            j = int(g.next() % (2 * span)) - span
            if i == 0 or j == 0:
                continue
            v = 0.0 if g.next() % 11 == 0 else gv.unit12()
            I.append(i); J.append(j); V.append(v)
            if g.next() % 3 == 0:                       # a second entry in the same row / column
                I.append(i); J.append(int(g.next() % (2 * span)) - span or 7); V.append(gv.unit12())
        a.set_batch(I, J, V)
        b.set_batch(I, J, V)
        assert_mat_equal(a, b)
        done += batch
    # tombstones: afterwards new keys take the reference's own middle-insert path (reuse of the tombstoned id, or the
    # @assert of src/pcsr.jl:132 — then both sides must fail at the same op with the same code and the same state)
    jdel = next(j for j, v in zip(J, V) if v != 0.0)
    idel = next(i for i, v in zip(I[::-1], V[::-1]) if v != 0.0)
    for m_ in (a, b):
        m_.deletecolumn(jdel)
        m_.deleterow(idel)
    assert_mat_equal(a, b)
    # re-create the deleted column and row (the tombstoned ids are reused, src/pcsr.jl:121-126) and append behind the last keys
    live = [(i, j) for i, j, v in zip(I, J, V) if v != 0.0 and j != jdel and i != idel]
    iex, jex = live[0]
    I = [idel, idel, 5 * span, 5 * span + 1, iex]
    J = [jex, jdel, jdel, 6 * span, jdel]
    V = [gv.unit12() for _ in I]
    for m_ in (a, b):
        m_.set_batch(I, J, V)
    assert_mat_equal(a, b)
    # a new key in front of a tombstone that is not adjacent: the reference's @assert (src/pcsr.jl:132) — same error on both
    # sides (the table state after that crash is a documented divergence, DESIGN.md §4: not compared)
    for m_ in (a, b):
        m_.deletecolumn(jdel)
    I = [int(g.next() % (2 * span)) - span or 3 for _ in range(40)]
    J = [int(g.next() % (2 * span)) - span or 5 for _ in range(40)]
    V = [gv.unit12() for _ in range(40)]
    codes = []
    for m_ in (a, b):
        try:
            m_.set_batch(I, J, V)
            codes.append(0)
        except dsa.DsaError as e:
            codes.append(e.code)
    assert codes[0] == codes[1], codes
    if codes[0] != 0:
        return
    assert_mat_equal(a, b)
    n = a.size()[1]
    if n >= 1:
        x = unit12_array(seed + 5, n)
        np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=RTOL, atol=0)


def test_c5_mid_scale_parallel_column_creation_matches_oracle(dsa, hip, oracle):
    """BASELINE config 5 at 1/5 of full size (20k rows, 6k columns x 16, 96k element writes) in batches of 1000 columns: most
    new rows are created by the batch-parallel rounds (k_plan / k_apply PB_NEWCOL, table entries pending until the sequencer
    merges them), the rest by the sequencer's deferred inserts.  Tables, ids, slot layout and SpMV vs the oracle after every batch."""
    import bench
    m_rows, ncols, per, every = 20_000, 6_000, 16, 1000
    I, J, V = bench.c5_columns(m_rows, ncols, per)
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    x = unit12_array(13, ncols)
    for c0 in range(0, ncols, every):
        sl = slice(c0 * per, (c0 + every) * per)
        a.set_batch(I[sl], J[sl], V[sl])
        b.set_batch(I[sl], J[sl], V[sl])
        assert_mat_equal(a, b)
    st = a.info(dsa.ROWMAJOR)
    assert st["stat_par_ops"] > 20_000, st            # the parallel path really created rows
    np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=RTOL, atol=0)
    np.testing.assert_allclose(a.mul(unit12_array(14, m_rows), transpose=True), b.mul(unit12_array(14, m_rows), transpose=True), rtol=RTOL, atol=0)


@pytest.mark.parametrize("seed", [41, 42, 43, 44, 45, 46])
def test_parallel_column_creation_stress(dsa, hip, oracle, seed):
    """Randomised mixes around the batch-parallel creation of rows / columns: batches of random (i, j, v) over a key space that
    keeps producing new keys, a varying share of deletes (sparser windows -> other rebalance levels), dense rows, and batches
    small enough for the plain sequencer in between.  Layout and tables vs the oracle after every batch."""
    g = SplitMix64(seed)
    gv = SplitMix64(seed + 500)
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    span_i = [400, 3000, 20000][seed % 3]
    span_j = [5000, 700, 20000][seed % 3]
    live = []
    for step in range(14):
        nb = [900, 60, 2500, 300, 1500][step % 5]
        del_share = [0, 5, 2, 9, 3][(step + seed) % 5]
        I, J, V = [], [], []
        for _ in range(nb):
            r = g.next() % 10
            if r < del_share and live:
                i, j = live[g.next() % len(live)]
                I.append(i); J.append(j); V.append(0.0)
            elif r == 9 and live:                          # grow one row into a long one
                i, _ = live[g.next() % len(live)]
                j = 1 + int(g.next() % span_j)
                I.append(i); J.append(j); V.append(gv.unit12()); live.append((i, j))
            else:
                i = 1 + int(g.next() % span_i); j = 1 + int(g.next() % span_j)
                I.append(i); J.append(j); V.append(gv.unit12()); live.append((i, j))
        a.set_batch(I, J, V)
        b.set_batch(I, J, V)
        assert_mat_equal(a, b)
    n = a.size()[1]
    x = unit12_array(seed + 7, n)
    np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=RTOL, atol=0)


def _column_run(g, gv, cols, m_rows, per_lo, per_hi):
    """(I, J, V) for the given new columns: rows ascending inside each column (an append run of the colmajor orientation)."""
    I, J, V = [], [], []
    for j in cols:
        per = per_lo + g.next() % (per_hi - per_lo + 1)
        rows = set()
        while len(rows) < per:
            rows.add(1 + g.next() % m_rows)
        for r in sorted(rows):
            I.append(r); J.append(j); V.append(gv.unit12())
    return I, J, V


@pytest.mark.parametrize("seed,m_rows,per_lo,per_hi,batches", [(21, 300, 1, 1, [70, 200, 64, 500]), (22, 50, 1, 12, [100, 400, 30, 1500]),
                                                              (23, 5000, 16, 16, [500, 500, 2000]), (24, 40, 3, 30, [10, 90, 90, 700])])
def test_matrix_column_append_runs_match_oracle(dsa, hip, oracle, seed, m_rows, per_lo, per_hi, batches):
    """Column streaming (Coluna pattern): every batch appends new columns in (col, row) order -> the colmajor orientation takes
    the bitmap-only append-run path including the semaphore cells of the new partitions; the rowmajor orientation takes the
    general path.  Starts from an empty matrix, runs through several _extend!s and table growths; between the runs, ops that
    must not be swallowed by a run: a write into an older column, an update of an existing cell, a delete, a repeated row."""
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    g, gv = SplitMix64(seed), SplitMix64(seed + 100)
    nxt = 1
    for bi, nb in enumerate(batches):
        I, J, V = _column_run(g, gv, range(nxt, nxt + nb), m_rows, per_lo, per_hi)
        nxt += nb
        if bi >= 1:
            # breakers in the middle of the batch: older column, update, delete, duplicate row in the current column
            k = len(I) // 2
            I[k:k] = [1 + g.next() % m_rows, I[0], I[1], I[k - 1]]
            J[k:k] = [1, J[0], J[1], J[k - 1]]
            V[k:k] = [4.25, 7.5, 0.0, 8.125]
        a.set_batch(I, J, V)
        b.set_batch(I, J, V)
        assert_mat_equal(a, b)
        for o in (0, 1):
            ia, ib = a.info(o), b.info(o)
            for key in ("stat_extends", "stat_rebalances", "stat_window_slots"):
                assert ia[key] == ib[key], (o, key, bi)
    # the batch continues the last existing column before opening new ones
    last_rows = [m_rows + 1, m_rows + 2, m_rows + 5]
    I, J, V = _column_run(g, gv, range(nxt, nxt + 80), m_rows, per_lo, per_hi)
    I = last_rows + I; J = [nxt - 1] * 3 + J; V = [1.0, 2.0, 3.0] + V
    a.set_batch(I, J, V); b.set_batch(I, J, V)
    assert_mat_equal(a, b)
    nxt += 80
    rep = a.check(0)
    assert not rep[2:7].any(), rep
    x = unit12_array(seed, a.size()[1])
    np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=RTOL, atol=0)
    # a tombstone at the end of the table: no run; the reference's addcolumn! stores the key in the tombstoned slot and
    # addpartition! then throws (no semaphore follows, src/pcsr.jl:121-123) — same error, same state afterwards
    a.deletecolumn(nxt - 1); b.deletecolumn(nxt - 1)
    I, J, V = _column_run(g, gv, range(nxt, nxt + 70), m_rows, per_lo, per_hi)
    errs = []
    for m_ in (a, b):
        try:
            m_.set_batch(I, J, V)
            errs.append(None)
        except dsa.DsaError as e:
            errs.append(e.code)
    assert errs[0] == errs[1]
    assert_mat_equal(a, b)


def test_matrix_row_append_runs_and_negative_rows_match_oracle(dsa, hip, oracle):
    """Rows streamed in (row, col) order make the ROWMAJOR orientation the append run; rows <= 0 never enter a run
    (the semaphore key is 0) but must still match."""
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    g, gv = SplitMix64(31), SplitMix64(32)
    J, I, V = _column_run(g, gv, range(1, 301), 200, 2, 9)          # transposed roles: "columns" are rows here
    a.set_batch(I, J, V); b.set_batch(I, J, V)
    assert_mat_equal(a, b)
    I2, J2, V2 = [], [], []
    for j in range(400, 500):
        for r in (-5, -2, 3, 9):
            I2.append(r); J2.append(j); V2.append(gv.unit12())
    a.set_batch(I2, J2, V2); b.set_batch(I2, J2, V2)
    assert_mat_equal(a, b)


def test_error_codes_match_reference_sites(dsa, hip):
    a = dsa.dynamicsparse([1, 2], [1, 2], [1.0, 2.0], binding=hip)
    with pytest.raises(dsa.DsaArgumentError):
        a.deletecolumn(99)                      # src/pcsr.jl:208
    with pytest.raises(dsa.DsaArgumentError):
        a[0, 1] = 1.0                           # reserved semaphore key
    with pytest.raises(dsa.DsaErrorException):
        a.closefillmode()                       # src/matrix.jl:127
    p = dsa.packedcsc([[1, 2], [3]], [[1.0, 2.0], [3.0]], binding=hip)
    p.deletepartition(1)
    with pytest.raises(dsa.DsaErrorException) as ei:
        p[1, 1] = 5.0                           # src/pcsr.jl:299
    assert ei.value.code == dsa.binding.EDELETED
    with pytest.raises(dsa.DsaBoundsError):
        p.deletepartition(7)                    # src/pcsr.jl:190


@pytest.mark.parametrize("pad", [0, 300])
def test_state_after_a_failed_batch_is_the_references(dsa, hip, oracle, pad):
    """src/matrix.jl:43-62 writes colmajor, then rowmajor: when write k of a batch throws, both orientations hold writes [0, k) and colmajor
    also holds write k if it was the rowmajor statement that threw.  Until round 6 the library ran the colmajor half of the batch first and
    could hold writes BEHIND k.  Crash paths of addpartition!(pcsc, prev) (src/pcsr.jl:114-146) provoked in the rowmajor
    table, in the colmajor table, by both kinds of error, with writes queued behind the failing one; `pad` harmless writes in front push the
    batch onto the batch-parallel path.  Compared: status, size(m), and the orientation that did not refuse slot for slot."""
    rng = np.random.default_rng(3 + pad)
    keys = np.arange(1, 51, dtype=np.int64) * 3                       # rows / columns 3, 6, ..., 150
    I0 = np.repeat(keys, 4); J0 = rng.choice(keys, len(I0))
    V0 = rng.integers(1, 9, len(I0)).astype(np.float64)

    def fresh(deleted_rows=(), deleted_cols=()):
        ms = [dsa.dynamicsparse(I0, J0, V0, binding=b) for b in (hip, oracle)]
        for m in ms:
            for r in deleted_rows:
                m.deleterow(r)
            for c in deleted_cols:
                m.deletecolumn(c)
        assert_mat_equal(*ms)
        return ms

    def run(ms, I, J, V, failing):
        """failing: 1 = rowmajor refuses (colmajor must be the reference's), 0 = colmajor refuses, None = the batch succeeds"""
        padI = rng.choice(keys[keys < 60], pad); padJ = rng.choice(keys[keys < 60], pad)          # existing rows / columns in front of every tombstone
        I = np.concatenate([padI, np.asarray(I, dtype=np.int64)]); J = np.concatenate([padJ, np.asarray(J, dtype=np.int64)])
        V = np.concatenate([np.full(pad, 2.5), np.asarray(V, dtype=np.float64)])
        codes = []
        for m in ms:
            try:
                m.set_batch(I, J, V); codes.append(None)
            except dsa.DsaError as e:
                codes.append(e.code)
        assert codes[0] == codes[1], codes
        assert ms[0].size() == ms[1].size()
        if failing is None:
            assert codes[0] is None
            assert_mat_equal(*ms)
        else:
            assert codes[0] is not None
            assert orientation_equal(ms[0], ms[1], 1 - failing), ("the orientation that did not refuse the write differs", failing)
        return codes[0]

    # rowmajor asserts (new row 31 in front of live row 33 while row 105 is a tombstone further up); writes behind it must not reach colmajor
    e = run(fresh(deleted_rows=(60, 105)), [6, 9, 31, 12, 200, 15], [3, 6, 9, 12, 15, 18], [1.5, 0.0, 2.5, 3.5, 4.5, 5.5], failing=1)
    assert e == dsa.binding.EASSERT
    # rowmajor BoundsError: the last row is a tombstone and a larger row key arrives (reuse branch, semaphores[0])
    e = run(fresh(deleted_rows=(150,)), [6, 151, 9, 12], [3, 6, 9, 999], [1.5, 2.5, 3.5, 4.5], failing=1)
    assert e == dsa.binding.EBOUNDS
    # a tombstone reused (row 59 lands on the id of row 60), a re-created row, then the assert two writes later
    e = run(fresh(deleted_rows=(60, 105, 120)), [59, 6, 31, 9], [3, 9, 12, 15], [1.5, 3.5, 4.5, 5.5], failing=1)
    assert e == dsa.binding.EASSERT
    # both tombstones taken again (59 on the id of 60, 105 re-created): row 31 then shifts a table without tombstones
    run(fresh(deleted_rows=(60, 105)), [59, 105, 6, 31, 9], [3, 6, 9, 12, 15], [1.5, 2.5, 3.5, 4.5, 5.5], failing=None)
    # the same batch without the failing write succeeds
    run(fresh(deleted_rows=(60, 105)), [59, 105, 6, 9], [3, 6, 9, 15], [1.5, 2.5, 3.5, 5.5], failing=None)
    # colmajor refuses (new column 31): rowmajor holds the writes in front of it only
    e = run(fresh(deleted_cols=(60, 105)), [3, 6, 9, 12], [6, 31, 9, 12], [1.5, 2.5, 3.5, 4.5], failing=0)
    assert e == dsa.binding.EASSERT
    # tombstones in BOTH tables: rowmajor refuses write 2, colmajor would have refused write 4
    e = run(fresh(deleted_rows=(60, 105), deleted_cols=(60, 105)), [6, 9, 31, 12, 15], [3, 6, 9, 12, 31], [1.5, 2.5, 3.5, 4.5, 5.5], failing=1)
    assert e == dsa.binding.EASSERT
    # ... and the other way round: colmajor refuses write 1, rowmajor would have refused write 3
    e = run(fresh(deleted_rows=(60, 105), deleted_cols=(60, 105)), [6, 9, 12, 31], [3, 31, 9, 12], [1.5, 2.5, 3.5, 4.5], failing=0)
    assert e == dsa.binding.EASSERT


# ---------------------------------------------------------------- SpMV
@pytest.mark.parametrize("force", [None, "0", "1"])
def test_sparse_x_product_two_step_and_device_entry_points(dsa, hip, oracle, force):
    """the product Coluna calls (_mul + _mul_output, src/operations.jl:11-12,107-135).  dsa_mat_spmv_sparse_begin / _fetch (one
    product whatever the result size) and dsa_mat_spmv_sparse_dev (xi / xv in, yi / yv / count out, all HBM) against the oracle's Dict
    accumulator: touched rows identical — stored zeros of x and cancelling sums kept —, values within 1e-12; both strategies (driven by
    x's entries / gather over the twin + pattern pass, forced through the development switch in child processes), both transposes, results
    above and below the pinned landing area, repeated products on the same handle (the zero invariant of the accumulator), a negative
    column key, tombstones."""
    if force is not None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, DSA_DEV="1", DSA_SPX_XDRIVEN=force)
        r = _run_child([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_hip_parity.py"), "-m", "gpu", "-x", "-q", "-k",
                        "two_step_and_device_entry_points and None"], env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        return
    import torch
    m, n, per = 30000, 20000, 6
    rows = 1 + (splitmix_array(11, n * per) % np.uint64(m)).astype(np.int64)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per)
    vals = (1 + splitmix_array(12, n * per) % np.uint64(9)).astype(np.float64)
    vals[::7] *= -1.0                                              # cancelling sums: a touched row may sum to exactly 0
    a = dsa.dynamicsparse(rows, cols, vals, m, n, binding=hip)
    b = dsa.dynamicsparse(rows, cols, vals, m, n, binding=oracle)
    for mm in (a, b):
        mm.deletecolumn(17); mm.deleterow(23)                      # tombstones in both tables
    dev = torch.device("cuda")
    d_yi = torch.empty(max(m, n), dtype=torch.int64, device=dev); d_yv = torch.empty(max(m, n), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    for rep in range(2):
        for cnt in (1, 40, 700, 2600, 9000, n):
            xi = np.unique(1 + (splitmix_array(100 + cnt + rep, cnt) % np.uint64(n)).astype(np.int64))
            xv = unit12_array(7 + rep, len(xi))
            xv[::5] = 0.0                                          # stored zeros of x still touch their rows (src/operations.jl:101)
            for tr in (False, True):
                xi3 = xi if not tr else xi[xi <= m]
                xv3 = xv[: len(xi3)]
                ib, vb = b.mul((xi3, xv3), transpose=tr)
                ia, va = a.mul((xi3, xv3), transpose=tr)           # _begin + _fetch
                assert np.array_equal(ia, ib), (cnt, tr, len(ia), len(ib))
                # (atol=1e-13 is not derived from anything: x is unit12, not exactly summable, so the bound stays as it was.  The exact
                # comparisons — inputs that sum to the same bits in any order — are in tests/test_sparse_x.py.)
                np.testing.assert_allclose(va, vb, rtol=RTOL, atol=1e-13)
                d_xi = torch.from_numpy(xi3).to(dev); d_xv = torch.from_numpy(xv3).to(dev)
                a.mul_dev(d_xi.data_ptr(), d_xv.data_ptr(), len(xi3), d_yi.data_ptr(), d_yv.data_ptr(), d_yi.numel(), d_cnt.data_ptr(), transpose=tr)
                a.sync()
                k = int(d_cnt.item())
                assert k == len(ib)
                assert np.array_equal(d_yi[:k].cpu().numpy(), ib)
                np.testing.assert_allclose(d_yv[:k].cpu().numpy(), vb, rtol=RTOL, atol=1e-13)
                # a result buffer that is too small: the count still says how much, the pairs that fit are the first ones
                if k > 10:
                    a.mul_dev(d_xi.data_ptr(), d_xv.data_ptr(), len(xi3), d_yi.data_ptr(), d_yv.data_ptr(), 10, d_cnt.data_ptr(), transpose=tr)
                    a.sync()
                    assert int(d_cnt.item()) == k and np.array_equal(d_yi[:10].cpu().numpy(), ib[:10])
    # a column key below 1 (test/functional/sparsematrix.jl:251): only the kernel driven by x's entries can address it — also when
    # nearly every column is stored
    a2 = dsa.dynamicsparse(rows[:6000], cols[:6000], vals[:6000], m, n, binding=hip)
    b2 = dsa.dynamicsparse(rows[:6000], cols[:6000], vals[:6000], m, n, binding=oracle)
    for mm in (a2, b2):
        mm[5, -3] = 2.0
    for xi in ([-3, 5], np.concatenate([[-3], np.arange(1, n + 1, dtype=np.int64)])):
        xv = unit12_array(3, len(xi))
        ia, va = a2.mul((xi, xv)); ib, vb = b2.mul((xi, xv))
        assert np.array_equal(ia, ib) and np.allclose(va, vb, rtol=RTOL, atol=1e-13)
    # the one-shot entry point with a buffer that is too small reports DSA_ECAP and the size; the result stays fetchable
    import ctypes as C
    xi = np.arange(1, 2001, dtype=np.int64); xv = np.ones(2000)
    yi = np.empty(4, dtype=np.int64); yv = np.empty(4); k = C.c_int64()
    P_I64, P_F64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    with pytest.raises(dsa.DsaError) as ei:
        hip.call("mat_spmv_sparse", a.h, 0, xi.ctypes.data_as(P_I64), xv.ctypes.data_as(P_F64), 2000, yi.ctypes.data_as(P_I64), yv.ctypes.data_as(P_F64), 4, C.byref(k))
    assert ei.value.code == dsa.binding.ECAP and k.value > 4
    yi = np.empty(k.value, dtype=np.int64); yv = np.empty(k.value)
    hip.call("mat_spmv_sparse_fetch", a.h, yi.ctypes.data_as(P_I64), yv.ctypes.data_as(P_F64), k.value, C.byref(k))
    ib, vb = b.mul((xi, xv))
    assert np.array_equal(yi, ib) and np.allclose(yv, vb, rtol=RTOL, atol=1e-13)
    assert_mat_equal(a, b)


@pytest.mark.parametrize("m,n,per_col,seed", [(50, 40, 3, 1), (3000, 2500, 7, 2), (100000, 80000, 10, 3), (64, 100000, 2, 4)])
def test_spmv_matches_oracle(dsa, hip, oracle, m, n, per_col, seed):
    rows = 1 + (splitmix_array(seed, n * per_col) % np.uint64(m)).astype(np.int64)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per_col)
    # integer-valued floats: duplicate (i,j) fold order is irrelevant
    vals = (1 + splitmix_array(seed + 1, n * per_col) % np.uint64(9)).astype(np.float64)
    a = dsa.dynamicsparse(rows, cols, vals, m, n, binding=hip)
    b = dsa.dynamicsparse(rows, cols, vals, m, n, binding=oracle)
    assert_mat_equal(a, b)
    x = unit12_array(seed + 2, max(m, n))
    for transpose, nx in ((False, n), (True, m)):
        ya = a.mul(x[:nx], transpose=transpose)
        yb = b.mul(x[:nx], transpose=transpose)
        np.testing.assert_allclose(ya, yb, rtol=RTOL, atol=0)
    # sparse x: touched-row pattern and values
    xi = np.unique(1 + (splitmix_array(seed + 3, 200) % np.uint64(n)).astype(np.int64))
    xv = unit12_array(seed + 4, len(xi))
    ia, va = a.mul((xi, xv))
    ib, vb = b.mul((xi, xv))
    assert np.array_equal(ia, ib)
    np.testing.assert_allclose(va, vb, rtol=RTOL, atol=0)
    # a few entries only (x-driven kernel) and nearly all of them (densify + pattern pass), both transposes
    for cnt in (3, max(3, (7 * n) // 8)):
        xi2 = np.unique(1 + (splitmix_array(seed + 5, cnt) % np.uint64(n)).astype(np.int64))
        xv2 = unit12_array(seed + 6, len(xi2))
        for tr in (False, True):
            xi3 = xi2 if not tr else xi2[xi2 <= m]
            ia, va = a.mul((xi3, xv2[: len(xi3)]), transpose=tr)
            ib, vb = b.mul((xi3, xv2[: len(xi3)]), transpose=tr)
            assert np.array_equal(ia, ib), (cnt, tr)
            np.testing.assert_allclose(va, vb, rtol=RTOL, atol=0)


def test_spmv_long_rows_and_tile_straddling(dsa, hip, oracle):
    """A few very long rows (thousands of cells: many 2048-slot tiles per row) next to short ones."""
    n = 30000
    I = np.concatenate([np.full(n, 1), np.full(n // 2, 2), np.arange(3, 3 + 2000), np.full(n, 9000)])
    J = np.concatenate([np.arange(1, n + 1), np.arange(1, n + 1, 2), np.arange(1, 2001), np.arange(1, n + 1)])
    V = unit12_array(21, len(I))
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    assert_mat_equal(a, b)
    x = unit12_array(22, n)
    np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=RTOL, atol=0)
    np.testing.assert_allclose(a.mul(x[:9000], transpose=True), b.mul(x[:9000], transpose=True), rtol=RTOL, atol=0)


def test_spmv_device_pointers_gather_and_scatter(dsa, hip, oracle):
    import ctypes as C
    import torch
    m, n, per = 20000, 15000, 6
    rows = 1 + (splitmix_array(5, n * per) % np.uint64(m)).astype(np.int64)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per)
    vals = (1 + splitmix_array(6, n * per) % np.uint64(9)).astype(np.float64)
    a = dsa.dynamicsparse(rows, cols, vals, m, n, binding=hip)
    b = dsa.dynamicsparse(rows, cols, vals, m, n, binding=oracle)
    x = unit12_array(7, max(m, n))
    dev = torch.device("cuda:0")
    hip.call("mat_set_stream", a.h, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for transpose, nx, ny in ((0, n, m), (1, m, n)):
        xd = torch.from_numpy(x[:nx].copy()).to(dev)
        ref = b.mul(x[:nx], transpose=bool(transpose))
        for algo in (0, 1):
            yd = torch.full((ny,), 7.0, dtype=torch.float64, device=dev)
            hip.call("mat_spmv_dense_dev", a.h, transpose, algo, C.c_void_p(xd.data_ptr()), nx, C.c_void_p(yd.data_ptr()), ny)
            torch.cuda.synchronize()
            np.testing.assert_allclose(yd.cpu().numpy(), ref, rtol=RTOL, atol=0)


def test_rebalance_from_skewed_sources_and_extend_shrink(dsa, hip, oracle):
    """The root pack + spread only depends on the ORDER and NUMBER of the cells (src/moves.jl:94-171): from a source packed to
    the left (pack!), packed to the right (all gaps at the left) or uniformly spread, the single-launch rebalance must
    produce the same slots as the oracle's layout; _extend! / _shrink! (src/pma.jl:143-161) round-trip to it as well."""
    for n in (5, 90, 3000, 46000, 300000):
        keys = np.arange(1, n + 1, dtype=np.int64) * 7 - 3
        vals = unit12_array(30 + n % 7, n)
        a = dsa.dynamicsparsevec(keys, vals, binding=hip)
        b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
        ref = b.export_layout()
        for mode in (1, 2):
            hip.call("vec_dev_relayout", a.h, mode)
            k, v, o = a.export_layout()
            assert int(o.sum()) == n
            occ = o.astype(bool)
            pos = np.nonzero(occ)[0]
            assert (pos[0] == 0 and pos[-1] == n - 1) if mode == 1 else (pos[0] == len(o) - n and pos[-1] == len(o) - 1)
            np.testing.assert_array_equal(k[occ], keys)
            a.rebalance_root()
            got = a.export_layout()
            for x, y in zip(got, ref):
                np.testing.assert_array_equal(x, y)
        cap = a.info()["capacity"]
        hip.call("vec_dev_relayout", a.h, 3)                      # _extend!: capacity doubles, cells spread over it
        assert a.info()["capacity"] == 2 * cap and a.info()["height"] == b.info()["height"] + 1
        k, v, o = a.export_layout()
        np.testing.assert_array_equal(k[o.astype(bool)], keys)
        np.testing.assert_array_equal(v[o.astype(bool)], vals)
        assert not a.check()[2:7].any()
        hip.call("vec_dev_relayout", a.h, 4)                      # _shrink!: back to the reference layout
        got = a.export_layout()
        for x, y in zip(got, ref):
            np.testing.assert_array_equal(x, y)
        assert a.info()["capacity"] == cap


def test_spmv_without_memset_and_its_fallbacks(dsa, hip, oracle):
    """The gather SpMV skips the memset of y when every row is written exactly once by the kernel:
    rows without a partition are zeroed by the owner of the next partition.  y is pre-filled with NaN; the path
    actually taken is read from the `stat_spmv_nomemset` counter.  Fallbacks to the memset: a partition longer than a
    span (fp64 atomics join its parts), tombstones, wide key gaps."""
    import ctypes as C
    import torch
    dev = torch.device("cuda:0")
    m, n, per = 30000, 9000, 5
    rows = 1 + (splitmix_array(15, n * per) % np.uint64(m)).astype(np.int64)
    rows[rows % 7 == 3] += 1                                   # rows = 3 (mod 7) never occur: gaps of one key everywhere
    rows = np.minimum(rows, m - 40)                            # and the last 40 rows stay empty (tail fill)
    rows[rows < 6] = 6                                         # and the first 5 (head fill)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per)
    vals = unit12_array(16, n * per)
    a = dsa.dynamicsparse(rows, cols, vals, m, n, binding=hip)
    b = dsa.dynamicsparse(rows, cols, vals, m, n, binding=oracle)
    hip.call("mat_set_stream", a.h, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    x = unit12_array(17, max(m, n))

    def check(expect_nomemset):
        for transpose, nx, ny, o in ((0, n, m, 1), (1, m, n, 0)):
            before = a.info(o)["stat_spmv_nomemset"]
            xd = torch.from_numpy(x[:nx].copy()).to(dev)
            yd = torch.full((ny,), float("nan"), dtype=torch.float64, device=dev)
            hip.call("mat_spmv_dense_dev", a.h, transpose, 0, C.c_void_p(xd.data_ptr()), nx, C.c_void_p(yd.data_ptr()), ny)
            torch.cuda.synchronize()
            ref = b.mul(x[:nx], transpose=bool(transpose))
            np.testing.assert_allclose(yd.cpu().numpy(), ref, rtol=RTOL, atol=0)
            took = a.info(o)["stat_spmv_nomemset"] - before
            if expect_nomemset is not None:
                assert took == (1 if expect_nomemset[transpose] else 0), (transpose, took)

    check({0: True, 1: True})
    # a batch of writes keeps the property (and invalidates the cached meta: new rows 3 (mod 7) appear)
    I2 = np.arange(3, 3 + 7 * 500, 7, dtype=np.int64)
    J2 = 1 + (splitmix_array(18, len(I2)) % np.uint64(n)).astype(np.int64)
    V2 = unit12_array(19, len(I2))
    for mat in (a, b):
        mat.set_batch(I2, J2, V2)
    check({0: True, 1: True})
    # one row longer than a span (600 cells): its parts are joined by atomics, so y must be zeroed in front
    I3 = np.full(600, 77, dtype=np.int64)
    J3 = np.arange(1, 601, dtype=np.int64) * 13
    for mat in (a, b):
        mat.set_batch(I3, J3, unit12_array(20, 600))
    check({0: False, 1: True})
    # a tombstone in the column table (deletecolumn!) and, through it, in no row: only the colmajor side falls back
    for mat in (a, b):
        mat.deletecolumn(4000)
    check({0: False, 1: False})


def test_spmv_without_memset_sparse_rows_fall_back(dsa, hip, oracle):
    """Row keys 10 000 apart: zero-filling the gaps inside the kernel would serialise on single lanes -> memset path."""
    rows = np.arange(1, 41, dtype=np.int64) * 10000
    I = np.repeat(rows, 3)
    J = np.tile(np.array([1, 2, 3], dtype=np.int64), 40)
    V = unit12_array(21, len(I))
    a = dsa.dynamicsparse(I, J, V, 400000, 3, binding=hip)
    b = dsa.dynamicsparse(I, J, V, 400000, 3, binding=oracle)
    x = np.array([1.0, 2.0, 3.0])
    before = a.info(1)["stat_spmv_nomemset"]
    np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=RTOL, atol=0)
    assert a.info(1)["stat_spmv_nomemset"] == before
    np.testing.assert_allclose(a.mul(np.ones(400000), transpose=True), b.mul(np.ones(400000), transpose=True), rtol=RTOL, atol=0)


def test_column_shard_device_path_single_rank(dsa, hip, oracle):
    """The class bench.py drives on N GPUs, here with world = 1 on the one GPU of the box: x and y stay CUDA tensors, the
    partial product goes through dsa_shard_spmv_dev on torch's stream, every schedule is the identity."""
    import torch
    from dsa_amd import sharding
    m, n, per = 5000, 3000, 7
    rows = 1 + (splitmix_array(23, n * per) % np.uint64(m)).astype(np.int64)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per)
    vals = unit12_array(24, n * per)
    sh = sharding.ColumnShard(dsa, rows, cols, vals, m, n, 0, 1, binding=hip)
    assert sh.device.type == "cuda"
    x = unit12_array(25, n)
    ref = dsa.dynamicsparse(rows, cols, vals, m, n, binding=oracle).mul(x)
    xs = sh.x_slice(x)
    for sched in sharding.SCHEDULES:
        y = torch.full((m,), float("nan"), dtype=torch.float64, device=sh.device)
        sh.spmv(xs, y, schedule=sched)
        torch.cuda.synchronize()
        np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=RTOL, atol=0)


def test_abi_communicator_world_1_rccl_smoke(dsa, hip, oracle):
    """The collective behind the C ABI (include/dsa.h: dsa_comm_*, csrc/comm.hip) with ONE rank on the one GPU of the box: librccl is
    bound at run time, ncclGetUniqueId / ncclCommInitRank / ncclAllReduce(ncclDouble, ncclSum) really run (a single-rank all-reduce
    is the identity), dsa_shard_spmv_allreduce_dev = local product + that all-reduce on the shard's stream; and the communicator
    without RCCL (id == NULL) a single-GPU host gets.  More ranks cannot be tried here: the pool hands out one GPU."""
    import ctypes as C
    import torch
    from dsa_amd import sharding
    m, n, per = 4000, 2500, 6
    rows = 1 + (splitmix_array(61, n * per) % np.uint64(m)).astype(np.int64)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per)
    vals = unit12_array(62, n * per)
    x = unit12_array(63, n)
    ref = dsa.dynamicsparse(rows, cols, vals, m, n, binding=oracle).mul(x)
    for with_rccl in (True, False):
        comm = sharding.AbiComm(hip, 0, 1, with_rccl=with_rccl)
        r, w = C.c_int32(-1), C.c_int32(-1)
        hip.call("comm_info", comm.h, C.byref(r), C.byref(w))
        assert (r.value, w.value) == (0, 1)
        sh = sharding.ColumnShard(dsa, rows, cols, vals, m, n, 0, 1, binding=hip, comm=comm)
        xs = sh.x_slice(x)
        y = torch.full((m,), float("nan"), dtype=torch.float64, device=sh.device)
        sh.spmv(xs, y)                                      # spmv_partial + reduce through dsa_shard_allreduce_dev
        torch.cuda.synchronize()
        np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=RTOL, atol=0)
        y2 = torch.full((m,), float("nan"), dtype=torch.float64, device=sh.device)
        hip.call("shard_spmv_allreduce_dev", sh.A.h, comm.h, C.c_void_p(xs.data_ptr()), n, C.c_void_p(y2.data_ptr()), m)
        hip.call("mat_sync", sh.A.h)
        torch.cuda.synchronize()
        np.testing.assert_allclose(y2.cpu().numpy(), ref, rtol=RTOL, atol=0)
        del sh
        comm.close()
    with pytest.raises(dsa.DsaError):
        sharding.AbiComm.__new__(sharding.AbiComm)           # placeholder object; the next line is the real check
        h = C.c_void_p()
        hip.call("comm_init", 1, 2, None, C.byref(h))          # two ranks need an id


def test_c3_scale_build_and_spmv_properties(dsa, hip):
    """BASELINE config 3 at a quarter of full size on the GPU alone (the oracle needs tens of seconds
    there): size-independent properties — capacity rule, sorted partitions, semaphore table,
    linearity of SpMV, A x vs A' (checksum identity  1' (A x) == (A' 1)' x)."""
    m = n = 250000
    per = 10
    rows = 1 + (splitmix_array(5, n * per) % np.uint64(m)).astype(np.int64)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per)
    vals = unit12_array(6, n * per)
    key = cols * (m + 1) + rows
    _, first = np.unique(key, return_index=True)          # duplicate-free
    rows, cols, vals = rows[first], cols[first], vals[first]
    a = dsa.dynamicsparse(rows, cols, vals, m, n, binding=hip)
    for o in (0, 1):
        L = a.export_layout(o)
        nelem = len(rows) + L["info"]["nb_partitions"]
        assert L["info"]["nb_elements"] == nelem
        assert L["info"]["capacity"] == 1 << int(np.ceil(np.log2(np.ceil(nelem / 0.7))))
        assert int(L["occ"].sum()) == nelem
        occ = L["occ"].astype(bool)
        k = L["keys"][occ]
        sem = k == 0
        assert int(sem.sum()) == L["info"]["nb_partitions"]
        pos = np.nonzero(occ)[0] + 1
        assert np.array_equal(pos[sem], L["semaphores"])            # table <-> slots
        assert np.array_equal(L["vals"][occ][sem], np.arange(1, sem.sum() + 1, dtype=np.float64))
        d = np.diff(k)
        assert np.all((d > 0) | sem[1:] | sem[:-1])                 # ascending keys inside partitions
        assert np.all(np.diff(L["col_keys"]) > 0)
    x1 = unit12_array(7, n)
    x2 = unit12_array(8, n)
    y1, y2, y12 = a.mul(x1), a.mul(x2), a.mul(x1 + 2.0 * x2)
    np.testing.assert_allclose(y12, y1 + 2.0 * y2, rtol=1e-11, atol=0)
    ones = np.ones(m)
    colsum = a.mul(ones, transpose=True)
    assert abs(y1.sum() - colsum @ x1) <= 1e-10 * abs(y1.sum())
    # independent value check with scipy on the same triplets
    import scipy.sparse as sp
    A = sp.csr_matrix((vals, (rows - 1, cols - 1)), shape=(m, n))
    np.testing.assert_allclose(y1, A @ x1, rtol=1e-12, atol=0)


def test_parallel_batches_share_occupancy_words(dsa, hip, oracle):
    """DESIGN §3.2b invariant (I2): many writes of ONE batch land in the same 64-slot occupancy words — small arrays, dense key
    ranges — so that k_apply waves on different XCDs update bits of the same word in the same launch; slot layout vs the oracle
    and the device invariant checker after every batch (the scenario of tools/fuzz.py::run_shared_words)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz
    for seed in range(4005, 4005 + 8 * 12, 8):
        assert fuzz.run_shared_words(seed) == "ok"


def test_c3_full_size_build_spmv_checker_and_rebalance_idempotence(dsa, hip, oracle):
    """BASELINE config 3 at FULL size (1M x 1M, exactly 10M nnz, the matrix bench.py times): bulk build of both orientations
    compared SLOT FOR SLOT with the CPU oracle's build of the same triples (2 x 2^24 slots: keys, value bits, occupancy, scalars,
    semaphore and column-key tables; ~3 s of oracle time), the device-side invariant checker, y = A x and y = A' x against the
    oracle's products and scipy on the same triplets (1e-12), the capacity rule, and the root pack + spread of both orientations
    leaving every slot where the oracle has it (idempotence of _even_rebalance! on an even layout)."""
    import scipy.sparse as sp
    import bench
    m = n = 1_000_000
    I, J, V = bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6)
    assert len(I) == 10_000_000
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    b = dsa.dynamicsparse(I, J, V, m, n, binding=oracle)
    assert_mat_equal(a, b)
    A = sp.csr_matrix((V, (I - 1, J - 1)), shape=(m, n))
    x = bench.unit12(7, n)
    ya, yt = a.mul(x), a.mul(x, transpose=True)
    np.testing.assert_allclose(ya, A @ x, rtol=1e-12, atol=0)
    np.testing.assert_allclose(yt, A.T @ x, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ya, b.mul(x), rtol=1e-12, atol=0)
    np.testing.assert_allclose(yt, b.mul(x, transpose=True), rtol=1e-12, atol=0)
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        inf = a.info(o)
        nelem = len(I) + inf["nb_partitions"]
        assert inf["nb_elements"] == nelem and inf["capacity"] == 1 << int(np.ceil(np.log2(np.ceil(nelem / 0.7)))) == 1 << 24
        assert not a.check(o)[2:7].any()
    assert a.info(dsa.COLMAJOR)["nb_partitions"] == n
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        a.rebalance_root(o)
        b.rebalance_root(o)
    assert_mat_equal(a, b)
    assert not a.check(dsa.COLMAJOR)[2:7].any() and not a.check(dsa.ROWMAJOR)[2:7].any()
    np.testing.assert_allclose(a.mul(x), A @ x, rtol=1e-12, atol=0)


def test_inserts_on_the_c3_matrix_match_oracle(dsa, hip, oracle):
    """The `inserts_on_c3` leg of bench.py at FULL size against the oracle: the 10 M-nnz matrix, 100 000 uniformly random A[i, j] = v
    (both 2^24-slot orientations take a random insert each), then 10 000 NEW columns of 10 rows (one append run in the colmajor
    orientation — the count-only replay on 16-slot segments with semaphore cells — and random inserts in the rowmajor twin).  Both
    orientations slot for slot after each half, the rebalance statistics, the invariant checker and y = A x (1e-12)."""
    import bench
    m = n = 1_000_000
    I, J, V = bench.c3_triplets(m, n, 10, 0, seed_rows=5, seed_vals=6)
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    b = dsa.dynamicsparse(I, J, V, m, n, binding=oracle)
    (ri, rj, rv), (ai, aj, av) = bench.c3_insert_leg(m, n)
    for Ii, Jj, Vv in ((ri[:256], rj[:256], rv[:256]), (ri[256:], rj[256:], rv[256:]), (ai, aj, av)):
        a.set_batch(Ii, Jj, Vv)
        b.set_batch(Ii, Jj, Vv)
        assert_mat_equal(a, b)
        for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
            ia, ib = a.info(o), b.info(o)
            for k in ("stat_extends", "stat_rebalances", "stat_window_slots"):
                assert ia[k] == ib[k], (o, k, ia[k], ib[k])
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        assert not a.check(o)[2:7].any(), o
    assert a.size() == (m, n + 10_000)
    x = bench.unit12(7, n + 10_000)
    np.testing.assert_allclose(a.mul(x), b.mul(x), rtol=1e-12, atol=0)


def test_root_rebalance_at_2_24_slots_from_every_relayout_mode_matches_oracle(dsa, hip, oracle):
    """The window the north-star roofline is quoted on: 11 M cells in 2^24 slots (the density of config 3).  From a source packed
    to the left (pack!), packed to the right (all gaps at the left), after _extend! (2^25 slots: compared with the oracle's
    pack! + spread! of the same cells over 2^25 raw slots) and after _shrink! back, the root rebalance must reproduce the oracle's
    layout slot for slot (src/moves.jl:94-171, src/pma.jl:94-103,143-161)."""
    import ctypes as C
    n = 11_000_000
    keys = np.arange(1, n + 1, dtype=np.int64) * 3 - 1
    vals = unit12_array(41, n)
    a = dsa.dynamicsparsevec(keys, vals, binding=hip)
    b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
    assert a.info()["capacity"] == 1 << 24
    assert_vec_equal(a, b)
    ref = b.export_layout()
    for mode in (1, 2):
        hip.call("vec_dev_relayout", a.h, mode)
        a.rebalance_root()
        assert layouts_equal(a.export_layout(), ref), mode
    hip.call("vec_dev_relayout", a.h, 3)                          # _extend!
    assert a.info()["capacity"] == 1 << 25
    cap2 = 1 << 25
    k2 = np.zeros(cap2, dtype=np.int64); v2 = np.zeros(cap2, dtype=np.float64); o2 = np.zeros(cap2, dtype=np.uint8)
    k2[:n], v2[:n], o2[:n] = keys, vals, 1
    P_I64, P_F64, P_U8 = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    rc = oracle.lib.ora_raw_pack_spread(k2.ctypes.data_as(P_I64), v2.ctypes.data_as(P_F64), o2.ctypes.data_as(P_U8), C.c_int64(cap2),
                                        C.c_int64(1), C.c_int64(cap2), C.c_int64(n), None, C.c_int64(0), C.c_int32(0), C.c_int32(1))
    assert rc == 0
    assert layouts_equal(a.export_layout(), (k2, v2, o2))
    del k2, v2, o2
    hip.call("vec_dev_relayout", a.h, 4)                          # _shrink!
    assert_vec_equal(a, b)
    assert not a.check()[2:7].any()


def test_c5_full_size_streaming_all_columns_vs_oracle(dsa, hip, oracle):
    """BASELINE config 5 at FULL size (100 000 rows, 16 rows per column, 50 000 columns streamed in ascending id, SpMV every 1000
    columns), ALL of it side by side with the CPU oracle (about 5 s of oracle time on the GPU box): y after every batch, slot layout
    and tables of both orientations after the first two batches and then every 5000 columns — the steady-state append replay of the
    colmajor orientation and the batch-parallel rounds of the rowmajor twin included —, rebalance statistics at the end, and y
    against scipy on all triples (1e-12)."""
    import scipy.sparse as sp
    import bench
    m5, ncols5, per5 = bench.C5_FULL[:3]
    every = 1000
    I5, J5, V5 = bench.c5_columns(m5, ncols5, per5)
    x5 = bench.unit12(13, ncols5)
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    ya = None
    for c0 in range(0, ncols5, every):
        sl = slice(c0 * per5, (c0 + every) * per5)
        a.set_batch(I5[sl], J5[sl], V5[sl])
        b.set_batch(I5[sl], J5[sl], V5[sl])
        nc = c0 + every
        ya = a.mul(x5[:nc], dense_out=m5)
        np.testing.assert_allclose(ya, b.mul(x5[:nc], dense_out=m5), rtol=RTOL, atol=0)
        if nc <= 2000 or nc % 5000 == 0:
            assert_mat_equal(a, b)
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        assert not a.check(o)[2:7].any(), o
        ia, ib = a.info(o), b.info(o)
        for k in ("stat_extends", "stat_rebalances", "stat_window_slots"):
            assert ia[k] == ib[k], (o, k, ia[k], ib[k])
    assert a.nnz() == ncols5 * per5
    A = sp.csr_matrix((V5, (I5 - 1, J5 - 1)), shape=(m5, ncols5))
    np.testing.assert_allclose(ya, A @ x5, rtol=1e-12, atol=0)
    assert a.size() == (int(I5.max()), ncols5)


def test_c5_streaming_with_deletions_20k_columns_vs_oracle(dsa, hip, oracle):
    """Config 5 with deletions at 20 000 columns (the shape of bench.py's c5_streaming_with_deletions leg): after every batch of 1000
    streamed columns 1 of 20 of them is deleted again (tombstones in the colmajor tables, purged partitions in the slot array, element
    deletes in the rowmajor twin), all of it side by side with the oracle: y after every batch, both layouts and tables every 5000
    columns, statistics at the end."""
    import bench
    m5, _, per5 = bench.C5_FULL[:3]
    ncols, every = 20_000, 1000
    I5, J5, V5 = bench.c5_columns(m5, ncols, per5)
    x5 = bench.unit12(13, ncols)
    a = dsa.dynamicsparse(fill_mode=False, binding=hip)
    b = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    for c0 in range(0, ncols, every):
        sl = slice(c0 * per5, (c0 + every) * per5)
        a.set_batch(I5[sl], J5[sl], V5[sl])
        b.set_batch(I5[sl], J5[sl], V5[sl])
        for j in range(c0 + 1, c0 + every + 1, 20):
            a.deletecolumn(j)
            b.deletecolumn(j)
        nc = c0 + every
        np.testing.assert_allclose(a.mul(x5[:nc], dense_out=m5), b.mul(x5[:nc], dense_out=m5), rtol=RTOL, atol=0)
        if nc <= 1000 or nc % 5000 == 0:
            assert_mat_equal(a, b)
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        assert not a.check(o)[2:7].any(), o
        ia, ib = a.info(o), b.info(o)
        for k in ("stat_extends", "stat_shrinks", "stat_rebalances", "stat_window_slots"):
            assert ia[k] == ib[k], (o, k, ia[k], ib[k])


# ---------------------------------------------------------------- the reference's functional tests, our RNG, HIP vs oracle
@pytest.mark.parametrize("n", [20, 1000, 20000])
def test_vec_fill_then_empty_matches_oracle(dsa, hip, oracle, n):
    """test/functional/sparsevector.jl:88-119: fill with n random keys then empty — every shrink level."""
    g = SplitMix64(n)
    keys = []
    seen = set()
    while len(keys) < n:
        k = 1 + g.next() % 10 ** 10
        if k not in seen:
            seen.add(k); keys.append(k)
    vals = [g.unit12() for _ in keys]
    a = dsa.dynamicsparsevec([], [], binding=hip)
    b = dsa.dynamicsparsevec([], [], binding=oracle)
    for v in (a, b):
        v.set_batch(keys, vals)
    assert_vec_equal(a, b)
    assert a.nnz() == n
    half = keys[: n // 2]
    for v in (a, b):
        v.set_batch(half, np.zeros(len(half)))
    assert_vec_equal(a, b)
    rest = keys[n // 2:]
    for v in (a, b):
        v.set_batch(rest, np.zeros(len(rest)))
    assert_vec_equal(a, b)
    assert a.nnz() == 0 and a.info()["stat_shrinks"] == b.info()["stat_shrinks"]


def test_pcsc_42_partitions_matches_oracle(dsa, hip, oracle):
    """test/functional/sparsematrix.jl:123-156 through the PackedCSC entry points."""
    g = SplitMix64(42)
    parts = [{1 + g.next() % 10000: float(1 + g.next() % 99) for _ in range(20 + g.next() % 300)} for _ in range(42)]
    rk, vv = [list(d) for d in parts], [list(d.values()) for d in parts]
    a = dsa.packedcsc(rk, vv, binding=hip)
    b = dsa.packedcsc(rk, vv, binding=oracle)
    for _ in range(1500):
        pid = 1 + g.next() % 42
        key = 1 + g.next() % 10000
        val = float(g.next() % 5)           # zeros delete
        a[key, pid] = val
        b[key, pid] = val
    a[3, 45] = 1.0                          # auto-creates partitions 43..45 (src/pcsr.jl:295-297)
    b[3, 45] = 1.0
    a.deletepartition(7)
    b.deletepartition(7)
    la, lb = a.export_layout(), b.export_layout()
    assert layouts_equal(la[:3], lb[:3]) and np.array_equal(la[3], lb[3])
    assert a.nnz() == b.nnz() and a.nbpartitions() == b.nbpartitions() == 44
    for _ in range(300):
        pid = 1 + g.next() % 42
        key = 1 + g.next() % 10000
        if pid != 7:
            assert a[key, pid] == b[key, pid]


def test_matrix_append_thousands_of_columns_matches_oracle(dsa, hip, oracle):
    """test/functional/sparsematrix.jl:369-382: `for col in nb_cols:5000; matrix[1,col] = 1`."""
    I, J, V = rand_matrix_ops(77, 340, 1000, 17000, pzero=0.0)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    cols = np.arange(1000, 5001)
    for m_ in (a, b):
        m_.set_batch(np.ones(len(cols), dtype=np.int64), cols, np.ones(len(cols)))
    assert_mat_equal(a, b)
    assert np.all(a.get_batch(np.ones(len(cols), dtype=np.int64), cols) == 1.0)


def test_fill_mode_flush_matches_oracle(dsa, hip, oracle):
    """closefillmode! (src/matrix.jl:126-134) through the device K-build: duplicates fold in input order."""
    g = SplitMix64(8)
    row = [1 + g.next() % 1000 for _ in range(10000)]
    col = [1 + g.next() % 1000 for _ in range(10000)]
    val = [float(1 + g.next() % 100000) for _ in range(10000)]
    mats = []
    for bnd in (hip, oracle):
        m_ = dsa.dynamicsparse(fill_mode=True, binding=bnd)
        m_.addrow(2000, [5, 3, 9], [1.0, 2.0, 3.0])
        m_.set_batch(row, col, val)
        m_.closefillmode()
        mats.append(m_)
    assert_mat_equal(*mats)
    # non-integer duplicates: the fold order (input order) must match bit for bit
    I = [1, 1, 1, 2, 2]
    J = [1, 1, 1, 3, 3]
    V = [0.1, 0.2, 0.3, 1e16, 1.0]
    assert_mat_equal(dsa.dynamicsparse(I, J, V, binding=hip), dsa.dynamicsparse(I, J, V, binding=oracle))


@pytest.mark.parametrize("nnz", [1, 63, 64, 65, 4095, 4096, 4097, 8193, 70001])
def test_kbuild_sort_tile_boundaries_match_oracle(dsa, hip, oracle, nnz):
    """the hand-written radix sort of K-build (csrc/build.hip) around its tile sizes (64-element wave rows, 4096-element tiles):
    random triples with duplicates, both orientations slot for slot; the vector constructor with each combine."""
    g = np.random.default_rng(nnz)
    I = g.integers(1, 300, nnz)
    J = g.integers(1, 70000, nnz)
    V = g.integers(1, 1000, nnz).astype(np.float64) / 7.0
    assert_mat_equal(dsa.dynamicsparse(I, J, V, binding=hip), dsa.dynamicsparse(I, J, V, binding=oracle))
    for comb in ("+", "*", "last"):
        K = g.integers(1, max(2, nnz // 3), nnz)
        assert_vec_equal(dsa.dynamicsparsevec(K, V, comb, binding=hip), dsa.dynamicsparsevec(K, V, comb, binding=oracle))


def test_kbuild_long_duplicate_runs_fold_in_input_order(dsa, hip, oracle):
    """duplicates of one (i, j) far beyond what a lane folds itself (64): the rest of the run is folded by a wave, 64 values per
    coalesced load, still left to right in input order (src/pcsr.jl:374-375) — non-associative Float64 sums must match bit for bit."""
    g = np.random.default_rng(77)
    n_other = 20000
    I = np.concatenate([g.integers(1, 500, n_other), np.full(30000, 42), np.full(65, 7), np.full(64, 8), np.full(129, 9)])
    J = np.concatenate([g.integers(1, 500, n_other), np.full(30000, 17), np.full(65, 3), np.full(64, 3), np.full(129, 3)])
    V = g.random(len(I)) * np.where(g.random(len(I)) < 0.5, 1e10, 1e-3)
    perm = g.permutation(len(I))
    I, J, V = I[perm], J[perm], V[perm]
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    assert_mat_equal(a, b)
    assert a[42, 17] == b[42, 17] and a[9, 3] == b[9, 3]
    K = np.concatenate([np.full(100000, 5), g.integers(1, 50, 1000)])
    W = 1.0 + g.random(len(K)) * 1e-6
    for comb in ("+", "*", "last"):
        assert_vec_equal(dsa.dynamicsparsevec(K, W, comb, binding=hip), dsa.dynamicsparsevec(K, W, comb, binding=oracle))


def test_kbuild_key_ranges_composite_and_general_paths(dsa, hip, oracle):
    """the composite (partition, key) of K-build is as wide as the two key RANGES: negative keys, offsets near 2^62, one side wide and
    the other narrow (still one 64-bit composite), and both sides wider than 32 bits (the general two-sort path)."""
    g = np.random.default_rng(5)
    n = 30000
    cases = {
        "negative": (g.integers(-5000, 5000, n), g.integers(-300, 300, n)),
        "offset": (g.integers(1, 1000, n) + (1 << 62), g.integers(1, 1000, n) - (1 << 61)),
        "wide_rows": (g.integers(1, 1 << 50, n), g.integers(1, 4000, n)),
        "wide_cols": (g.integers(1, 4000, n), g.integers(-(1 << 45), 1 << 45, n)),
        "both_wide": (g.integers(1, 1 << 40, n), g.integers(1, 1 << 40, n)),            # 80-bit composite: general path
        "single_column": (g.integers(1, 100000, n), np.full(n, 12)),
        "single_row": (np.full(n, -3), g.integers(1, 100000, n)),
    }
    for name, (I, J) in cases.items():
        I = np.where(I == 0, 1, I)
        J = np.where(J == 0, 1, J)
        V = g.integers(1, 50, n).astype(np.float64)
        assert_mat_equal(dsa.dynamicsparse(I, J, V, binding=hip), dsa.dynamicsparse(I, J, V, binding=oracle))
    rows = [np.sort(g.choice(5000, size=int(c), replace=True)) + 1 for c in g.integers(0, 40, 200)]
    rows[0] = np.array([], dtype=np.int64)
    rows[57] = np.array([], dtype=np.int64)
    rows[199] = np.array([], dtype=np.int64)
    vals = [g.random(len(r)) + 1.0 for r in rows]
    pa, pb = dsa.packedcsc(rows, vals, binding=hip), dsa.packedcsc(rows, vals, binding=oracle)
    la, lb = pa.export_layout(), pb.export_layout()
    assert layouts_equal(la[:3], lb[:3]) and np.array_equal(la[3], lb[3])


def test_failed_closefillmode_leaves_a_usable_fill_mode_matrix(dsa, hip, oracle):
    """A build that fails inside closefillmode! (out of memory, a HIP error: injected with DSA_FAIL_BUILD) must leave the matrix in
    fill mode with every triple it held — no dangling device pointers, no leaked streams — so that more rows can be appended and
    the next closefillmode! builds everything; also for a matrix built from caller memory (nothing half-built survives)."""
    g = SplitMix64(18)
    row = [1 + g.next() % 500 for _ in range(6000)]
    col = [1 + g.next() % 500 for _ in range(6000)]
    val = [float(1 + g.next() % 1000) for _ in range(6000)]
    a = dsa.dynamicsparse(fill_mode=True, binding=hip)
    b = dsa.dynamicsparse(fill_mode=True, binding=oracle)
    for m_ in (a, b):
        m_.set_batch(row[:4000], col[:4000], val[:4000])
    os.environ["DSA_DEV"] = "1"          # development switches are honoured only with DSA_DEV=1 (include/dsa.h)
    os.environ["DSA_FAIL_BUILD"] = "1"
    try:
        for _ in range(2):
            with pytest.raises(dsa.DsaError) as ei:
                a.closefillmode()
            assert ei.value.code == dsa.binding.EHIP
        with pytest.raises(dsa.DsaError):
            dsa.dynamicsparse(row, col, val, binding=hip)
    finally:
        del os.environ["DSA_FAIL_BUILD"]
        del os.environ["DSA_DEV"]
    with pytest.raises(dsa.DsaError):           # still in fill mode: no lookups
        a[1, 1]
    for m_ in (a, b):
        m_.addrow(2000, [5, 3, 9], [1.0, 2.0, 3.0])
        m_.set_batch(row[4000:], col[4000:], val[4000:])
        m_.closefillmode()
    assert_mat_equal(a, b)
    assert not a.check(0)[2:7].any() and not a.check(1)[2:7].any()


def test_negative_and_huge_keys_match_oracle(dsa, hip, oracle):
    res = []
    for bnd in (hip, oracle):
        v = dsa.dynamicsparsevec([-5, 10 ** 15, 3, -(10 ** 12)], [1.0, 2.0, 3.0, 4.0], binding=bnd)
        v[-7] = 9.0
        v[3] = 0
        a = dsa.dynamicsparse([1, 2, 3], [5, -2, 10 ** 13], [1.0, 2.0, 3.0], binding=bnd)
        a[7, -9] = 4.0
        a[-4, 5] = 2.5                       # negative row key: lands in the rowmajor twin's tables
        a[-4, 5] = 0.0                       # delete path on a range that starts at the semaphore, key < 0
        res.append((v, a))
    assert_vec_equal(res[0][0], res[1][0])
    assert_mat_equal(res[0][1], res[1][1])
    assert res[0][1].col_view(-9) == [(7, 4.0)]
    # sparse x with a negative column key: only the x-driven kernel can address it (like the reference's _mul)
    ya = res[0][1].mul(([-9, 5], [2.0, 3.0]))
    yb = res[1][1].mul(([-9, 5], [2.0, 3.0]))
    assert np.array_equal(ya[0], yb[0]) and np.array_equal(ya[1], yb[1])


def test_row_and_column_slices_match_oracle(dsa, hip, oracle):
    """m[:, j] / m[i, :] as new dynamic sparse vectors (src/pcsr.jl:247-291); the HIP row slice comes from the
    rowmajor twin, the oracle's from the reference's scan of the colmajor array — same entries, same layout."""
    I, J, V = rand_matrix_ops(31, 60, 90, 2500, pzero=0.0)
    a = dsa.dynamicsparse(I, J, V, binding=hip)
    b = dsa.dynamicsparse(I, J, V, binding=oracle)
    for key in (1, 7, 33, 60, 89, 1000):
        assert_vec_equal(a.col_slice(key), b.col_slice(key))
        assert_vec_equal(a.row_slice(key), b.row_slice(key))


def test_slices_and_views_stay_on_the_device(dsa, hip, oracle):
    """m[:, j] / m[i, :] are built device to device (view kernel -> ONE spread launch from the orientation's idle slot
    buffer; csrc/dsa_host.hip vec_from_packed_dev) and dsa_mat_*_view_dev deliver a view into caller-owned HBM.  Short partitions
    (one wave), partitions above 16384 slots (tile counts + scan + K-pack), 64-bit keys, empty and missing columns; the new vectors slot
    for slot against the oracle's (src/pcsr.jl:247-291, src/pma.jl:69-84), the matrix untouched and writable afterwards."""
    import torch
    rng = np.random.default_rng(77)
    # column 5 holds 30 000 rows (a partition of > 16384 slots), row 3 holds 2000 columns, the rest is sparse
    I = np.concatenate([rng.choice(200000, 30000, replace=False) + 1, np.full(2000, 3), rng.integers(1, 200001, 5000)])
    J = np.concatenate([np.full(30000, 5), rng.choice(40000, 2000, replace=False) + 1, rng.integers(1, 40001, 5000)])
    V = rng.integers(1, 100, len(I)).astype(np.float64)
    for wide in (False, True):
        if wide:
            I = I.copy(); J = J.copy()
            I[I == 77] = 2 ** 40 + 7; J[J == 9] = 2 ** 36
            I[0] = 2 ** 40 + 9                       # (column 5 holds a 64-bit row key: its slice is a wide vector)
        a = dsa.dynamicsparse(I, J, V, binding=hip)
        b = dsa.dynamicsparse(I, J, V, binding=oracle)
        cols = [5, 1, 2, int(J[-1]), 2 ** 36, 40001, 123456789]
        rows = [3, 1, int(I[-1]), 2 ** 40 + 7, 2 ** 40 + 9, 200001]
        for key in cols:
            assert_vec_equal(a.col_slice(key), b.col_slice(key))
        for key in rows:
            assert_vec_equal(a.row_slice(key), b.row_slice(key))
        dk = torch.empty(40000, dtype=torch.int64, device="cuda"); dv = torch.empty(40000, dtype=torch.float64, device="cuda")
        for key in cols:
            n = a.col_view_dev(key, dk.data_ptr(), dv.data_ptr(), 40000)
            a.sync()
            want = b.col_view(key)
            assert n == len(want)
            assert list(zip(dk[:n].cpu().tolist(), dv[:n].cpu().tolist())) == want
        for key in rows:
            n = a.row_view_dev(key, dk.data_ptr(), dv.data_ptr(), 40000)
            a.sync()
            want = b.row_view(key)
            assert n == len(want) and list(zip(dk[:n].cpu().tolist(), dv[:n].cpu().tolist())) == want
        with pytest.raises(dsa.DsaError):
            a.col_view_dev(5, dk.data_ptr(), dv.data_ptr(), 100)        # DSA_ECAP
        # a slice is a vector of its own: writes to it leave the matrix alone, and the matrix keeps working
        va, vb = a.col_slice(5), b.col_slice(5)
        for v in (va, vb):
            v.set_batch(np.arange(1, 3001, dtype=np.int64) * 7, np.ones(3000))
        assert_vec_equal(va, vb)
        assert_mat_equal(a, b)
        I2 = rng.integers(1, 200001, 3000); J2 = rng.integers(1, 40001, 3000); V2 = rng.integers(0, 5, 3000).astype(np.float64)
        for m in (a, b):
            m.set_batch(I2, J2, V2)
        assert_mat_equal(a, b)
        assert_vec_equal(a.col_slice(5), b.col_slice(5))
        assert_vec_equal(a.row_slice(3), b.row_slice(3))


def test_c4_shard_scale_build_spmv_and_root_rebalance(dsa, hip, oracle):
    """One shard of BASELINE config 4 at full size: 1.25 M columns x 10 M rows, 12.5 M nnz -> capacity 2^25 in both
    orientations (colmajor density 0.41, rowmajor 0.67).  Both orientations SLOT FOR SLOT against the oracle's build of the
    same triples (scalars, 2 x 2^25 slots, tables), again after a root rebalance of each; capacity rule, element counts,
    semaphore table, SpMV vs scipy and the oracle (1e-12), device invariant checker."""
    import scipy.sparse as sp
    m, n, per = 10_000_000, 1_250_000, 10
    rows = 1 + (splitmix_array(8, n * per) % np.uint64(m)).astype(np.int64)
    cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), per)
    vals = unit12_array(9, n * per)
    key = cols * np.int64(m + 1) + rows
    _, first = np.unique(key, return_index=True)
    rows, cols, vals = rows[first], cols[first], vals[first]
    del key, first
    a = dsa.dynamicsparse(rows, cols, vals, m, n, binding=hip)
    b = dsa.dynamicsparse(rows, cols, vals, m, n, binding=oracle)
    for o in (0, 1):
        inf = a.info(o)
        assert inf["capacity"] == 1 << 25, inf
        assert inf["nb_elements"] == len(rows) + inf["nb_partitions"]
    assert a.info(0)["nb_partitions"] == n
    assert_mat_equal(a, b)
    x = unit12_array(10, n)
    y = a.mul(x)
    A = sp.csr_matrix((vals, (rows - 1, cols - 1)), shape=(m, n))
    np.testing.assert_allclose(y, A @ x, rtol=RTOL, atol=0)
    np.testing.assert_allclose(y, b.mul(x), rtol=RTOL, atol=0)
    xt = unit12_array(11, m)
    np.testing.assert_allclose(a.mul(xt, transpose=True), A.T @ xt, rtol=RTOL, atol=0)
    del A
    L0 = a.export_layout(0)
    occ = L0["occ"].astype(bool)
    pos = np.nonzero(occ)[0] + 1
    sem = L0["keys"][occ] == 0
    assert np.array_equal(pos[sem], L0["semaphores"])
    del L0, occ, pos, sem
    for o in (0, 1):                         # device-side invariant checker at full size
        rep = a.check(o)
        assert rep[0] == a.info(o)["nb_elements"] and rep[1] == a.info(o)["nb_partitions"] and not rep[2:7].any(), rep
    for o in (0, 1):                         # full 2^25-slot windows: layout-idempotent, on both implementations
        a.rebalance_root(o)
        b.rebalance_root(o)
    assert_mat_equal(a, b)


def test_c4_full_config_eight_shards_sum_of_partials_vs_scipy(dsa, hip):
    """BASELINE config 4 as a CONFIG: 10 M x 10 M, 10 rows per column = 10^8 triples, split into 8 contiguous column ranges of
    1.25 M columns.  The test box has one GPU, so the 8 shards are built and multiplied one after the other through the product
    class bench.py drives (sharding.ColumnShard, world = 8, rank g) and their partial y are summed on the device — exactly what
    the all-reduce computes; compared with scipy on all 10^8 triples (1e-12).  Every shard: capacity 2^25, invariant checker."""
    import scipy.sparse as sp
    import torch
    from dsa_amd import sharding
    m = n = 10_000_000
    per, G = 10, 8
    dev = torch.device("cuda:0")
    x = unit12_array(10, n)
    y_sum = torch.zeros(m, dtype=torch.float64, device=dev)
    y_ref = np.zeros(m)
    for g in range(G):
        c0 = g * (n // G)
        nc = n // G
        rows = 1 + (splitmix_array(8, nc * per) % np.uint64(m)).astype(np.int64) if g == 0 else \
            1 + (splitmix_array(8 + 100 * g, nc * per) % np.uint64(m)).astype(np.int64)
        cols = np.repeat(np.arange(c0 + 1, c0 + nc + 1, dtype=np.int64), per)
        vals = unit12_array(9 + 100 * g, nc * per)
        # the shard receives the triples of ITS column range with GLOBAL column keys, as bench.py hands them over
        sh = sharding.ColumnShard(dsa, rows, cols, vals, m, n, g, G, binding=hip)
        assert (sh.col0, sh.ncols) == (c0, nc)
        for o in (0, 1):
            inf = sh.A.info(o)
            assert inf["capacity"] == 1 << 25, (g, o, inf)
            assert not sh.A.check(o)[2:7].any()
        xs = sh.x_slice(x)
        yp = torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
        sh.spmv_partial(xs, yp)
        torch.cuda.synchronize()
        y_sum += yp
        A = sp.csr_matrix((vals, (rows - 1, cols - 1 - c0)), shape=(m, nc))      # duplicates inside a column are summed by both
        y_ref += A @ x[c0:c0 + nc]
        del A, sh, rows, cols, vals, yp
    np.testing.assert_allclose(y_sum.cpu().numpy(), y_ref, rtol=RTOL, atol=1e-300)


def test_write_combined_single_sets_match_oracle(dsa, hip, oracle):
    """dsa_vec_set / dsa_mat_set queue their writes and flush them in order (65536 pending, or the next observing
    call): 70k single-op calls must leave exactly the layout of 70k sequential setindex! calls."""
    g = SplitMix64(123)
    ks = [1 + g.next() % 200000 for _ in range(70000)]
    vs = [0.0 if g.next() % 5 == 0 else g.unit12() for _ in ks]
    a = dsa.dynamicsparsevec([], [], binding=hip)
    b = dsa.dynamicsparsevec([], [], binding=oracle)
    for k, v in zip(ks, vs):
        a[k] = v
    b.set_batch(ks, vs)
    assert len(a) == len(b)                      # length is updated eagerly
    assert_vec_equal(a, b)
    I, J, V = rand_matrix_ops(55, 300, 400, 8000)
    ma = dsa.dynamicsparse(fill_mode=False, binding=hip)
    mb = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    for i, j, v in zip(I, J, V):
        ma[i, j] = v
    mb.set_batch(I, J, V)
    assert ma.size() == mb.size()
    assert ma[I[0], J[0]] == mb[I[0], J[0]]      # a read in the middle forces the flush
    assert_mat_equal(ma, mb)
    ma.deletecolumn(J[1]); mb.deletecolumn(J[1])  # tombstones: later single writes apply eagerly
    for i, j, v in zip(I[:500], J[:500], V[:500]):
        if j != J[1]:
            ma[i, j + 1000] = v
            mb[i, j + 1000] = v
    assert_mat_equal(ma, mb)


def test_device_checker_counts_on_small_structures(dsa, hip):
    """dsa_*_check: cell / semaphore counts and zero violations on freshly built structures (the public API offers no
    way to corrupt a structure, so the failing direction is exercised only through the counters' consistency)."""
    m = dsa.dynamicsparse([1, 2, 3], [1, 1, 2], [1.0, 2.0, 3.0], binding=hip)
    assert not m.check(0)[2:7].any() and not m.check(1)[2:7].any()
    v = dsa.dynamicsparsevec([3, 1, 2], [1.0, 2.0, 3.0], binding=hip)
    r = v.check()
    assert r[0] == 3 and not r[2:7].any()


def test_wide_keys_and_widening(dsa, hip, oracle):
    """Keys are kept in 32 bits in HBM until the first key outside Int32 (KeyArr, csrc/dsa_dev.h): structures built wide, structures
    widened by a later write (vector keys, matrix row keys, matrix column keys separately), values straddling +-2^31, and the usual
    observers (layout export, views, lookups) on both sides of the switch."""
    big = [2**31 - 1, 2**31, 2**31 + 5, 2**40 + 3, -(2**31), -(2**31) - 1, -(2**45)]
    # vector: narrow -> widened by a batch, then more writes
    ks = np.arange(1, 5001, dtype=np.int64) * 7
    va = [dsa.dynamicsparsevec(ks, ks.astype(np.float64), binding=b) for b in (hip, oracle)]
    for v in va:
        v.set_batch(np.array(big, dtype=np.int64), np.arange(1, len(big) + 1, dtype=np.float64))
        v.set_batch(ks[:300] + 1, np.ones(300))
        v[2**33] = 4.5
        v[2**33] = 0.0
    ka, kb = va[0].export_layout(), va[1].export_layout()
    assert np.array_equal(ka[2], kb[2])
    occ = ka[2].astype(bool)
    assert np.array_equal(ka[0][occ], kb[0][occ]) and np.array_equal(ka[1][occ], kb[1][occ])
    assert va[0][2**40 + 3] == va[1][2**40 + 3] == 4.0
    # vector built wide from the start
    wa = [dsa.dynamicsparsevec(np.array(sorted(big) + [5, 6]), np.arange(9, dtype=np.float64) + 1, binding=b) for b in (hip, oracle)]
    assert np.array_equal(wa[0].export_layout()[0][wa[0].export_layout()[2].astype(bool)], wa[1].export_layout()[0][wa[1].export_layout()[2].astype(bool)])
    # matrix: first narrow, then a huge ROW key (colmajor keys widen), then a huge COLUMN key (rowmajor keys widen)
    I = 1 + (splitmix_array(71, 4000) % np.uint64(900)).astype(np.int64)
    J = 1 + (splitmix_array(72, 4000) % np.uint64(700)).astype(np.int64)
    V = (1 + splitmix_array(73, 4000) % np.uint64(9)).astype(np.float64)
    ms = [dsa.dynamicsparse(I, J, V, binding=b) for b in (hip, oracle)]
    assert_mat_equal(*ms)
    for step, (ii, jj) in enumerate([([2**35, 3, 4], [5, 5, 6]), ([7, 8], [2**34 + 1, 9]), ([2**35, 2**35 + 1], [2**34 + 1, 2**34 + 2])]):
        for m_ in ms:
            m_.set_batch(ii, jj, [1.5 + step] * len(ii))
        assert_mat_equal(*ms)
    big_batch_i = np.concatenate([I[:500] + 1, np.array([2**36, 2**36 + 1])])
    big_batch_j = np.concatenate([J[:500], np.array([3, 2**37])])
    for m_ in ms:
        m_.set_batch(big_batch_i, big_batch_j, np.ones(len(big_batch_i)))          # batch-parallel path with wide keys
    assert_mat_equal(*ms)
    assert ms[0].col_view(5) == ms[1].col_view(5) and ms[0].row_view(2**35) == ms[1].row_view(2**35)
    assert np.array_equal(ms[0].get_batch([2**35, 7, 1], [5, 2**34 + 1, 1]), ms[1].get_batch([2**35, 7, 1], [5, 2**34 + 1, 1]))
    # (no SpMV here: with indices beyond 2^31 the dense result vector of the product would not fit any memory)
    # matrix built wide from the start
    mw = [dsa.dynamicsparse(np.array([1, 2**33, 5]), np.array([2**32 + 7, 2, 2]), np.array([1.0, 2.0, 3.0]), binding=b) for b in (hip, oracle)]
    assert_mat_equal(*mw)


def test_differential_fuzz_short(dsa, hip, oracle):
    """60 scenarios of tools/fuzz.py (random write batches: column / row streams, delete- and overwrite-heavy mixes, negative keys,
    tombstones, vectors) — HIP vs oracle after every batch.  The long run is `python tools/fuzz.py 240` (1540 scenarios clean in round 1)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("dsa_fuzz", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    res = {}
    for seed in range(9000, 9060):
        r = fz.run_matrix(seed) if seed % 4 else fz.run_vector(seed)
        res[r] = res.get(r, 0) + 1
    assert res.get("ok", 0) >= 30, res


def test_forced_64bit_keys_and_replay_variants_in_subprocesses(dsa, hip, oracle):
    """DSA_KEYS_WIDE=1 (read when the library is loaded) keeps every structure in 64-bit keys: the wide instantiations of the
    streaming kernels and the wide side of the key proxy stay covered — 12 s of the differential fuzzer in a child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # DSA_POS_WIDE=1 additionally selects the 64-bit-position instantiation of the append-run replay (used for capacities > 2^30)
    env = dict(os.environ, DSA_DEV="1", DSA_KEYS_WIDE="1", DSA_POS_WIDE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz.py"), "12", "12345"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fuzz done" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "appendbench.py"), "--check"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "append parity ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    # DSA_COUNT_MODEL=0: the bitmap-only append replay (the path every op takes outside the count model's regime) on a whole batch
    env = dict(os.environ, DSA_DEV="1", DSA_COUNT_MODEL="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "appendbench.py"), "--check"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "append parity ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz.py"), "8", "777"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    # DSA_LOCAL_ROUNDS=0: small structures through the grid rounds only (the suite itself runs them on the local rounds)
    env = dict(os.environ, DSA_DEV="1", DSA_LOCAL_ROUNDS="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz.py"), "8", "4242"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    # DSA_BUILD_WIDE=1: every bulk build (vectors, PackedCSC, matrices, fill-mode flushes) through the GENERAL path of K-build — two runs
    # of the hand-written radix sort with the input index as payload, hand-written flag scans (the path composites wider than 64 bits take)
    env = dict(os.environ, DSA_DEV="1", DSA_BUILD_WIDE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz.py"), "10", "9090"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    # DSA_MODEL3=0: long append runs on the per-op replay alone (what the count-only model hands back: short runs, small typed segments)
    env = dict(os.environ, DSA_DEV="1", DSA_MODEL3="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "appendbench.py"), "--check"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "append parity ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_vector_equality_axpby_filter_match_oracle(dsa, hip, oracle):
    """== (src/vector.jl:85-87, src/pma.jl:236-266), + / - / unary - (AbstractSparseVector fallbacks, test/functional/math.jl:53-94)
    and filter (src/pma.jl:224-234) on device vectors: verdicts and result pairs identical to the oracle's, over small, large,
    32-bit and 64-bit-key vectors."""
    def build(b, k, v, **kw):
        return dsa.dynamicsparsevec(k, v, binding=b, **kw)

    for seed, n, keyspace in [(1, 25, 100), (2, 25, 100), (3, 3000, 5000), (4, 200000, 400000), (5, 1, 10), (6, 0, 10)]:
        k1 = 1 + (splitmix_array(100 + seed, n) % np.uint64(keyspace)).astype(np.int64)
        v1 = (1 + splitmix_array(200 + seed, n) % np.uint64(10)).astype(np.float64)
        k2 = 1 + (splitmix_array(300 + seed, n) % np.uint64(keyspace)).astype(np.int64)
        v2 = (1 + splitmix_array(400 + seed, n) % np.uint64(10)).astype(np.float64)
        res = []
        for b in (hip, oracle):
            x, y = build(b, k1, v1, n=keyspace), build(b, k2, v2, n=keyspace)
            r = [x + y, x - y, y - x, -x, x - x, x.axpby(2.5, y, -0.75), x == y, x == x]
            z = build(b, k1[: n // 2], v1[: n // 2], n=keyspace)
            z.set_batch(k1[n // 2:], np.zeros(n - n // 2))              # deletes of absent keys / of first-half duplicates
            z2 = build(b, *z.nonzeros(), n=keyspace)
            r += [z == z2, z2 == z, z == x]
            f = x.filter(lambda e: e[0] % 3 == 1)
            r += [f.nonzeros(), len(f), f.export_layout()]
            res.append(r)
        for got, want in zip(*res):
            if isinstance(got, tuple):
                assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
            else:
                assert got == want
        assert len(res[0][4][0]) == 0 and res[0][7] is True and res[0][8] is True
    # same content behind 32-bit and 64-bit physical keys; NaN; different lengths
    k = np.arange(1, 3001, dtype=np.int64) * 5
    v = np.arange(1, 3001, dtype=np.float64)
    for b in (hip, oracle):
        a, w = build(b, k, v), build(b, k, v)
        w[2**40] = 1.0
        assert not (a == w) and not (w == a)
        w[2**40] = 0.0                                    # w keeps 64-bit keys in the HIP library
        w.shrink_size()
        assert a == w and w == a
        s = a + w
        assert np.array_equal(s[0], k) and np.array_equal(s[1], 2 * v)
        w[5] = float("nan")
        c = build(b, *w.nonzeros())
        assert w == w and not (w == c) and not (a == w)
        big = build(b, np.array([2**35, 7, -(2**33)]), np.array([1.0, 2.0, 3.0]))
        ks, vs = big - a
        want_k = np.concatenate([[-(2**33)], k, [2**35]]).astype(np.int64)
        want_k = np.unique(np.concatenate([want_k, [7]]))
        assert np.array_equal(ks, want_k)


@pytest.mark.gpu
def test_shard_entry_points_split_spmv_exactly(dsa, hip, oracle):
    """dsa_shard_create_from_coo / dsa_shard_spmv_dev (include/dsa.h): every shard is the reference layout of ITS
    sub-matrix (slot-for-slot equal to the oracle's build of the filtered triples) and the partial products sum to A*x."""
    import ctypes as C
    import torch
    import cpu_shard
    from dsa_amd import sharding
    m, n, nnz, G = 5000, 3001, 40000, 3
    I = 1 + (splitmix_array(501, nnz) % np.uint64(m)).astype(np.int64)
    J = 1 + (splitmix_array(502, nnz) % np.uint64(n)).astype(np.int64)
    V = unit12_array(503, nnz)
    x = unit12_array(504, n)
    full = dsa.dynamicsparse(I, J, V, m, n, binding=oracle)
    y_ref = full.mul(x, dense_out=m)
    y = np.zeros(m)
    for g in range(G):
        sh = sharding.ColumnShard(dsa, I, J, V, m, n, g, G, binding=hip)
        ref = cpu_shard.make_cpu_shard_class(sharding)(dsa, I, J, V, m, n, g, G, binding=oracle)
        assert_mat_equal(sh.A, ref.A)
        assert sh.A.size() == (m, sh.ncols)
        dx = sh.x_slice(x)                                       # CUDA tensor next to the HIP library
        assert dx.is_cuda and not ref.x_slice(x).is_cuda
        dy = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
        hip.call("shard_spmv_dev", sh.A.h, C.c_void_p(dx.data_ptr()), sh.ncols, C.c_void_p(dy.data_ptr()), m)
        torch.cuda.synchronize()
        part = dy.cpu().numpy()
        assert np.array_equal(part, sh.spmv_partial(dx).cpu().numpy())
        np.testing.assert_allclose(part, ref.spmv_partial(ref.x_slice(x)).numpy(), rtol=RTOL, atol=0)
        y += part
    np.testing.assert_allclose(y, y_ref, rtol=RTOL, atol=0)


# ---------------------------------------------------------------- round 2: the replay's memo between runs, grid-wide table merges
@pytest.mark.gpu
@pytest.mark.parametrize("n_first,total,runs", [(3, 120000, [40000, 700, 90000, 5000]), (150, 200000, [100000, 100000, 3000]),
                                                (90000, 90000, [513, 30000, 512, 2000, 250000])])
def test_append_runs_count_only_model_on_vectors_of_every_segment_size(dsa, hip, oracle, n_first, total, runs):
    """The count-only replay of long append runs (csrc/appendmodel.hip: tables of per-level epochs, a driver above them, one
    bitmap write) against sequential setindex! on the oracle: vectors GROWN from a few keys keep segments of 2 / 8 slots for life
    (_extend! doubles the segment count, src/pma.jl:143-151), a vector built from 90 000 keys has 16-slot segments.  Runs around
    the model's minimum length, runs that cross one and two _extend!s, layouts / scalars / rebalance statistics after every run."""
    keys = np.arange(1, total + 1, dtype=np.int64) * 2
    a = dsa.dynamicsparsevec(keys[:n_first], unit12_array(9, n_first), binding=hip)
    b = dsa.dynamicsparsevec(keys[:n_first], unit12_array(9, n_first), binding=oracle)
    if total > n_first:
        a.set_batch(keys[n_first:], unit12_array(10, total - n_first))
        b.set_batch(keys[n_first:], unit12_array(10, total - n_first))
    nxt = int(keys[-1]) + 1
    for r_i, r in enumerate(runs):
        ks = np.arange(nxt, nxt + r, dtype=np.int64)
        nxt += r
        vs = unit12_array(20 + r_i, r)
        a.set_batch(ks, vs)
        b.set_batch(ks, vs)
        assert_vec_equal(a, b)
        ia, ib = a.info(), b.info()
        for k in ("stat_extends", "stat_rebalances", "stat_window_slots"):
            assert ia[k] == ib[k], (k, r_i, ia[k], ib[k])
    rep = a.check()
    assert rep[0] == a.nnz() and not rep[2:7].any(), rep


def test_append_runs_count_only_model_on_a_built_matrix_with_ragged_columns(dsa, hip, oracle):
    """Typed runs (semaphore cells of new columns among the appended cells) on a matrix BUILT from triples — 16-slot segments, the
    geometry the count-only replay takes for MappedPackedCSC runs: columns of 1..40 rows streamed in ascending column id in batches
    of several thousand cells, across an _extend! of the colmajor orientation; both orientations slot for slot after every batch."""
    g = SplitMix64(4242)
    m, n0 = 40000, 12000
    I0, J0 = [], []
    for j in range(1, n0 + 1):
        for i in sorted({1 + g.next() % m for _ in range(1 + g.next() % 12)}):
            I0.append(i); J0.append(j)
    V0 = unit12_array(7, len(I0))
    A = dsa.dynamicsparse(I0, J0, V0, binding=hip)
    B = dsa.dynamicsparse(I0, J0, V0, binding=oracle)
    assert A.info(0)["segment_capacity"] == 16
    cap0 = A.info(0)["capacity"]
    col = n0
    for r_i, ncols in enumerate([300, 1200, 40, 2500, 6000]):
        I, J = [], []
        for _ in range(ncols):
            col += 1
            for i in sorted({1 + g.next() % m for _ in range(1 + g.next() % 40)}):
                I.append(i); J.append(col)
        V = unit12_array(50 + r_i, len(I))
        A.set_batch(I, J, V)
        B.set_batch(I, J, V)
        assert_mat_equal(A, B)
        for o in (0, 1):
            ia, ib = A.info(o), B.info(o)
            for k in ("stat_extends", "stat_rebalances", "stat_window_slots"):
                assert ia[k] == ib[k], (o, k, r_i, ia[k], ib[k])
    assert A.info(0)["capacity"] > cap0
    x = unit12_array(3, col)
    ya, yb = A.mul(x), B.mul(x)
    assert np.allclose(ya, yb, rtol=RTOL, atol=0)


def test_append_memo_survives_runs_on_one_geometry_and_is_dropped_at_extend(dsa, hip, oracle):
    """Several append runs on the SAME handle: the replay's memo (a pure function of the geometry) is reloaded from HBM while the
    capacity is unchanged and rebuilt after _extend! (csrc/appendrun.hip: k_append_run, saved_memo).  Vector runs and matrix runs
    with columns of different lengths (epochs through semaphore cells are keyed by the cell types)."""
    n0 = 300000
    keys0 = np.arange(1, n0 + 1, dtype=np.int64) * 2
    vals0 = unit12_array(3, n0)
    a = dsa.dynamicsparsevec(keys0, vals0, binding=hip)
    b = dsa.dynamicsparsevec(keys0, vals0, binding=oracle)
    nxt = 2 * n0 + 1
    cap0 = a.info()["capacity"]
    extended = False
    for r, cnt in enumerate([3000, 3000, 5000, 700, 80000, 3000, 3000]):       # the 80000 run crosses the extend
        ks = np.arange(nxt, nxt + cnt, dtype=np.int64)
        vs = unit12_array(40 + r, cnt)
        a.set_batch(ks, vs)
        b.set_batch(ks, vs)
        nxt += cnt
        assert_vec_equal(a, b)
        extended = extended or a.info()["capacity"] != cap0
    assert extended
    # matrix: columns streamed in ascending id, 1..9 ascending rows each, four batches on one geometry
    A = dsa.dynamicsparse(fill_mode=False, binding=hip)
    B = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    g = SplitMix64(77)
    col = 0
    for r, ncols in enumerate([900, 900, 2500, 900]):
        I, J = [], []
        for _ in range(ncols):
            col += 1
            rows = sorted({1 + g.next() % 5000 for _ in range(1 + g.next() % 9)})
            I += rows
            J += [col] * len(rows)
        V = unit12_array(60 + r, len(I))
        A.set_batch(I, J, V)
        B.set_batch(I, J, V)
        assert_mat_equal(A, B)
    for o in (0, 1):
        assert not A.check(o)[2:7].any(), A.check(o)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,batches", [(91, [200, 300, 1500, 5000, 40, 9000]), (92, [3000, 3000, 3000])])
def test_new_partitions_by_the_thousand_merge_between_launches(dsa, hip, oracle, seed, batches):
    """Batches that create 100 .. several 1000 new rows AND columns in random key order next to writes to existing ones, from an
    empty matrix on: the first batches run on the local rounds, every batch leaves pending table entries across several launches
    and the grid-wide merge (csrc/tables.hip) brings the tables back to key order between them and before the batch returns."""
    A = dsa.dynamicsparse(fill_mode=False, binding=hip)
    B = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    g = SplitMix64(seed)
    span = 20000
    for r, nb in enumerate(batches):
        I = [int(1 + g.next() % span) for _ in range(nb)]
        J = [int(1 + g.next() % span) for _ in range(nb)]
        V = unit12_array(seed * 10 + r, nb)
        A.set_batch(I, J, V)
        B.set_batch(I, J, V)
        assert_mat_equal(A, B)
        for o in (0, 1):
            assert not A.check(o)[2:7].any(), A.check(o)     # report[6] also covers "no table entry pending outside a batch"
    # a few deletes of whole columns afterwards (tombstones: the literal paths), then more new columns
    for j in sorted({int(1 + g.next() % span) for _ in range(40)}):
        try:
            A.deletecolumn(j)
            ok = True
        except Exception:
            ok = False
        try:
            B.deletecolumn(j)
            okb = True
        except Exception:
            okb = False
        assert ok == okb
    nb = 2000
    I = [int(1 + g.next() % span) for _ in range(nb)]
    J = [int(span + 1 + g.next() % span) for _ in range(nb)]
    V = unit12_array(seed * 10 + 9, nb)
    try:
        A.set_batch(I, J, V); ea = None
    except Exception as e:
        ea = type(e).__name__
    try:
        B.set_batch(I, J, V); eb = None
    except Exception as e:
        eb = type(e).__name__
    assert ea == eb
    if ea is None:
        assert_mat_equal(A, B)


# ---------------------------------------------------------------- round 4: wait policy, allocator entry points, landing-area leases
def test_wait_policy_block_gives_the_same_results(dsa, hip, oracle):
    """dsa_*_set_wait_policy(DSA_WAIT_BLOCK): blocking calls park in hipStreamSynchronize instead of polling pinned memory — same
    kernels, same hand-over, same results: a vector and a matrix driven through writes, lookups, views, slices, deletes and products
    under the blocking policy against the oracle, then back to spinning."""
    g = SplitMix64(99)
    keys = sorted({1 + g.next() % 100000 for _ in range(3000)})
    vals = unit12_array(1, len(keys))
    a = dsa.dynamicsparsevec(keys, vals, binding=hip)
    b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
    a.set_wait_policy(1)
    ks = [1 + g.next() % 100000 for _ in range(2000)]
    vs = [float(g.next() % 4) for _ in ks]
    a.set_batch(ks, vs); b.set_batch(ks, vs)
    a[77] = 2.5; b[77] = 2.5
    assert a[77] == b[77] and a[keys[5]] == b[keys[5]]
    assert_vec_equal(a, b)
    assert np.array_equal(a.nonzeros()[0], b.nonzeros()[0])
    with pytest.raises(dsa.DsaArgumentError):
        a.set_wait_policy(7)
    a.set_wait_policy(0)
    a[78] = 1.5; b[78] = 1.5
    assert_vec_equal(a, b)
    A = dsa.dynamicsparse(fill_mode=False, binding=hip)
    B = dsa.dynamicsparse(fill_mode=False, binding=oracle)
    A.set_wait_policy(1)
    I = [1 + g.next() % 500 for _ in range(4000)]
    J = [1 + g.next() % 300 for _ in range(4000)]
    V = [float(1 + g.next() % 9) for _ in range(4000)]
    A.set_batch(I, J, V); B.set_batch(I, J, V)
    A[3, 4] = 0.0; B[3, 4] = 0.0
    A.deletecolumn(J[0]); B.deletecolumn(J[0])
    assert_mat_equal(A, B)
    assert A.col_view(J[1]) == B.col_view(J[1])
    x = unit12_array(5, 300)
    np.testing.assert_allclose(A.mul(x, dense_out=500), B.mul(x, dense_out=500), rtol=RTOL, atol=0)


def test_pool_idle_bytes_and_trim(dsa, hip):
    """dsa_pool_idle_bytes / dsa_pool_trim: a destroyed structure leaves its HBM blocks idle in the caching allocator; a trim hands
    them back to the driver (a host sharing the card with another allocator); a structure built afterwards is none the worse."""
    keys = np.arange(1, 200001, dtype=np.int64)
    v = dsa.dynamicsparsevec(keys, unit12_array(2, len(keys)), binding=hip)
    v.close()
    idle = dsa.pool_idle_bytes(binding=hip)
    assert idle >= 2 * 200000 * 12, idle
    dsa.pool_trim(1 << 20, binding=hip)
    assert dsa.pool_idle_bytes(binding=hip) <= 1 << 20
    dsa.pool_trim(0, binding=hip)
    assert dsa.pool_idle_bytes(binding=hip) == 0
    w = dsa.dynamicsparsevec(keys, unit12_array(2, len(keys)), binding=hip)
    assert w.nnz() == len(keys) and w[777] == unit12_array(2, len(keys))[776]


def test_many_small_vectors_lease_their_landing_area(dsa, hip):
    """2000 live small vectors, each built by the one-launch small builder and read once: the pinned landing area of those operations
    is leased per operation (not held per handle), so values and layouts are right however the leases interleave."""
    vs = []
    for i in range(2000):
        k = np.arange(1, 6, dtype=np.int64) * (i + 1)
        vs.append(dsa.dynamicsparsevec(k, np.full(5, float(i + 1)), binding=hip))
    for i in (0, 1, 999, 1999):
        kk, vv = vs[i].nonzeros()
        assert np.array_equal(kk, np.arange(1, 6, dtype=np.int64) * (i + 1)) and np.all(vv == float(i + 1))
        assert vs[i][3 * (i + 1)] == float(i + 1)


def test_pool_cap_from_the_environment_is_honoured(dsa, hip):
    """DSA_POOL_MAX_MB (read when the library is loaded) caps the idle HBM the caching allocator keeps: in a child process with a
    64 MB cap a destroyed 200 MB structure leaves at most 64 MB behind."""
    import subprocess
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import dsa_loader
dsa = dsa_loader.load(); hip = dsa.product()
keys = np.arange(1, 6_000_001, dtype=np.int64)
v = dsa.dynamicsparsevec(keys, np.ones(len(keys)), binding=hip)          # 2 x 2^24 slots x 12 B = 400 MB of slot buffers
held = v.info()["hbm_bytes"]
v.close()
idle = dsa.pool_idle_bytes(binding=hip)
assert held > 300e6, held
assert idle <= 64 << 20, (idle, held)
print("ok", idle)
"""
    env = dict(os.environ, DSA_POOL_MAX_MB="64")
    r = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.gpu
def test_spmv_shared_words_form_is_bit_identical_to_the_plain_form(dsa, hip, tmp_path):
    """k_spmv_gather<SHARE> (waves of a workgroup read the word behind their span from the neighbour's LDS slice, csrc/spmv.hip) adds the
    same terms in the same order as the form without the barrier (DSA_SPMV_SHARE=0): every product of tools/spmv_sharecheck.py's
    matrices with rows shorter than a span must be bit-identical between the two, both orientations, also after deletions; the ragged
    and very long rows (partial sums joined by fp64 atomics in either form) agree to the tolerance of the path."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for share in ("1", "0"):
        f = str(tmp_path / ("y_share%s.npz" % share))
        env = dict(os.environ, DSA_DEV="1", DSA_SPMV_SHARE=share, DSA_SPMV_STREAM="nt")      # (SHARE is the form of the non-temporal instantiations)
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "spmv_sharecheck.py"), f], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "sharecheck wrote" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(np.load(f))
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 28
    shared_used = False
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        if a[k].dtype != np.float64:
            assert np.array_equal(a[k], b[k]), k
        elif k.startswith(("uniform0", "uniform1", "uniform2", "uniform3")):
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k      # every row shorter than a span: one writer, fixed order
        else:
            # rows longer than a 512-slot span are joined with fp64 atomics in either form: equal up to the order of those additions
            np.testing.assert_allclose(a[k], b[k], rtol=RTOL, atol=0, err_msg=k)
        if k.endswith("_cap"):
            shared_used = shared_used or bool((a[k] % 2048 == 0).any())
    assert shared_used          # at least one capacity of whole 2048-slot tiles: the SHARE instantiation ran in the first child


@pytest.mark.gpu
def test_two_deletes_from_a_leaf_whose_last_slot_starts_a_hash_cell(dsa, hip, oracle):
    """Regression (tools/fuzz.py, FUZZ_BIG seed 91098): slots are 1-based, so the LAST slot of a leaf is a multiple of the segment size and —
    for the leaf that ends at slot 12288 — the first slot of the next 4096-slot cell of the resolver's spatial hash (csrc/parbatch.hip).  An op
    that deletes that slot is chained in the next cell; the count bookkeeping of tight footprints walked only the cell of the leaf's FIRST
    slot, let two deletes from that leaf into one round, and the leaf went below its threshold without the rebalance of src/pma.jl:105-141."""
    n = 60007
    keys = np.arange(1, n + 1, dtype=np.int64) * 2
    vals = unit12_array(77, n)
    a = dsa.dynamicsparsevec(keys, vals, binding=hip)
    b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
    assert_vec_equal(a, b)
    K, V, O = b.export_layout()
    inf = b.info()
    assert inf["capacity"] == 131072 and inf["segment_capacity"] == 16        # (above 2^16 slots: the grid rounds, not the one-workgroup rounds)
    leaf = slice(12288 - 16, 12288)
    in_leaf = [int(x) for x in K[leaf][O[leaf].astype(bool)]]
    assert O[12287] == 1 and in_leaf == [11238, 11240, 11242, 11244, 11246, 11248, 11250, 11252]
    for k in in_leaf[:5]:                                                      # 8 -> 3 cells, one call each: the leaf accepts (>= 2), nothing moves
        for v in (a, b):
            v[k] = 0.0
    assert_vec_equal(a, b)
    K, V, O = b.export_layout()
    assert [int(x) for x in K[leaf][O[leaf].astype(bool)]] == [11248, 11250, 11252] and O[12287] == 1
    # one batch = one round of the batch-parallel path: value updates far away (no footprint in common with anything) around the two deletes
    far = np.arange(40000, 40000 + 2 * 298, 2, dtype=np.int64)
    bk = np.concatenate([far[:50], [11250], far[50:150], [11252], far[150:]])
    bv = np.concatenate([unit12_array(78, 50), [0.0], unit12_array(79, 100), [0.0], unit12_array(80, len(far) - 150)])
    reb0 = b.info()["stat_rebalances"]
    for v in (a, b):
        v.set_batch(bk, bv)
    assert b.info()["stat_rebalances"] == reb0 + 1          # the second delete leaves 1 cell < 2: the reference rebalances a wider window
    assert a.info()["stat_par_ops"] >= len(bk) - 8            # ... and the HIP library took the batch through the parallel rounds
    assert_vec_equal(a, b)
    assert a.info()["stat_rebalances"] == b.info()["stat_rebalances"] and a.info()["stat_window_slots"] == b.info()["stat_window_slots"]


@pytest.mark.gpu
def test_same_leaf_fuzz_scenarios_that_found_resolver_bugs(dsa, hip, oracle):
    """tools/fuzz.py run_same_leaf (several count-changing ops per leaf and round, half of them in leaves that end on a hash-cell boundary)
    around the two seeds that exposed resolver bugs of rounds 2-4: 712 (two deletes from a leaf whose last slot starts the next 4096-slot
    hash cell: the count bookkeeping walked one cell only) and 2000 (an insert that falls back to the LEFT because nothing behind it is free
    has read every slot up to the end of the array; its footprint ended at p + 1, so a delete of the last cell shared its round); and the
    seed of run_tombstones that exposed the wrong error code of a batch whose two orientations fail at different writes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FUZZ_ONLY="leaf")
    for first in (700, 1990):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz.py"), "6", str(first)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        done = int(r.stdout.strip().splitlines()[-1].split("scenarios")[0].split()[-1])
        assert done >= 15, r.stdout[-500:]          # the named seed lies within the first 13 scenarios of each run
    # run_tombstones seed 503707: a batch on a matrix with tombstones in BOTH orientations whose rowmajor half fails (the @assert of
    # src/pcsr.jl:132) three writes before its colmajor half does (BoundsError): the reference throws the earlier one
    env = dict(os.environ, FUZZ_ONLY="tomb")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz.py"), "4", "503700"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.strip().splitlines()[-1].split("scenarios")[0].split()[-1]) >= 10, r.stdout[-500:]


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_gloo_rehearsal(dsa, hip, oracle, tmp_path):
    """The N > 1 branch of bench.py — the only code the driver's 8-GPU run executes that no multi-GPU box has ever run — as two fresh child
    processes on the ONE GPU of the test box (DSA_BENCH_SAME_GPU=1: both ranks on cuda:0; DSA_BENCH_BACKEND=gloo: the process group
    without RCCL, which needs one device per rank): config-4-shaped shards (200 000 rows, 25 000 columns per rank), the overlapped timed
    steps, all three reduction schedules of the sum of y.  Checks the JSON line (rccl_ranks, collective_schedules, metric / config) and
    y of every schedule against the CPU oracle's product of the whole matrix.  What stays unmeasured: RCCL itself and xGMI."""
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    ydump = str(tmp_path / "y.npz")
    env = dict(os.environ, DSA_BENCH_SAME_GPU="1", DSA_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    rows, cpg, world = 200_000, 25_000, 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", str(world), "--config", "c4", "--rows", str(rows),
           "--cols-per-gpu", str(cpg), "--steps", "3", "--warmup", "1", "--full", "--all-schedules", "--dump-y", ydump,
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]               # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d["metric"] == "spmv_gbps_10M_nnz_pcsr" and d["n_gpus"] == world and d["rccl_ranks"] == world and d["steps"] == 3
    assert d["scaling"] == "weak" and d["config"]["name"] == "c4" and d["config"]["sharding"] == "column-range x2"
    assert d["value"] > 0 and d["roofline"]["frac"] > 0 and d["ms_per_step"] >= d["roofline"]["kernel_ms"] * 0.98
    cs = d["collective_schedules"]
    assert cs["local_spmv_ms"] > 0
    for name in ("all_reduce", "rs_ag", "direct"):
        assert isinstance(cs[name + "_ms"], float) and cs[name + "_ms"] > 0, (name, cs)
    # y of every schedule == the oracle's product of the WHOLE matrix on the same inputs (the ranks' column ranges side by side)
    n_total = world * cpg
    I, J, V = [], [], []
    for rk in range(world):
        i_, j_, v_ = bench.c3_triplets(rows, cpg, 10, rk * cpg, seed_rows=8, seed_vals=9)
        I.append(i_); J.append(j_); V.append(v_)
    I, J, V = np.concatenate(I), np.concatenate(J), np.concatenate(V)
    x = bench.unit12(10, n_total)
    ref = dsa.dynamicsparse(I, J, V, rows, n_total, binding=oracle).mul(x, dense_out=rows)
    got = np.load(ydump)
    assert set(got.files) >= {"all_reduce", "rs_ag", "direct"}
    for name in got.files:
        np.testing.assert_allclose(got[name], ref, rtol=1e-12, atol=0, err_msg=name)
    # --dump-outputs: y of the last timed step (the overlapped all_reduce schedule), as rank 0 received it
    y_last = np.load(str(tmp_path / "out" / "y.npy"))
    assert y_last.dtype == np.float64
    np.testing.assert_allclose(y_last, ref, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_the_last_y(dsa, hip, oracle, tmp_path):
    """A plain `bench.py --gpus 1` (no --full) on a small C3-shaped matrix: one result line with the headline fields, none of the legs
    that --full adds, and --dump-outputs writes y of the last timed step, equal to the CPU oracle's product on the same inputs."""
    import subprocess
    sys.path.insert(0, ROOT)
    import bench
    rows, cols = 30_000, 20_000
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c3", "--rows", str(rows), "--cols-per-gpu", str(cols),
           "--steps", "4", "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "spmv_gbps_10M_nnz_pcsr" and d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] - d["roofline"]["algorithmic_bytes"] / (d["ms_per_step"] * 1e-3) / 1e9) / d["value"] < 0.01
    for k in ("cpu_baseline", "inserts_per_s", "roofline_rebalance", "c5_streaming", "collective_schedules"):
        assert k not in d, k
    assert "cold_kernel_ms" not in d["roofline"] and d["roofline"]["kernel_ms_event_pair_per_launch"] is None
    assert sorted(os.listdir(out_dir)) == ["y.npy"]
    y = np.load(str(out_dir / "y.npy"))
    assert y.dtype == np.float64 and y.shape == (rows,)
    I, J, V = bench.c3_triplets(rows, cols, 10, 0, seed_rows=5, seed_vals=6)
    ref = dsa.dynamicsparse(I, J, V, rows, cols, binding=oracle).mul(bench.unit12(7, cols), dense_out=rows)
    np.testing.assert_allclose(y, ref, rtol=RTOL, atol=0)


@pytest.mark.gpu
def test_release_library_ignores_development_switches(dsa, hip, oracle):
    """include/dsa.h, release configuration: DSA_TIGHT=0 (no tight footprints: ~twice the rounds for uniformly random inserts) changes
    nothing unless DSA_DEV=1 is set as well — a parity-critical path cannot be selected by whatever environment the host inherits."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import dsa_loader
from util import splitmix_array, unit12_array
dsa = dsa_loader.load(); hip = dsa.product()
n0 = 700000
v = dsa.dynamicsparsevec(np.arange(1, n0 + 1, dtype=np.int64) * 2, unit12_array(3, n0), binding=hip)
odd = np.unique(1 + 2 * (np.array(splitmix_array(4, 60000), dtype=np.uint64) % np.uint64(700000)).astype(np.int64))[:50000]
np.random.default_rng(4).shuffle(odd)
v.set_batch(odd, unit12_array(4, len(odd)))
inf = v.info()
print("ROUNDS", inf["stat_par_rounds"], inf["nb_elements"], dsa.dev_switches(hip)[1])
"""
    res = {}
    # (DSA_RUN_AHEAD=0 with it: the prefix rule of rounds 2-5 — with run-ahead rounds the tight footprints alone change the count by a quarter only)
    for tag, extra in (("default", {}), ("tight0_release", {"DSA_TIGHT": "0", "DSA_RUN_AHEAD": "0"}), ("tight0_dev", {"DSA_TIGHT": "0", "DSA_RUN_AHEAD": "0", "DSA_DEV": "1"})):
        env = {k: v for k, v in os.environ.items() if k not in ("DSA_DEV", "DSA_TIGHT", "DSA_RUN_AHEAD")}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", code, root], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        f = [ln for ln in r.stdout.splitlines() if ln.startswith("ROUNDS")][0].split()
        res[tag] = (int(f[1]), int(f[2]), f[3])
    assert res["default"][0] == res["tight0_release"][0] and res["tight0_release"][2] == "False", res
    assert res["tight0_dev"][0] > 1.3 * res["default"][0] and res["tight0_dev"][2] == "True", res
    assert res["default"][1] == res["tight0_dev"][1]


def _run_child(cmd, env, timeout=600):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=root)


@pytest.mark.gpu
def test_footprint_check_build_fires_on_the_two_resolver_bugs_of_round_4_and_is_clean_on_the_tree(dsa, hip, oracle):
    """csrc/pb_fpcheck.h, -DDSA_FP_CHECK (libdsa_hip_fpcheck.so): the soundness of a round of the batch-parallel writes checked mechanically —
    mode 1 re-derives the resolver's verdict by brute force from what every plan literally scanned and counted and every apply touched, mode 2
    applies the prefix one op after the other and requires each op's plan, recomputed on the live state, to equal the plan the round was
    resolved on.  (a) Both modes FAIL on the two libraries that re-introduce the resolver defects of round 4 (DSA_FP_REGRESS=1: the leaf
    walk of one hash cell — two deletes from one leaf in one round; =2: the footprint of a left-falling insert ending at p + 1), on the
    scenarios that found them.  (b) Both modes are clean on the tree: the same scenarios, the default fuzzer mix, the same-leaf scenarios."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "dynamicsparsearrays.jl_amd", "csrc")
    fuzz = [sys.executable, os.path.join(root, "tools", "fuzz.py")]
    leaf_test = [sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_hip_parity.py"), "-m", "gpu", "-x", "-q", "-k", "two_deletes_from_a_leaf"]
    for mode in ("1", "2"):
        env = dict(os.environ, DSA_DEV="1", DSA_LIBRARY=os.path.join(csrc, "libdsa_hip_fpcheck_bug1.so"), DSA_FP_MODE=mode)
        r = _run_child(leaf_test, env)
        assert r.returncode != 0 and "DSA_FP_CHECK" in r.stdout + r.stderr, (mode, r.stdout[-1500:])
        env = dict(os.environ, DSA_DEV="1", DSA_LIBRARY=os.path.join(csrc, "libdsa_hip_fpcheck_bug2.so"), DSA_FP_MODE=mode, FUZZ_ONLY="leaf")
        r = _run_child(fuzz + ["8", "1990"], env)
        assert r.returncode != 0 and "DSA_FP_CHECK" in r.stdout + r.stderr, (mode, r.stdout[-1500:])
        env = dict(os.environ, DSA_DEV="1", DSA_LIBRARY=os.path.join(csrc, "libdsa_hip_fpcheck.so"), DSA_FP_MODE=mode)
        r = _run_child(leaf_test, env)
        assert r.returncode == 0, (mode, r.stdout[-2500:])
        r = _run_child(fuzz + ["6", "1990"], dict(env, FUZZ_ONLY="leaf"))
        assert r.returncode == 0 and "fuzz done" in r.stdout and "DSA_FP_CHECK" not in r.stdout, (mode, r.stdout[-2500:] + r.stderr[-1500:])
        r = _run_child(fuzz + ["15", str(31000 + int(mode))], env)
        assert r.returncode == 0 and "fuzz done" in r.stdout and "DSA_FP_CHECK" not in r.stdout, (mode, r.stdout[-2500:] + r.stderr[-1500:])


@pytest.mark.gpu
def test_grid_rebalance_that_never_gets_its_prefix_raises_ehip_instead_of_hanging():
    """k_move2 (csrc/rebalance.hip) lets a workgroup wait for prefix words published by workgroups with a lower index — deadlock-free as
    long as the hardware dispatches a 1-D grid in order.  The wait is bounded all the same: a workgroup that gives up raises a fault word
    and carries on, and the next check of the structure reports DSA_EHIP.  Provoked here with the development switches (group totals
    never published, 4096 polls instead of 2^24): the launch must come back, the checker must raise EHIP, the process must live on and
    a fresh structure must still work."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import dsa_loader
dsa = dsa_loader.load(); hip = dsa.product()
n = 1_300_000                                   # capacity 2^21: 1024 tiles, 16 groups of 64 — every tile behind the first group waits
keys = np.arange(1, n + 1, dtype=np.int64) * 3
v = dsa.dynamicsparsevec(keys, np.ones(n), binding=hip)
assert v.info()["capacity"] == 1 << 21
v.check()                                       # the build spreads a PACKED source: closed-form prefixes, nobody waits
v.rebalance_root()                              # a general source: the prefix table is needed and never completed
try:
    v.check()
    print("no error raised")
except dsa.DsaError as e:
    print("raised", e.code)
    assert e.code == 7          # DSA_EHIP (include/dsa.h)
del v
w = dsa.dynamicsparsevec(np.arange(1, 5001, dtype=np.int64), np.ones(5000), binding=hip)      # small: one workgroup per window, no table
w.set_batch(np.arange(5001, 6001, dtype=np.int64), np.ones(1000))
w.check()
print("ok")
"""
    env = dict(os.environ, DSA_DEV="1", DSA_DBG_MOVE2="24")
    r = subprocess.run([sys.executable, "-c", code, root], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "raised" in r.stdout and r.stdout.strip().endswith("ok"), r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.gpu
def test_concurrent_grid_rebalances_on_the_twin_streams_and_other_handles(dsa, hip, oracle):
    """k_move2 (csrc/rebalance.hip) lets a workgroup wait for status words of LOWER block indices of its own launch — deadlock-free as long as
    the workgroups of a launch start in index order, whatever else runs on the chip.  Here up to six launches of it are in flight at once:
    one orientation each of two 2^21-slot matrices (every handle on its own streams, one host thread per handle) and two 2^20-slot vectors on theirs, 25
    root rebalances each, while a third thread keeps a write batch running — then every layout must still equal the oracle's (a root rebalance
    is layout-idempotent) and no launch may have raised its fault word (dsa_*_check turns it into DSA_EHIP)."""
    import threading
    m = n = 200_000
    I = 1 + (np.array(splitmix_array(91, 1_000_000), dtype=np.uint64) % np.uint64(m)).astype(np.int64)
    J = 1 + (np.array(splitmix_array(92, 1_000_000), dtype=np.uint64) % np.uint64(n)).astype(np.int64)
    V = unit12_array(93, 1_000_000)
    a = dsa.dynamicsparse(I, J, V, m, n, binding=hip)
    a2 = dsa.dynamicsparse(I, J, V, m, n, binding=hip)          # (a handle is single-writer: one thread per handle)
    b = dsa.dynamicsparse(I, J, V, m, n, binding=oracle)
    assert a.info(dsa.COLMAJOR)["capacity"] >= 1 << 21
    kv = np.arange(1, 700_001, dtype=np.int64) * 2
    vecs = [dsa.dynamicsparsevec(kv, unit12_array(94 + q, len(kv)), binding=hip) for q in range(2)]
    vref = [dsa.dynamicsparsevec(kv, unit12_array(94 + q, len(kv)), binding=oracle) for q in range(2)]
    w = dsa.dynamicsparsevec(kv[:200_000], np.ones(200_000), binding=hip)
    errors = []

    def guard(fn):
        def run():
            try:
                fn()
            except Exception as e:      # noqa: BLE001 — reported by the main thread
                errors.append(repr(e))
        return run

    def reb_mat(o):
        for _ in range(25):
            (a if o == dsa.COLMAJOR else a2).rebalance_root(o)

    def reb_vec(v):
        for _ in range(25):
            v.rebalance_root()

    def writer():
        odd = 1 + 2 * (np.array(splitmix_array(97, 60_000), dtype=np.uint64) % np.uint64(200_000)).astype(np.int64)
        for q in range(6):
            w.set_batch(odd[q * 10_000:(q + 1) * 10_000], np.full(10_000, 2.0))

    threads = [threading.Thread(target=guard(lambda o=o: reb_mat(o))) for o in (dsa.COLMAJOR, dsa.ROWMAJOR)]
    threads += [threading.Thread(target=guard(lambda v=v: reb_vec(v))) for v in vecs]
    threads.append(threading.Thread(target=guard(writer)))
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        b.rebalance_root(o)
    a.rebalance_root(dsa.ROWMAJOR); a2.rebalance_root(dsa.COLMAJOR)
    assert_mat_equal(a, b)
    assert_mat_equal(a2, b)
    for v, r in zip(vecs, vref):
        r.rebalance_root()
        assert_vec_equal(v, r)
    import ctypes as C
    rep = (C.c_int64 * 8)()
    for o in (dsa.COLMAJOR, dsa.ROWMAJOR):
        hip.call("mat_check", a.h, o, rep)
        assert list(rep)[2:7] == [0, 0, 0, 0, 0], list(rep)
    for v in vecs + [w]:
        hip.call("vec_check", v.h, rep)
        assert list(rep)[2:7] == [0, 0, 0, 0, 0], list(rep)
