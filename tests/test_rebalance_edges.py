"""The grid-wide rebalance kernel k_move2 (csrc/rebalance.hip) at its tile, group and gap-geometry edges.

Every structural change of a PMA ends in this kernel: the root rebalance, _extend! / _shrink!, the pack + spread of an interior
window too wide for the LDS paths, and the spread that finishes every bulk build.  A source tile is 2048 slots, 64 tiles form a
group with one prefix table entry, the write phase works on groups of 128 destination offsets, and the gap positions
D(k) = floor(fl(k * fl(W / E))) are inverted by a guess and a fix-up.  Nothing is computed, only moved: every comparison below is
exact (keys, occupancy and tables equal, values bit for bit).

1. The reference is a numpy model written from pack! / spread! (src/moves.jl:94-171).  The unmarked tests validate it on the CPU
   against the oracle's pack + spread for EVERY case list the GPU tests use (the lists are module-level, both sides share them),
   against a literal transcription of spread!'s backward loop, and check that the closed-form gap offsets are distinct and inside
   the window.
2. GPU, one launch, general source in place (parity hook, engine GRID): a window inside a larger array.
3. GPU, the write path's own window_rebalance (engine GRID_WINDOW): pack launch + packed-spread launch, m == 0, the root branch.
4. GPU, destination != source: _extend!, _shrink! and pack through restored vector layouts (dsa_vec_dev_relayout).
5. GPU, the foreign packed source of the bulk build at n = 2048 k +- 1 and at the group edge."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest

from rawhooks import GRID, GRID_WINDOW, P_F64, P_I64, P_U8, Raw

TILE = 2048                      # source slots per workgroup
GROUP = 64 * TILE                # source slots per prefix-table group
LEAD, TAIL = 192, 128            # slots in front of / behind the window: ws - 1 = 192 is a multiple of 64 but not of 2048
WIDE_OFF = 1 << 40

PLACEMENTS = ["rand", "left", "right", "ends", "alternate", "full_tiles", "last_tile_empty"]
KEYS = [False, True]
KEY_IDS = ["keys32", "keys64"]

# (W, m) with W >= 2^16 and floor(fl(k * fl(W / E))) != floor(k W / E) for some k, found by a CPU search over 400 random m per
# width with the model below (test_fp_edge_pairs_really_are_edges recomputes the property)
FP_LARGE = [(63 * TILE, 752), (64 * TILE, 4404), (64 * TILE + 64, 20704), (65 * TILE, 3328), (129 * TILE, 10464)]
# the pairs of the raw-primitive test that fall on a width used here
FP_SMALL = [(64, 15), (128, 25), (128, 21)]

GRID_WIDTHS = [64, 128, 192, 1984, 2048, 2112, 4096, 4160, 63 * TILE, 64 * TILE, 64 * TILE + 64, 65 * TILE, 129 * TILE]
WINDOW_WIDTHS = sorted([W for W in GRID_WIDTHS if W >= 2048] + [16384])


def m_list(W, extra=()):
    """cell counts for a W-slot window: the full list up to 16384 slots, the fixed sub-list from 63 tiles on"""
    if W >= 63 * TILE:
        ms = [1, 129, 2047, 2049, W // 2, W - 129, W - 128, W - 1, W]
    else:
        ms = [1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, W // 2, W - 129, W - 128, W - 65, W - 64, W - 1, W]
    ms += list(extra) + [m for w, m in FP_LARGE + FP_SMALL if w == W]
    return sorted({m for m in ms if 1 <= m <= W})


def n_tiles(W):
    return -(-W // TILE)


GRID_CASES = [(W, m, p) for W in GRID_WIDTHS for m in m_list(W) for p in PLACEMENTS]
WINDOW_CASES = [(W, m, p) for W in WINDOW_WIDTHS for m in m_list(W, (4095, 4096, 4097)) for p in PLACEMENTS]
NO_TABLE_CASES = [(2112, 65, "rand"), (4160, 2049, "ends"), (65 * TILE, 65 * TILE - 129, "alternate")]
EMPTY_WINDOWS = [2048, 16384, 65 * TILE]
ROOT_CASES = [(4096, 2049, "rand"), (4160, 129, "right"), (65 * TILE, 65 * TILE // 2, "alternate"), (65 * TILE, 65 * TILE - 1, "left")]
TWICE = [(16384, 129, "rand"), (16384, 4097, "right")]

RELAYOUT_CAPS = [1 << 12, 1 << 17, 1 << 18]
SEG = 16


def relayout_cases():
    out = []
    for ci, cap in enumerate(RELAYOUT_CAPS):
        for mi, m in enumerate([1, 129, 2049, cap // 4, cap // 2 - 1, cap // 2, cap - 1]):
            for wide in KEYS:
                out.append((cap, m, PLACEMENTS[(3 * ci + mi + 3 * wide) % len(PLACEMENTS)], wide))
    return out


RELAYOUT_CASES = relayout_cases()
BUILD_N = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 131071, 131072, 131073]


def case_id(W, m, p):
    return "W%d-%dtiles-m%d-%s" % (W, n_tiles(W), m, p)


def group_id(W, p):
    return "W%d-%dtiles-%s" % (W, n_tiles(W), p)


# one GPU test per (width, placement, key width); the cell counts of the width run inside it
GRID_GROUPS = [(W, p) for W in GRID_WIDTHS for p in PLACEMENTS]
WINDOW_GROUPS = [(W, p) for W in WINDOW_WIDTHS for p in PLACEMENTS]


def key_name(wide):
    return KEY_IDS[int(wide)]


# ------------------------------------------------------------------ the model (src/moves.jl:94-171)
def gap_offsets(W, m):
    """1-based offsets of the E = W - m empty cells spread! leaves in a W-slot window: floor(k * (W / E)), k = 1..E, in Float64
    (next_empty_cell of src/moves.jl:122-124,130)"""
    E = W - m
    if E == 0:
        return np.zeros(0, dtype=np.int64)
    freq = np.float64(W) / np.float64(E)
    return np.floor(np.arange(1, E + 1, dtype=np.float64) * freq).astype(np.int64)


def spread_model(W, m):
    occ = np.ones(W, dtype=np.uint8)
    occ[gap_offsets(W, m) - 1] = 0
    return occ


def rebalance_model(k, v, o, ws, we, dst_w=None, sems=None):
    """pack! of [ws, we] + spread! over [ws, ws + dst_w - 1]: the occupied cells of the source window, in order, on the non-gap
    offsets of the destination window; every other destination slot empty; semaphores[id] = new position of the cell (0, id);
    everything outside the window unchanged (slots behind it keep their distance to its end)"""
    W = we - ws + 1
    dw = W if dst_w is None else dst_w
    src = ws - 1 + np.nonzero(o[ws - 1:we])[0]
    occ_w = spread_model(dw, len(src))
    dst = ws - 1 + np.nonzero(occ_w)[0]
    n = len(o) - W + dw
    k2, v2, o2 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint8)
    for new, old in ((k2, k), (v2, v), (o2, o)):
        new[:ws - 1] = old[:ws - 1]
        new[ws - 1 + dw:] = old[we:]
    k2[dst], v2[dst], o2[dst] = k[src], v[src], 1
    s2 = None
    if sems is not None:
        s2 = sems.copy()
        is_sem = k[src] == 0
        s2[v[src][is_sem].astype(np.int64) - 1] = dst[is_sem] + 1
    return k2, v2, o2, s2


def spread_loop(W, m):
    """spread!(array, 1, W, m) of src/moves.jl:120-140, line for line, on the occupancy alone"""
    occ = [1] * m + [0] * (W - m)
    nb_empty = W - m
    if nb_empty == 0:
        return np.array(occ, dtype=np.uint8)          # i == j at entry: the loop body never runs
    freq = W / nb_empty
    nxt = math.floor(nb_empty * freq)
    i, j = m, W
    while i != j and i >= 1:
        if j == nxt:
            nb_empty -= 1
            nxt = math.floor(nb_empty * freq)
            j -= 1
        else:
            occ[j - 1] = occ[i - 1]
            occ[i - 1] = 0
            i -= 1
            j -= 1
    return np.array(occ, dtype=np.uint8)


# ------------------------------------------------------------------ inputs (vectorised)
def place(W, m, placement, rng):
    """0-based offsets of the m cells inside a W-slot window, ascending"""
    s = np.arange(W)
    tile = s // TILE
    if placement == "left":
        return s[:m]
    if placement == "right":
        return s[W - m:]
    if placement == "ends":                       # half at the front of the first tile, half at the back of the last
        a = (m + 1) // 2
        return np.concatenate([s[:a], s[W - (m - a):]])
    if placement == "full_tiles":                 # whole tiles: the even-numbered ones first, then the odd-numbered
        order = np.concatenate([s[tile % 2 == 0], s[tile % 2 == 1]])
        return np.sort(order[:m])
    if placement == "rand":
        pref = np.ones(W, dtype=bool)
    elif placement == "alternate":                # cells in even-numbered tiles only: tiles without a cell between owners
        pref = tile % 2 == 0
    elif placement == "last_tile_empty":          # the last tile owns the trailing gaps only
        pref = tile < n_tiles(W) - 1
    else:
        raise ValueError(placement)
    first, rest = s[pref], s[~pref]
    if m <= len(first):
        return np.sort(rng.choice(first, size=m, replace=False))
    return np.sort(np.concatenate([first, rest[:m - len(first)]]))      # (more cells than the preferred slots: the rest from the left)


def build_case(W, m, placement, wide, table=True, lead=LEAD, tail=TAIL):
    """a raw array with the window [lead + 1, lead + W] holding m cells in the given placement and sentinel cells around it.
    With a table: every 9th cell of the window and its last cell are semaphores (0, id) — so is its first —, two more sit outside
    the window and the last table entry is a tombstone.  Empty slots hold (0, 0.0), as an export reports them."""
    rng = np.random.default_rng(zlib.crc32(("%d/%d/%s" % (W, m, placement)).encode()))
    n = lead + W + tail
    k, v, o = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint8)
    out = np.concatenate([np.arange(0, lead, 2), np.arange(max(lead - 1, 0), lead), np.arange(lead + W, min(lead + W + 1, n)),
                          np.arange(lead + W + 1, n, 2)]).astype(np.int64)
    out = np.unique(out)
    k[out], v[out], o[out] = 10 ** 6 + out, 0.5 + out, 1
    pos = lead + place(W, m, placement, rng)
    j = np.arange(m)
    k[pos] = 5 + 2 * j + (WIDE_OFF if wide else 0)
    v[pos] = 1.0 + rng.random(m)
    o[pos] = 1
    if not table:
        return k, v, o, None
    sem = j % 9 == 0
    sem[-1:] = True
    ids = [pos[sem] + 1]
    if len(out) > 0:                                  # semaphores outside the window: their table entries must survive
        k[out[[1, -1]]] = 0
        v[out[[1, -1]]] = [1.0, 2.0]
        ids.insert(0, out[[1, -1]] + 1)
    sems = np.concatenate(ids + [np.zeros(1, dtype=np.int64)]).astype(np.int64)
    first_id = len(sems) - 1 - int(sem.sum())
    k[pos[sem]] = 0
    v[pos[sem]] = first_id + 1.0 + np.arange(int(sem.sum()))
    return k, v, o, sems


def same_layout(a, b):
    """occupancy equal slot for slot; keys equal and values bit-identical on the occupied slots"""
    if len(a[2]) != len(b[2]) or not np.array_equal(a[2], b[2]):
        return False
    s = a[2].astype(bool)
    return bool(np.array_equal(a[0][s], b[0][s]) and np.array_equal(a[1][s].view(np.uint64), b[1][s].view(np.uint64)))


def oracle_pack_spread(oracle, k, v, o, ws, we, dst_w, sems):
    """the oracle's pack! over the source window and spread! over the destination window (one call when they coincide)"""
    W = we - ws + 1
    m = int(o[ws - 1:we].sum())
    n = max(len(o), ws - 1 + dst_w)
    kk, vv, oo = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint8)
    kk[:len(o)], vv[:len(o)], oo[:len(o)] = k, v, o
    ss = None if sems is None else sems.copy()
    sp = None if ss is None else ss.ctypes.data_as(P_I64)
    ns = 0 if ss is None else len(ss)

    def call(a, b, do_pack, do_spread):
        rc = oracle.lib.ora_raw_pack_spread(kk.ctypes.data_as(P_I64), vv.ctypes.data_as(P_F64), oo.ctypes.data_as(P_U8), C.c_int64(n),
                                            C.c_int64(a), C.c_int64(b), C.c_int64(m), sp, C.c_int64(ns), C.c_int32(do_pack),
                                            C.c_int32(do_spread))
        assert rc == 0
    if dst_w == W:
        call(ws, we, 1, 1)
    else:
        call(ws, we, 1, 0)
        call(ws, ws + dst_w - 1, 0, 1)
    n_out = len(o) - W + dst_w
    return kk[:n_out], vv[:n_out], oo[:n_out], ss


def relayout_steps(cap, m):
    """(W_src, W_dst) of every launch section 4 makes for one case"""
    steps = [(cap, 2 * cap), (cap, m), (cap, cap)]
    if 2 * m <= cap:
        steps += [(cap, cap // 2), (cap // 2, cap)]
    return steps


def all_wm_pairs():
    """every (destination width, cell count) the GPU tests hand to the kernel"""
    pairs = {(W, m) for W, m, _ in GRID_CASES + WINDOW_CASES + NO_TABLE_CASES + ROOT_CASES + TWICE}
    pairs |= {(m, m) for _, m, _ in WINDOW_CASES}                       # the pack launch: a destination of exactly m slots
    for cap, m, _, _ in RELAYOUT_CASES:
        pairs |= {(wd, m) for _, wd in relayout_steps(cap, m)}
    pairs |= {(build_capacity(n), n) for n in BUILD_N}
    return sorted(pairs)


def build_capacity(n):
    """capacity of a vector built from n cells, as the oracle sizes it (src/pma.jl:69-84); test_model_matches_oracle_bulk_build
    checks every entry against the oracle"""
    return {1: 2, 2: 4, 63: 128, 64: 128, 65: 128, 2047: 4096, 2048: 4096, 2049: 4096, 4095: 8192, 4096: 8192, 4097: 8192,
            131071: 262144, 131072: 262144, 131073: 262144}[n]


# ------------------------------------------------------------------ 1. the model, validated on the CPU
def _model_vs_oracle(oracle, W, m, placement, lead=LEAD, tail=TAIL):
    k, v, o, sems = build_case(W, m, placement, False, lead=lead, tail=tail)
    ws, we = lead + 1, lead + W
    exp = rebalance_model(k, v, o, ws, we, sems=sems)
    ref = oracle_pack_spread(oracle, k, v, o, ws, we, W, sems)
    assert same_layout(exp, ref), (W, m, placement)
    assert np.array_equal(exp[3], ref[3]), (W, m, placement)


@pytest.mark.parametrize("W", sorted(set(GRID_WIDTHS + WINDOW_WIDTHS)), ids=lambda W: "W%d" % W)
def test_model_matches_oracle_pack_spread_on_window_cases(oracle, W):
    cases = sorted({c for c in GRID_CASES + WINDOW_CASES + TWICE if c[0] == W})
    assert cases
    for _, m, placement in cases:
        _model_vs_oracle(oracle, W, m, placement)


def test_model_matches_oracle_on_root_and_tableless_cases(oracle):
    for W, m, placement in ROOT_CASES:
        _model_vs_oracle(oracle, W, m, placement, lead=0, tail=0)
    for W, m, placement in NO_TABLE_CASES:
        k, v, o, _ = build_case(W, m, placement, False, table=False)
        exp = rebalance_model(k, v, o, LEAD + 1, LEAD + W)
        assert same_layout(exp, oracle_pack_spread(oracle, k, v, o, LEAD + 1, LEAD + W, W, None)), (W, m, placement)


@pytest.mark.parametrize("cap", RELAYOUT_CAPS, ids=lambda c: "cap%d" % c)
def test_model_matches_oracle_pack_spread_on_relayout_cases(oracle, cap):
    """destination != source: the oracle packs over the source window, then spreads over the destination window"""
    for _, m, placement, wide in [c for c in RELAYOUT_CASES if c[0] == cap]:
        k, v, o, _ = build_case(cap, m, placement, wide, table=False, lead=0, tail=0)
        for ws_, wd in relayout_steps(cap, m):
            if ws_ != cap:          # the _extend! that follows a _shrink!: its source is the shrunk layout
                k2, v2, o2, _ = rebalance_model(k, v, o, 1, cap, dst_w=ws_)
            else:
                k2, v2, o2 = k, v, o
            exp = rebalance_model(k2, v2, o2, 1, ws_, dst_w=wd)
            ref = oracle_pack_spread(oracle, k2, v2, o2, 1, ws_, wd, None)
            assert len(exp[2]) == wd and same_layout(exp, ref), (cap, m, placement, ws_, wd)


@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
def test_model_matches_oracle_bulk_build(dsa, oracle, wide):
    for n in BUILD_N:
        keys, vals = build_input(n, wide)
        b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
        cap = b.info()["capacity"]
        assert cap == build_capacity(n), n
        k, v, o = b.export_layout()
        assert np.array_equal(o, spread_model(cap, n)), n
        s = o.astype(bool)
        assert np.array_equal(k[s], keys) and np.array_equal(v[s].view(np.uint64), vals.view(np.uint64)), n


def test_model_matches_literal_spread_loop():
    pairs = [(W, m) for W, m in all_wm_pairs() if W <= 1 << 16]
    assert len(pairs) > 150
    for W, m in pairs:
        assert np.array_equal(spread_model(W, m), spread_loop(W, m)), (W, m)


def _gaps_ok(W, m):
    g = gap_offsets(W, m)
    return len(g) == W - m and (len(g) == 0 or (g[0] >= 1 and g[-1] <= W and bool((np.diff(g) > 0).all())))


def test_gap_offsets_are_distinct_and_inside_the_window():
    for W, m in all_wm_pairs():
        assert _gaps_ok(W, m), (W, m)
        assert int(spread_model(W, m).sum()) == m, (W, m)
    for W in (64, 128, 2048, 4096):
        for m in range(1, W + 1):
            assert _gaps_ok(W, m), (W, m)


def test_fp_edge_pairs_really_are_edges():
    """at the listed pairs the Float64 gap offsets differ from the exact floor(k W / E) for some k: a kernel that inverted the
    exact positions would put a gap one slot off"""
    assert len([p for p in FP_LARGE if p[0] >= 1 << 16]) >= 3
    for W, m in FP_LARGE + FP_SMALL:
        E = W - m
        exact = (np.arange(1, E + 1, dtype=np.int64) * W) // E
        assert (gap_offsets(W, m) != exact).any(), (W, m)
        assert any(m == mm for mm in m_list(W)), (W, m)


def test_case_lists_cover_the_edges():
    """the properties the parametrisation ids promise, computed from the case lists themselves"""
    tiles = {n_tiles(W) for W in GRID_WIDTHS}
    assert {1, 2, 3, 63, 64, 65, 129} <= tiles
    assert any(W % TILE not in (0, 64) for W in GRID_WIDTHS) and any(W % TILE == 64 for W in GRID_WIDTHS)
    for cases in (GRID_CASES, WINDOW_CASES):
        for W in {c[0] for c in cases}:
            ms = {c[1] for c in cases if c[0] == W}
            assert {1, W} <= ms and (W < 129 or {129, W - 129, W - 1} <= ms), W
            assert {p for w, _, p in cases if w == W} == set(PLACEMENTS)
    ms = {m for _, m, _ in WINDOW_CASES}
    assert {2047, 2048, 2049, 4095, 4096, 4097} <= ms and any(m % 2 == 1 for m in ms)
    rng = np.random.default_rng(0)
    for W in (4160, 65 * TILE):                 # tiles without a cell: in front (right), between owners (alternate), last
        def per_tile(p, m):
            return np.bincount(place(W, m, p, rng) // TILE, minlength=n_tiles(W))
        assert per_tile("right", 129)[0] == 0 and per_tile("last_tile_empty", 129)[-1] == 0
        assert (per_tile("alternate", 2049)[1::2] == 0).all() and (per_tile("ends", 129)[1:-1] == 0).all()
    c = np.bincount(place(65 * TILE, 4096, "full_tiles", rng) // TILE, minlength=65)
    assert set(c.tolist()) == {0, TILE} and c.sum() == 4096


# ------------------------------------------------------------------ 2. / 3. GPU: windows through the parity hook
def run_window(hip, engine, W, m, placement, wide, table=True, lead=LEAD, tail=TAIL):
    what = (W, m, placement, key_name(wide))
    k, v, o, sems = build_case(W, m, placement, wide, table=table, lead=lead, tail=tail)
    ws, we = lead + 1, lead + W
    exp = rebalance_model(k, v, o, ws, we, sems=sems)
    got = (k.copy(), v.copy(), o.copy(), None if sems is None else sems.copy())
    Raw(hip, engine).rebalance(got[0], got[1], got[2], ws, we, got[3])
    win = slice(ws - 1, we)
    assert int(got[2][win].sum()) == m, what
    assert np.array_equal(got[2][win], exp[2][win]), what
    assert np.array_equal(got[0][win], exp[0][win]), what
    assert np.array_equal(got[1][win].view(np.uint64), exp[1][win].view(np.uint64)), what
    outside = np.ones(len(o), dtype=bool)
    outside[win] = False
    for x, y in zip(got[:3], (k, v, o)):
        assert np.array_equal(x[outside].view(np.uint64 if x.dtype == np.float64 else x.dtype),
                              y[outside].view(np.uint64 if y.dtype == np.float64 else y.dtype)), what
    if sems is not None:
        assert np.array_equal(got[3], exp[3]), what
        inside = (sems >= ws) & (sems <= we)
        assert np.array_equal(got[3][~inside], sems[~inside]), what
        if lead > 0:
            assert got[3][0] > 0 and got[3][1] > we and got[3][-1] == 0, what
        cells = np.nonzero(got[2][win])[0]
        assert got[0][ws - 1 + cells[0]] == 0 and got[0][ws - 1 + cells[-1]] == 0, what   # first and last cell: semaphores


@pytest.mark.gpu
@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("W,placement", GRID_GROUPS, ids=[group_id(*c) for c in GRID_GROUPS])
def test_grid_single_launch_in_place(hip, W, placement, wide):
    """one launch, general source, destination = the same window (of the alternate buffer, copied back by the hook); every cell
    count of m_list(W): 1 (E = W - 1) ... W (E = 0), around the word, the 128-offset group and the tile, the Float64 edge pairs"""
    ms = [m for w, m, p in GRID_CASES if w == W and p == placement]
    assert ms == m_list(W)
    for m in ms:
        run_window(hip, GRID, W, m, placement, wide)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("engine", [GRID, GRID_WINDOW], ids=["grid", "grid-window"])
def test_window_without_a_semaphore_table(hip, engine, wide):
    for W, m, placement in NO_TABLE_CASES:
        run_window(hip, engine, W, m, placement, wide, table=False)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("W,placement", WINDOW_GROUPS, ids=[group_id(*c) for c in WINDOW_GROUPS])
def test_production_interior_window(hip, W, placement, wide):
    """window_rebalance as the write path calls it: the pack launch (general source -> a destination of exactly m slots, E = 0,
    odd widths among them) and the spread launch (PACKED source of m cells, semaphore updates); every cell count of
    m_list(W, (4095, 4096, 4097)): the PACKED counts 2048 k - 1, 2048 k, 2048 k + 1 for k = 1, 2 among them"""
    ms = [m for w, m, p in WINDOW_CASES if w == W and p == placement]
    assert ms == m_list(W, (4095, 4096, 4097))
    for m in ms:
        run_window(hip, GRID_WINDOW, W, m, placement, wide)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("W", EMPTY_WINDOWS, ids=lambda W: "W%d" % W)
def test_production_window_without_cells(hip, W, wide):
    """m == 0: the window's occupancy is cleared, nothing else changes"""
    k, v, o, sems = build_case(W, 1, "left", wide)
    o[LEAD] = 0
    k[LEAD] = 0
    v[LEAD] = 0.0
    sems[-2] = 0                                     # (the cell that was removed: a tombstone)
    got = (k.copy(), v.copy(), o.copy(), sems.copy())
    Raw(hip, GRID_WINDOW).rebalance(got[0], got[1], got[2], LEAD + 1, LEAD + W, got[3])
    assert int(got[2][LEAD:LEAD + W].sum()) == 0, (W, key_name(wide))
    assert same_layout(got, (k, v, o)) and np.array_equal(got[3], sems), (W, key_name(wide))


@pytest.mark.gpu
@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("W,m,placement", ROOT_CASES, ids=[case_id(*c) for c in ROOT_CASES])
def test_production_window_is_the_whole_array(hip, W, m, placement, wide):
    """ws == 1, we == len: window_rebalance hands over to the root rebalance (the other buffer becomes current)"""
    run_window(hip, GRID_WINDOW, W, m, placement, wide, lead=0, tail=0)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
def test_two_windows_one_after_the_other(hip, wide):
    """arrays of one size, rebalanced back to back in one process: the hook's temporary structures share pooled buffers, never a
    status generation or a scratch content"""
    for W, m, placement in TWICE + TWICE[:1]:
        run_window(hip, GRID_WINDOW, W, m, placement, wide)


# ------------------------------------------------------------------ 4. GPU: destination != source through restored layouts
def _is_layout(vec, exp, what):
    got = vec.export_layout()
    assert len(got[2]) == len(exp[2]), what
    assert np.array_equal(got[2], exp[2]), what
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.uint64), exp[1].view(np.uint64)), what
    assert not vec.check()[2:7].any(), (what, vec.check())


@pytest.mark.gpu
@pytest.mark.parametrize("cap,m,placement,wide", RELAYOUT_CASES,
                         ids=["cap%d-m%d-%s-%s" % (c, m, p, key_name(w)) for c, m, p, w in RELAYOUT_CASES])
def test_extend_shrink_pack_of_restored_layouts(dsa, hip, cap, m, placement, wide):
    k, v, o, _ = build_case(cap, m, placement, wide, table=False, lead=0, tail=0)
    what = (cap, m, placement, key_name(wide))

    def fresh():
        a = dsa.import_vector_layout(k, v, o, SEG, binding=hip)
        assert not a.check()[2:7].any(), what
        return a
    # _extend!: capacity doubled (src/pma.jl:143-151)
    a = fresh()
    hip.call("vec_dev_relayout", a.h, 3)
    assert a.info()["capacity"] == 2 * cap, what
    _is_layout(a, rebalance_model(k, v, o, 1, cap, dst_w=2 * cap), what + ("extend",))
    # pack!: the cells on slots 1..m, nothing behind them up to the capacity; then the root rebalance
    a = fresh()
    hip.call("vec_dev_relayout", a.h, 1)
    assert a.info()["capacity"] == cap, what
    packed = rebalance_model(k, v, o, 1, cap, dst_w=m)
    got = a.export_layout()
    assert np.array_equal(got[2][:m], np.ones(m, dtype=np.uint8)) and not got[2][m:].any(), what + ("pack",)
    assert np.array_equal(got[0][:m], packed[0]) and np.array_equal(got[1][:m].view(np.uint64), packed[1].view(np.uint64)), what + ("pack",)
    assert not a.check()[2:7].any(), what + ("pack",)
    a.rebalance_root()
    _is_layout(a, rebalance_model(k, v, o, 1, cap), what + ("root",))
    # _shrink!: capacity halved (src/pma.jl:153-161; m == cap / 2: no gap left), then _extend! back over the stale upper half
    if 2 * m <= cap:
        a = fresh()
        hip.call("vec_dev_relayout", a.h, 4)
        assert a.info()["capacity"] == cap // 2, what
        half = rebalance_model(k, v, o, 1, cap, dst_w=cap // 2)
        _is_layout(a, half, what + ("shrink",))
        hip.call("vec_dev_relayout", a.h, 3)
        assert a.info()["capacity"] == cap, what
        back = rebalance_model(half[0], half[1], half[2], 1, cap // 2, dst_w=cap)
        _is_layout(a, back, what + ("shrink, extend",))
        assert same_layout(back, rebalance_model(k, v, o, 1, cap)), what


# ------------------------------------------------------------------ 5. GPU: the bulk build's foreign PACKED source
def build_input(n, wide):
    keys = np.arange(1, n + 1, dtype=np.int64) * 3 + (WIDE_OFF if wide else 0)
    vals = 1.0 + np.random.default_rng(n).random(n)
    return keys, vals


@pytest.mark.gpu
@pytest.mark.parametrize("wide", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("n", BUILD_N, ids=lambda n: "n%d" % n)
def test_bulk_build_spread_matches_oracle_and_model(dsa, hip, oracle, n, wide):
    keys, vals = build_input(n, wide)
    a = dsa.dynamicsparsevec(keys, vals, binding=hip)
    b = dsa.dynamicsparsevec(keys, vals, binding=oracle)
    cap = a.info()["capacity"]
    what = (n, cap, key_name(wide))
    assert cap == b.info()["capacity"] == build_capacity(n), what
    got, ref = a.export_layout(), b.export_layout()
    assert same_layout(got, ref), what
    assert np.array_equal(got[2], spread_model(cap, n)), what
    assert not a.check()[2:7].any(), what
