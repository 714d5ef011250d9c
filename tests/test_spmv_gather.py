"""k_spmv_gather (csrc/spmv.hip) in each of its forms, at the edges of its slot geometry and of the zero fill; k_spmv_scatter over the
same catalogue.

The kernel is compiled as WIDE x NT x ZFILL x SHARE.  The host picks the form (dsa_host.hip: spmv_dev, spmv.hip: launch_gather_t):
  WIDE   the gathered orientation keeps 64-bit keys: some stored inner key lies outside Int32 (the rule of KeyArr);
  NT     8 * nx > 3 MiB, i.e. nx >= 393 217: non-temporal slot streams;
  ZFILL  tables in key order without tombstones, longest extent <= 512 slots, largest key gap, first key and ny - last key <= 4096:
         y is not zeroed in front of the launch, the owner of a semaphore zeroes the rows in front of it;
  SHARE  NT and the capacity a whole number of 2048-slot tiles.
Which form ran: ZFILL from the `stat_spmv_nomemset` delta of every product; NT from the test's own nx; SHARE from NT and
info()["capacity"] % 2048; WIDE from the inputs (one cell with the inner key 2**33), confirmed by info()["hbm_bytes"]: both slot
buffers of the orientation grow by four bytes per slot against the same matrix with that key replaced by a small one.

Every product goes through mat_spmv_dense_dev on the handle's stream into a y of ny + 64 words pre-filled with NaN, twice into the
same y without a refill, on a fresh handle with at most two products per (nx, ny) (`stat_spmv_plan` must not move).  After either
product the 64 guard words are NaN bit for bit and no word of y[:ny] is.  Where one wave writes a row (extent <= 512) the second
result equals the first bit for bit: an atomic path that ran without its memset would double the row.

Reference: computed here from the input triples, never by the library.  Per row p_i = v_i * x[j_i - 1] in numpy (cells whose column
lies outside 1..nx add nothing), ref = math.fsum(p), and |y - ref| <= (c + 1) * 2**-53 * sum|p_i| with c the number of products: the
bound of recursive summation of c rounded products in any order (c - 1 additions) plus the rounding of ref itself.  It covers the
left fold, the wave reduction and the atomic joins alike.  A row without products is +0.0 bit for bit.  On top of it, a row whose
span holds more than 4 semaphores and that ends within the span's nine words is summed by one lane left to right: such rows are
compared bit for bit with the CPU oracle's own product, which adds in the reference's order (src/operations.jl:101).  The
classification restates the kernel's constants (512, 9 words, 4) and only chooses the rows that get the stricter check.

Geometry comes from the oracle, whose slot layout is the library's (asserted again here for every case): semaphore slot, extent
(next semaphore - own; the last one: capacity + 1 - own, the definition of k_spmv_meta), semaphores per span.  test_oracle_alone
asserts on the CPU that every situation below is present in the committed inputs, that the host's rule gives the path each case
expects, and that the fsum reference agrees with the oracle's product within the bound.

Catalogue (every case as A * x and, built transposed, as A' * x; forms as WIDE NT ZFILL SHARE):
  g1        3000 rows of 1..3 cells, ~94 semaphores per span (second trip of the lane loop), gaps of one key     0010 0111
  g1w       g1 + one cell with the inner key 2**33                                                                1010 1111
  g2        rows of 20..120 cells and one of 700: spans with exactly 4, exactly 5 and 0 semaphores                0000
  g3        semaphores in slot 1, in the first / last slot of a span, in the last slot of a tile (the next span
            is wave 0 of another workgroup), a row in front that ends on the span border, the last cell in the
            last slot of the array                                                                                0010 0111
  g4_512    unique longest extent 512, semaphore at offset 422: closed by the overrun loop behind the ninth word  0010 0111
  g4_512f   extent 512 from offset 5: ends in the ninth word, the only semaphore of its span sits in the last word
            the next wave's backward search of 8 words reads                                                      0010 0111
  g4_512l   extent 512 from offset 500: ends in the last word the overrun loop reads                              0010 0111
  g4_513    the neighbour input of g4_512, extent 513: memset path                                                0000 0101
  g4_512w / g4_513w   with the 2**33 cell                                                                          1010 1111 / 1000 1101
  g5        rows of extent (512, 1024], (1024, 2560] and above 2560 + 512 (the backward scans of 8 + 32 words give
            up, carry_in_partition bisects the table); a long row first, last, and across a tile border; the longest
            one starts in the first word of its span: the last word of the 8-word and of the 32-word search       0000 0101
  g5d       g5 after deleterow of short rows: tombstone runs on the bisection's midpoints                         0000 0101
  g6_*      MAX_FILL = 4096 from both sides: key gap, first key, ny - last key (4096: ZFILL, 4097: memset); then
            with ZFILL: ny inside a gap below the last key, ny = last key, ny = 1 (first key 1 and 5), ny = 0, nx below
            the largest column key, column keys -3 and -1                                                         0010 / 0000
  tiny*     one partition, one cell, capacity below a tile, nx = 393 217: NT without SHARE; _far: ny - key = 4097;
            w: with the 2**33 cell                                                                                0110 0100 1110 1100
  g8        70 000 rows of one cell, 128 tiles: the XCD tile map, rows on both sides of its seven seams           0010 0111
Unreachable: the four forms with SHARE and without NT (launch_gather_t asks for NT first).  The other twelve are reached; the
table FORMS below is asserted against the oracle's capacities on the CPU and against the library's on the GPU.
"""
import ctypes as C
import math

import numpy as np
import pytest

from util import splitmix_array, unit12_array

COLMAJOR, ROWMAJOR = 0, 1
SPAN, TILE, NINE_WORDS, COOP, MAX_FILL = 512, 2048, 576, 4, 4096
NX_PLAIN = (3 << 20) // 8            # 393 216: the largest x that keeps the plain stream
NX_NT = NX_PLAIN + 1
GUARD = 64
U = 2.0 ** -53
WIDE_KEY = 2 ** 33


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def signed(a, seed):
    """every other value or so negated"""
    return a * (1.0 - 2.0 * (splitmix_array(seed, len(a)) & np.uint64(1)).astype(np.float64))


_x_all = []


def x_of(nx):
    if not _x_all:
        _x_all.append(signed(unit12_array(77, NX_NT), 78))
    return _x_all[0][:nx]


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, keys, lens, width, ny, nxs, zfill, extra=(), append=(), delete=(), strict_min=None):
        self.name, self.width, self.ny, self.nxs, self.zfill = name, width, ny, tuple(nxs), zfill
        self.keys, self.lens = np.asarray(keys, np.int64), np.asarray(lens, np.int64)
        self.extra, self.append, self.delete = tuple(extra), tuple(append), tuple(delete)      # append: cells written behind the build
        self.strict_min = strict_min
        assert len(self.keys) == len(self.lens) and np.all(np.diff(self.keys) > 0) and np.all(self.lens >= 1)

    @property
    def wide(self):
        return any(abs(j) > 2 ** 31 for _, j in self.extra)


CASES = {}


def narrow_twin(c):
    """the same matrix with the 2**33 key replaced by a small one behind every column: the same layout in 32-bit keys"""
    return Case(c.name, c.keys, c.lens, c.width, c.ny, c.nxs, c.zfill, extra=tuple((i, NX_NT + 7 if j == WIDE_KEY else j) for i, j in c.extra))


def case(*a, **kw):
    c = Case(*a, **kw)
    CASES[c.name] = c
    return c


def _g1_keys():
    r = np.arange(3000)
    return 6 + r + r // 7


BOTH = (NX_PLAIN, NX_NT)
case("g1", _g1_keys(), 1 + np.arange(3000) % 3, NX_PLAIN, int(_g1_keys()[-1]) + 40, BOTH, True, strict_min=0.95)
case("g1w", _g1_keys(), 1 + np.arange(3000) % 3, NX_PLAIN, int(_g1_keys()[-1]) + 40, BOTH, True, extra=((706, WIDE_KEY),),
     strict_min=0.95)

_g2_lens = [20 + (r * 53) % 101 for r in range(1, 200)]
_g2_lens[100] = 700
case("g2", np.arange(1, 200) * 2, _g2_lens, 5000, 420, (5000,), False)

_g3_lens = [c for c in ((r * 41) % 97 for r in range(1, 300)) if c > 0]
case("g3", 3 + np.arange(len(_g3_lens)) * 3, _g3_lens, NX_PLAIN - 1, 3 * len(_g3_lens) + 9, BOTH, True,
     append=((3 * len(_g3_lens), NX_PLAIN),))                      # one cell written behind the last one: it takes the last slot


G4_ROW, G4_ROW_FRONT, G4_ROW_LATE = 113, 41, 119


def _g4_lens(big, row=G4_ROW):
    lens = [5] * 120
    lens[row - 1] = big
    return lens                              # (w: one cell fewer, the 2**33 cell is the row's last)


for _big, _name, _z in ((237, "g4_512", True), (238, "g4_513", False)):
    case(_name, np.arange(1, 121), _g4_lens(_big), NX_PLAIN, 125, BOTH, _z)
    case(_name + "w", np.arange(1, 121), _g4_lens(_big - 1), NX_PLAIN, 125, BOTH, _z, extra=((G4_ROW, WIDE_KEY),))
# the same 512 slots from offset 5: the only semaphore of its span, in the first of the 8 words the next wave searches backwards
case("g4_512f", np.arange(1, 121), _g4_lens(237, G4_ROW_FRONT), NX_PLAIN, 125, BOTH, True)
# and from offset 500: ends in the last word the overrun loop reads
case("g4_512l", np.arange(1, 121), _g4_lens(237, G4_ROW_LATE), NX_PLAIN, 125, BOTH, True)

# the 2000-cell row: its semaphore in slot 2 of span 8, found by span 9 in the last word of the 8-word search, by span 13 in the last of
# the 32 words; span 14 bisects
_g5_lens = [632] + [3] * 60 + [300] + [3] * 60 + [900] + [3] * 70 + [2000] + [3] * 60 + [350]
_g5_keys = 1 + np.arange(len(_g5_lens))
G5_LONG = 1 + _g5_lens.index(2000)
case("g5", _g5_keys, _g5_lens, 8000, len(_g5_lens) + 3, (8000, NX_NT), False)
# the 2000-cell row is table entry 194; the bisection's midpoints behind it: 224, 208, 200, 196, 194, 195.  Tombstones on 222..224 (a dead
# midpoint, live entries on its left) and on 195, 196 (a dead midpoint next to the answer, then everything from lo to the midpoint dead)
case("g5d", _g5_keys, _g5_lens, 8000, len(_g5_lens) + 3, (8000, NX_NT), False, delete=(222, 223, 224, 195, 196))


def _g6(name, keys, ny, zfill, nx=2000, extra=()):
    case("g6_" + name, keys, [3] * len(keys), 2000, ny, (nx,), zfill, extra=extra)


_k = 5 + 3 * np.arange(40)
for _d, _z in ((0, True), (1, False)):
    _s = "4096" if _z else "4097"
    _g6("gap" + _s, np.concatenate([_k[:20], _k[20:] - _k[20] + _k[19] + MAX_FILL + _d]), int(_k[-1]) + MAX_FILL + 10, _z)
    _g6("first" + _s, _k - _k[0] + MAX_FILL + _d, int(_k[-1]) + MAX_FILL + 10, _z)
    _g6("tail" + _s, _k, int(_k[-1]) + MAX_FILL + _d, _z)
_kg = np.concatenate([_k[:20], _k[20:] + 100])
_g6("ny_in_gap", _kg, int(_kg[19]) + 50, True)
_g6("ny_eq_last", _k, int(_k[-1]), True)
_g6("ny1_key1", _k - 4, 1, True)
_g6("ny1_key5", _k, 1, True)
_g6("ny0", _k, 0, True)
_g6("nx_small", _k, int(_k[-1]) + 7, True, nx=1000)
_g6("col_below_1", _k, int(_k[-1]) + 7, True, extra=((int(_k[3]), -3), (int(_k[7]), -1), (int(_k[39]), -1)))

case("tiny", [3], [1], NX_PLAIN, 10, (NX_NT,), True)
case("tiny_far", [3], [1], NX_PLAIN, 3 + MAX_FILL + 1, (NX_NT,), False)
case("tinyw", [3], [1], NX_PLAIN, 10, (NX_NT,), True, extra=((3, WIDE_KEY),))
case("tinyw_far", [3], [1], NX_PLAIN, 3 + MAX_FILL + 1, (NX_NT,), False, extra=((3, WIDE_KEY),))

_g8_keys = 2 + np.arange(70000) + np.arange(70000) // 1000
case("g8", _g8_keys, [1] * 70000, NX_PLAIN, int(_g8_keys[-1]) + 5, BOTH, True, strict_min=0.95)

# WIDE NT ZFILL SHARE of every product of a case (one entry per nx)
FORMS = {
    "g1": {"0010", "0111"}, "g1w": {"1010", "1111"}, "g2": {"0000"}, "g3": {"0010", "0111"},
    "g4_512": {"0010", "0111"}, "g4_512f": {"0010", "0111"}, "g4_512l": {"0010", "0111"}, "g4_513": {"0000", "0101"},
    "g4_512w": {"1010", "1111"}, "g4_513w": {"1000", "1101"},
    "g5": {"0000", "0101"}, "g5d": {"0000", "0101"},
    "tiny": {"0110"}, "tiny_far": {"0100"}, "tinyw": {"1110"}, "tinyw_far": {"1100"}, "g8": {"0010", "0111"},
}
for _c in CASES.values():
    if _c.name.startswith("g6_"):
        FORMS[_c.name] = {"0010" if _c.zfill else "0000"}
UNREACHABLE = {"0001", "0011", "1001", "1011"}          # SHARE without NT

PARAMS = [pytest.param(name, swap, id="%s-%s" % (name, "At" if swap else "A")) for name in CASES for swap in (False, True)]


def triples(c):
    """(row key, column key, value) of the case: row r holds lens[r] cells at ascending columns start + i * step within 1..width"""
    R = len(c.keys)
    h = splitmix_array(len(c.name) * 1000 + R, 2 * R)
    step = 1 + (h[:R] % np.maximum(1, (c.width - 1) // c.lens).astype(np.uint64)).astype(np.int64)
    start = 1 + (h[R:] % (c.width - (c.lens - 1) * step).astype(np.uint64)).astype(np.int64)
    first = np.cumsum(c.lens) - c.lens
    idx = np.arange(int(c.lens.sum())) - np.repeat(first, c.lens)
    I = np.repeat(c.keys, c.lens)
    J = np.repeat(start, c.lens) + idx * np.repeat(step, c.lens)
    assert J.min() >= 1 and J.max() <= c.width
    more = c.extra + c.append
    if more:
        I = np.concatenate([I, [i for i, _ in more]]).astype(np.int64)
        J = np.concatenate([J, [j for _, j in more]]).astype(np.int64)
        assert len(set(zip(I.tolist(), J.tolist()))) == len(I)
    return I, J, signed(unit12_array(len(c.name) + 31, len(I)), R + 5)


def orientation(swap):
    """the orientation the gather walks: partitions = rows of the result"""
    return COLMAJOR if swap else ROWMAJOR


def build(dsa, binding, c, swap):
    I, J, V = triples(c)
    m, n = max(int(I.max()), c.ny, 1), max(int(J.max()), max(c.nxs))
    if swap:
        I, J, m, n = J, I, n, m
    k = len(I) - len(c.append)
    a = dsa.dynamicsparse(I[:k], J[:k], V[:k], m, n, binding=binding)
    if c.append:
        a.set_batch(I[k:], J[k:], V[k:])
    for k in c.delete:
        a.deletecolumn(int(k)) if swap else a.deleterow(int(k))
    return a


# ---- geometry of an exported layout ------------------------------------------------------------------------------------------------
class Geometry:
    def __init__(self, L):
        sems, self.cap = L["semaphores"], L["info"]["capacity"]
        live = np.flatnonzero(sems > 0)
        self.table_len = len(sems)
        self.sems = sems
        self.key = L["col_keys"][live]
        self.pos = sems[live] - 1                                   # 0-based slot of the semaphore
        assert np.all(np.diff(self.pos) > 0)                        # ids ascend along the array
        nxt = np.append(self.pos[1:], self.cap)
        self.ext = nxt - self.pos
        self.off, self.span = self.pos % SPAN, self.pos // SPAN
        self.per = np.bincount(self.span, minlength=(self.cap + SPAN - 1) // SPAN)
        span_end = (self.span + 1) * SPAN
        has_next = np.append(np.ones(len(live) - 1, bool), False) if len(live) else np.zeros(0, bool)
        nine = (has_next & (nxt < span_end + 64)) | (span_end >= self.cap)
        self.strict = (self.per[self.span] > COOP) & nine
        self.ordered = len(live) == len(sems) and len(live) > 0 and bool(np.all(np.diff(self.key) > 0))
        self.occ = L["occ"]

    def host_zfill(self, ny):
        """spmv_dev's rule over the words k_spmv_meta computes"""
        if not self.ordered:
            return False
        gap = int(np.diff(self.key).max()) if len(self.key) > 1 else 0
        return bool(self.ext.max() <= SPAN and gap <= MAX_FILL and 1 <= self.key[0] <= MAX_FILL and ny - self.key[-1] <= MAX_FILL)

    def bisect_spans(self):
        """first slots of the spans whose wave finds no semaphore in the 8 + 32 words in front of it (and has that many)"""
        out = []
        for s in range(0, self.cap, SPAN):
            lo = s - SPAN - 32 * 64
            if lo > 0 and not np.any((self.pos >= lo) & (self.pos < s)) and np.any(self.pos < lo):
                out.append(s)
        return out


def bisection_trace(sems, b0):
    """carry_in_partition's table bisection for the slots in front of b0: (partition id, a dead midpoint with a live entry on its
    left was met, a wholly dead [lo, mid] was met)"""
    lo, hi, best, dead_mid, dead_run = 0, len(sems) - 1, -1, False, False
    while lo <= hi:
        mid = i = (lo + hi) >> 1
        while i >= lo and sems[i] == 0:
            i -= 1
        if i < lo:
            dead_run = True
            lo = mid + 1
            continue
        dead_mid |= i != mid
        if sems[i] <= b0:
            best, lo = i, mid + 1
        else:
            hi = i - 1
    return best + 1, dead_mid, dead_run


# ---- the reference ----------------------------------------------------------------------------------------------------------------
class Reference:
    """what one product of a case is compared with: built once, never modified"""

    def __init__(self, c, G, nx, oracle_y):
        I, J, V = triples(c)
        keep = ~np.isin(I, np.asarray(c.delete, np.int64))
        I, J, V = I[keep], J[keep], V[keep]
        o = np.lexsort((J, I))
        I, J, V = I[o], J[o], V[o]
        x = x_of(nx)
        ok = (J >= 1) & (J <= nx) & (I >= 1) & (I <= c.ny)
        I, p = I[ok], V[ok] * x[J[ok] - 1]
        ny = self.ny = c.ny
        self.ref, self.bound = np.zeros(ny), np.zeros(ny)
        rows, start, cnt = np.unique(I, return_index=True, return_counts=True)
        for r, a, n in zip(rows.tolist(), start.tolist(), cnt.tolist()):
            q = p[a:a + n]
            self.ref[r - 1] = math.fsum(q)
            self.bound[r - 1] = (n + 1) * U * math.fsum(np.abs(q))
        inside = (G.key >= 1) & (G.key <= ny)
        self.single, self.strict = np.ones(ny, bool), np.zeros(ny, bool)
        self.single[G.key[inside & (G.ext > SPAN)] - 1] = False
        self.strict[G.key[inside & G.strict] - 1] = True
        self.oracle = oracle_y
        self.rows_with_partition = int(inside.sum())


def first_bad(mask):
    w = np.flatnonzero(mask)
    return "%d rows, first %s" % (len(w), (w[:5] + 1).tolist())


def verdict(R, y1, y2, atomic=False):
    """the whole comparison of two successive products into the same NaN-filled y of ny + GUARD words with the reference"""
    ny = R.ny
    nan = bits(np.full(GUARD, np.nan))
    for k, y in enumerate((y1, y2)):
        assert len(y) == ny + GUARD
        assert np.array_equal(bits(y[ny:]), nan), "product %d wrote behind y[:ny]" % k
        y = y[:ny]
        assert not np.isnan(y).any(), "product %d left NaN in y: %s" % (k, first_bad(np.isnan(y)))
        over = np.abs(y - R.ref) > R.bound
        assert not over.any(), "product %d outside the bound: %s" % (k, first_bad(over))
        nonzero = (R.bound == 0) & (bits(y) != 0)
        assert not nonzero.any(), "product %d: a row without products is not +0.0: %s" % (k, first_bad(nonzero))
    if not atomic:
        differ = R.single & (bits(y1[:ny]) != bits(y2[:ny]))
        assert not differ.any(), "the second product differs where one wave writes the row: %s" % first_bad(differ)
        differ = R.strict & (bits(y1[:ny]) != bits(R.oracle))
        assert not differ.any(), "one-lane rows differ from the left fold: %s" % first_bad(differ)


_refs = {}


def references(dsa, oracle, name, swap):
    """(geometry, {nx: Reference}, forms) of a case from the oracle; kept for the module"""
    if (name, swap) not in _refs:
        c = CASES[name]
        b = build(dsa, oracle, c, swap)
        G = Geometry(b.export_layout(orientation(swap)))
        refs = {nx: Reference(c, G, nx, b.mul(x_of(nx).copy(), transpose=swap, dense_out=c.ny)) for nx in c.nxs}
        _refs[(name, swap)] = (G, refs, {form_of(c, nx, G.cap) for nx in c.nxs})
    return _refs[(name, swap)]


def form_of(c, nx, capacity):
    nt = 8 * nx > (3 << 20)
    share = nt and capacity >= TILE and capacity % TILE == 0
    return "%d%d%d%d" % (c.wide, nt, c.zfill, share)


# ---- the situations each case is there for, asserted on the oracle's layout -------------------------------------------------------
def _sit_g1(G, c):
    assert G.per.max() > 64 and G.ext.max() <= 8


def _sit_g2(G, c):
    assert {0, 4, 5} <= set(G.per.tolist())


def _sit_g3(G, c):
    assert G.ext.max() <= SPAN
    assert np.any(G.off == SPAN - 1) and G.pos[0] == 1 and np.any(G.off[1:] == 1)     # (slot 0 of the array is a gap here; g5: a semaphore)
    first = np.flatnonzero(G.off[1:] == 0) + 1                      # a semaphore in the first slot of a span, a row in front of it
    assert len(first) and np.all(G.pos[first - 1] + G.ext[first - 1] == G.pos[first])
    assert np.any((G.pos % TILE == TILE - 1) & (G.pos + 1 < G.cap))  # last slot of a tile, another tile behind it
    assert G.occ[G.cap - 1] and G.pos[-1] + G.ext[-1] == G.cap       # the last row's last cell in the last slot of the array
    assert {4, 5} <= set(G.per.tolist())


def _sit_g4(G, c):
    want = SPAN if c.zfill else SPAN + 1
    i = int(np.argmax(G.ext))
    assert G.ext[i] == want and int((G.ext >= SPAN).sum()) == 1 and G.cap == TILE
    if c.name == "g4_512f":
        # ends in the ninth word; the wave behind finds its semaphore in the last word of its backward search and nowhere else
        assert G.key[i] == G4_ROW_FRONT and G.off[i] < 64 and SPAN < G.off[i] + G.ext[i] < NINE_WORDS and G.per[G.span[i]] == 1
    elif c.name == "g4_512l":
        assert G.key[i] == G4_ROW_LATE and 2 * SPAN - 64 < G.off[i] + G.ext[i] <= 2 * SPAN      # the 16th word from the span's first
    else:
        assert G.key[i] == G4_ROW and G.off[i] + G.ext[i] > NINE_WORDS and G.off[i] + G.ext[i] <= 2 * SPAN


def _sit_g5(G, c):
    e = G.ext
    assert np.any((e > SPAN) & (e <= 2 * SPAN)) and np.any((e > 2 * SPAN) & (e <= 5 * SPAN)) and np.any(e > 6 * SPAN)
    assert e[0] > SPAN and e[-1] > SPAN and G.pos[0] == 0
    assert np.any((e > SPAN) & (G.pos // TILE != (G.pos + e - 1) // TILE))
    spans = G.bisect_spans()
    assert spans
    i = int(np.flatnonzero(G.key == G5_LONG)[0])
    # the long row's semaphore in the first word of its span: the edge of the 8-word and of the 32-word search; the first span that bisects
    assert G.off[i] < 64 and G.per[G.span[i]] == 1 and spans[0] == (G.span[i] + 6) * SPAN and G.pos[i] + e[i] > spans[0] + 64
    traces = [bisection_trace(G.sems, s - SPAN) for s in spans]
    for s, (pid, _, _) in zip(spans, traces):
        assert G.sems[pid - 1] - 1 == G.pos[G.pos < s].max()          # the bisection's answer is the row that covers the span
    if c.delete:
        assert G.table_len > len(G.pos) and not G.ordered
        assert any(t[1] for t in traces) and any(t[2] for t in traces)
    else:
        assert G.table_len == len(G.pos)


def _sit_g6(G, c):
    gap, first, tail = int(np.diff(G.key).max()), int(G.key[0]), c.ny - int(G.key[-1])
    n = c.name[3:]
    if n.startswith(("gap", "first", "tail")):
        want = MAX_FILL + (not c.zfill)
        assert {"gap": gap, "first": first, "tail": tail}[n[:-4]] == want
        assert sorted([gap > MAX_FILL, first > MAX_FILL, tail > MAX_FILL]) == [False, False, not c.zfill]
    if n == "ny_in_gap":
        below = G.key[G.key <= c.ny]
        assert len(below) == 20 and G.key[20] - c.ny > 40 and c.ny - below[-1] > 40
    if n == "ny_eq_last":
        assert tail == 0
    if n.startswith("ny1"):
        assert c.ny == 1 and first == (1 if n == "ny1_key1" else 5)
    if n == "ny0":
        assert c.ny == 0
    if n == "nx_small":
        _, J, _ = triples(c)
        assert (J > c.nxs[0]).sum() > 10 and (J <= c.nxs[0]).sum() > 10
    if n == "col_below_1":
        _, J, _ = triples(c)
        assert sorted(J[J < 1].tolist()) == [-3, -1, -1]


def _sit_tiny(G, c):
    assert len(G.pos) == 1 and G.cap < TILE
    assert (c.ny - int(G.key[0]) > MAX_FILL) == (not c.zfill)


def _sit_g8(G, c):
    ntiles = G.cap // TILE
    assert G.cap >= 131072 and G.cap % TILE == 0 and ntiles >= 64
    per = (ntiles + 7) // 8
    inside = (G.key >= 1) & (G.key <= c.ny)
    for g in range(1, 8):                                              # both sides of every seam between two XCDs' tile ranges
        assert np.any(inside & (G.pos >= g * per * TILE - SPAN) & (G.pos < g * per * TILE)), g
        assert np.any(inside & (G.pos >= g * per * TILE) & (G.pos < g * per * TILE + SPAN)), g


SITUATIONS = {"g1": _sit_g1, "g2": _sit_g2, "g3": _sit_g3, "g4": _sit_g4, "g5": _sit_g5, "g6": _sit_g6, "tiny": _sit_tiny, "g8": _sit_g8}


def situations(name):
    return SITUATIONS[[k for k in SITUATIONS if name.startswith(k)][-1]]


@pytest.mark.parametrize("name,swap", PARAMS)
def test_oracle_alone(dsa, oracle, name, swap):
    c = CASES[name]
    G, refs, forms = references(dsa, oracle, name, swap)
    situations(name)(G, c)
    assert G.host_zfill(c.ny) == c.zfill
    assert forms == FORMS[name]
    if c.wide:
        I, J, _ = triples(c)
        assert int((np.abs(J) > 2 ** 31).sum()) == 1 and np.all(np.abs(I) < 2 ** 31)      # inner keys wide, partition keys small
    for nx, R in refs.items():
        y = np.concatenate([R.oracle, np.full(GUARD, np.nan)])
        verdict(R, y, y)                                             # the oracle's left fold against the fsum reference
        assert R.single[R.strict].all()
        if c.strict_min is not None:
            assert R.strict.sum() >= c.strict_min * R.rows_with_partition, (int(R.strict.sum()), R.rows_with_partition)


def test_every_reachable_form_has_a_case():
    reached = set().union(*FORMS.values())
    every = {"%d%d%d%d" % (w, n, z, s) for w in (0, 1) for n in (0, 1) for z in (0, 1) for s in (0, 1)}
    assert reached == every - UNREACHABLE
    assert set(FORMS) == set(CASES)


# ---- the products on the GPU -------------------------------------------------------------------------------------------------------
def products(hip, a, transpose, algo, nx, ny):
    """two products into the same NaN-filled y of ny + GUARD words"""
    import torch
    dev = torch.device("cuda:0")
    hip.call("mat_set_stream", a.h, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    xd = torch.from_numpy(x_of(nx).copy()).to(dev)
    yd = torch.from_numpy(np.full(ny + GUARD, np.nan)).to(dev)
    ys = []
    for _ in range(2):
        hip.call("mat_spmv_dense_dev", a.h, int(transpose), algo, C.c_void_p(xd.data_ptr()), nx, C.c_void_p(yd.data_ptr()), ny)
        torch.cuda.synchronize()
        ys.append(yd.cpu().numpy())
    return ys


def stats(a):
    return {o: a.info(o) for o in (COLMAJOR, ROWMAJOR)}


@pytest.mark.gpu
@pytest.mark.parametrize("name,swap", PARAMS)
def test_gather(dsa, hip, oracle, name, swap):
    c = CASES[name]
    G, refs, forms = references(dsa, oracle, name, swap)
    o = orientation(swap)
    seen, first = set(), {}
    for nx in c.nxs:
        a = build(dsa, hip, c, swap)                                  # a fresh handle: two products per (nx, ny), no plan
        La = a.export_layout(o)
        assert La["info"]["capacity"] == G.cap and np.array_equal(La["semaphores"], G.sems) and np.array_equal(La["occ"], G.occ)
        if c.wide:
            n = build(dsa, hip, narrow_twin(c), swap)
            Ln = n.export_layout(o)
            assert Ln["info"]["capacity"] == G.cap and np.array_equal(Ln["occ"], G.occ)
            assert La["info"]["hbm_bytes"] - Ln["info"]["hbm_bytes"] >= 2 * 4 * G.cap     # both slot buffers, 8- instead of 4-byte keys
            del n
        s0 = stats(a)
        ys = products(hip, a, swap, 0, nx, c.ny)
        s1 = stats(a)
        assert s1[o]["stat_spmv_nomemset"] - s0[o]["stat_spmv_nomemset"] == (2 if c.zfill else 0)
        assert all(s1[q]["stat_spmv_plan"] == s0[q]["stat_spmv_plan"] for q in s0)
        verdict(refs[nx], ys[0], ys[1])
        seen.add(form_of(c, nx, La["info"]["capacity"]))
        first[nx] = ys[0][:c.ny]
        del a
    assert seen == forms == FORMS[name]
    if len(first) == 2:
        # the plain and the non-temporal form of the same matrix (no column beyond the smaller nx): the same sums in the same order
        R = refs[c.nxs[0]]
        differ = R.single & (bits(first[c.nxs[0]]) != bits(first[c.nxs[1]]))
        assert not differ.any(), first_bad(differ)


@pytest.mark.gpu
@pytest.mark.parametrize("name,swap", PARAMS)
def test_scatter(dsa, hip, oracle, name, swap):
    """k_spmv_scatter (algo = 1) walks the other orientation and adds every product atomically behind a memset"""
    c = CASES[name]
    _, refs, _ = references(dsa, oracle, name, swap)
    nx = c.nxs[0]
    a = build(dsa, hip, c, swap)
    s0 = stats(a)
    ys = products(hip, a, swap, 1, nx, c.ny)
    s1 = stats(a)
    assert all(s1[q][k] == s0[q][k] for q in s0 for k in ("stat_spmv_nomemset", "stat_spmv_plan"))
    verdict(refs[nx], ys[0], ys[1], atomic=True)
