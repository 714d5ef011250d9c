"""The whole-vector operations at their edges: v1 == v2 (dsa_vec_equal -> k_packed_equal), alpha*v1 + beta*v2 (dsa_vec_axpby ->
k_merge_axpby with packed_bound) and the pack behind both and behind nonzeros() (vec_pack_alt: pack_small up to VIEW_SMALL_SLOTS =
65536 slots, k_tile_count / k_tile_scan / k_compact of 4096-slot tiles, 16 tiles per count workgroup, above).

The expected results come from two numpy models that use nothing of the library:

* `model_axpby`: union of the keys; fl(alpha*x) / fl(beta*y) for a key stored in one operand (kept whatever the value);
  fl(fl(alpha*x) + fl(beta*y)) for a key stored in both, dropped exactly when that is == 0.0.  numpy rounds every step on its own.
* `model_equal`: lengths, counts, keys, and values under IEEE == (NaN differs from NaN, -0.0 equals +0.0).

Every comparison is bitwise (keys array_equal, values as uint64; a NaN matches a NaN of any payload), no tolerance anywhere.

Every group of cases runs twice: `test_model_matches_oracle` (no GPU) runs it on the CPU oracle, which qualifies the model on
exactly the inputs `test_hip_matches_model` then gives the HIP library.  Each case asserts the regime it claims (capacities of the
operands and the merged total against 65536) on the structure at hand before it compares.  Every operand built here also goes
through `check_operand`: nonzeros() equals the stored cells of export_layout() in slot order and the content the test put in.

Contraction.  The library and the oracle are built with -ffp-contract=off and k_merge_axpby spells out __dadd_rn(__dmul_rn, __dmul_rn).
A kernel that computes alpha*x + beta*y with one or two fused multiply-adds is wrong by an ulp on some keys only, so the inputs must
make that visible: values are standard normal, the default coefficients are 1/3 and 0.7, and on the CPU half every axpby case with
at least 256 both-stored keys computes the three contracted forms exactly with fractions.Fraction and asserts that each differs from
the model on at least 10 % of those keys (up to 2000 sampled).  Cases whose coefficients are 0 or powers of two (the cancellations
with (1, -1), the special-value runs with (1, 1), (0, 1), (2, 2)) have exact products: a contraction cannot show there by construction
and the condition is not applied."""
import ctypes as C
import math
from fractions import Fraction as F

import numpy as np
import pytest

SMALL = 65536                      # VIEW_SMALL_SLOTS: one-launch pack up to here, tile kernels above
TILE = 4096                        # slots per k_compact tile
A3, B7 = 1.0 / 3.0, 0.7            # default coefficients: both products round
W31, W40 = 1 << 31, 1 << 40


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def same_values(got, want):
    """bitwise, but a NaN matches a NaN of any payload"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


# ================================================================== the models
def model_axpby(xk, xv, alpha, yk, yv, beta):
    xk, yk = np.asarray(xk, dtype=np.int64), np.asarray(yk, dtype=np.int64)
    xv, yv = np.asarray(xv, dtype=np.float64), np.asarray(yv, dtype=np.float64)
    assert np.all(xk[1:] > xk[:-1]) and np.all(yk[1:] > yk[:-1])
    keys = np.union1d(xk, yk).astype(np.int64)
    ix, iy = np.searchsorted(keys, xk), np.searchsorted(keys, yk)
    inx, iny = np.zeros(len(keys), dtype=bool), np.zeros(len(keys), dtype=bool)
    inx[ix] = True
    iny[iy] = True
    ax, by = np.zeros(len(keys)), np.zeros(len(keys))
    with np.errstate(all="ignore"):
        ax[ix] = np.float64(alpha) * xv              # one rounding
        by[iy] = np.float64(beta) * yv               # one rounding
        both = inx & iny
        out = np.where(inx, ax, by)
        out[both] = (ax + by)[both]                  # one more
    keep = ~(both & (out == 0.0))
    return keys[keep], out[keep]


def model_equal(n_a, a, n_b, b):
    (ak, av), (bk, bv) = a, b
    if n_a != n_b or len(ak) != len(bk):
        return False
    return bool(np.array_equal(ak, bk) and np.all(np.asarray(av) == np.asarray(bv)))


def apply_sets(k, v, sk, sv):
    """content after setindex! of (sk, sv) in order: a zero value deletes"""
    d = dict(zip(k.tolist(), v.tolist()))
    for a, b in zip(np.asarray(sk).tolist(), np.asarray(sv, dtype=np.float64).tolist()):
        if b == 0.0:
            d.pop(a, None)
        else:
            d[a] = b
    keys = sorted(d)
    return np.array(keys, dtype=np.int64), np.array([d[q] for q in keys], dtype=np.float64)


def exact_products(alpha, beta):
    return all(c == 0.0 or math.frexp(abs(c))[0] == 0.5 for c in (alpha, beta))


def contraction_shares(xv, yv, alpha, beta):
    """share of the pairs on which each contracted form differs from fl(fl(alpha*x) + fl(beta*y)): fully fused, x fused, y fused"""
    diff = [0, 0, 0]
    fa, fb = F(alpha), F(beta)
    for x, y in zip(xv.tolist(), yv.tolist()):
        ax, by = alpha * x, beta * y
        m = ax + by
        forms = (float(fa * F(x) + fb * F(y)), float(fa * F(x) + F(by)), float(F(ax) + fb * F(y)))
        for q, f in enumerate(forms):
            diff[q] += f != m
    return [d / len(xv) for d in diff]


# ================================================================== vectors with the content the test put into them
class Tracked:
    def __init__(self, vec, k, v, n):
        self.vec, self.k, self.v, self.n = vec, np.asarray(k, dtype=np.int64), np.asarray(v, dtype=np.float64), int(n)

    def set(self, key, val):                         # queued in the HIP library
        self.vec[key] = val
        self.k, self.v = apply_sets(self.k, self.v, [key], [val])
        if val != 0.0:
            self.n = max(self.n, int(key))

    def set_batch(self, keys, vals):
        self.vec.set_batch(keys, vals)
        self.k, self.v = apply_sets(self.k, self.v, keys, vals)
        nz = np.asarray(keys)[np.asarray(vals) != 0.0]
        if len(nz):
            self.n = max(self.n, int(nz.max()))

    def shrink_size(self):
        self.vec.shrink_size()
        self.n = int(self.k.max()) if len(self.k) else 0

    def capacity(self):
        return self.vec.info()["capacity"]


class Env:
    def __init__(self, dsa, b, cpu):
        self.dsa, self.b, self.cpu = dsa, b, cpu
        self.axpby_cases = self.equal_cases = self.operands = self.contraction_cases = 0

    def mk(self, k, v, n=None):
        k, v = np.asarray(k, dtype=np.int64), np.asarray(v, dtype=np.float64)
        vec = self.dsa.dynamicsparsevec(k, v, n=n, binding=self.b)
        t = Tracked(vec, k, v, n if n is not None else max(0, int(k.max()) if len(k) else 0))
        self.check_operand(t)
        return t

    def imp(self, K, V, O, seg, n):
        vec = self.dsa.import_vector_layout(K, V, O, seg, n=n, binding=self.b)
        m = np.asarray(O).astype(bool)
        t = Tracked(vec, K[m].copy(), V[m].copy(), n)
        self.check_operand(t)
        return t

    def check_operand(self, t):
        """nonzeros() against the stored cells of export_layout() in slot order and against the content the test tracks"""
        k, v = t.vec.nonzeros()
        K, V, O = t.vec.export_layout()
        m = O.astype(bool)
        assert len(k) == t.vec.nnz() == int(m.sum()) == len(t.k)
        assert k.dtype == np.int64 and np.all(k[1:] > k[:-1])
        assert np.array_equal(k, K[m]) and np.array_equal(bits(v), bits(V[m]))
        assert np.array_equal(k, t.k) and np.array_equal(bits(v), bits(t.v))
        assert len(t.vec) == t.n
        self.operands += 1

    def check_axpby(self, x, alpha, y, beta):
        wk, wv = model_axpby(x.k, x.v, alpha, y.k, y.v, beta)
        gk, gv = x.vec.axpby(alpha, y.vec, beta)
        assert len(gk) == len(gv) == len(wk), (len(gk), len(wk))
        assert np.array_equal(gk, wk)
        assert same_values(gv, wv), np.flatnonzero(bits(gv) != bits(wv))[:8]
        self.axpby_cases += 1
        if self.cpu and not exact_products(alpha, beta):
            sx = np.isin(x.k, y.k, assume_unique=True)
            sy = np.isin(y.k, x.k, assume_unique=True)
            if int(sx.sum()) >= 256:
                pick = np.unique(np.linspace(0, int(sx.sum()) - 1, 2000).astype(np.int64))
                shares = contraction_shares(x.v[sx][pick], y.v[sy][pick], alpha, beta)
                assert min(shares) >= 0.10, shares
                self.contraction_cases += 1
        return wk, wv

    def check_equal(self, a, b, expect):
        want = model_equal(a.n, (a.k, a.v), b.n, (b.k, b.v))
        assert want is expect
        assert (a.vec == b.vec) is want
        assert (b.vec == a.vec) is want
        self.equal_cases += 1


def small(t):
    return t.capacity() <= SMALL


def merged_small(x, y):
    return len(x.k) + len(y.k) <= SMALL


def value_of(wk, wv, key):
    i = np.searchsorted(wk, key)
    assert i < len(wk) and wk[i] == key, key
    return wv[i]


# ================================================================== axpby 1: the x / y thread split of a workgroup
SPLIT_COUNTS = [(0, 1), (1, 0), (0, 300), (300, 0), (63, 1), (64, 64), (65, 191), (255, 1), (256, 256), (257, 255), (192, 64)]


def g_split(env):
    rng = np.random.default_rng(3101)
    for na, nb in SPLIT_COUNTS:
        for shape in ("interleaved", "x_below", "y_below", "overlap"):
            s = 0
            if shape == "interleaved":
                xk, yk = 2 * np.arange(na) + 1, 2 * np.arange(nb) + 2
            elif shape == "x_below":
                xk, yk = np.arange(1, na + 1), na + np.arange(1, nb + 1)
            elif shape == "y_below":
                yk, xk = np.arange(1, nb + 1), nb + np.arange(1, na + 1)
            else:                                     # the last keys of x are the first keys of y: both-stored cells at the split
                s = (min(na, nb) + 1) // 2
                xk, yk = np.arange(1, na + 1), na - s + np.arange(1, nb + 1)
            x, y = env.mk(xk, rng.standard_normal(na)), env.mk(yk, rng.standard_normal(nb))
            assert small(x) and small(y) and merged_small(x, y)
            wk, _ = env.check_axpby(x, A3, y, B7)
            assert len(wk) == na + nb - s


# ================================================================== axpby 2: words of the keep bitmap
def g_keep_words(env):
    rng = np.random.default_rng(3102)
    for n in (32, 33, 64, 4096):
        k = 3 * np.arange(1, n + 1)
        xv, yv = rng.standard_normal(n), rng.standard_normal(n)
        x, y = env.mk(k, xv), env.mk(k, yv)
        assert small(x) and small(y) and merged_small(x, y)
        wk, _ = env.check_axpby(x, A3, y, B7)        # merged cells are x / y pairs: the keep bits alternate 1, 0
        assert len(wk) == n                          # nothing cancels, every x cell is kept
        wk, wv = env.check_axpby(x, 1.0, env.mk(k, xv.copy()), -1.0)
        assert len(wk) == 0 and len(wv) == 0 and 2 * n > 0        # everything cancels
        i = np.arange(n)
        for name, drop in (("first", i == 0), ("last", i == n - 1), ("word_edge", np.isin(i % 64, (31, 32)))):
            # key i sits at merged positions 2i (x) and 2i + 1 (y): i = 31, 32 mod 64 are positions 62..65 mod 128
            assert drop.any(), (n, name)
            v3 = yv.copy()
            v3[drop] = xv[drop]
            wk, _ = env.check_axpby(x, 1.0, env.mk(k, v3), -1.0)
            assert np.array_equal(wk, k[~drop])


# ================================================================== axpby 3: one operand on each side of the pack switch
def g_operand_switch(env):
    rng = np.random.default_rng(3103)
    for na, cap in ((45875, 65536), (45876, 131072)):
        xk = 2 * np.arange(1, na + 1)
        shared = xk[np.linspace(0, na - 1, 50).astype(np.int64)]      # first and last key of x among them
        yk = np.sort(np.concatenate([shared, 2 * rng.choice(na, 50, replace=False) + 1]))
        x, y = env.mk(xk, rng.standard_normal(na)), env.mk(yk, rng.standard_normal(100))
        assert x.capacity() == cap and small(y) and merged_small(x, y)
        env.check_axpby(x, A3, y, B7)
        env.check_axpby(y, A3, x, B7)


# ================================================================== axpby 4: the merged array on each side of the pack switch
def g_merged_switch(env):
    rng = np.random.default_rng(3104)
    for nb in (32768, 32769):
        na = 32768
        xk = 2 * np.arange(na) + 1
        x = env.mk(xk, rng.standard_normal(na))
        for nshared in (0, 1000):
            sh = xk[np.linspace(0, na - 1, nshared).astype(np.int64)] if nshared else xk[:0]
            yk = np.sort(np.concatenate([sh, 2 * np.arange(1, nb - nshared + 1)]))
            y = env.mk(yk, rng.standard_normal(nb))
            assert small(x) and small(y) and len(x.k) + len(y.k) == na + nb
            assert merged_small(x, y) == (nb == 32768)
            wk, _ = env.check_axpby(x, A3, y, B7)
            assert len(wk) == na + nb - nshared      # shared keys lower the count, not the total
            env.check_axpby(y, B7, x, A3)


# ================================================================== axpby 5: tiles of k_compact, workgroups of k_tile_count
def merged_keep(x, alpha, y, beta):
    """the keep bit of every cell of the merged array (x's cell in front of y's at equal keys), restated from the model's rule"""
    order = np.argsort(np.concatenate([x.k, y.k]), kind="stable")
    inx, iny = np.isin(x.k, y.k, assume_unique=True), np.isin(y.k, x.k, assume_unique=True)
    s = np.float64(alpha) * x.v[inx] + np.float64(beta) * y.v[iny]
    kx = np.ones(len(x.k), dtype=bool)
    kx[inx] = s != 0.0
    return np.concatenate([kx, ~iny])[order]


def g_tiles(env):
    rng = np.random.default_rng(3105)
    for na, nb in ((34816, 34816), (34816, 34817), (65537, 4096), (34816, 34815)):
        total = na + nb
        xk = 2 * np.arange(na) + 1
        xv = rng.standard_normal(na)
        sh = np.linspace(0, na - 1, 600).astype(np.int64)
        yk = np.sort(np.concatenate([xk[sh], 2 * np.arange(1, nb - 600 + 1)]))
        yv = rng.standard_normal(nb)
        at = np.searchsorted(yk, xk[sh[::2]])
        yv[at] = xv[sh[::2]]                          # 300 of the 600 shared keys cancel under (1, -1)
        x, y = env.mk(xk, xv), env.mk(yk, yv)
        assert small(x) == (na <= 45875) and small(y) and not merged_small(x, y) and len(x.k) + len(y.k) == total
        wk, _ = env.check_axpby(x, A3, y, B7)
        assert len(wk) == total - 600
        wk, _ = env.check_axpby(x, 1.0, y, -1.0)
        assert len(wk) == total - 600 - 300
    assert 34816 + 34816 == 17 * TILE and 34816 + 34815 == 17 * TILE - 1 and 65537 + 4096 == 69633
    # a whole tile of the keep bitmap is zero between tiles that are not: 4200 consecutive shared keys with equal values
    na, nb = 40000, 30000
    xk = 2 * np.arange(1, na + 1)
    xv = rng.standard_normal(na)
    run = np.arange(10000, 14200)
    yk = np.sort(np.concatenate([xk[run], 2 * np.arange(0, 5000) + 1, 2 * np.arange(20000, 20000 + nb - 4200 - 5000) + 1]))
    yv = rng.standard_normal(nb)
    yv[np.searchsorted(yk, xk[run])] = xv[run]
    x, y = env.mk(xk, xv), env.mk(yk, yv)
    assert small(x) and small(y) and not merged_small(x, y)
    keep = merged_keep(x, 1.0, y, -1.0)
    tiles = np.add.reduceat(keep.astype(np.int64), np.arange(0, na + nb, TILE))
    empty = np.flatnonzero(tiles == 0)
    assert len(empty) >= 1 and empty[0] > 0 and tiles[empty[0] - 1] > 0 and tiles[empty[-1] + 1] > 0
    wk, _ = env.check_axpby(x, 1.0, y, -1.0)
    assert len(wk) == int(keep.sum()) == na + nb - 2 * 4200
    env.check_axpby(x, A3, y, B7)
    env.check_axpby(y, 1.0, x, -1.0)


# ================================================================== axpby 6: key widths
def g_key_widths(env):
    rng = np.random.default_rng(3106)
    nk = 7 * np.arange(1, 301)
    narrow = env.mk(nk, rng.standard_normal(300))
    wide_k = np.concatenate([nk[::2], W31 + 3 * np.arange(50), W40 + np.arange(1, 51)])
    wide = env.mk(wide_k, rng.standard_normal(len(wide_k)))
    for a, b in ((narrow, wide), (wide, narrow)):
        wk, _ = env.check_axpby(a, A3, b, B7)
        assert wk[-1] == W40 + 50 and len(wk) == 300 + 100
    neg_k = np.concatenate([[-(1 << 33), -W31 - 1, -W31, -9, -2], nk[1::3], [W31 - 1]])
    neg = env.mk(neg_k, rng.standard_normal(len(neg_k)))
    assert neg.n == W31 - 1
    for a, b in ((neg, narrow), (narrow, neg), (neg, wide), (wide, neg)):
        wk, _ = env.check_axpby(a, A3, b, B7)
        assert wk[0] == -(1 << 33)
    small_neg = env.mk(np.concatenate([[-9, -2], nk[::5]]), rng.standard_normal(62))      # negative keys that fit 32 bits
    env.check_axpby(small_neg, A3, narrow, B7)
    env.check_axpby(narrow, A3, small_neg, B7)
    # narrow content behind 64-bit physical keys: a key beyond 2^40 came and went
    kept64 = env.mk(nk, narrow.v.copy())
    kept64.set(W40, 1.0)
    kept64.set(W40, 0.0)
    env.check_operand(kept64)
    other = env.mk(nk[::2] + np.arange(150) % 2 * 3, rng.standard_normal(150))      # every second one shared with nk
    for a, b in ((kept64, other), (other, kept64), (kept64, narrow)):
        env.check_axpby(a, A3, b, B7)
    wk, _ = env.check_axpby(kept64, 1.0, narrow, -1.0)
    assert len(wk) == 0


# ================================================================== axpby 7: the operand with itself
def g_self(env):
    rng = np.random.default_rng(3107)
    for n in (1, 300, 45876):
        x = env.mk(5 * np.arange(1, n + 1), rng.standard_normal(n))
        assert small(x) == (n < 45876) and (2 * n <= SMALL) == (n < 45876)
        wk, wv = env.check_axpby(x, A3, x, B7)
        assert len(wk) == n and np.array_equal(bits(wv), bits(A3 * x.v + B7 * x.v))
        wk, _ = env.check_axpby(x, 1.0, x, -1.0)
        assert len(wk) == 0


# ================================================================== axpby 8: special values
SPECIALS = [np.inf, -np.inf, np.nan, -0.0, 5e-324, 1.7e308, 0.0]


def g_specials(env):
    rng = np.random.default_rng(3108)
    S = len(SPECIALS)
    # keys 1..: S x-only specials, S y-only specials, S*S shared combinations, then ordinary cells of each kind
    x_only, y_only = np.arange(1, S + 1), np.arange(101, 101 + S)
    shared = np.arange(201, 201 + S * S)
    xk = np.concatenate([x_only, shared, [400, 402, 404, 500]])
    yk = np.concatenate([y_only, shared, [401, 402, 404, 501]])
    ops = []
    for k, special in ((xk, np.concatenate([SPECIALS, np.repeat(SPECIALS, S)])), (yk, np.concatenate([SPECIALS, np.tile(SPECIALS, S)]))):
        base = env.mk(k, rng.standard_normal(len(k)))
        K, V, O = base.vec.export_layout()
        pos = np.flatnonzero(O)
        assert np.array_equal(K[pos], k)
        V[pos[:len(special)]] = special
        ops.append(env.imp(K, V, O, base.vec.info()["segment_capacity"], base.n))
    x, y = ops
    combo = {(i, j): 201 + i * S + j for i in range(S) for j in range(S)}      # x holds SPECIALS[i], y holds SPECIALS[j]
    INF, NINF, NAN, NZ, DEN, BIG, PZ = range(S)
    for alpha, beta in ((1.0, 1.0), (0.0, 1.0), (A3, B7), (2.0, 2.0)):
        wk, wv = env.check_axpby(x, alpha, y, beta)
        env.check_axpby(y, alpha, x, beta)
        if (alpha, beta) == (0.0, 1.0):
            # one-sided x cells are fl(0 * x): NaN for +-inf and NaN, else a zero that is KEPT with its sign
            assert all(np.isnan(value_of(wk, wv, 1 + q)) for q in (INF, NINF, NAN))
            for q, neg in ((NZ, True), (DEN, False), (BIG, False), (PZ, False)):
                z = value_of(wk, wv, 1 + q)
                assert z == 0.0 and bool(np.signbit(z)) == neg
            assert np.signbit(value_of(wk, wv, 500)) == (x.v[-1] < 0)
            # both-stored: 0 * x + 1 * 0.0 is +0.0 and dropped whatever finite x was; with -0.0 on the y side it takes x's sign, dropped too
            for q in (NZ, DEN, BIG, PZ):
                assert combo[(q, PZ)] not in wk and combo[(q, NZ)] not in wk
            assert np.isnan(value_of(wk, wv, combo[(INF, PZ)]))
        if (alpha, beta) == (1.0, 1.0):
            assert combo[(NZ, NZ)] not in wk and combo[(NZ, PZ)] not in wk and combo[(PZ, PZ)] not in wk      # -0.0 + -0.0 = -0.0: dropped
            assert np.isnan(value_of(wk, wv, combo[(INF, NINF)])) and value_of(wk, wv, combo[(BIG, BIG)]) == np.inf
            assert bits(value_of(wk, wv, 1 + NZ))[0] == bits(-0.0)[0]                    # one-sided -0.0 is kept as it is
        if (alpha, beta) == (2.0, 2.0):
            assert value_of(wk, wv, 1 + BIG) == np.inf and value_of(wk, wv, 101 + BIG) == np.inf
            assert value_of(wk, wv, combo[(DEN, DEN)]) == 2e-323


# ================================================================== axpby 9: a buffer that is too small
def raw_axpby(env, x, alpha, y, beta, cap):
    k, v = np.empty(max(cap, 1), dtype=np.int64), np.empty(max(cap, 1), dtype=np.float64)
    out = C.c_int64()
    env.b.call("vec_axpby", x.vec.h, float(alpha), y.vec.h, float(beta), k.ctypes.data_as(C.POINTER(C.c_int64)),
               v.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(out))
    return k[:out.value], v[:out.value]


def g_capacity_error(env):
    rng = np.random.default_rng(3109)
    xk = 2 * np.arange(1, 301)
    yk = np.concatenate([xk[:50], 2 * np.arange(150) + 1001])
    x, y = env.mk(xk, rng.standard_normal(300)), env.mk(np.sort(yk), rng.standard_normal(200))
    wk, wv = env.check_axpby(x, A3, y, B7)                        # the scratch of this size has been in the pool once
    count = len(wk)
    assert count == 450
    idle = None if env.cpu else env.dsa.pool_idle_bytes(env.b)
    with pytest.raises(env.dsa.binding.DsaError) as ei:
        raw_axpby(env, x, A3, y, B7, count - 1)
    assert ei.value.code == env.dsa.binding.ECAP
    if idle is not None:
        assert env.dsa.pool_idle_bytes(env.b) >= idle             # the scratch went back
    gk, gv = raw_axpby(env, x, A3, y, B7, count)
    assert np.array_equal(gk, wk) and same_values(gv, wv)
    env.check_axpby(x, A3, y, B7)
    env.check_axpby(y, 1.0, x, -1.0)


# ================================================================== axpby 10: queued writes, reuse of the alternate buffers
def g_queued_and_reuse(env):
    rng = np.random.default_rng(3110)
    xk = 3 * np.arange(1, 301)
    x, y = env.mk(xk, rng.standard_normal(300)), env.mk(xk[::2] + np.arange(150) % 2, rng.standard_normal(150))
    for t, keys in ((x, xk), (y, y.k.copy())):
        t.set(1000, 1.5)
        t.set(2, -0.25)
        t.set(W31 - 5, 3.0)                           # new keys
        t.set(int(keys[10]), 7.125)                   # overwrite
        t.set(int(keys[20]), 0.0)                     # delete
    env.check_axpby(x, A3, y, B7)                     # nothing has observed x or y since the writes were queued
    env.check_equal(x, y, False)
    env.check_operand(x)
    env.check_operand(y)
    for nx, ny in ((3000, 3000), (45876, 3000)):
        xk = 4 * np.arange(1, nx + 1)
        x = env.mk(xk, rng.standard_normal(nx))
        y = env.mk(xk[:: nx // ny][:ny] + np.arange(ny) % 2, rng.standard_normal(ny), n=x.n)      # every second key shared with x
        assert small(x) == (nx == 3000) and small(y)
        fresh = np.zeros(0, dtype=np.int64)
        for r in range(6):
            gone = fresh[::2]                          # half of the last round's keys leave again
            fresh = 4 * rng.choice(nx, 2000, replace=False) + 2 + (r % 2)      # absent from x; shared with nothing
            keys = np.concatenate([gone, fresh])
            y.set_batch(keys, np.concatenate([np.zeros(len(gone)), rng.standard_normal(2000)]))
            assert merged_small(x, y)
            env.check_axpby(x, A3, y, B7)
            env.check_axpby(y, A3, x, B7)
            env.check_equal(x, y, False)
            env.check_equal(y, env.mk(y.k, y.v, n=y.n), True)
        env.check_operand(y)
        env.check_operand(x)


# ================================================================== == 1: counts and twins
EQ_COUNTS = (1, 63, 64, 65, 255, 256, 257, 4096, 45875, 45876)


def g_eq_twins(env):
    rng = np.random.default_rng(3201)
    for n in EQ_COUNTS:
        k = 2 * np.arange(1, n + 1)
        a = env.mk(k, rng.standard_normal(n))
        assert small(a) == (n != 45876)
        if n >= 45875:
            assert a.capacity() == (65536 if n == 45875 else 131072)
        twin = env.mk(*a.vec.nonzeros(), n=a.n)
        env.check_equal(a, twin, True)
        env.check_equal(a, env.mk(k, rng.standard_normal(n)), False)
        assert (a.vec == a.vec) is True


# ================================================================== == 2: one mismatch
def g_eq_single(env):
    rng = np.random.default_rng(3202)
    for n in (256, 257, 4096, 45875, 45876):
        k = 2 * np.arange(1, n + 1)                   # every cell has room before its successor
        a = env.mk(k, rng.standard_normal(n))
        assert small(a) == (n != 45876)
        K, V, O = a.vec.export_layout()
        seg = a.vec.info()["segment_capacity"]
        pos = np.flatnonzero(O)
        for i in sorted({0, 63, 64, 255, 256, n - 1} - {n}):
            p = pos[i]

            def variant(key=None, val=None):
                K2, V2 = K.copy(), V.copy()
                if key is not None:
                    K2[p] = key
                if val is not None:
                    V2[p] = val
                return env.imp(K2, V2, O, seg, a.n)

            env.check_equal(a, variant(key=K[p] + 1), False)
            env.check_equal(a, variant(val=np.nextafter(V[p], np.inf)), False)
            nan1, nan2 = variant(val=np.nan), variant(val=np.nan)
            env.check_equal(nan1, nan2, False)
            assert (nan1.vec == nan1.vec) is True     # the identity shortcut of the reference
            env.check_equal(variant(val=0.0), variant(val=-0.0), True)
            env.check_equal(a, variant(), True)


# ================================================================== == 3: same content, other layout and pack path
def g_eq_layouts(env):
    rng = np.random.default_rng(3203)
    n = 45875
    k = 2 * np.arange(1, n + 1)
    a = env.mk(k, rng.standard_normal(n))
    K, V, O = a.vec.export_layout()
    seg = a.vec.info()["segment_capacity"]
    K2, V2, O2 = (np.concatenate([q, np.zeros(len(q), dtype=q.dtype)]) for q in (K, V, O))
    b = env.imp(K2, V2, O2, seg, a.n)
    assert a.capacity() == 65536 and b.capacity() == 131072
    env.check_equal(a, b, True)
    env.check_axpby(a, A3, b, B7)
    env.check_axpby(b, A3, a, B7)
    wk, _ = env.check_axpby(a, 1.0, b, -1.0)
    assert len(wk) == 0
    V3 = V2.copy()
    last = np.flatnonzero(O2)[-1]
    V3[last] = np.nextafter(V3[last], -np.inf)
    env.check_equal(a, env.imp(K2, V3, O2, seg, a.n), False)
    # cells packed to the left against the same content spread by rebalance_root
    for n, cap in ((3000, 8192), (45876, 131072)):
        k = 3 * np.arange(1, n + 1)
        v = rng.standard_normal(n)
        Kl, Vl, Ol = np.zeros(cap, dtype=np.int64), np.zeros(cap), np.zeros(cap, dtype=np.uint8)
        Kl[:n], Vl[:n], Ol[:n] = k, v, 1
        left, spread = env.imp(Kl, Vl, Ol, 64, int(k[-1])), env.imp(Kl, Vl, Ol, 64, int(k[-1]))
        spread.vec.rebalance_root()
        assert not np.array_equal(left.vec.export_layout()[2], spread.vec.export_layout()[2])
        env.check_operand(spread)
        env.check_equal(left, spread, True)
        env.check_equal(left, env.mk(k, v), True)
        env.check_axpby(left, A3, spread, B7)


# ================================================================== == 4: the length rule
def g_eq_length(env):
    rng = np.random.default_rng(3204)
    n = 500
    k = 2 * np.arange(1, n + 1)
    v = rng.standard_normal(n)
    a, w = env.mk(k, v), env.mk(k, v)
    w.set(1 << 20, 1.0)
    w.set(1 << 20, 0.0)
    assert w.n == 1 << 20 and a.n == 2 * n
    env.check_equal(a, w, False)                      # equal content, different length
    env.check_operand(w)
    w.shrink_size()
    env.check_equal(a, w, True)
    one_less = env.mk(np.delete(k, 250), np.delete(v, 250), n=a.n)
    env.check_equal(a, one_less, False)               # equal length, one cell fewer
    other_last = env.mk(np.concatenate([k[:-1], [k[-1] - 1]]), v, n=a.n)
    env.check_equal(a, other_last, False)


# ================================================================== == 5: 32-bit against 64-bit physical keys
def g_eq_widths(env):
    rng = np.random.default_rng(3205)
    n = 45876
    k = 2 * np.arange(1, n + 1)
    v = rng.standard_normal(n)
    a, w = env.mk(k, v), env.mk(k, v)
    w.set(W40, 1.0)
    w.set(W40, 0.0)                                   # w keeps 64-bit keys in the HIP library
    w.shrink_size()
    assert a.capacity() == w.capacity() == 131072
    env.check_operand(w)
    env.check_equal(a, w, True)
    w.set(int(k[-1]), np.nextafter(v[-1], np.inf))
    env.check_equal(a, w, False)


# ================================================================== nonzeros() / pack on large and hand-made layouts
def g_pack_layouts(env):
    rng = np.random.default_rng(3301)
    n = 100000
    big = env.mk(3 * np.arange(1, n + 1), rng.standard_normal(n))
    assert big.capacity() == 262144
    env.check_equal(big, env.mk(*big.vec.nonzeros()), True)
    cap = 131072
    last_word = np.zeros(cap, dtype=np.uint8)
    last_word[cap - 64:] = 1                          # cells only in the last 64-slot word of the last tile
    borders = np.zeros(cap, dtype=np.uint8)
    edge = TILE * np.arange(1, cap // TILE)
    borders[edge - 1] = 1                             # the last slot of every tile and the first of the next one
    borders[edge] = 1
    borders[[0, cap - 1]] = 1
    for occ in (last_word, borders):
        m = occ.astype(bool)
        cnt = int(m.sum())
        K, V = np.zeros(cap, dtype=np.int64), np.zeros(cap)
        K[m], V[m] = 11 * np.arange(1, cnt + 1), rng.standard_normal(cnt)
        t = env.imp(K, V, occ, 64, 11 * cnt)
        twin = env.mk(K[m], V[m])
        assert not small(t) and small(twin)
        env.check_equal(t, twin, True)                # the same content through k_compact and through the one-launch pack
        env.check_axpby(t, A3, twin, B7)
        wk, _ = env.check_axpby(twin, 1.0, t, -1.0)
        assert len(wk) == 0


GROUPS = {
    "axpby1_split": g_split, "axpby2_keep_words": g_keep_words, "axpby3_operand_switch": g_operand_switch,
    "axpby4_merged_switch": g_merged_switch, "axpby5_tiles": g_tiles, "axpby6_key_widths": g_key_widths, "axpby7_self": g_self,
    "axpby8_specials": g_specials, "axpby9_capacity_error": g_capacity_error, "axpby10_queued_and_reuse": g_queued_and_reuse,
    "eq1_twins": g_eq_twins, "eq2_single": g_eq_single, "eq3_layouts": g_eq_layouts, "eq4_length": g_eq_length,
    "eq5_widths": g_eq_widths, "pack_layouts": g_pack_layouts,
}
# the groups in which at least one case has 256 both-stored keys under rounding coefficients: the contraction condition was applied
CONTRACTION_GROUPS = {"axpby2_keep_words", "axpby4_merged_switch", "axpby5_tiles", "axpby6_key_widths", "axpby7_self",
                      "axpby10_queued_and_reuse", "eq3_layouts"}


def run_group(env, name):
    GROUPS[name](env)
    print(f"{name}: {env.axpby_cases} axpby cases, {env.equal_cases} == cases, {env.operands} operands checked, "
          f"contraction condition on {env.contraction_cases}")


def test_models_on_literals():
    """the models on answers worked out by hand"""
    k, v = model_axpby([1, 3, 5], [1.0, 2.0, -0.0], 2.0, [3, 4, 5], [-4.0, 0.5, 0.0], 1.0)
    assert k.tolist() == [1, 4] and v.tolist() == [2.0, 0.5]                 # 2*2 - 4 = 0 and -0.0 + 0.0 = 0.0 are dropped
    k, v = model_axpby([7], [np.inf], 0.0, [8], [-3.0], 0.0)
    assert k.tolist() == [7, 8] and np.isnan(v[0]) and v[1] == 0.0 and np.signbit(v[1])      # one-sided cells are kept
    k, v = model_axpby([], [], A3, [2], [3.0], B7)
    assert k.tolist() == [2] and v[0] == 0.7 * 3.0
    x, y = 0.1, 0.3
    assert model_axpby([1], [x], A3, [1], [y], B7)[1][0] == (A3 * x) + (B7 * y)
    assert model_equal(5, ([1, 2], [0.0, 1.0]), 5, ([1, 2], [-0.0, 1.0]))
    assert not model_equal(5, ([1], [np.nan]), 5, ([1], [np.nan]))
    assert not model_equal(5, ([1], [1.0]), 6, ([1], [1.0]))
    assert not model_equal(5, ([1], [1.0]), 5, ([2], [1.0]))
    assert not model_equal(5, ([1], [1.0]), 5, ([1, 2], [1.0, 1.0]))
    assert not same_values([0.0], [-0.0]) and same_values([np.nan, 1.0], [-np.nan, 1.0])
    assert exact_products(1.0, -1.0) and exact_products(0.0, 2.0) and not exact_products(A3, B7) and not exact_products(2.5, -0.75)


def test_contraction_would_show_on_normal_pairs():
    """the three contracted forms differ from the separately rounded one on at least 10 % of 2000 normal pairs, for the default
    coefficients and for (2.5, -0.75); with (1, +-1) no pair shows it, which is why those are not the default"""
    rng = np.random.default_rng(3001)
    x, y = rng.standard_normal(2000), rng.standard_normal(2000)
    for alpha, beta in ((A3, B7), (2.5, -0.75)):
        assert min(contraction_shares(x, y, alpha, beta)) >= 0.10
    assert max(contraction_shares(x[:200], y[:200], 1.0, -1.0)) == 0.0


@pytest.mark.parametrize("group", list(GROUPS))
def test_model_matches_oracle(dsa, oracle, group):
    """CPU half: every case of the group on the oracle, bit for bit against the model; the contraction condition on its inputs"""
    env = Env(dsa, oracle, cpu=True)
    run_group(env, group)
    assert (env.contraction_cases > 0) == (group in CONTRACTION_GROUPS)


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_hip_matches_model(dsa, hip, group):
    """GPU half: the same cases on the HIP library, bit for bit against the model"""
    run_group(Env(dsa, hip, cpu=False), group)
