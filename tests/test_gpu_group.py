"""nbg_group_by on the GPU: GROUP BY with COUNT / SUM / AVG / MIN / MAX over result tables.

The expected tables are restated here in plain Python over canonical key tuples (a double becomes
("nan",) for every NaN and 0.0 for either zero; everything else compares by value), built with a
dict in first-occurrence order:

    key columns   the values of the group's first row (their bits: NaN payloads and the sign of a
                  zero travel with that row)
    COUNT         len(rows)
    SUM (int)     the sum wrapped to int64;   AVG (int)   float(that) / float(count)
    MIN / MAX     ORDER BY's order; a double extreme is canonical (+0.0, the quiet NaN)
    SUM (double)  the tree nebula_amd/csrc/group_agg.h documents, restated below (`tree_sum`): the
                  rows of a group in input order, summed by one lane (up to 16 values), by 64 lanes
                  and a halving (up to 4096) or in chunks of 16384 by 4 x 64 lanes each, the chunk
                  sums by 4 x 64 lanes again.  AVG (double) = that / count

and compared exactly, order included: doubles by bit pattern, except that a NaN sum is only
required to be a NaN.  Random finite groups are checked against math.fsum as well, within
n_g * 2^-52 * sum(|x_i|): any summation tree of n_g values is within (n_g - 1) * 2^-53 * sum(|x_i|)
to first order, so this is that standard bound with a factor 2 of slack; it is derived, not measured.
Without a DOUBLE sum the atomic path, the ordered path (option group_sorted) and both atomic
variants (option group_lds_max) must return the same bits, and every case runs through all of them.
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import fixtures as F
import oracle as O
from nebula_amd import GraphSpace, GroupByExecutor, NbgError, OrderByExecutor, _lib, synth
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

BOOL, INT, VID, DOUBLE, STRING = O.BOOL, O.INT, O.VID, O.DOUBLE, O.STRING
TIMESTAMP = _lib.T_TIMESTAMP
SUM, COUNT, AVG, MIN, MAX = _lib.AGG_SUM, _lib.AGG_COUNT, _lib.AGG_AVG, _lib.AGG_MIN, _lib.AGG_MAX
I64_MIN, I64_MAX = -2**63, 2**63 - 1
UNSET = -2**63  # nbg_set_option: removes the option
QNAN = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0]
NAN2 = struct.unpack("<d", struct.pack("<Q", 0xfff8000000000abc))[0]  # another payload, sign set
INF = math.inf
LARGE = 4096 * 256 + 1  # the grid-stride loops (4096 workgroups of 256) take a second trip


@pytest.fixture(scope="module")
def sp():
    s = GraphSpace(1)  # no snapshot: the call works on any context
    yield s
    s.close()


# ---- the restatement ---------------------------------------------------------------------------
def _canon(t, v):
    if t == DOUBLE:
        v = float(v)
        return ("nan",) if math.isnan(v) else (0.0 if v == 0 else v)
    if t == STRING:
        return v.encode() if isinstance(v, str) else bytes(v)
    if t == BOOL:
        return bool(v)
    return int(v)


def wrap64(s):
    return (s + 2**63) % 2**64 - 2**63


def tree_sum(x):
    """group_agg.h's segment tree in scalar code (the identity of the double sum is -0.0)"""
    def lane(first, step):
        s = -0.0
        for j in range(first, len(x), step):
            s = s + x[j]
        return s

    def halve(p):
        o = 32
        while o >= 1:
            for l in range(o):
                p[l] = p[l] + p[l + o]
            o //= 2
        return p[0]

    if len(x) <= 16:
        return lane(0, 1)
    if len(x) <= 4096:
        return halve([lane(l, 64) for l in range(64)])
    if len(x) > 16384:  # chunks of 16384 values, a workgroup each, and their sums by a workgroup again
        x = [tree_sum_block(x[at:at + 16384]) for at in range(0, len(x), 16384)]
    return tree_sum_block(x)


def tree_sum_block(x):
    """the 256-thread tree: thread t adds values t, t + 256, ...; each wave of 64 halves its sums;
    the four wave sums join as (w0 + w1) + (w2 + w3)"""
    w = []
    for wv in range(4):
        p = []
        for l in range(64):
            s = -0.0
            for j in range(wv * 64 + l, len(x), 256):
                s = s + x[j]
            p.append(s)
        o = 32
        while o >= 1:
            for l in range(o):
                p[l] = p[l] + p[l + o]
            o //= 2
        w.append(p[0])
    return (w[0] + w[1]) + (w[2] + w[3])


def _dkey(v):  # ORDER BY's double order: numeric, every NaN after +inf
    return (1, 0.0) if math.isnan(v) else (0, v)


def _dcanon(v):
    return QNAN if math.isnan(v) else 0.0 if v == 0 else v


def aggregate(fn, t, vals):
    """(output type, value) of one aggregate over one group's values (input order)"""
    if fn == COUNT:
        return INT, len(vals)
    if fn in (SUM, AVG):
        if t == DOUBLE:
            s = tree_sum([float(v) for v in vals])
            return DOUBLE, s if fn == SUM else s / float(len(vals))
        s = wrap64(sum(int(v) for v in vals))
        return (INT, s) if fn == SUM else (DOUBLE, float(s) / float(len(vals)))
    pick = min if fn == MIN else max
    if t == DOUBLE:
        return DOUBLE, _dcanon(pick((float(v) for v in vals), key=_dkey))
    if t == BOOL:
        return BOOL, pick(bool(v) for v in vals)
    return t, pick(int(v) for v in vals)


def agg_type(fn, t):
    if fn == COUNT:
        return INT
    if fn == AVG:
        return DOUBLE
    if fn == SUM:
        return DOUBLE if t == DOUBLE else INT
    return t


def expected(table, keys, aggs):
    """the output table as [(type, values)]"""
    n = len(table[0][1]) if table else 0
    groups = {}
    for r in range(n):
        groups.setdefault(tuple(_canon(table[k][0], table[k][1][r]) for k in keys), []).append(r)
    out = [(table[k][0], [table[k][1][rows[0]] for rows in groups.values()]) for k in keys]
    for fn, col in aggs:
        t = INT if fn == COUNT else table[col][0]
        vals = [aggregate(fn, t, [table[col][1][r] for r in rows] if fn != COUNT else rows)[1]
                for rows in groups.values()]
        out.append((agg_type(fn, t), vals))
    return out


def _bits(vals):
    return np.asarray(vals, dtype=np.float64).view(np.uint64)


def assert_table(rs, want, what=""):
    n = len(want[0][1]) if want else 0
    assert rs.n_rows == n, what
    assert rs.types == [t for t, _ in want], what
    for c, (t, vals) in enumerate(want):
        got = rs.columns[c]
        msg = f"column {c} (type {t}) {what}"
        if t == DOUBLE:
            g, w = _bits(got), _bits(vals)
            nan = np.isnan(np.asarray(vals, dtype=np.float64))
            if c >= what_keys(what) and nan.any():  # a NaN sum / average: any NaN
                assert np.isnan(np.asarray(got, dtype=np.float64)[nan]).all(), msg
                g, w = g[~nan], w[~nan]
            assert np.array_equal(g, w), msg
        elif t == STRING:
            assert [v.encode() if isinstance(v, str) else bytes(v) for v in got] == \
                   [v.encode() if isinstance(v, str) else bytes(v) for v in vals], msg
        elif t == BOOL:
            assert np.array_equal(np.asarray(got, dtype=bool), np.asarray(vals, dtype=bool)), msg
        else:
            assert np.array_equal(np.asarray(got, dtype=np.int64), np.asarray(vals, dtype=np.int64)), msg


def what_keys(what):
    """the number of key columns `what` carries (NaN leniency applies to SUM / AVG columns only:
    MIN / MAX return the one quiet NaN and key columns their row's bits)"""
    return what[0] if isinstance(what, tuple) else 10**9


class Opts:
    """engine options for the length of a with block"""

    def __init__(self, sp, **kv):
        self.sp, self.kv = sp, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.sp.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.sp.set_option(k, UNSET)


def has_double_sum(table, aggs):
    return any(fn in (SUM, AVG) and table[col][0] == DOUBLE for fn, col in aggs)


def lenient(table, keys, aggs):
    """assert_table's `what`: MIN / MAX over DOUBLE return the canonical NaN exactly, so only calls
    whose DOUBLE aggregate columns are all sums get the any-NaN rule"""
    if any(fn in (MIN, MAX) and table[col][0] == DOUBLE for fn, col in aggs):
        return f"keys {keys} aggs {aggs}"
    return (len(keys), f"keys {keys} aggs {aggs}")


VARIANTS = [dict(group_sorted=1), dict(group_lds_max=0), dict(group_lds_max=1 << 20)]


def check(sp, table, keys, aggs, want=None, variants=True):
    """run the call on every path defined for it and compare each result to the restatement"""
    if want is None:
        want = expected(table, keys, aggs)
    what = lenient(table, keys, aggs)
    rs = sp.group_by(table, keys, aggs)
    assert not rs.on_device
    assert_table(rs, want, what)
    if variants and not has_double_sum(table, aggs):
        for opt in VARIANTS:
            with Opts(sp, **opt):
                assert_table(sp.group_by(table, keys, aggs), want, what)
    return rs


# ---- sizes -------------------------------------------------------------------------------------
def value_table(n, groups, seed):
    """an INT key uniform over `groups` values, then INT, DOUBLE (integer-valued: every association
    of their sum is exact) and BOOL value columns"""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, max(groups, 1), n, dtype=np.int64) * 1_000_003 - 77
    return [(INT, key), (INT, rng.integers(-10**12, 10**12, n, dtype=np.int64)),
            (DOUBLE, rng.integers(-2**20, 2**20, n).astype(np.float64)), (BOOL, rng.integers(0, 2, n).astype(bool))]


EXACT_AGGS = [(COUNT, None), (SUM, 1), (AVG, 1), (MIN, 1), (MAX, 1), (MIN, 3), (MAX, 3), (MIN, 2), (MAX, 2)]
DOUBLE_AGGS = [(SUM, 2), (AVG, 2), (COUNT, None), (MAX, 1)]


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1023, 1024, 1025])
def test_sizes(sp, n):
    for groups in (1, max(1, n // 3), 10 * n + 1):  # G = 1, a few rows per group, G = n (or nearly)
        t = value_table(n, groups, 100 + n)
        if groups > n:
            t[0] = (INT, np.arange(n, dtype=np.int64)[::-1] * 3)  # G = n exactly
        check(sp, t, [0], EXACT_AGGS)
        check(sp, t, [0], DOUBLE_AGGS)
    t = value_table(n, 7, 200 + n)
    check(sp, t, [], EXACT_AGGS)       # n_keys = 0: one group (none for n = 0)
    check(sp, t, [], DOUBLE_AGGS)      # (1025 rows in one group: a wave's segment)
    check(sp, t, [0, 3], [])           # n_aggs = 0: DISTINCT projection


def np_expected(key, ival, dval):
    """COUNT, SUM / MIN / MAX of ival and SUM of the integer-valued dval per key, in
    first-occurrence order, with numpy"""
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    cnt = np.bincount(inv, minlength=len(uniq))
    by_group = np.argsort(inv, kind="stable")
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    iv, dv = ival[by_group], dval[by_group]
    s = np.add.reduceat(iv, starts)  # int64: wraps
    mn, mx = np.minimum.reduceat(iv, starts), np.maximum.reduceat(iv, starts)
    ds = np.add.reduceat(dv, starts)
    return [a[order] for a in (uniq, cnt, s, mn, mx, ds)]


@pytest.fixture(scope="module")
def large():
    out = {}
    for groups in (3, 100_000):
        t = value_table(LARGE, groups, 7 + groups)
        out[groups] = (t, np_expected(t[0][1], t[1][1], t[2][1]))
    return out


@pytest.mark.parametrize("groups", [3, 100_000])
def test_large_table(sp, large, groups):
    t, (uniq, cnt, s, mn, mx, ds) = large[groups]
    aggs = [(COUNT, None), (SUM, 1), (MIN, 1), (MAX, 1)]
    want = [(INT, uniq), (INT, cnt), (INT, s), (INT, mn), (INT, mx)]
    dev = sp.order_by(t, [], keep_on_device=True)
    for opt, waits in ((dict(), 2), (dict(group_lds_max=0), 2), (dict(group_sorted=1), 3)):
        with Opts(sp, **opt):
            rs = sp.group_by(dev, [0], aggs)
            tm = sp.last_timing()
        assert_table(rs, want, str(opt))
        assert tm["host_waits"] == waits and tm["hops"] == [] and tm["launches"] > 0 and tm["total_ms"] > 0, opt
    # the integer-valued DOUBLE sum is exact under every association (segments of ~350,000 rows
    # take the workgroup's tree, of ~10 rows a lane's)
    rs = sp.group_by(dev, [0], [(SUM, 2), (COUNT, None)])
    assert sp.last_timing()["host_waits"] == 3
    assert_table(rs, [(INT, uniq), (DOUBLE, ds), (INT, cnt)], "double sum")
    # no keys: one wait (the hand-out) on either path
    for opt in (dict(), dict(group_sorted=1)):
        with Opts(sp, **opt):
            rs = sp.group_by(dev, [], [(COUNT, None), (SUM, 1), (MIN, 1), (MAX, 1)])
            assert sp.last_timing()["host_waits"] == 1
        assert rs.rows() == [(LARGE, int(wrap64(int(t[1][1].sum()))), int(t[1][1].min()), int(t[1][1].max()))]


def test_lds_threshold(sp):
    # G = 5 on both sides of group_lds_max
    t = value_table(3000, 5, 31)
    want = expected(t, [0], EXACT_AGGS)
    assert len(want[0][1]) == 5
    for lds_max in (0, 4, 5):
        with Opts(sp, group_lds_max=lds_max):
            assert_table(sp.group_by(t, [0], EXACT_AGGS), want, f"group_lds_max {lds_max}")
    # G x accumulator words on both sides of the 4096-word LDS block: 9 aggregates, 8 of them with
    # a word of their own + the count = 9 words; 455 x 9 = 4095, 456 x 9 = 4104
    for groups in (455, 456):
        t = value_table(4000, groups, 32)
        t[0] = (INT, np.arange(4000, dtype=np.int64) % groups)
        check(sp, t, [0], EXACT_AGGS)


# ---- keys --------------------------------------------------------------------------------------
def test_int_keys_at_the_extremes(sp):
    k = [I64_MAX, I64_MIN, 0, -1, I64_MAX, 1, I64_MIN, I64_MIN + 1, I64_MAX - 1, 0]
    for t in (INT, VID, TIMESTAMP):
        rs = check(sp, [(t, k), (INT, list(range(10)))], [0], [(COUNT, None), (SUM, 1)])
        assert rs.rows()[:3] == [(I64_MAX, 2, 4), (I64_MIN, 2, 7), (0, 2, 11)]


def test_double_keys_zeros_and_nans(sp):
    k = [-0.0, QNAN, 0.0, 1.5, NAN2, -0.0, INF, -INF, NAN2, 1.5, 5e-324, -5e-324]
    rs = check(sp, [(DOUBLE, k), (INT, list(range(12)))], [0], [(COUNT, None), (SUM, 1)])
    # both zeros are one group, both NaN payloads one group, each with the bits of its first row
    assert rs.n_rows == 7
    assert list(_bits(rs.columns[0])[:2]) == [0x8000000000000000, 0x7ff8000000000000]
    assert list(rs.columns[1]) == [3, 3, 2, 1, 1, 1, 1] and list(rs.columns[2]) == [7, 13, 12, 6, 7, 10, 11]
    # the other first rows
    k2 = [0.0, NAN2, -0.0, QNAN]
    rs = check(sp, [(DOUBLE, k2)], [0], [(COUNT, None)])
    assert list(_bits(rs.columns[0])) == [0, 0xfff8000000000abc] and list(rs.columns[1]) == [2, 2]


def test_bool_and_string_keys(sp):
    b = [True, False, True, True, False]
    check(sp, [(BOOL, b), (INT, [1, 2, 3, 4, 5])], [0], [(COUNT, None), (SUM, 1), (MIN, 0), (MAX, 0)])
    # empty, embedded NUL, a value and its proper prefix, and values differing only in trailing NULs
    s = [b"", b"ab", b"a\0b", b"abc", b"", b"a\0b", b"ab\0", b"ab", b"a", b"a\0", b"abcdefgh", b"abcdefghi",
         b"abcdefgh", b"\0", b"\0\0"]
    rs = check(sp, [(STRING, s), (INT, list(range(len(s))))], [0], [(COUNT, None), (SUM, 1), (MIN, 1)])
    assert rs.n_rows == 11 and rs.columns[0][:4] == [b"", b"ab", b"a\0b", b"abc"]
    assert list(rs.columns[1])[:4] == [2, 2, 2, 1]
    check(sp, [(STRING, s)], [0], [])  # DISTINCT projection of a STRING column


def test_multi_column_and_repeated_keys(sp):
    n = 600
    rng = np.random.default_rng(5)
    t = [(INT, rng.integers(0, 3, n)), (STRING, [(b"x", b"", b"x\0")[i] for i in rng.integers(0, 3, n)]),
         (DOUBLE, np.array([0.0, -0.0, QNAN, NAN2, 2.5])[rng.integers(0, 5, n)]), (BOOL, rng.integers(0, 2, n).astype(bool)),
         (INT, rng.integers(-50, 50, n))]
    aggs = [(COUNT, None), (SUM, 4), (MIN, 4), (MAX, 2)]
    check(sp, t, [0, 1], aggs)
    rs = check(sp, t, [2, 0, 3], aggs)
    assert rs.n_rows == 3 * 3 * 2
    check(sp, t, [1, 2, 3, 0], [(AVG, 4)])
    # a repeated key column decides nothing and is output again
    rs = check(sp, t, [0, 0], [(COUNT, None)])
    assert rs.n_rows == 3 and rs.types == [INT, INT, INT] and list(rs.columns[0]) == list(rs.columns[1])
    rs = check(sp, t, [1, 0, 1], [(SUM, 4), (COUNT, -1)])  # COUNT ignores its column, -1 included
    assert rs.columns[0] == rs.columns[2]


# ---- aggregates --------------------------------------------------------------------------------
def test_integer_aggregates_at_the_extremes(sp):
    k = [1, 1, 2, 2, 2, 3, 3, 4]
    v = [I64_MAX, 1, I64_MIN, -1, 5, I64_MAX, I64_MIN, I64_MIN]
    for t in (INT, VID, TIMESTAMP):
        rs = check(sp, [(INT, k), (t, v)], [0], [(SUM, 1), (AVG, 1), (MIN, 1), (MAX, 1), (COUNT, None)])
        assert rs.types == [INT, INT, DOUBLE, t, t, INT]
        # INT64_MAX + 1 wraps to INT64_MIN, and AVG divides the wrapped sum
        assert rs.rows()[0] == (1, I64_MIN, -2.0**62, 1, I64_MAX, 2)
        assert rs.rows()[1] == (2, wrap64(I64_MIN - 1 + 5), float(wrap64(I64_MIN - 1 + 5)) / 3.0, I64_MIN, 5, 3)
        assert rs.rows()[2] == (3, -1, -0.5, I64_MIN, I64_MAX, 2)
    check(sp, [(INT, k), (INT, v)], [], [(SUM, 1), (AVG, 1), (MIN, 1), (MAX, 1)])


def test_double_min_max(sp):
    k = [1, 1, 1, 2, 2, 3, 3, 4, 4, 4, 5, 5, 6]
    v = [INF, -INF, 3.0, -0.0, 0.0, NAN2, NAN2, 7.5, NAN2, -2.5, 0.0, -0.0, -0.0]
    rs = check(sp, [(INT, k), (DOUBLE, v)], [0], [(MIN, 1), (MAX, 1)])
    mn, mx = _bits(rs.columns[1]), _bits(rs.columns[2])
    assert (mn[0], mx[0]) == tuple(_bits([-INF, INF]))
    assert (mn[1], mx[1]) == (0, 0) and (mn[4], mx[4]) == (0, 0) and (mn[5], mx[5]) == (0, 0)  # mixed zeros: +0.0
    assert (mn[2], mx[2]) == (0x7ff8000000000000, 0x7ff8000000000000)  # all NaN: the canonical NaN
    assert (mn[3], mx[3]) == (_bits([-2.5])[0], 0x7ff8000000000000)     # some NaN: NaN is the largest
    check(sp, [(INT, k), (DOUBLE, v)], [], [(MIN, 1), (MAX, 1)])


def test_double_sum_special_values(sp):
    k = [1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5, 5, 6, 6]
    v = [INF, -INF, 1.0, NAN2, 2.0, INF, 5.0, -INF, -INF, 1e308, 1e308, 1.0, -0.0, -0.0]
    rs = check(sp, [(INT, k), (DOUBLE, v)], [0], [(SUM, 1), (AVG, 1)])
    s, a = np.asarray(rs.columns[1]), np.asarray(rs.columns[2])
    assert np.isnan(s[0]) and np.isnan(s[1]) and np.isnan(a[0]) and np.isnan(a[1])  # inf + -inf, a NaN
    assert (s[2], s[3], s[4]) == (INF, -INF, INF) and (a[2], a[3]) == (INF, -INF)
    assert _bits(s)[5] == 0x8000000000000000  # a sum of -0.0s stays -0.0
    # the same values in groups long enough for the wave's tree
    reps = 40
    rs = check(sp, [(INT, k * reps), (DOUBLE, v * reps)], [0], [(SUM, 1), (AVG, 1)])
    s = np.asarray(rs.columns[1])
    assert np.isnan(s[0]) and np.isnan(s[1]) and (s[2], s[3], s[4]) == (INF, -INF, INF)


def test_double_sum_against_fsum_and_twice(sp):
    rng = np.random.default_rng(77)
    # groups of about 8 rows (a lane), 300 (a wave), one of 6000 (one chunk) and one of 40,000 (three)
    n = 64_000
    key = np.concatenate([rng.integers(0, 1000, 8000), 5000 + rng.integers(0, 33, 10_000), np.full(6000, 9999),
                          np.full(40_000, 9998)])
    val = rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))
    perm = rng.permutation(n)
    key, val = key[perm], val[perm]
    t = [(INT, key), (DOUBLE, val)]
    rs = check(sp, t, [0], [(SUM, 1), (AVG, 1), (COUNT, None)])  # bit-exact against the documented tree
    groups = {}
    for i in range(n):
        groups.setdefault(int(key[i]), []).append(float(val[i]))
    assert list(rs.columns[0]) == list(groups)
    classes = set()
    for g, (k, xs) in enumerate(groups.items()):
        classes.add(0 if len(xs) <= 16 else 1 if len(xs) <= 4096 else 2)
        bound = len(xs) * 2.0**-52 * math.fsum(abs(x) for x in xs)
        assert abs(rs.columns[1][g] - math.fsum(xs)) <= bound, (k, len(xs))
        assert abs(rs.columns[2][g] - math.fsum(xs) / len(xs)) <= bound / len(xs) + 2.0**-52 * abs(math.fsum(xs) / len(xs))
    assert classes == {0, 1, 2}
    # the same input gives the same bits on every run, on a host and on a device table
    dev = sp.order_by(t, [], keep_on_device=True)
    for again in (sp.group_by(t, [0], [(SUM, 1), (AVG, 1), (COUNT, None)]),
                  sp.group_by(dev, [0], [(SUM, 1), (AVG, 1), (COUNT, None)])):
        for c in range(4):
            assert np.asarray(again.columns[c]).tobytes() == np.asarray(rs.columns[c]).tobytes()


# ---- forced collisions -------------------------------------------------------------------------
def test_forced_hash_collisions(sp):
    rng = np.random.default_rng(9)
    n = 700
    t = [(INT, rng.integers(0, 40, n)), (STRING, [(b"k", b"k\0", b"", b"kk")[i] for i in rng.integers(0, 4, n)]),
         (DOUBLE, np.array([0.0, -0.0, QNAN, NAN2, 1.0])[rng.integers(0, 5, n)]), (INT, rng.integers(-9, 9, n))]
    aggs = [(COUNT, None), (SUM, 3), (MIN, 3), (MAX, 3)]
    for keys in ([0], [1], [2], [0, 1, 2]):
        want = expected(t, keys, aggs)
        for bits in (64, 4, 0):  # 0: every row collides with every other
            with Opts(sp, set_hash_bits=bits):
                assert_table(sp.group_by(t, keys, aggs), want, f"keys {keys} set_hash_bits {bits}")
                with Opts(sp, group_sorted=1):
                    assert_table(sp.group_by(t, keys, aggs), want, f"keys {keys} set_hash_bits {bits} sorted")


# ---- residency ---------------------------------------------------------------------------------
def test_residency(sp):
    n = 3000
    rng = np.random.default_rng(13)
    t = [(INT, rng.integers(0, 50, n)), (STRING, [b"s%d" % (i % 7) for i in range(n)]),
         (DOUBLE, rng.integers(-99, 99, n).astype(np.float64)), (INT, rng.integers(-10**6, 10**6, n))]
    keys, aggs = [1, 0], [(COUNT, None), (SUM, 3), (SUM, 2), (MIN, 3)]
    want = expected(t, keys, aggs)
    dev_in = sp.order_by(t, [], keep_on_device=True)
    for table in (t, dev_in):
        host = sp.group_by(table, keys, aggs)
        assert_table(host, want)
        dev = sp.group_by(table, keys, aggs, keep_on_device=True)
        assert dev.on_device and dev.n_rows == host.n_rows and dev.types == host.types
        assert_table(sp.order_by(dev, []), want)  # a device table comes back unchanged
    # the device input reads back unchanged after the calls
    back = sp.order_by(dev_in, [])
    assert_table(back, t)
    # a device output feeds order_by and set_op in place
    dev = sp.group_by(dev_in, keys, aggs, keep_on_device=True)
    ordered = sp.order_by(dev, [(2, 1), (0, 0), (1, 0)])
    rows = list(zip(*[v for _, v in want]))
    want_rows = sorted(rows, key=lambda r: (-r[2], r[0], r[1]))
    assert [tuple(r) for r in ordered.rows()] == [(a.decode(), int(b), int(c), int(d), float(e), int(f))
                                                   for a, b, c, d, e, f in want_rows]
    both = sp.set_op(_lib.SET_INTERSECT, dev, sp.group_by(t, keys, aggs, keep_on_device=True))
    assert_table(both, want)
    # zero rows: the output's column count and types, on either side of the link and without keys
    empty = [(INT, []), (STRING, []), (DOUBLE, []), (INT, [])]
    for k in (keys, []):
        for keep in (False, True):
            rs = sp.group_by(empty, k, aggs, keep_on_device=keep)
            assert rs.n_rows == 0 and rs.types == [t[c][0] for c in k] + [INT, INT, DOUBLE, INT] and rs.on_device == keep
            assert sp.last_timing()["host_waits"] == 1


# ---- chains ------------------------------------------------------------------------------------
NBA_TAGS = {F.NBA_PLAYER: ("player", [("name", O.STRING), ("age", O.INT)]),
            F.NBA_TEAM: ("team", [("name", O.STRING)])}


@pytest.fixture(scope="module")
def nba():
    s = GraphSpace(1)
    for et, (name, fields) in F.NBA_EDGE_SCHEMAS.items():
        s.set_edge_schema(et, fields)
    for tag, (name, fields) in NBA_TAGS.items():
        s.set_tag_schema(tag, name, fields)
    parts, vid = F.nba_kv()
    for p, kv in parts.items():
        s.load_part(p, kv)
    s.finalize()
    yield s, vid, F.nba()
    s.close()


def test_nba_players_per_team(nba):
    s, vid, data = nba
    # GO FROM <all players> OVER serve YIELD serve._dst AS team, $^.player.age AS age
    #   | GROUP BY $-.team YIELD $-.team, COUNT(*), AVG($-.age), MIN($-.age), MAX($-.age)
    players = [p["vid"] for p in data["players"]]
    go = s.go(players, 1, F.NBA_SERVE, yields=[X.EdgeDst("serve"), X.SourceProp("player", "age")],
              order_by=[], keep_on_device=True)  # the GO result stays in HBM
    serve = list(dict.fromkeys((who, team) for who, team, a, b in data["serve"]))  # one edge per (src, dst)
    assert go.on_device and go.n_rows == len(serve)
    ex = GroupByExecutor(s, ["$-.team"], [("COUNT", "*"), ("avg", "$-.age"), ("MIN", "age"), ("Max", "$-.age")],
                         ["team", "age"])
    dev = ex.execute(go, keep_on_device=True)
    rs = s.order_by(dev, [])
    age = {p["name"]: p["age"] for p in data["players"]}
    per_team = {}
    for who, team in serve:
        per_team.setdefault(vid[team], []).append(age[who])
    got = {r[0]: r[1:] for r in rs.rows()}
    assert len(got) == rs.n_rows == len(per_team)
    for team, ages in per_team.items():
        assert got[team] == (len(ages), float(sum(ages)) / float(len(ages)), min(ages), max(ages)), team
    # the groups come in the order of their first GO row
    first = list(dict.fromkeys(s.order_by(go, []).columns[0].tolist()))
    assert list(rs.columns[0]) == first
    # ... | ORDER BY $-.n DESC, on the device table
    top = OrderByExecutor(s, [("$-.n", "DESC"), ("team", "ASC")], ["team", "n", "avg", "lo", "hi"]).execute(dev)
    assert [(r[0], r[1]) for r in top.rows()] == sorted(((t, len(a)) for t, a in per_team.items()),
                                                        key=lambda r: (-r[1], r[0]))
    # a get_bound response is not a plain row table
    gb = s.get_bound(F.NBA_SERVE, [1], [vid["Boris Diaw"]], ["_dst", "start_year"])
    with pytest.raises(NbgError) as e:
        s.group_by(gb, [0], [(COUNT, None)])
    assert e.value.code == -1001
    assert s.group_by([(VID, gb.columns[0])], [], [(COUNT, None)]).rows() == [(5,)]


def test_rmat_two_hop_path_counts():
    s = GraphSpace(64)
    try:
        s.set_edge_schema(1, [("weight", 2)])
        s.gen_rmat(12, 16, 1, 1)
        s.finalize()
        starts = synth.seeds(12, 16, 1, 16)
        # GO 2 STEPS FROM starts OVER e | GROUP BY $-.id YIELD $-.id, COUNT(*): 2-hop paths per end vertex
        go = s.go(starts, 2, 1, order_by=[], keep_on_device=True)
        ids = s.order_by(go, []).columns[0]
        rs = GroupByExecutor(s, ["$-.id"], [("COUNT", None)], ["id"]).execute(go)
        uniq, cnt = np.unique(ids, return_counts=True)
        o = np.argsort(rs.columns[0], kind="stable")
        assert np.array_equal(np.asarray(rs.columns[0])[o], uniq) and np.array_equal(np.asarray(rs.columns[1])[o], cnt)
        assert int(np.asarray(rs.columns[1]).sum()) == go.n_rows > 1000
        assert rs.edges_scanned == go.edges_scanned > 0
        with Opts(s, group_sorted=1):
            again = s.group_by(go, [0], [(COUNT, None)])
        assert np.array_equal(again.columns[0], rs.columns[0]) and np.array_equal(again.columns[1], rs.columns[1])
    finally:
        s.close()


# ---- errors ------------------------------------------------------------------------------------
def raw_call(sp, table, keys, fns, cols, keep=0, n_keys=None, n_aggs=None, n_rows=None):
    """nbg_group_by below GraphSpace.group_by's own checks; returns the code"""
    rows, _keepalive, _ = sp._table_rows(table, "group_by")
    if n_rows is not None:
        rows.n_rows = n_rows
    arr = lambda v: None if v is None else C.cast((C.c_int32 * max(len(v), 1))(*v), C.c_void_p)
    out = _lib.Rows()
    rc = sp.L.nbg_group_by(sp.h, C.byref(rows), arr(keys), len(keys or []) if n_keys is None else n_keys, arr(fns),
                           arr(cols), len(fns or []) if n_aggs is None else n_aggs, keep, C.byref(out))
    if rc == 0:
        sp.L.nbg_rows_free(C.byref(out))
    return rc


T4 = [(INT, [1, 2, 1]), (BOOL, [True, False, True]), (STRING, [b"a", b"b", b"a"]), (DOUBLE, [1.0, 2.0, 3.0])]

BAD_CALLS = [
    ("neither a key nor an aggregate", dict(keys=[], fns=[], cols=[]), -1001),
    ("key column out of range", dict(keys=[4], fns=[COUNT], cols=[-1]), -1001),
    ("negative key column", dict(keys=[-1], fns=[COUNT], cols=[-1]), -1001),
    ("aggregate column out of range", dict(keys=[0], fns=[SUM], cols=[4]), -1001),
    ("negative aggregate column", dict(keys=[0], fns=[MIN], cols=[-1]), -1001),
    ("function 0", dict(keys=[0], fns=[0], cols=[0]), -1001),
    ("function 6", dict(keys=[0], fns=[6], cols=[0]), -1001),
    ("keep_on_device 2", dict(keys=[0], fns=[COUNT], cols=[-1], keep=2), -1001),
    ("null key array with a count", dict(keys=None, fns=[COUNT], cols=[-1], n_keys=1), -1001),
    ("null function array with a count", dict(keys=[0], fns=None, cols=[0], n_aggs=1), -1001),
    ("null column array with a count", dict(keys=[0], fns=[COUNT], cols=None, n_aggs=1), -1001),
    ("17 output columns", dict(keys=[0] * 9, fns=[COUNT] * 8, cols=[-1] * 8), -1003),
    ("2^32 rows", dict(keys=[0], fns=[COUNT], cols=[-1], n_rows=2**32), -1003),
    ("SUM over BOOL", dict(keys=[0], fns=[SUM], cols=[1]), -23),
    ("AVG over BOOL", dict(keys=[0], fns=[AVG], cols=[1]), -23),
    ("SUM over STRING", dict(keys=[0], fns=[SUM], cols=[2]), -23),
    ("AVG over STRING", dict(keys=[0], fns=[AVG], cols=[2]), -23),
    ("MIN over STRING", dict(keys=[0], fns=[MIN], cols=[2]), -1003),
    ("MAX over STRING", dict(keys=[0], fns=[MAX], cols=[2]), -1003),
]


@pytest.mark.parametrize("what, args, code", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_errors(sp, what, args, code):
    assert raw_call(sp, T4, **args) == code, what
    # after the refused call a good call still works
    assert sp.group_by(T4, [0], [(COUNT, None), (SUM, 3), (MAX, 1)]).rows() == [(1, 2, 4.0, True), (2, 1, 2.0, False)]


def test_sixteen_columns_and_bad_options(sp):
    rs = sp.group_by(T4, [0] * 8, [(COUNT, None)] * 8)
    assert rs.n_rows == 2 and len(rs.types) == 16
    with Opts(sp, group_sorted=2):
        with pytest.raises(NbgError) as e:
            sp.group_by(T4, [0], [(COUNT, None)])
        assert e.value.code == -1001
    with Opts(sp, group_lds_max=-1):
        with pytest.raises(NbgError) as e:
            sp.group_by(T4, [0], [(COUNT, None)])
        assert e.value.code == -1001
    with Opts(sp, set_hash_bits=65):
        with pytest.raises(NbgError) as e:
            sp.group_by(T4, [0], [(COUNT, None)])
        assert e.value.code == -1001
    assert sp.group_by(T4, [0], [(COUNT, None)]).rows() == [(1, 2), (2, 1)]


# ---- timing ------------------------------------------------------------------------------------
def test_timing_small_table(sp):
    t = value_table(257, 20, 3)
    exact, dbl = [(COUNT, None), (SUM, 1), (MIN, 1)], [(SUM, 2)]
    one = [(INT, np.zeros(257, dtype=np.int64))] + t[1:]
    cases = [
        (t, [0], exact, {}, 2),                      # atomic path: the group count, the hand-out
        (t, [0], exact, dict(group_lds_max=0), 2),
        (t, [0], [], {}, 2),                         # DISTINCT projection
        (t, [0], exact, dict(group_sorted=1), 3),    # ordered path: + the order's digit histogram
        (t, [0], dbl, {}, 3),
        (one, [0], dbl, {}, 2),                      # one group: nothing to order
        (t, [], exact, {}, 1),                       # no keys: the hand-out alone
        (t, [], dbl, {}, 1),
    ]
    for table, keys, aggs, opt, waits in cases:
        with Opts(sp, **opt):
            rs = sp.group_by(table, keys, aggs)
            tm = sp.last_timing()
        assert tm["host_waits"] == waits, (keys, aggs, opt)
        assert tm["hops"] == [] and tm["total_ms"] > 0 and tm["launches"] > 0
        assert rs.edges_scanned == 0
    # + the byte total of a device input's STRING column
    dev = sp.order_by([(INT, t[0][1]), (STRING, [b"s"] * 257)], [], keep_on_device=True)
    sp.group_by(dev, [0], [(COUNT, None)])
    assert sp.last_timing()["host_waits"] == 3
