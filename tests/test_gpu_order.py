"""nbg_order_by on the GPU: ORDER BY over result tables (src/graph/OrderByExecutor.cpp).

The expected order is restated here without the engine's key encoder: numpy's stable argsort /
lexsort on the raw values for integer tables, Python's stable `sorted` chained from the last
factor to the first otherwise.  The engine's sort is stable (rows equal under every factor keep
their input order), so values AND order are compared exactly; every table carries a row-number
column, which makes the permutation itself visible.

Sizes straddle a wave (64), a workgroup (256), both tile sizes (1024 rows up to 2^18 rows, 4096
above) and the point where the per-tile count scan spans more than one block.
"""
import itertools
import json
import math
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixtures as F
import oracle as O
from nebula_amd import GraphSpace, NbgError, OrderByExecutor, synth
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

BOOL, INT, VID, DOUBLE, STRING = O.BOOL, O.INT, O.VID, O.DOUBLE, O.STRING
I64_MIN, I64_MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module")
def sp():
    s = GraphSpace(1)  # no snapshot: the call works on any context
    yield s
    s.close()


# ---- the restatement ---------------------------------------------------------------------------
def _cmp_key(t, v):
    if t == DOUBLE:
        v = float(v)
        return (1, 0.0) if math.isnan(v) else (0, v)  # NaNs tie, after +inf; -0.0 == 0.0
    if t == STRING:
        return v.encode() if isinstance(v, str) else bytes(v)  # unsigned bytes, a prefix first
    if t == BOOL:
        return bool(v)
    return int(v)


def expected_perm(columns, factors):
    """row numbers in output order: stable sorts from the last factor to the first"""
    n = len(columns[0][1]) if columns else 0
    perm = list(range(n))
    for c, desc in reversed(factors):
        t, vals = columns[c]
        keys = [_cmp_key(t, v) for v in vals]
        perm = sorted(perm, key=lambda r: keys[r], reverse=bool(desc))  # reverse keeps ties in order
    return perm


def _same(t, got, want):
    if t == DOUBLE:  # bit patterns: NaN payloads and the sign of zero travel with their rows
        return np.array_equal(np.asarray(got, dtype=np.float64).view(np.int64),
                              np.asarray(want, dtype=np.float64).view(np.int64))
    if t == STRING:
        return list(got) == list(want)
    if t == BOOL:
        return np.array_equal(np.asarray(got, dtype=bool), np.asarray(want, dtype=bool))
    return np.array_equal(np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64))


def check(sp, columns, factors, perm=None, keep_on_device=False):
    """order `columns` by `factors`; every output column must be the input permuted by the expected
    permutation.  Returns the RowSet."""
    if perm is None:
        perm = expected_perm(columns, factors)
    rs = sp.order_by(columns, factors, keep_on_device=keep_on_device)
    host = sp.order_by(rs, []) if keep_on_device else rs  # a device table comes back unchanged
    assert host.n_rows == len(perm)
    assert host.types == [t for t, _ in columns]
    for c, (t, vals) in enumerate(columns):
        if t == STRING:
            want = [vals[r] for r in perm]
        else:
            want = np.asarray(vals)[np.asarray(perm, dtype=np.int64)] if len(perm) else np.asarray(vals)[:0]
        assert _same(t, host.columns[c], want), f"column {c} (type {t}) of {len(perm)} rows, factors {factors}"
    return rs


def rownum(n):
    return (VID, np.arange(n, dtype=np.int64))


# ---- sizes -------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257]
for _k in range(9, 15):
    SIZES += [2**_k - 1, 2**_k, 2**_k + 1]
SIZES += [50_000, 2**18, 2**18 + 1, 2**20 + 3]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_single_int_factor(sp, n):
    rng = np.random.default_rng(n + 1)
    span = max(2, n // 3)  # heavy ties: the payload shows that they keep their input order
    keys = rng.integers(-span, span, n, dtype=np.int64)
    perm = np.argsort(keys, kind="stable")
    check(sp, [(INT, keys), rownum(n)], [(0, 0)], perm=perm)
    t = sp.last_timing()
    assert t["hops"] == [] and t["host_waits"] >= 1
    if n > 1:
        assert t["launches"] > 0 and t["total_ms"] > 0


# ---- key shapes at n = 16 385 ------------------------------------------------------------------
N_SHAPE = 16_385


def _shape(name):
    rng = np.random.default_rng(11)
    if name == "all_equal":
        return np.full(N_SHAPE, -12345, dtype=np.int64)
    if name == "top_byte":
        return (rng.integers(0, 256, N_SHAPE, dtype=np.int64) << 56) + 0x1234  # negative for bytes >= 128
    if name == "low_byte":
        return (np.int64(0x0123456789ABCD) << 8) + rng.integers(0, 256, N_SHAPE, dtype=np.int64)
    if name == "full_range":
        k = rng.integers(I64_MIN, I64_MAX, N_SHAPE, dtype=np.int64, endpoint=True)
        k[[5, 77, 16_384]] = [I64_MAX, I64_MIN, I64_MIN]
        k[[6, 78]] = [I64_MIN, I64_MAX]
        return k
    assert name == "below_2_26"
    return rng.integers(0, 2**26, N_SHAPE, dtype=np.int64)


@pytest.mark.parametrize("name", ["all_equal", "top_byte", "low_byte", "full_range", "below_2_26"])
def test_key_shapes(sp, name):
    keys = _shape(name)
    perm = np.argsort(keys, kind="stable")
    rs = check(sp, [(INT, keys), rownum(N_SHAPE)], [(0, 0)], perm=perm)
    launches = sp.last_timing()["launches"]
    if name == "all_equal":  # no pass runs: the histogram pass alone, and the output is the input
        assert np.array_equal(rs.columns[1], np.arange(N_SHAPE))
        assert launches == 1
    if name in ("top_byte", "low_byte"):  # one digit differs: one pass (count, scan, scatter) + gather
        assert launches == 1 + 3 + 1
    if name == "below_2_26":
        check(sp, [(INT, _shape("full_range")), rownum(N_SHAPE)], [(0, 0)])
        full = sp.last_timing()["launches"]
        assert launches < full, (launches, full)
        assert launches == 1 + 4 * 3 + 1 and full == 1 + 8 * 3 + 1


# ---- types, DESC, ties -------------------------------------------------------------------------
def _doubles(n, rng):
    special = np.array([0.0, -0.0, math.inf, -math.inf, math.nan, 5e-324, -5e-324, 1.5, -1.5, 2.2250738585072014e-308],
                       dtype=np.float64)
    v = rng.choice(special, n)
    some = rng.random(n) < 0.3
    v[some] = rng.normal(0, 1e6, int(some.sum()))
    # NaNs with other payloads and signs: all tie
    bits = v.view(np.int64)
    nan_at = np.flatnonzero(np.isnan(v))
    bits[nan_at[::2]] = np.int64(-0x0007FFFFFFFFFFFF)  # 0xfff8000000000001: negative, payload 1
    bits[nan_at[1::3]] = np.int64(0x7FF0000000000123)  # signalling
    return v


@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("t", [INT, VID, DOUBLE, BOOL, STRING])
def test_single_factor_types(sp, t, desc):
    n = 3001
    rng = np.random.default_rng(100 + t)
    if t in (INT, VID):
        vals = rng.integers(-40, 40, n, dtype=np.int64)
        vals[:4] = [I64_MIN, I64_MAX, 0, -1]
    elif t == DOUBLE:
        vals = _doubles(n, rng)
    elif t == BOOL:
        vals = rng.random(n) < 0.4
    else:
        r = random.Random(5)
        vals = ["".join(r.choice("xyz") for _ in range(r.randrange(0, 12))) for _ in range(n)]
    check(sp, [(t, vals), rownum(n)], [(0, desc)])
    check(sp, [rownum(n), (t, vals)], [(1, desc)])  # the factor is not column 0


@pytest.mark.parametrize("d0,d1", list(itertools.product([0, 1], repeat=2)))
def test_two_factors_heavy_ties(sp, d0, d1):
    n = 20_011
    rng = np.random.default_rng(7)
    a = rng.integers(-3, 3, n, dtype=np.int64)
    b = _doubles(n, rng)
    cols = [(INT, a), (DOUBLE, b), rownum(n)]
    check(sp, cols, [(0, d0), (1, d1)])
    check(sp, cols, [(1, d1), (0, d0)])


def test_three_factors_mixed(sp):
    n = 10_007
    rng = np.random.default_rng(8)
    r = random.Random(8)
    cols = [(BOOL, rng.random(n) < 0.5), (STRING, [r.choice(["", "a", "ab", "b", "ba"]) for _ in range(n)]),
            (VID, rng.integers(0, 7, n, dtype=np.int64)), rownum(n), (DOUBLE, rng.random(n))]
    check(sp, cols, [(0, 1), (1, 0), (2, 1)])
    check(sp, cols, [(2, 0), (0, 0), (1, 1)])
    check(sp, cols, [(1, 1), (2, 1), (0, 0)], keep_on_device=True)


def test_duplicate_and_empty_factor_lists(sp):
    n = 5000
    rng = np.random.default_rng(9)
    cols = [(INT, rng.integers(0, 5, n, dtype=np.int64)), (INT, rng.integers(0, 5, n, dtype=np.int64)), rownum(n)]
    # a later repeat of a column decides nothing, whatever its direction
    perm = expected_perm(cols, [(0, 0), (1, 1)])
    check(sp, cols, [(0, 0), (1, 1), (0, 1)], perm=perm)
    check(sp, cols, [(0, 0), (0, 1), (1, 1), (1, 0)], perm=perm)
    # no factor: the input order (OrderByTest.WrongFactor)
    rs = check(sp, cols, [], perm=list(range(n)))
    assert sp.last_timing()["launches"] == 0
    assert np.array_equal(rs.columns[2], np.arange(n))


# ---- strings -----------------------------------------------------------------------------------
# the set of tests/cpp/order_keys_test.cpp
STRING_SET = [
    b"", b"a", b"a\0", b"a\0\0", b"ab", b"b", b"\0", b"abcdefgh", b"abcdefgi", b"abcdefgh0", b"abcdefgh1",
    b"abcdefgh\0", b"abcdefghijklmnop", b"abcdefghijklmnoq", b"abcdefghijklmnopq", b"abcdefghijklmnopr",
    b"abcdefghijklmnop\0", b"\x80", b"\xff", b"a\x80", b"a\x7f", b"\xff" * 8, b"\xff" * 8 + b"\x01", b"Z", b"z",
]


def _string_table():
    r = random.Random(21)
    vals = [bytes(r.choice(b"abc") for _ in range(r.randrange(0, 41))) for _ in range(5000)]
    vals += STRING_SET * 3  # every special value three times: ties
    r.shuffle(vals)
    return vals


@pytest.mark.parametrize("desc", [0, 1])
def test_strings_sole_factor(sp, desc):
    vals = _string_table()
    n = len(vals)
    rs = check(sp, [(STRING, vals), rownum(n)], [(0, desc)])
    assert all(isinstance(v, bytes) for v in rs.columns[0])  # bytes in, bytes out
    # longest value 40 bytes: the length key + 5 chunk keys, one host wait each, plus the hand-out
    # (and the STRING output's byte total)
    assert sp.last_timing()["host_waits"] <= 6 + 2


@pytest.mark.parametrize("d0,d1", [(0, 0), (1, 0), (0, 1)])
def test_strings_behind_an_int(sp, d0, d1):
    vals = _string_table()
    n = len(vals)
    lead = np.random.default_rng(22).integers(-2, 2, n, dtype=np.int64)
    check(sp, [(INT, lead), (STRING, vals), rownum(n)], [(0, d0), (1, d1)])


def test_string_factor_length_limit(sp):
    ok = [b"q" * 256, b"q" * 255 + b"p", b"", b"q" * 256 + b""]
    check(sp, [(STRING, ok), rownum(len(ok))], [(0, 0)])
    with pytest.raises(NbgError) as e:
        sp.order_by([(STRING, [b"a", b"q" * 257, b"b"]), rownum(3)], [(0, 0)])
    assert e.value.code == -1003
    # a long value in a column that is no factor is only carried along
    check(sp, [(STRING, [b"a", b"q" * 257, b"b"]), (INT, [3, 1, 2])], [(1, 0)])


# ---- the keys-only path ------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("n", [1, 1000, 70_001, 2**18 + 5])
def test_one_column_matches_the_general_path(sp, n, desc):
    rng = np.random.default_rng(n)
    keys = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    keys[rng.random(n) < 0.5] >>= 40  # a mix of wide and narrow values, both signs
    want = np.sort(keys)[::-1] if desc else np.sort(keys)
    alone = sp.order_by([(VID, keys)], [(0, desc)])
    assert np.array_equal(alone.columns[0], want)
    paired = sp.order_by([(VID, keys), rownum(n)], [(0, desc)])
    assert np.array_equal(paired.columns[0], alone.columns[0])
    dev = sp.order_by([(VID, keys)], [(0, desc)], keep_on_device=True)
    assert dev.on_device and np.array_equal(sp.order_by(dev, []).columns[0], want)


def test_one_constant_column(sp):
    keys = np.full(3000, 42, dtype=np.int64)
    assert np.array_equal(sp.order_by([(INT, keys)], [(0, 1)]).columns[0], keys)
    for t, vals in ((BOOL, np.arange(777) % 3 == 0), (DOUBLE, np.array([0.0, -0.0, 1.0, -0.0] * 50))):
        check(sp, [(t, vals)], [(0, 0)])  # one column of another type: the general path


# ---- errors ------------------------------------------------------------------------------------
def test_errors(sp):
    cols = [(INT, [3, 1, 2]), (VID, [0, 1, 2])]
    for bad in ([(2, 0)], [(-1, 0)], [(0, 0), (5, 1)]):
        with pytest.raises(NbgError) as e:
            sp.order_by(cols, bad)
        assert e.value.code == -1001
    for bad in ([(0, 2)], [(0, -1)], [(1, 0), (0, 7)]):
        with pytest.raises(NbgError) as e:
            sp.order_by(cols, bad)
        assert e.value.code == -1001
    check(sp, cols, [(0, 0)])  # the context still works


# ---- on graphs ---------------------------------------------------------------------------------
NBA_TAGS = {F.NBA_PLAYER: ("player", [("name", O.STRING), ("age", O.INT)]),
            F.NBA_TEAM: ("team", [("name", O.STRING)])}
GOLDEN = json.loads((F.GOLDEN / "order_by.json").read_text())


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
    yield s, vid
    s.close()


SERVE_YIELDS = [X.SourceProp("player", "name"), X.AliasProp("serve", "start_year"), X.DestProp("team", "name")]


def test_reference_single_factor(nba):
    s, vid = nba
    g = GOLDEN["single_factor"]
    for case in g["cases"]:
        ex = OrderByExecutor(s, [tuple(f) for f in case["factors"]], g["columns"])
        # through the executor on a host result, and as one GO ... | ORDER BY on the device
        rs = ex.execute(s.go([vid[g["start"]]], 1, F.NBA_SERVE, yields=SERVE_YIELDS))
        assert rs.rows() == [tuple(r) for r in case["rows"]]
        rs = s.go([vid[g["start"]]], 1, F.NBA_SERVE, yields=SERVE_YIELDS, order_by=ex.sort_factors)
        assert rs.rows() == [tuple(r) for r in case["rows"]]


def test_reference_multi_factors(nba):
    s, vid = nba
    g = GOLDEN["multi_factors"]
    ys = [X.DestProp("team", "name"), X.SourceProp("player", "name"), X.SourceProp("player", "age"),
          X.AliasProp("serve", "start_year")]
    w = X.AliasProp("serve", "start_year") >= g["min_start_year"]
    starts = [vid[p] for p in g["starts"]]
    for case in g["cases"]:
        ex = OrderByExecutor(s, [tuple(f) for f in case["factors"]], g["columns"])
        assert len(ex.sort_factors) == 2
        rs = s.go(starts, 1, F.NBA_SERVE, where=w, yields=ys, order_by=ex.sort_factors)
        assert rs.rows() == [tuple(r) for r in case["rows"]]


def test_reference_wrong_factor_and_no_input(nba):
    s, vid = nba
    g = GOLDEN["wrong_factor"]
    ex = OrderByExecutor(s, [tuple(f) for f in g["factors"]], g["columns"])
    assert ex.sort_factors == []
    plain = s.go([vid[g["start"]]], 1, F.NBA_SERVE, yields=SERVE_YIELDS)
    assert sorted(plain.rows()) == sorted(tuple(r) for r in g["rows"])
    assert ex.execute(plain).rows() == plain.rows()  # the GO order, untouched
    g = GOLDEN["no_input"]
    ex = OrderByExecutor(s, [tuple(f) for f in g["factors"]], g["columns"])
    assert ex.sort_factors == [(0, 0)]
    empty = s.go([vid[g["start"]]], 1, F.NBA_SERVE, yields=SERVE_YIELDS)
    assert empty.n_rows == 0
    for rs in (ex.execute(empty), s.go([vid[g["start"]]], 1, F.NBA_SERVE, yields=SERVE_YIELDS, order_by=[(0, 0)]),
               s.go([vid[g["start"]]], 1, F.NBA_SERVE, yields=SERVE_YIELDS, order_by=[(0, 0)], keep_on_device=True)):
        assert rs.n_rows == 0 and rs.types == empty.types
    assert g["rows"] == []


def test_reference_interim_result(nba):
    s, vid = nba
    g = GOLDEN["interim_result"]
    liked = s.go([vid[g["start"]]], 1, F.NBA_LIKE, order_by=[(0, 0)])  # GO OVER like | ORDER BY $-.id
    ids = liked.columns[0]
    assert len(ids) == 2 and ids[0] < ids[1]
    served = s.go(ids, 1, F.NBA_SERVE)                                  # | GO FROM $-.id OVER serve
    assert sorted(int(v) for v in served.columns[0]) == sorted(vid[t] for t in g["teams"])


def test_get_bound_result_is_refused(nba):
    s, vid = nba
    rs = s.get_bound(F.NBA_SERVE, [1], [vid["Boris Diaw"]], ["_dst", "start_year"])
    assert rs.n_rows == 5 and len(rs.row_vertex) == 5
    with pytest.raises(NbgError) as e:
        s.order_by(rs, [(0, 0)])
    assert e.value.code == -1001


def _rmat_space(rank=0, world=1):
    s = GraphSpace(64, device=0, rank=rank, world_size=world)
    s.set_edge_schema(1, [("weight", O.INT)])
    return s


@pytest.fixture(scope="module")
def rmat12():
    s = _rmat_space()
    s.gen_rmat(12, 16, 1, 1)
    s.finalize()
    yield s
    s.close()


def test_go_distinct_dst_ordered(rmat12):
    s = rmat12
    starts = synth.seeds(12, 16, 1, 16)
    q = dict(yields=[X.EdgeDst("follow")], distinct=True)
    plain = s.go(starts, 2, 1, **q)
    assert plain.n_rows > 100
    for desc in (0, 1):
        want = np.sort(plain.columns[0])[::-1] if desc else np.sort(plain.columns[0])
        for _ in range(2):  # the second call repeats the first one's arguments (the prepared spec)
            got = s.go(starts, 2, 1, order_by=[(0, desc)], **q)
            assert not got.on_device and np.array_equal(got.columns[0], want)
    again = s.go(starts, 2, 1, **q)  # and a call without order_by is not ordered by the cache's doing
    assert np.array_equal(again.columns[0], plain.columns[0])


def test_host_against_device_input(rmat12):
    s = rmat12
    starts = synth.seeds(12, 16, 1, 8)
    q = dict(where=X.AliasProp("follow", "weight") > 300, yields=[X.EdgeDst("follow"), X.AliasProp("follow", "weight")])
    factors = [(1, 1), (0, 0)]  # every column is a factor: the order is total whatever order GO gave
    plain = s.go(starts, 2, 1, **q)
    w, d = plain.columns[1], plain.columns[0]
    perm = np.lexsort((d, -w))
    assert len(perm) > 1000
    host = s.order_by(plain, factors)
    via_go = s.go(starts, 2, 1, order_by=factors, **q)
    dev = s.go(starts, 2, 1, order_by=factors, keep_on_device=True, **q)
    assert dev.on_device and dev.n_rows == plain.n_rows and dev.edges_scanned == plain.edges_scanned
    back = s.order_by(dev, [])
    dev2 = s.order_by(plain, factors, keep_on_device=True)
    back2 = s.order_by(dev2, [(0, 0), (1, 0)], keep_on_device=False)  # a device table as the input of a real sort
    for rs in (host, via_go, back):
        assert np.array_equal(rs.columns[0], d[perm]) and np.array_equal(rs.columns[1], w[perm])
    p2 = np.lexsort((w, d))
    assert np.array_equal(back2.columns[0], d[p2]) and np.array_equal(back2.columns[1], w[p2])


def test_two_ranks_order_their_own_rows():
    world = 2
    sps = [_rmat_space(r, world) for r in range(world)]
    pool = ThreadPoolExecutor(max_workers=world)
    try:
        for s in sps:
            s.comm_init_local(9100)

        def each(fn):
            return [f.result(timeout=300) for f in [pool.submit(fn, s) for s in sps]]

        each(lambda s: s.gen_rmat(12, 16, 1, 1))
        each(lambda s: s.finalize())
        starts = synth.seeds(12, 16, 1, 16)
        q = dict(yields=[X.EdgeDst("follow")], distinct=True)
        plain = each(lambda s: s.go(starts, 2, 1, **q))
        ordered = each(lambda s: s.go(starts, 2, 1, order_by=[(0, 0)], **q))
        for p, o in zip(plain, ordered):  # rank-local: each rank's own rows, ordered; no exchange
            assert o.n_rows == p.n_rows > 0
            assert np.array_equal(o.columns[0], np.sort(p.columns[0]))
        assert np.array_equal(np.sort(np.concatenate([o.columns[0] for o in ordered])),
                              np.sort(np.concatenate([p.columns[0] for p in plain])))
        assert all(t["comm_calls"] == 0 for t in each(lambda s: s.last_timing()))
    finally:
        for s in sps:
            s.close()
        pool.shutdown()
