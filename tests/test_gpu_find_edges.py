"""FIND props FROM an edge type WHERE (nbg_find_edges): the device column scan.

The expectation is restated here from the KV pairs the test writes, as test_gpu_fetch_edges.py's
Writer does: the own-part (src, rank, dst) groups, the bytewise-first version of each, the last write
of identical keys.  Inside one source's row the entries follow the row's own order (bytewise by rank,
then dst), so a space whose edges all leave one source has a known entry order and its rows are
compared as exact lists; with several sources the order of the rows among each other is the
engine's numbering, so the rows are compared source by source (each source's rows contiguous and in
row order) and as a multiset.  Doubles are compared by bits, strings as bytes.  Every case runs with
find_fast 0, 1 and unset; the three must agree with the restatement and with each other row for row
(and a repeated call with itself): the determinism check.

The numbering puts sources with in-edges first, then the vertices with in-edges only (empty rows),
then the sources without in-edges, so the spaces below have runs of empty rows between rows and at
the end; a leading run is covered by tests/cpp/find_scan_test.cpp.

Launch and wait counts asserted below (include/nebula_amd.h): typed compare 3 launches + the
materialiser's 1 (+ 1 on the first call on a type), otherwise 5 + 1; host_waits 3 with rows, 2 without,
1 with nothing to scan.
"""
import ctypes as C
import struct
from collections import Counter

import numpy as np
import pytest

import oracle as O
from nebula_amd import FindExecutor, GraphSpace, NbgError, _lib
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

PARTS = 3
REL = 7
FIELDS = [("i", O.INT), ("d", O.DOUBLE), ("b", O.BOOL), ("s", O.STRING), ("j", O.INT)]
PI, PD, PB, PS, PJ = (X.AliasProp("rel", f) for f in ("i", "d", "b", "s", "j"))
KSRC, KDST, KRANK = (X.AliasProp("rel", f) for f in ("_src", "_dst", "_rank"))
MODES = [0, 1, None]
E_STATE, E_INVALID_ARG, E_UNSUPPORTED, E_IMPROPER_DATA_TYPE, E_EVAL = -1002, -1001, -1003, -23, -1004
TILE = 2048


def le(v):
    return struct.pack("<q", v)


def bits(v):
    if isinstance(v, float):
        return ("f64", struct.pack("<d", v))
    if isinstance(v, str):
        return v.encode()
    return v


def got(rs):
    return [tuple(bits(c) for c in r) for r in rs.rows()]


def mix(j):
    v = (j * 0x9E3779B97F4A7C15 + 0x1234567) % (1 << 64)
    return v - (1 << 64) if v >= (1 << 63) else v


class Writer:
    """collects KV pairs and the restated winner of every own-part (src, rank, dst) group"""

    def __init__(self, parts):
        self.n_parts = parts
        self.parts = {p: [] for p in range(1, parts + 1)}
        self.groups = {}
        self.seq = 0

    def edge(self, src, dst, rank, ver, props, part=None, etype=REL, encoded=None):
        own = O.part_of(src, self.n_parts)
        part = own if part is None else part
        self.seq += 1
        val = encoded if encoded is not None else O.encode_row(list(props))
        self.parts[part].append((O.edge_key(part, src, etype, rank, dst, ver), val))
        pd = O.part_of(dst, self.n_parts)
        self.parts[pd].append((O.edge_key(pd, dst, -etype, rank, src, ver), b""))
        if part == own and etype == REL:
            self.groups.setdefault((src, rank, dst), []).append((le(ver), self.seq, tuple(props)))

    def edges(self):
        out = {}
        for k, ws in self.groups.items():
            first = min(w[0] for w in ws)
            out[k] = max((w for w in ws if w[0] == first), key=lambda w: w[1])[2]
        return out

    def load(self, sp, write=False):
        for p, kv in self.parts.items():
            if kv:
                (sp.write_part if write else sp.load_part)(p, kv)


def set_mode(sp, m):
    if m is None:
        sp.unset_option("find_fast")
    else:
        sp.set_option("find_fast", m)


def row_order(edges, src):
    return sorted(((k[1], k[2]) for k in edges if k[0] == src), key=lambda e: (le(e[0]), le(e[1])))


def restate(edges, where=lambda k, p: True, cols=lambda k, p: ()):
    """{src: [row]} of the passing entries, each source's in its row's order; a row = (_src, _dst, _rank) + cols"""
    out = {}
    for src in sorted({k[0] for k in edges}):
        rows = []
        for r, d in row_order(edges, src):
            k, p = (src, r, d), edges[(src, r, d)]
            if where(k, p):
                rows.append((src, d, r) + tuple(bits(c) for c in cols(k, p)))
        if rows:
            out[src] = rows
    return out


def check_rows(rows, want):
    """rows against restate()'s {src: [row]}: every source's rows contiguous and in row order"""
    assert Counter(rows) == Counter(r for rs in want.values() for r in rs)
    seen, at = [], 0
    while at < len(rows):
        src = rows[at][0]
        assert src not in seen, "a source's rows are contiguous"
        seen.append(src)
        n = len(want[src])
        assert rows[at:at + n] == want[src]
        at += n


def find_all_modes(sp, where, yields=(), keep=False, et=REL):
    """the call under find_fast 0, 1, unset and unset again; asserts the four results equal, returns one"""
    res = []
    for m in MODES + [None]:
        set_mode(sp, m)
        rs = sp.find_edges(et, where, yields, keep_on_device=keep)
        assert rs.on_device == keep
        if keep:
            rs = sp.order_by(rs, [])  # the rows on the host, in place order
        res.append((rs.types, got(rs)))
    assert res[0] == res[1] == res[2] == res[3]
    return res[0]


def code_of(fn):
    with pytest.raises(NbgError) as e:
        fn()
    return e.value.code


# ---- one source: the entry order is the row's order -------------------------------------------------
OFFSET = {1: 0, 2: 1000, 4: 100000, 8: 1 << 40}  # the stored width of column i follows its value range
SRC1 = 500


def value_at(pos, n, width):
    """column i by entry position: 0..99 cycling, and a value of its own at the positions the tile logic turns on"""
    special = {0: 120, TILE - 1: 121, TILE: 122, n - 1: 123}
    return OFFSET[width] + (special[pos] if pos in special else pos % 100)


def one_row_space(n, width):
    """n edges out of SRC1 (one row: it spans every tile boundary below n) and one edge of another type, so
    the space has vertices when n = 0.  Every dst has in-edges only: their empty rows follow the row."""
    w = Writer(PARTS)
    dsts = sorted((mix(j) for j in range(1, n + 1)), key=le)
    for pos, d in enumerate(dsts):
        v = value_at(pos, n, width)
        w.edge(SRC1, d, 0, 9, (v, pos * 0.5, pos % 2 == 0, f"p{pos}", -pos))
    w.edge(1, 2, 0, 9, (1,), etype=REL + 1)
    sp = GraphSpace(PARTS)
    sp.set_edge_schema(REL, FIELDS, name="rel")
    sp.set_edge_schema(REL + 1, [("x", O.INT)], name="other")
    w.load(sp)
    sp.finalize()
    return sp, w.edges(), dsts


@pytest.mark.parametrize("width", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5])
def test_one_row_tiles_and_widths(n, width):
    sp, edges, dsts = one_row_space(n, width)
    try:
        off = OFFSET[width]
        vals = [value_at(p, n, width) for p in range(n)]
        cases = [("none", PI > off + 126, lambda v: v > off + 126),
                 ("all", PI >= off, lambda v: True),
                 ("entry 0", PI.eq(off + 120), lambda v: v == off + 120),
                 ("last of tile 0", PI.eq(off + 121), lambda v: v == off + 121),
                 ("first of tile 1", PI.eq(off + 122), lambda v: v == off + 122),
                 ("last", X.Primary(off + 123).eq(PI), lambda v: v == off + 123),
                 ("scattered <", PI < off + 37, lambda v: v < off + 37),
                 ("scattered <=", PI <= off + 37, lambda v: v <= off + 37),
                 ("scattered !=", PI.ne(off + 5), lambda v: v != off + 5),
                 ("constant first", X.Primary(off + 90) < PI, lambda v: v > off + 90),
                 ("general: arithmetic", PI + 1 > off + 91, lambda v: v > off + 90),
                 ("general: no where", None, lambda v: True)]
        for name, where, f in cases:
            types, rows = find_all_modes(sp, where, [PI])
            want = [(SRC1, dsts[p], 0, vals[p]) for p in range(n) if f(vals[p])]
            assert rows == want, name
            assert types == [_lib.T_VID] * 4
        if n > TILE + 1:  # the special positions are distinct entries
            assert [len([v for v in vals if v == off + s]) for s in (120, 121, 122, 123)] == [1, 1, 1, 1]
        # the timing contract, typed compare and general
        for m, where, launches in ((1, PI >= off, 3), (0, PI >= off, 5), (None, PD < 1e9, 5)):
            set_mode(sp, m)
            sp.find_edges(REL, where)  # (a first typed call on the type builds its tile table: one more launch)
            rs = sp.find_edges(REL, where)
            t = sp.last_timing()
            assert t["hops"] == [] and t["edges_scanned"] == rs.edges_scanned == n
            if n == 0:
                assert t["host_waits"] == 1 and t["launches"] == 0 and t["expand_launches"] == 0
                continue
            assert rs.n_rows > 0 and t["host_waits"] == 3
            assert t["launches"] == launches + 1  # + the materialiser
            assert t["expand_launches"] == (2 if launches == 3 else 1)
            assert t["expand_bytes"] > 0 and t["expand_ms"] > 0 and t["total_ms"] >= t["expand_ms"]
        if n:
            set_mode(sp, None)
            sp.find_edges(REL, PI > off + 126)
            t = sp.last_timing()
            assert t["host_waits"] == 2 and t["launches"] == 2 and t["expand_launches"] == 1  # count, scan
    finally:
        sp.close()


def test_first_typed_call_builds_the_tile_table():
    sp, edges, dsts = one_row_space(TILE + 1, 2)
    try:
        counts = []
        for _ in range(3):
            sp.find_edges(REL, PI >= 0)
            counts.append(sp.last_timing()["launches"])
        assert counts == [5, 4, 4]
    finally:
        sp.close()


# ---- several sources: ranks, versions, parts, schemas ----------------------------------------------
def props_of(src, j):
    return (src * 1000 + j, j * 0.25 - 3.0, j % 3 == 0, f"s{src}_{j}" if j % 5 else "", j - 50)


RANK_SRC, RANK_DST = 2000, 2001
RANKS = [0, 1, -1, 1 << 40]
VER_SRC, VER_DST = 2100, 2101
FOREIGN_SRC = 2200
SHORT_SRC = 2300


def hand_space(short_own=False, extra=None):
    """sources of degree 1..300 (some with in-edges, some without), one pair under four ranks, three
    versions of one edge, an overwritten edge, and a row whose keys sit in a foreign part and whose value
    lacks field j.  short_own: such a short value on an own-part edge of SHORT_SRC too."""
    w = Writer(PARTS)
    j = 0
    for src, deg in ((1000, 1), (1001, 15), (1002, 300), (1003, 64), (1004, 17)):
        for _ in range(deg):
            j += 1
            w.edge(src, mix(j), 0, 9, props_of(src, j))
    w.edge(1003, 1000, 0, 9, props_of(1003, 999))  # 1000 has an in-edge, the others none
    w.edge(1002, 1001, 0, 9, props_of(1002, 998))
    for r in RANKS:
        w.edge(RANK_SRC, RANK_DST, r, 9, (r, float(r % 1000), r < 0, f"rank{r}", r % 7))
    for k in range(20):
        w.edge(RANK_SRC, mix(900 + k), (k % 3) - 1, 9, props_of(RANK_SRC, k))
    for ver in (1, 65536, 256):  # little-endian: 65536 -> 00 00 01 is first
        w.edge(VER_SRC, VER_DST, 0, ver, (ver, 0.5, True, f"v{ver}", ver))
    w.edge(VER_SRC, VER_DST + 1, 0, 4, (4, 1.5, False, "overwritten", 4))
    w.edge(VER_SRC, VER_DST + 1, 0, 4, (5, 2.5, True, "last write", 5))
    short = O.encode_row([77, 1.0, True, "short"])  # an older schema: no field j
    w.edge(FOREIGN_SRC, 1001, 0, 9, (77, 1.0, True, "short", None), part=O.part_of(FOREIGN_SRC, PARTS) % PARTS + 1,
           encoded=short)
    if short_own:
        w.edge(SHORT_SRC, 1001, 0, 9, (77, 1.0, True, "short", None), encoded=short)
    if extra:
        extra(w)
    sp = GraphSpace(PARTS)
    sp.set_edge_schema(REL, FIELDS, name="rel")
    w.load(sp)
    sp.finalize()
    return sp, w


@pytest.fixture(scope="module")
def hand():
    sp, w = hand_space()
    yield sp, w.edges()
    sp.close()


def test_hand_typed_compares(hand):
    sp, edges = hand
    assert edges[(VER_SRC, 0, VER_DST)][3] == "v65536" and edges[(VER_SRC, 0, VER_DST + 1)][3] == "last write"
    assert not any(k[0] == FOREIGN_SRC for k in edges)
    for where, f in ((PI > 1002100, lambda p: p[0] > 1002100), (PI <= 5, lambda p: p[0] <= 5),
                     (PJ.eq(3), lambda p: p[4] == 3), (PJ.ne(-49), lambda p: p[4] != -49),
                     (PI >= -(1 << 62), lambda p: True), (PI < -5, lambda p: p[0] < -5)):
        types, rows = find_all_modes(sp, where, [PI, PJ])
        check_rows(rows, restate(edges, lambda k, p: f(p), lambda k, p: (p[0], p[4])))
    # the foreign-part row lacks j and passes every compare on i: invisible, and no evaluation error
    types, rows = find_all_modes(sp, PJ >= -1000)
    assert len(rows) == len(edges) and FOREIGN_SRC not in {r[0] for r in rows}
    assert sp.go([FOREIGN_SRC], 1, REL).n_rows == 0  # the GO visibility rule


def test_hand_ranks_and_versions(hand):
    sp, edges = hand
    types, rows = find_all_modes(sp, PI.eq(1 << 40), [PS])
    assert rows == [(RANK_SRC, RANK_DST, 1 << 40, b"rank%d" % (1 << 40))]
    types, rows = find_all_modes(sp, KRANK.ne(0), [PI])
    want = restate(edges, lambda k, p: k[1] != 0, lambda k, p: (p[0],))
    check_rows(rows, want)
    assert {r[2] for r in rows} == {1, -1, 1 << 40} and list(want) == [RANK_SRC]
    types, rows = find_all_modes(sp, PI <= 65536, [PI, PS])
    assert (VER_SRC, VER_DST, 0, 65536, b"v65536") in rows and (VER_SRC, VER_DST + 1, 0, 5, b"last write") in rows
    assert not [r for r in rows if r[0] == VER_SRC and r[3] in (1, 256, 4)]


def test_hand_general_predicates(hand):
    sp, edges = hand
    cases = [(PD < -1.0, lambda k, p: p[1] < -1.0),
             (PS.eq("s1002_17"), lambda k, p: p[3] == "s1002_17"),
             (PS.eq(""), lambda k, p: p[3] == ""),
             (KDST.eq(RANK_DST), lambda k, p: k[2] == RANK_DST),
             (KRANK.eq(-1), lambda k, p: k[1] == -1),
             (KSRC.eq(1004), lambda k, p: k[0] == 1004),
             ((PI > 1002000) & (PJ < 0), lambda k, p: p[0] > 1002000 and p[4] < 0),
             (PB, lambda k, p: p[2]),
             (PI % 2, lambda k, p: p[0] % 2 != 0),  # not a bool: as nbg_go's asBool
             (X.Primary(True), lambda k, p: True),  # no prop node
             (X.Primary(0) > 1, lambda k, p: False),
             (None, lambda k, p: True)]
    for where, f in cases:
        types, rows = find_all_modes(sp, where, [PI])
        check_rows(rows, restate(edges, f, lambda k, p: (p[0],)))
    g = sp.go([1002], 1, REL, where=PI % 2, yields=[KSRC, KDST, KRANK, PI])
    assert Counter(got(g)) == Counter(r for r in find_all_modes(sp, PI % 2, [PI])[1] if r[0] == 1002)


@pytest.mark.parametrize("keep", [False, True])
def test_hand_yields(hand, keep):
    sp, edges = hand
    ys = [PI, PD, PB, PS, PJ, PI * 2 + PJ, PD / 2, KDST, KRANK, KSRC, PS.eq(""), X.AliasProp("any", "i"), X.Primary("c")]
    cols = lambda k, p: (p[0], p[1], p[2], p[3], p[4], p[0] * 2 + p[4], p[1] / 2, k[2], k[1], k[0], p[3] == "", p[0], "c")
    types, rows = find_all_modes(sp, PI > 1000290, ys, keep)
    assert types == [_lib.T_VID] * 4 + [_lib.T_DOUBLE, _lib.T_BOOL, _lib.T_STRING, _lib.T_VID, _lib.T_VID, _lib.T_DOUBLE] + \
        [_lib.T_VID] * 3 + [_lib.T_BOOL, _lib.T_VID, _lib.T_STRING]
    check_rows(rows, restate(edges, lambda k, p: p[0] > 1000290, cols))
    assert len(rows) > 300
    # no yields: the key columns alone; no rows: the columns and their types stay
    types, rows = find_all_modes(sp, PI.eq(1002100), (), keep)
    assert types == [_lib.T_VID] * 3 and rows == [r[:3] for r in restate(edges, lambda k, p: p[0] == 1002100)[1002]]
    types, rows = find_all_modes(sp, PI < -5, [PS, PB], keep)
    assert types == [_lib.T_VID] * 3 + [_lib.T_STRING, _lib.T_BOOL] and rows == []


def test_hand_pipes(hand):
    sp, edges = hand
    set_mode(sp, None)
    dev = sp.find_edges(REL, (PI > 1002000) & KRANK.eq(0), [PI, PS], keep_on_device=True)
    assert dev.on_device and dev.n_rows > 200
    table = sp.order_by(dev, [])
    f = sp.fetch_edges(REL, (dev, 0), (dev, 1), None, [PI, PS])
    assert got(f) == [r[3:] for r in got(table)]
    asc = sp.order_by(dev, [(3, 0)])
    assert list(asc.columns[3]) == sorted(table.columns[3]) and asc.n_rows == dev.n_rows
    both = sp.set_op(_lib.SET_INTERSECT, dev, table)
    assert Counter(got(both)) == Counter(got(table))
    ex = FindExecutor(sp, "rel", ["i", "s"], (PI > 1002000) & KRANK.eq(0))
    assert got(ex.execute()) == got(table)
    with pytest.raises(ValueError):
        FindExecutor(sp, "nope", ["i"])


def test_older_schema_rows():
    sp, w = hand_space(short_own=True)
    try:
        edges = w.edges()
        for m in MODES:
            set_mode(sp, m)
            assert code_of(lambda: sp.find_edges(REL, PJ > 0)) == E_EVAL  # typed compare on the missing field
            assert code_of(lambda: sp.find_edges(REL, (PJ > 0) | (PI > 0))) == E_EVAL
            assert code_of(lambda: sp.find_edges(REL, PI.eq(77), [PJ])) == E_EVAL  # YIELD on the selected row
            assert sp.find_edges(REL, PI.eq(5), [PJ]).rows() == [(VER_SRC, VER_DST + 1, 0, 5)]  # the row is not selected
        # lacking only a field nobody reads
        types, rows = find_all_modes(sp, PI.eq(77), [PS])
        assert rows == [(SHORT_SRC, 1001, 0, b"short")]
        types, rows = find_all_modes(sp, PD >= 1.0, [PI])
        check_rows(rows, restate(edges, lambda k, p: p[1] >= 1.0, lambda k, p: (p[0],)))
    finally:
        sp.close()


def test_commit_is_seen():
    sp = GraphSpace(PARTS)
    try:
        sp.set_option("writable", 1)
        sp.set_edge_schema(REL, FIELDS, name="rel")
        w = Writer(PARTS)
        for j in range(1, 40):
            w.edge(10 + j % 3, mix(j), 0, 9, props_of(10, j))
        w.load(sp)
        sp.finalize()
        before = find_all_modes(sp, PI > 10020, [PI])[1]
        check_rows(before, restate(w.edges(), lambda k, p: p[0] > 10020, lambda k, p: (p[0],)))
        batch = Writer(PARTS)
        batch.seq = w.seq
        batch.edge(11, 424242, 0, 9, (10999, 0.0, True, "new", 0))
        k = sorted(k for k in w.edges() if w.edges()[k][0] > 10020)[0]
        batch.edge(k[0], k[2], k[1], 9, (1, 0.0, True, "overwrites", 0))  # the same key: the last write wins
        batch.load(sp, write=True)
        assert find_all_modes(sp, PI > 10020, [PI])[1] == before  # queries read the last commit
        sp.commit()
        for key, ws in batch.groups.items():
            w.groups.setdefault(key, []).extend(ws)
        after = find_all_modes(sp, PI > 10020, [PI])[1]
        check_rows(after, restate(w.edges(), lambda k, p: p[0] > 10020, lambda k, p: (p[0],)))
        assert (11, 424242, 0, 10999) in after and len(after) == len(before)
        assert not [r for r in after if r[:3] == (k[0], k[2], k[1])]
    finally:
        sp.close()


def raw_find(sp, fn, type_id, where=b"", yields=(), keep=0, null_where=False, null_yields=False, where_len=None):
    ys = [y.encode() for y in yields]
    bufs = [C.create_string_buffer(y, len(y) + 1) for y in ys]
    yp = (C.c_void_p * max(len(ys), 1))(*[C.cast(b, C.c_void_p) for b in bufs])
    yl = (C.c_size_t * max(len(ys), 1))(*[len(y) for y in ys])
    wb = C.create_string_buffer(where, len(where) + 1)
    out = _lib.Rows()
    rc = fn(sp.h, type_id, None if null_where else C.cast(wb, C.c_void_p), len(where) if where_len is None else where_len,
            None if null_yields else yp, None if null_yields else yl, len(ys), keep, C.byref(out))
    if rc == 0:
        sp.L.nbg_rows_free(C.byref(out))
    return rc


def test_errors(hand):
    sp, edges = hand
    set_mode(sp, None)
    fresh = GraphSpace(PARTS)
    try:
        fresh.set_edge_schema(REL, FIELDS)
        assert code_of(lambda: fresh.find_edges(REL, PI > 0)) == E_STATE
    finally:
        fresh.close()
    assert code_of(lambda: sp.find_edges(99, PI > 0)) == E_INVALID_ARG  # a type not in the snapshot
    assert code_of(lambda: sp.find_edges(-REL, PI > 0)) == E_UNSUPPORTED  # in-edges carry no props
    fn = sp.L.nbg_find_edges
    for keep in (2, -1):
        assert raw_find(sp, fn, REL, keep=keep) == E_INVALID_ARG
    assert raw_find(sp, fn, REL, (PI > 0).encode(), null_where=True) == E_INVALID_ARG
    assert raw_find(sp, fn, REL, yields=[PI], null_yields=True) == E_INVALID_ARG
    assert raw_find(sp, fn, REL, null_where=True, null_yields=True) == 0  # lengths 0: nothing is read
    assert raw_find(sp, fn, REL, b"\xff\xff") == E_INVALID_ARG  # undecodable
    for node in (X.SourceProp("t", "i"), X.DestProp("t", "i"), X.InputProp("i"), X.VariableProp("v", "i"),
                 X.EdgeDst("rel"), X.EdgeSrc("rel"), X.EdgeRank("rel"), X.EdgeType("rel")):
        assert code_of(lambda: sp.find_edges(REL, PI > 0, [node])) == E_INVALID_ARG
        assert "alias.prop" in sp.L.nbg_last_error(sp.h).decode()
        assert code_of(lambda: sp.find_edges(REL, node.eq(1))) == E_INVALID_ARG
        assert "alias.prop" in sp.L.nbg_last_error(sp.h).decode()
    for bad, code in ((X.AliasProp("rel", "nope"), E_IMPROPER_DATA_TYPE), (X.AliasProp("rel", "_type"), E_UNSUPPORTED)):
        assert code_of(lambda: sp.find_edges(REL, bad.eq(1))) == code
        assert code_of(lambda: sp.find_edges(REL, None, [bad])) == code
    assert sp.find_edges(REL, PI.eq(5), [PI] * 13).types == [_lib.T_VID] * 16
    assert code_of(lambda: sp.find_edges(REL, PI.eq(5), [PI] * 14)) == E_UNSUPPORTED
    sp.set_option("find_fast", 2)
    try:
        assert code_of(lambda: sp.find_edges(REL, PI.eq(5))) == E_INVALID_ARG
    finally:
        sp.unset_option("find_fast")


# ---- RMAT-12 ---------------------------------------------------------------------------------------
FOLLOW = 1
WEIGHT = X.AliasProp("follow", "weight")


@pytest.fixture(scope="module")
def rmat12():
    sp = GraphSpace(64)
    sp.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    sp.gen_rmat(12, 16, 1, FOLLOW)
    sp.finalize()
    st = O.Store(64)
    st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    st.load_rmat(12, 16, 1, FOLLOW)
    s, _, _ = O.rmat_edges(12, 16, 1)
    yield sp, st, np.unique(s)
    sp.close()


@pytest.mark.parametrize("op", ["<", "<=", ">", ">=", "==", "!="])
def test_rmat_weight(rmat12, op):
    """expected rows: nbg_go 1 STEPS from every source with the same WHERE (k_expand); counts: the C++ oracle"""
    sp, st, srcs = rmat12
    where = {"<": WEIGHT < 499, "<=": WEIGHT <= 499, ">": WEIGHT > 499, ">=": WEIGHT >= 499, "==": WEIGHT.eq(499),
             "!=": WEIGHT.ne(499)}[op]
    ys = [X.AliasProp("follow", f) for f in ("_src", "_dst", "_rank", "weight")]
    want = sp.go(srcs, 1, FOLLOW, where=where, yields=ys)
    r = st.go(srcs, 1, FOLLOW, where=where.encode(), yields=[WEIGHT.encode()])
    assert r.code == 0
    types, rows = find_all_modes(sp, where, [WEIGHT], et=FOLLOW)
    assert len(rows) == want.n_rows == r.nrows > 0
    assert Counter(rows) == Counter(got(want))
    assert sp.find_edges(FOLLOW, where).edges_scanned == sp.info(FOLLOW)["local_out_edges"]
