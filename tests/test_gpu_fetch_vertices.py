"""FETCH PROP ON a tag (nbg_fetch_vertices; FetchVerticesExecutor over QueryVertexPropsProcessor).

The C++ oracle has no FETCH, so the expectation is restated here: the test builds every KV pair
itself and therefore knows every row, part and version.  Expected rows are
[row(v) for v in keys if v has a row of the tag in its own part], the bytewise-first version of
that row (identical keys: the last write), with key-dedup then row-dedup under DISTINCT.  Every
column is compared exactly and in order (doubles by bit pattern, strings as bytes).
"""
import ctypes as C
import struct

import numpy as np
import pytest

import fixtures as F
import oracle as O
from nebula_amd import (AddVerticesProcessor, AddVerticesRequest, FetchVerticesExecutor, GraphSpace, NbgError, Tag,
                        Vertex, _lib)
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

NAME, AGE = X.AliasProp("player", "name"), X.AliasProp("player", "age")
E_STATE, E_INVALID_ARG, E_UNSUPPORTED, E_EVAL = -1002, -1001, -1003, -1004
E_TAG_PROP_NOT_FOUND, E_IMPROPER_DATA_TYPE = -22, -23
EMPTY_VID, NUL_VID, LONELY_VID, UNKNOWN_VID = 900001, 900002, 900003, 987654321


def bits(v):
    """a cell in its exact form: doubles by bit pattern, strings as bytes"""
    if isinstance(v, float):
        return ("f64", struct.pack("<d", v))
    if isinstance(v, str):
        return v.encode()
    return v


def got(rs):
    return [tuple(bits(c) for c in r) for r in rs.rows()]


def dedup(seq):
    seen, out = set(), []
    for x in seq:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def expect(rows, keys, cols, distinct=False):
    """rows: {vid: tuple of cells}; cols: a function row -> output tuple"""
    keys = dedup(keys) if distinct else list(keys)
    out = [tuple(bits(c) for c in cols(rows[v])) for v in keys if v in rows]
    return dedup(out) if distinct else out


def row_with_nul(name_with_nul, age):
    """encode_row takes C strings: encode a stand-in of the same length, then put the NUL back"""
    stand_in = name_with_nul.replace("\0", "#")
    return O.encode_row([stand_in, age]).replace(stand_in.encode(), name_with_nul.encode())


def nba_space(writable=False):
    sp = GraphSpace(1)
    for et, (name, fields) in F.NBA_EDGE_SCHEMAS.items():
        sp.set_edge_schema(et, fields, name=name)
    sp.set_tag_schema(F.NBA_PLAYER, "player", [("name", O.STRING), ("age", O.INT)])
    sp.set_tag_schema(F.NBA_TEAM, "team", [("name", O.STRING)])
    if writable:
        sp.set_option("writable", 1)
    parts, vid = F.nba_kv()
    kv = list(parts[1])
    # vertices no edge names: an empty name, an embedded NUL, a plain one
    kv.append((O.vertex_key(1, EMPTY_VID, F.NBA_PLAYER, 0), O.encode_row(["", 20])))
    kv.append((O.vertex_key(1, NUL_VID, F.NBA_PLAYER, 0), row_with_nul("a\0b", 21)))
    kv.append((O.vertex_key(1, LONELY_VID, F.NBA_PLAYER, 0), O.encode_row(["Lonely", 30])))
    sp.load_part(1, kv)
    sp.finalize()
    d = F.nba()
    rows = {p["vid"]: (p["name"], p["age"]) for p in d["players"]}
    rows.update({EMPTY_VID: ("", 20), NUL_VID: ("a\0b", 21), LONELY_VID: ("Lonely", 30)})
    return sp, vid, rows, d


@pytest.fixture(scope="module")
def nba():
    sp, vid, rows, d = nba_space()
    yield sp, vid, rows, d
    sp.close()


def test_nba_name_and_age(nba):
    sp, vid, rows, d = nba
    keys = [vid[n] for n in ("Tim Duncan", "Tony Parker", "Manu Ginobili", "Boris Diaw")]
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [NAME, AGE])
    assert rs.types == [_lib.T_STRING, _lib.T_VID]
    assert got(rs) == expect(rows, keys, lambda r: r)
    golden = {p["name"]: p["age"] for p in d["players"]}
    assert rs.rows() == [(n, golden[n]) for n in ("Tim Duncan", "Tony Parker", "Manu Ginobili", "Boris Diaw")]
    t = sp.last_timing()
    assert t["hops"] == [] and t["edges_scanned"] == 0 and t["launches"] > 0
    assert t["host_waits"] == 3  # match count, error count + STRING totals, hand-out


def test_nba_team_and_unknown_give_no_row(nba):
    sp, vid, rows, d = nba
    keys = [vid["Spurs"], vid["Tim Duncan"], UNKNOWN_VID, d["nonexist_hash"], vid["Tony Parker"]]
    assert vid["Spurs"] not in rows
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [NAME, AGE])
    assert got(rs) == expect(rows, keys, lambda r: r)
    assert rs.n_rows == 2
    # the team's row is there under its own tag
    assert sp.fetch_vertices(F.NBA_TEAM, [vid["Spurs"]], [X.AliasProp("team", "name")]).rows() == [("Spurs",)]


@pytest.mark.parametrize("distinct", [False, True])
def test_nba_duplicate_vids(nba, distinct):
    sp, vid, rows, d = nba
    a, b, c = vid["Tim Duncan"], vid["Tony Parker"], vid["Manu Ginobili"]
    keys = [b, a, b, UNKNOWN_VID, c, a, a, UNKNOWN_VID, b]
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [AGE, NAME], distinct=distinct)
    assert got(rs) == expect(rows, keys, lambda r: (r[1], r[0]), distinct)
    assert rs.n_rows == (3 if distinct else 7)


def test_nba_equal_rows_collapse_under_distinct(nba):
    sp, vid, rows, d = nba
    keys = [p["vid"] for p in d["players"]][:12]
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [AGE > 0])
    assert rs.types == [_lib.T_BOOL] and got(rs) == [(True,)] * 12
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [AGE > 0], distinct=True)
    assert got(rs) == [(True,)]
    # two columns, one of them distinguishing: nothing collapses
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [AGE > 0, NAME], distinct=True)
    assert got(rs) == expect(rows, keys, lambda r: (r[1] > 0, r[0]), True) and rs.n_rows == 12


def test_nba_no_yield_gives_every_field(nba):
    sp, vid, rows, d = nba
    keys = [vid["Tracy McGrady"], LONELY_VID, vid["Spurs"]]
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys)
    assert rs.types == [_lib.T_STRING, _lib.T_VID]
    assert got(rs) == expect(rows, keys, lambda r: r)
    assert sp.fetch_vertices(F.NBA_TEAM, keys).rows() == [("Spurs",)]


def test_nba_arithmetic_yield(nba):
    sp, vid, rows, d = nba
    keys = [p["vid"] for p in d["players"]]
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [AGE + 1, AGE * 0.5, NAME.eq("Tim Duncan") | (AGE < 25)])
    assert rs.types == [_lib.T_VID, _lib.T_DOUBLE, _lib.T_BOOL]
    assert got(rs) == expect(rows, keys, lambda r: (r[1] + 1, r[1] * 0.5, r[0] == "Tim Duncan" or r[1] < 25))


@pytest.mark.parametrize("keep", [False, True])
def test_nba_empty_and_nul_strings(nba, keep):
    sp, vid, rows, d = nba
    keys = [NUL_VID, vid["Tim Duncan"], EMPTY_VID, LONELY_VID, EMPTY_VID]
    rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [NAME, AGE], keep_on_device=keep)
    assert rs.on_device == keep
    if keep:
        rs = sp.order_by(rs, [])  # the device table back on the host, unchanged
    assert got(rs) == expect(rows, keys, lambda r: r)
    assert got(rs)[0] == (b"a\0b", 21) and got(rs)[2] == (b"", 20)


@pytest.mark.parametrize("keep", [False, True])
def test_nba_no_keys_and_no_matches(nba, keep):
    sp, vid, rows, d = nba
    for keys in ([], [UNKNOWN_VID, vid["Spurs"]]):
        for distinct in (False, True):
            rs = sp.fetch_vertices(F.NBA_PLAYER, keys, [NAME, AGE, AGE > 3], distinct=distinct, keep_on_device=keep)
            assert rs.n_rows == 0 and rs.types == [_lib.T_STRING, _lib.T_VID, _lib.T_BOOL]
            assert rs.on_device == keep
    assert sp.fetch_vertices(F.NBA_PLAYER, []).types == [_lib.T_STRING, _lib.T_VID]


def test_vertex_without_edges_at_load(nba):
    sp, vid, rows, d = nba
    n_before = sp.info(F.NBA_LIKE)["num_vertices"]
    assert sp.out_degree(F.NBA_LIKE, LONELY_VID) <= 0
    assert sp.go([LONELY_VID], 1, F.NBA_LIKE).n_rows == 0  # still no vertex of the graph
    assert sp.fetch_vertices(F.NBA_PLAYER, [LONELY_VID], [NAME, AGE]).rows() == [("Lonely", 30)]
    assert sp.fetch_vertices(F.NBA_TEAM, [LONELY_VID]).n_rows == 0  # a tail index of another tag is no row
    # the tail adds no vertex to the graph: the count is that of the edges' endpoints
    ends = {vid[x] for e in d["serve"] + d["like"] for x in e[:2]}
    assert sp.info(F.NBA_LIKE)["num_vertices"] == n_before == len(ends)


def test_vertex_without_edges_after_commit():
    sp, vid, rows, d = nba_space(writable=True)
    try:
        new_vid, tim = 900100, vid["Tim Duncan"]
        ys = [X.EdgeDst("like"), X.AliasProp("like", "likeness"), X.DestProp("player", "name")]
        cols = [("_dst", O.EDGE, 0), ("likeness", O.EDGE, 0), ("name", O.SOURCE, F.NBA_PLAYER)]

        def snapshot():
            g = sp.go([tim, vid["Tony Parker"]], 2, F.NBA_LIKE, yields=ys)
            b = sp.get_bound(F.NBA_LIKE, [1, 1], [tim, vid["Manu Ginobili"]], cols)
            return sorted(g.rows()), b.rows(), list(b.vertex_ids), b.vertex_columns, sp.info(F.NBA_LIKE)["num_vertices"]

        before = snapshot()
        assert sp.fetch_vertices(F.NBA_PLAYER, [new_vid, LONELY_VID], [NAME]).rows() == [("Lonely",)]
        req = AddVerticesRequest({1: [Vertex(new_vid, [Tag(F.NBA_PLAYER, O.encode_row(["Rookie", 19]))])]})
        assert AddVerticesProcessor.instance(sp, version=0x0200).process(req).failed_codes == []
        rs = sp.fetch_vertices(F.NBA_PLAYER, [new_vid, tim, LONELY_VID], [NAME, AGE])
        assert rs.rows() == [("Rookie", 19), ("Tim Duncan", rows[tim][1]), ("Lonely", 30)]
        assert snapshot() == before
        # a second version of the row whose key bytes come first (00 01 .. before 00 02 ..) wins
        req = AddVerticesRequest({1: [Vertex(new_vid, [Tag(F.NBA_PLAYER, O.encode_row(["Sophomore", 20]))])]})
        AddVerticesProcessor.instance(sp, version=0x0100).process(req)
        assert sp.fetch_vertices(F.NBA_PLAYER, [new_vid]).rows() == [("Sophomore", 20)]
        assert snapshot() == before
    finally:
        sp.close()


# ---- part and version rules -----------------------------------------------------------------------
PARTS = 4
PERSON = 5
ET = 1
PFIELDS = [("name", O.STRING), ("age", O.INT), ("wt", O.DOUBLE)]
PNAME, PAGE, PWT = (X.AliasProp("person", f) for f in ("name", "age", "wt"))


def ver_bytes(ver):
    return struct.pack("<q", ver)


def rules_space():
    """vids 1..3 have edges, 10..13 have none.  Returns the space and the restated rows."""
    parts = {p: [] for p in range(1, PARTS + 1)}
    written = {}  # vid -> [(version bytes, write sequence, row)] of own-part rows

    def own(v):
        return O.part_of(v, PARTS)

    def put(part, v, ver, row, encoded=None):
        parts[part].append((O.vertex_key(part, v, PERSON, ver), encoded if encoded is not None else O.encode_row(list(row))))
        if part == own(v):
            written.setdefault(v, []).append((ver_bytes(ver), len(parts[part]), row))

    for s, t in ((1, 2), (2, 3), (3, 1)):
        parts[own(s)].append((O.edge_key(own(s), s, ET, 0, t, 7), O.encode_row([s * 10 + t])))
        parts[own(t)].append((O.edge_key(own(t), t, -ET, 0, s, 7), b""))
    for base in (0, 9):  # the same cases on vertices with edges (1..3) and without (10..12)
        put(own(base + 1), base + 1, 5, ("plain", 1, 0.5))
        # versions 1 and 256: little-endian bytes 01 00 .. and 00 01 ..: 256 is first bytewise
        put(own(base + 2), base + 2, 1, ("numerically first", -1, -1.0))
        put(own(base + 2), base + 2, 256, ("bytewise first, overwritten", -2, -2.0))
        put(own(base + 2), base + 2, 256, ("bytewise first", 2, -0.0))
        foreign = own(base + 3) % PARTS + 1
        put(foreign, base + 3, 0, ("foreign part only", 3, 3.0))
    put(own(13), 13, 0, ("short",), encoded=O.encode_row(["short"]))  # an older schema: name only
    sp = GraphSpace(PARTS)
    sp.set_edge_schema(ET, [("w", O.INT)], name="e")
    sp.set_tag_schema(PERSON, "person", PFIELDS)
    for p, kv in parts.items():
        if kv:
            sp.load_part(p, kv)
    sp.finalize()
    rows = {}
    for v, ws in written.items():
        first = min(w[0] for w in ws)
        rows[v] = max((w for w in ws if w[0] == first), key=lambda w: w[1])[2]
    return sp, rows


@pytest.fixture(scope="module")
def rules():
    sp, rows = rules_space()
    yield sp, rows
    sp.close()


def test_rules_part_and_version(rules):
    sp, rows = rules
    assert sorted(rows) == [1, 2, 10, 11, 13] and rows[2][0] == rows[11][0] == "bytewise first"
    keys = [12, 11, 3, 2, 10, 1, 99, 11]
    rs = sp.fetch_vertices(PERSON, keys, [PNAME, PAGE, PWT])
    assert got(rs) == expect(rows, keys, lambda r: r)
    assert rs.n_rows == 5
    assert got(rs)[0][2] == ("f64", struct.pack("<d", -0.0))  # the double's bits, not its value
    rs = sp.fetch_vertices(PERSON, keys, [PNAME, PAGE, PWT], distinct=True)
    assert got(rs) == expect(rows, keys, lambda r: r, True) and rs.n_rows == 2  # 11 == 2 and 10 == 1 by value


def test_rules_row_lacking_a_field(rules):
    sp, rows = rules
    assert sp.fetch_vertices(PERSON, [13, 10], [PNAME]).rows() == [("short",), ("plain",)]
    with pytest.raises(NbgError) as e:
        sp.fetch_vertices(PERSON, [10, 13], [PNAME, PAGE])
    assert e.value.code == E_EVAL
    with pytest.raises(NbgError) as e:
        sp.fetch_vertices(PERSON, [13])  # every field
    assert e.value.code == E_EVAL
    assert sp.fetch_vertices(PERSON, [10, 12], [PNAME, PAGE]).n_rows == 1  # no such row emitted: no error


def raw_fetch(sp, tag, n, on_dev, distinct, keep, yields=(NAME,), vids=None):
    ys = [y.encode() for y in yields]
    bufs = [C.create_string_buffer(y, len(y) + 1) for y in ys]
    yp = (C.c_void_p * max(len(ys), 1))(*[C.cast(b, C.c_void_p) for b in bufs])
    yl = (C.c_size_t * max(len(ys), 1))(*[len(y) for y in ys])
    a = np.zeros(8, dtype=np.int64)
    out = _lib.Rows()
    rc = sp.L.nbg_fetch_vertices(sp.h, tag, vids if vids is not None else a.ctypes.data, n, on_dev, yp, yl, len(ys),
                                 distinct, keep, C.byref(out))
    if rc == 0:
        sp.L.nbg_rows_free(C.byref(out))
    return rc


def code_of(fn):
    with pytest.raises(NbgError) as e:
        fn()
    return e.value.code


def test_error_before_finalize():
    sp = GraphSpace(1)
    try:
        sp.set_tag_schema(F.NBA_PLAYER, "player", [("name", O.STRING), ("age", O.INT)])
        assert code_of(lambda: sp.fetch_vertices(F.NBA_PLAYER, [1], [NAME])) == E_STATE
    finally:
        sp.close()


def test_error_unknown_tag(nba):
    sp = nba[0]
    assert code_of(lambda: sp.fetch_vertices(999, [1], [NAME])) == E_TAG_PROP_NOT_FOUND


@pytest.mark.parametrize("flags", [(2, 0, 0), (0, 2, 0), (0, 0, 2), (-1, 0, 0), (0, -1, 0), (0, 0, -1)])
def test_error_flags(nba, flags):
    assert raw_fetch(nba[0], F.NBA_PLAYER, 1, *flags) == E_INVALID_ARG


def test_error_null_pointers(nba):
    sp = nba[0]
    assert raw_fetch(sp, F.NBA_PLAYER, 1, 0, 0, 0, vids=0) == E_INVALID_ARG
    out = _lib.Rows()
    assert sp.L.nbg_fetch_vertices(sp.h, F.NBA_PLAYER, None, 0, 0, None, None, 1, 0, 0, C.byref(out)) == E_INVALID_ARG
    assert sp.L.nbg_fetch_vertices(sp.h, F.NBA_PLAYER, None, 0, 0, None, None, 0, 0, 0, None) == E_INVALID_ARG
    assert raw_fetch(sp, F.NBA_PLAYER, 0, 0, 0, 0, vids=0) == 0  # n = 0 needs no key pointer


def test_error_alias_of_another_tag(nba):
    sp = nba[0]
    assert code_of(lambda: sp.fetch_vertices(F.NBA_PLAYER, [1], [X.AliasProp("team", "name")])) == E_INVALID_ARG


@pytest.mark.parametrize("node", [X.SourceProp("player", "name"), X.DestProp("player", "name"), X.InputProp("name"),
                                  X.VariableProp("v", "name"), X.EdgeDst("player"), X.EdgeSrc("player"),
                                  X.EdgeRank("player"), X.EdgeType("player")])
def test_error_not_alias_prop(nba, node):
    sp = nba[0]
    assert code_of(lambda: sp.fetch_vertices(F.NBA_PLAYER, [1], [AGE, node])) == E_INVALID_ARG
    assert "alias.prop" in sp.L.nbg_last_error(sp.h).decode()


def test_error_no_props(nba):
    sp = nba[0]
    assert code_of(lambda: sp.fetch_vertices(F.NBA_PLAYER, [1], [X.Primary(1) + 2, X.Primary("x")])) == E_INVALID_ARG
    assert "No props declared" in sp.L.nbg_last_error(sp.h).decode()


def test_error_unknown_prop(nba):
    sp = nba[0]
    assert code_of(lambda: sp.fetch_vertices(F.NBA_PLAYER, [1], [X.AliasProp("player", "height")])) == E_IMPROPER_DATA_TYPE


def test_error_unsupported(nba):
    sp = nba[0]
    assert sp.fetch_vertices(F.NBA_PLAYER, [1], [AGE] * 16).types == [_lib.T_VID] * 16
    assert code_of(lambda: sp.fetch_vertices(F.NBA_PLAYER, [1], [AGE] * 17)) == E_UNSUPPORTED
    assert raw_fetch(sp, F.NBA_PLAYER, 1 << 32, 0, 0, 0) == E_UNSUPPORTED  # refused before a key is read


# ---- device-resident keys and results ------------------------------------------------------------
def test_keys_from_a_device_go_result(nba):
    sp, vid, rows, d = nba
    starts = [vid[n] for n in ("Tim Duncan", "Tony Parker", "Manu Ginobili", "LaMarcus Aldridge")]
    # (order_by=[]: the GO's table stays in HBM and keeps owning its columns)
    dev = sp.go(starts, 2, F.NBA_LIKE, yields=[X.EdgeDst("like")], keep_on_device=True, order_by=[])
    assert dev.on_device and dev.n_rows > 4
    host_keys = sp.order_by(dev, []).columns[0]
    assert len(set(host_keys.tolist())) < len(host_keys)  # duplicates among the dsts
    for distinct in (False, True):
        a = sp.fetch_vertices(F.NBA_PLAYER, (dev, 0), [NAME, AGE], distinct=distinct)
        b = sp.fetch_vertices(F.NBA_PLAYER, host_keys, [NAME, AGE], distinct=distinct)
        assert got(a) == got(b) == expect(rows, host_keys.tolist(), lambda r: r, distinct)
    assert np.array_equal(sp.order_by(dev, []).columns[0], host_keys)  # the keys were read, not consumed
    # the output kept in HBM and ordered there equals the host sort
    out = sp.fetch_vertices(F.NBA_PLAYER, (dev, 0), [NAME, AGE], keep_on_device=True)
    assert out.on_device and out.columns == [None, None]
    ordered = sp.order_by(out, [(1, 1), (0, 0)])
    want = sorted(expect(rows, host_keys.tolist(), lambda r: r), key=lambda r: (-r[1], r[0]))
    assert got(ordered) == want
    # the operator shape: a piped sentence names its input column
    ex = FetchVerticesExecutor(sp, "player", [NAME, AGE], distinct=True, ref_col=0)
    assert got(ex.execute(dev)) == expect(rows, host_keys.tolist(), lambda r: r, True)
    assert got(FetchVerticesExecutor(sp, "player", [NAME]).execute(starts[:2])) == [(b"Tim Duncan",), (b"Tony Parker",)]
    with pytest.raises(ValueError):
        FetchVerticesExecutor(sp, "coach")
