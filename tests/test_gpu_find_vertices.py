"""FIND props FROM a tag WHERE (nbg_find_vertices): the scan of the tag's per-vertex columns.

Expectations are restated from the rows the test writes (the own-part row, the bytewise-first
version, the last write of identical keys) and from the NBA fixture's rows.  The rows come in column
index order: the vertices with edges in the engine's numbering (compared as a multiset), then the
vertices no edge names in ascending vid order (compared as a list); a repeated call returns the same
list.  Doubles are compared by bits, strings as bytes.
"""
import ctypes as C
import struct
from collections import Counter

import numpy as np
import pytest

import fixtures as F
import oracle as O
from nebula_amd import FindExecutor, GoExecutor, GraphSpace, NbgError, _lib
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

E_STATE, E_INVALID_ARG, E_UNSUPPORTED, E_IMPROPER_DATA_TYPE, E_EVAL, E_TAG = -1002, -1001, -1003, -23, -1004, -22
NAME, AGE = X.AliasProp("player", "name"), X.AliasProp("player", "age")
LONELY_VID, EMPTY_VID = 900001, 900002


def bits(v):
    if isinstance(v, float):
        return ("f64", struct.pack("<d", v))
    if isinstance(v, str):
        return v.encode()
    return v


def got(rs):
    return [tuple(bits(c) for c in r) for r in rs.rows()]


def code_of(fn):
    with pytest.raises(NbgError) as e:
        fn()
    return e.value.code


def find(sp, tag, where, yields=(), keep=False):
    """the call twice (and under find_fast 0: the option does not touch vertices); the same list each time"""
    res = []
    for m in (None, 0, None):
        if m is None:
            sp.unset_option("find_fast")
        else:
            sp.set_option("find_fast", m)
        rs = sp.find_vertices(tag, where, yields, keep_on_device=keep)
        assert rs.on_device == keep
        if keep:
            rs = sp.order_by(rs, [])
        res.append((rs.types, got(rs)))
    sp.unset_option("find_fast")
    assert res[0] == res[1] == res[2]
    return res[0]


def check(rows, want, tail):
    """want: {vid: row}; tail: the vids no edge names"""
    assert Counter(rows) == Counter(want.values())
    last = [r[0] for r in rows if r[0] in tail]
    assert [r[0] for r in rows][len(rows) - len(last):] == last == sorted(last)


# ---- the NBA fixture ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nba():
    sp = GraphSpace(1)
    for et, (name, fields) in F.NBA_EDGE_SCHEMAS.items():
        sp.set_edge_schema(et, fields, name=name)
    sp.set_tag_schema(F.NBA_PLAYER, "player", [("name", O.STRING), ("age", O.INT)])
    sp.set_tag_schema(F.NBA_TEAM, "team", [("name", O.STRING)])
    parts, vid = F.nba_kv()
    kv = list(parts[1])
    kv.append((O.vertex_key(1, EMPTY_VID, F.NBA_PLAYER, 0), O.encode_row(["", 20])))
    kv.append((O.vertex_key(1, LONELY_VID, F.NBA_PLAYER, 0), O.encode_row(["Lonely", 30])))
    sp.load_part(1, kv)
    sp.finalize()
    d = F.nba()
    rows = {p["vid"]: (p["name"], p["age"]) for p in d["players"]}
    rows.update({EMPTY_VID: ("", 20), LONELY_VID: ("Lonely", 30)})
    yield sp, vid, rows
    sp.close()


@pytest.mark.parametrize("keep", [False, True])
def test_nba_age(nba, keep):
    sp, vid, rows = nba
    tail = {EMPTY_VID, LONELY_VID}
    for k in (0, 25, 30, 33, 40, 100):
        types, out = find(sp, F.NBA_PLAYER, AGE > k, [NAME, AGE], keep)
        assert types == [_lib.T_VID, _lib.T_STRING, _lib.T_VID]
        check(out, {v: (v, r[0].encode(), r[1]) for v, r in rows.items() if r[1] > k}, tail)
    types, out = find(sp, F.NBA_PLAYER, (AGE >= 30) & NAME.ne("Lonely"), (), keep)
    assert types == [_lib.T_VID]
    check(out, {v: (v,) for v, r in rows.items() if r[1] >= 30 and r[0] != "Lonely"}, tail)
    types, out = find(sp, F.NBA_PLAYER, NAME.eq(""), [AGE], keep)
    assert out == [(EMPTY_VID, 20)]
    types, out = find(sp, F.NBA_PLAYER, None, [NAME], keep)  # no WHERE: every player, no team
    check(out, {v: (v, r[0].encode()) for v, r in rows.items()}, tail)
    assert vid["Spurs"] not in {r[0] for r in out}
    types, out = find(sp, F.NBA_TEAM, None, [X.AliasProp("team", "name")], keep)
    assert (vid["Spurs"], b"Spurs") in out and not {r[0] for r in out} & set(rows)


def test_nba_timing(nba):
    sp, vid, rows = nba
    for where, ys, n, waits, launches in ((AGE > 30, [NAME, AGE], None, 3, 3 + 3), (AGE > 30, [AGE], None, 3, 3 + 1),
                                          (AGE > 30, [], None, 2, 3), (AGE > 1000, [NAME], 0, 2, 2)):
        rs = sp.find_vertices(F.NBA_PLAYER, where, ys)
        t = sp.last_timing()
        assert n is None or rs.n_rows == n
        assert t["hops"] == [] and t["edges_scanned"] == rs.edges_scanned == 0 and t["expand_launches"] == 0
        assert (t["host_waits"], t["launches"]) == (waits, launches)


def test_nba_piped_into_go(nba):
    sp, vid, rows = nba
    rs = FindExecutor(sp, "player", [], AGE > 33).execute()
    starts = rs.columns[0]
    literal = [v for v, r in rows.items() if r[1] > 33]
    assert sorted(starts.tolist()) == sorted(literal) and len(literal) > 3
    ys = [X.EdgeSrc("like"), X.EdgeDst("like"), X.AliasProp("like", "likeness")]
    a = GoExecutor(sp, starts, F.NBA_LIKE, yields=ys).execute()
    b = sp.go(literal, 1, F.NBA_LIKE, yields=ys)
    assert Counter(a.rows()) == Counter(b.rows()) and a.n_rows > 0
    dev = sp.find_vertices(F.NBA_PLAYER, AGE > 33, keep_on_device=True)
    f = sp.fetch_vertices(F.NBA_PLAYER, (dev, 0), [NAME, AGE])
    assert f.rows() == [rows[v] for v in starts.tolist()]
    ex = FindExecutor(sp, "player", ["name", "age"], AGE > 33).execute()
    assert [r[1:] for r in ex.rows()] == f.rows()
    with pytest.raises(ValueError):
        FindExecutor(sp, "nobody", ["name"])


# ---- part and version rules ----------------------------------------------------------------------
PARTS = 4
PERSON, GHOST, HERMIT = 5, 6, 8
ET = 1
PFIELDS = [("name", O.STRING), ("age", O.INT), ("wt", O.DOUBLE)]
PNAME, PAGE, PWT = (X.AliasProp("person", f) for f in ("name", "age", "wt"))


@pytest.fixture(scope="module")
def rules():
    """vids 1..3 have edges, 10..13 have none; tag ghost has no row at all, tag hermit only rows of vertices
    without edges.  Yields the space and the restated own-part rows of person."""
    parts = {p: [] for p in range(1, PARTS + 1)}
    written = {}

    def own(v):
        return O.part_of(v, PARTS)

    def put(part, v, ver, row, encoded=None, tag=PERSON):
        parts[part].append((O.vertex_key(part, v, tag, ver), encoded if encoded is not None else O.encode_row(list(row))))
        if part == own(v) and tag == PERSON:
            written.setdefault(v, []).append((struct.pack("<q", ver), len(parts[part]), row))

    for s, t in ((1, 2), (2, 3), (3, 1)):
        parts[own(s)].append((O.edge_key(own(s), s, ET, 0, t, 7), O.encode_row([s * 10 + t])))
        parts[own(t)].append((O.edge_key(own(t), t, -ET, 0, s, 7), b""))
    for base in (0, 9):  # the same cases on vertices with edges (1..3) and without (10..12)
        put(own(base + 1), base + 1, 5, ("plain", 1 + base, 0.5))
        put(own(base + 2), base + 2, 1, ("numerically first", -1, -1.0))
        put(own(base + 2), base + 2, 256, ("bytewise first, overwritten", -2, -2.0))
        put(own(base + 2), base + 2, 256, ("bytewise first", 2 + base, -0.0))
        put(own(base + 3) % PARTS + 1, base + 3, 0, ("foreign part only", 3, 3.0))
    put(own(13), 13, 0, ("short", None, None), encoded=O.encode_row(["short"]))  # an older schema: name only
    for v in (40, 41, 42):
        put(own(v), v, 0, (v,), tag=HERMIT)
    sp = GraphSpace(PARTS)
    sp.set_edge_schema(ET, [("w", O.INT)], name="e")
    sp.set_tag_schema(PERSON, "person", PFIELDS)
    sp.set_tag_schema(GHOST, "ghost", [("x", O.INT)])
    sp.set_tag_schema(HERMIT, "hermit", [("x", O.INT)])
    for p, kv in parts.items():
        if kv:
            sp.load_part(p, kv)
    sp.finalize()
    rows = {}
    for v, ws in written.items():
        first = min(w[0] for w in ws)
        rows[v] = max((w for w in ws if w[0] == first), key=lambda w: w[1])[2]
    yield sp, rows
    sp.close()


TAIL = {10, 11, 13, 40, 41, 42}


def test_rules_part_and_version(rules):
    sp, rows = rules
    assert sorted(rows) == [1, 2, 10, 11, 13] and rows[2][0] == rows[11][0] == "bytewise first"
    types, out = find(sp, PERSON, None, [PNAME])  # name is present in every row, the short one too
    check(out, {v: (v, r[0].encode()) for v, r in rows.items()}, TAIL)
    assert [r[0] for r in out][2:] == [10, 11, 13]
    full = {v: r for v, r in rows.items() if v != 13}
    types, out = find(sp, PERSON, PNAME.ne("short"), [PNAME, PAGE, PWT])
    check(out, {v: (v,) + tuple(bits(c) for c in r) for v, r in full.items()}, TAIL)
    assert (11, b"bytewise first", 11, ("f64", struct.pack("<d", -0.0))) in out  # the double's bits


def test_rules_row_lacking_a_field(rules):
    sp, rows = rules
    assert code_of(lambda: sp.find_vertices(PERSON, PAGE > 0)) == E_EVAL  # the short row is a candidate
    assert code_of(lambda: sp.find_vertices(PERSON, PNAME.eq("short"), [PAGE])) == E_EVAL  # selected, YIELD fails
    assert code_of(lambda: sp.find_vertices(PERSON, None, [PWT])) == E_EVAL
    assert find(sp, PERSON, PNAME.eq("short"), [PNAME])[1] == [(13, b"short")]
    # the foreign-part rows (vids 3, 12) are no candidates: never evaluated, never selected
    assert 3 not in rows and 12 not in rows
    assert sorted(r[0] for r in find(sp, PERSON, PNAME.ne("short"), [PAGE])[1]) == [1, 2, 10, 11]


def test_no_rows_and_tail_only(rules):
    sp, rows = rules
    for keep in (False, True):
        types, out = find(sp, GHOST, None, [X.AliasProp("ghost", "x")], keep)
        assert out == [] and types == [_lib.T_VID, _lib.T_VID]
        types, out = find(sp, GHOST, X.AliasProp("ghost", "x") > 0, (), keep)
        assert out == [] and types == [_lib.T_VID]
        hx = X.AliasProp("hermit", "x")
        assert find(sp, HERMIT, None, [hx], keep)[1] == [(40, 40), (41, 41), (42, 42)]
        assert find(sp, HERMIT, hx > 40, [hx * 2], keep)[1] == [(41, 82), (42, 84)]
    sp.find_vertices(GHOST, None)
    t = sp.last_timing()
    assert t["host_waits"] == 2 and t["launches"] == 2  # the columns exist: scanned, nothing selected


def raw_find(sp, tag, where=b"", yields=(), keep=0, null_where=False, null_yields=False):
    ys = [y.encode() for y in yields]
    bufs = [C.create_string_buffer(y, len(y) + 1) for y in ys]
    yp = (C.c_void_p * max(len(ys), 1))(*[C.cast(b, C.c_void_p) for b in bufs])
    yl = (C.c_size_t * max(len(ys), 1))(*[len(y) for y in ys])
    wb = C.create_string_buffer(where, len(where) + 1)
    out = _lib.Rows()
    rc = sp.L.nbg_find_vertices(sp.h, tag, None if null_where else C.cast(wb, C.c_void_p), len(where),
                                None if null_yields else yp, None if null_yields else yl, len(ys), keep, C.byref(out))
    if rc == 0:
        sp.L.nbg_rows_free(C.byref(out))
    return rc


def test_errors(rules):
    sp, rows = rules
    fresh = GraphSpace(PARTS)
    try:
        fresh.set_tag_schema(PERSON, "person", PFIELDS)
        assert code_of(lambda: fresh.find_vertices(PERSON, PAGE > 0)) == E_STATE
    finally:
        fresh.close()
    assert code_of(lambda: sp.find_vertices(99, PAGE > 0)) == E_TAG
    for keep in (2, -1):
        assert raw_find(sp, PERSON, keep=keep) == E_INVALID_ARG
    assert raw_find(sp, PERSON, (PAGE > 0).encode(), null_where=True) == E_INVALID_ARG
    assert raw_find(sp, PERSON, yields=[PAGE], null_yields=True) == E_INVALID_ARG
    assert raw_find(sp, PERSON, null_where=True, null_yields=True) == 0
    for node in (X.SourceProp("person", "age"), X.DestProp("person", "age"), X.InputProp("age"),
                 X.VariableProp("v", "age"), X.EdgeDst("e"), X.EdgeSrc("e"), X.EdgeRank("e"), X.EdgeType("e")):
        for call in (lambda: sp.find_vertices(PERSON, node > 0), lambda: sp.find_vertices(PERSON, None, [node])):
            assert code_of(call) == E_INVALID_ARG
            assert "alias.prop" in sp.L.nbg_last_error(sp.h).decode()
    other = X.AliasProp("hermit", "x")  # an alias that names another tag
    assert code_of(lambda: sp.find_vertices(PERSON, other > 0)) == E_INVALID_ARG
    assert code_of(lambda: sp.find_vertices(PERSON, None, [other])) == E_INVALID_ARG
    assert code_of(lambda: sp.find_vertices(PERSON, X.AliasProp("person", "nope") > 0)) == E_IMPROPER_DATA_TYPE
    assert code_of(lambda: sp.find_vertices(PERSON, None, [X.AliasProp("person", "nope")])) == E_IMPROPER_DATA_TYPE
    assert sp.find_vertices(PERSON, PNAME.eq("plain"), [PNAME] * 15).types == [_lib.T_VID] + [_lib.T_STRING] * 15
    assert code_of(lambda: sp.find_vertices(PERSON, PNAME.eq("plain"), [PNAME] * 16)) == E_UNSUPPORTED
    both = GraphSpace(PARTS)
    try:
        both.set_edge_schema(ET, [("w", O.INT)], name="same")
        both.set_tag_schema(PERSON, "same", PFIELDS)
        with pytest.raises(ValueError):
            FindExecutor(both, "same", ["name"])
    finally:
        both.close()
