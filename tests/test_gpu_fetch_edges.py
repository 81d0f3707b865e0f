"""FETCH PROP ON an edge type (nbg_fetch_edges; FetchEdgesExecutor over QueryEdgePropsProcessor).

The C++ oracle has no FETCH, so the expectation is restated here from the KV pairs the test writes:
[row(k) for k in keys if k is an edge whose keys sit in src's own part], the bytewise-first version
of the (src, rank, dst) group, key-dedup then row-dedup under DISTINCT.  Every case runs with the
lookup forced to scan (fetch_search = 0), forced to search (1) and as the hybrid (unset); all three
must give the restated rows, column by column and in order (doubles by bit pattern, strings as
bytes).
"""
import ctypes as C
import struct
from collections import Counter

import numpy as np
import pytest

import oracle as O
from nebula_amd import FetchEdgesExecutor, GraphSpace, NbgError, _lib
from nebula_amd import expr as X
from test_gpu_upto_multirank import Group

pytestmark = pytest.mark.gpu

PARTS = 3
REL = 7
FIELDS = [("i", O.INT), ("d", O.DOUBLE), ("b", O.BOOL), ("s", O.STRING)]
PI, PD, PB, PS = (X.AliasProp("rel", f) for f in ("i", "d", "b", "s"))
ALL = [PI, PD, PB, PS]
DEGREES = [0, 1, 15, 16, 17, 63, 64, 65, 300]  # group width 16 and threshold 64, each - 1, + 0, + 1
MODES = [0, 1, None]
UNKNOWN = 42424242
E_STATE, E_INVALID_ARG, E_UNSUPPORTED, E_IMPROPER_DATA_TYPE = -1002, -1001, -1003, -23


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


def dedup(seq):
    seen, out = set(), []
    for x in seq:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def expect(edges, keys, cols=lambda k, p: p, distinct=False):
    """edges: {(src, rank, dst): props}; keys: [(src, dst, rank)]"""
    keys = dedup(keys) if distinct else list(keys)
    out = [tuple(bits(c) for c in cols(k, edges[(k[0], k[2], k[1])])) for k in keys if (k[0], k[2], k[1]) in edges]
    return dedup(out) if distinct else out


def mix(j):
    """a spread of dst vids over the signed range (their bytewise order is not their numeric one)"""
    v = (j * 0x9E3779B97F4A7C15 + 0x1234567) % (1 << 64)
    return v - (1 << 64) if v >= (1 << 63) else v


class Writer:
    """collects KV pairs and the restated winner of every own-part (src, rank, dst) group"""

    def __init__(self, parts):
        self.n_parts = parts
        self.parts = {p: [] for p in range(1, parts + 1)}
        self.groups = {}
        self.seq = 0

    def edge(self, src, dst, rank, ver, props, part=None, etype=REL):
        own = O.part_of(src, self.n_parts)
        part = own if part is None else part
        self.seq += 1
        self.parts[part].append((O.edge_key(part, src, etype, rank, dst, ver), O.encode_row(list(props))))
        pd = O.part_of(dst, self.n_parts)
        self.parts[pd].append((O.edge_key(pd, dst, -etype, rank, src, ver), b""))
        if part == own:
            self.groups.setdefault((src, rank, dst), []).append((le(ver), self.seq, tuple(props)))

    def edges(self):
        out = {}
        for k, ws in self.groups.items():
            first = min(w[0] for w in ws)
            out[k] = max((w for w in ws if w[0] == first), key=lambda w: w[1])[2]
        return out

    def load(self, sp):
        for p, kv in self.parts.items():
            if kv:
                sp.load_part(p, kv)


def props_of(src, j):
    return (src * 1000 + j, j * 0.25 - 3.0, j % 3 == 0, f"s{src}_{j}" if j % 5 else "")


SRC = {deg: 1000 + i for i, deg in enumerate(DEGREES)}
RANK_SRC, RANK_DST = 2000, 2001
RANKS = [0, 1, -1, 1 << 40]
VER_SRC, VER_DST = 2100, 2101
FOREIGN_SRC = 2200


def hand_space():
    w = Writer(PARTS)
    j = 0
    for deg, src in SRC.items():
        for _ in range(deg):
            j += 1
            w.edge(src, mix(j), 0, 9, props_of(src, j))
    w.edge(5000, SRC[0], 0, 9, props_of(5000, 1))  # the degree-0 source is a known vertex
    for r in RANKS:  # one pair under four ranks, and neighbours around it in the row
        w.edge(RANK_SRC, RANK_DST, r, 9, (r, float(r % 1000), r < 0, f"rank{r}"))
    for k in range(20):
        w.edge(RANK_SRC, mix(900 + k), (k % 3) - 1, 9, props_of(RANK_SRC, k))
    # three versions: little-endian 1 -> 01 00 00, 256 -> 00 01 00, 65536 -> 00 00 01: 65536 is first
    for ver in (1, 65536, 256):
        w.edge(VER_SRC, VER_DST, 0, ver, (ver, 0.5, True, f"v{ver}"))
    w.edge(VER_SRC, VER_DST + 1, 0, 4, (4, 1.5, False, "overwritten"))
    w.edge(VER_SRC, VER_DST + 1, 0, 4, (5, 2.5, True, "last write"))
    # a row whose keys sit in a foreign part: invisible, as to GO
    w.edge(FOREIGN_SRC, 1001, 0, 9, (1, 1.0, True, "foreign"), part=O.part_of(FOREIGN_SRC, PARTS) % PARTS + 1)
    sp = GraphSpace(PARTS)
    sp.set_edge_schema(REL, FIELDS, name="rel")
    w.load(sp)
    sp.finalize()
    return sp, w.edges()


@pytest.fixture(scope="module")
def hand():
    sp, edges = hand_space()
    yield sp, edges
    sp.close()


@pytest.fixture(params=MODES, ids=["scan", "search", "hybrid"])
def mode(request):
    return request.param


def set_mode(sp, m):
    if m is None:
        sp.unset_option("fetch_search")
    else:
        sp.set_option("fetch_search", m)


def row_order(edges, src):
    """the (rank, dst) entries of src's row in the row's own order: bytewise by rank, then dst"""
    return sorted(((k[1], k[2]) for k in edges if k[0] == src), key=lambda e: (le(e[0]), le(e[1])))


def test_hand_degrees(hand, mode):
    sp, edges = hand
    set_mode(sp, mode)
    keys = []
    for deg, src in SRC.items():
        row = row_order(edges, src)
        assert len(row) == deg
        if row:
            keys += [(src, row[0][1], 0), (src, row[-1][1], 0), (src, row[len(row) // 2][1], 0)]
        keys += [(src, SRC[300], 0), (src, UNKNOWN, 0)]  # a known vertex that is no neighbour, an unknown vid
    keys += [(UNKNOWN, SRC[1], 0), (UNKNOWN, UNKNOWN, 0)]  # an unknown src
    src, dst, rank = (list(x) for x in zip(*keys))
    rs = sp.fetch_edges(REL, src, dst, rank, ALL)
    assert rs.types == [_lib.T_VID, _lib.T_DOUBLE, _lib.T_BOOL, _lib.T_STRING]
    assert got(rs) == expect(edges, keys)
    assert rs.n_rows == 3 * (len(DEGREES) - 1)
    t = sp.last_timing()
    assert t["hops"] == [] and t["launches"] > 0 and t["host_waits"] == 3 and rs.edges_scanned == t["edges_scanned"] > 0
    # every edge of the 300-row, in row order and reversed
    row = row_order(edges, SRC[300])
    for seq in (row, row[::-1]):
        keys = [(SRC[300], d, r) for r, d in seq]
        rs = sp.fetch_edges(REL, [k[0] for k in keys], [k[1] for k in keys], None, [PI, PS])
        assert got(rs) == expect(edges, keys, lambda k, p: (p[0], p[3])) and rs.n_rows == 300


def test_hand_ranks(hand, mode):
    sp, edges = hand
    set_mode(sp, mode)
    keys = [(RANK_SRC, RANK_DST, r) for r in (1 << 40, 5, -1, 0, 1, -2, 1 << 41)]
    rs = sp.fetch_edges(REL, *(list(x) for x in zip(*keys)), ALL + [X.AliasProp("rel", "_rank")])
    assert got(rs) == expect(edges, keys, lambda k, p: p + (k[2],)) and rs.n_rows == 4
    # rank = None: every key has rank 0
    rs = sp.fetch_edges(REL, [RANK_SRC, RANK_SRC], [RANK_DST, mix(900)], None, [PS])
    assert got(rs) == expect(edges, [(RANK_SRC, RANK_DST, 0), (RANK_SRC, mix(900), 0)], lambda k, p: (p[3],))
    assert (b"rank0",) in got(rs)
    # the whole row, whose ranks -1, 0, 1, 2^40 interleave bytewise (0, 2^40, 1, -1)
    row = row_order(edges, RANK_SRC)
    assert [r for r, _ in row if _ == RANK_DST] == [0, 1 << 40, 1, -1]
    keys = [(RANK_SRC, d, r) for r, d in row]
    rs = sp.fetch_edges(REL, *(list(x) for x in zip(*keys)), [PI])
    assert got(rs) == expect(edges, keys, lambda k, p: (p[0],)) and rs.n_rows == len(row) == 24


def test_hand_versions_and_foreign_part(hand, mode):
    sp, edges = hand
    set_mode(sp, mode)
    assert edges[(VER_SRC, 0, VER_DST)][3] == "v65536" and edges[(VER_SRC, 0, VER_DST + 1)][3] == "last write"
    assert not any(k[0] == FOREIGN_SRC for k in edges)
    keys = [(VER_SRC, VER_DST + 1, 0), (FOREIGN_SRC, 1001, 0), (VER_SRC, VER_DST, 0)]
    rs = sp.fetch_edges(REL, *(list(x) for x in zip(*keys)), ALL)
    assert got(rs) == expect(edges, keys) and rs.n_rows == 2
    assert sp.go([FOREIGN_SRC], 1, REL).n_rows == 0  # the GO visibility rule


@pytest.mark.parametrize("distinct", [False, True])
def test_hand_duplicates_and_key_props(hand, mode, distinct):
    sp, edges = hand
    set_mode(sp, mode)
    a, b = row_order(edges, SRC[17])[3], row_order(edges, SRC[65])[64]
    keys = [(SRC[17], a[1], 0), (SRC[65], b[1], 0), (SRC[17], a[1], 0), (SRC[17], UNKNOWN, 0), (SRC[65], b[1], 0),
            (RANK_SRC, RANK_DST, -1), (SRC[17], a[1], 0), (RANK_SRC, RANK_DST, 1)]
    ys = [X.AliasProp("rel", "_src"), X.AliasProp("x", "_dst"), X.AliasProp("", "_rank"), PI + 1, PS]
    rs = sp.fetch_edges(REL, *(list(x) for x in zip(*keys)), ys, distinct=distinct)
    assert rs.types == [_lib.T_VID] * 4 + [_lib.T_STRING]
    assert got(rs) == expect(edges, keys, lambda k, p: (k[0], k[1], k[2], p[0] + 1, p[3]), distinct)
    assert rs.n_rows == (4 if distinct else 7)
    # different keys with equal rows collapse under DISTINCT
    rs = sp.fetch_edges(REL, *(list(x) for x in zip(*keys)), [PI > -(1 << 62)], distinct=True)
    assert got(rs) == [(True,)]
    # no yields: every field in schema order
    rs = sp.fetch_edges(REL, *(list(x) for x in zip(*keys)), distinct=distinct)
    assert got(rs) == expect(edges, keys, distinct=distinct)


@pytest.mark.parametrize("keep", [False, True])
def test_hand_no_keys_and_no_matches(hand, mode, keep):
    sp, edges = hand
    set_mode(sp, mode)
    for src, dst in (([], []), ([SRC[0], UNKNOWN], [SRC[1], SRC[1]])):
        for distinct in (False, True):
            rs = sp.fetch_edges(REL, src, dst, None, [PS, PI, PB], distinct=distinct, keep_on_device=keep)
            assert rs.n_rows == 0 and rs.types == [_lib.T_STRING, _lib.T_VID, _lib.T_BOOL] and rs.on_device == keep
    assert sp.fetch_edges(REL, [], []).types == [_lib.T_VID, _lib.T_DOUBLE, _lib.T_BOOL, _lib.T_STRING]


def test_constant_nonzero_rank(mode):
    """every edge carries rank 3: the CSR's rank column is one constant"""
    w = Writer(PARTS)
    for j in range(1, 41):
        w.edge(10 + j % 4, mix(j), 3, 9, props_of(1, j))
    sp = GraphSpace(PARTS)
    try:
        sp.set_edge_schema(REL, FIELDS, name="rel")
        w.load(sp)
        sp.finalize()
        set_mode(sp, mode)
        edges = w.edges()
        some = sorted(edges)[::3]
        keys = [(s, d, r) for s, _, d in some for r in (3, 0, -3)]
        rs = sp.fetch_edges(REL, *(list(x) for x in zip(*keys)), ALL + [X.AliasProp("rel", "_rank")])
        assert got(rs) == expect(edges, keys, lambda k, p: p + (3,)) and rs.n_rows == len(some)
        assert sp.fetch_edges(REL, [s for s, _, _ in some], [d for _, _, d in some], None, [PI]).n_rows == 0
    finally:
        sp.close()


def raw_fetch(sp, et, n, on_dev, distinct, keep, yields=(PI,), src=-1, dst=-1):
    ys = [y.encode() for y in yields]
    bufs = [C.create_string_buffer(y, len(y) + 1) for y in ys]
    yp = (C.c_void_p * max(len(ys), 1))(*[C.cast(b, C.c_void_p) for b in bufs])
    yl = (C.c_size_t * max(len(ys), 1))(*[len(y) for y in ys])
    a = np.zeros(8, dtype=np.int64)
    out = _lib.Rows()
    rc = sp.L.nbg_fetch_edges(sp.h, et, a.ctypes.data if src == -1 else src, a.ctypes.data if dst == -1 else dst, None, n,
                              on_dev, yp, yl, len(ys), distinct, keep, C.byref(out))
    if rc == 0:
        sp.L.nbg_rows_free(C.byref(out))
    return rc


def code_of(fn):
    with pytest.raises(NbgError) as e:
        fn()
    return e.value.code


def test_errors(hand):
    sp, edges = hand
    set_mode(sp, None)
    one = ([SRC[1]], [SRC[1]], None)
    fresh = GraphSpace(PARTS)
    try:
        fresh.set_edge_schema(REL, FIELDS)
        assert code_of(lambda: fresh.fetch_edges(REL, *one, [PI])) == E_STATE
    finally:
        fresh.close()
    assert code_of(lambda: sp.fetch_edges(99, *one, [PI])) == E_INVALID_ARG  # unknown edge type
    assert code_of(lambda: sp.fetch_edges(0, *one, [PI])) == E_INVALID_ARG
    for flags in ((2, 0, 0), (0, 2, 0), (0, 0, 2), (-1, 0, 0)):
        assert raw_fetch(sp, REL, 1, *flags) == E_INVALID_ARG
    assert raw_fetch(sp, REL, 1, 0, 0, 0, src=0) == E_INVALID_ARG  # null pointers with n > 0
    assert raw_fetch(sp, REL, 1, 0, 0, 0, dst=0) == E_INVALID_ARG
    assert raw_fetch(sp, REL, 0, 0, 0, 0, src=0, dst=0) == 0
    for node in (X.SourceProp("t", "i"), X.DestProp("t", "i"), X.InputProp("i"), X.VariableProp("v", "i"),
                 X.EdgeDst("rel"), X.EdgeSrc("rel"), X.EdgeRank("rel"), X.EdgeType("rel")):
        assert code_of(lambda: sp.fetch_edges(REL, *one, [PI, node])) == E_INVALID_ARG
        assert "alias.prop" in sp.L.nbg_last_error(sp.h).decode()
    assert code_of(lambda: sp.fetch_edges(REL, *one, [X.Primary(1), X.Primary(2) + 3])) == E_INVALID_ARG
    assert "No props declared" in sp.L.nbg_last_error(sp.h).decode()
    assert code_of(lambda: sp.fetch_edges(REL, *one, [X.AliasProp("rel", "nope")])) == E_IMPROPER_DATA_TYPE
    assert sp.fetch_edges(REL, *one, [PI] * 16).types == [_lib.T_VID] * 16
    assert code_of(lambda: sp.fetch_edges(REL, *one, [PI] * 17)) == E_UNSUPPORTED
    assert code_of(lambda: sp.fetch_edges(REL, *one, [X.AliasProp("rel", "_type")])) == E_UNSUPPORTED
    assert code_of(lambda: sp.fetch_edges(-REL, *one, [PI])) == E_UNSUPPORTED
    assert raw_fetch(sp, REL, 1 << 32, 0, 0, 0) == E_UNSUPPORTED  # refused before a key is read
    with pytest.raises(ValueError):
        sp.fetch_edges(REL, [1, 2], [1], None, [PI])


# ---- RMAT-12 ---------------------------------------------------------------------------------------
FOLLOW = 1
WEIGHT = X.AliasProp("follow", "weight")


@pytest.fixture(scope="module")
def rmat_edges():
    """the graph's (src, dst) -> weight from the oracle store (duplicate samples collapsed as the
    store collapses them), its keys in a seeded shuffled order with 1000 non-edges mixed in"""
    st = O.Store(64)
    st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    st.load_rmat(12, 16, 1, FOLLOW)
    s, d, _ = O.rmat_edges(12, 16, 1)
    r = st.go(np.unique(s), 1, FOLLOW, yields=[X.EdgeSrc("follow").encode(), X.EdgeDst("follow").encode(), WEIGHT.encode()])
    assert r.code == 0
    es, ed, ew = r.int_col(0), r.int_col(1), r.int_col(2)
    edges = {(int(a), int(b)): int(c) for a, b, c in zip(es, ed, ew)}
    assert len(edges) == len(es) > 30000
    rng = np.random.default_rng(11)
    vids = np.unique(np.concatenate([s, d]))
    non = []
    while len(non) < 1000:
        a, b = (int(x) for x in rng.choice(vids, 2))
        if (a, b) not in edges:
            non.append((a, b))
    keys = list(edges) + non
    keys = [keys[i] for i in rng.permutation(len(keys))]
    ks = np.array([k[0] for k in keys], dtype=np.int64)
    kd = np.array([k[1] for k in keys], dtype=np.int64)
    want = np.array([edges[k] for k in keys if k in edges], dtype=np.int64)
    return edges, ks, kd, want


@pytest.fixture(scope="module", params=[1, 0], ids=["col_vid", "vid_of"])
def rmat12(request):
    sp = GraphSpace(64)
    sp.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    sp.set_option("rows_vid_col", request.param)  # 0: the search reads vid_of[col[e]]
    sp.gen_rmat(12, 16, 1, FOLLOW)
    sp.finalize()
    yield sp
    sp.close()


def test_rmat_every_edge(rmat12, rmat_edges, mode):
    edges, ks, kd, want = rmat_edges
    set_mode(rmat12, mode)
    rs = rmat12.fetch_edges(FOLLOW, ks, kd, None, [WEIGHT])
    assert rs.n_rows == len(edges) and np.array_equal(rs.columns[0], want)


def test_rmat_chain_from_go(rmat12, rmat_edges, mode):
    edges, ks, kd, want = rmat_edges
    sp = rmat12
    set_mode(sp, mode)
    starts = np.unique(ks)[:64]
    ys = [X.AliasProp("follow", "_src"), X.AliasProp("follow", "_dst"), WEIGHT]
    dev = sp.go(starts, 2, FOLLOW, yields=ys, keep_on_device=True, order_by=[])
    assert dev.on_device and dev.n_rows > 1000
    rs = sp.fetch_edges(FOLLOW, (dev, 0), (dev, 1), None, [WEIGHT])
    table = sp.order_by(dev, [])  # the GO's own rows on the host (and: the keys were not consumed)
    assert rs.n_rows == dev.n_rows  # every key matches
    assert np.array_equal(rs.columns[0], table.columns[2])
    assert np.array_equal(rs.columns[0], [edges[(int(a), int(b))] for a, b in zip(table.columns[0], table.columns[1])])
    second = sp.go(starts, 2, FOLLOW, yields=[WEIGHT])  # a second GO's weights (its row order is its own)
    assert Counter(second.columns[0].tolist()) == Counter(rs.columns[0].tolist())
    ex = FetchEdgesExecutor(sp, "follow", [WEIGHT], False, src_col=0, dst_col=1)
    assert np.array_equal(ex.execute(dev).columns[0], table.columns[2])
    host = FetchEdgesExecutor(sp, "follow", [WEIGHT]).execute((table.columns[0], table.columns[1]))
    assert np.array_equal(host.columns[0], table.columns[2])


# ---- two ranks on one GPU ------------------------------------------------------------------------
PERSON = 5


def test_two_ranks(mode):
    """every rank passes the same keys and emits the rows of the keys it owns, in key order"""
    w = Writer(4)
    j = 0
    for src, deg in ((1, 3), (2, 70), (3, 17), (4, 1), (6, 90), (7, 5)):
        for _ in range(deg):
            j += 1
            w.edge(src, mix(j) if j % 4 else 1 + j % 7, 0, 9, props_of(src, j))
    edges = w.edges()
    tag_rows = {v: (f"n{v}", v * 3) for v in (1, 2, 3, 6, 50, 51, 52, 53)}  # 50..53: vertices without edges
    for v, row in tag_rows.items():
        p = O.part_of(v, 4)
        w.parts[p].append((O.vertex_key(p, v, PERSON, 0), O.encode_row(list(row))))
    rng = np.random.default_rng(3)
    ekeys = [(k[0], k[2], 0) for k in edges] + [(1, UNKNOWN, 0), (UNKNOWN, 2, 0), (5, 1, 0)]
    ekeys = [ekeys[i] for i in rng.permutation(len(ekeys))]
    vkeys = [int(x) for x in rng.permutation([1, 2, 3, 4, 6, 7, 50, 51, 52, 53, 54, UNKNOWN, 2, 51])]
    vy = [X.AliasProp("person", "name"), X.AliasProp("person", "age")]

    def setup(sp):
        sp.set_edge_schema(REL, FIELDS, name="rel")
        sp.set_tag_schema(PERSON, "person", [("name", O.STRING), ("age", O.INT)])

    def run(sp):
        set_mode(sp, mode)
        e = sp.fetch_edges(REL, *(list(x) for x in zip(*ekeys)), [X.AliasProp("rel", "_src"), X.AliasProp("rel", "_dst")] + ALL)
        v = sp.fetch_vertices(PERSON, vkeys, vy)
        return got(e), got(v)

    one = GraphSpace(4)
    g = Group(2, parts=4)
    try:
        setup(one)
        w.load(one)
        one.finalize()
        one_e, one_v = run(one)
        assert one_e == expect(edges, ekeys, lambda k, p: (k[0], k[1]) + p) and len(one_e) == len(edges)
        assert one_v == [tuple(bits(c) for c in tag_rows[v]) for v in vkeys if v in tag_rows]

        def load(r, sp):
            setup(sp)
            for p, kv in w.parts.items():
                if kv and p % 2 == r:
                    sp.load_part(p, kv)
            sp.finalize()

        g.each(load)
        res = g.each(lambda r, sp: run(sp))
        for which, whole in ((0, one_e), (1, one_v)):
            per_rank = [x[which] for x in res]
            assert Counter(per_rank[0] + per_rank[1]) == Counter(whole)
            assert all(per_rank), "both ranks own some of the keys"
            for r, rows in enumerate(per_rank):  # a rank's rows: the one-rank rows of the keys it owns, in key order
                owner = (lambda row: O.part_of(row[0], 4) % 2) if which == 0 else None
                if owner:
                    assert rows == [x for x in whole if owner(x) == r]
        by_name = {bits(row[0]): v for v, row in tag_rows.items()}
        for r, rows in enumerate(res[i][1] for i in range(2)):
            assert rows == [x for x in one_v if O.part_of(by_name[x[0]], 4) % 2 == r]
            assert any(by_name[x[0]] >= 50 for x in rows)  # a vertex without edges on each rank
    finally:
        g.close()
        one.close()
