"""Integer edge columns off the RMAT `weight` shape ([0, 999], int16, q_min 0): every stored width
(1, 2, 4, 8 bytes), negative values, values on the width boundaries, the whole int64 range
(q_range wraps to 0), a constant column, a predicate on a column that is not the packed one, BOOL /
STRING / DOUBLE columns ahead of the int, VID and TIMESTAMP columns -- through the typed compare
(PK_FAST) of the top-down expansion (k_expand<.., PK_FAST>, also behind a bottom-up first hop) and
of getBound's filter, and through the expression VM on the same columns.  (A column loaded from KV
pairs keeps its present bytes and is therefore never transposed: the bottom-up final hop does not
run on these spaces.)  A writable space starting from the 1-byte layout takes three commits whose
batches push the column to 2, 4 and 8 bytes, as merge commits and as full rebuilds.

One small random graph (8 parts, ~6000 edges, vids over +-2^40), built with exactly 511 and with
512 vertices: at 511 the gidx of the -1 pad word (511) lies inside the last frontier bitmap word
that the bottom-up first hop probes.  Expected rows come from a BFS in plain Python over the edge list (`Ref`);
the oracle store is asserted equal to it on the CPU (test_reference_*), so the GPU tests compare
against both.
"""
import operator
import random
import struct
import zlib
from collections import Counter, defaultdict
from functools import lru_cache

import pytest

import oracle as O
from nebula_amd import GraphSpace
from nebula_amd import expr as X

PARTS, ET, VER = 8, 7, 2**63 - 2
I64_MIN, I64_MAX = -2**63, 2**63 - 1
N_EDGES = 6000

# name -> (expression op, the same compare on Python ints, the op of the mirrored form k op' col)
OPS = {"<": (X.LT, operator.lt, X.GT), "<=": (X.LE, operator.le, X.GE), ">": (X.GT, operator.gt, X.LT),
       ">=": (X.GE, operator.ge, X.LE), "==": (X.EQ, operator.eq, X.EQ), "!=": (X.NE, operator.ne, X.NE)}


def pred(col, op, k, mirrored=False):
    """col op k, or the same compare written k op' col"""
    code, _, mcode = OPS[op]
    c = X.AliasProp("e", col)
    return X.Relational(mcode, X.Primary(k), c) if mirrored else X.Relational(code, c, X.Primary(k))


# ---------------------------------------------------------------------------------------------
# the graph and the column layouts (plain data, no GPU)
# ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def graph(n):
    """n vertices, every one with an in-edge and an out-edge (a ring), five hubs with in-degree
    above 64, random edges up to N_EDGES (mean in-degree ~12: most rows continue past the 4-slot
    slab); no (src, dst) pair twice"""
    rng = random.Random(1000 + n)
    vids = set()
    while len(vids) < n:
        vids.add(rng.randrange(-2**40, 2**40))
    vids = sorted(vids)
    rng.shuffle(vids)
    pairs = {(vids[i], vids[(i + 1) % n]) for i in range(n)}
    for h in vids[:5]:
        for s in rng.sample(vids, 80):
            pairs.add((s, h))
    while len(pairs) < N_EDGES:
        pairs.add((rng.choice(vids), rng.choice(vids)))
    edges = sorted(pairs)
    rng.shuffle(edges)
    return vids, edges


def uniform(rng, m, lo, hi):
    """m values uniform over [lo, hi], both ends present"""
    vals = [rng.randint(lo, hi) for _ in range(m)]
    a, b = rng.sample(range(m), 2)
    vals[a], vals[b] = lo, hi
    return vals


def fixed8(v):
    """the row of one VID / TIMESTAMP column: header byte 0, then the value's 8 bytes (RowWriter)"""
    return b"\x00" + struct.pack("<q", v)


# layout -> (schema fields, predicate column, {column: (lo, hi)} of the int-like columns)
LAYOUTS = {
    "w1": ([("x", O.INT)], "x", {"x": (-128, 127)}),
    "w2": ([("x", O.INT)], "x", {"x": (-129, 128)}),
    "w2b": ([("x", O.INT)], "x", {"x": (-32768, 32767)}),
    "w4": ([("x", O.INT)], "x", {"x": (-32769, 32768)}),
    "w4b": ([("x", O.INT)], "x", {"x": (-2**31, 2**31 - 1)}),
    "w8": ([("x", O.INT)], "x", {"x": (-2**31 - 1, 2**31)}),
    "w8full": ([("x", O.INT)], "x", {"x": (I64_MIN, I64_MAX)}),
    "const": ([("x", O.INT)], "x", {"x": (7, 7)}),
    "two": ([("a", O.INT), ("b", O.INT)], "b", {"a": (0, 999), "b": (-70000, 70000)}),
    "boolfirst": ([("f", O.BOOL), ("x", O.INT)], "x", {"x": (-300, 300)}),
    "strfirst": ([("s", O.STRING), ("d", O.DOUBLE), ("x", O.INT)], "x", {"x": (0, 100000)}),
    "vid": ([("v", O.VID)], "v", {"v": (-2**40, 2**40)}),
    "ts": ([("t", O.TIMESTAMP)], "t", {"t": (1_500_000_000, 1_700_000_000)}),
}
SIZES = (511, 512)
# The reference cannot run GO over a VID / TIMESTAMP edge column: storage collects the value into a
# schemaless row as a varint INT while the response schema names the column's 8-byte type, and
# graphd fails to read its own response ("get edge prop failed"; the oracle restates that).  The
# device evaluates the stored value; for these layouts the Python reference alone is the yardstick.
NO_ORACLE_GO = ("vid", "ts")


def stored_width(lo, hi):
    """bytes of an int-like column holding [lo, hi] (the narrowest of 1, 2, 4, 8)"""
    for w in (1, 2, 4):
        if -(1 << (8 * w - 1)) <= lo and hi < (1 << (8 * w - 1)):
            return w
    return 8


class Ref:
    """GO over an edge list in plain Python: the frontier of a step is the distinct dsts of the
    step before; edges_scanned counts every out-edge of every frontier vertex"""

    def __init__(self, edges, cols):
        self.edges, self.cols = list(edges), {c: list(v) for c, v in cols.items()}
        self.out = defaultdict(list)
        for i, (s, _) in enumerate(self.edges):
            self.out[s].append(i)
        self._final = {}

    def final(self, starts, steps):
        """(edge indices the final step scans, edges scanned over all steps)"""
        key = (tuple(starts), steps)
        if key not in self._final:
            self._final[key] = self._walk(starts, steps)
        return self._final[key]

    def _walk(self, starts, steps):
        front, scanned = sorted(set(starts)), 0
        for _ in range(steps - 1):
            idx = [i for v in front for i in self.out.get(v, ())]
            scanned += len(idx)
            front = sorted({self.edges[i][1] for i in idx})
        idx = [i for v in front for i in self.out.get(v, ())]
        return idx, scanned + len(idx)

    def keep(self, idx, col, op, k):
        if op is None:
            return idx
        cmp, vals = OPS[op][1], self.cols[col]
        return [i for i in idx if cmp(vals[i], k)]

    def distinct_dst(self, starts, steps, col=None, op=None, k=None):
        idx, scanned = self.final(starts, steps)
        return {self.edges[i][1] for i in self.keep(idx, col, op, k)}, scanned

    def rows(self, starts, steps, ycols, col=None, op=None, k=None):
        """multiset of (dst, *ycols) rows"""
        idx, _ = self.final(starts, steps)
        return Counter((self.edges[i][1],) + tuple(self.cols[c][i] for c in ycols) for i in self.keep(idx, col, op, k))


class Case:
    """one (layout, vertex count): the KV pairs per part, the reference and the constants"""

    def __init__(self, layout, n, extra=()):
        self.layout, self.n = layout, n
        self.fields, self.pcol, ranges = LAYOUTS[layout]
        self.vids, edges = graph(n)
        rng = random.Random(zlib.crc32(f"{layout}/{n}".encode()))
        m = len(edges)
        cols = {}
        for name, t in self.fields:
            if name in ranges:
                cols[name] = uniform(rng, m, *ranges[name])
            elif t == O.BOOL:
                cols[name] = [rng.random() < 0.5 for _ in range(m)]
            elif t == O.DOUBLE:
                cols[name] = [rng.uniform(-1.0, 1.0) for _ in range(m)]
            else:
                cols[name] = ["s%d" % rng.randrange(50) for _ in range(m)]
        self.ref = Ref(edges, cols)
        self.parts = self.kv(range(m))
        self.starts = sorted(rng.sample(self.vids, 4))
        self.int_cols = [name for name, t in self.fields if t in (O.INT, O.VID, O.TIMESTAMP)]
        self.width = stored_width(min(cols[self.pcol]), max(cols[self.pcol]))

    def row(self, i):
        vals = [self.ref.cols[name][i] for name, _ in self.fields]
        if self.fields[0][1] in (O.VID, O.TIMESTAMP):
            return fixed8(vals[0])
        return O.encode_row(vals)

    def kv(self, idx):
        """{part: [(key, value)]}: the out-edge row and the empty in-edge key of edges idx"""
        parts = defaultdict(list)
        for i in idx:
            s, d = self.ref.edges[i]
            ps, pd = O.part_of(s, PARTS), O.part_of(d, PARTS)
            parts[ps].append((O.edge_key(ps, s, ET, 0, d, VER), self.row(i)))
            parts[pd].append((O.edge_key(pd, d, -ET, 0, s, VER), b""))
        return parts

    def constants(self):
        """the column's min - 1, min, min + 1, median, max - 1, max, max + 1 and the int64 ends"""
        vals = sorted(self.ref.cols[self.pcol])
        lo, hi = vals[0], vals[-1]
        ks = {lo - 1, lo, lo + 1, vals[len(vals) // 2], hi - 1, hi, hi + 1, I64_MIN, I64_MAX}
        return sorted(k for k in ks if I64_MIN <= k <= I64_MAX)

    def median(self):
        vals = sorted(self.ref.cols[self.pcol])
        return vals[len(vals) // 2]

    def queries(self, ops=tuple(OPS)):
        return [(op, k) for k in self.constants() for op in ops]

    def oracle(self):
        st = O.Store(PARTS)
        st.set_edge_schema(ET, self.fields, name="e")
        for p, kv in self.parts.items():
            st.put(p, kv)
        st.finalize()
        return st

    def space(self, **options):
        sp = GraphSpace(PARTS)
        for k, v in options.items():
            sp.set_option(k, v)
        sp.set_edge_schema(ET, self.fields)
        for p, kv in self.parts.items():
            sp.load_part(p, kv)
        sp.finalize()
        return sp


@lru_cache(maxsize=None)
def case(layout, n):
    return Case(layout, n)


CASES = [(layout, n) for layout in LAYOUTS for n in SIZES]
CASE_IDS = [f"{layout}-{n}" for layout, n in CASES]
DST = X.EdgeDst("e")


# ---------------------------------------------------------------------------------------------
# CPU: the reference against the oracle store, and that its expectations are worth asserting
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,n", CASES, ids=CASE_IDS)
def test_reference_matches_oracle_and_is_not_vacuous(layout, n):
    c = case(layout, n)
    assert len(c.vids) == n and len({v for e in c.ref.edges for v in e}) == n
    indeg = Counter(d for _, d in c.ref.edges)
    assert set(indeg) == set(c.vids) and set(c.ref.out) == set(c.vids)  # an in- and an out-edge each
    assert sum(1 for v in indeg.values() if v > 4) > 100 and sum(1 for v in indeg.values() if v > 64) >= 5
    st = c.oracle()
    full, _ = c.ref.distinct_dst(c.starts, 2)
    telling = 0
    for op, k in c.queries():
        want, scanned = c.ref.distinct_dst(c.starts, 2, c.pcol, op, k)
        telling += bool(want) and want != full
        for mirrored in (False, True):
            r = st.go(c.starts, 2, ET, where=pred(c.pcol, op, k, mirrored).encode(), yields=[DST.encode()], distinct=True)
            if layout in NO_ORACLE_GO:
                assert r.code != 0
                continue
            assert r.code == 0, r.error
            assert set(int(v) for v in r.int_col(0)) == want and r.nrows == len(want), (op, k, mirrored)
            assert r.edges_scanned == scanned
    if layout == "const":  # one value: a compare passes every edge or none, and both happen
        outcomes = {frozenset(c.ref.distinct_dst(c.starts, 2, c.pcol, op, k)[0]) for op, k in c.queries()}
        assert outcomes == {frozenset(), frozenset(full)}
    else:
        assert telling >= 3
    # plain rows with every int-like column, 1 and 2 steps
    ys = [DST] + [X.AliasProp("e", name) for name in c.int_cols]
    op, k = ">=", c.median()
    for steps in (1, 2) if layout not in NO_ORACLE_GO else ():
        r = st.go(c.starts, steps, ET, where=pred(c.pcol, op, k).encode(), yields=[y.encode() for y in ys])
        assert r.code == 0, r.error
        assert Counter(r.rows()) == c.ref.rows(c.starts, steps, c.int_cols, c.pcol, op, k)
    # the column ends are where the layout says, at the width it names
    lo, hi = LAYOUTS[layout][2][c.pcol]
    vals = c.ref.cols[c.pcol]
    assert (min(vals), max(vals)) == (lo, hi)
    expect = {"w1": 1, "w2": 2, "w2b": 2, "w4": 4, "w4b": 4, "w8": 8, "w8full": 8, "const": 1}
    assert layout not in expect or c.width == expect[layout]


# ---------------------------------------------------------------------------------------------
# commits that push the column across a width boundary (plain data + the CPU check of it)
# ---------------------------------------------------------------------------------------------
# per commit: the batch's value range (both ends present) and the width the column then needs
CROSS_STEPS = [(-128, 128, 2), (-40000, 40000, 4), (-2**31, 2**31, 8)]
CROSS_OPS = (">", "==", "<=")


def edge_kv(edges, vals, ver):
    """{part: [(key, value)]} of one-INT-column edges: out-edge rows and empty in-edge keys"""
    parts = defaultdict(list)
    for (s, d), v in zip(edges, vals):
        ps, pd = O.part_of(s, PARTS), O.part_of(d, PARTS)
        parts[ps].append((O.edge_key(ps, s, ET, 0, d, ver), O.encode_row([v])))
        parts[pd].append((O.edge_key(pd, d, -ET, 0, s, ver), b""))
    return parts


class Crossing:
    """the `w1` graph at 512 vertices plus three write batches of 300 new edges each between its
    vertices (no new vertex: the commit can merge); refs[r] is the reference after commit r"""

    def __init__(self):
        self.base = case("w1", 512)
        rng = random.Random(77)
        edges, vals = list(self.base.ref.edges), list(self.base.ref.cols["x"])
        have = set(edges)
        self.batches, self.refs, self.consts = [], [], []
        prev_hi = 127
        for r, (lo, hi, _) in enumerate(CROSS_STEPS):
            new = []
            while len(new) < 300:
                e = (rng.choice(self.base.vids), rng.choice(self.base.vids))
                if e not in have:
                    have.add(e)
                    new.append(e)
            nv = uniform(rng, len(new), lo, hi)
            self.batches.append(edge_kv(new, nv, VER - 10 * (r + 1)))
            edges, vals = edges + new, vals + nv
            self.refs.append(Ref(edges, {"x": vals}))
            # the ends, the old column's top and the first value past it, a middle value
            self.consts.append(sorted({min(vals), sorted(vals)[len(vals) // 2], prev_hi, prev_hi + 1, hi - 1, hi}))
            prev_hi = hi
        self.starts = self.base.starts

    def median(self, r):
        vals = sorted(self.refs[r].cols["x"])
        return vals[len(vals) // 2]

    def oracle(self, r):
        merged = defaultdict(list)
        for parts in [self.base.parts] + self.batches[:r + 1]:
            for p, kv in parts.items():
                merged[p].extend(kv)
        st = O.Store(PARTS)
        st.set_edge_schema(ET, self.base.fields, name="e")
        for p, kv in merged.items():
            st.put(p, kv)
        st.finalize()
        return st


@lru_cache(maxsize=None)
def crossing():
    return Crossing()


def test_crossing_reference_matches_oracle_and_is_not_vacuous():
    x = crossing()
    ys = [DST, X.AliasProp("e", "x")]
    for r, (_, _, width) in enumerate(CROSS_STEPS):
        ref, st = x.refs[r], x.oracle(r)
        assert stored_width(min(ref.cols["x"]), max(ref.cols["x"])) == width
        full, _ = ref.distinct_dst(x.starts, 2)
        before, _ = (x.refs[r - 1] if r else x.base.ref).distinct_dst(x.starts, 2)
        assert full != before  # the batch is seen from the starts
        telling = 0
        for k in x.consts[r]:
            for op in CROSS_OPS:
                want, scanned = ref.distinct_dst(x.starts, 2, "x", op, k)
                telling += bool(want) and want != full
                for mirrored in (False, True):
                    g = st.go(x.starts, 2, ET, where=pred("x", op, k, mirrored).encode(), yields=[DST.encode()], distinct=True)
                    assert g.code == 0, g.error
                    assert set(int(v) for v in g.int_col(0)) == want and g.nrows == len(want), (r, op, k, mirrored)
                    assert g.edges_scanned == scanned
        assert telling >= 3
        for steps in (1, 2):
            g = st.go(x.starts, steps, ET, where=pred("x", ">=", x.median(r)).encode(), yields=[y.encode() for y in ys])
            assert g.code == 0, g.error
            assert Counter(g.rows()) == ref.rows(x.starts, steps, ["x"], "x", ">=", x.median(r))


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CASES, ids=CASE_IDS)
def loaded(request):
    c = case(*request.param)
    sp = c.space()
    yield c, sp
    sp.close()


@pytest.fixture(autouse=True)
def _reset_options(request):
    """the spaces are module-scoped: engine options a test sets on one end with that test"""
    yield
    if "loaded" in request.fixturenames:
        request.getfixturevalue("loaded")[1].reset_options()


@pytest.mark.gpu
def test_where_after_a_bottom_up_hop(loaded):
    """bu_force 1: the first hop runs bottom-up; a column loaded from KV pairs keeps its present
    bytes and is not transposed, so the final hop evaluates the WHERE top-down.  The bottom-up hop
    leaves its counters (entries the rest pass read) in the words the final hop's evaluation-error
    count lives in: the query must not report them as E_EVAL"""
    c, sp = loaded
    sp.set_option("bu_force", 1)
    for op, k in c.queries():
        want, scanned = c.ref.distinct_dst(c.starts, 2, c.pcol, op, k)
        for mirrored in (False, True):
            g = sp.go(c.starts, 2, ET, where=pred(c.pcol, op, k, mirrored), yields=[DST], distinct=True)
            got = [int(v) for v in g.columns[0]]
            assert len(got) == len(set(got)) and set(got) == want, (op, k, mirrored, len(got), len(want))
            assert g.edges_scanned == scanned, (op, k, mirrored)
            hops = sp.last_timing()["hops"]
            assert hops[0]["mode"] == "bottom-up" and hops[-1]["mode"] == "top-down", hops
            assert hops[0]["c"][4] > 0  # the rest pass read entries: the stale word was not zero


@pytest.mark.gpu
def test_top_down_compare_and_vm(loaded):
    """bu_force -1: k_expand<.., PK_FAST> on the same queries; (col + 0) op k is not classified as a
    typed compare and runs the VM (load_int at the column's width): the same rows; YIELD _dst, cols
    without DISTINCT returns every column's exact values"""
    c, sp = loaded
    sp.set_option("bu_force", -1)
    col = X.AliasProp("e", c.pcol)
    n_final = len(c.ref.final(c.starts, 2)[0])
    assert n_final > 0
    for op, k in c.queries():
        want, scanned = c.ref.distinct_dst(c.starts, 2, c.pcol, op, k)
        wheres = [pred(c.pcol, op, k), pred(c.pcol, op, k, True), X.Relational(OPS[op][0], col + 0, X.Primary(k))]
        moved = []
        for i, w in enumerate(wheres):
            g = sp.go(c.starts, 2, ET, where=w, yields=[DST], distinct=True)
            got = [int(v) for v in g.columns[0]]
            assert len(got) == len(set(got)) and set(got) == want, (op, k, i)
            assert g.edges_scanned == scanned, (op, k, i)
            t = sp.last_timing()
            assert t["bu_steps"] == 0
            moved.append(t["expand_bytes"])
        # the byte model counts the predicate column's stored width per final-hop edge for the typed
        # compare alone (the VM's reads are not modelled): both written forms ran as PK_FAST at
        # this layout's width, (col + 0) op k did not
        assert moved[0] == moved[1] and moved[0] - moved[2] == n_final * c.width, (op, k, moved)
    ys = [DST] + [X.AliasProp("e", name) for name in c.int_cols]
    k = c.median()
    for steps in (1, 2):
        for where, args in [(None, ()), (pred(c.pcol, ">=", k), (c.pcol, ">=", k)),
                            (X.Relational(X.LT, col + 0, X.Primary(k)), (c.pcol, "<", k))]:
            g = sp.go(c.starts, steps, ET, where=where, yields=ys)
            assert Counter(g.rows()) == c.ref.rows(c.starts, steps, c.int_cols, *args), (steps, args)
            assert g.n_rows > 0 or args


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["w1", "w4b", "w8full"])
def test_get_bound_filter(layout):
    """getBound's push-down filter col op k (the storage use of the typed compare): per-vertex
    rows in key order, against the oracle store and the reference's row counts"""
    c = case(layout, 512)
    st = c.oracle()
    q = sorted(c.vids)[::7]
    parts = [O.part_of(v, PARTS) for v in q]
    cols = [("_dst", O.EDGE, 0), (c.pcol, O.EDGE, 0)]
    with c.space() as sp:
        for op, k in c.queries():
            f = pred(c.pcol, op, k)
            g = sp.get_bound(ET, parts, q, cols, filter=f)
            r = st.get_bound(ET, parts, q, cols, filt=f.encode())
            rows = g.rows()
            got = {int(v): rows[g.vertex_row_offsets[i]:g.vertex_row_offsets[i + 1]] for i, v in enumerate(g.vertex_ids)}
            want = defaultdict(list)
            for i, row in enumerate(r.rows()):
                want[r.row_vertex(i)].append(row)
            assert {v: rs for v, rs in got.items() if rs} == dict(want), (op, k)
            assert Counter(rows) == c.ref.rows(q, 1, [c.pcol], c.pcol, op, k), (op, k)


def check_crossed(sp, x, r):
    """the queries after commit r: the typed compare top-down and behind a bottom-up first hop, the
    VM form, and the column's values themselves, against the reference of that commit"""
    ref, width = x.refs[r], CROSS_STEPS[r][2]
    col = X.AliasProp("e", "x")
    n_final = len(ref.final(x.starts, 2)[0])
    for force in (-1, 1):
        sp.set_option("bu_force", force)
        for k in x.consts[r]:
            for op in CROSS_OPS:
                want, scanned = ref.distinct_dst(x.starts, 2, "x", op, k)
                moved = []
                for mirrored in (False, True):
                    g = sp.go(x.starts, 2, ET, where=pred("x", op, k, mirrored), yields=[DST], distinct=True)
                    got = [int(v) for v in g.columns[0]]
                    assert len(got) == len(set(got)) and set(got) == want, (r, force, op, k, mirrored, len(got), len(want))
                    assert g.edges_scanned == scanned, (r, force, op, k, mirrored)
                    t = sp.last_timing()
                    assert [h["mode"] for h in t["hops"]] == ["bottom-up" if force == 1 else "top-down", "top-down"]
                    moved.append(t["expand_bytes"])
                if force == -1:
                    # the typed compare read the column at its new stored width (the byte model
                    # counts it per final-hop edge; the VM form's reads are not modelled)
                    g = sp.go(x.starts, 2, ET, where=X.Relational(OPS[op][0], col + 0, X.Primary(k)), yields=[DST], distinct=True)
                    assert set(int(v) for v in g.columns[0]) == want, (r, op, k)
                    vm = sp.last_timing()["expand_bytes"]
                    assert moved[0] == moved[1] and moved[0] - vm == n_final * width, (r, op, k, moved, vm)
    sp.set_option("bu_force", -1)
    k = x.median(r)
    for steps in (1, 2):
        for where, args in [(None, ()), (pred("x", ">=", k), ("x", ">=", k)),
                            (X.Relational(X.LT, col + 0, X.Primary(k)), ("x", "<", k))]:
            g = sp.go(x.starts, steps, ET, where=where, yields=[DST, col])
            assert Counter(g.rows()) == ref.rows(x.starts, steps, ["x"], *args), (r, steps, args)
    q = sorted(x.base.vids)  # every vertex: the batch's top value sits on one or two edges
    parts = [O.part_of(v, PARTS) for v in q]
    g = sp.get_bound(ET, parts, q, [("_dst", O.EDGE, 0), ("x", O.EDGE, 0)], filter=pred("x", ">", CROSS_STEPS[r][1] - 1))
    assert Counter(g.rows()) == ref.rows(q, 1, ["x"], "x", ">", CROSS_STEPS[r][1] - 1) and g.rows()


@pytest.mark.gpu
@pytest.mark.parametrize("merge", [1, 0])
def test_commit_crosses_width_boundaries(merge):
    """a writable space loaded with the 1-byte column; three commits add edges whose values reach
    128, 40000 and 2^31, so the committed column has to be re-narrowed to 2, 4 and 8 bytes -- by
    the merge commit (merge = 1) and by the full rebuild (merge = 0).  Top-down final hops only
    (the bottom-up final hop does not run on KV-loaded columns, module docstring)"""
    x = crossing()
    sp = GraphSpace(PARTS)
    try:
        sp.set_option("writable", 1)
        sp.set_option("merge_commit", merge)
        sp.set_edge_schema(ET, x.base.fields)
        for p, kv in x.base.parts.items():
            sp.load_part(p, kv)
        sp.finalize()
        for r in range(len(CROSS_STEPS)):
            for p, kv in x.batches[r].items():
                sp.write_part(p, kv)
            sp.commit()
            check_crossed(sp, x, r)
        info = sp.info(ET)
        assert info["commits"] == 3
        assert info["merge_commits"] == (3 if merge else 0)
    finally:
        sp.close()
