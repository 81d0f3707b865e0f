"""Tile shapes in the non-final bottom-up first pass (k_bu_lean, option bu_lean_shape).

EdgeSpace::tile_shape holds one word per 128-row slab tile: the tile_wide bit and the out-degree
every row of the tile with an in-edge has (or "mixed").  A two-slot tile (bit clear) never reads its second
half; a uniform tile reads no per-row out-degree and adds degree x found rows to the next hop's
edge count.  Every case runs with bu_lean_shape 1 and 0 and must give the oracle's rows, the same
hop modes, found counts (c[0]) and out-degree sums (c[1]), and never more slab words (c[2]) with
the option on.  bu_force = 1 makes every hop past the first run bottom-up.

The counting instantiation (bu_probe_stats = 2) counts the first pass's work tiles by shape in
c[6] (two-slot) and c[7] (uniform), so a case cannot pass without reaching the new paths; on the
hand-built graphs the counts are compared with the numbering restated here in numpy (layout()).

Hand-built graphs (KV pairs, GO 2 / 3 STEPS without a WHERE, as tests/test_gpu_narrow_tiles.py):
hop 2 of GO 3 STEPS FROM R is the non-final pass under test, its frontier the sources FH and FL.
Sources NH are never in the frontier and have the largest out-degrees, FL the smallest, so in a
hub-first row an FL source sits behind every other one.  See hand_edges().
"""
from collections import Counter

import numpy as np
import pytest

import oracle as O
from nebula_amd import GraphSpace, synth
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

FOLLOW = 1
WCOL = X.AliasProp("follow", "weight")
OPTS = ("bu_force", "bu_lean_shape", "bu_probe_stats", "bu_hub_cap")


# ------------------------------------------------------------------------------------------
# the numbering and the tile shapes, restated
# ------------------------------------------------------------------------------------------
def layout(src, dst, od_key=None):
    """rows in the class-ordered numbering (snapshot k_class_key: class, descending out-degree,
    descending min(in-degree, 3), vid) of the graph with edges src -> dst, and the shapes of the
    tiles below the last row with an in- and an out-edge.  od_key: the out-degrees the numbering
    sorts by when they differ from the graph's (RMAT: sample counts before duplicates collapse)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    vids = np.unique(np.concatenate([src, dst]))
    od = np.bincount(np.searchsorted(vids, src), minlength=len(vids))
    ind = np.bincount(np.searchsorted(vids, dst), minlength=len(vids))
    ok = od if od_key is None else od_key
    cls = np.where(ind > 0, np.where(ok > 0, 0, 1), np.where(ok > 0, 2, 3))
    order = np.lexsort((vids, 3 - np.minimum(ind, 3), -ok, cls))
    vids, od, ind = vids[order], od[order], ind[order]
    live = np.nonzero((od > 0) & (ind > 0))[0]
    work = 0 if len(live) == 0 else (int(live[-1]) + 128) // 128
    tiles = []
    for t in range(work):
        o, i = od[t * 128:(t + 1) * 128], ind[t * 128:(t + 1) * 128]
        o = o[i > 0]  # rows without an in-edge can never be found: their degree does not count
        tiles.append({"rows": len(i), "wide": bool((i >= 3).any()), "uniform": len(o) > 0 and bool((o == o[0]).all()),
                      "deg": int(o[0]) if len(o) else -1})
    return {"vids": vids, "od": od, "ind": ind, "tiles": tiles, "row_of": {int(v): k for k, v in enumerate(vids)}}


def shape_counts(lay):
    return (sum(not t["wide"] for t in lay["tiles"]), sum(t["uniform"] for t in lay["tiles"]))


def hop_records(sp):
    return [(h["mode"], h["final"], list(h["c"][:8])) for h in sp.last_timing()["hops"]]


def assert_same_hops(on, off, diag):
    """hop records with the option on / off: modes, found and out-degree sums equal, never more
    slab words with the option on"""
    assert len(on) == len(off), diag
    for a, b in zip(on, off):
        assert a[:2] == b[:2], diag
        assert (a[2][0], a[2][1]) == (b[2][0], b[2][1]), diag
        assert a[2][2] <= b[2][2], diag


# ------------------------------------------------------------------------------------------
# hand-built graphs
# ------------------------------------------------------------------------------------------
PARTS, ET, VER = 8, 1, 2**63 - 2
R, R2, R3, XV, ZV = 1, 2, 3, 4, 5   # starts; X (only out-edge to the sink Z) and Z: the open variant
FH = list(range(10, 16))            # frontier sources
NH = list(range(20, 26))            # never in the frontier, the largest out-degrees
FL = list(range(30, 36))            # frontier sources, the smallest out-degrees of the sources
POOL = [100000 + j for j in range(300)]  # what the target rows point to; each points back to R, R2
G1, G2W, G2N, G3, G4, G5 = 1000, 2000, 3000, 4000, 5000, 6000  # first vids of the target groups


def narrow_sources(i):
    """in-neighbours of a target row with at most two entries: 2-entry rows with no frontier source /
    FL in slot 1 / FH in slot 1 (hub-first: NH sits in slot 0), 1-entry rows without / with one"""
    j = i // 5
    return [(NH[j % 6], NH[(j + 1) % 6]), (NH[j % 6], FL[j % 6]), (FH[j % 6], NH[j % 6]), (NH[j % 6],),
            (FH[j % 6],)][i % 5]


def wide_sources(i):
    """... with a third entry or more: the only frontier source in slot 2 / slot 3 / fifth (found
    by the rest pass), none among 3 / 5 entries, a frontier source in slot 0 of 3"""
    j = i // 6
    nh = [NH[(j + k) % 6] for k in range(5)]
    return [nh[:2] + [FL[j % 6]], nh[:3] + [FL[j % 6]], nh[:4] + [FL[j % 6]], nh[:3], nh[:5],
            [FH[j % 6]] + nh[:2]][i % 6]


def hand_edges(tail, open_graph=False):
    """(src, dst) pairs.  Rows by descending out-degree, 128 to a tile:
    tile 0: G1, out-degree 300, at most two entries a row (two-slot, uniform, degree > 255);
    tile 1: the 18 sources and R, then 109 wide rows of out-degree 7, R2 among them (mixed, wide);
    tile 2: 20 more wide rows and 108 narrow ones of out-degree 7 (uniform, wide);
    tiles 3-5: 192 rows of out-degree 5 and 192 of out-degree 4 (uniform, mixed, uniform);
    tiles 6-8: the 300 pool vertices (out-degree 2, hundreds of in-edges), then `tail` narrow rows
    of out-degree 1: 30 end inside tile 8 (the last work tile partial and mixed), 262 end 50 rows
    into tile 10 (partial and uniform).  Every vertex has an in- and an out-edge, so the work tiles
    are all tiles.  open_graph: R3 -> X -> Z (Z has no out-edge) is added: GO 3 STEPS FROM R3 finds
    nothing in hop 2."""
    e = [(R, v) for v in FH + FL] + [(R2, v) for v in NH] + [(R2, FH[0])]
    e += [(p, R) for p in POOL] + [(p, R2) for p in POOL]

    def group(first, n, deg, srcs):
        for i in range(n):
            e.extend((s, first + i) for s in srcs(i))
            e.extend((first + i, POOL[k]) for k in range(deg))

    group(G1, 128, 300, narrow_sources)
    group(G2W, 128, 7, wide_sources)  # with R2: 129 wide rows of out-degree 7
    group(G2N, 108, 7, narrow_sources)
    group(G3, 192, 5, narrow_sources)
    group(G4, 192, 4, narrow_sources)
    group(G5, tail, 1, narrow_sources)
    # the sources' out-degrees: NH 280 + i > FH 240 + i > FL 200 + i, padded with edges to the pool
    od = Counter(s for s, _ in e)
    for base, grp in ((280, NH), (240, FH), (200, FL)):
        for i, s in enumerate(grp):
            pad = base + i - od[s]
            assert 0 <= pad <= len(POOL), (s, od[s])
            e.extend((s, POOL[k]) for k in range(pad))
    if open_graph:
        e += [(R3, XV), (XV, ZV)]
    assert len(set(e)) == len(e)
    return e


def kv(edges):
    batch = {}
    for s, d in edges:
        ps, pd = O.part_of(s, PARTS), O.part_of(d, PARTS)
        batch.setdefault(ps, []).append((O.edge_key(ps, s, ET, 0, d, VER), O.encode_row([7])))
        batch.setdefault(pd, []).append((O.edge_key(pd, d, -ET, 0, s, VER), b""))
    return batch


class Hand:
    """a hand-built graph: its layout, the oracle store and (lazily) the engine's space"""

    def __init__(self, tail, open_graph=False):
        self.edges = hand_edges(tail, open_graph)
        self.lay = layout([s for s, _ in self.edges], [d for _, d in self.edges])
        self.batch = kv(self.edges)
        self.st = O.Store(PARTS)
        self.st.set_edge_schema(ET, [("weight", O.INT)], name="e")
        for p, pairs in self.batch.items():
            self.st.put(p, pairs)
        self.st.finalize()
        self._want = {}
        self.sp = None

    def space(self):
        if self.sp is None:
            self.sp = GraphSpace(PARTS)
            self.sp.set_edge_schema(ET, [("weight", O.INT)])
            for p, pairs in self.batch.items():
                self.sp.load_part(p, pairs)
            self.sp.finalize()
        return self.sp

    def want(self, start, steps):
        if (start, steps) not in self._want:
            ref = self.st.go([start], steps, ET, yields=[X.EdgeDst("e").encode()], distinct=True)
            assert ref.code == 0, ref.error
            self._want[start, steps] = Counter(tuple(r) for r in ref.rows())
        return self._want[start, steps]

    def close(self):
        if self.sp is not None:
            self.sp.close()


@pytest.fixture(scope="module")
def hands():
    h = {"mixed_tail": Hand(30), "uniform_tail": Hand(262), "open": Hand(262, True)}
    yield h
    for x in h.values():
        x.close()


def tile_of(lay, vid):
    return lay["row_of"][vid] // 128


def test_hand_graph_layout(hands):
    """the graphs are what hand_edges() says, by the restated numbering (no GPU work)"""
    for name, h in hands.items():
        lay, t = h.lay, h.lay["tiles"]
        od, ind, row = Counter(s for s, _ in h.edges), Counter(d for _, d in h.edges), lay["row_of"]
        # hub-first rows: every NH source before every FH before every FL; all behind G1 rows only
        assert min(od[v] for v in NH) > max(od[v] for v in FH) and min(od[v] for v in FH) > max(od[v] for v in FL)
        assert max(od[v] for v in NH) < 300 and min(od[v] for v in FL) > od[R] > 7
        # tile 0: two-slot, uniform 300, with found / unfound 2-entry rows and 1-entry rows
        assert (t[0]["wide"], t[0]["uniform"], t[0]["deg"]) == (False, True, 300)
        assert {tile_of(lay, G1 + i) for i in range(128)} == {0}
        assert {ind[G1 + i] for i in range(5)} == {1, 2}
        # tile 1: mixed and wide, holding the slot-2 / slot-3 / fifth-entry rows; tile 2 uniform and wide
        assert (t[1]["wide"], t[1]["uniform"]) == (True, False)
        assert {tile_of(lay, G2W + i) for i in range(6)} <= {1, 2} and tile_of(lay, R2) in (1, 2)
        assert [ind[G2W + i] for i in range(6)] == [3, 4, 5, 3, 5, 3]
        assert (t[2]["wide"], t[2]["uniform"], t[2]["deg"]) == (True, True, 7)
        # a mixed tile between two uniform ones
        assert [(x["uniform"], x["deg"]) for x in t[3:6]] == [(True, 5), (False, 5), (True, 4)]
        assert not any(x["wide"] for x in t[3:6])
        # the pool: out-degree 2, wide
        assert (t[6]["wide"], t[6]["uniform"], t[6]["deg"]) == (True, True, 2)
        n = len(lay["vids"])
        if name == "mixed_tail":  # every vertex has both kinds of edge; the last tile partial and mixed
            assert len(t) == 9 and len(t) == (n + 127) // 128 and t[8]["rows"] == 74 and not t[8]["uniform"]
        elif name == "uniform_tail":  # ... partial and uniform
            assert len(t) == 11 and len(t) == (n + 127) // 128
            assert (t[10]["rows"], t[10]["uniform"], t[10]["deg"], t[10]["wide"]) == (50, True, 1, False)
        else:  # X joins the out-degree-1 run; Z and R3 follow the last work row in its tile
            assert len(t) == 11 and row[XV] < row[ZV] < row[R3] and tile_of(lay, ZV) == 10 and not t[10]["uniform"]
        two, uni = shape_counts(lay)
        assert two >= 4 and uni >= 5


def hand_go(sp, start, steps, shape, stats):
    sp.set_option("bu_force", 1)
    sp.set_option("bu_lean_shape", shape)
    sp.set_option("bu_probe_stats", 2 if stats else 0)
    r = sp.go([start], steps, ET, yields=[X.EdgeDst("e")], distinct=True)
    return Counter(tuple(x) for x in r.rows()), hop_records(sp), sp.last_timing()["hops"]


@pytest.mark.parametrize("name", ["mixed_tail", "uniform_tail", "open"])
def test_hand_graph_both_settings(hands, name):
    h = hands[name]
    sp = h.space()
    two, uni = shape_counts(h.lay)
    try:
        for steps in (2, 3):
            want = h.want(R, steps)
            recs = {}
            for stats in (0, 1):
                for shape in (1, 0):
                    got, recs[shape], hops = hand_go(sp, R, steps, shape, stats)
                    diag = (name, steps, shape, stats, recs[shape])
                    print(diag)
                    assert got == want, diag
                    lean = [x for x in hops if x["mode"] == "bottom-up" and not x["final"]]
                    if steps == 3:
                        assert lean and hops[1]["mode"] == "bottom-up" and not hops[1]["final"], diag
                    for x in lean:
                        assert x["kernels"][0].startswith("nbg::k_bu_lean<0, 1, "), diag
                        if not stats:
                            continue
                        # every work tile is counted by its shape -- or none with the option off
                        assert (x["c"][6], x["c"][7]) == ((two, uni) if shape else (0, 0)), diag
                assert_same_hops(recs[1], recs[0], (name, steps, stats, recs))
            if steps == 2:
                found = {v for (v,) in want}
                # G1 (two-slot tile): 2-entry rows found through slot 1 / slot 0, a found 1-entry row,
                # an unfound 2-entry and an unfound 1-entry row
                assert {G1 + 1, G1 + 2, G1 + 4} <= found and not ({G1, G1 + 3} & found)
                # wide tile: the only frontier source in slot 2 / slot 3 / fifth; none among 3 / 5
                assert {G2W, G2W + 1, G2W + 2, G2W + 5} <= found and not ({G2W + 3, G2W + 4} & found)
            else:
                # hop 2 found rows of every out-degree: hop 3 reaches the first 300 pool vertices
                assert {(p,) for p in POOL} <= set(want)
    finally:
        for o in OPTS:
            sp.unset_option(o)


def test_hand_graph_hop2_counters(hands):
    """hop 2 of GO 3 STEPS FROM R on the closed graph: found rows and their out-degree sum are the
    numbers the graph gives, with both settings and in the shipped instantiation"""
    h = hands["uniform_tail"]
    sp = h.space()
    od, front = Counter(s for s, _ in h.edges), set(FH + FL)
    hit = {d for s, d in h.edges if s in front}
    try:
        for shape in (1, 0):
            _, recs, hops = hand_go(sp, R, 3, shape, 0)
            assert hops[1]["kernels"][0] == "nbg::k_bu_lean<0, 1, 1, 0, 1, 3>", hops[1]["kernels"]
            assert recs[1][2][0] == len(hit) and recs[1][2][1] == sum(od[v] for v in hit), (shape, recs)
    finally:
        for o in OPTS:
            sp.unset_option(o)


def test_empty_next_frontier(hands):
    """GO 3 STEPS FROM R3: hop 2's frontier is X, whose only out-edge ends in a vertex without
    out-edges -- no row found, out-degree sum 0, an empty result"""
    h = hands["open"]
    sp = h.space()
    try:
        assert h.want(R3, 3) == Counter() and h.want(R3, 2) == Counter({(ZV,): 1})
        for shape in (1, 0):
            got, recs, hops = hand_go(sp, R3, 3, shape, 0)
            assert got == Counter(), (shape, recs)
            assert hops[1]["mode"] == "bottom-up" and not hops[1]["final"], recs
            assert recs[1][2][:2] == [0, 0], (shape, recs)
            got, _, _ = hand_go(sp, R3, 2, shape, 0)
            assert got == h.want(R3, 2), shape
    finally:
        for o in OPTS:
            sp.unset_option(o)


# ------------------------------------------------------------------------------------------
# a merge commit that introduces new vertices (the snapshot is renumbered and rebuilt)
# ------------------------------------------------------------------------------------------
NEW = [7000 + i for i in range(40)]


def written_edges():
    """40 new rows of out-degree 300 with one in-edge each, from a frontier source or not, and one
    more in-edge, from a frontier source, for two unfound rows of the two-slot tile 0: G1 then has
    three entries (the tile turns wide), G1 + 3 two"""
    e = []
    for i, v in enumerate(NEW):
        e.append(((FH if i % 2 else NH)[i % 6], v))
        e.extend((v, POOL[k]) for k in range(300))
    e += [(FL[0], G1), (FL[1], G1 + 3)]
    return e


@pytest.mark.parametrize("merge", [0, 1])
def test_commit_with_new_vertices(hands, merge):
    base = hands["uniform_tail"]
    after = base.edges + written_edges()
    lay = layout([s for s, _ in after], [d for _, d in after])
    two, uni = shape_counts(lay)
    assert lay["tiles"][0]["wide"] and two >= 3 and uni >= 4  # G1 and G1 + 3 made tile 0 wide
    st = O.Store(PARTS)
    st.set_edge_schema(ET, [("weight", O.INT)], name="e")
    for b in (base.batch, kv(written_edges())):
        for p, pairs in b.items():
            st.put(p, pairs)
    st.finalize()
    sp = GraphSpace(PARTS)
    try:
        sp.set_option("writable", 1)
        sp.set_option("merge_commit", merge)
        sp.set_edge_schema(ET, [("weight", O.INT)])
        for p, pairs in base.batch.items():
            sp.load_part(p, pairs)
        sp.finalize()
        got, _, _ = hand_go(sp, R, 3, 1, 0)
        assert got == base.want(R, 3)
        for p, pairs in kv(written_edges()).items():
            sp.write_part(p, pairs)
        sp.commit()
        for steps in (2, 3):
            ref = st.go([R], steps, ET, yields=[X.EdgeDst("e").encode()], distinct=True)
            assert ref.code == 0, ref.error
            want = Counter(tuple(r) for r in ref.rows())
            recs = {}
            for stats in (0, 1):
                for shape in (1, 0):
                    got, recs[shape], hops = hand_go(sp, R, steps, shape, stats)
                    diag = (merge, steps, shape, stats, recs[shape])
                    print(diag)
                    assert got == want, diag
                    if stats and shape and steps == 3:
                        # the shape words are rebuilt with the slab: still on after the commit, and
                        # after a full rebuild (which renumbers) they are the new numbering's
                        c6, c7 = hops[1]["c"][6], hops[1]["c"][7]
                        assert c6 >= 1 and c7 >= 1, diag
                        if not merge:
                            assert (c6, c7) == (two, uni), diag
                assert_same_hops(recs[1], recs[0], (merge, steps, stats, recs))
            if steps == 2:
                found = {v for (v,) in want}
                assert {G1, G1 + 3, NEW[1], NEW[3]} <= found and not ({NEW[0], NEW[2]} & found)
    finally:
        sp.close()


# ------------------------------------------------------------------------------------------
# RMAT-12 / RMAT-14 against the index-space oracle
# ------------------------------------------------------------------------------------------
class Rmat:
    def __init__(self, scale):
        self.scale = scale
        self.sp = GraphSpace(64)
        self.sp.set_edge_schema(FOLLOW, [("weight", O.INT)])
        self.sp.gen_rmat(scale, 16, 1, FOLLOW)
        self.sp.finalize()
        self.g = O.RmatGraph(scale, 16, 1)
        self.starts = synth.seeds(scale, 16, 1, 16)
        self._want = {}

    def want(self, steps, gt):
        if (steps, gt) not in self._want:
            self._want[steps, gt] = self.g.go(self.starts, steps, where_gt=gt, distinct=True)
        return self._want[steps, gt]


@pytest.fixture(scope="module", params=[12, 14])
def rmat(request):
    r = Rmat(request.param)
    yield r
    r.sp.close()


def test_rmat_has_both_kinds_of_tile(rmat):
    """on the CPU: the scale has two-slot and uniform tiles below the last live row, whether the
    numbering sorts by collapsed out-degrees or by sample counts"""
    s, d, _ = O.rmat_edges(rmat.scale, 16, 1)
    pairs = np.unique(np.stack([s, d], axis=1), axis=0)
    vids = np.unique(pairs)
    samples = np.bincount(np.searchsorted(vids, s), minlength=len(vids))
    for od_key in (None, samples):
        two, uni = shape_counts(layout(pairs[:, 0], pairs[:, 1], od_key))
        print(rmat.scale, "two-slot / uniform tiles:", two, uni)
        assert two >= 1 and uni >= 1


@pytest.mark.parametrize("query", ["go3", "go3_where499", "upto3"])
def test_rmat_both_settings(rmat, query):
    sp = rmat.sp
    gt = 499 if query == "go3_where499" else None
    where = None if gt is None else WCOL > gt
    upto = query == "upto3"
    if upto:
        want = np.unique(np.concatenate([rmat.want(k, None)[0] for k in (1, 2, 3)]))
    else:
        want, scanned = rmat.want(3, gt)
    sp.set_option("bu_force", 1)
    try:
        for hub_cap in (None, 64):
            if hub_cap:
                sp.set_option("bu_hub_cap", hub_cap)
            for stats in (0, 1):
                sp.set_option("bu_probe_stats", 2 if stats else 0)
                recs, scan = {}, {}
                for shape in (1, 0):
                    sp.set_option("bu_lean_shape", shape)
                    r = sp.go(rmat.starts, 3, FOLLOW, where=where, yields=[X.EdgeDst("follow")], distinct=True,
                              upto=upto)
                    recs[shape], scan[shape] = hop_records(sp), r.edges_scanned
                    diag = (rmat.scale, query, hub_cap, stats, shape, recs[shape])
                    print(diag)
                    assert np.array_equal(np.sort(r.columns[0]), want), diag
                    if not upto:
                        assert r.edges_scanned == scanned, diag
                        hops = sp.last_timing()["hops"]
                        assert hops[1]["mode"] == "bottom-up" and not hops[1]["final"], diag
                        assert hops[1]["kernels"][0].startswith("nbg::k_bu_lean<0, 1, "), diag
                        if stats:  # the new paths were reached -- or not, with the option off
                            c6, c7 = hops[1]["c"][6], hops[1]["c"][7]
                            assert (c6 >= 1 and c7 >= 1) if shape else (c6, c7) == (0, 0), diag
                assert scan[1] == scan[0]
                assert_same_hops(recs[1], recs[0], (rmat.scale, query, hub_cap, stats, recs))
    finally:
        for o in OPTS:
            sp.unset_option(o)
