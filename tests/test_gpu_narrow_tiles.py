"""Two-slot tiles of the final bottom-up first pass (k_bu_fin, option bu_fin_narrow).

A 128-row slab tile whose rows all have at most two in-edges has its tile_wide bit clear: the
kernel reads slots 0-1 only and counts 4 * 64 slab words for it instead of 8 * 64.  The bit comes
from the transposed row_ptr the slab was cut from, so it must stay exact when a merge commit leaves
the numbering stale.  Every case runs with bu_fin_narrow 0 and 1 and must give the oracle's rows.

RMAT-12: the index-space oracle, GO 2 / 3 STEPS ... WHERE weight <op> k YIELD DISTINCT _dst with
the bottom-up direction forced, so the packed predicate decides in the first pass.

Hand-built graph (KV pairs): the column of a space loaded from KV pairs keeps its present bytes and
is not transposed, so a WHERE never runs in a bottom-up hop there (the engine filters top-down
whatever bu_force says).  "The only passing edge sits in slot k" is therefore built a second way,
which does reach k_bu_fin: without a WHERE every edge passes and the frontier decides -- the only
in-neighbour inside the frontier sits in slot k.  Both forms are compared with the oracle store;
the kernel name is asserted for the form without a WHERE.
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
OPS = {">": lambda c, k: c > k, "<=": lambda c, k: c <= k, "==": lambda c, k: c.eq(k)}


def final_hop(sp):
    h = sp.last_timing()["hops"][-1]
    assert h["mode"] == "bottom-up" and h["final"], h
    assert h["kernels"][0].startswith("nbg::k_bu_fin<"), h["kernels"]
    return h


# ------------------------------------------------------------------------------------------
# 1. RMAT-12 against the index-space oracle
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat12():
    sp = GraphSpace(64)
    sp.set_edge_schema(FOLLOW, [("weight", O.INT)])
    sp.gen_rmat(12, 16, 1, FOLLOW)
    sp.finalize()
    g = O.RmatGraph(12, 16, 1)
    want = {}

    def oracle(starts, steps, op, k):
        if (steps, op, k) not in want:
            want[(steps, op, k)] = g.go(starts, steps, distinct=True, where=(op, k))
        return want[(steps, op, k)]

    yield sp, oracle
    sp.close()


@pytest.mark.parametrize("hub_cap", [None, 64])
@pytest.mark.parametrize("op", list(OPS))
def test_rmat12_oracle_both_settings(rmat12, op, hub_cap):
    sp, oracle = rmat12
    starts = synth.seeds(12, 16, 1, 64)
    sp.set_option("bu_force", 1)
    if hub_cap:
        sp.set_option("bu_hub_cap", hub_cap)
    try:
        for k in (0, 499, 998):
            for steps in (2, 3):
                want, scanned = oracle(starts, steps, op, k)
                hops = {}
                for narrow in (0, 1):
                    sp.set_option("bu_fin_narrow", narrow)
                    r = sp.go(starts, steps, FOLLOW, where=OPS[op](WCOL, k), yields=[X.EdgeDst("follow")],
                              distinct=True)
                    diag = (op, k, steps, narrow)
                    assert np.array_equal(np.sort(r.columns[0]), want), diag
                    assert r.edges_scanned == scanned, diag
                    final_hop(sp)
                    hops[narrow] = [h["c"][:4] for h in sp.last_timing()["hops"]]
                print(op, k, steps, hub_cap, "final c, narrow 0 / 1:", hops[0][-1], hops[1][-1])
                assert len(hops[0]) == len(hops[1])
                for c0, c1 in zip(hops[0], hops[1]):
                    assert (c0[0], c0[1], c0[3]) == (c1[0], c1[1], c1[3]), (op, k, steps, hops)
                saved = hops[0][-1][2] - hops[1][-1][2]  # 4 * 64 slab words per two-slot tile
                assert saved > 0 and saved % 256 == 0, (op, k, steps, hops)
    finally:
        for o in ("bu_force", "bu_hub_cap", "bu_fin_narrow"):
            sp.unset_option(o)


# ------------------------------------------------------------------------------------------
# 2. / 3. hand-built graph against the oracle store
# ------------------------------------------------------------------------------------------
PARTS, ET, VER = 8, 1, 2**63 - 2
R, R2 = 1, 2                      # the start (in-edges of the frontier sources) / of the other sources
NH = list(range(20, 26))          # highest out-degree, never in the frontier (in-edges from R2)
FH = list(range(10, 16))          # in the frontier (in-edges from R)
FL = list(range(30, 36))          # in the frontier, the lowest out-degree: last in every row
N1, N2 = 50, 51                   # test 3: written after finalize; N2 in the frontier
HI, LO = 900, 100                 # weights: edges out of FL / N2 pass weight > 499, the others fail


def base_edges():
    """(src, dst, weight).  Sinks (out-degree 0): A in-degree 1, B in-degree 2, C 3 / 4 / 5; the
    numbering puts C, then B, then A behind the 18 sources, so the tiles from row 128 on hold only
    rows of in-degree <= 2."""
    e = [(R, v, 0 if i % 2 else 999) for i, v in enumerate(FH + FL)] + [(R2, v, 500) for v in NH]
    nh = lambda i, j=0: NH[(i + j) % 6]  # noqa: E731
    for i in range(200):  # A: one in-edge
        e.append(((NH if i % 2 else FH)[i // 2 % 6], 1000 + i, LO))
    for i in range(300):  # B: two in-edges
        d, j = 2000 + i, i // 4
        pair = [(nh(j), nh(j, 1)),       # no in-neighbour in the frontier
                (nh(j), FL[j % 6]),      # the only one in the frontier (and the only HI) in slot 1
                (FH[j % 6], nh(j)),
                (FH[j % 6], FL[j % 6])][i % 4]
        e += [(pair[0], d, LO), (pair[1], d, HI if pair[1] in FL else LO)]
    for i in range(12):  # C: the only frontier in-neighbour in slot 2 / slot 3 (every third row: none)
        none = i % 3 == 2
        e += [(nh(i), 3000 + i, LO), (nh(i, 1), 3000 + i, LO)]
        e.append((nh(i, 2), 3000 + i, LO) if none else (FL[i % 6], 3000 + i, HI))
        e += [(nh(i), 4000 + i, LO), (nh(i, 1), 4000 + i, LO), (nh(i, 2), 4000 + i, LO)]
        e.append((nh(i, 3), 4000 + i, LO) if none else (FL[i % 6], 4000 + i, HI))
    for i in range(4):  # a fifth entry: pending after the slab, found by the rest pass
        e += [(nh(i, j), 5000 + i, LO) for j in range(4)] + [(FL[i], 5000 + i, HI)]
    return e


# test 3: rows of a two-slot tile (B rows without a frontier in-neighbour, among the last by vid)
TO3, TO4, UNTOUCHED = [2280, 2284], [2288, 2292], 2296


def written_edges():
    e = [(R, N2, 7), (R2, N1, 7)]
    e += [(N2, d, HI) for d in TO3 + TO4] + [(N1, d, LO) for d in TO4]
    return e


def kv(edges, ver):
    batch = {}
    for s, d, w in edges:
        ps, pd = O.part_of(s, PARTS), O.part_of(d, PARTS)
        batch.setdefault(ps, []).append((O.edge_key(ps, s, ET, 0, d, ver), O.encode_row([w])))
        batch.setdefault(pd, []).append((O.edge_key(pd, d, -ET, 0, s, ver), b""))
    return batch


def oracle_rows(batches, where):
    st = O.Store(PARTS)
    st.set_edge_schema(ET, [("weight", O.INT)], name="e")
    merged = {}
    for b in batches:
        for p, pairs in b.items():
            merged.setdefault(p, []).extend(pairs)
    for p, pairs in merged.items():
        st.put(p, pairs)
    st.finalize()
    ref = st.go([R], 2, ET, where=X.encode(where), yields=[X.EdgeDst("e").encode()], distinct=True)
    assert ref.code == 0, ref.error
    return Counter(tuple(r) for r in ref.rows())


WHERES = {"none": None, "w499": X.AliasProp("e", "weight") > 499}


@pytest.fixture(scope="module")
def hand_want():
    base, wr = kv(base_edges(), VER), kv(written_edges(), VER - 10)
    return {(n, k): oracle_rows(b, w) for n, b in (("base", [base]), ("written", [base, wr])) for k, w in WHERES.items()}


def hand_space(merge=None):
    sp = GraphSpace(PARTS)
    if merge is not None:
        sp.set_option("writable", 1)
        sp.set_option("merge_commit", merge)
    sp.set_edge_schema(ET, [("weight", O.INT)])
    for p, pairs in kv(base_edges(), VER).items():
        sp.load_part(p, pairs)
    sp.finalize()
    sp.set_option("bu_force", 1)
    return sp


def hand_go(sp, where, narrow):
    sp.set_option("bu_fin_narrow", narrow)
    r = sp.go([R], 2, ET, where=where, yields=[X.EdgeDst("e")], distinct=True)
    return r, Counter(tuple(x) for x in r.rows())


def test_hand_graph_shape():
    """the graph is what the docstrings say: degrees, the slot order's premise, a partial last tile"""
    e = base_edges()
    assert len({(s, d) for s, d, _ in e}) == len(e)
    od, ind = Counter(s for s, _, _ in e), Counter(d for _, d, _ in e)
    verts = set(od) | set(ind)
    assert len(verts) < 700 and len(verts) % 128 != 0
    sinks = [v for v in verts if od[v] == 0]
    assert sum(ind[v] == 1 for v in sinks) >= 130 and sum(ind[v] == 2 for v in sinks) >= 130
    # hub-first rows: every FL source sorts behind every other source
    assert max(od[v] for v in FL) < min(od[v] for v in FH) and max(od[v] for v in FH) < min(od[v] for v in NH)


def test_hand_graph_both_settings(hand_want):
    sp = hand_space()
    try:
        assert sp.info(ET)["num_vertices"] % 128 != 0
        c2 = {}
        for narrow in (0, 1):
            r, got = hand_go(sp, None, narrow)
            assert got == hand_want["base", "none"], narrow
            h = final_hop(sp)
            c2[narrow] = h["c"][2]
            found = {v for (v,) in got}
            # slot 1 / 2 / 3 / past the slab, and rows without a frontier in-neighbour
            assert {2001, 2005, 3000, 3001, 4000, 4001, 5000} <= found
            assert not ({2000, 2004, 3002, 4002} & found)
            _, got = hand_go(sp, WHERES["w499"], narrow)
            assert got == hand_want["base", "w499"], narrow
        # rows 0-127 (sources, C, B) are the one tile with a third entry; 128-545 are four tiles of
        # in-degree <= 2, the last one partial
        assert c2[0] == 5 * 512 and c2[1] == 512 + 4 * 256, c2
    finally:
        sp.close()


@pytest.mark.parametrize("merge", [0, 1])
def test_stale_numbering_after_commit(hand_want, merge):
    """rows of a two-slot tile gain a third and a fourth in-edge after finalize; the only
    in-neighbour in the frontier (and the only edge passing weight > 499) is the new one"""
    sp = hand_space(merge)
    try:
        for p, pairs in kv(written_edges(), VER - 10).items():
            sp.write_part(p, pairs)
        _, got = hand_go(sp, None, 1)
        assert got == hand_want["base", "none"]  # not committed yet
        sp.commit()
        assert sp.info(ET)["merge_commits"] == merge
        for narrow in (1, 0):
            _, got = hand_go(sp, None, narrow)
            final_hop(sp)
            found = {v for (v,) in got}
            assert set(TO3 + TO4) <= found and UNTOUCHED not in found, (merge, narrow)
            assert got == hand_want["written", "none"], (merge, narrow)
            _, got = hand_go(sp, WHERES["w499"], narrow)
            assert got == hand_want["written", "w499"], (merge, narrow)
    finally:
        sp.close()
