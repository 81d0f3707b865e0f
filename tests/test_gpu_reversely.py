"""GO ... OVER e REVERSELY on one rank (include/nebula_amd.h, DESIGN.md divergence 11): nbg_go with
edge_type = -t expands the in keys.  Parity against the oracle's own path with a negative type
(`Store.go(starts, steps, -etype, ...)`): rows as multisets (sets under DISTINCT) together with
edges_scanned.  The pull hop (nbg::k_rev_pull, hop mode 6) is forced with bu_force = 1 and
forbidden with bu_force = -1; the result never depends on it, and it runs only where the in keys
mirror the out keys.
"""
from collections import Counter

import numpy as np
import pytest

import fixtures as F
import oracle as O
from nebula_amd import GraphSpace, NbgError, _lib
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

FOLLOW = 1
SEED = 1
VER = 2**63 - 2
E_IMPROPER = -23  # NBG_E_IMPROPER_DATA_TYPE
KLANE = 4         # entries a lane of k_rev_pull scans alone (kRevLane)


def ms(rows):
    return Counter(tuple(r) for r in rows)


def enc(yields):
    return [y.encode() for y in yields]


def modes(sp):
    return [(h["mode_id"], h["final"], h["kernels"]) for h in sp.last_timing()["hops"]]


def forced(sp, force):
    """context manager: bu_force for the block"""
    class _F:
        def __enter__(self):
            if force is not None:
                sp.set_option("bu_force", force)

        def __exit__(self, *a):
            sp.set_option("bu_force", 0)
    return _F()


def check_go(sp, st, starts, steps, et, where=None, yields=(), distinct=False, inputs=None, reversely=True):
    """one REVERSELY query against the oracle's negative-type run; returns the engine's RowSet"""
    want = st.go(starts, steps, -et if reversely else et, where=X.encode(where), yields=enc(yields), distinct=distinct,
                 inputs=inputs)
    assert want.code == 0, want.error
    got = sp.go(starts, steps, et, where=where, yields=yields, distinct=distinct, inputs=inputs, reversely=reversely)
    diag = (list(starts)[:8], steps, distinct, modes(sp))
    assert ms(got.rows()) == ms(want.rows()), diag
    assert got.edges_scanned == want.edges_scanned, diag
    return got


# ------------------------------------------------------------------------------------------
# NBA space (KV-loaded, one part)
# ------------------------------------------------------------------------------------------
NBA_TAGS = {F.NBA_PLAYER: ("player", [("name", O.STRING), ("age", O.INT)]),
            F.NBA_TEAM: ("team", [("name", O.STRING)])}


@pytest.fixture(scope="module")
def nba():
    sp = GraphSpace(1)
    for et, (name, fields) in F.NBA_EDGE_SCHEMAS.items():
        sp.set_edge_schema(et, fields)
    for tag, (name, fields) in NBA_TAGS.items():
        sp.set_tag_schema(tag, name, fields)
    parts, vid = F.nba_kv()
    for p, kv in parts.items():
        sp.load_part(p, kv)
    sp.finalize()
    st, _ = F.nba_oracle_store()
    yield sp, st, vid, F.nba()
    sp.close()


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("steps", [1, 2])
def test_nba_followers(nba, steps, distinct):
    sp, st, vid, d = nba
    starts = [vid["Tim Duncan"], vid["Tony Parker"], vid["Tim Duncan"]]
    got = check_go(sp, st, starts, steps, F.NBA_LIKE, distinct=distinct)
    assert got.n_rows > 0
    if steps == 1 and distinct:
        want = {vid[a] for a, b, _ in d["like"] if b in ("Tim Duncan", "Tony Parker")}
        assert set(got.columns[0].tolist()) == want  # "who likes Tim or Tony", from the edge list itself


def test_nba_edge_key_yields(nba):
    sp, st, vid, d = nba
    ys = [X.EdgeSrc("like"), X.EdgeDst("like"), X.EdgeRank("like"), X.EdgeType("like")]
    for steps in (1, 2):
        got = check_go(sp, st, [vid["Tim Duncan"]], steps, F.NBA_LIKE, yields=ys)
        assert got.n_rows > 0
    got = sp.go([vid["Tim Duncan"]], 1, -F.NBA_LIKE, yields=ys)  # a negative type passed directly
    for src, dst, rank, typ in got.rows():
        assert src == vid["Tim Duncan"] and rank == 0 and typ == "like"
        assert dst in {vid[a] for a, b, _ in d["like"] if b == "Tim Duncan"}


def test_nba_tag_props_and_where(nba):
    sp, st, vid, d = nba
    ys = [X.SourceProp("player", "name"), X.DestProp("player", "name"), X.DestProp("player", "age")]
    starts = [vid["Tim Duncan"], vid["LeBron James"], vid["Tony Parker"]]
    for steps in (1, 2):
        for distinct in (False, True):
            got = check_go(sp, st, starts, steps, F.NBA_LIKE, yields=ys, distinct=distinct)
            assert got.n_rows > 0
            w = X.DestProp("player", "age") > 33
            got = check_go(sp, st, starts, steps, F.NBA_LIKE, where=w, yields=ys, distinct=distinct)
            assert got.n_rows > 0 and all(r[2] > 33 for r in got.rows())
            check_go(sp, st, starts, steps, F.NBA_LIKE, where=w, distinct=distinct)  # the default YIELD


def test_nba_edge_props_are_refused(nba):
    """in-bound keys carry no schema props: reported once the final step runs (its frontier has in-edges)"""
    sp, st, vid, d = nba
    tim = [vid["Tim Duncan"]]
    like = X.AliasProp("like", "likeness")
    for steps in (1, 2):
        assert st.go(tim, steps, -F.NBA_LIKE, yields=enc([like])).code != 0
        assert st.go(tim, steps, -F.NBA_LIKE, where=(like > 80).encode()).code != 0
        with pytest.raises(NbgError) as e:
            sp.go(tim, steps, F.NBA_LIKE, yields=[like], reversely=True)
        assert e.value.code == E_IMPROPER and "in-bound" in str(e.value)
        with pytest.raises(NbgError) as e:
            sp.go(tim, steps, F.NBA_LIKE, where=like > 80, reversely=True)
        assert e.value.code == E_IMPROPER
    assert sp.go(tim, 1, F.NBA_LIKE, reversely=True).n_rows > 0  # the context still answers


def test_nba_unknown_start_and_errors(nba):
    sp, st, vid, d = nba
    for steps in (1, 2):
        assert check_go(sp, st, [d["nonexist_hash"]], steps, F.NBA_LIKE).n_rows == 0
    assert sp.go([], 2, F.NBA_LIKE, reversely=True).n_rows == 0
    # the deferred error is not raised when the frontier empties first
    assert sp.go([d["nonexist_hash"]], 2, F.NBA_LIKE, where=X.AliasProp("like", "likeness") > 1,
                 reversely=True).n_rows == 0
    for bad in (0, -77):
        with pytest.raises(NbgError) as e:
            sp.go([vid["Tim Duncan"]], 1, bad)
        assert e.value.code == -1001  # NBG_E_INVALID_ARG
    with pytest.raises(ValueError):
        sp.go([vid["Tim Duncan"]], 1, -F.NBA_LIKE, reversely=True)


@pytest.mark.parametrize("steps", [1, 2])
def test_nba_input_props(nba, steps):
    sp, st, vid, d = nba
    starts = [vid["Tim Duncan"], vid["Tony Parker"], vid["Manu Ginobili"]]
    inputs = [("tag", O.STRING, ["a", "b", "c"]), ("n", O.INT, [1, 2, 3])]
    ys = [X.InputProp("tag"), X.InputProp("n") * 10, X.EdgeDst("like"), X.DestProp("player", "name")]
    got = check_go(sp, st, starts, steps, F.NBA_LIKE, yields=ys, inputs=inputs)
    assert got.n_rows > 0
    check_go(sp, st, starts, steps, F.NBA_LIKE, where=X.InputProp("n") > 1, yields=ys, inputs=inputs)


def test_nba_serve_from_a_team(nba):
    sp, st, vid, d = nba
    got = check_go(sp, st, [vid["Spurs"]], 1, F.NBA_SERVE,
                   yields=[X.DestProp("player", "name"), X.SourceProp("team", "name")])
    assert got.n_rows == 17 and all(r[1] == "Spurs" for r in got.rows())
    assert {r[0] for r in got.rows()} == {a for a, t, _, _ in d["serve"] if t == "Spurs"}


# ------------------------------------------------------------------------------------------
# RMAT-12: gen_rmat against Store.load_rmat; the pull hop forced, free and forbidden
# ------------------------------------------------------------------------------------------
class Rmat12:
    def __init__(self):
        self.sp = GraphSpace(64)
        self.sp.set_edge_schema(FOLLOW, [("weight", O.INT)])
        self.sp.gen_rmat(12, 16, SEED, FOLLOW)
        self.sp.finalize()
        self.st = O.Store(64)
        self.st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
        self.st.load_rmat(12, 16, SEED, FOLLOW)
        s, d, _ = O.rmat_edges(12, 16, SEED)
        self.src, self.dst = s, d
        pairs = np.unique(np.stack([s, d], axis=1), axis=0)  # duplicate (src, dst) collapse
        self.vids = np.unique(pairs)
        self.si = np.searchsorted(self.vids, pairs[:, 0])
        self.di = np.searchsorted(self.vids, pairs[:, 1])
        self.ideg = np.bincount(self.di, minlength=len(self.vids))
        self._want = {}

    def dsts(self, n, seed):
        return np.random.default_rng(seed).choice(np.unique(self.dst), n, replace=False).astype(np.int64)

    def want(self, key, starts, steps, distinct, et=-FOLLOW):
        """the oracle's answer (computed once per case, never changed)"""
        ck = (key, steps, distinct, et)
        if ck not in self._want:
            r = self.st.go(starts, steps, et, distinct=distinct)
            assert r.code == 0
            self._want[ck] = (ms(r.rows()), r.edges_scanned)
        return self._want[ck]

    def upto_scanned(self, starts, n_steps):
        """sum_{k<N} indeg(B_k) + indeg(U): the pruned BFS over in-edges (nebula_amd.h)"""
        n = len(self.vids)
        st = np.unique(starts)
        B = np.searchsorted(self.vids, st[np.isin(st, self.vids)])
        seen = np.zeros(n, bool)
        seen[B] = True
        total = 0
        for _ in range(1, n_steps):
            total += int(self.ideg[B].sum())
            front = np.zeros(n, bool)
            front[B] = True
            reached = np.unique(self.si[front[self.di]])
            B = reached[~seen[reached]]
            seen[B] = True
        return total + int(self.ideg[seen].sum())


@pytest.fixture(scope="module")
def rmat12():
    r = Rmat12()
    yield r
    r.sp.close()


def rmat_starts(r, which):
    s = r.dsts(4, 3)
    return s if which == "four" else np.concatenate([s, s[:2], s[:1]])


def check_pull_modes(hops, steps, distinct, force):
    pulled = [m == 6 for m, _, _ in hops]
    if force == -1:
        assert not any(pulled), hops
    if force == 1:
        for m, final, kernels in hops:
            if not final or distinct:  # (the default YIELD is the lone e._dst)
                assert m == 6 and kernels[0] == "nbg::k_rev_pull", hops
            else:
                assert m == 0, hops
        assert len(hops) == steps, hops


@pytest.mark.parametrize("force", [-1, None, 1])
@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("which", ["four", "dups"])
def test_rmat12_reversely(rmat12, which, steps, distinct, force):
    r, sp = rmat12, rmat12.sp
    assert sp.info(FOLLOW)["num_vertices"] % 64 != 0  # the last bitmap word is partial
    starts = rmat_starts(r, which)
    want, scanned = r.want(which, starts, steps, distinct)
    assert sum(want.values()) > 0
    with forced(sp, force):
        got = sp.go(starts, steps, FOLLOW, distinct=distinct, reversely=True)
        hops = modes(sp)
    assert ms(got.rows()) == want, (which, steps, distinct, force, hops)
    assert got.edges_scanned == scanned, (which, steps, distinct, force, hops)
    check_pull_modes(hops, steps, distinct, force)


def test_rmat12_forward_unchanged(rmat12):
    """bu_force is shared with the forward direction: plain GO on the same space still equals the oracle"""
    r, sp = rmat12, rmat12.sp
    starts = np.random.default_rng(9).choice(np.unique(r.src), 4, replace=False).astype(np.int64)
    for force in (-1, None, 1):
        for distinct in (False, True):
            want, scanned = r.want("fwd", starts, 3, distinct, et=FOLLOW)
            with forced(sp, force):
                got = sp.go(starts, 3, FOLLOW, distinct=distinct)
                assert all(m != 6 for m, _, _ in modes(sp))
            assert ms(got.rows()) == want and got.edges_scanned == scanned, (force, distinct)


@pytest.mark.parametrize("force", [None, 1])
def test_rmat12_upto_reversely(rmat12, force):
    r, sp = rmat12, rmat12.sp
    starts = rmat_starts(r, "four")
    per_step = [r.want("four", starts, k, False) for k in (1, 2, 3)]
    concat = sum((w for w, _ in per_step), Counter())
    with forced(sp, force):
        got = sp.go(starts, 3, FOLLOW, upto=True, reversely=True)
        assert all(m != 6 for m, _, _ in modes(sp))  # UPTO REVERSELY runs top-down hops only
        assert ms(got.rows()) == concat
        assert got.edges_scanned == sum(concat.values())  # the (step, adjacency entry) pairs examined
        got = sp.go(starts, 3, FOLLOW, distinct=True, upto=True, reversely=True)
        hops = modes(sp)
        assert all(m != 6 for m, _, _ in hops)
        assert "nbg::k_upto_bu" not in [k for _, _, ks in hops for k in ks]
    assert ms(got.rows()) == Counter(set(concat))
    assert got.edges_scanned == r.upto_scanned(starts, 3)


def test_rmat12_chaining_on_device(rmat12):
    """followers-of-A INTERSECT followers-of-B, then ORDER BY, without a host copy in between"""
    r, sp = rmat12, rmat12.sp
    hubs = r.vids[np.argsort(-r.ideg)[:2]]  # the two vertices with the most followers
    a, b = int(hubs[0]), int(hubs[1])
    # (order_by=[] keeps a GO's table in HBM with its RowSet; a plain keep_on_device hands it back at once)
    fa = sp.go([a], 1, FOLLOW, distinct=True, keep_on_device=True, order_by=[], reversely=True)
    fb = sp.go([b], 1, FOLLOW, distinct=True, keep_on_device=True, order_by=[], reversely=True)
    assert fa.on_device and fb.on_device
    both = sp.set_op(_lib.SET_INTERSECT, fa, fb, keep_on_device=True)
    assert both.on_device
    out = sp.order_by(both, [(0, 0)])
    sa, sb = set(r.src[r.dst == a].tolist()), set(r.src[r.dst == b].tolist())
    assert out.columns[0].tolist() == sorted(sa & sb) and len(sa & sb) > 0


# ------------------------------------------------------------------------------------------
# a hand-built KV graph for k_rev_pull's branches (one part, mirrored)
# ------------------------------------------------------------------------------------------
LAST, FIRST = 209, 1          # the largest / smallest vid: last / first in every row's key order
DEAD, DL1, DL2 = 250, 251, 252  # DEAD's in-neighbours have no in-edges: a frontier that dies
DEGS = {0: KLANE, 1: KLANE + 1, 2: KLANE + 64, 3: KLANE + 65, 4: 200}


def branch_edges():
    """every u in 2..208 is a source: by u % 7 its out-degree is K, K+1, K+64, K+65 or 200 with LAST
    as the only frontier dst (the last entry in key order: all vids < 256, one key byte decides), or
    its first entry is FIRST, or it has no frontier dst at all.  Whatever the numbering, local rows
    63, 64 and the last one hold such a row.  The fillers are the smallest vids, so 202..208 have
    no in-edge: found by a hop from LAST, dropped at a non-final hop, kept at the final one."""
    edges = []
    for u in range(2, 209):
        fill = [v for v in range(2, 209) if v != u]
        k = u % 7
        if k in DEGS:
            edges += [(u, v) for v in fill[:DEGS[k] - 1]] + [(u, LAST)]
        elif k == 5:
            edges += [(u, FIRST)] + [(u, v) for v in fill[:5]]
        else:
            edges += [(u, v) for v in fill[:10]]
    edges += [(DL1, DEAD), (DL2, DEAD)]
    return edges


def kv_pairs(edges, parts=1, in_keys=None):
    """{part: [(key, value)]}: an out key with its row and the in key of every edge (rank 0);
    in_keys overrides the in side as (v, rank, u) triples"""
    kv = {p: [] for p in range(1, parts + 1)}
    for s, d in edges:
        ps = O.part_of(s, parts)
        kv[ps].append((O.edge_key(ps, s, FOLLOW, 0, d, VER), O.encode_row([s + d])))
    for v, rank, u in (in_keys if in_keys is not None else [(d, 0, s) for s, d in edges]):
        pv = O.part_of(v, parts)
        kv[pv].append((O.edge_key(pv, v, -FOLLOW, rank, u, VER), b""))
    return kv


def load_both(kv, parts=1, writable=False):
    sp = GraphSpace(parts)
    sp.set_edge_schema(FOLLOW, [("weight", O.INT)])
    if writable:
        sp.set_option("writable", 1)
    st = O.Store(parts)
    st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    for p, pairs in kv.items():
        if pairs:
            sp.load_part(p, pairs)
            st.put(p, pairs)
    sp.finalize()
    st.finalize()
    return sp, st


@pytest.fixture(scope="module")
def branches():
    sp, st = load_both(kv_pairs(branch_edges()))
    yield sp, st
    sp.close()


@pytest.mark.parametrize("force", [1, -1])
@pytest.mark.parametrize("distinct", [True, False])
@pytest.mark.parametrize("starts", [[LAST], [FIRST], [LAST, FIRST, DEAD], [DEAD], [7, 8, 9, LAST]],
                         ids=["last", "first", "all", "dying", "fillers"])
def test_pull_branches(branches, starts, distinct, force):
    sp, st = branches
    assert sp.info(FOLLOW)["num_vertices"] == 212  # 3 words and 20 rows: not a multiple of 64
    with forced(sp, force):
        for steps in (1, 2, 3):
            got = check_go(sp, st, starts, steps, FOLLOW, distinct=distinct)
            hops = modes(sp)
            if force == -1:
                assert all(m != 6 for m, _, _ in hops)
            elif got.n_rows:
                check_pull_modes(hops, steps, distinct, 1)
            if starts == [DEAD]:
                assert got.n_rows == (2 if steps == 1 else 0)


def test_pull_drops_sources_without_in_edges_only_before_the_final_hop(branches):
    """a found row without in-edges adds nothing to the next hop's E and is not in its frontier (a
    dropped row yields no rows either way: what shows is the count and the final hop keeping it)"""
    sp, st = branches
    lonely = {u for u in range(202, 209) if u % 7 in DEGS}  # reach LAST, nobody reaches them
    assert lonely
    with forced(sp, 1):
        one = check_go(sp, st, [LAST], 1, FOLLOW, distinct=True)
        assert lonely <= set(one.columns[0].tolist())  # kept by the final hop
        sp.go([LAST], 2, FOLLOW, distinct=True, reversely=True)
        t = sp.last_timing()["hops"]
        assert t[0]["mode_id"] == 6 and not t[0]["final"]
        assert t[0]["c"][0] == one.n_rows  # found: every source of LAST, the lonely ones included
        # c[1], the kept rows' in-degree sum, is the second hop's E: with LAST's in-degree the oracle's count
        two = check_go(sp, st, [LAST], 2, FOLLOW, distinct=True)
        assert two.edges_scanned == one.edges_scanned + t[0]["c"][1]


@pytest.mark.parametrize("distinct", [False, True])
def test_pull_graph_upto(branches, distinct):
    sp, st = branches
    for starts in ([DEAD], [LAST, DEAD]):
        want = Counter()
        for k in (1, 2, 3):
            want.update(ms(st.go(starts, k, -FOLLOW, distinct=distinct).rows()))
        if distinct:
            want = Counter(set(want))
        with forced(sp, 1):
            got = sp.go(starts, 3, FOLLOW, distinct=distinct, upto=True, reversely=True)
        assert ms(got.rows()) == want and got.n_rows > 0, starts
    # plain GO 3 STEPS from DEAD is empty, UPTO 3 keeps the steps before the frontier died
    assert sp.go([DEAD], 3, FOLLOW, reversely=True).n_rows == 0
    assert ms(sp.go([DEAD], 3, FOLLOW, upto=True, reversely=True).rows()) == Counter({(DL1,): 1, (DL2,): 1})


# ------------------------------------------------------------------------------------------
# in keys that do not mirror the out keys: the reference reads in keys, the pull would read out keys
# ------------------------------------------------------------------------------------------
SMALL = [(1, 2), (2, 3), (3, 1), (1, 3), (4, 2), (5, 4), (6, 5), (3, 6), (7, 3), (2, 7)]


def broken_in_keys():
    ins = [(d, 0, s) for s, d in SMALL]
    ins.remove((7, 0, 2))   # an out key 2 -> 7 without its in key
    ins.append((5, 0, 1))   # an in key (5 <- 1) without its out key
    ins.remove((3, 0, 7))
    ins.append((3, 7, 7))   # a rank-7 in key whose out key has rank 0
    return ins


@pytest.mark.parametrize("repaired", [False, True])
def test_not_mirrored_runs_top_down(repaired):
    sp, st = load_both(kv_pairs(SMALL, in_keys=None if repaired else broken_in_keys()))
    try:
        for force in (None, 1):
            saw = []
            with forced(sp, force):
                for starts in ([3], [5], [7], [1, 2, 3, 4, 5, 6, 7]):
                    for steps in (1, 2, 3):
                        for distinct in (False, True):
                            check_go(sp, st, starts, steps, FOLLOW, distinct=distinct,
                                     yields=[X.EdgeSrc("follow"), X.EdgeDst("follow"), X.EdgeRank("follow")])
                            check_go(sp, st, starts, steps, FOLLOW, distinct=distinct)
                            saw += [m for m, _, _ in modes(sp)]
            if not repaired:
                assert 6 not in saw
            elif force == 1:
                assert 6 in saw
    finally:
        sp.close()


def test_writable_commit_resets_the_mirror():
    edges = SMALL
    kv = kv_pairs(edges)
    sp, st = load_both(kv, writable=True)
    try:
        with forced(sp, 1):
            check_go(sp, st, [3, 5], 2, FOLLOW, distinct=True)
            assert 6 in [m for m, _, _ in modes(sp)]  # mirrored: checked at this query, then pulled
            extra = [(O.edge_key(1, 5, -FOLLOW, 0, 1, VER), b"")]  # an in key (5 <- 1) without its out key
            sp.write_part(1, extra)
            sp.commit()
            st2 = O.Store(1)
            st2.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
            st2.put(1, kv[1] + extra)
            st2.finalize()
            for steps in (1, 2, 3):
                for distinct in (False, True):
                    got = check_go(sp, st2, [3, 5], steps, FOLLOW, distinct=distinct)
                    assert 6 not in [m for m, _, _ in modes(sp)]
            assert (1,) in ms(sp.go([5], 1, FOLLOW, reversely=True).rows())
            assert got.n_rows > 0
    finally:
        sp.close()
