"""GO UPTO N STEPS on one rank (include/nebula_amd.h, DESIGN.md divergence 7): the rows of
GO 1 STEPS .. GO N STEPS together.  The expected result is always built from unchanged oracle
GO k STEPS calls; rows are compared as multisets (sets under DISTINCT) or sorted columns.

DISTINCT runs as a visited-pruned BFS (k_upto_claim behind a top-down hop, k_upto_bu bottom-up)
and one final step over the union of the levels, so its edges_scanned is
sum_{k<N} outdeg(B_k) + outdeg(U), recomputed here in numpy from the generator's edge list.
"""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import oracle as O
from nebula_amd import GraphSpace, NbgError, _lib
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

FOLLOW = 1
SEED = 1
WEIGHT = X.AliasProp("follow", "weight")
DST = X.EdgeDst("follow")


def ms(rows):
    return Counter(tuple(r) for r in rows)


# ------------------------------------------------------------------------------------------
# DISTINCT _dst on RMAT-12 / RMAT-16 against the index-space oracle
# ------------------------------------------------------------------------------------------
class Rmat:
    """the engine's snapshot, the index-space oracle and the collapsed edge list of one scale"""

    def __init__(self, scale):
        self.sp = GraphSpace(64)
        self.sp.set_edge_schema(FOLLOW, [("weight", O.INT)])
        self.sp.gen_rmat(scale, 16, SEED, FOLLOW)
        self.sp.finalize()
        self.g = O.RmatGraph(scale, 16, SEED)
        s, d, _ = O.rmat_edges(scale, 16, SEED)
        self.src_vids = s
        pairs = np.unique(np.stack([s, d], axis=1), axis=0)  # duplicate (src, dst) collapse (P3 / P4)
        self.vids = np.unique(pairs)
        self.si = np.searchsorted(self.vids, pairs[:, 0])
        self.di = np.searchsorted(self.vids, pairs[:, 1])
        self.deg = np.bincount(self.si, minlength=len(self.vids))
        self._want = {}

    def seeds(self, n, seed):
        """n distinct vertices with out-edges"""
        rng = np.random.default_rng(seed)
        return rng.choice(np.unique(self.src_vids), n, replace=False).astype(np.int64)

    def want(self, key, starts, k, gt):
        """sorted GO k STEPS DISTINCT _dst of the oracle (computed once per case, never changed)"""
        ck = (key, k, gt)
        if ck not in self._want:
            self._want[ck] = self.g.go(starts, k, where_gt=gt, distinct=True)[0]
        return self._want[ck]

    def levels_and_scanned(self, starts, n_steps):
        """BFS level sizes and sum_{k<N} outdeg(B_k) + outdeg(U)"""
        n = len(self.vids)
        st = np.unique(starts)
        st = st[np.isin(st, self.vids)]
        B = np.searchsorted(self.vids, st)
        seen = np.zeros(n, bool)
        seen[B] = True
        total, levels = 0, [len(B)]
        for _ in range(1, n_steps):
            total += int(self.deg[B].sum())
            front = np.zeros(n, bool)
            front[B] = True
            reached = np.unique(self.di[front[self.si]])
            B = reached[~seen[reached]]
            seen[B] = True
            levels.append(len(B))
        return levels, total + int(self.deg[seen].sum())


@pytest.fixture(scope="module")
def rmat12():
    r = Rmat(12)
    yield r
    r.sp.close()


@pytest.fixture(scope="module")
def rmat16():
    r = Rmat(16)
    yield r
    r.sp.close()


def check_distinct_dst(r, key, starts, force):
    sp = r.sp
    assert sp.info(FOLLOW)["num_vertices"] % 128 != 0  # the last tile and bitmap word are partial
    sp.set_option("bu_force", force)
    try:
        for gt in (None, 499, 998):
            w = None if gt is None else WEIGHT > gt
            for n in (1, 2, 3, 4):
                got = sp.go(starts, n, FOLLOW, where=w, yields=[DST], distinct=True, upto=True)
                t = sp.last_timing()
                want = np.unique(np.concatenate([r.want(key, starts, k, gt) for k in range(1, n + 1)]))
                diag = (gt, n, force, [(h["mode"], h["final"], h["kernels"], h["c"][:4]) for h in t["hops"]])
                assert np.array_equal(np.sort(got.columns[0]), want), diag
                levels, scanned = r.levels_and_scanned(starts, n)
                assert got.edges_scanned == scanned, diag + (levels,)
                hop_kernels = [k for h in t["hops"] if not h["final"] for k in h["kernels"]]
                if n >= 2 and force == 1:
                    assert "nbg::k_upto_bu" in hop_kernels, diag
                if n >= 2 and force == -1:
                    assert "nbg::k_upto_claim" in hop_kernels and t["bu_steps"] == 0, diag
    finally:
        sp.set_option("bu_force", 0)


@pytest.mark.parametrize("force", [0, 1, -1])
@pytest.mark.parametrize("nseeds", [64, 4])
def test_upto_distinct_dst_rmat12(rmat12, nseeds, force):
    starts = rmat12.seeds(nseeds, 11)
    levels, _ = rmat12.levels_and_scanned(starts, 4)
    assert all(x > 0 for x in levels), levels  # every N <= 4 has work
    check_distinct_dst(rmat12, nseeds, starts, force)


@pytest.mark.parametrize("force", [0, 1, -1])
def test_upto_distinct_dst_rmat16(rmat16, force):
    check_distinct_dst(rmat16, 16, rmat16.seeds(16, 5), force)


# ------------------------------------------------------------------------------------------
# general YIELD lists, DISTINCT and not, against the faithful KV-store oracle
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store12():
    st = O.Store(64)
    st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    st.load_rmat(12, 16, SEED, FOLLOW)
    return st


def oracle_upto(st, starts, n, et, where=None, yields=(), distinct=False):
    """the rows of GO 1 .. n STEPS concatenated (a set under DISTINCT) and the no-WHERE row count"""
    rows = Counter()
    for k in range(1, n + 1):
        r = st.go(starts, k, et, where=X.encode(where), yields=[y.encode() for y in yields], distinct=distinct)
        rows.update(tuple(x) for x in r.rows())
    return rows


@pytest.mark.parametrize("force", [1, -1])
@pytest.mark.parametrize("n", [2, 3])
def test_upto_general_yields_rmat12(rmat12, store12, n, force):
    sp, st = rmat12.sp, store12
    rng = np.random.default_rng(3)
    starts = [int(x) for x in rmat12.src_vids[rng.integers(0, len(rmat12.src_vids), 24)]]
    w = (WEIGHT % 3).eq(1) & (X.EdgeSrc("follow") > 0)
    ys = [X.EdgeSrc("follow"), DST, WEIGHT * 2]
    plain = sum(st.go(starts, k, FOLLOW).nrows for k in range(1, n + 1))  # no WHERE: every entry is a row
    sp.set_option("bu_force", force)
    try:
        for where, yields in ((w, ys), (None, ()), (w, ())):
            want = oracle_upto(st, starts, n, FOLLOW, where, yields)
            got = sp.go(starts, n, FOLLOW, where=where, yields=yields, upto=True)
            t = sp.last_timing()
            assert ms(got.rows()) == want, (n, force, where is not None, len(yields))
            assert got.edges_scanned == plain
            assert len(t["hops"]) <= 2 * n
            got = sp.go(starts, n, FOLLOW, where=where, yields=yields, distinct=True, upto=True)
            assert ms(got.rows()) == Counter(set(want)), (n, force, where is not None, len(yields))
    finally:
        sp.set_option("bu_force", 0)


# ------------------------------------------------------------------------------------------
# a hand-built KV graph: cycles, sinks, starts without in-edges, unknown vids
# ------------------------------------------------------------------------------------------
PARTS = 4
A, B, Cc, D, Z, E, F, G, H, I, J, K = range(101, 113)
UNKNOWN = 999
EDGES = [(A, B, 10), (B, Cc, 20), (Cc, A, 30), (A, Cc, 40),  # a -> b -> c -> a and a -> c
         (Z, D, 50), (B, D, 60),                              # d is a sink; z has no in-edge
         (E, F, 70), (F, G, 80), (G, H, 90), (H, E, 100),     # a second cycle
         (I, J, 110), (J, K, 120)]                            # a chain that dies at step 3


@pytest.fixture(scope="module")
def small():
    parts = {p: [] for p in range(1, PARTS + 1)}
    for s, d, w in EDGES:
        ps, pd = O.part_of(s, PARTS), O.part_of(d, PARTS)
        parts[ps].append((O.edge_key(ps, s, FOLLOW, 0, d, 2**63 - 2), O.encode_row([w])))
        parts[pd].append((O.edge_key(pd, d, -FOLLOW, 0, s, 2**63 - 2), b""))
    sp = GraphSpace(PARTS)
    sp.set_edge_schema(FOLLOW, [("weight", O.INT)])
    st = O.Store(PARTS)
    st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    for p, kv in parts.items():
        if kv:
            sp.load_part(p, kv)
            st.put(p, kv)
    sp.finalize()
    st.finalize()
    yield sp, st
    sp.close()


SMALL_YIELDS = [X.EdgeSrc("follow"), DST, WEIGHT]


@pytest.mark.parametrize("force", [0, 1, -1])
@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("starts", [[A], [Z], [D], [UNKNOWN], [I], [A, A, Z], [A, Z, D, UNKNOWN, E, I], []],
                         ids=["cycle", "no-in-edge", "sink", "unknown", "dying", "dups", "all", "empty"])
def test_upto_small_graph(small, starts, distinct, force):
    sp, st = small
    sp.set_option("bu_force", force)
    try:
        for n in (1, 2, 3, 4):
            for yields in ((), SMALL_YIELDS):
                want = oracle_upto(st, starts, n, FOLLOW, None, yields, distinct)
                if distinct:
                    want = Counter(set(want))
                got = sp.go(starts, n, FOLLOW, yields=yields, distinct=distinct, upto=True)
                assert ms(got.rows()) == want, (starts, n, distinct, force, len(yields))
    finally:
        sp.set_option("bu_force", 0)


def test_upto_keeps_rows_of_a_dead_frontier(small):
    """UPTO 3 from z returns z's step-1 row although plain GO 3 STEPS is empty"""
    sp, _ = small
    assert sp.go([Z], 3, FOLLOW).n_rows == 0
    assert ms(sp.go([Z], 3, FOLLOW, upto=True).rows()) == Counter({(D,): 1})
    assert ms(sp.go([I], 4, FOLLOW, distinct=True, upto=True).rows()) == Counter({(J,): 1, (K,): 1})


def test_upto_duplicate_starts_double_step1_rows(small):
    sp, _ = small
    one = ms(sp.go([A, A], 1, FOLLOW).rows())
    assert one == Counter({(B,): 2, (Cc,): 2})
    got = ms(sp.go([A, A], 2, FOLLOW, upto=True).rows())
    assert got == one + ms(sp.go([A, A], 2, FOLLOW).rows())


def test_upto_one_step_is_go_one_step(small):
    sp, _ = small
    for distinct in (False, True):
        a = sp.go([A, B, Z], 1, FOLLOW, yields=SMALL_YIELDS, distinct=distinct, upto=True)
        b = sp.go([A, B, Z], 1, FOLLOW, yields=SMALL_YIELDS, distinct=distinct)
        assert ms(a.rows()) == ms(b.rows()) and a.edges_scanned == b.edges_scanned


# ------------------------------------------------------------------------------------------
# errors, the repeated-call cache, keep_on_device
# ------------------------------------------------------------------------------------------
def test_upto_rejects_input_props(small):
    sp, _ = small
    with pytest.raises(NbgError) as e:
        sp.go([A, Z], 2, FOLLOW, yields=[X.InputProp("n"), DST], inputs=[("n", O.INT, [1, 2])], upto=True)
    assert e.value.code == -1003  # NBG_E_UNSUPPORTED
    assert "UPTO" in str(e.value)
    # piped starts without input properties work
    got = sp.go([A, Z], 2, FOLLOW, inputs=[("n", O.INT, [1, 2])], upto=True)
    assert ms(got.rows()) == ms(sp.go([A, Z], 1, FOLLOW).rows()) + ms(sp.go([A, Z], 2, FOLLOW).rows())


@pytest.mark.parametrize("distinct", [False, True])
def test_upto_eval_error_fails_the_query(small, distinct):
    sp, _ = small
    bad = WEIGHT / 0 > 1  # division by zero -> E_EVAL on some row
    with pytest.raises(NbgError) as e:
        sp.go([A], 3, FOLLOW, where=bad, distinct=distinct, upto=True)
    assert e.value.code == -1004  # NBG_E_EVAL
    assert sp.go([A], 2, FOLLOW, upto=True).n_rows == 5  # the context still answers


def test_upto_invalid_flag(small):
    sp, _ = small
    starts = np.asarray([A], dtype=np.int64)
    sp.go(starts, 2, FOLLOW, upto=True)
    spec = sp._last_spec[1]
    spec.upto = 2
    rows = _lib.Rows()
    try:
        assert sp.L.nbg_go(sp.h, C.byref(spec), C.byref(rows)) == -1001  # NBG_E_INVALID_ARG
    finally:
        sp._last_spec = None


def test_upto_not_confused_by_the_call_cache(rmat12, store12):
    sp, st = rmat12.sp, store12
    starts = rmat12.seeds(8, 21)
    w = WEIGHT > 499
    want_upto = np.unique(np.concatenate([rmat12.want("cache", starts, k, 499) for k in (1, 2, 3)]))
    want_go = rmat12.want("cache", starts, 3, 499)
    for upto, want in ((True, want_upto), (False, want_go), (True, want_upto)):
        got = sp.go(starts, 3, FOLLOW, where=w, yields=[DST], distinct=True, upto=upto)  # the same array object
        assert np.array_equal(np.sort(got.columns[0]), want), upto


def device_column(sp):
    """the query sp.go(keep_on_device=True) just ran, issued again from its prepared spec with the
    rows held: the first column copied from the device"""
    rows = _lib.Rows()
    sp._check(sp.L.nbg_go(sp.h, C.byref(sp._last_spec[1]), C.byref(rows)))
    try:
        assert rows.on_device == 1 and rows.n_cols == 1
        copy = sp.L.hipMemcpy
        copy.restype, copy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        col = np.empty(int(rows.n_rows), dtype=np.int64)
        if rows.n_rows:
            assert copy(col.ctypes.data, rows.cols[0], col.nbytes, 2) == 0  # 2: hipMemcpyDeviceToHost
        return col, int(rows.edges_scanned)
    finally:
        sp.L.nbg_rows_free(C.byref(rows))


@pytest.mark.parametrize("distinct", [True, False])
def test_upto_keep_on_device(rmat12, distinct):
    sp = rmat12.sp
    starts = rmat12.seeds(8, 31)
    w = WEIGHT > 499
    host = sp.go(starts, 3, FOLLOW, where=w, yields=[DST], distinct=distinct, upto=True)
    dev = sp.go(starts, 3, FOLLOW, where=w, yields=[DST], distinct=distinct, keep_on_device=True, upto=True)
    assert dev.on_device and dev.n_rows == host.n_rows and len(dev.device_ptrs) == 1
    col, scanned = device_column(sp)
    assert np.array_equal(np.sort(col), np.sort(host.columns[0])) and scanned == host.edges_scanned
