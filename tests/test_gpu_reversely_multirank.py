"""GO ... REVERSELY sharded over in-process ranks on one GPU (nbg_comm_init_local, the Group pattern
of test_gpu_upto_multirank.py): the union of the ranks' rows equals the oracle's negative-type run,
each row is reported by its owner only, the ranks' edges_scanned sum to the one-rank figure, and
every rank takes the same direction: the pull hop (mode 6) on all of them under bu_force = 1 over
gen_rmat's mirrored keys, on none over a KV-loaded space, whose mirror state stays unknown.
"""
from collections import Counter
from concurrent.futures import ThreadPoolExecutor
import itertools

import numpy as np
import pytest

import oracle as O
from nebula_amd import GraphSpace
from nebula_amd import expr as X

pytestmark = pytest.mark.gpu

FOLLOW = 1
SEED = 1
PARTS = 64
_keys = itertools.count(7600)


class Group:
    """`world` contexts on device 0, one per rank; every call runs on all ranks in threads."""

    def __init__(self, world, parts=PARTS):
        key = next(_keys)
        self.world = world
        self.sp = [GraphSpace(parts, device=0, rank=r, world_size=world) for r in range(world)]
        for s in self.sp:
            s.comm_init_local(key)
        self.pool = ThreadPoolExecutor(max_workers=world)

    def each(self, fn):
        futs = [self.pool.submit(fn, r, s) for r, s in enumerate(self.sp)]
        out, err = [], None
        for f in futs:
            try:
                out.append(f.result(timeout=300))
            except Exception as e:  # collect, so every rank has finished before raising
                out.append(None)
                err = err or e
        if err:
            raise err
        return out

    def go(self, *a, **k):
        return self.each(lambda r, s: s.go(*a, **k))

    def close(self):
        for s in self.sp:
            s.close()
        self.pool.shutdown()


@pytest.fixture(scope="module")
def oracle12():
    st = O.Store(PARTS)
    st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    st.load_rmat(12, 16, SEED, FOLLOW)
    return st


@pytest.fixture(scope="module")
def one_rank():
    sp = GraphSpace(PARTS)
    sp.set_edge_schema(FOLLOW, [("weight", O.INT)])
    sp.gen_rmat(12, 16, SEED, FOLLOW)
    sp.finalize()
    yield sp
    sp.close()


@pytest.fixture(scope="module", params=[2, 3])
def rmat_group(request):
    g = Group(request.param)
    for s in g.sp:
        s.set_edge_schema(FOLLOW, [("weight", O.INT)])
    g.each(lambda r, s: s.gen_rmat(12, 16, SEED, FOLLOW))
    g.each(lambda r, s: s.finalize())
    yield g
    g.close()


def dst_seeds(n, seed=7):
    _, d, _ = O.rmat_edges(12, 16, SEED)
    return np.random.default_rng(seed).choice(np.unique(d), n, replace=False).astype(np.int64)


def gather(res):
    got = Counter()
    for x in res:
        got.update(tuple(r) for r in x.rows())
    return got


def run_forced(g, force, *a, **k):
    g.each(lambda r, s: s.set_option("bu_force", force))
    try:
        res = g.go(*a, **k)
        t = g.each(lambda r, s: [(h["mode_id"], h["final"]) for h in s.last_timing()["hops"]])
    finally:
        g.each(lambda r, s: s.set_option("bu_force", 0))
    return res, t


@pytest.mark.parametrize("force", [-1, 1])
@pytest.mark.parametrize("distinct", [False, True])
def test_sharded_reversely_rmat(rmat_group, oracle12, one_rank, distinct, force):
    g = rmat_group
    starts = dst_seeds(4)
    for steps in (1, 2, 3):
        ref = oracle12.go(starts, steps, -FOLLOW, distinct=distinct)
        want = Counter(tuple(r) for r in ref.rows())
        one = one_rank.go(starts, steps, FOLLOW, distinct=distinct, reversely=True)
        assert Counter(tuple(r) for r in one.rows()) == want and one.edges_scanned == ref.edges_scanned
        res, t = run_forced(g, force, starts, steps, FOLLOW, distinct=distinct, reversely=True)
        assert gather(res) == want, (steps, distinct, force, t)
        assert sum(x.edges_scanned for x in res) == one.edges_scanned, (steps, distinct, force, t)
        for hops in t:
            pulled = [m == 6 for m, final in hops if not final or distinct]
            if force == 1:
                assert all(pulled) and (pulled or (steps == 1 and not distinct)), (steps, t)  # mode 6 on every rank
            else:
                assert not any(m == 6 for m, _ in hops), (steps, t)


def test_sharded_reversely_rows_come_from_their_owner(rmat_group, oracle12):
    """sharding by owner: a row (v, u) of a reverse hop is reported by v's owner, as its in keys live there"""
    g = rmat_group
    starts = dst_seeds(8, 11)
    ys = [X.EdgeSrc("follow"), X.EdgeDst("follow")]
    want = Counter(tuple(r) for r in oracle12.go(starts, 2, -FOLLOW, yields=[y.encode() for y in ys]).rows())
    res = g.go(starts, 2, FOLLOW, yields=ys, reversely=True)
    assert gather(res) == want
    # every rank's rows have distinct srcs from every other rank's: one owner per frontier vertex
    srcs = [set(x.columns[0].tolist()) if x.n_rows else set() for x in res]
    for a, b in itertools.combinations(range(g.world), 2):
        assert not srcs[a] & srcs[b]
    # DISTINCT _dst: each vertex once over all ranks
    res, _ = run_forced(g, 1, starts, 2, FOLLOW, distinct=True, reversely=True)
    cols = np.concatenate([x.columns[0] for x in res])
    assert len(cols) == len(np.unique(cols)) > 0


def test_sharded_reversely_dying_frontier(rmat_group, oracle12):
    """starts whose every in-neighbour has no in-edge: the frontier dies at step 2 on all ranks"""
    g = rmat_group
    s, d, _ = O.rmat_edges(12, 16, SEED)
    roots = np.setdiff1d(s, d)                              # vertices without in-edges
    only_roots = np.setdiff1d(d, d[~np.isin(s, roots)])     # ... whose every in-edge starts at one
    assert len(only_roots) > 0
    starts = only_roots[:8].astype(np.int64)
    assert oracle12.go(starts, 1, -FOLLOW).nrows > 0 and oracle12.go(starts, 2, -FOLLOW).nrows == 0
    for force in (-1, 1):
        for distinct in (False, True):
            for steps in (2, 3):
                res, _ = run_forced(g, force, starts, steps, FOLLOW, distinct=distinct, reversely=True)
                assert sum(x.n_rows for x in res) == 0


def test_sharded_kv_loaded_space_runs_top_down(oracle12):
    """a KV-loaded sharded space keeps its mirror state unknown: bu_force = 1 still runs top-down"""
    world = 2
    g = Group(world)
    try:
        for sp in g.sp:
            sp.set_edge_schema(FOLLOW, [("weight", O.INT)])

        def load(r, sp):
            for p in range(1, PARTS + 1):
                if p % world == r:  # the part's owner rank
                    sp.load_part(p, oracle12.dump_part(p))

        g.each(load)
        g.each(lambda r, sp: sp.finalize())
        starts = dst_seeds(4)
        for distinct in (False, True):
            for steps in (1, 2, 3):
                ref = oracle12.go(starts, steps, -FOLLOW, distinct=distinct)
                res, t = run_forced(g, 1, starts, steps, FOLLOW, distinct=distinct, reversely=True)
                assert gather(res) == Counter(tuple(r) for r in ref.rows()), (steps, distinct)
                assert sum(x.edges_scanned for x in res) == ref.edges_scanned
                assert all(m != 6 for hops in t for m, _ in hops), t
    finally:
        g.close()
