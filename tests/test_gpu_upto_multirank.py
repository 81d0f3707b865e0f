"""GO UPTO N STEPS sharded over in-process ranks on one GPU (nbg_comm_init_local, as
test_gpu_multirank.py): the union of the ranks' results equals the concatenation of the oracle's
GO k STEPS results, each vertex or row reported by its owner only, and the ranks' edges_scanned
sum to the one-rank figure.  Every rank branches on counts summed over ranks, so a frontier that
dies ends the query on all of them.
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
_keys = itertools.count(7000)
WEIGHT = X.AliasProp("follow", "weight")
DST = X.EdgeDst("follow")


class Group:
    """`world` contexts on device 0, one per rank; every call runs on all ranks in threads."""

    def __init__(self, world, parts=64):
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
    st = O.Store(64)
    st.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    st.load_rmat(12, 16, SEED, FOLLOW)
    return st


@pytest.fixture(scope="module")
def one_rank():
    sp = GraphSpace(64)
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


def seeds(n, seed=7):
    s, _, _ = O.rmat_edges(12, 16, SEED)
    return np.random.default_rng(seed).choice(np.unique(s), n, replace=False).astype(np.int64)


@pytest.mark.parametrize("force", [0, 1, -1])
def test_sharded_upto_distinct_dst(rmat_group, oracle12, one_rank, force):
    g = rmat_group
    starts = seeds(64)
    w = WEIGHT > 499
    want = np.unique(np.concatenate([
        oracle12.go(starts, k, FOLLOW, where=w.encode(), yields=[DST.encode()], distinct=True).int_col(0)
        for k in (1, 2, 3)]))
    one = one_rank.go(starts, 3, FOLLOW, where=w, yields=[DST], distinct=True, upto=True)
    assert np.array_equal(np.sort(one.columns[0]), want)
    g.each(lambda r, s: s.set_option("bu_force", force))
    try:
        res = g.go(starts, 3, FOLLOW, where=w, yields=[DST], distinct=True, upto=True)
        t = g.each(lambda r, s: s.last_timing())
    finally:
        g.each(lambda r, s: s.set_option("bu_force", 0))
    got = np.sort(np.concatenate([x.columns[0] for x in res]))
    assert np.array_equal(got, want)  # (sorted and unique: each vertex reported by its owner only)
    assert sum(x.edges_scanned for x in res) == one.edges_scanned
    for x in t:
        hop_kernels = [k for h in x["hops"] if not h["final"] for k in h["kernels"]]
        if force == 1:
            assert "nbg::k_upto_bu" in hop_kernels
        if force == -1:
            assert "nbg::k_upto_claim" in hop_kernels and x["bu_steps"] == 0


def test_sharded_upto_plain_rows(rmat_group, oracle12, one_rank):
    g = rmat_group
    s, _, _ = O.rmat_edges(12, 16, SEED)
    starts = [int(x) for x in s[np.random.default_rng(5).integers(0, len(s), 24)]]  # duplicates allowed
    want = Counter()
    for k in (1, 2):
        want.update(tuple(r) for r in oracle12.go(starts, k, FOLLOW).rows())
    one = one_rank.go(starts, 2, FOLLOW, upto=True)
    res = g.go(starts, 2, FOLLOW, upto=True)
    got = Counter()
    for x in res:
        got.update(tuple(r) for r in x.rows())
    assert got == want
    assert sum(x.edges_scanned for x in res) == one.edges_scanned == sum(want.values())


def test_sharded_upto_dying_frontier(rmat_group, oracle12):
    """a start set whose frontier dies at step 2: every rank returns, with the step-1 rows"""
    g = rmat_group
    s, d, _ = O.rmat_edges(12, 16, SEED)
    sinks = np.setdiff1d(d, s)                                  # vertices without out-edges
    only_sinks = np.setdiff1d(s, s[~np.isin(d, sinks)])         # ... whose every out-edge ends in one
    assert len(only_sinks) > 0
    starts = only_sinks[:8].astype(np.int64)
    assert oracle12.go(starts, 2, FOLLOW).nrows == 0
    for distinct in (False, True):
        want = Counter(tuple(r) for r in oracle12.go(starts, 1, FOLLOW, distinct=distinct).rows())
        assert sum(want.values()) > 0
        res = g.go(starts, 4, FOLLOW, distinct=distinct, upto=True)
        got = Counter()
        for x in res:
            got.update(tuple(r) for r in x.rows())
        assert got == want
