"""FIND over 2 and 3 in-process ranks on one GPU (nbg_comm_init_local, the Group helper of
test_gpu_upto_multirank.py): every rank scans what it owns and emits those rows, no collective is
issued; the ranks' rows together are the one-rank result as a multiset, and every row a rank emits is
a row it owns (the source's / the vid's part owner)."""
from collections import Counter

import numpy as np
import pytest

import oracle as O
from nebula_amd import GraphSpace
from nebula_amd import expr as X
from test_gpu_find_edges import FIELDS, PI, PJ, PS, REL, Writer, got, mix, props_of, set_mode
from test_gpu_upto_multirank import Group

pytestmark = pytest.mark.gpu

FOLLOW = 1
WEIGHT = X.AliasProp("follow", "weight")
PARTS = 4
PERSON = 5
PAGE, PNAME = X.AliasProp("person", "age"), X.AliasProp("person", "name")


@pytest.fixture(scope="module")
def one_rmat():
    sp = GraphSpace(64)
    sp.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
    sp.gen_rmat(12, 16, 1, FOLLOW)
    sp.finalize()
    yield sp
    sp.close()


@pytest.mark.parametrize("world", [2, 3])
def test_rmat(one_rmat, world):
    g = Group(world)
    try:
        for s in g.sp:
            s.set_edge_schema(FOLLOW, [("weight", O.INT)], name="follow")
        g.each(lambda r, s: s.gen_rmat(12, 16, 1, FOLLOW))
        g.each(lambda r, s: s.finalize())
        for where in (WEIGHT > 499, WEIGHT.eq(499), WEIGHT * 2 > 1978, None):
            whole = Counter(got(one_rmat.find_edges(FOLLOW, where, [WEIGHT])))
            per_mode = []
            for m in (0, 1, None):
                def run(r, sp):
                    set_mode(sp, m)
                    rs = sp.find_edges(FOLLOW, where, [WEIGHT])
                    return got(rs), sp.last_timing()["comm_calls"]
                res = g.each(run)
                per_mode.append([x[0] for x in res])
                assert all(x[1] == 0 for x in res)
            assert per_mode[0] == per_mode[1] == per_mode[2]
            rows = per_mode[0]
            assert sum((Counter(x) for x in rows), Counter()) == whole and len(whole) > 0
            for r, x in enumerate(rows):
                assert x and all(O.part_of(row[0], 64) % world == r for row in x)
    finally:
        g.close()


@pytest.mark.parametrize("world", [2, 3])
def test_hand_built(world):
    w = Writer(PARTS)
    j = 0
    for src, deg in ((1, 3), (2, 70), (3, 17), (4, 1), (6, 90), (7, 5), (9, 2100)):
        for _ in range(deg):
            j += 1
            w.edge(src, mix(j) if j % 4 else 1 + j % 7, j % 3 if src == 7 else 0, 9, props_of(src, j))
    edges = w.edges()
    tag_rows = {v: (f"n{v}", v * 3) for v in (1, 2, 3, 6, 50, 51, 52, 53, 54, 55)}  # 50..55: vertices without edges
    for v, row in tag_rows.items():
        p = O.part_of(v, PARTS)
        w.parts[p].append((O.vertex_key(p, v, PERSON, 0), O.encode_row(list(row))))

    def setup(sp):
        sp.set_edge_schema(REL, FIELDS, name="rel")
        sp.set_tag_schema(PERSON, "person", [("name", O.STRING), ("age", O.INT)])

    queries = [(PI > 6000, [PI, PS]), (PJ < 0, [PJ]), (PS.eq(""), [PI]), (None, [])]

    def run(sp):
        out = []
        for m in (0, 1, None):
            set_mode(sp, m)
            out.append([got(sp.find_edges(REL, wh, ys)) for wh, ys in queries])
        assert out[0] == out[1] == out[2]
        v = [got(sp.find_vertices(PERSON, wh, [PNAME, PAGE])) for wh in (PAGE > 5, None, PNAME.eq("n52"))]
        return out[0], v

    one = GraphSpace(PARTS)
    g = Group(world, parts=PARTS)
    try:
        setup(one)
        w.load(one)
        one.finalize()
        one_e, one_v = run(one)
        assert len(one_e[3]) == len(edges) and len(one_v[1]) == len(tag_rows)

        def load(r, sp):
            setup(sp)
            for p, kv in w.parts.items():
                if kv and p % world == r:
                    sp.load_part(p, kv)
            sp.finalize()

        g.each(load)
        res = g.each(lambda r, sp: run(sp))
        for which in (0, 1):
            for q in range(len(one_e) if which == 0 else len(one_v)):
                whole = (one_e, one_v)[which][q]
                per_rank = [x[which][q] for x in res]
                assert sum((Counter(x) for x in per_rank), Counter()) == Counter(whole)
                for r, rows in enumerate(per_rank):
                    assert all(O.part_of(row[0], PARTS) % world == r for row in rows)
        assert all(x[0][3] for x in res) and all(x[1][1] for x in res), "every rank owns some rows"
    finally:
        g.close()
        one.close()
