#!/usr/bin/env python3
"""FETCH PROP ON edge keys / vertex keys on the device against the only way to answer the same
question without the call (GPU box only).

Edges: RMAT --scale, 2^--log2-keys (src, dst) keys taken from a GO 2 STEPS ... YIELD _src, _dst
result, kept in HBM; once in the order the GO produced them and once shuffled; fetching
follow.weight.  For each of the three lookup modes (engine option fetch_search: 0 scan, 1 search,
unset hybrid), after a warm-up, from nbg_last_timing: the call's HIP-event total_ms, the lookup
kernel alone (expand_ms), launches, host waits, and the kernel's algorithmic bytes (DESIGN.md
section 3b, expand_bytes) per second against the 8 TB/s HBM peak.  The baseline is what a caller
does without nbg_fetch_edges: get_bound over the distinct srcs returning _dst and weight, joined to
the keys on the host (host clock, first call to joined weights).

Vertices: a ring of --ring vertices carrying tag person(age); 2^--log2-keys vids drawn from it and
from --ring more vids that have a row but no edge; nbg_fetch_vertices of person.age against the
closest equivalent, GO 1 STEPS from each key's ring predecessor YIELD $$.person.age (which cannot
reach the vertices without edges: it runs over the ring half of the keys only).

Nothing is gated on the figures; nothing is retried.  Prints one JSON line and appends a table to
--md (default profiles/fetch.md).

    python3 tools/fetch_compare.py --scale 20
"""
import argparse
import json
import statistics
import struct
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK_BPS = 8e12
MODES = [("scan", 0), ("search", 1), ("hybrid", None)]  # + ("hybrid, threshold T", None) per --thresholds
T_INT, T_VID = 2, 3


def med(v):
    return round(statistics.median(v), 4) if v else None


def set_mode(sp, m):
    if m is None:
        sp.unset_option("fetch_search")
    else:
        sp.set_option("fetch_search", m)


def pair_hash(a, b):
    with np.errstate(over="ignore"):
        return (a.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (b.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))


def edge_side(args, X, GraphSpace, synth):
    sp = GraphSpace(64)
    sp.set_edge_schema(1, [("weight", T_INT)], name="follow")
    sp.gen_rmat(args.scale, 16, 1, 1)
    sp.finalize()
    n = 1 << args.log2_keys
    w = X.AliasProp("follow", "weight")
    for steps in (2, 3):  # (a small scale needs the third step to give that many rows)
        go = sp.go(synth.seeds(args.scale, 16, 1, 64), steps, 1,
                   yields=[X.AliasProp("follow", "_src"), X.AliasProp("follow", "_dst"), w])
        if go.n_rows >= n:
            break
    if go.n_rows < n:
        raise SystemExit(f"fetch_compare: the GO gave {go.n_rows} rows, fewer than {n} keys")
    ks, kd, kw = (np.ascontiguousarray(c[:n]) for c in go.columns)
    perm = np.random.default_rng(5).permutation(n)
    # a third key set: every edge of up to 65536 of the GO's srcs whose rows have at most 16 entries
    # (one scan step), tiled to n keys and shuffled
    us = np.random.default_rng(6).permutation(np.unique(go.columns[0]))[:65536]
    parts = (us.astype(np.uint64) % np.uint64(64) + np.uint64(1)).astype(np.int32)
    b = sp.get_bound(1, parts, us, [("_dst", 3, 0), ("weight", 3, 0)])
    deg = np.diff(b.vertex_row_offsets)
    rows = np.flatnonzero(np.repeat(deg, deg) <= 16)
    sets = [("as produced", (ks, kd, kw)), ("shuffled", (ks[perm], kd[perm], kw[perm]))]
    if len(rows):
        rows = np.resize(rows, n)[perm]
        sets.append(("rows of <= 16 entries only", (np.repeat(b.vertex_ids, deg)[rows], b.columns[0][rows], b.columns[1][rows])))
    out = []
    for order, (s, d, want) in sets:
        keys = sp.order_by([(T_VID, s), (T_VID, d)], [], keep_on_device=True)  # the keys in HBM
        for name, m, thr in [(a, b, None) for a, b in MODES] + [(f"hybrid, threshold {t}", None, t) for t in args.thresholds]:
            set_mode(sp, m)
            if thr is None:
                sp.unset_option("fetch_threshold")
            else:
                sp.set_option("fetch_threshold", thr)
            tot, ker = [], []
            t = None
            # (the forced scan serialises a wave on a hub row: fewer rounds of it)
            warm, rounds = (1, min(3, args.rounds)) if m == 0 else (args.warmup, args.rounds)
            for i in range(warm + rounds):
                rs = sp.fetch_edges(1, (keys, 0), (keys, 1), None, [w])
                t = sp.last_timing()
                if i >= warm:
                    tot.append(t["total_ms"]), ker.append(t["expand_ms"])
            if rs.n_rows != n or not np.array_equal(rs.columns[0], want):
                raise SystemExit(f"fetch_compare: {order} {name}: the fetched weights differ from the GO's")
            km = med(ker)
            out.append({"keys": n, "order": order, "mode": name, "total_ms": med(tot), "lookup_ms": km,
                        "launches": int(t["launches"]), "host_waits": int(t["host_waits"]),
                        "entries_read": int(t["edges_scanned"]), "model_bytes": int(t["expand_bytes"]),
                        "lookup_bytes_per_s": round(t["expand_bytes"] / (km * 1e-3)) if km else None,
                        "fraction_of_hbm_peak": round(t["expand_bytes"] / (km * 1e-3) / HBM_PEAK_BPS, 4) if km else None})
        set_mode(sp, None)
        sp.unset_option("fetch_threshold")
        # the parent's way: get_bound over the distinct srcs, joined on the host
        base = []
        for i in range(1 + args.base_rounds):
            t0 = time.perf_counter()
            us = np.unique(s)
            parts = (us.astype(np.uint64) % np.uint64(64) + np.uint64(1)).astype(np.int32)
            b = sp.get_bound(1, parts, us, [("_dst", 3, 0), ("weight", 3, 0)])
            bsrc = np.repeat(b.vertex_ids, np.diff(b.vertex_row_offsets))
            # a sort-merge join in numpy on a 64-bit mix of (src, dst) (checked against the GO below)
            hb, hk = pair_hash(bsrc, b.columns[0]), pair_hash(s, d)
            o = np.argsort(hb)
            joined = b.columns[1][o[np.searchsorted(hb[o], hk)]]
            if i:
                base.append((time.perf_counter() - t0) * 1e3)
        if not np.array_equal(joined, want):
            raise SystemExit("fetch_compare: the get_bound join differs from the GO's weights")
        out.append({"keys": n, "order": order, "mode": "get_bound + host join", "total_ms": med(base),
                    "distinct_srcs": int(len(us)), "bound_rows": int(b.n_rows)})
    sp.close()
    return out


def vertex_side(args, X, GraphSpace):
    ring, n = args.ring, 1 << args.log2_keys
    ekey, vkey = struct.Struct("<iqiqqq"), struct.Struct("<iqiq")
    sp = GraphSpace(1)
    sp.set_edge_schema(1, [("weight", T_INT)], name="next")
    sp.set_tag_schema(5, "person", [("age", T_INT)])
    kv = []
    for v in range(ring):
        nxt = (v + 1) % ring
        kv.append((ekey.pack(1, v, 1, 0, nxt, 0), bytes([0, v % 100])))
        kv.append((ekey.pack(1, nxt, -1, 0, v, 0), b""))
    for v in range(2 * ring):  # the upper half: rows of vertices without edges
        kv.append((vkey.pack(1, v, 5, 0), bytes([0, v % 90])))
    sp.load_part(1, kv)
    sp.finalize()
    rng = np.random.default_rng(9)
    age = X.AliasProp("person", "age")
    out = []
    for name, hi in (("ring vids", ring), ("ring + edge-less vids", 2 * ring)):
        vids = rng.integers(0, hi, n).astype(np.int64)
        keys = sp.order_by([(T_VID, vids)], [], keep_on_device=True)
        tot, t = [], None
        for i in range(args.warmup + args.rounds):
            rs = sp.fetch_vertices(5, (keys, 0), [age])
            t = sp.last_timing()
            if i >= args.warmup:
                tot.append(t["total_ms"])
        if not np.array_equal(rs.columns[0], vids % 90):
            raise SystemExit("fetch_compare: fetched ages differ")
        row = {"keys": n, "vids": name, "fetch_total_ms": med(tot), "launches": int(t["launches"]),
               "host_waits": int(t["host_waits"])}
        if hi == ring:
            starts = np.ascontiguousarray((vids - 1) % ring)
            gt = []
            for i in range(args.warmup + args.rounds):
                g = sp.go(starts, 1, 1, yields=[X.DestProp("person", "age")])
                if i >= args.warmup:
                    gt.append(sp.last_timing()["total_ms"])
            if not np.array_equal(np.sort(g.columns[0]), np.sort(vids % 90)):
                raise SystemExit("fetch_compare: the GO's ages differ")
            row["go_dst_props_total_ms"] = med(gt)
        out.append(row)
    sp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--log2-keys", type=int, default=20)
    ap.add_argument("--ring", type=int, default=4096)
    ap.add_argument("--thresholds", type=int, nargs="*", default=[], help="further hybrid thresholds to time")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--base-rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=str(ROOT / "profiles" / "fetch.md"))
    args = ap.parse_args()
    from nebula_amd import GraphSpace, synth
    from nebula_amd import expr as X
    res = {"scale": args.scale, "edges": edge_side(args, X, GraphSpace, synth), "vertices": vertex_side(args, X, GraphSpace)}
    print(json.dumps(res))
    if args.md:
        lines = [f"## RMAT-{args.scale}, 2^{args.log2_keys} keys (medians of {args.rounds} rounds after {args.warmup} warm-ups)", "",
                 "| keys | mode | total ms | lookup kernel ms | launches | host waits | entries read | model bytes | "
                 "lookup B/s | of 8 TB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in res["edges"]:
            lines.append(f"| {r['order']} | {r['mode']} | {r['total_ms']} | {r.get('lookup_ms', '')} | {r.get('launches', '')} | "
                         f"{r.get('host_waits', '')} | {r.get('entries_read', '')} | {r.get('model_bytes', '')} | "
                         f"{r.get('lookup_bytes_per_s', '')} | {r.get('fraction_of_hbm_peak', '')} |")
        lines += ["", "| vertex keys | fetch_vertices total ms | GO $$ props total ms | launches | host waits |", "|---|---|---|---|---|"]
        for r in res["vertices"]:
            lines.append(f"| {r['vids']} | {r['fetch_total_ms']} | {r.get('go_dst_props_total_ms', '')} | {r['launches']} | "
                         f"{r['host_waits']} |")
        lines.append("")
        p = Path(args.md)
        p.parent.mkdir(parents=True, exist_ok=True)
        with p.open("a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
