#!/usr/bin/env python3
"""GO N STEPS ... REVERSELY YIELD DISTINCT e._dst on the bench's RMAT graph and start rule: the pull
hop (nbg::k_rev_pull) against the top-down form, hop by hop (REVERSELY).

    python tools/rev_compare.py --scale 26 --out profiles/rev_compare_rmat26.json
    python tools/rev_compare.py --scale 22 --mirror-check      # the exact mirror check's cost

Runs the query with bu_force = -1 (top-down), 1 (pull) and 0 (the heuristic: pull when
E >= in-entries / rev_bu_div), hop statistics on, after a warm-up, and prints one JSON document:
per setting and hop the mode, ms, kernel ms, E (the frontier's in-degree sum), entries read and rows
found; the results' digests must agree.  The frontiers of a hop are the same under every setting,
so the hops compare one to one.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from nebula_amd import GraphSpace, synth  # noqa: E402

FOLLOW = 1


def run(sp, starts, hops, force, reps):
    sp.set_option("bu_force", force)
    per_hop, total, scanned, digest = None, [], 0, None
    for i in range(reps + 1):  # the first is the warm-up
        r = sp.go(starts, hops, FOLLOW, distinct=True, reversely=True)
        t = sp.last_timing()
        if i == 0:
            continue
        total.append(t["total_ms"])
        scanned = r.edges_scanned
        col = np.sort(r.columns[0])
        digest = (int(r.n_rows), int(col.sum() & 0x7FFFFFFFFFFFFFFF), int(col[::max(1, len(col) // 64)].sum() & 0xFFFFFFFF))
        hs = t["hops"]
        if per_hop is None:
            per_hop = [{"mode": h["mode"], "final": h["final"], "kernels": h["kernels"], "ms": [], "kernel_ms": [],
                        "c": h["c"], "bytes": h["bytes"]} for h in hs]
        for a, h in zip(per_hop, hs):
            a["ms"].append(h["ms"])
            a["kernel_ms"].append(h["kernel_ms"])
    for a in per_hop:
        a["ms_all"] = [round(x, 4) for x in a["ms"]]
        a["ms"] = round(statistics.median(a["ms"]), 4)
        a["kernel_ms"] = round(statistics.median(a["kernel_ms"]), 4)
    return {"bu_force": force, "total_ms": round(statistics.median(total), 4), "edges_scanned": int(scanned),
            "digest": digest, "hops": per_hop}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--hops", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mirror-check", action="store_true",
                    help="time the exact mirror check (option rev_mirror_recheck clears the cached state per query)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sp = GraphSpace(64)
    sp.set_edge_schema(FOLLOW, [("weight", 2)])
    t0 = time.time()
    sp.gen_rmat(args.scale, args.edge_factor, 1, FOLLOW)
    sp.finalize()
    info = sp.info(FOLLOW)
    doc = {"scale": args.scale, "edge_factor": args.edge_factor, "seeds": args.seeds, "hops": args.hops,
           "build_s": round(time.time() - t0, 2), "num_vertices": info["num_vertices"], "out_edges": info["local_out_edges"],
           "in_edges": info["local_in_edges"]}
    starts = synth.seeds(args.scale, args.edge_factor, 1, args.seeds)
    if args.mirror_check:
        sp.set_option("bu_force", 1)
        wall = {}
        for recheck in (0, 1, 0, 1, 0, 1):
            sp.set_option("rev_mirror_recheck", recheck)
            t1 = time.perf_counter()
            r = sp.go(starts, args.hops, FOLLOW, distinct=True, reversely=True)
            wall.setdefault(recheck, []).append(round((time.perf_counter() - t1) * 1e3, 3))
            pulled = [h["mode_id"] for h in sp.last_timing()["hops"]]
            assert 6 in pulled, pulled  # the check answered "mirrored"
        doc["mirror_check"] = {"query_wall_ms_cached": wall[0], "query_wall_ms_with_check": wall[1], "rows": int(r.n_rows)}
    else:
        doc["runs"] = [run(sp, starts, args.hops, f, args.reps) for f in (-1, 1, 0)]
        assert len({tuple(x["digest"]) for x in doc["runs"]}) == 1, [x["digest"] for x in doc["runs"]]
        assert len({x["edges_scanned"] for x in doc["runs"]}) == 1
    sp.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
