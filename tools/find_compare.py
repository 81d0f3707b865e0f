#!/usr/bin/env python3
"""FIND props FROM follow WHERE weight > k on the device against the only way to answer the same
question without the call (GPU box only; needs no reference tree).

RMAT --scale, WHERE follow.weight > 989 (about 1 % of the edges pass) and > 499 (about half),
keep_on_device = 1, no yields (the key columns _src, _dst, _rank alone).  Timed, after --warmup
calls, as medians of --rounds calls, from nbg_last_timing (HIP events on the engine's stream):

  fast      nbg_find_edges on the typed-compare path (k_find_count / k_find_emit)
  general   nbg_find_edges with option find_fast = 0 (k_expand's flag mode + select)
  baseline  nbg_go 1 STEPS from every source vid with the same WHERE and keep_on_device, yielding
            _src, _dst, _rank: the API as it stood before nbg_find_edges

total_ms is the call's device time, expand_ms the scan kernels alone.  For the fast path the scan
pair's achieved bytes per second on its own byte model (expand_bytes) and that
figure as a fraction of the 8 TB/s HBM peak are reported.  The row counts of the three must agree.
Nothing is gated on the figures; nothing is retried.  Prints one JSON line and appends a table to
--md (default profiles/find.md).

    python3 tools/find_compare.py --scale 26
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK_BPS = 8e12
T_INT = 2


def med(v):
    return round(statistics.median(v), 4) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--thresholds", type=int, nargs="*", default=[989, 499])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=str(ROOT / "profiles" / "find.md"))
    args = ap.parse_args()
    from nebula_amd import GraphSpace, synth
    from nebula_amd import expr as X

    sp = GraphSpace(64)
    sp.set_edge_schema(1, [("weight", T_INT)], name="follow")
    sp.gen_rmat(args.scale, 16, 1, 1)
    sp.finalize()
    info = sp.info(1)
    w = X.AliasProp("follow", "weight")
    keys = [X.AliasProp("follow", f) for f in ("_src", "_dst", "_rank")]
    starts = np.ascontiguousarray(synth.vid(np.arange(1 << args.scale, dtype=np.uint64), 1).astype(np.int64))
    out = []
    for k in args.thresholds:
        where = w > k
        rows = {}
        for name in ("fast", "general", "baseline"):
            if name == "general":
                sp.set_option("find_fast", 0)
            else:
                sp.unset_option("find_fast")
            tot, ker, t, n = [], [], None, None
            for i in range(args.warmup + args.rounds):
                if name == "baseline":
                    rs = sp.go(starts, 1, 1, where=where, yields=keys, keep_on_device=True)
                else:
                    rs = sp.find_edges(1, where, keep_on_device=True)
                t = sp.last_timing()
                n = rs.n_rows
                del rs
                if i >= args.warmup:
                    tot.append(t["total_ms"]), ker.append(t["expand_ms"])
            rows[name] = n
            km = med(ker)
            r = {"where": f"weight > {k}", "path": name, "rows": int(n), "total_ms": med(tot), "scan_ms": km,
                 "launches": int(t["launches"]), "host_waits": int(t["host_waits"]), "model_bytes": int(t["expand_bytes"])}
            if name == "fast" and km:
                r["scan_bytes_per_s"] = round(t["expand_bytes"] / (km * 1e-3))
                r["fraction_of_hbm_peak"] = round(t["expand_bytes"] / (km * 1e-3) / HBM_PEAK_BPS, 4)
            out.append(r)
        sp.unset_option("find_fast")
        if len(set(rows.values())) != 1:
            raise SystemExit(f"find_compare: weight > {k}: the row counts differ: {rows}")
    res = {"scale": args.scale, "out_edges": int(info["local_out_edges"]), "vertices": int(info["num_vertices"]), "runs": out}
    sp.close()
    print(json.dumps(res))
    if args.md:
        lines = [f"## RMAT-{args.scale}, {res['out_edges']} out-edges (medians of {args.rounds} calls after {args.warmup} warm-ups)", "",
                 "| WHERE | path | rows | total ms | scan kernels ms | launches | host waits | model bytes | scan B/s | of 8 TB/s |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for r in out:
            lines.append(f"| {r['where']} | {r['path']} | {r['rows']} | {r['total_ms']} | {r['scan_ms']} | {r['launches']} | "
                         f"{r['host_waits']} | {r['model_bytes']} | {r.get('scan_bytes_per_s', '')} | "
                         f"{r.get('fraction_of_hbm_peak', '')} |")
        lines.append("")
        p = Path(args.md)
        p.parent.mkdir(parents=True, exist_ok=True)
        with p.open("a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
