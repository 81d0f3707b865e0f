#!/usr/bin/env python3
"""GO UPTO 3 STEPS against the way to get the same result without it (GPU box only).

The C3 shape (64 seeds, WHERE weight > 499, YIELD DISTINCT _dst, keep_on_device) on one RMAT
scale.  After a warm-up, two sides alternate for --rounds rounds:

  (A) three calls GO 1 / 2 / 3 STEPS, their last_timing()["total_ms"] summed (a caller would
      still have to union the three results; that host work is not counted);
  (B) one GO UPTO 3 STEPS.

Prints one JSON line (median, min, max and spread of both sides, per-hop ms and counters of the
last round, edges_scanned) and, with --md, appends a table section to that file.

    python3 tools/upto_compare.py --scale 22 --md profiles/upto_compare.md
    rocprofv3 --kernel-trace --stats -d /tmp/upto -- python3 tools/upto_compare.py --scale 26 --only-upto
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "spread": round(max(v) - min(v), 4)}


def hops_of(t):
    return [{"mode": h["mode"], "final": h["final"], "ms": round(h["ms"], 4), "kernel": h["kernels"][0],
             "c": h["c"][:4], "bytes": h["bytes"]} for h in t["hops"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only-upto", action="store_true", help="side (B) alone (a profiler run)")
    ap.add_argument("--md", default=None)
    ap.add_argument("--option", action="append", default=[], help="engine option key=value")
    args = ap.parse_args()
    from nebula_amd import GraphSpace, synth
    from nebula_amd import expr as X
    sp = GraphSpace(64)
    for kv in args.option:
        k, v = kv.split("=")
        sp.set_option(k, int(v))
    sp.set_edge_schema(1, [("weight", 2)])
    sp.gen_rmat(args.scale, 16, 1, 1)
    sp.finalize()
    starts = synth.seeds(args.scale, 16, 1, 64)
    q = dict(where=X.AliasProp("follow", "weight") > 499, yields=[X.EdgeDst("follow")], distinct=True,
             keep_on_device=True)

    def side_a():
        ms, scanned, rows, hops = 0.0, 0, 0, []
        for k in range(1, args.steps + 1):
            r = sp.go(starts, k, 1, **q)
            t = sp.last_timing()
            ms += t["total_ms"]
            scanned += r.edges_scanned
            rows += r.n_rows
            hops.append(hops_of(t))
        return ms, scanned, rows, hops

    def side_b():
        r = sp.go(starts, args.steps, 1, upto=True, **q)
        t = sp.last_timing()
        return t["total_ms"], r.edges_scanned, r.n_rows, hops_of(t)

    for _ in range(args.warmup):
        if not args.only_upto:
            side_a()
        side_b()
    a_ms, b_ms, a, b = [], [], None, None
    for _ in range(args.rounds):
        if not args.only_upto:
            a = side_a()
            a_ms.append(a[0])
        b = side_b()
        b_ms.append(b[0])
    out = {"scale": args.scale, "steps": args.steps, "rounds": args.rounds, "options": args.option,
           "upto": {"ms": summary(b_ms), "edges_scanned": b[1], "rows": b[2], "hops": b[3]}}
    if a:
        out["separate"] = {"ms": summary(a_ms), "edges_scanned": a[1], "rows_summed": a[2], "hops": a[3]}
        out["upto_le_separate"] = out["upto"]["ms"]["median"] <= out["separate"]["ms"]["median"]
    print(json.dumps(out))
    if args.md:
        lines = [f"## RMAT-{args.scale}, GO UPTO {args.steps} STEPS against GO 1..{args.steps} STEPS "
                 f"({args.rounds} alternated rounds)", "",
                 "| side | median ms | min | max | spread | edges_scanned | rows |", "|---|---|---|---|---|---|---|"]
        for name, key, rk in (("(A) separate calls, summed", "separate", "rows_summed"), ("(B) one UPTO call", "upto", "rows")):
            if key in out:
                m = out[key]["ms"]
                lines.append(f"| {name} | {m['median']} | {m['min']} | {m['max']} | {m['spread']} | "
                             f"{out[key]['edges_scanned']} | {out[key][rk]} |")
        lines += ["", "Per hop, last round (ms; c = first reached / their out-degree sum / level size / entries "
                  "read for the BFS hops, the engine's usual counters otherwise):", ""]
        if a:
            for k, hs in enumerate(out["separate"]["hops"], 1):
                for h in hs:
                    lines.append(f"- (A) GO {k}: {h['mode']}{' final' if h['final'] else ''} {h['ms']} ms "
                                 f"`{h['kernel']}` c={h['c']}")
        for h in out["upto"]["hops"]:
            lines.append(f"- (B) {h['mode']}{' final' if h['final'] else ''} {h['ms']} ms `{h['kernel']}` "
                         f"c={h['c']} bytes={h['bytes']}")
        lines.append("")
        p = Path(args.md)
        p.parent.mkdir(parents=True, exist_ok=True)
        with p.open("a") as f:
            f.write("\n".join(lines) + "\n")
    sp.close()


if __name__ == "__main__":
    main()
