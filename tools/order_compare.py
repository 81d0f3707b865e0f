#!/usr/bin/env python3
"""GO ... | ORDER BY on the device against ordering the same result on the host (GPU box only).

The C3 shape (64 seeds, WHERE weight > 499, YIELD DISTINCT _dst) on one RMAT scale.  After a
warm-up, two sides alternate for --rounds rounds, each timed on the host clock from the call to
the ordered ids in host memory:

  (A) what a caller does without nbg_order_by: go() to the host, then np.sort on the id column;
  (B) go(order_by=[(0, 0)]) to the host: the result stays in HBM, is sorted there, and only the
      ordered ids cross the link.

For the sort alone (side B's nbg_order_by call, from nbg_last_timing): device total_ms, the radix
passes that ran, the algorithmic bytes of the keys-only path (rows x 8 for the histogram read plus
rows x 16 per executed pass; the per-tile count kernel's second read of the keys is not in this
figure) and the fraction of the 8 TB/s HBM peak they amount to.

Prints one JSON line and appends a table section to --md (default profiles/order_by.md).

    python3 tools/order_compare.py --scale 22
    python3 tools/order_compare.py --scale 26 --rounds 10
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK_BPS = 8e12


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "spread": round(max(v) - min(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--md", default=str(ROOT / "profiles" / "order_by.md"))
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
    q = dict(where=X.AliasProp("follow", "weight") > 499, yields=[X.EdgeDst("follow")], distinct=True)

    def side_a():
        t0 = time.perf_counter()
        r = sp.go(starts, args.steps, 1, **q)
        t1 = time.perf_counter()
        ids = np.sort(r.columns[0])
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, ids

    def side_b():
        t0 = time.perf_counter()
        r = sp.go(starts, args.steps, 1, order_by=[(0, 0)], **q)
        ids = r.columns[0]
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, sp.last_timing(), ids

    for _ in range(args.warmup):
        a = side_a()
        b = side_b()
    if not np.array_equal(a[3], b[2]):
        raise SystemExit("order_compare: the device order differs from np.sort of the same result")
    a_ms, a_go, a_sort, b_ms, s_ms = [], [], [], [], []
    for _ in range(args.rounds):
        a = side_a()
        a_ms.append(a[0]), a_go.append(a[1]), a_sort.append(a[2])
        b = side_b()
        b_ms.append(b[0]), s_ms.append(b[1]["total_ms"])
    t = b[1]
    rows = int(len(b[2]))
    passes = int(t["steps_run"])
    model = rows * 8 + rows * 16 * passes
    sort_med = statistics.median(s_ms)
    out = {"scale": args.scale, "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
           "options": args.option, "rows": rows,
           "host_sort": {"ms": summary(a_ms), "go_to_host_ms": summary(a_go), "np_sort_ms": summary(a_sort)},
           "device_sort": {"ms": summary(b_ms)},
           "sort_alone": {"total_ms": summary(s_ms), "passes": passes, "launches": int(t["launches"]),
                          "host_waits": int(t["host_waits"]), "model_bytes": model,
                          "fraction_of_hbm_peak": round(model / (sort_med * 1e-3) / HBM_PEAK_BPS, 4) if sort_med > 0 else None},
           "device_beats_host": statistics.median(b_ms) < statistics.median(a_ms)}
    print(json.dumps(out))
    if args.md:
        sa = out["sort_alone"]
        lines = [f"## RMAT-{args.scale}, GO {args.steps} STEPS ... YIELD DISTINCT _dst | ORDER BY $-.id "
                 f"({rows} rows, {args.rounds} alternated rounds after {args.warmup} warm-up rounds)", "",
                 "Host clock, call to ordered ids in host memory (ms):", "",
                 "| side | median | min | max | spread |", "|---|---|---|---|---|"]
        for name, m in (("(A) go() to the host + np.sort", out["host_sort"]["ms"]),
                        ("(A) ... its go() alone", out["host_sort"]["go_to_host_ms"]),
                        ("(A) ... its np.sort alone", out["host_sort"]["np_sort_ms"]),
                        ("(B) go(order_by=[(0, 0)]) to the host", out["device_sort"]["ms"])):
            lines.append(f"| {name} | {m['median']} | {m['min']} | {m['max']} | {m['spread']} |")
        m = sa["total_ms"]
        lines += ["", f"nbg_order_by alone (device time): median {m['median']} ms, min {m['min']}, max {m['max']}; "
                      f"{sa['passes']} of 8 passes ran, {sa['launches']} launches, {sa['host_waits']} host waits; "
                      f"model {sa['model_bytes']} B (rows x 8 + rows x 16 per pass) = "
                      f"{sa['fraction_of_hbm_peak']} of 8 TB/s.", ""]
        p = Path(args.md)
        p.parent.mkdir(parents=True, exist_ok=True)
        with p.open("a") as f:
            f.write("\n".join(lines) + "\n")
    sp.close()


if __name__ == "__main__":
    main()
