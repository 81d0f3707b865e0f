#!/usr/bin/env python3
"""UNION / INTERSECT / MINUS of two GO results on the device against combining them on the host
(GPU box only).

Two C3-shaped results on one RMAT scale: 64 seeds each, the two seed sets sharing --overlap seeds.
Two table shapes:

  1col   GO --steps STEPS ... WHERE weight > 499 YIELD DISTINCT _dst
  3col   GO --steps3 STEPS ... WHERE weight > --min3 YIELD _src, _dst, weight

For every operator, after a warm-up, two sides alternate for --rounds rounds, each timed on the
host clock from the first call to the combined rows in host memory:

  (A) both results to the host, combined there: numpy on one column (np.concatenate, np.unique,
      np.isin), a Python set of row tuples on three;
  (B) both GOs kept in HBM, nbg_set_op on the device tables, only the result copied back.  (A GO
      result kept in HBM is handed to the call through a zero-factor order_by, which copies it once
      on the device: the price of a device table that owns its columns.)

For the set operator alone (side B's nbg_set_op, from nbg_last_timing): device total_ms, launches,
host waits, rows in and out, and the algorithmic bytes under DESIGN.md's model against the 8 TB/s
HBM peak.  Nothing is gated on the figures.  The run stops starting new rounds once --budget
seconds have passed; nothing is retried.

Prints one JSON line and appends a table section to --md (default profiles/set_ops.md).

    python3 tools/setop_compare.py --scale 22
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
OPS = [("UNION ALL", 1, False), ("UNION DISTINCT", 1, True), ("INTERSECT", 2, False), ("MINUS", 3, False)]


def med(v):
    return round(statistics.median(v), 4) if v else None


def model_bytes(name, n_l, n_r, n_out, row_bytes):
    """DESIGN.md section 3 "Set operators": hash pass = column bytes read + 8 B a row written; build
    and probe = 8 B hash + one 8 B table access a row (the lower bound); gather = 4 B index + the
    row read and written.  UNION ALL: the rows read and written once."""
    n = n_l + n_r
    if name == "UNION ALL":
        return 2 * n * row_bytes
    gather = n_out * (4 + 2 * row_bytes)
    if name == "UNION DISTINCT":
        return 2 * n * row_bytes + n * (row_bytes + 8) + 2 * n * 16 + gather
    return n * (row_bytes + 8) + n_r * 16 + n_l * 16 + gather


def host_combine(name, left, right):
    """what a caller does without the call; returns the combined columns"""
    if len(left) == 1:
        a, b = left[0], right[0]
        if name == "UNION ALL":
            return [np.concatenate([a, b])]
        if name == "UNION DISTINCT":
            return [np.unique(np.concatenate([a, b]))]
        hit = np.isin(a, b)
        return [a[hit] if name == "INTERSECT" else a[~hit]]
    lrows, rrows = list(zip(*[c.tolist() for c in left])), list(zip(*[c.tolist() for c in right]))
    if name == "UNION ALL":
        rows = lrows + rrows
    elif name == "UNION DISTINCT":
        rows = list(dict.fromkeys(lrows + rrows))
    else:
        rs = set(rrows)
        rows = [r for r in lrows if r in rs] if name == "INTERSECT" else [r for r in lrows if r not in rs]
    return [np.asarray(c, dtype=np.int64) for c in zip(*rows)] if rows else [np.zeros(0, np.int64)] * len(left)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--rounds3", type=int, default=3, help="rounds of the 3-column shape (its host side is slow)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--steps3", type=int, default=2)
    ap.add_argument("--min3", type=int, default=899)
    ap.add_argument("--overlap", type=int, default=32, help="seeds the two 64-seed sets share")
    ap.add_argument("--budget", type=float, default=240.0, help="seconds after which no new round starts")
    ap.add_argument("--md", default=str(ROOT / "profiles" / "set_ops.md"))
    args = ap.parse_args()
    from nebula_amd import GraphSpace, synth
    from nebula_amd import expr as X
    t_start = time.perf_counter()
    sp = GraphSpace(64)
    sp.set_edge_schema(1, [("weight", 2)])
    sp.gen_rmat(args.scale, 16, 1, 1)
    sp.finalize()
    pool = synth.seeds(args.scale, 16, 1, 128 - args.overlap)
    starts_l, starts_r = np.ascontiguousarray(pool[:64]), np.ascontiguousarray(pool[64 - args.overlap:])
    w = X.AliasProp("follow", "weight")
    shapes = [("1col", args.steps, args.rounds,
               dict(where=w > 499, yields=[X.EdgeDst("follow")], distinct=True)),
              ("3col", args.steps3, args.rounds3,
               dict(where=w > args.min3, yields=[X.EdgeSrc("follow"), X.EdgeDst("follow"), w]))]
    results = []
    for shape, steps, rounds, q in shapes:
        for name, op, distinct in OPS:
            def side_a():
                t0 = time.perf_counter()
                l = sp.go(starts_l, steps, 1, **q)
                r = sp.go(starts_r, steps, 1, **q)
                cols = host_combine(name, l.columns, r.columns)
                return (time.perf_counter() - t0) * 1e3, cols, l.n_rows, r.n_rows

            def side_b():
                t0 = time.perf_counter()
                l = sp.go(starts_l, steps, 1, order_by=[], keep_on_device=True, **q)
                r = sp.go(starts_r, steps, 1, order_by=[], keep_on_device=True, **q)
                out = sp.set_op(op, l, r, distinct=distinct)
                cols = out.columns
                return (time.perf_counter() - t0) * 1e3, cols, sp.last_timing()

            a = b = None
            for _ in range(max(1, args.warmup)):
                a, b = side_a(), side_b()
            # the same rows (UNION DISTINCT: the host side sorts or keeps first occurrences; compare as sets)
            ga, gb = np.stack(a[1]), np.stack(b[1])
            if ga.shape != gb.shape or not np.array_equal(ga[:, np.lexsort(ga[::-1])], gb[:, np.lexsort(gb[::-1])]):
                raise SystemExit(f"setop_compare: {shape} {name}: the device rows differ from the host's")
            a_ms, b_ms, s_ms = [], [], []
            for _ in range(rounds):
                if time.perf_counter() - t_start > args.budget:
                    break
                a = side_a()
                a_ms.append(a[0])
                b = side_b()
                b_ms.append(b[0]), s_ms.append(b[2]["total_ms"])
            t = b[2]
            n_l, n_r, n_out = int(a[2]), int(a[3]), int(len(b[1][0]))
            row_bytes = 8 * len(b[1])
            mb = model_bytes(name, n_l, n_r, n_out, row_bytes)
            sm = med(s_ms)
            results.append({"shape": shape, "op": name, "steps": steps, "rounds": len(a_ms), "rows_left": n_l,
                            "rows_right": n_r, "rows_out": n_out, "host_ms": med(a_ms), "device_ms": med(b_ms),
                            "set_op_total_ms": sm, "launches": int(t["launches"]), "host_waits": int(t["host_waits"]),
                            "model_bytes": mb,
                            "fraction_of_hbm_peak": round(mb / (sm * 1e-3) / HBM_PEAK_BPS, 4) if sm else None,
                            "device_beats_host": (med(b_ms) < med(a_ms)) if a_ms else None})
    out = {"scale": args.scale, "overlap": args.overlap, "warmup": args.warmup, "min3": args.min3, "results": results}
    print(json.dumps(out))
    if args.md:
        lines = [f"## RMAT-{args.scale}, two 64-seed results sharing {args.overlap} seeds "
                 f"(alternated rounds after {args.warmup} warm-up rounds)", "",
                 "Host clock from the first GO to the combined rows in host memory, medians (ms); the set "
                 "operator alone is nbg_set_op's device total_ms.", "",
                 "| shape | operator | rows left | rows right | rows out | (A) host ms | (B) device ms | set op alone ms "
                 "| launches | host waits | model bytes | of 8 TB/s | rounds |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in results:
            lines.append(f"| {r['shape']} (GO {r['steps']} STEPS) | {r['op']} | {r['rows_left']} | {r['rows_right']} | "
                         f"{r['rows_out']} | {r['host_ms']} | {r['device_ms']} | {r['set_op_total_ms']} | {r['launches']} | "
                         f"{r['host_waits']} | {r['model_bytes']} | {r['fraction_of_hbm_peak']} | {r['rounds']} |")
        lines.append("")
        p = Path(args.md)
        p.parent.mkdir(parents=True, exist_ok=True)
        with p.open("a") as f:
            f.write("\n".join(lines) + "\n")
    sp.close()


if __name__ == "__main__":
    main()
