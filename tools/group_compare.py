#!/usr/bin/env python3
"""GROUP BY on device-resident tables: nbg_group_by's two paths against numpy on the host and
against the HBM time of the call's algorithmic bytes (GPU box only).

Synthetic tables of 2^--log-rows rows kept in HBM: one VID key uniform over G groups, one INT and
one DOUBLE value column, for G in --groups (default 1, 16, 2^10, 2^16, 2^20, 2^24).  Per G, after
--warmup rounds, the variants alternate for --rounds rounds:

  A lds      COUNT(*), SUM(int), MIN(int) on the atomic path, LDS stage on wherever
             G x 3 words fit the workgroup's 4096-word block (option group_lds_max = 2^30)
  A direct   the same with the LDS stage off (group_lds_max = 0)
  B exact    the same aggregates on the ordered path (group_sorted = 1)
  B dsum     SUM(double), which always takes the ordered path

Each figure is the call's device total_ms (nbg_last_timing: events around the kernels; the output
stays in HBM), median over the rounds.  Beside it: numpy on the same host over the same columns
already in host memory (np.unique with the inverse, np.bincount, np.add.at, np.minimum.at; the
copy of the table to the host that a caller without the call pays first is NOT in it), and the
time the call's algorithmic bytes (model_bytes below, DESIGN.md section 3 "GROUP BY") take at the
8 TB/s HBM peak DESIGN.md uses.  Nothing is gated on the figures; the device rows are checked
against numpy's once per G.  The run stops starting new rounds once --budget seconds have passed;
nothing is retried.

Prints one JSON line and appends a table section to --md (default profiles/group.md).

    python3 tools/group_compare.py
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
UNSET = -2**63
T_INT, T_VID, T_DOUBLE = 2, 3, 5
LDS_WORDS = 4096  # group.hip kLdsWords


def med(v):
    return round(statistics.median(v), 4) if v else None


def model_bytes(variant, n, g):
    """DESIGN.md section 3 "GROUP BY".  Group ids, per row: hash pass 8 B key + 8 B hash; table
    memset 16 B (8 B x the power of two >= 2n); build 8 B hash + one 8 B slot; representative probe
    8 + 8 + 4 B + 1 B; scan 1 + 4 B; group numbers 4 + 4 + 1 + 4 B; per group 4 B first row + the
    8 B key read and written.  Atomic path: 4 B gid + 8 B value column a row, 3 accumulator words of
    8 B a group initialised, added into at least once and read back.  Ordered path: the digit
    histogram 4 B a row, a radix pass per byte of G - 1 at 32 B a row (key and index read and
    written, the key read twice), segment offsets 8 B a row, and per aggregate with a column 4 B
    index + 8 B value a row."""
    ids = n * (16 + 16 + 16 + 21 + 5 + 13) + g * (4 + 16)
    if variant.startswith("A"):
        return ids + n * (4 + 8) + g * 3 * 8 * 3
    passes = 0
    while (1 << (8 * passes)) < g:
        passes += 1
    cols = 2 if variant == "B exact" else 1  # SUM and MIN each walk the segment
    return ids + n * (4 + 32 * passes + 8 + 12 * cols) + g * (4 + 8 * 3)


def numpy_group(key, ival, dval):
    uniq, inv = np.unique(key, return_inverse=True)
    cnt = np.bincount(inv, minlength=len(uniq))
    s = np.zeros(len(uniq), dtype=np.int64)
    np.add.at(s, inv, ival)
    mn = np.full(len(uniq), np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(mn, inv, ival)
    ds = np.zeros(len(uniq), dtype=np.float64)
    np.add.at(ds, inv, dval)
    return uniq, cnt, s, mn, ds


VARIANTS = [("A lds", dict(group_lds_max=1 << 30), "exact"), ("A direct", dict(group_lds_max=0), "exact"),
            ("B exact", dict(group_sorted=1), "exact"), ("B dsum", dict(), "dsum")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=24)
    ap.add_argument("--groups", type=int, nargs="*", default=[1, 16, 1 << 10, 1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget", type=float, default=400.0, help="seconds after which no new round starts")
    ap.add_argument("--md", default=str(ROOT / "profiles" / "group.md"))
    args = ap.parse_args()
    from nebula_amd import GraphSpace, _lib
    aggs = {"exact": [(_lib.AGG_COUNT, None), (_lib.AGG_SUM, 1), (_lib.AGG_MIN, 1)], "dsum": [(_lib.AGG_SUM, 2)]}
    t_start = time.perf_counter()
    sp = GraphSpace(1)
    n = 1 << args.log_rows
    rng = np.random.default_rng(1)
    ival = rng.integers(-10**9, 10**9, n, dtype=np.int64)
    dval = rng.integers(-2**20, 2**20, n).astype(np.float64)  # integer-valued: every sum order is exact
    results = []
    for g in args.groups:
        key = rng.integers(0, g, n, dtype=np.int64)
        dev = sp.order_by([(T_VID, key), (T_INT, ival), (T_DOUBLE, dval)], [], keep_on_device=True)

        def run(opts, which):
            for k, v in opts.items():
                sp.set_option(k, v)
            try:
                out = sp.group_by(dev, [0], aggs[which], keep_on_device=True)
                return out, sp.last_timing()
            finally:
                for k in opts:
                    sp.set_option(k, UNSET)

        t0 = time.perf_counter()
        uniq, cnt, s, mn, ds = numpy_group(key, ival, dval)
        numpy_ms = [(time.perf_counter() - t0) * 1e3]
        n_groups = len(uniq)
        # the device rows against numpy's, once per variant (first-occurrence order: sort by key)
        for name, opts, which in VARIANTS:
            for _ in range(max(1, args.warmup)):
                out, _ = run(opts, which)
            host = sp.order_by(out, [(0, 0)])
            want = [uniq, cnt, s, mn] if which == "exact" else [uniq, ds]
            if host.n_rows != n_groups or any(not np.array_equal(a, b) for a, b in zip(host.columns, want)):
                raise SystemExit(f"group_compare: G={g} {name}: the device rows differ from numpy's")
        ms = {name: [] for name, _, _ in VARIANTS}
        last = {}
        for r in range(args.rounds):
            if time.perf_counter() - t_start > args.budget:
                break
            for name, opts, which in VARIANTS:
                _, tm = run(opts, which)
                ms[name].append(tm["total_ms"])
                last[name] = tm
            if r == 0:  # numpy a second time: the median of two runs, the host side is slow
                t0 = time.perf_counter()
                numpy_group(key, ival, dval)
                numpy_ms.append((time.perf_counter() - t0) * 1e3)
        for name, _, _ in VARIANTS:
            mb = model_bytes(name, n, n_groups)
            m = med(ms[name])
            results.append({"groups": n_groups, "variant": name, "rounds": len(ms[name]), "device_ms": m,
                            "lds_stage": bool(name == "A lds" and n_groups * 3 <= LDS_WORDS),
                            "launches": int(last[name]["launches"]) if name in last else None,
                            "host_waits": int(last[name]["host_waits"]) if name in last else None,
                            "numpy_ms": med(numpy_ms), "model_bytes": mb,
                            "model_ms_at_hbm_peak": round(mb / HBM_PEAK_BPS * 1e3, 4),
                            "fraction_of_hbm_peak": round(mb / (m * 1e-3) / HBM_PEAK_BPS, 4) if m else None})
        del dev
        print(f"G={n_groups}: done at {time.perf_counter() - t_start:.0f} s", file=sys.stderr, flush=True)
    out = {"rows": n, "warmup": args.warmup, "results": results}
    print(json.dumps(out))
    if args.md:
        lines = [f"## 2^{args.log_rows} rows in HBM, one VID key uniform over G groups "
                 f"(variants alternated for up to {args.rounds} rounds after {args.warmup} warm-up calls each)", "",
                 "Device total_ms of the call (medians, ms); numpy on the same host over the columns already in host "
                 "memory; model = the call's algorithmic bytes at 8 TB/s.", "",
                 "| G | variant | LDS stage | device ms | numpy ms | model bytes | model ms | of 8 TB/s | launches "
                 "| host waits | rounds |",
                 "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in results:
            lines.append(f"| {r['groups']} | {r['variant']} | {'on' if r['lds_stage'] else 'off'} | {r['device_ms']} | "
                         f"{r['numpy_ms']} | {r['model_bytes']} | {r['model_ms_at_hbm_peak']} | "
                         f"{r['fraction_of_hbm_peak']} | {r['launches']} | {r['host_waits']} | {r['rounds']} |")
        lines.append("")
        p = Path(args.md)
        p.parent.mkdir(parents=True, exist_ok=True)
        with p.open("a") as f:
            f.write("\n".join(lines) + "\n")
    sp.close()


if __name__ == "__main__":
    main()
