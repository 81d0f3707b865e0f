#!/usr/bin/env python3
"""profiles/<tag>_sharded_cost.md from tools/sharded_cost.py's JSON lines: the measured per-rank
work of C3 (LocalComm rank groups on one GPU) and C4 (rank 0's pair subset alone on one GPU),
and the per-GPU time projected for W GPUs from them.

Projection model (stated in the output):
  C3 per GPU = K1 x (rank's kernel bytes / one-rank kernel bytes)
               + host (one-rank wall - one-rank busy span)
               + exchanges: N_coll collectives (counted by the engine, nbg_timing.comm_calls) x
                 (L1 + dL), plus the rank's exchange bytes over its W - 1 xGMI links at B_link
  where the one-rank numbers come from the SHARDED algorithm run through a real one-rank RCCL
  communicator (bench.py --full --comm-single, tools/kt_timeline.sh ... --comm-single): K1 = its kernels
  without the RCCL ones, L1 = one RCCL call on the engine stream (its kernel + the idle gap before
  the next launch), measured; dL = the extra latency of a W-rank exchange over xGMI, ASSUMED
  (a one-GPU lease cannot measure it).
  C4 per GPU = rank 0's measured batch time (no collective in the traversal)

    python tools/sharded_summary.py gpurun_out/<tag>/sharded.jsonl <comm-single bench json> \
        <comm-single query timeline txt> <out.md> [round label]
"""
import json
import sys

DL_COLL_US = 5.0      # ASSUMED extra latency of a W-rank xGMI exchange over the one-rank call
B_LINK_GBS = 153.0    # per xGMI link and direction (the task statement's figure)


# kernels whose work does not shrink with W: the start frontier, hop 1 from 64 seeds (latency-
# bound at any size; with go_rep1 every rank runs it whole), the byte map -> bitmap pass over the
# whole gidx space (k_map_to_bits; go_rep1: the whole-space k_compact and the copy of the owned
# slice), the counter publish
FIXED = ("k_starts_small", "k_expand<0, 0>", "k_map_to_bits", "nbg::k_compact", "k_reduce_partials", "copyBuffer",
         "k_publish")


def timeline_stats(path):
    """(busy us, RCCL kernel us, RCCL calls, us of RCCL kernel + the gap after it, span us,
    us of the FIXED kernels)"""
    rows = []
    for line in open(path):
        if line.startswith("#"):
            continue
        f = line.split()
        if len(f) < 6:
            continue
        rows.append((float(f[0]), float(f[2]), float(f[4]), " ".join(f[5:])))
    busy = sum(r[2] for r in rows)
    rccl = [i for i, r in enumerate(rows) if "nccl" in r[3].lower()]
    rk = sum(rows[i][2] for i in rccl)
    per = sum(rows[i][2] + (rows[i + 1][1] if i + 1 < len(rows) else 0.0) for i in rccl)
    span = rows[-1][0] + rows[-1][2] if rows else 0.0
    fixed = sum(r[2] for r in rows if any(k in r[3] for k in FIXED))
    return busy, rk, len(rccl), per, span, fixed


def main():
    lines = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
    bench = json.loads([l for l in open(sys.argv[2]) if l.startswith("{")][-1])
    busy, rk_us, n_rccl, rccl_us, span, fixed_us = timeline_stats(sys.argv[3])
    out = sys.argv[4]
    label = sys.argv[5] if len(sys.argv) > 5 else "round 6"
    one_hops = bench["roofline"]["hops"]
    one_bytes = sum(h["kernel_bytes"] for h in one_hops if h.get("kernel_bytes"))
    one_wall = bench["ms_per_step"] * 1e3
    k1_us = busy - rk_us                       # the sharded algorithm's kernels on one rank
    l1_us = rccl_us / n_rccl if n_rccl else 0.0  # one RCCL call on the engine stream
    # host: the synchronous call's entry and its counter wait beyond the query's kernel span (the
    # span's own idle gaps -- the ~4.7 us after each RCCL kernel -- are in the collective term)
    host_us = max(0.0, one_wall - span)
    md = [f"# Multi-GPU cost evidence from one MI355X ({label})", "",
          "Measured on the one-GPU lease; the 8-GPU scaling curve itself is the driver's (SCALE_rNN).", "",
          "## C4: FIND SHORTEST PATH, 1024 pairs, RMAT-26 -- rank r's pair subset (pairs r, r + W, ...) alone", "",
          "Pairs are sharded i % W over replicated CSRs and the traversal exchanges nothing, so these are the",
          "per-GPU batch times of a W-GPU run (device-driven batches, one batch per rank).", "",
          "| W | rank | pairs | ms / batch | device ms | host waits | whole-job pairs/s (1024 / slowest rank) |",
          "|---|---|---|---|---|---|---|"]
    c4 = [d for d in lines if d.get("c4")]
    for w in sorted({d["world"] for d in c4}):
        rows = [d for d in c4 if d["world"] == w]
        slow = max(d["ms_per_batch"] for d in rows)
        for d in rows:
            md.append(f"| {w} | {d['rank']} | {d['pairs']} | {d['ms_per_batch']:.3f} | {d['device_ms']:.3f} | "
                      f"{d['host_waits']} | {1024 / slow * 1e3:,.0f} |")
    one = next((d["ms_per_batch"] for d in c4 if d["world"] == 1), None)
    if one:
        md += ["", "What bounds it: the scan kernels shrink with the pairs (the rank's `scan ms`), the batch's",
               "fixed chain (selects, steps, post, walk fronts, result launches: ~0.2 ms) does not.", "",
               "| W | scan ms (rank 0) | rest of the batch ms |", "|---|---|---|"]
        for d in c4:
            if d["rank"] == 0:
                md.append(f"| {d['world']} | {d['scan_ms']:.3f} | {d['ms_per_batch'] - d['scan_ms']:.3f} |")
    md += ["", "## C3: GO 3 STEPS ... YIELD DISTINCT on RMAT-26, W LocalComm ranks sharing the one GPU", "",
           "Per rank: the hop records' kernel bytes (byte models of section 3), exchange bytes and host waits.",
           "The ranks share one GPU here, so their kernel times are contention times, not a W-GPU run's.", "",
           "| W | rank | hop bytes MB (td, bu, fin) | exchange MB | host waits | spec hops |", "|---|---|---|---|---|---|"]
    proj = []
    for d in [d for d in lines if d.get("c3")]:
        w = d["world"]
        mx_bytes = 0
        for r in d["ranks"]:
            hb = [h["kernel_bytes"] / 1e6 for h in r["hops"]]
            mx_bytes = max(mx_bytes, sum(h["kernel_bytes"] for h in r["hops"]))
            md.append(f"| {w} | {r['rank']} | {', '.join(f'{x:.1f}' for x in hb)} | {r['comm_bytes'] / 1e6:.1f} | "
                      f"{r['host_waits']} | {r['spec_hops']} |")
        comm_mb = max(r["comm_bytes"] for r in d["ranks"]) / 1e6
        ncoll = max((r.get("comm_calls") or 0) for r in d["ranks"]) or n_rccl
        k_us = fixed_us + (k1_us - fixed_us) * mx_bytes / one_bytes if one_bytes else float("nan")
        c_us = ncoll * (l1_us + DL_COLL_US) + comm_mb / (max(w - 1, 1) * B_LINK_GBS) * 1e3
        proj.append((w, ncoll, k_us, c_us, host_us, k_us + c_us + host_us))
    md += ["", "## Projected per-GPU C3 query time at W GPUs", "",
           "The one-rank numbers are the sharded algorithm run through a real one-rank RCCL communicator",
           f"(`bench.py --full --comm-single`: {one_wall:.0f} us/query wall, digest {bench['parity'].get('status')};",
           f"kernel timeline: {busy:.0f} us busy, of it {rk_us:.0f} us in {n_rccl} RCCL kernels).", "",
           f"* kernels = {fixed_us:.0f} us that do not shrink with W ({', '.join(FIXED)}) + the other",
           f"  {k1_us - fixed_us:.0f} us of the one-rank sharded query's kernels (RCCL's excluded) x the slowest",
           "  rank's share of the bytes;",
           f"* exchanges = the rank's collectives (engine count) x ({l1_us:.1f} us measured one-rank RCCL call on the",
           f"  engine stream: kernel + the gap before the next launch, + {DL_COLL_US:.0f} us ASSUMED for a W-rank xGMI",
           f"  exchange) + its exchange bytes over W - 1 links at {B_LINK_GBS:.0f} GB/s;",
           f"* host = {host_us:.0f} us (the call's entry and its counter wait beyond the kernels).", "",
           "| W | collectives / query | kernels us | exchanges us | host us | per query us | projected GTEPS (1.545 G edges / query) |",
           "|---|---|---|---|---|---|---|"]
    for w, n, k, c, h, t in proj:
        md.append(f"| {w} | {n} | {k:.0f} | {c:.0f} | {h:.0f} | {t:.0f} | {1.545e9 / (t * 1e-6) / 1e9:,.0f} |")
    md += ["", f"One GPU, unsharded: see the round's bench line.  Past W = 4 the exchange latency, not the bytes,",
           "bounds a query: its collectives' latency plus the kernels' 1 / W share."]
    open(out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
