// edge_lookup.h -- the 16-lane group lookup of one (rank, dst) key in a CSR row: a binary search
// under the row's bytewise order down to a window, then a coalesced scan of the window.  Shared by
// k_fetch_edge (fetch.hip: FETCH PROP ON an edge type) and k_mirror_check (go_variants.hip: do the in
// keys mirror the out keys, GO ... REVERSELY).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"

namespace nbg {

constexpr int kLookupGroup = 16;  // lanes per key

// the CSR a group searches
struct EdgeRows {
  const int32_t* col;
  const int64_t* col_vid;  // or null: vid_of[col[e]]
  const int64_t* erank;    // or null: every edge has rank 0
  const int64_t* vid_of;
  int64_t window;  // entries the search leaves to the scan: 1 search, INT64_MAX scan, else the threshold
};

// One 16-lane group per key, every lane of a group called with the same arguments: the entry of
// [beg, end) holding (rk, dv) -- dg = dv's gidx -- or -1.  Inside a row the entries ascend in
// (bswap64(rank), bswap64(dst vid)) compared unsigned (the reference's key order), and the CSR
// keeps one entry per (rank, dst), so a key matches at most one entry.  A binary search under that
// order narrows the row to a window of at most `window` entries that holds the match if there is
// one (every lane of the group runs the same probes: one broadcast address per group); then the
// group scans the window, col (and rank) 16 entries a step, and a ballot picks the hit.  window =
// 1: a pure search; window >= the row: a pure scan; the hybrid scans rows up to the threshold whole
// and searches longer rows down to a threshold-sized window, which spares them the last
// log2(threshold) dependent probes.  The scan loop's condition is wave-uniform, so the ballot runs
// with every lane active: the whole wave calls this together (a group without a key: beg == end).
// scanned / probed: lane 0 of the group counts the entries its scans read and its searches probed.
__device__ __forceinline__ int64_t group_find_edge(const EdgeRows& a, int64_t beg, int64_t end, int64_t rk, int64_t dv,
                                                   int32_t dg, unsigned long long& scanned,
                                                   unsigned long long& probed) {
  const int lane = threadIdx.x & (kWave - 1), sub = lane & (kLookupGroup - 1), grp = lane / kLookupGroup;
  // the match, if any, is the lower bound of (krk, kdv), which lies in [l, h]: entries below l
  // are less than the key, entry h (when h < end) is not
  const uint64_t krk = bswap64(uint64_t(rk)), kdv = bswap64(uint64_t(dv));
  int64_t l = beg, h = end;
  while ((h < end ? h + 1 : end) - l > a.window) {
    const int64_t m = l + ((h - l) >> 1);
    const uint64_t er = a.erank ? bswap64(uint64_t(a.erank[m])) : 0;
    bool less = er < krk;
    if (er == krk) {
      const int64_t ev = a.col_vid ? a.col_vid[m] : a.vid_of[a.col[m]];
      less = bswap64(uint64_t(ev)) < kdv;
    }
    if (less) l = m + 1;
    else h = m;
    probed += sub == 0;
  }
  const int64_t wend = h < end ? h + 1 : end;
  int64_t found = -1, base = l;
  while (__any(base < wend)) {
    const int64_t e = base + sub;
    const bool live = base < wend;
    const bool hit = live && e < wend && a.col[e] == dg && (!a.erank || a.erank[e] == rk);
    const unsigned long long m = __ballot(hit);
    const unsigned gm = unsigned(m >> (grp * kLookupGroup)) & 0xffffu;
    if (live) {
      if (sub == 0) scanned += (unsigned long long)min(int64_t(kLookupGroup), wend - base);
      if (gm) {
        found = base + (__ffs(int(gm)) - 1);
        base = wend;
      } else {
        base += kLookupGroup;
      }
    }
  }
  return found;
}

}  // namespace nbg
