// find_scan.h -- the arithmetic of FIND's column scan (find.hip: k_find_count, k_find_emit), host
// and device.
//
// A tile is kFindTile consecutive entries of an INT column stored W bytes wide (1, 2, 4, 8): 256
// lanes with 8 consecutive entries each.  A lane reads its 8 entries as W 64-bit words (8 W bytes:
// one 8-byte load for W = 1, W / 2 16-byte loads otherwise):
//   find_elem        element k of those words, sign-extended
//   find_lane_mask   the lane's 8-bit pass mask of `element op constant` (fast_cmp, qpred.h)
//   find_absent_mask the lane's 8-bit mask of zero presence bytes
//   find_rank        a passer's rank inside its lane from the mask
//   find_lane_valid  how many of a lane's 8 entries lie inside the column (the tail tile)
//   find_lane_wide   may the lane read its whole 8 W bytes?
//   find_row         the CSR row of an entry: an upper-bound search of row_ptr
// Plain functions only: tests/cpp/find_scan_test.cpp compiles this header with the host compiler.
#pragma once
#include <cstdint>

#include "qpred.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NBG_UNROLL _Pragma("unroll")
#else
#define NBG_UNROLL
#endif

namespace nbg {

constexpr int kFindThreads = 256;
constexpr int kFindItems = 8;  // consecutive entries per lane
constexpr int kFindTile = kFindThreads * kFindItems;

// element k (0..7) of a lane's W words, sign-extended to int64 (little-endian, as stored)
template <int W>
NBG_HD int64_t find_elem(const uint64_t* w, int k) {
  if (W == 1) return int64_t(int8_t(w[0] >> (8 * k)));
  if (W == 2) return int64_t(int16_t(w[k >> 2] >> (16 * (k & 3))));
  if (W == 4) return int64_t(int32_t(w[k >> 1] >> (32 * (k & 1))));
  return int64_t(w[k]);
}

// bit k set: element k `op` c holds (k < nvalid; the bits from nvalid up are clear)
template <int W>
NBG_HD uint32_t find_lane_mask(const uint64_t* w, int op, int64_t c, int nvalid = kFindItems) {
  uint32_t m = 0;
  NBG_UNROLL
  for (int k = 0; k < kFindItems; k++)
    if (k < nvalid && fast_cmp(op, find_elem<W>(w, k), c)) m |= 1u << k;
  return m;
}

// bit k set: presence byte k of the 8 bytes in p is zero (k < nvalid)
NBG_HD uint32_t find_absent_mask(uint64_t p, int nvalid = kFindItems) {
  uint32_t m = 0;
  NBG_UNROLL
  for (int k = 0; k < kFindItems; k++)
    if (k < nvalid && ((p >> (8 * k)) & 0xffu) == 0) m |= 1u << k;
  return m;
}

// rank of passer k among the lane's passers: the set bits of m below bit k
NBG_HD int find_rank(uint32_t m, int k) { return __builtin_popcount(m & ((1u << k) - 1u)); }

// entries of the lane starting at entry e0 that lie inside a column of nnz entries: 0..8
NBG_HD int find_lane_valid(int64_t e0, int64_t nnz) {
  const int64_t left = nnz - e0;
  return left <= 0 ? 0 : left >= kFindItems ? kFindItems : int(left);
}
// the lane may read all its 8 W bytes: none of them lies past the column's last element
NBG_HD bool find_lane_wide(int64_t e0, int64_t nnz) { return e0 + kFindItems <= nnz; }
// tiles of a column of nnz entries, and the entries [first, last) of tile t
NBG_HD int64_t find_tiles(int64_t nnz) { return (nnz + kFindTile - 1) / kFindTile; }
NBG_HD int64_t find_tile_end(int64_t t, int64_t nnz) {
  const int64_t e1 = (t + 1) * int64_t(kFindTile);
  return e1 < nnz ? e1 : nnz;
}

// The row of entry e among rows [lo, hi): rp(lo) <= e < rp(hi) must hold (rp(r) = row_ptr[r], the
// first entry of row r; nondecreasing).  Returns the r with rp(r) <= e < rp(r + 1): an upper-bound
// search, so of a run of empty rows that share a start with their non-empty successor it returns
// the successor, never an empty row.
template <typename RowPtr>
NBG_HD int64_t find_row(RowPtr rp, int64_t lo, int64_t hi, int64_t e) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (rp(mid) <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace nbg
