// set_hash.h -- the row hash, the row equality and the open-addressing row table that nbg_set_op
// (setops.hip) and nbg_group_by (group.hip) share; every definition is translation-unit local, as
// in row_gather.h.
//
//   k_set_hash     one 64-bit hash per row (doubles through the ORDER BY canonical encoding,
//                  strings by content); the later kernels read the row itself only on a tag match
//   k_set_build    open addressing, entries (hash tag : 32 | row : 32); a class of equal rows owns
//                  one slot, which ends up holding the class's smallest row number
//   k_set_probe    a keep byte per row: found / not found in the right table (INTERSECT / MINUS),
//                  or "I am my class's first row" (UNION DISTINCT over the concatenation)
//   scan of the keep bytes, k_set_compact -> the kept row numbers, in input order
// Every dependency between workgroups is a kernel boundary: no workgroup waits for another one.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "device_common.h"
#include "engine.h"
#include "order_keys.h"
#include "query_common.h"
#include "row_gather.h"

namespace nbg {
namespace {

constexpr int kSetThreads = 256;
constexpr uint64_t kSetEmpty = ~uint64_t(0);

enum SetKind : int32_t { SK_INT = 0, SK_DOUBLE, SK_BOOL, SK_STRING };

SetKind kind_of(int32_t t) {
  return t == NBG_T_DOUBLE ? SK_DOUBLE : t == NBG_T_BOOL ? SK_BOOL : t == NBG_T_STRING ? SK_STRING : SK_INT;
}

// one column of a table in HBM
struct SetCol {
  const void* data;
  const int64_t* off;  // STRING
  int32_t kind;
  int32_t pad;
};

// ---- row hash and row equality ------------------------------------------------------------------
// the canonical word of a fixed-width value: equal values (under the call's equality) have equal
// words, and for these three kinds the reverse holds too
__device__ __forceinline__ uint64_t canon_word(const SetCol& c, int64_t r) {
  if (c.kind == SK_DOUBLE) return okey::enc_double(static_cast<const double*>(c.data)[r]);
  if (c.kind == SK_BOOL) return okey::enc_bool(static_cast<const uint8_t*>(c.data)[r]);
  return uint64_t(static_cast<const int64_t*>(c.data)[r]);
}

__device__ inline uint64_t set_row_hash(const SetCol* __restrict__ cols, int ncols, int64_t r) {
  uint64_t h = 0x12345678ull;
  for (int c = 0; c < ncols; c++) {
    const SetCol col = cols[c];
    if (col.kind == SK_STRING) {  // by content, 8 bytes a step, then the length
      const int64_t a = col.off[r], len = col.off[r + 1] - a;
      const uint8_t* p = static_cast<const uint8_t*>(col.data) + a;
      for (int64_t ch = 0; ch < okey::str_chunks(len); ch++) h = splitmix64(h ^ okey::enc_str_chunk(p, len, ch));
      h = splitmix64(h ^ okey::enc_str_len(len));
    } else {
      h = splitmix64(h ^ canon_word(col, r));
    }
  }
  return h;
}

// row ra of table A against row rb of table B (the same column kinds on both sides)
__device__ inline bool set_row_eq(const SetCol* __restrict__ A, int64_t ra, const SetCol* __restrict__ B, int64_t rb,
                                  int ncols) {
  for (int c = 0; c < ncols; c++) {
    const SetCol ca = A[c], cb = B[c];
    if (ca.kind == SK_STRING) {
      const int64_t a = ca.off[ra], la = ca.off[ra + 1] - a;
      const int64_t b = cb.off[rb], lb = cb.off[rb + 1] - b;
      if (la != lb) return false;
      const uint8_t* pa = static_cast<const uint8_t*>(ca.data) + a;
      const uint8_t* pb = static_cast<const uint8_t*>(cb.data) + b;
      for (int64_t j = 0; j < la; j++)
        if (pa[j] != pb[j]) return false;
    } else if (canon_word(ca, ra) != canon_word(cb, rb)) {
      return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(kSetThreads) void k_set_hash(const SetCol* __restrict__ cols, int ncols, int64_t n,
                                                          uint64_t mask, uint64_t* __restrict__ hash) {
  for (int64_t i = int64_t(blockIdx.x) * kSetThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kSetThreads)
    hash[i] = set_row_hash(cols, ncols, i) & mask;
}

// A row's chain starts at the COMPLEMENT of its hash's low bits: a hash masked to a few bits
// (option set_hash_bits) then starts at the table's last slots and wraps at once.
__device__ __forceinline__ uint32_t home_slot(uint64_t h, uint32_t capmask) { return uint32_t(~h) & capmask; }
__device__ __forceinline__ uint64_t entry_of(uint64_t h, uint32_t row) { return (h & 0xffffffff00000000ull) | row; }

__device__ __forceinline__ uint64_t slot_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The table has at least twice as many slots as rows are inserted, so a chain always ends at an
// empty slot.  A slot never changes its class once claimed, and every row of a class walks the
// same chain, so the class owns exactly one slot; atomicMin leaves the smallest row there.
__global__ __launch_bounds__(kSetThreads) void k_set_build(const SetCol* __restrict__ cols, int ncols, int64_t n,
                                                           const uint64_t* __restrict__ hash,
                                                           unsigned long long* __restrict__ table, uint32_t capmask) {
  for (int64_t i = int64_t(blockIdx.x) * kSetThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kSetThreads) {
    const uint64_t h = hash[i];
    const uint64_t e = entry_of(h, uint32_t(i));
    uint32_t s = home_slot(h, capmask);
    while (true) {
      uint64_t cur = slot_load(table + s);
      if (cur == kSetEmpty) {
        cur = atomicCAS(table + s, (unsigned long long)kSetEmpty, (unsigned long long)e);
        if (cur == kSetEmpty) break;  // claimed
      }
      if ((cur >> 32) == (e >> 32) && set_row_eq(cols, i, cols, int64_t(cur & 0xffffffffu), ncols)) {
        if (e < cur) atomicMin(table + s, (unsigned long long)e);
        break;
      }
      s = (s + 1) & capmask;
    }
  }
}

enum ProbeMode : int32_t { PM_FOUND = 0, PM_NOT_FOUND = 1, PM_FIRST = 2 };

// keep[i] for i < n, keep[n] = 0 (the scan's last word is then the number of kept rows).
// PM_FOUND / PM_NOT_FOUND: row i of P against the table built over B.  PM_FIRST (P == B, the
// table built over it): keep the row whose number its class's slot holds.
__global__ __launch_bounds__(kSetThreads) void k_set_probe(const SetCol* __restrict__ P, const SetCol* __restrict__ B,
                                                           int ncols, int64_t n, const uint64_t* __restrict__ hash,
                                                           const unsigned long long* __restrict__ table,
                                                           uint32_t capmask, int32_t mode, uint8_t* __restrict__ keep) {
  for (int64_t i = int64_t(blockIdx.x) * kSetThreads + threadIdx.x; i <= n; i += int64_t(gridDim.x) * kSetThreads) {
    if (i == n) {
      keep[i] = 0;
      continue;
    }
    const uint64_t h = hash[i];
    uint32_t s = home_slot(h, capmask);
    bool found = false;
    uint32_t at = 0;
    while (true) {
      const uint64_t cur = table[s];
      if (cur == kSetEmpty) break;
      if ((cur >> 32) == (h >> 32)) {
        at = uint32_t(cur);
        if ((mode == PM_FIRST && int64_t(at) == i) || set_row_eq(P, i, B, int64_t(at), ncols)) {
          found = true;
          break;
        }
      }
      s = (s + 1) & capmask;
    }
    keep[i] = mode == PM_FOUND ? found : mode == PM_NOT_FOUND ? !found : (found && int64_t(at) == i);
  }
}

// idx[pos[i]] = i for every kept row: the kept row numbers in input order
__global__ __launch_bounds__(kSetThreads) void k_set_compact(const uint8_t* __restrict__ keep,
                                                             const uint32_t* __restrict__ pos, int64_t n,
                                                             uint32_t* __restrict__ idx) {
  for (int64_t i = int64_t(blockIdx.x) * kSetThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kSetThreads)
    if (keep[i]) idx[pos[i]] = uint32_t(i);
}

// ---- host ---------------------------------------------------------------------------------------
struct SetTable {
  std::vector<InCol> cols;
  int64_t n = 0;
  DevBuf desc;  // SetCol[ncols]
  std::vector<SetCol> host_desc;
  const SetCol* dev() const { return desc.as<SetCol>(); }

  void describe(Ctx& c) {
    host_desc.clear();
    for (const InCol& ic : cols) host_desc.push_back(SetCol{ic.data, ic.off, int32_t(kind_of(ic.type)), 0});
    if (host_desc.empty()) return;
    desc.alloc(host_desc.size() * sizeof(SetCol));
    NBG_HIP(hipMemcpyAsync(desc.p, host_desc.data(), host_desc.size() * sizeof(SetCol), hipMemcpyHostToDevice, c.stream));
  }
};

struct SetWork {
  Ctx& c;
  const uint64_t mask;
  // `who`: the call's name in the messages ("set_op", "group_by")
  explicit SetWork(Ctx& c_, const char* who = "set_op") : c(c_), mask(hash_mask(c_, who)) {}

  static uint64_t hash_mask(const Ctx& c, const char* who) {
    const int64_t bits = c.opt("set_hash_bits", 64);
    if (bits < 0 || bits > 64)
      throw Error(NBG_E_INVALID_ARG, std::string(who) + ": option set_hash_bits must be in [0, 64]");
    return bits == 64 ? ~uint64_t(0) : (uint64_t(1) << bits) - 1;
  }

  void hash(const SetTable& t, DevBuf& out) {
    if (t.n == 0) return;
    out.alloc(size_t(t.n) * 8);
    k_set_hash<<<grid_for(t.n, kSetThreads), kSetThreads, 0, c.stream>>>(t.dev(), int(t.cols.size()), t.n, mask,
                                                                         out.as<uint64_t>());
    kernel_launched(c);
  }

  // the table over t's rows: capacity = the power of two >= 2 x rows (at least 2)
  uint32_t build(const SetTable& t, const DevBuf& hashes, DevBuf& table) {
    uint64_t cap = 2;
    while (cap < 2 * uint64_t(t.n)) cap <<= 1;
    table.alloc(size_t(cap) * 8);
    NBG_HIP(hipMemsetAsync(table.p, 0xff, size_t(cap) * 8, c.stream));
    if (t.n > 0) {
      k_set_build<<<grid_for(t.n, kSetThreads), kSetThreads, 0, c.stream>>>(
          t.dev(), int(t.cols.size()), t.n, hashes.as<uint64_t>(), table.as<unsigned long long>(), uint32_t(cap - 1));
      kernel_launched(c);
    }
    return uint32_t(cap - 1);
  }

  // the rows of p that `mode` keeps, as row numbers in input order; returns their count (the
  // call's one counter fetch)
  int64_t select(const SetTable& p, const SetTable& b, const DevBuf& hashes, const DevBuf& table, uint32_t capmask,
                 int32_t mode, DevBuf& idx) {
    DevBuf keep, pos;
    keep.alloc(size_t(p.n) + 1);
    pos.alloc((size_t(p.n) + 1) * 4);
    k_set_probe<<<grid_for(p.n + 1, kSetThreads), kSetThreads, 0, c.stream>>>(
        p.dev(), b.dev(), int(p.cols.size()), p.n, hashes.as<uint64_t>(), table.as<unsigned long long>(), capmask, mode,
        keep.as<uint8_t>());
    kernel_launched(c);
    exclusive_scan_dev(c, keep.as<uint8_t>(), pos.as<uint32_t>(), p.n + 1);
    c.timing.launches++;
    uint32_t kept = 0;
    NBG_HIP(hipMemcpyAsync(&kept, pos.as<uint32_t>() + p.n, 4, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    c.timing.host_waits++;
    if (kept > 0) {
      idx.alloc(size_t(kept) * 4 + 16);
      k_set_compact<<<grid_for(p.n, kSetThreads), kSetThreads, 0, c.stream>>>(keep.as<uint8_t>(), pos.as<uint32_t>(),
                                                                              p.n, idx.as<uint32_t>());
      kernel_launched(c);
    }
    return int64_t(kept);
  }
};

}  // namespace
}  // namespace nbg
