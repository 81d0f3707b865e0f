// setops.hip -- UNION / INTERSECT / MINUS on result tables (nbg_set_op): device hash set operators.
//
// Replaces SetExecutor::doUnion / doDistinct / doIntersect / doMinus (src/graph/SetExecutor.cpp:
// 143-328: a sort + unique, and two nested loops over the rows) with one hash build and one probe.
// DESIGN.md section 3 "Set operators" has the byte model and the determinism argument.
//
//   k_set_cast     a right column whose type differs from the left's, cast to the left's type
//   k_set_hash     one 64-bit hash per row (doubles through the ORDER BY canonical encoding,
//                  strings by content); the later kernels read the row itself only on a tag match
//   k_set_build    open addressing, entries (hash tag : 32 | row : 32); a class of equal rows owns
//                  one slot, which ends up holding the class's smallest row number
//   k_set_probe    a keep byte per row: found / not found in the right table (INTERSECT / MINUS),
//                  or "I am my class's first row" (UNION DISTINCT over the concatenation)
//   scan of the keep bytes, k_set_compact -> the kept row numbers, in input order
// and the output columns are gathered by that index (row_gather.h).  Every dependency between
// workgroups is one of these kernel boundaries: no workgroup waits for another one.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "device_common.h"
#include "engine.h"
#include "order_keys.h"
#include "query_common.h"
#include "row_gather.h"
#include "rows.h"

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

// ---- casts (InterimResult::castTo, InterimResult.cpp:215-347) -----------------------------------
// double -> int64 saturates and NaN becomes 0 (undefined in the reference's static_cast)
__device__ __forceinline__ int64_t cast_d2i(double v) {
  if (v != v) return 0;
  if (v >= 9223372036854775808.0) return INT64_MAX;
  if (v <= -9223372036854775808.0) return INT64_MIN;
  return int64_t(v);
}

__global__ __launch_bounds__(kSetThreads) void k_set_cast(const void* __restrict__ src, void* __restrict__ dst, int64_t n,
                                                          int32_t from, int32_t to) {
  for (int64_t i = int64_t(blockIdx.x) * kSetThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kSetThreads) {
    if (from == SK_INT) {
      const int64_t v = static_cast<const int64_t*>(src)[i];
      if (to == SK_DOUBLE) static_cast<double*>(dst)[i] = double(v);
      else static_cast<uint8_t*>(dst)[i] = v != 0;
    } else if (from == SK_DOUBLE) {
      const double v = static_cast<const double*>(src)[i];
      if (to == SK_INT) static_cast<int64_t*>(dst)[i] = cast_d2i(v);
      else static_cast<uint8_t*>(dst)[i] = v != 0;
    } else {
      const uint8_t v = static_cast<const uint8_t*>(src)[i];
      if (to == SK_INT) static_cast<int64_t*>(dst)[i] = v ? 1 : 0;
      else static_cast<double*>(dst)[i] = v ? 1.0 : 0.0;
    }
  }
}

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

// UNION: the right table's STRING offsets behind the left's: out[j] = off[j] + base, j in [0, n]
// (off == nullptr: a right table without rows, out[0] = base)
__global__ __launch_bounds__(kSetThreads) void k_set_off_rebase(const int64_t* __restrict__ off, int64_t n, int64_t base,
                                                                int64_t* __restrict__ out) {
  for (int64_t j = int64_t(blockIdx.x) * kSetThreads + threadIdx.x; j <= n; j += int64_t(gridDim.x) * kSetThreads)
    out[j] = (off ? off[j] : 0) + base;
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
  explicit SetWork(Ctx& c_) : c(c_), mask(hash_mask(c_)) {}

  static uint64_t hash_mask(const Ctx& c) {
    const int64_t bits = c.opt("set_hash_bits", 64);
    if (bits < 0 || bits > 64) throw Error(NBG_E_INVALID_ARG, "set_op: option set_hash_bits must be in [0, 64]");
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

// right column k in the left's type (a cast column lives in `ws`)
void cast_right(Ctx& c, SetTable& right, const std::vector<int32_t>& types, std::vector<DevBuf>& ws) {
  for (size_t k = 0; k < types.size(); k++) {
    InCol& rc = right.cols[k];
    const SetKind from = kind_of(rc.type), to = kind_of(types[k]);
    rc.type = types[k];
    if (from == to || right.n == 0) continue;
    DevBuf b;
    b.alloc(size_t(right.n) * (to == SK_BOOL ? 1 : 8));
    k_set_cast<<<grid_for(right.n, kSetThreads), kSetThreads, 0, c.stream>>>(rc.data, b.p, right.n, from, to);
    kernel_launched(c);
    rc.data = b.p;
    ws.push_back(std::move(b));
  }
}

// left's rows, then right's: device-to-device column copies into `dev` (and out_off for STRING)
void concat(Ctx& c, const SetTable& l, const SetTable& r, std::vector<DevBuf>& dev, std::vector<DevBuf>& out_off,
            std::vector<int64_t>& str_bytes) {
  const int64_t n = l.n + r.n;
  for (size_t k = 0; k < l.cols.size(); k++) {
    const InCol& a = l.cols[k];
    const InCol& b = r.cols[k];
    if (a.type == NBG_T_STRING) {
      str_bytes[k] = a.str_bytes + b.str_bytes;
      dev[k].alloc(size_t(str_bytes[k]) + 8);
      out_off[k].alloc(size_t(n + 1) * 8);
      if (a.str_bytes) NBG_HIP(hipMemcpyAsync(dev[k].p, a.data, size_t(a.str_bytes), hipMemcpyDeviceToDevice, c.stream));
      if (b.str_bytes)
        NBG_HIP(hipMemcpyAsync(dev[k].as<uint8_t>() + a.str_bytes, b.data, size_t(b.str_bytes), hipMemcpyDeviceToDevice,
                               c.stream));
      if (l.n) NBG_HIP(hipMemcpyAsync(out_off[k].p, a.off, size_t(l.n + 1) * 8, hipMemcpyDeviceToDevice, c.stream));
      k_set_off_rebase<<<grid_for(r.n + 1, kSetThreads), kSetThreads, 0, c.stream>>>(r.n ? b.off : nullptr, r.n, a.str_bytes,
                                                                                     out_off[k].as<int64_t>() + l.n);
      kernel_launched(c);
      continue;
    }
    const size_t w = a.type == NBG_T_BOOL ? 1 : 8;
    dev[k].alloc(size_t(n) * w);
    if (l.n) NBG_HIP(hipMemcpyAsync(dev[k].p, a.data, size_t(l.n) * w, hipMemcpyDeviceToDevice, c.stream));
    if (r.n)
      NBG_HIP(hipMemcpyAsync(dev[k].as<uint8_t>() + size_t(l.n) * w, b.data, size_t(r.n) * w, hipMemcpyDeviceToDevice,
                             c.stream));
  }
}

int32_t set_op_impl(Ctx& c, int32_t op, const nbg_rows& lin, const nbg_rows& rin, const std::vector<int32_t>& types,
                    bool distinct, bool keep_on_device, nbg_rows* out) {
  const size_t ncols = types.size();
  NBG_HIP(hipEventRecord(c.ev[0], c.stream));

  std::vector<DevBuf> up, ws;
  SetTable left, right;
  left.n = lin.n_rows;
  right.n = rin.n_rows;
  // (a side without columns is the reference's nullptr result: no rows, the other side's schema)
  if (lin.n_cols) left.cols = upload_table(c, lin, up, "set_op");
  else left.cols.resize(ncols);
  if (rin.n_cols) right.cols = upload_table(c, rin, up, "set_op");
  else right.cols.resize(ncols);
  for (size_t k = 0; k < ncols; k++) {
    if (!lin.n_cols) left.cols[k].type = types[k];
    if (!rin.n_cols) right.cols[k].type = types[k];
  }
  cast_right(c, right, types, ws);

  auto h = std::make_unique<HostRows>();
  h->types = types;
  h->dev.resize(ncols);
  std::vector<DevBuf> out_off(ncols);
  std::vector<int64_t> str_bytes(ncols, 0);
  SetWork w(c);
  int64_t n_out = 0;

  if (op == NBG_SET_UNION) {
    const int64_t n = left.n + right.n;
    if (n > 0 && !distinct) {
      concat(c, left, right, h->dev, out_off, str_bytes);
      n_out = n;
    } else if (n > 0) {
      // the concatenation in the workspace, then the first row of every class
      SetTable cat;
      std::vector<DevBuf> cat_dev(ncols), cat_off(ncols);
      concat(c, left, right, cat_dev, cat_off, str_bytes);
      cat.n = n;
      cat.cols.resize(ncols);
      for (size_t k = 0; k < ncols; k++)
        cat.cols[k] = InCol{types[k], cat_dev[k].p, cat_off[k].as<int64_t>(), str_bytes[k]};
      cat.describe(c);
      DevBuf hashes, table, idx;
      w.hash(cat, hashes);
      const uint32_t capmask = w.build(cat, hashes, table);
      n_out = w.select(cat, cat, hashes, table, capmask, PM_FIRST, idx);
      if (n_out > 0) gather_rows(c, cat.cols, idx.as<uint32_t>(), n_out, h->dev, out_off);
      // (cat_dev / cat_off / idx return to the pool here; stream order keeps the reuse safe)
    }
  } else if (left.n > 0) {
    left.describe(c);
    right.describe(c);
    DevBuf hl, hr, table, idx;
    w.hash(right, hr);
    const uint32_t capmask = w.build(right, hr, table);
    w.hash(left, hl);
    n_out = w.select(left, right, hl, table, capmask, op == NBG_SET_INTERSECT ? PM_FOUND : PM_NOT_FOUND, idx);
    for (size_t k = 0; k < ncols; k++) str_bytes[k] = left.cols[k].str_bytes;
    if (n_out > 0) gather_rows(c, left.cols, idx.as<uint32_t>(), n_out, h->dev, out_off);
  }
  if (n_out == 0) {
    for (size_t k = 0; k < ncols; k++) {
      h->dev[k].alloc(8);
      str_bytes[k] = 0;
    }
  }
  NBG_HIP(hipEventRecord(c.ev[1], c.stream));
  c.total_pending = true;

  hand_out_rows(c, std::move(h), out_off, str_bytes, n_out, keep_on_device, out);
  out->edges_scanned = lin.edges_scanned + rin.edges_scanned;
  return NBG_OK;
}

}  // namespace

// FETCH PROP ON ... DISTINCT (fetch.hip) deduplicates its keys and its rows with the UNION DISTINCT
// machinery: hash, build, probe PM_FIRST over the one table
int64_t distinct_first_rows(Ctx& c, const std::vector<TableCol>& cols, int64_t n, DevBuf& idx) {
  SetTable t;
  t.n = n;
  for (const TableCol& tc : cols) t.cols.push_back(InCol{tc.type, tc.data, tc.off, tc.str_bytes});
  t.describe(c);
  SetWork w(c);
  DevBuf hashes, table;
  w.hash(t, hashes);
  const uint32_t capmask = w.build(t, hashes, table);
  return w.select(t, t, hashes, table, capmask, PM_FIRST, idx);
}

int32_t set_op_run(Ctx& c, int32_t op, const nbg_rows& left, const nbg_rows& right, int32_t distinct,
                   int32_t keep_on_device, nbg_rows* out) {
  if (op != NBG_SET_UNION && op != NBG_SET_INTERSECT && op != NBG_SET_MINUS)
    throw Error(NBG_E_INVALID_ARG, "set_op: op must be NBG_SET_UNION, NBG_SET_INTERSECT or NBG_SET_MINUS");
  if (distinct != 0 && distinct != 1) throw Error(NBG_E_INVALID_ARG, "set_op: distinct must be 0 or 1");
  check_plain_table(left, "set_op");
  check_plain_table(right, "set_op");
  // checkSchema (SetExecutor.cpp:188-218); a side with neither columns nor rows adopts the other's
  const bool lnull = left.n_cols == 0 && left.n_rows == 0, rnull = right.n_cols == 0 && right.n_rows == 0;
  if (!lnull && !rnull && left.n_cols != right.n_cols) throw Error(NBG_E_INVALID_ARG, "Field count not match.");
  if ((left.n_cols == 0 && left.n_rows) || (right.n_cols == 0 && right.n_rows))
    throw Error(NBG_E_INVALID_ARG, "set_op: a table with rows needs columns");
  const nbg_rows& schema = lnull ? right : left;
  std::vector<int32_t> types(schema.col_types, schema.col_types + schema.n_cols);
  if (!lnull && !rnull)
    for (int32_t k = 0; k < left.n_cols; k++) {
      const int32_t a = left.col_types[k], b = right.col_types[k];
      if ((a == NBG_T_STRING) != (b == NBG_T_STRING))
        throw Error(NBG_E_UNSUPPORTED, "set_op: column " + std::to_string(k) + " needs a cast to or from STRING");
    }
  if (uint64_t(left.n_rows) + uint64_t(right.n_rows) >= (uint64_t(1) << 32))
    throw Error(NBG_E_UNSUPPORTED, "set_op: 2^32 rows or more");

  PoolScope pool_scope(query_pool(c));
  c.timing = Timing{};
  timing_reset(c);
  c.total_pending = false;
  try {
    return set_op_impl(c, op, left, right, types, distinct != 0, keep_on_device != 0, out);
  } catch (...) {
    // no launch or copy may still use a block this call frees on the way out
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
}

}  // namespace nbg
