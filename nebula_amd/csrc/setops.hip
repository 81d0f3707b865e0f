// setops.hip -- UNION / INTERSECT / MINUS on result tables (nbg_set_op): device hash set operators.
//
// Replaces SetExecutor::doUnion / doDistinct / doIntersect / doMinus (src/graph/SetExecutor.cpp:
// 143-328: a sort + unique, and two nested loops over the rows) with one hash build and one probe.
// DESIGN.md section 3 "Set operators" has the byte model and the determinism argument.
//
//   k_set_cast     a right column whose type differs from the left's, cast to the left's type
//   k_set_hash, k_set_build, k_set_probe, the scan of the keep bytes and k_set_compact
//                  (set_hash.h, shared with group.hip) -> the kept row numbers, in input order
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
#include "set_hash.h"

namespace nbg {
namespace {

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

// UNION: the right table's STRING offsets behind the left's: out[j] = off[j] + base, j in [0, n]
// (off == nullptr: a right table without rows, out[0] = base)
__global__ __launch_bounds__(kSetThreads) void k_set_off_rebase(const int64_t* __restrict__ off, int64_t n, int64_t base,
                                                                int64_t* __restrict__ out) {
  for (int64_t j = int64_t(blockIdx.x) * kSetThreads + threadIdx.x; j <= n; j += int64_t(gridDim.x) * kSetThreads)
    out[j] = (off ? off[j] : 0) + base;
}

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
