// yield.hip -- YIELD and DISTINCT over result rows (processFinalResult, GoExecutor.cpp:585-782):
// k_materialize runs one program per output column over a (src, edge) row list, STRING columns are
// packed (str_offsets, str_pack), whole rows are de-duplicated through a hash table (dedup_rows)
// after meeting on one rank (shuffle_rows).  GO (traverse.hip) calls the steps; FETCH PROP
// (fetch.hip) calls yield_rows, getBound (bound.hip) column_result_type.
#include <algorithm>
#include <vector>

#include "device_common.h"
#include "engine.h"
#include "expr_device.h"
#include "go_launch.h"
#include "program.h"
#include "query_common.h"

namespace nbg {

__global__ void k_flag_dest(const uint32_t* dest, int64_t n, uint32_t p, uint8_t* flag) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    flag[i] = dest[i] == p;
}

// gidx list (local indices + lo) -> vids
__global__ void k_local_to_vid(const int32_t* loc, int64_t n, int64_t lo, const int64_t* vid_of, int64_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = vid_of[lo + loc[i]];
}

// EDGE = false (FETCH PROP ON a tag): a row is a vertex; rows_edge and env.col are never read
template <bool EDGE = true>
__global__ void k_materialize(const int32_t* rows_src, const int64_t* rows_edge, int64_t n, const Program* progs,
                              YieldArgs ya, EvalEnv env, int64_t lo, unsigned long long* err) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t ge = EDGE ? rows_edge[i] : 0;
    const int32_t sg = int32_t(lo) + rows_src[i];
    const int32_t dg = EDGE ? env.col[ge] : sg;
    for (int c = 0; c < ya.ncols; c++) {
      Val v = eval_program(progs + c, env, ge, sg, dg);
      if (v.t == VT_ERR || v.t != ya.cols[c].type) {
        atomicAdd(err, 1ull);
        continue;
      }
      if (v.t == VT_BOOL) static_cast<uint8_t*>(ya.cols[c].data)[i] = uint8_t(v.b != 0);
      else static_cast<int64_t*>(ya.cols[c].data)[i] = v.b;
      if (v.t == VT_STR) ya.cols[c].len[i] = v.len;
    }
  }
}
// STRING YIELD columns: (address, length) per row -> packed bytes at exclusive-scan offsets
__global__ void k_str_pack(const int64_t* addr, const int64_t* off, int64_t n, uint8_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const uint8_t* s = reinterpret_cast<const uint8_t*>(uintptr_t(addr[i]));
    const int64_t len = off[i + 1] - off[i];
    for (int64_t j = 0; j < len; j++) out[off[i] + j] = s[j];
  }
}
// fast path for YIELD e._dst (the default YIELD)
__global__ void k_yield_dst(const int64_t* rows_edge, int64_t n, const int32_t* col, const int64_t* vid_of,
                            int64_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = vid_of[col[rows_edge[i]]];
}

// DISTINCT over materialised rows (GoExecutor.cpp:638-646 dedups by encoded row bytes; for the
// fixed-width VID/DOUBLE/BOOL columns the engine emits, equal bytes == equal 64-bit words).
__device__ inline uint64_t row_hash(const YieldArgs& ya, int64_t i) {
  uint64_t h = 0x12345678ull;
  for (int c = 0; c < ya.ncols; c++) {
    uint64_t w;
    if (ya.cols[c].type == VT_STR) {  // by content: equal strings may sit at different addresses
      const uint8_t* p = reinterpret_cast<const uint8_t*>(uintptr_t(static_cast<const int64_t*>(ya.cols[c].data)[i]));
      const int64_t len = ya.cols[c].len[i];
      w = 0xcbf29ce484222325ull ^ uint64_t(len);
      for (int64_t k = 0; k < len; k++) w = (w ^ p[k]) * 0x100000001b3ull;
    } else {
      w = ya.cols[c].type == VT_BOOL ? static_cast<const uint8_t*>(ya.cols[c].data)[i]
                                     : uint64_t(static_cast<const int64_t*>(ya.cols[c].data)[i]);
    }
    h = splitmix64(h ^ w);
  }
  return h;
}
__device__ inline bool row_eq(const YieldArgs& ya, int64_t i, int64_t j) {
  for (int c = 0; c < ya.ncols; c++) {
    if (ya.cols[c].type == VT_STR) {
      const int64_t li = ya.cols[c].len[i];
      if (li != ya.cols[c].len[j]) return false;
      const uint8_t* a = reinterpret_cast<const uint8_t*>(uintptr_t(static_cast<const int64_t*>(ya.cols[c].data)[i]));
      const uint8_t* b = reinterpret_cast<const uint8_t*>(uintptr_t(static_cast<const int64_t*>(ya.cols[c].data)[j]));
      for (int64_t k = 0; k < li; k++)
        if (a[k] != b[k]) return false;
    } else if (ya.cols[c].type == VT_BOOL) {
      if (static_cast<const uint8_t*>(ya.cols[c].data)[i] != static_cast<const uint8_t*>(ya.cols[c].data)[j]) return false;
    } else if (static_cast<const int64_t*>(ya.cols[c].data)[i] != static_cast<const int64_t*>(ya.cols[c].data)[j]) {
      return false;
    }
  }
  return true;
}
__global__ void k_row_dedup(YieldArgs ya, int64_t n, long long* table, uint64_t mask, uint8_t* keep) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    uint64_t h = row_hash(ya, i) & mask;
    bool k = true;
    while (true) {
      long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(table + h), ~0ull, (unsigned long long)i);
      if (prev == -1) break;
      if (row_eq(ya, prev, i)) {
        k = false;
        break;
      }
      h = (h + 1) & mask;
    }
    keep[i] = k;
  }
}

__global__ void k_row_dest(YieldArgs ya, int64_t n, uint32_t G, uint32_t* dest) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    dest[i] = uint32_t((row_hash(ya, i) >> 17) % G);
}

// the rows per destination rank (shuffle_rows)
namespace {
__global__ void k_hist_dest(const uint32_t* dest, int64_t n, int G, unsigned long long* counts) {
  __shared__ unsigned int h[64];
  if (threadIdx.x < 64) h[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    atomicAdd(&h[dest[i]], 1u);
  __syncthreads();
  if (threadIdx.x < unsigned(G) && h[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)h[threadIdx.x]);
}
}  // namespace

// ------------------------------------------------------------------------------------------
// host drivers
// ------------------------------------------------------------------------------------------
void launch_materialize(Ctx& c, const int32_t* rows_src, const int64_t* rows_edge, int64_t n, const Program* progs,
                        const YieldArgs& ya, const EvalEnv& env, int64_t lo, unsigned long long* err) {
  if (rows_edge) k_materialize<true><<<grid_cap(n), 256, 0, c.stream>>>(rows_src, rows_edge, n, progs, ya, env, lo, err);
  else k_materialize<false><<<grid_cap(n), 256, 0, c.stream>>>(rows_src, nullptr, n, progs, ya, env, lo, err);
}
void launch_yield_dst(Ctx& c, const int64_t* rows_edge, int64_t n, const int32_t* col, int64_t* out) {
  k_yield_dst<<<grid_cap(n), 256, 0, c.stream>>>(rows_edge, n, col, c.vid_of.as<int64_t>(), out);
}
void launch_local_to_vid(Ctx& c, const int32_t* loc, int64_t n, int64_t lo, int64_t* out) {
  k_local_to_vid<<<grid_cap(n), 256, 0, c.stream>>>(loc, n, lo, c.vid_of.as<int64_t>(), out);
}
void str_offsets(Ctx& c, const int64_t* len, int64_t n, DevBuf& off, int64_t* total) {
  off.alloc(size_t(n + 1) * 8);
  exclusive_scan_dev<int64_t>(c, len, off.as<int64_t>(), n + 1);
  NBG_HIP(hipMemcpyAsync(total, off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c.stream));
}
bool str_pack(Ctx& c, const int64_t* addr, const int64_t* off, int64_t n, int64_t total, DevBuf& bytes) {
  bytes.alloc(size_t(total) + 8);
  if (!n || !total) return false;
  k_str_pack<<<grid_cap(n), 256, 0, c.stream>>>(addr, off, n, bytes.as<uint8_t>());
  NBG_HIP(hipGetLastError());
  return true;
}

// DISTINCT with several ranks: every row goes to rank hash(row) % G (all copies of a row meet
// on one rank), then the local dedup runs as with one rank.  Returns the received row count.
int64_t shuffle_rows(Ctx& c, YieldArgs& ya, std::vector<DevBuf>& cols, int64_t n) {
  CommTimer t(c);
  const size_t G = size_t(c.world);
  if (G > 64) throw Error(NBG_E_UNSUPPORTED, "more than 64 ranks");
  DevBuf dest, flag, cnt, dcounts;
  dest.alloc(size_t(n + 1) * 4);
  flag.alloc(size_t(n + 1));
  cnt.alloc(8);
  dcounts.alloc(G * G * 8 + 8);
  NBG_HIP(hipMemsetAsync(dcounts.p, 0, G * 8, c.stream));
  if (n) {
    k_row_dest<<<grid_cap(n), 256, 0, c.stream>>>(ya, n, uint32_t(G), dest.as<uint32_t>());
    k_hist_dest<<<grid_cap(n), 256, 0, c.stream>>>(dest.as<uint32_t>(), n, int(G), dcounts.as<unsigned long long>());
  }
  std::vector<int64_t> all(G * G);
  DevBuf dall;
  dall.alloc(G * G * 8);
  comm_allgather_bytes(c, dcounts.p, G * 8, dall.p);
  NBG_HIP(hipMemcpyAsync(all.data(), dall.p, G * G * 8, hipMemcpyDeviceToHost, c.stream));
  host_sync(c);
  const size_t me = size_t(c.rank);
  std::vector<int64_t> soff(G + 1, 0), roff(G + 1, 0);
  for (size_t p = 0; p < G; p++) {
    soff[p + 1] = soff[p] + all[me * G + p];
    roff[p + 1] = roff[p] + all[p * G + me];
  }
  const int64_t R = roff[G];
  std::vector<DevBuf> send(cols.size()), recv(cols.size());
  for (size_t cc = 0; cc < cols.size(); cc++) {
    size_t w = ya.cols[cc].type == VT_BOOL ? 1 : 8;
    send[cc].alloc(size_t(n + 1) * w);
    recv[cc].alloc(size_t(R + 1) * w);
  }
  for (size_t p = 0; p < G && n; p++) {
    if (!all[me * G + p]) continue;
    k_flag_dest<<<grid_cap(n), 256, 0, c.stream>>>(dest.as<uint32_t>(), n, uint32_t(p), flag.as<uint8_t>());
    for (size_t cc = 0; cc < cols.size(); cc++) {
      if (ya.cols[cc].type == VT_BOOL) {
        uint8_t* o = send[cc].as<uint8_t>() + soff[p];
        select_dev(c, cols[cc].as<uint8_t>(), flag.as<uint8_t>(), o, cnt.as<uint64_t>(), n);
      } else {
        int64_t* o = send[cc].as<int64_t>() + soff[p];
        select_dev(c, cols[cc].as<int64_t>(), flag.as<uint8_t>(), o, cnt.as<uint64_t>(), n);
      }
    }
  }
  for (size_t cc = 0; cc < cols.size(); cc++) {
    size_t w = ya.cols[cc].type == VT_BOOL ? 1 : 8;
    std::vector<size_t> sb(G), so(G), rb(G), ro(G);
    for (size_t p = 0; p < G; p++) {
      sb[p] = size_t(soff[p + 1] - soff[p]) * w;
      so[p] = size_t(soff[p]) * w;
      rb[p] = size_t(roff[p + 1] - roff[p]) * w;
      ro[p] = size_t(roff[p]) * w;
    }
    comm_alltoallv_bytes(c, send[cc].p, sb.data(), so.data(), recv[cc].p, rb.data(), ro.data());
    c.timing.comm_bytes += uint64_t(n - (soff[me + 1] - soff[me])) * w;
  }
  host_sync(c);
  for (size_t cc = 0; cc < cols.size(); cc++) {
    cols[cc] = std::move(recv[cc]);
    ya.cols[cc].data = cols[cc].p;
  }
  return R;
}

// the NBG_T_* column type of a program's VT_* result
int32_t result_type(int32_t vt) {
  return vt == VT_DOUBLE ? NBG_T_DOUBLE : vt == VT_BOOL ? NBG_T_BOOL : vt == VT_STR ? NBG_T_STRING : NBG_T_VID;
}
// the type a stored column is returned as: FLOAT widens to DOUBLE, VID and TIMESTAMP are INTs
int32_t column_result_type(int32_t t) {
  return t == NBG_T_FLOAT ? NBG_T_DOUBLE : (t == NBG_T_VID || t == NBG_T_TIMESTAMP) ? NBG_T_INT : t;
}

static_assert(kMaxYields == kMaxYieldCols, "query_common.h states YieldArgs' column count");
// The YIELD materialiser for callers outside GO (fetch.hip): programs over a (rows_src, rows_edge)
// list, STRING columns packed.  One host wait: the error count and the STRING byte totals together.
void yield_rows(Ctx& c, const std::vector<Program>& progs, const EvalEnv& env, const int32_t* rows_src,
                const int64_t* rows_edge, int64_t lo, int64_t n, const char* err_what, YieldOut& out) {
  const size_t ny = progs.size();
  out.types.clear();
  out.dev.clear();
  out.off.clear();
  out.dev.resize(ny);
  out.off.resize(ny);
  out.str_bytes.assign(ny, 0);
  for (const Program& p : progs) out.types.push_back(result_type(p.result_type));
  if (n == 0) {
    for (size_t k = 0; k < ny; k++) out.dev[k].alloc(8);
    return;
  }
  DevBuf dprog, cnt;
  dprog.alloc(sizeof(Program) * ny);
  c.h2d(dprog.p, progs.data(), sizeof(Program) * ny);
  cnt.alloc(8);
  NBG_HIP(hipMemsetAsync(cnt.p, 0, 8, c.stream));
  std::vector<DevBuf> slen(ny), addr(ny);
  YieldArgs ya{};
  ya.ncols = int32_t(ny);
  for (size_t k = 0; k < ny; k++) {
    const int32_t t = progs[k].result_type;
    DevBuf& b = t == VT_STR ? addr[k] : out.dev[k];
    b.alloc(size_t(n + 1) * (t == VT_BOOL ? 1 : 8));
    if (t == VT_STR) {
      // (a row whose evaluation fails writes nothing: zero lengths keep the scan below defined)
      slen[k].alloc(size_t(n + 1) * 8);
      NBG_HIP(hipMemsetAsync(slen[k].p, 0, size_t(n + 1) * 8, c.stream));
    }
    ya.cols[k] = ColOut{b.p, t, slen[k].as<int64_t>()};
  }
  launch_materialize(c, rows_src, rows_edge, n, dprog.as<Program>(), ya, env, lo, cnt.as<unsigned long long>());
  NBG_HIP(hipGetLastError());
  c.timing.launches++;
  std::vector<int64_t> totals(ny + 1, 0);
  for (size_t k = 0; k < ny; k++) {
    if (progs[k].result_type != VT_STR) continue;
    str_offsets(c, slen[k].as<int64_t>(), n, out.off[k], &totals[k]);
    c.timing.launches++;
  }
  NBG_HIP(hipMemcpyAsync(&totals[ny], cnt.p, 8, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  c.timing.host_waits++;
  c.host_stage_used = 0;
  if (totals[ny]) throw Error(NBG_E_EVAL, err_what);
  for (size_t k = 0; k < ny; k++) {
    if (progs[k].result_type != VT_STR) continue;
    out.str_bytes[k] = totals[k];
    if (str_pack(c, addr[k].as<int64_t>(), out.off[k].as<int64_t>(), n, totals[k], out.dev[k])) c.timing.launches++;
  }
}

// DISTINCT over whole rows: a hash table keeps one row of each value, then every column (and
// STRING length column) is compacted by the keep flags
int64_t dedup_rows(Ctx& c, YieldArgs& ya, std::vector<DevBuf>& cols, std::vector<DevBuf>& slen, int64_t nrows) {
  uint64_t cap = 1024;
  while (cap < uint64_t(2 * nrows)) cap <<= 1;
  for (size_t cc = 0; cc < cols.size(); cc++) ya.cols[cc].data = cols[cc].p;
  DevBuf table, keep, idx, cnt;
  table.alloc(cap * 8);
  NBG_HIP(hipMemsetAsync(table.p, 0xff, cap * 8, c.stream));
  keep.alloc(size_t(nrows));
  k_row_dedup<<<grid_cap(nrows), 256, 0, c.stream>>>(ya, nrows, table.as<long long>(), cap - 1, keep.as<uint8_t>());
  cnt.alloc(8);
  int64_t kept = 0;
  for (size_t cc = 0; cc < cols.size(); cc++) {
    DevBuf nb;
    bool is_bool = ya.cols[cc].type == VT_BOOL;
    nb.alloc(size_t(nrows + 1) * (is_bool ? 1 : 8));
    if (is_bool)
      select_dev(c, cols[cc].as<uint8_t>(), keep.as<uint8_t>(), nb.as<uint8_t>(), cnt.as<uint64_t>(), nrows);
    else
      select_dev(c, cols[cc].as<int64_t>(), keep.as<uint8_t>(), nb.as<int64_t>(), cnt.as<uint64_t>(), nrows);
    if (ya.cols[cc].type == VT_STR) {
      DevBuf nl;
      nl.alloc(size_t(nrows + 1) * 8);
      select_dev(c, slen[cc].as<int64_t>(), keep.as<uint8_t>(), nl.as<int64_t>(), cnt.as<uint64_t>(), nrows);
      slen[cc] = std::move(nl);
    }
    uint64_t kc = 0;
    NBG_HIP(hipMemcpyAsync(&kc, cnt.p, 8, hipMemcpyDeviceToHost, c.stream));
    host_sync(c);
    kept = int64_t(kc);
    cols[cc] = std::move(nb);
  }
  return kept;
}

}  // namespace nbg
