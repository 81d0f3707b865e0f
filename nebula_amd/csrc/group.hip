// group.hip -- GROUP BY with COUNT / SUM / AVG / MIN / MAX on a result table (nbg_group_by).
//
// The reference (v1.0.0-beta) has no GROUP BY; the semantics are this build's (DESIGN.md
// divergence 13, section 3 "GROUP BY" has the byte models).
//
// Group ids: the key columns are hashed and entered into set_hash.h's row table, whose slot of a
// class of equal key tuples ends up holding the class's first row.
//   k_grp_rep      every row's representative (that first row) and a first-occurrence byte
//   scan of the bytes -> G (the call's one counter fetch) and each first row's group number
//   k_grp_gid      gid[i] = pos[rep[i]], and the first rows' numbers in input order, by which the
//                  key columns are gathered (row_gather.h)
// Path A (no SUM / AVG over DOUBLE): every accumulator is one uint64 word per group and every
// operator is exact and order-free (group_agg.h), so rows add themselves with atomics:
//   k_grp_init     the identities
//   k_grp_accum    a thread takes four consecutive rows (one 16-byte load of gid, 16-byte loads of
//                  the value columns), joins neighbours of the same group in registers and issues
//                  64-bit atomics: into LDS first when G x words fits (then one global atomic per
//                  touched word and workgroup), else straight into HBM
//   k_grp_finish   the words decoded into the typed output columns
// Path B (a SUM / AVG over DOUBLE, or option group_sorted = 1): no float atomics anywhere.
//   the rows in a stable order by gid (ORDER BY's radix sort, order_rows_by_u32)
//   k_grp_seg_off  each group's first position in that order
//   k_grp_seg_lane / _wave   a segment of up to 16 / 4096 rows is reduced by a lane / a wave
//   k_grp_nchunks, scan, k_grp_seg_chunk, k_grp_seg_join   a longer one is cut into chunks of
//                  16384 rows, a workgroup reduces each chunk, and one joins the segment's chunks
//                  The class is chosen by the segment's length alone and the tree is group_agg.h's
//                  fixed one; every aggregate of the call goes through the same kernels and is
//                  written typed at once
// Every dependency between workgroups is a kernel boundary: no workgroup waits for another one.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "device_common.h"
#include "engine.h"
#include "group_agg.h"
#include "order_keys.h"
#include "query_common.h"
#include "row_gather.h"
#include "rows.h"
#include "set_hash.h"

namespace nbg {
namespace {

constexpr int kGrpThreads = 256;
constexpr int kGrpWaves = kGrpThreads / 64;
constexpr int kMaxAggs = 16;
constexpr int64_t kLdsWords = 4096;     // 32 KiB of LDS accumulators a workgroup at most
constexpr int64_t kLdsMaxDefault = 1024;  // option group_lds_max (profiles/group.md)

// one aggregate of the call
struct AggCol {
  const void* data;  // the value column (nullptr: COUNT)
  void* out;         // the typed output column, one value per group
  int32_t fn;        // NBG_AGG_*
  int32_t kind;      // SK_* of the value column
  int32_t op;        // agg::Op of its accumulator word
  int32_t word;      // path A: its accumulator array (0: the shared row count)
};
struct AggCols {
  AggCol a[kMaxAggs];
  int32_t wop[kMaxAggs + 1];  // path A: operator of accumulator array w
  int32_t n, nw;
};

// ---- group ids ----------------------------------------------------------------------------------
// rep[i] = the row its class's slot holds (the class's first row); first[i] = (rep[i] == i),
// first[n] = 0 (the scan's last word is then the number of groups)
__global__ __launch_bounds__(kGrpThreads) void k_grp_rep(const SetCol* __restrict__ K, int ncols, int64_t n,
                                                         const uint64_t* __restrict__ hash,
                                                         const unsigned long long* __restrict__ table,
                                                         uint32_t capmask, uint32_t* __restrict__ rep,
                                                         uint8_t* __restrict__ first) {
  for (int64_t i = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; i <= n; i += int64_t(gridDim.x) * kGrpThreads) {
    if (i == n) {
      first[i] = 0;
      continue;
    }
    const uint64_t h = hash[i];
    uint32_t s = home_slot(h, capmask);
    uint32_t at = uint32_t(i);
    while (true) {
      const uint64_t cur = table[s];
      if (cur == kSetEmpty) break;  // (not reached: the build entered every row)
      if ((cur >> 32) == (h >> 32)) {
        const uint32_t r = uint32_t(cur);
        if (int64_t(r) == i || set_row_eq(K, i, K, int64_t(r), ncols)) {
          at = r;
          break;
        }
      }
      s = (s + 1) & capmask;
    }
    rep[i] = at;
    first[i] = int64_t(at) == i;
  }
}

// rep_gid[i]: in the representative, out the group number (only thread i touches word i);
// idx[g] = group g's first row
__global__ __launch_bounds__(kGrpThreads) void k_grp_gid(uint32_t* __restrict__ rep_gid, const uint8_t* __restrict__ first,
                                                         const uint32_t* __restrict__ pos, int64_t n,
                                                         uint32_t* __restrict__ idx) {
  for (int64_t i = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kGrpThreads) {
    const uint32_t g = pos[rep_gid[i]];
    rep_gid[i] = g;
    if (first[i]) idx[g] = uint32_t(i);
  }
}

// ---- values and results -------------------------------------------------------------------------
// row r's value as the accumulator word its operator combines
__device__ __forceinline__ uint64_t word_of(int32_t op, int32_t kind, uint64_t raw) {
  if (op == agg::OP_ADD_I64 || op == agg::OP_ADD_F64) return raw;
  if (kind == SK_DOUBLE) return okey::enc_double(agg::dval(raw));
  if (kind == SK_BOOL) return okey::enc_bool(uint8_t(raw));
  return okey::enc_int(int64_t(raw));
}
__device__ __forceinline__ uint64_t load_raw(const AggCol& a, int64_t r) {
  return a.kind == SK_BOOL ? uint64_t(static_cast<const uint8_t*>(a.data)[r]) : static_cast<const uint64_t*>(a.data)[r];
}

// group g's result of aggregate a from its word and its row count
__device__ __forceinline__ void write_result(const AggCol& a, int64_t g, uint64_t w, uint64_t count) {
  uint64_t* o64 = static_cast<uint64_t*>(a.out);
  switch (a.fn) {
    case NBG_AGG_COUNT: o64[g] = count; break;
    case NBG_AGG_SUM: o64[g] = w; break;  // the int64 sum, or the double's bits
    case NBG_AGG_AVG:
      o64[g] = agg::dbits(a.kind == SK_DOUBLE ? agg::avg_double(agg::dval(w), count) : agg::avg_int(int64_t(w), count));
      break;
    default:  // MIN / MAX
      if (a.kind == SK_BOOL) static_cast<uint8_t*>(a.out)[g] = agg::dec_bool(w);
      else if (a.kind == SK_DOUBLE) o64[g] = agg::dbits(agg::dec_double(w));
      else o64[g] = uint64_t(okey::dec_int(w));
  }
}

// ---- path A -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGrpThreads) void k_grp_init(AggCols A, int64_t G, unsigned long long* __restrict__ acc) {
  const int64_t total = int64_t(A.nw) * G;
  for (int64_t j = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; j < total; j += int64_t(gridDim.x) * kGrpThreads)
    acc[j] = agg::identity(A.wop[j / G]);
}

__device__ __forceinline__ void atomic_word(int32_t op, unsigned long long* p, uint64_t v) {
  if (op == agg::OP_ADD_I64) atomicAdd(p, (unsigned long long)v);
  else if (op == agg::OP_MIN_U64) atomicMin(p, (unsigned long long)v);
  else atomicMax(p, (unsigned long long)v);
}

// the atomics of four consecutive rows into dst[w * G + g]: neighbours of one group are joined first
__device__ __forceinline__ void add_quad(int32_t op, unsigned long long* dst, const uint32_t* g, const uint64_t* v, int m) {
  int e = 0;
  while (e < m) {
    uint64_t acc = v[e];
    int f = e + 1;
    while (f < m && g[f] == g[e]) acc = agg::combine(op, acc, v[f++]);
    atomic_word(op, dst + g[e], acc);
    e = f;
  }
}

// gid == nullptr: every row is in group 0.  LDS: the workgroup's own accumulators (A.nw * G words
// of dynamic LDS) take the rows, and every touched one goes to HBM once at the end.
template <bool LDS>
__global__ __launch_bounds__(kGrpThreads) void k_grp_accum(AggCols A, const uint32_t* __restrict__ gid, int64_t n,
                                                           int64_t G, unsigned long long* __restrict__ acc) {
  extern __shared__ unsigned long long lacc[];
  const int total = LDS ? int(A.nw * G) : 0;
  if (LDS) {
    for (int j = threadIdx.x; j < total; j += kGrpThreads) lacc[j] = agg::identity(A.wop[j / int(G)]);
    __syncthreads();
  }
  unsigned long long* dst = LDS ? lacc : acc;
  const int64_t quads = (n + 3) / 4;
  for (int64_t q = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; q < quads; q += int64_t(gridDim.x) * kGrpThreads) {
    const int64_t i0 = q * 4;
    const int m = int(min(int64_t(4), n - i0));
    uint32_t g[4] = {0, 0, 0, 0};
    if (gid) {
      if (m == 4) {
        const uint4 t = *reinterpret_cast<const uint4*>(gid + i0);
        g[0] = t.x, g[1] = t.y, g[2] = t.z, g[3] = t.w;
      } else {
        for (int e = 0; e < m; e++) g[e] = gid[i0 + e];
      }
    }
    uint64_t v[4] = {1, 1, 1, 1};
    add_quad(agg::OP_ADD_I64, dst, g, v, m);  // array 0: the row count
    for (int k = 0; k < A.n; k++) {
      const AggCol a = A.a[k];
      if (a.word == 0) continue;  // COUNT
      if (a.kind == SK_BOOL) {
        const uint8_t* p = static_cast<const uint8_t*>(a.data);
        if (m == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
          const uchar4 t = *reinterpret_cast<const uchar4*>(p + i0);
          v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
          for (int e = 0; e < m; e++) v[e] = p[i0 + e];
        }
      } else {
        const uint64_t* p = static_cast<const uint64_t*>(a.data);
        if (m == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
          const ulonglong2 t0 = *reinterpret_cast<const ulonglong2*>(p + i0);
          const ulonglong2 t1 = *reinterpret_cast<const ulonglong2*>(p + i0 + 2);
          v[0] = t0.x, v[1] = t0.y, v[2] = t1.x, v[3] = t1.y;
        } else {
          for (int e = 0; e < m; e++) v[e] = p[i0 + e];
        }
      }
      for (int e = 0; e < m; e++) v[e] = word_of(a.op, a.kind, v[e]);
      add_quad(a.op, dst + int64_t(a.word) * G, g, v, m);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < total; j += kGrpThreads) {
      const int32_t op = A.wop[j / int(G)];
      const uint64_t w = lacc[j];
      if (w != agg::identity(op)) atomic_word(op, acc + j, w);  // (an untouched word holds the identity)
    }
  }
}

__global__ __launch_bounds__(kGrpThreads) void k_grp_finish(AggCols A, int64_t G,
                                                            const unsigned long long* __restrict__ acc) {
  for (int64_t g = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; g < G; g += int64_t(gridDim.x) * kGrpThreads) {
    const uint64_t count = acc[g];
    for (int k = 0; k < A.n; k++) write_result(A.a[k], g, acc[int64_t(A.a[k].word) * G + g], count);
  }
}

// ---- path B -------------------------------------------------------------------------------------
// idx: the rows ordered by gid (nullptr: the input order); seg_off[g] = the first position of group
// g, seg_off[G] = n.  Every group has a row, so every word is written.
__global__ __launch_bounds__(kGrpThreads) void k_grp_seg_off(const uint32_t* __restrict__ gid,
                                                             const uint32_t* __restrict__ idx, int64_t n, int64_t G,
                                                             uint32_t* __restrict__ seg_off) {
  for (int64_t j = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; j <= n; j += int64_t(gridDim.x) * kGrpThreads) {
    if (j == n) {
      seg_off[G] = uint32_t(n);
      continue;
    }
    const uint32_t g = gid ? gid[idx ? idx[j] : j] : 0;
    if (j == 0 || (gid && g != gid[idx ? idx[j - 1] : j - 1])) seg_off[g] = uint32_t(j);
  }
}

// the segment's values (positions [a, a + len) of the order) as lane `lane` of `width` adds them
__device__ __forceinline__ uint64_t seg_partial(const AggCol& c, const uint32_t* __restrict__ idx, int64_t a, int64_t len,
                                                int lane, int width) {
  return agg::strided_partial(
      c.op,
      [&](int64_t j) {
        const int64_t r = idx ? int64_t(idx[a + j]) : a + j;
        return word_of(c.op, c.kind, load_raw(c, r));
      },
      len, lane, width);
}

// group_agg.h's halve64 across the wave: lane 0 ends with the tree's root
__device__ __forceinline__ uint64_t wave_halve(int32_t op, uint64_t v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t t = __shfl_down((unsigned long long)v, o);
    v = agg::combine(op, v, t);
  }
  return v;
}

__global__ __launch_bounds__(kGrpThreads) void k_grp_seg_lane(AggCols A, const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ seg_off, int64_t G) {
  for (int64_t g = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; g < G; g += int64_t(gridDim.x) * kGrpThreads) {
    const int64_t a = seg_off[g], len = int64_t(seg_off[g + 1]) - a;
    if (agg::seg_class(len) != 0) continue;
    for (int k = 0; k < A.n; k++) {
      const AggCol c = A.a[k];
      write_result(c, g, c.data ? seg_partial(c, idx, a, len, 0, 1) : 0, uint64_t(len));
    }
  }
}

// A wave looks at 64 groups a step and takes those of its class one after the other.  spread = 0:
// the 64 are consecutive (coalesced reads of seg_off; for many groups); spread = 1: they lie one
// wave count apart, so that a few groups still go to as many waves.
__global__ __launch_bounds__(kGrpThreads) void k_grp_seg_wave(AggCols A, const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ seg_off, int64_t G,
                                                              int32_t spread) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = int64_t(gridDim.x) * kGrpWaves, wave = int64_t(blockIdx.x) * kGrpWaves + threadIdx.x / 64;
  for (int64_t step = 0; step * nwaves * 64 < G; step++) {  // wave-uniform
    const int64_t mine = step * nwaves * 64 + (spread ? lane * nwaves + wave : wave * 64 + lane);
    int64_t a = 0, len = 0;
    if (mine < G) {
      a = seg_off[mine];
      len = int64_t(seg_off[mine + 1]) - a;
    }
    uint64_t todo = __ballot(agg::seg_class(len) == 1);
    while (todo) {  // wave-uniform
      const int b = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t sa = __shfl((long long)a, b), sl = __shfl((long long)len, b), sg = __shfl((long long)mine, b);
      for (int k = 0; k < A.n; k++) {
        const AggCol c = A.a[k];
        uint64_t w = 0;
        if (c.data) w = wave_halve(c.op, seg_partial(c, idx, sa, sl, lane, 64));
        if (lane == 0) write_result(c, sg, w, uint64_t(sl));
      }
    }
  }
}

// group_agg.h's block_reduce across the workgroup: every thread brings its partial word and
// every thread gets the root
__device__ __forceinline__ uint64_t block_tree(int32_t op, uint64_t partial, uint64_t* wsum) {
  const uint64_t w = wave_halve(op, partial);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x / 64] = w;
  __syncthreads();
  const uint64_t r = agg::combine(op, agg::combine(op, wsum[0], wsum[1]), agg::combine(op, wsum[2], wsum[3]));
  __syncthreads();  // wsum is rewritten by the next call
  return r;
}

// nch[g] = the chunks of a segment of the third class (0 for the others), nch[G] = 0: its scan
// numbers the call's chunks, and the scan's last word is their count
__global__ __launch_bounds__(kGrpThreads) void k_grp_nchunks(const uint32_t* __restrict__ seg_off, int64_t G,
                                                             uint32_t* __restrict__ nch) {
  for (int64_t g = int64_t(blockIdx.x) * kGrpThreads + threadIdx.x; g <= G; g += int64_t(gridDim.x) * kGrpThreads) {
    const int64_t len = g < G ? int64_t(seg_off[g + 1]) - int64_t(seg_off[g]) : 0;
    nch[g] = agg::seg_class(len) == 2 ? uint32_t(agg::seg_chunks(len)) : 0;
  }
}

// a workgroup per chunk: part[k * max_chunks + chunk] = the chunk's word of aggregate k
__global__ __launch_bounds__(kGrpThreads) void k_grp_seg_chunk(AggCols A, const uint32_t* __restrict__ idx,
                                                               const uint32_t* __restrict__ seg_off,
                                                               const uint32_t* __restrict__ choff, int64_t G,
                                                               uint64_t* __restrict__ part, int64_t max_chunks) {
  __shared__ uint64_t wsum[kGrpWaves];
  const int64_t total = min(int64_t(choff[G]), max_chunks);  // (never more: the host's bound holds)
  for (int64_t ch = blockIdx.x; ch < total; ch += gridDim.x) {  // workgroup-uniform
    // the segment of chunk ch: the last g with choff[g] <= ch (a segment without chunks repeats
    // its successor's number, so that one has chunks)
    int64_t lo = 0, hi = G;  // choff[lo] <= ch < choff[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) / 2;
      if (int64_t(choff[mid]) <= ch) lo = mid;
      else hi = mid;
    }
    const int64_t at = int64_t(seg_off[lo]) + (ch - int64_t(choff[lo])) * agg::kSegChunk;
    const int64_t len = min(agg::kSegChunk, int64_t(seg_off[lo + 1]) - at);
    for (int k = 0; k < A.n; k++) {
      const AggCol c = A.a[k];
      if (!c.data) continue;
      const uint64_t r = block_tree(c.op, seg_partial(c, idx, at, len, threadIdx.x, kGrpThreads), wsum);
      if (threadIdx.x == 0) part[int64_t(k) * max_chunks + ch] = r;
    }
  }
}

// a workgroup looks at 256 groups a step and joins the chunk words of those of the third class
__global__ __launch_bounds__(kGrpThreads) void k_grp_seg_join(AggCols A, const uint32_t* __restrict__ seg_off,
                                                              const uint32_t* __restrict__ choff, int64_t G,
                                                              const uint64_t* __restrict__ part, int64_t max_chunks) {
  __shared__ uint8_t todo[kGrpThreads];
  __shared__ uint64_t wsum[kGrpWaves];
  const int tid = threadIdx.x;
  for (int64_t base = int64_t(blockIdx.x) * kGrpThreads; base < G; base += int64_t(gridDim.x) * kGrpThreads) {
    const int64_t mine = base + tid;
    todo[tid] = mine < G && choff[mine + 1] != choff[mine];
    __syncthreads();
    for (int b = 0; b < kGrpThreads; b++) {
      if (!todo[b]) continue;  // workgroup-uniform
      const int64_t g = base + b, first = choff[g], nchunks = min(int64_t(choff[g + 1]), max_chunks) - first;
      const uint64_t len = uint64_t(seg_off[g + 1]) - uint64_t(seg_off[g]);
      for (int k = 0; k < A.n; k++) {
        const AggCol c = A.a[k];
        uint64_t r = 0;
        if (c.data) {
          const uint64_t* words = part + int64_t(k) * max_chunks + first;
          r = block_tree(c.op, agg::strided_partial(c.op, [&](int64_t j) { return words[j]; }, nchunks, tid, kGrpThreads),
                         wsum);
        }
        if (tid == 0) write_result(c, g, r, len);
      }
    }
    __syncthreads();  // todo is rewritten by the next step
  }
}

// ---- host ---------------------------------------------------------------------------------------
struct GroupPlan {
  std::vector<int32_t> keys;                    // key column indices
  std::vector<std::pair<int32_t, int32_t>> aggs;  // (fn, col)
  std::vector<int32_t> out_types;
  bool double_sum = false;
};

int32_t group_by_impl(Ctx& c, const nbg_rows& in, const GroupPlan& plan, bool keep_on_device, nbg_rows* out) {
  const int64_t n = in.n_rows;
  const size_t nk = plan.keys.size(), na = plan.aggs.size(), ncols = nk + na;
  const bool sorted = plan.double_sum || c.opt("group_sorted", 0) != 0;
  const int64_t lds_max = c.opt("group_lds_max", kLdsMaxDefault);
  NBG_HIP(hipEventRecord(c.ev[0], c.stream));

  std::vector<DevBuf> up;
  const std::vector<InCol> cols = upload_table(c, in, up, "group_by");

  auto h = std::make_unique<HostRows>();
  h->types = plan.out_types;
  h->dev.resize(ncols);
  std::vector<DevBuf> out_off(ncols);
  std::vector<int64_t> str_bytes(ncols, 0);
  int64_t G = 0;

  if (n > 0) {
    // ---- group ids ----
    DevBuf gid_buf, order;
    const uint32_t* gid = nullptr;  // nullptr: one group
    G = 1;
    if (nk > 0) {
      SetTable kt;
      kt.n = n;
      for (int32_t k : plan.keys) kt.cols.push_back(cols[size_t(k)]);
      kt.describe(c);
      SetWork w(c, "group_by");
      DevBuf hashes, table, first, pos, idx;
      w.hash(kt, hashes);
      const uint32_t capmask = w.build(kt, hashes, table);
      gid_buf.alloc(size_t(n) * 4 + 16);
      first.alloc(size_t(n) + 1);
      pos.alloc((size_t(n) + 1) * 4);
      k_grp_rep<<<grid_for(n + 1, kGrpThreads), kGrpThreads, 0, c.stream>>>(
          kt.dev(), int(nk), n, hashes.as<uint64_t>(), table.as<unsigned long long>(), capmask, gid_buf.as<uint32_t>(),
          first.as<uint8_t>());
      kernel_launched(c);
      exclusive_scan_dev(c, first.as<uint8_t>(), pos.as<uint32_t>(), n + 1);
      c.timing.launches++;
      uint32_t groups = 0;
      NBG_HIP(hipMemcpyAsync(&groups, pos.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipStreamSynchronize(c.stream));
      c.timing.host_waits++;
      G = int64_t(groups);
      idx.alloc(size_t(G) * 4 + 16);
      k_grp_gid<<<grid_for(n, kGrpThreads), kGrpThreads, 0, c.stream>>>(gid_buf.as<uint32_t>(), first.as<uint8_t>(),
                                                                       pos.as<uint32_t>(), n, idx.as<uint32_t>());
      kernel_launched(c);
      gid = gid_buf.as<uint32_t>();
      // the key columns of each group's first row (a repeated key column is gathered again)
      std::vector<DevBuf> kdev(nk), koff(nk);
      gather_rows(c, kt.cols, idx.as<uint32_t>(), G, kdev, koff);
      for (size_t k = 0; k < nk; k++) {
        h->dev[k] = std::move(kdev[k]);
        out_off[k] = std::move(koff[k]);
        str_bytes[k] = kt.cols[k].str_bytes;
      }
      // (hashes, table, first, pos, idx return to the pool here; stream order keeps the reuse safe)
    }

    // ---- the aggregates ----
    if (na > 0) {
      AggCols A{};
      A.n = int32_t(na);
      A.nw = 1;
      A.wop[0] = agg::OP_ADD_I64;
      for (size_t k = 0; k < na; k++) {
        AggCol& a = A.a[k];
        const int32_t fn = plan.aggs[k].first;
        const int32_t t = plan.out_types[nk + k];
        h->dev[nk + k].alloc(size_t(G) * (t == NBG_T_BOOL ? 1 : 8));
        a.out = h->dev[nk + k].p;
        a.fn = fn;
        if (fn == NBG_AGG_COUNT) {
          a.data = nullptr, a.kind = SK_INT, a.op = agg::OP_ADD_I64, a.word = 0;
          continue;
        }
        const InCol& ic = cols[size_t(plan.aggs[k].second)];
        a.data = ic.data;
        a.kind = kind_of(ic.type);
        a.op = fn == NBG_AGG_MIN   ? agg::OP_MIN_U64
               : fn == NBG_AGG_MAX ? agg::OP_MAX_U64
               : a.kind == SK_DOUBLE ? agg::OP_ADD_F64
                                     : agg::OP_ADD_I64;
        a.word = A.nw;
        A.wop[A.nw++] = a.op;
      }
      if (!sorted) {
        DevBuf acc;
        acc.alloc(size_t(A.nw) * size_t(G) * 8);
        k_grp_init<<<grid_for(int64_t(A.nw) * G, kGrpThreads), kGrpThreads, 0, c.stream>>>(
            A, G, acc.as<unsigned long long>());
        kernel_launched(c);
        const int64_t quads = (n + 3) / 4;
        if (G <= lds_max && int64_t(A.nw) * G <= kLdsWords) {
          // (at most four workgroups a CU: each one ends with up to nw * G global atomics)
          k_grp_accum<true><<<grid_for(quads, kGrpThreads, 1024), kGrpThreads, size_t(A.nw) * size_t(G) * 8, c.stream>>>(
              A, gid, n, G, acc.as<unsigned long long>());
        } else {
          k_grp_accum<false><<<grid_for(quads, kGrpThreads), kGrpThreads, 0, c.stream>>>(A, gid, n, G,
                                                                                         acc.as<unsigned long long>());
        }
        kernel_launched(c);
        k_grp_finish<<<grid_for(G, kGrpThreads), kGrpThreads, 0, c.stream>>>(A, G, acc.as<unsigned long long>());
        kernel_launched(c);
      } else {
        const uint32_t* idx = nullptr;
        if (gid && G > 1 && order_rows_by_u32(c, gid, n, order)) idx = order.as<uint32_t>();
        DevBuf seg_off;
        seg_off.alloc((size_t(G) + 1) * 4);
        k_grp_seg_off<<<grid_for(n + 1, kGrpThreads), kGrpThreads, 0, c.stream>>>(gid, idx, n, G, seg_off.as<uint32_t>());
        kernel_launched(c);
        k_grp_seg_lane<<<grid_for(G, kGrpThreads), kGrpThreads, 0, c.stream>>>(A, idx, seg_off.as<uint32_t>(), G);
        kernel_launched(c);
        // (which classes occur is not known on the host without a wait: the two kernels below
        // read 4 B per group and return where they find nothing; n bounds the lengths)
        if (n > agg::kSegLane) {
          // at most 2048 workgroups; a wave per group while the groups are fewer than the waves
          const int grid = grid_for(G, kGrpWaves, 2048);
          const int32_t spread = G < int64_t(grid) * kGrpThreads;
          k_grp_seg_wave<<<grid, kGrpThreads, 0, c.stream>>>(A, idx, seg_off.as<uint32_t>(), G, spread);
          kernel_launched(c);
        }
        if (n > agg::kSegWave) {
          // a segment of the third class has more than kSegWave rows and at most one chunk more
          // than len / kSegChunk, which bounds the call's chunks
          const int64_t max_chunks = n / agg::kSegChunk + n / (agg::kSegWave + 1) + 1;
          DevBuf nch, choff, part;
          nch.alloc((size_t(G) + 1) * 4);
          choff.alloc((size_t(G) + 1) * 4);
          part.alloc(size_t(A.n) * size_t(max_chunks) * 8);
          k_grp_nchunks<<<grid_for(G + 1, kGrpThreads), kGrpThreads, 0, c.stream>>>(seg_off.as<uint32_t>(), G,
                                                                                   nch.as<uint32_t>());
          kernel_launched(c);
          exclusive_scan_dev<uint32_t>(c, nch.as<uint32_t>(), choff.as<uint32_t>(), G + 1);
          c.timing.launches++;
          k_grp_seg_chunk<<<grid_for(max_chunks, 1), kGrpThreads, 0, c.stream>>>(
              A, idx, seg_off.as<uint32_t>(), choff.as<uint32_t>(), G, part.as<uint64_t>(), max_chunks);
          kernel_launched(c);
          k_grp_seg_join<<<grid_for(G, kGrpThreads, 1024), kGrpThreads, 0, c.stream>>>(
              A, seg_off.as<uint32_t>(), choff.as<uint32_t>(), G, part.as<uint64_t>(), max_chunks);
          kernel_launched(c);
        }
      }
    }
  }
  if (G == 0)
    for (size_t k = 0; k < ncols; k++) h->dev[k].alloc(8);
  NBG_HIP(hipEventRecord(c.ev[1], c.stream));
  c.total_pending = true;

  hand_out_rows(c, std::move(h), out_off, str_bytes, G, keep_on_device, out);
  out->edges_scanned = in.edges_scanned;
  return NBG_OK;
}

}  // namespace

int32_t group_by_run(Ctx& c, const nbg_rows& in, const int32_t* key_cols, size_t n_keys, const int32_t* agg_fns,
                     const int32_t* agg_cols, size_t n_aggs, int32_t keep_on_device, nbg_rows* out) {
  check_plain_table(in, "group_by");
  if (keep_on_device != 0 && keep_on_device != 1) throw Error(NBG_E_INVALID_ARG, "group_by: keep_on_device must be 0 or 1");
  if (n_keys == 0 && n_aggs == 0) throw Error(NBG_E_INVALID_ARG, "group_by: neither a key nor an aggregate");
  if (n_keys + n_aggs > size_t(kMaxAggs))
    throw Error(NBG_E_UNSUPPORTED, "group_by: a result has at most 16 columns");
  GroupPlan plan;
  for (size_t k = 0; k < n_keys; k++) {
    if (key_cols[k] < 0 || key_cols[k] >= in.n_cols) throw Error(NBG_E_INVALID_ARG, "group_by: key column index out of range");
    plan.keys.push_back(key_cols[k]);
    plan.out_types.push_back(in.col_types[key_cols[k]]);
  }
  for (size_t k = 0; k < n_aggs; k++) {
    const int32_t fn = agg_fns[k];
    if (fn < NBG_AGG_SUM || fn > NBG_AGG_MAX) throw Error(NBG_E_INVALID_ARG, "group_by: unknown aggregate function");
    if (fn == NBG_AGG_COUNT) {
      plan.aggs.emplace_back(fn, -1);
      plan.out_types.push_back(NBG_T_INT);
      continue;
    }
    const int32_t col = agg_cols[k];
    if (col < 0 || col >= in.n_cols) throw Error(NBG_E_INVALID_ARG, "group_by: aggregate column index out of range");
    const int32_t t = in.col_types[col];
    if (fn == NBG_AGG_SUM || fn == NBG_AGG_AVG) {
      // validOperation (QueryStatsProcessor): SUM / AVG need a numeric column
      if (t == NBG_T_BOOL || t == NBG_T_STRING)
        throw Error(NBG_E_IMPROPER_DATA_TYPE, "group_by: SUM / AVG over a BOOL or STRING column");
      plan.double_sum |= t == NBG_T_DOUBLE;
      plan.out_types.push_back(fn == NBG_AGG_AVG || t == NBG_T_DOUBLE ? NBG_T_DOUBLE : NBG_T_INT);
    } else {
      if (t == NBG_T_STRING) throw Error(NBG_E_UNSUPPORTED, "group_by: MIN / MAX over a STRING column");
      plan.out_types.push_back(t);
    }
    plan.aggs.emplace_back(fn, col);
  }
  if (uint64_t(in.n_rows) >= (uint64_t(1) << 32)) throw Error(NBG_E_UNSUPPORTED, "group_by: 2^32 rows or more");
  const int64_t lds_max = c.opt("group_lds_max", 0);
  const int64_t force = c.opt("group_sorted", 0);
  if (lds_max < 0 || (force != 0 && force != 1))
    throw Error(NBG_E_INVALID_ARG, "group_by: option group_lds_max must be >= 0 and group_sorted 0 or 1");

  PoolScope pool_scope(query_pool(c));
  c.timing = Timing{};
  timing_reset(c);
  c.total_pending = false;
  try {
    return group_by_impl(c, in, plan, keep_on_device != 0, out);
  } catch (...) {
    // no launch or copy may still use a block this call frees on the way out
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
}

}  // namespace nbg
