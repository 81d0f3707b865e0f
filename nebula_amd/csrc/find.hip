// find.hip -- FIND props FROM tag / edge WHERE (nbg_find_vertices, nbg_find_edges): the device column
// scan that answers "which vertices / which edges have a property like this".
//
// The reference parses the sentence (FindSentence, src/parser/TraverseSentences.h:83-113) and
// answers "Does not support" (src/graph/FindExecutor.cpp:20-22); the semantics here are this
// build's (divergence 12; section 3c has the byte model).
//
// Edges, fast path (WHERE = int prop REL int constant, classify_pred's PK_FAST):
//   k_find_count<W>   a tile = 2048 consecutive entries of the column, 8 per lane read as 8-byte /
//                     16-byte loads; one pass count per tile, no atomics
//   scan              exclusive scan of the tile counts; its total is the match count
//   k_find_emit<W>    tiles with passers again: rank inside the tile (wave prefix + per-wave bases
//                     in LDS), the entry and its row (upper-bound search of the tile's row_ptr
//                     slice staged in LDS) to rows_edge / rows_src at base + rank
// Edges, general path (any other WHERE, none, or option find_fast = 0): expand.hip's EXP_FLAGS
// expansion over the identity frontier of the rows, rocprim::select of the flagged slots.
// Vertices: k_find_vflag (state, ownership, the WHERE program per column index), select.
// Both orders are ascending by position, so the rows are the same on every run and path.
// Then yield.hip's materialiser and the hand-out, as FETCH PROP ON (fetch.hip).
#include <hip/hip_runtime.h>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>

#include "call_common.h"
#include "device_common.h"
#include "engine.h"
#include "expr_device.h"
#include "find_scan.h"
#include "go_launch.h"
#include "program.h"
#include "query_common.h"
#include "row_gather.h"
#include "rows.h"

namespace nbg {
namespace {

constexpr int kFindGrid = 2048;  // blocks at most; a block strides over tiles
constexpr int kFindWaves = kFindThreads / kWave;

struct FindScan {
  const void* data;        // the column, W bytes per entry
  const uint8_t* present;  // or null: every entry has the field
  int64_t nnz;
  int32_t op;  // fast_cmp
  int64_t k;
  const int64_t* row_ptr;  // [n_rows + 1]
  int64_t n_rows;
  const uint8_t* row_ok;    // or null: every row visible
  const int32_t* tile_row;  // [tiles + 1]: the row holding each tile's first entry (k_tile_rows)
  uint32_t* tile_cnt;       // count: [tiles + 1], the last one 0
  unsigned long long* stats;  // count: [0] evaluation errors, [1] tiles with passers
  const uint64_t* tile_base;  // emit: exclusive scan of tile_cnt
  int64_t* rows_edge;
  int32_t* rows_src;
};

// The pass and absent masks of the lane whose 8 entries start at e0.  A whole lane issues all its
// loads (the column's 8 W bytes, the 8 presence bytes) before the first compare; a lane that
// crosses the column's end reads its entries one by one and none past the last.
template <int W>
__device__ __forceinline__ void lane_masks(const FindScan& a, int64_t e0, uint32_t& pass, uint32_t& absent) {
  pass = 0;
  absent = 0;
  const int nv = find_lane_valid(e0, a.nnz);
  if (nv == 0) return;
  if (find_lane_wide(e0, a.nnz)) {
    uint64_t w[W];
    const char* p = static_cast<const char*>(a.data) + e0 * W;
    if constexpr (W == 1) {
      w[0] = *reinterpret_cast<const uint64_t*>(p);
    } else {
      ulonglong2 v[W / 2];
#pragma unroll
      for (int j = 0; j < W / 2; j++) v[j] = reinterpret_cast<const ulonglong2*>(p)[j];
#pragma unroll
      for (int j = 0; j < W / 2; j++) w[2 * j] = v[j].x, w[2 * j + 1] = v[j].y;
    }
    const uint64_t pr = a.present ? *reinterpret_cast<const uint64_t*>(a.present + e0) : ~uint64_t(0);
    pass = find_lane_mask<W>(w, a.op, a.k);
    absent = find_absent_mask(pr);
  } else {
    for (int k = 0; k < nv; k++) {
      const bool ab = a.present && !a.present[e0 + k];
      absent |= uint32_t(ab) << k;
      pass |= uint32_t(fast_cmp(a.op, load_int(a.data, W, e0 + k), a.k)) << k;
    }
  }
  pass &= ~absent;
}

// The rows of tile t: s_hdr = {first row, row count}; their row_ptr slice (count + 1 words) in LDS
// when it fits, else the searches read row_ptr itself (a run of empty rows under one tile).
__device__ __forceinline__ void stage_rows(const FindScan& a, int64_t t, int64_t* s_rp, int64_t* s_hdr) {
  if (threadIdx.x == 0) {
    int64_t i0, cnt;
    tile_entries(a.tile_row, a.row_ptr, a.n_rows, t, find_tile_end(t, a.nnz), a.nnz, i0, cnt);
    s_hdr[0] = i0;
    s_hdr[1] = cnt;
  }
  __syncthreads();
  const int64_t i0 = s_hdr[0], cnt = s_hdr[1];
  if (cnt <= kFindTile)
    for (int k = threadIdx.x; k <= int(cnt); k += kFindThreads) s_rp[k] = a.row_ptr[i0 + k];
  __syncthreads();
}
__device__ __forceinline__ int64_t tile_row_of(const FindScan& a, const int64_t* s_rp, const int64_t* s_hdr, int64_t e) {
  const int64_t i0 = s_hdr[0], cnt = s_hdr[1];
  if (cnt <= kFindTile) return i0 + find_row([&](int64_t r) { return s_rp[r]; }, 0, cnt, e);
  return find_row([&](int64_t r) { return a.row_ptr[r]; }, i0, i0 + cnt, e);
}

// ROWS (row_ok exists): an entry of a hidden row is no candidate: it neither passes nor fails the
// call, so passers and absent entries resolve their row here too.
template <int W, bool ROWS>
__global__ __launch_bounds__(kFindThreads) void k_find_count(FindScan a) {
  __shared__ int64_t s_rp[ROWS ? kFindTile + 1 : 1];
  __shared__ int64_t s_hdr[2];
  __shared__ uint32_t s_w[2][kFindWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t ntiles = find_tiles(a.nnz);
  unsigned long long errs = 0, nonempty = 0;
  int par = 0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t e0 = t * kFindTile + int64_t(threadIdx.x) * kFindItems;
    uint32_t pass, absent;
    lane_masks<W>(a, e0, pass, absent);
    if constexpr (ROWS) {
      stage_rows(a, t, s_rp, s_hdr);
      uint32_t m = pass | absent;
      while (m) {
        const int k = __ffs(m) - 1;
        m &= m - 1;
        if (!a.row_ok[tile_row_of(a, s_rp, s_hdr, e0 + k)]) pass &= ~(1u << k), absent &= ~(1u << k);
      }
    }
    errs += __popc(absent);
    uint32_t c = __popc(pass);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) s_w[par][wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
      for (int w = 0; w < kFindWaves; w++) tot += s_w[par][w];
      a.tile_cnt[t] = tot;
      nonempty += tot != 0;
    }
    par ^= 1;
    if constexpr (ROWS) __syncthreads();  // the next tile's slice replaces s_rp
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.tile_cnt[ntiles] = 0;
  errs = wave_sum_u64(errs);
  if (lane == 0 && errs) atomicAdd(a.stats, errs);
  if (threadIdx.x == 0 && nonempty) atomicAdd(a.stats + 1, nonempty);
}

template <int W, bool ROWS>
__global__ __launch_bounds__(kFindThreads) void k_find_emit(FindScan a) {
  __shared__ int64_t s_rp[kFindTile + 1];
  __shared__ int64_t s_hdr[2];
  __shared__ uint32_t s_w[kFindWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t ntiles = find_tiles(a.nnz);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = a.tile_base[t];
    if (a.tile_base[t + 1] == base) continue;  // (the whole block: no passer in the tile)
    const int64_t e0 = t * kFindTile + int64_t(threadIdx.x) * kFindItems;
    uint32_t pass, absent;
    lane_masks<W>(a, e0, pass, absent);
    stage_rows(a, t, s_rp, s_hdr);
    int32_t rr[kFindItems];
#pragma unroll
    for (int k = 0; k < kFindItems; k++) {
      rr[k] = 0;
      if (pass >> k & 1u) {
        rr[k] = int32_t(tile_row_of(a, s_rp, s_hdr, e0 + k));
        if (ROWS && !a.row_ok[rr[k]]) pass &= ~(1u << k);
      }
    }
    const uint32_t c0 = __popc(pass);
    uint32_t incl = c0;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    if (lane == kWave - 1) s_w[wv] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wv; w++) wbase += s_w[w];
    const uint64_t pos = base + wbase + (incl - c0);
#pragma unroll
    for (int k = 0; k < kFindItems; k++)
      if (pass >> k & 1u) {
        const uint64_t at = pos + uint64_t(find_rank(pass, k));
        a.rows_edge[at] = e0 + k;
        a.rows_src[at] = rr[k];
      }
    __syncthreads();  // the next tile's slice replaces s_rp, its sums s_w
  }
}

// ---- general path -------------------------------------------------------------------------------
__global__ void k_find_iota(int32_t* f, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    f[i] = int32_t(i);
}
// deg[i] = the entries of row i, 0 for a hidden row; deg[n] = 0
__global__ void k_find_vis_deg(const int64_t* __restrict__ row_ptr, const uint8_t* __restrict__ row_ok, int64_t n,
                               int64_t* __restrict__ deg) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += int64_t(gridDim.x) * blockDim.x)
    deg[i] = i < n && row_ok[i] ? row_ptr[i + 1] - row_ptr[i] : 0;
}
// a kept slot of the flattened frontier -> its row (the identity frontier: entry = row) and entry
__global__ void k_find_slot_rows(const int64_t* __restrict__ slots, int64_t m, const int64_t* __restrict__ off,
                                 const int64_t* __restrict__ row_ptr, int64_t n_rows, int32_t* __restrict__ rows_src,
                                 int64_t* __restrict__ rows_edge) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t s = slots[i];
    const int64_t r = find_row([&](int64_t x) { return off[x]; }, 0, n_rows, s);
    rows_src[i] = int32_t(r);
    rows_edge[i] = row_ptr[r] + (s - off[r]);
  }
}

// ---- vertices -----------------------------------------------------------------------------------
// flag[x] = column index x (gidx, or n_global + tail position) holds a row of the tag in the vid's
// own part, this rank owns the vid and WHERE is true there (prog null: no WHERE)
__global__ __launch_bounds__(kFindThreads) void k_find_vflag(int64_t n, int64_t ng, const int64_t* __restrict__ vid_of,
                                                             const int64_t* __restrict__ tail,
                                                             const uint8_t* __restrict__ state, int32_t parts,
                                                             int32_t world, int32_t rank,
                                                             const Program* __restrict__ prog, EvalEnv env,
                                                             uint8_t* __restrict__ flag, unsigned long long* err) {
  for (int64_t x = int64_t(blockIdx.x) * kFindThreads + threadIdx.x; x < n; x += int64_t(gridDim.x) * kFindThreads) {
    bool ok = state[x] == 1;
    if (ok && world > 1) ok = dev_owner(x < ng ? vid_of[x] : tail[x - ng], parts, world) == rank;
    if (ok && prog) {
      const Val v = eval_program(prog, env, 0, int32_t(x), int32_t(x));
      if (v.t == VT_ERR) {
        atomicAdd(err, 1ull);
        ok = false;
      } else {
        ok = as_bool(v);
      }
    }
    flag[x] = ok;
  }
}
__global__ void k_find_vids(const int32_t* __restrict__ idx, int64_t n, int64_t ng, const int64_t* __restrict__ vid_of,
                            const int64_t* __restrict__ tail, int64_t* __restrict__ out) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t x = idx[i];
    out[i] = x < ng ? vid_of[x] : tail[x - ng];
  }
}

// ---- host ---------------------------------------------------------------------------------------
Program program_key(uint8_t op) {
  Program p = program_dst();
  p.ins[0] = Ins{op, 0, 0};
  return p;
}

struct FindQuery {
  bool has_where = false;
  Program where;
  std::vector<Program> yields;  // edges: behind the three key programs
};

// WHERE and the yields under FETCH's rule (FetchMode); `who`: "find_vertices" / "find_edges"
FindQuery compile_find(Ctx& c, const char* who, const uint8_t* where, size_t where_len, const uint8_t* const* yields,
                       const size_t* yield_lens, size_t n_yields, const TagSpace* tag, const EdgeSpace* es) {
  static const std::vector<Field> no_fields;
  const size_t n_keys = tag ? 1 : 3;
  if (n_yields > size_t(kMaxYieldCols) - n_keys)
    throw Error(NBG_E_UNSUPPORTED, std::string(who) + ": too many YIELD columns");
  FetchMode fm;
  fm.kind = tag ? FETCH_VERTICES : FETCH_EDGES;
  if (tag) fm.tag = tag->name;
  const std::vector<Field>& fields = tag ? no_fields : es->fields;
  FindQuery q;
  std::string msg;
  if (where_len) {
    const int32_t rc = compile_expr(where, where_len, fields, true, true, &q.where, &msg, &c.tag_refs, nullptr, &fm);
    if (rc != NBG_OK) throw Error(rc, std::string(who) + ": WHERE: " + msg);
    q.has_where = true;
  }
  if (!tag) q.yields = {program_key(P_SRC), program_dst(), program_key(P_RANK)};
  for (size_t k = 0; k < n_yields; k++) {
    if (!yields[k]) throw Error(NBG_E_INVALID_ARG, std::string(who) + ": null yield");
    Program p;
    const int32_t rc = compile_expr(yields[k], yield_lens[k], fields, true, true, &p, &msg, &c.tag_refs, nullptr, &fm);
    if (rc != NBG_OK) throw Error(rc, std::string(who) + ": " + msg);
    if (p.result_type == VT_ERR)
      throw Error(NBG_E_EVAL, std::string(who) + ": yield " + std::to_string(k) + " has no value type");
    q.yields.push_back(p);
  }
  return q;
}

void check_selected(uint64_t n, const char* who) {
  if (n >= (uint64_t(1) << 32)) throw Error(NBG_E_UNSUPPORTED, std::string(who) + ": 2^32 selected rows or more");
}

// uint32 tile counts -> uint64 bases (2^32 rows or more must be seen, not wrapped)
void scan_tile_counts(Ctx& c, const uint32_t* in, uint64_t* out, int64_t n) {
  size_t tb = 0;
  NBG_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, uint64_t(0), size_t(n), rocprim::plus<uint64_t>(), c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::exclusive_scan(c.ws_tmp.p, tb, in, out, uint64_t(0), size_t(n), rocprim::plus<uint64_t>(), c.stream));
  c.timing.launches++;
}

void timed(Ctx& c, size_t ia) {
  const size_t ib = timing_event(c);
  c.tpend.push_back(Ctx::PendingTime{ia, ib, -1, 0});  // timing_resolve adds it to expand_ms
  c.timing.expand_launches++;
}

// the row holding the first entry of every 2048-entry tile of the type's out CSR; depends on
// row_ptr alone, so it is kept until a commit (or another type's scan) replaces it
const int32_t* tile_row_table(Ctx& c, const EdgeSpace& es) {
  const Csr& csr = es.out;
  Ctx::FindWork& w = c.find;
  if (w.tile_row.p && w.type == es.type && w.row_ptr == csr.row_ptr.p && w.n_rows == csr.n_rows && w.nnz == csr.nnz &&
      w.commits == c.commits)
    return w.tile_row.as<int32_t>();
  {
    PoolScope outside(nullptr);  // lives past the call
    w.tile_row.alloc(size_t(find_tiles(csr.nnz) + 2) * 4);
  }
  k_tile_rows<kFindTile><<<grid_cap(csr.n_rows), 256, 0, c.stream>>>(csr.row_ptr.as<int64_t>(), csr.n_rows,
                                                                    w.tile_row.as<int32_t>());
  kernel_launched(c);
  w.type = es.type;
  w.row_ptr = csr.row_ptr.p;
  w.n_rows = csr.n_rows;
  w.nnz = csr.nnz;
  w.commits = c.commits;
  return w.tile_row.as<int32_t>();
}

template <int W>
void launch_find(Ctx& c, FindScan a, bool rows, int grid, bool emit) {
  if (!emit) {
    if (rows) k_find_count<W, true><<<grid, kFindThreads, 0, c.stream>>>(a);
    else k_find_count<W, false><<<grid, kFindThreads, 0, c.stream>>>(a);
  } else {
    if (rows) k_find_emit<W, true><<<grid, kFindThreads, 0, c.stream>>>(a);
    else k_find_emit<W, false><<<grid, kFindThreads, 0, c.stream>>>(a);
  }
  kernel_launched(c);
}
void launch_find(Ctx& c, const FindScan& a, int width, bool emit) {
  const bool rows = a.row_ok != nullptr;
  const int grid = int(std::max<int64_t>(1, std::min<int64_t>(find_tiles(a.nnz), kFindGrid)));
  const size_t ia = timing_event(c);
  switch (width) {
    case 1: launch_find<1>(c, a, rows, grid, emit); break;
    case 2: launch_find<2>(c, a, rows, grid, emit); break;
    case 4: launch_find<4>(c, a, rows, grid, emit); break;
    default: launch_find<8>(c, a, rows, grid, emit); break;
  }
  timed(c, ia);
}

// the (row, entry) pairs of the selected entries in entry order
struct Selected {
  DevBuf src, edge;
  int64_t n = 0;
};

// count, scan, emit.  One host wait: the match count with the error and tile statistics.
void scan_fast(Ctx& c, EdgeSpace& es, const FastPred& fpk, Selected& sel) {
  Csr& csr = es.out;
  const PropCol& pc = csr.props[size_t(fpk.col)];
  const int64_t ntiles = find_tiles(csr.nnz);
  DevBuf cnt, base, stats;
  cnt.alloc(size_t(ntiles + 1) * 4);
  base.alloc(size_t(ntiles + 1) * 8);
  stats.alloc(16);
  NBG_HIP(hipMemsetAsync(stats.p, 0, 16, c.stream));
  FindScan a{};
  a.data = pc.data.p;
  a.present = pc.present.as<uint8_t>();
  a.nnz = csr.nnz;
  a.op = fpk.op;
  a.k = fpk.k;
  a.row_ptr = csr.row_ptr.as<int64_t>();
  a.n_rows = csr.n_rows;
  a.row_ok = csr.row_ok.as<uint8_t>();
  a.tile_row = tile_row_table(c, es);
  a.tile_cnt = cnt.as<uint32_t>();
  a.stats = stats.as<unsigned long long>();
  launch_find(c, a, pc.width, false);
  scan_tile_counts(c, cnt.as<uint32_t>(), base.as<uint64_t>(), ntiles + 1);
  uint64_t total = 0, hs[2] = {0, 0};
  NBG_HIP(hipMemcpyAsync(&total, base.as<uint64_t>() + ntiles, 8, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipMemcpyAsync(hs, stats.p, 16, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  c.timing.host_waits++;
  if (hs[0]) throw Error(NBG_E_EVAL, "find_edges: WHERE evaluation failed");
  check_selected(total, "find_edges");
  sel.n = int64_t(total);
  // the count pass reads the column (+ presence bytes) and writes 4 B a tile;
  // the scan moves 12 B a tile; the emit pass reads the tiles with passers again, their share of
  // row_ptr (8 B a row, pro rata) and 12 B of tile words, and writes 12 B a row.  With row_ok the
  // count pass stages row_ptr too and both read a byte per resolved entry (not modelled).
  const uint64_t per = uint64_t(pc.width) + (a.present ? 1 : 0);
  const uint64_t rp_share = ntiles ? uint64_t(double(csr.n_rows) * 8.0 * double(hs[1]) / double(ntiles)) : 0;
  c.timing.expand_bytes = uint64_t(csr.nnz) * per + uint64_t(ntiles) * 16 + hs[1] * uint64_t(kFindTile) * per + rp_share +
                          hs[1] * 12 + total * 12 + (a.row_ok ? uint64_t(csr.n_rows) * 8 : 0);
  if (sel.n == 0) return;
  sel.src.alloc(size_t(sel.n) * 4);
  sel.edge.alloc(size_t(sel.n) * 8);
  a.tile_base = base.as<uint64_t>();
  a.rows_src = sel.src.as<int32_t>();
  a.rows_edge = sel.edge.as<int64_t>();
  launch_find(c, a, pc.width, true);
}

// expand_flags over the identity frontier, select.  One host wait: the match and error counts.
void scan_general(Ctx& c, EdgeSpace& es, const FindQuery& q, const EvalEnv& env, Selected& sel) {
  Csr& csr = es.out;
  const int64_t nr = csr.n_rows, E = csr.nnz;
  DevBuf F, deg, off, flags, slots, cnt, dprog;
  F.alloc(size_t(nr) * 4);
  k_find_iota<<<grid_cap(nr), 256, 0, c.stream>>>(F.as<int32_t>(), nr);
  kernel_launched(c);
  flags.alloc(size_t(E) + 1);
  const int64_t* d_off = csr.row_ptr.as<int64_t>();
  if (csr.row_ok.p) {
    // hidden rows get degree 0: they are never evaluated.  The flattened space then ends before E;
    // the slots behind its end stay 0.
    deg.alloc(size_t(nr + 1) * 8);
    off.alloc(size_t(nr + 1) * 8);
    k_find_vis_deg<<<grid_cap(nr + 1), 256, 0, c.stream>>>(d_off, csr.row_ok.as<uint8_t>(), nr, deg.as<int64_t>());
    kernel_launched(c);
    scan_i64(c, deg.as<int64_t>(), off.as<int64_t>(), nr + 1);
    d_off = off.as<int64_t>();
    NBG_HIP(hipMemsetAsync(flags.p, 0, size_t(E) + 1, c.stream));
  }
  cnt.alloc(16);
  NBG_HIP(hipMemsetAsync(cnt.p, 0, 16, c.stream));
  if (q.has_where) {
    dprog.alloc(sizeof(Program));
    c.h2d(dprog.p, &q.where, sizeof(Program));
  }
  ExpandArgs a{};
  a.F = F.as<int32_t>();
  a.nF = nr;
  a.off = d_off;
  a.row_ptr = csr.row_ptr.as<int64_t>();
  a.col = csr.col.as<int32_t>();
  a.lo = c.owned_lo();
  a.flags = flags.as<uint8_t>();
  a.err = cnt.as<unsigned long long>() + 1;
  a.storage = 0;
  expand_flags(c, a, q.has_where ? PK_VM : PK_NONE, FastArgs{}, dprog.as<Program>(), env, E);
  c.timing.launches += 2;  // k_tile_rows, k_expand
  c.timing.expand_bytes = expand_bytes(nr, E, 0, EXP_FLAGS);
  slots.alloc(size_t(E) * 8 + 8);
  select_dev(c, rocprim::counting_iterator<int64_t>(0), flags.as<uint8_t>(), slots.as<int64_t>(), cnt.as<uint64_t>(), E);
  c.timing.launches++;
  uint64_t h[2] = {0, 0};
  NBG_HIP(hipMemcpyAsync(h, cnt.p, 16, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  c.timing.host_waits++;
  c.host_stage_used = 0;
  if (h[1]) throw Error(NBG_E_EVAL, "find_edges: WHERE evaluation failed");
  check_selected(h[0], "find_edges");
  sel.n = int64_t(h[0]);
  if (sel.n == 0) return;
  sel.src.alloc(size_t(sel.n) * 4);
  sel.edge.alloc(size_t(sel.n) * 8);
  k_find_slot_rows<<<grid_cap(sel.n), 256, 0, c.stream>>>(slots.as<int64_t>(), sel.n, d_off, csr.row_ptr.as<int64_t>(), nr,
                                                          sel.src.as<int32_t>(), sel.edge.as<int64_t>());
  kernel_launched(c);
}

int32_t find_edges_impl(Ctx& c, EdgeSpace& es, const FindQuery& q, bool keep_on_device, nbg_rows* out) {
  begin_call(c);
  c.hop_timing = true;  // the scan kernels' event pairs (expand_ms)
  const int64_t mode = c.opt("find_fast", -1);
  if (mode < -1 || mode > 1) throw Error(NBG_E_INVALID_ARG, "find_edges: option find_fast must be 0 or 1");
  Csr& csr = es.out;
  const EvalEnv env = make_env(c, es, csr, es.type);
  Selected sel;
  if (csr.nnz > 0) {
    if (csr.n_rows != c.owned_hi() - c.owned_lo())
      throw Error(NBG_E_UNKNOWN, "find_edges: the out CSR does not span the owned rows");
    const FastPred fpk = q.has_where ? classify_pred(q.where, es.fields) : FastPred{};
    // (the wide loads need the column at a 16-byte boundary: every DevBuf block is)
    const bool fast = mode != 0 && fpk.kind == PK_FAST &&
                      (reinterpret_cast<uintptr_t>(csr.props[size_t(fpk.col)].data.p) & 15u) == 0 &&
                      (reinterpret_cast<uintptr_t>(csr.props[size_t(fpk.col)].present.p) & 7u) == 0;
    if (fast) scan_fast(c, es, fpk, sel);
    else scan_general(c, es, q, env, sel);
    c.timing.edges_scanned = uint64_t(csr.nnz);
  }
  YieldOut y;
  yield_rows(c, q.yields, env, sel.src.as<int32_t>(), sel.edge.as<int64_t>(), c.owned_lo(), sel.n,
             "find_edges: YIELD evaluation failed", y);
  hand_out_call(c, y, sel.n, keep_on_device, out);
  return NBG_OK;
}

int32_t find_vertices_impl(Ctx& c, TagSpace& ts, const FindQuery& q, bool keep_on_device, nbg_rows* out) {
  begin_call(c);
  const int64_t ng = c.n_global, n = ng + ts.n_tail;
  Csr no_csr;
  EdgeSpace no_edges;
  const EvalEnv env = make_env(c, no_edges, no_csr, 0);
  DevBuf flag, rows, cnt, dprog, vids;
  int64_t n_rows = 0;
  if (n > 0 && ts.state.p) {
    if (uint64_t(n) >= (uint64_t(1) << 31)) throw Error(NBG_E_UNSUPPORTED, "find_vertices: 2^31 column entries or more");
    flag.alloc(size_t(n));
    rows.alloc(size_t(n) * 4 + 8);
    cnt.alloc(16);
    NBG_HIP(hipMemsetAsync(cnt.p, 0, 16, c.stream));
    if (q.has_where) {
      dprog.alloc(sizeof(Program));
      c.h2d(dprog.p, &q.where, sizeof(Program));
    }
    k_find_vflag<<<grid_for(n, kFindThreads), kFindThreads, 0, c.stream>>>(
        n, ng, c.vid_of.as<int64_t>(), ts.tail_vids.as<int64_t>(), ts.state.as<uint8_t>(), c.num_parts, c.world, c.rank,
        dprog.as<Program>(), env, flag.as<uint8_t>(), cnt.as<unsigned long long>() + 1);
    kernel_launched(c);
    select_dev(c, rocprim::counting_iterator<int32_t>(0), flag.as<uint8_t>(), rows.as<int32_t>(), cnt.as<uint64_t>(), n);
    c.timing.launches++;
    uint64_t h[2] = {0, 0};
    NBG_HIP(hipMemcpyAsync(h, cnt.p, 16, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    c.timing.host_waits++;
    c.host_stage_used = 0;
    if (h[1]) throw Error(NBG_E_EVAL, "find_vertices: WHERE evaluation failed");
    n_rows = int64_t(h[0]);
  }
  vids.alloc(size_t(n_rows) * 8 + 8);
  if (n_rows) {
    k_find_vids<<<grid_cap(n_rows), 256, 0, c.stream>>>(rows.as<int32_t>(), n_rows, ng, c.vid_of.as<int64_t>(),
                                                        ts.tail_vids.as<int64_t>(), vids.as<int64_t>());
    kernel_launched(c);
  }
  // vertex rows: src = the column index, no edge (the programs hold P_SRCTAG and constants only)
  YieldOut y;
  if (!q.yields.empty())
    yield_rows(c, q.yields, env, rows.as<int32_t>(), nullptr, 0, n_rows, "find_vertices: YIELD evaluation failed", y);
  y.types.insert(y.types.begin(), NBG_T_VID);
  y.dev.insert(y.dev.begin(), std::move(vids));
  y.off.insert(y.off.begin(), DevBuf());
  y.str_bytes.insert(y.str_bytes.begin(), 0);
  hand_out_call(c, y, n_rows, keep_on_device, out);
  return NBG_OK;
}

void check_keep(int32_t keep_on_device, const char* who) {
  if ((keep_on_device | 1) != 1) throw Error(NBG_E_INVALID_ARG, std::string(who) + ": keep_on_device must be 0 or 1");
}

}  // namespace

int32_t find_vertices_run(Ctx& c, int32_t tag_id, const uint8_t* where, size_t where_len, const uint8_t* const* yields,
                          const size_t* yield_lens, size_t n_yields, int32_t keep_on_device, nbg_rows* out) {
  PoolScope pool_scope(query_pool(c));
  if (!c.finalized) throw Error(NBG_E_STATE, "snapshot not finalized");
  check_keep(keep_on_device, "find_vertices");
  auto it = c.tags.find(tag_id);
  if (it == c.tags.end()) throw Error(NBG_E_TAG_PROP_NOT_FOUND, "find_vertices: unknown tag id " + std::to_string(tag_id));
  const FindQuery q = compile_find(c, "find_vertices", where, where_len, yields, yield_lens, n_yields, &it->second, nullptr);
  return run_guarded(c, [&]() { return find_vertices_impl(c, it->second, q, keep_on_device != 0, out); });
}

int32_t find_edges_run(Ctx& c, int32_t edge_type, const uint8_t* where, size_t where_len, const uint8_t* const* yields,
                       const size_t* yield_lens, size_t n_yields, int32_t keep_on_device, nbg_rows* out) {
  PoolScope pool_scope(query_pool(c));
  if (!c.finalized) throw Error(NBG_E_STATE, "snapshot not finalized");
  check_keep(keep_on_device, "find_edges");
  if (edge_type < 0) throw Error(NBG_E_UNSUPPORTED, "find_edges: in-edges carry no props (a negative edge type)");
  auto it = c.edges.find(edge_type);
  if (it == c.edges.end()) throw Error(NBG_E_INVALID_ARG, "find_edges: edge type not in snapshot");
  const FindQuery q = compile_find(c, "find_edges", where, where_len, yields, yield_lens, n_yields, nullptr, &it->second);
  return run_guarded(c, [&]() { return find_edges_impl(c, it->second, q, keep_on_device != 0, out); });
}

}  // namespace nbg
