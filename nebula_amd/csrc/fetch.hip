// fetch.hip -- FETCH PROP ON a tag / an edge type (nbg_fetch_vertices, nbg_fetch_edges): device key lookup.
//
// Replaces FetchVerticesExecutor / FetchEdgesExecutor (src/graph/FetchVerticesExecutor.cpp,
// FetchEdgesExecutor.cpp, FetchExecutor.cpp) over QueryVertexPropsProcessor / QueryEdgePropsProcessor
// (one RocksDB prefix scan per key) with a point lookup of every key in the resident snapshot.
// DESIGN.md section 3b has the byte model, the tail layout and the row-order divergence.
//
//   lookup_gidx       vid -> gidx of every key vid (the snapshot's hash)
//   k_fetch_vflag     vertices: a keep byte per key (resolved through the gidx space or the tag's tail of
//                     edge-less vertices, owned by this rank, the tag has a row of the vid's own part)
//   k_fetch_edge      edges: 16 lanes per key find (rank, dst) in src's out-CSR row: a binary search
//                     under the row's bytewise order down to a window, then a coalesced scan of the
//                     window's col segment (short rows: the scan alone)
//   select            the kept (row, edge) pairs in key order (rocprim::select)
//   yield_rows        yield.hip's YIELD materialiser over those pairs
// DISTINCT deduplicates the keys, then the rows, with nbg_set_op's hash machinery (setops.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "call_common.h"
#include "device_common.h"
#include "edge_lookup.h"
#include "engine.h"
#include "program.h"
#include "query_common.h"
#include "row_gather.h"
#include "rows.h"

namespace nbg {
namespace {

constexpr int kFetchThreads = 256;
constexpr int kFetchGroup = kLookupGroup;  // lanes per edge key
constexpr int64_t kFetchThreshold = 64;  // hybrid: rows longer than this are searched down to a window of it

// ---- vertices -----------------------------------------------------------------------------------
// idx[i] = the key's index into the tag's columns (gidx, or n_global + its tail position), flag[i] =
// the key yields a row.  A -1 gidx indexes nothing; a tail index is used for the tag's arrays only.
__global__ __launch_bounds__(kFetchThreads) void k_fetch_vflag(const int64_t* __restrict__ vids,
                                                               const int32_t* __restrict__ gidx, int64_t n, int64_t ng,
                                                               const int64_t* __restrict__ tail, int64_t nt,
                                                               const uint8_t* __restrict__ state, int32_t parts,
                                                               int32_t world, int32_t rank, int32_t* __restrict__ idx,
                                                               uint8_t* __restrict__ flag) {
  for (int64_t i = int64_t(blockIdx.x) * kFetchThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kFetchThreads) {
    const int64_t v = vids[i];
    int64_t x = gidx ? int64_t(gidx[i]) : -1;
    if (x < 0) {  // no edge names the vid: the tag's sorted tail
      int64_t l = 0, h = nt;
      while (l < h) {
        const int64_t m = l + ((h - l) >> 1);
        if (tail[m] < v) l = m + 1;
        else h = m;
      }
      x = (l < nt && tail[l] == v) ? ng + l : -1;
    }
    const bool ok = x >= 0 && state[x] == 1 && (world == 1 || dev_owner(v, parts, world) == rank);
    idx[i] = ok ? int32_t(x) : 0;
    flag[i] = ok;
  }
}

// ---- edges --------------------------------------------------------------------------------------
struct EdgeLookup {
  const int64_t* dst;   // key dst vids
  const int64_t* rank;  // key ranks, or null: every key has rank 0
  const int32_t* gs;    // gidx of the key src / dst vids (-1: unknown)
  const int32_t* gd;
  int64_t n;
  const int64_t* row_ptr;
  EdgeRows rows;           // col, col_vid, erank, vid_of and the search window (edge_lookup.h)
  const uint8_t* row_ok;   // or null: every row visible
  int64_t lo, n_rows;
  int32_t* out_src;   // local row of the key's src
  int64_t* out_edge;  // the matching entry
  uint8_t* flag;
  unsigned long long* scanned;  // [0] entries the scans read, [1] entries the searches probed
};

// One 16-lane group per key: the key's row, then group_find_edge (edge_lookup.h: the binary search
// under the row's bytewise order down to a window and the window's scan).
__global__ __launch_bounds__(kFetchThreads) void k_fetch_edge(EdgeLookup a) {
  const int lane = threadIdx.x & (kWave - 1), sub = lane & (kFetchGroup - 1);
  const int64_t groups = int64_t(gridDim.x) * (kFetchThreads / kFetchGroup);
  const int64_t g0 = (int64_t(blockIdx.x) * kFetchThreads + threadIdx.x) / kFetchGroup;
  const int64_t rounds = (a.n + groups - 1) / groups;
  unsigned long long scanned = 0, probed = 0;
  for (int64_t r = 0; r < rounds; r++) {
    const int64_t i = r * groups + g0;
    int64_t beg = 0, end = 0, rk = 0, dv = 0;
    int32_t dg = -1, row = 0;
    if (i < a.n) {
      const int32_t sg = a.gs[i];
      dg = a.gd[i];
      rk = a.rank ? a.rank[i] : 0;
      dv = a.dst[i];
      // (a CSR without a rank array holds rank 0 only: a key of another rank matches nothing)
      if (sg >= 0 && dg >= 0 && sg >= a.lo && sg - a.lo < a.n_rows && (a.rows.erank || rk == 0)) {
        row = int32_t(sg - a.lo);
        if (!a.row_ok || a.row_ok[row]) {
          beg = a.row_ptr[row];
          end = a.row_ptr[row + 1];
        }
      }
    }
    const int64_t found = group_find_edge(a.rows, beg, end, rk, dv, dg, scanned, probed);
    if (sub == 0 && i < a.n) {
      a.flag[i] = found >= 0;
      a.out_src[i] = row;
      a.out_edge[i] = found < 0 ? 0 : found;
    }
  }
  scanned = wave_sum_u64(scanned);
  probed = wave_sum_u64(probed);
  if (lane == 0 && scanned) atomicAdd(a.scanned, scanned);
  if (lane == 0 && probed) atomicAdd(a.scanned + 1, probed);
}

// ---- host ---------------------------------------------------------------------------------------
void check_flags(int32_t keys_on_device, int32_t distinct, int32_t keep_on_device) {
  if ((keys_on_device | 1) != 1 || (distinct | 1) != 1 || (keep_on_device | 1) != 1)
    throw Error(NBG_E_INVALID_ARG, "fetch: keys_on_device, distinct and keep_on_device must be 0 or 1");
}

// the call's key columns in HBM: uploaded, or read in place (keys_on_device); DISTINCT replaces them
// by their first occurrences in input order (getDistinctVIDs, EdgeKeyHashSet)
struct Keys {
  std::vector<const int64_t*> col;
  std::vector<DevBuf> own;
  int64_t n = 0;

  void add(Ctx& c, const int64_t* p, bool on_device) {
    if (on_device || n == 0) {
      col.push_back(p);
      return;
    }
    DevBuf b;
    b.alloc(size_t(n) * 8);
    NBG_HIP(hipMemcpyAsync(b.p, p, size_t(n) * 8, hipMemcpyHostToDevice, c.stream));
    col.push_back(b.as<int64_t>());
    own.push_back(std::move(b));
  }
  void dedup(Ctx& c) {
    if (n == 0) return;
    std::vector<TableCol> tab;
    std::vector<InCol> in;
    for (const int64_t* p : col) {
      tab.push_back(TableCol{NBG_T_VID, p, nullptr, 0});
      in.push_back(InCol{NBG_T_VID, p, nullptr, 0});
    }
    DevBuf idx;
    const int64_t kept = distinct_first_rows(c, tab, n, idx);
    if (kept == n) return;
    std::vector<DevBuf> dev(col.size()), off(col.size());
    gather_rows(c, in, idx.as<uint32_t>(), kept, dev, off);
    // (the stream orders the gather before the old blocks' reuse)
    own = std::move(dev);
    for (size_t k = 0; k < col.size(); k++) col[k] = own[k].as<int64_t>();
    n = kept;
  }
};

// `who`: "fetch_vertices" / "fetch_edges"; tag: FETCH_VERTICES the tag, else null
std::vector<Program> compile_yields(Ctx& c, const uint8_t* const* yields, const size_t* yield_lens, size_t n_yields,
                                    const TagSpace* tag, const EdgeSpace* es) {
  if (n_yields > size_t(kMaxYieldCols)) throw Error(NBG_E_UNSUPPORTED, "fetch: too many YIELD columns");
  std::vector<Program> progs;
  if (n_yields == 0) {  // every field of the schema, in schema order (FetchExecutor::setupColumns)
    if (tag) {
      for (size_t i = 0; i < c.tag_refs.size(); i++)
        if (c.tag_refs[i].tag == tag->name) progs.push_back(program_prop(P_SRCTAG, int16_t(i), c.tag_refs[i].type));
    } else {
      for (size_t i = 0; i < es->fields.size(); i++) progs.push_back(program_prop(P_PROP, int16_t(i), es->fields[i].type));
    }
    if (progs.empty()) throw Error(NBG_E_INVALID_ARG, "No props declared.");
    if (progs.size() > size_t(kMaxYieldCols)) throw Error(NBG_E_UNSUPPORTED, "fetch: too many schema fields for one result");
    return progs;
  }
  static const std::vector<Field> no_fields;
  FetchMode fm;
  fm.kind = tag ? FETCH_VERTICES : FETCH_EDGES;
  if (tag) fm.tag = tag->name;
  progs.resize(n_yields);
  for (size_t k = 0; k < n_yields; k++) {
    if (!yields[k]) throw Error(NBG_E_INVALID_ARG, "fetch: null yield");
    std::string msg;
    const int32_t rc = compile_expr(yields[k], yield_lens[k], tag ? no_fields : es->fields, true, true, &progs[k], &msg,
                                    &c.tag_refs, nullptr, &fm);
    if (rc != NBG_OK) throw Error(rc, msg);
    if (progs[k].result_type == VT_ERR) throw Error(NBG_E_EVAL, "fetch: yield " + std::to_string(k) + " has no value type");
  }
  if (fm.n_props == 0) throw Error(NBG_E_INVALID_ARG, "No props declared.");
  return progs;
}

// rows -> DISTINCT by value (uniqResult) -> the caller
void finish_call(Ctx& c, YieldOut& y, int64_t n_rows, bool distinct, bool keep_on_device, nbg_rows* out) {
  const size_t ncols = y.types.size();
  if (distinct && n_rows > 1) {
    std::vector<TableCol> tab;
    std::vector<InCol> in;
    for (size_t k = 0; k < ncols; k++) {
      tab.push_back(TableCol{y.types[k], y.dev[k].p, y.off[k].as<int64_t>(), y.str_bytes[k]});
      in.push_back(InCol{y.types[k], y.dev[k].p, y.off[k].as<int64_t>(), y.str_bytes[k]});
    }
    DevBuf idx;
    const int64_t kept = distinct_first_rows(c, tab, n_rows, idx);
    if (kept < n_rows) {
      std::vector<DevBuf> dev(ncols), off(ncols);
      gather_rows(c, in, idx.as<uint32_t>(), kept, dev, off);
      y.dev = std::move(dev);
      y.off = std::move(off);
      n_rows = kept;
    }
  }
  hand_out_call(c, y, n_rows, keep_on_device, out);
}

// the kept entries of `in` (flag != 0) in order behind `out`; the last select's count lands in cnt
template <typename T>
void keep_flagged(Ctx& c, const T* in, const uint8_t* flag, T* out, uint64_t* cnt, int64_t n) {
  select_dev(c, in, flag, out, cnt, n);
  c.timing.launches++;
}

int32_t fetch_vertices_impl(Ctx& c, TagSpace& ts, const int64_t* vids, size_t n, bool keys_on_device,
                            const std::vector<Program>& progs, bool distinct, bool keep_on_device, nbg_rows* out) {
  begin_call(c);
  Keys keys;
  keys.n = int64_t(n);
  keys.add(c, vids, keys_on_device);
  if (distinct) keys.dedup(c);
  const int64_t nk = keys.n;

  DevBuf gidx, idx, flag, rows, cnt;
  int64_t n_rows = 0;
  if (nk > 0) {
    if (c.n_global > 0) {
      gidx.alloc(size_t(nk) * 4);
      lookup_gidx(c, keys.col[0], gidx.as<int32_t>(), nk);
      c.timing.launches++;
    }
    idx.alloc(size_t(nk) * 4);
    flag.alloc(size_t(nk));
    rows.alloc(size_t(nk) * 4 + 8);
    cnt.alloc(8);
    k_fetch_vflag<<<grid_for(nk, kFetchThreads), kFetchThreads, 0, c.stream>>>(
        keys.col[0], gidx.as<int32_t>(), nk, c.n_global, ts.tail_vids.as<int64_t>(), ts.n_tail, ts.state.as<uint8_t>(),
        c.num_parts, c.world, c.rank, idx.as<int32_t>(), flag.as<uint8_t>());
    kernel_launched(c);
    keep_flagged(c, idx.as<int32_t>(), flag.as<uint8_t>(), rows.as<int32_t>(), cnt.as<uint64_t>(), nk);
    uint64_t kept = 0;
    NBG_HIP(hipMemcpyAsync(&kept, cnt.p, 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    c.timing.host_waits++;
    n_rows = int64_t(kept);
  }
  // vertex rows: src = the column index, no edge (the programs hold P_SRCTAG and constants only)
  Csr no_csr;
  EdgeSpace no_edges;
  const EvalEnv env = make_env(c, no_edges, no_csr, 0);
  YieldOut y;
  yield_rows(c, progs, env, rows.as<int32_t>(), nullptr, 0, n_rows, "fetch_vertices: YIELD evaluation failed", y);
  finish_call(c, y, n_rows, distinct, keep_on_device, out);
  return NBG_OK;
}

int32_t fetch_edges_impl(Ctx& c, EdgeSpace& es, const int64_t* src, const int64_t* dst, const int64_t* rank, size_t n,
                         bool keys_on_device, const std::vector<Program>& progs, bool distinct, bool keep_on_device,
                         nbg_rows* out) {
  begin_call(c);
  const int64_t mode = c.opt("fetch_search", -1);
  if (mode < -1 || mode > 1) throw Error(NBG_E_INVALID_ARG, "fetch_edges: option fetch_search must be 0 or 1");
  const int64_t threshold = c.opt("fetch_threshold", kFetchThreshold);  // (measurement: tools/fetch_compare.py)
  if (threshold < 0 || threshold > INT32_MAX) throw Error(NBG_E_INVALID_ARG, "fetch_edges: option fetch_threshold out of range");
  Keys keys;
  keys.n = int64_t(n);
  keys.add(c, src, keys_on_device);
  keys.add(c, dst, keys_on_device);
  if (rank) keys.add(c, rank, keys_on_device);
  if (distinct) keys.dedup(c);
  const int64_t nk = keys.n;

  Csr& csr = es.out;
  DevBuf gs, gd, ksrc, kedge, flag, rsrc, redge, cnt;
  int64_t n_rows = 0;
  if (nk > 0 && c.n_global > 0 && csr.nnz > 0) {
    gs.alloc(size_t(nk) * 4);
    gd.alloc(size_t(nk) * 4);
    lookup_gidx(c, keys.col[0], gs.as<int32_t>(), nk);
    lookup_gidx(c, keys.col[1], gd.as<int32_t>(), nk);
    c.timing.launches += 2;
    ksrc.alloc(size_t(nk) * 4);
    kedge.alloc(size_t(nk) * 8);
    flag.alloc(size_t(nk));
    rsrc.alloc(size_t(nk) * 4 + 8);
    redge.alloc(size_t(nk) * 8 + 8);
    cnt.alloc(24);
    NBG_HIP(hipMemsetAsync(cnt.p, 0, 24, c.stream));
    EdgeLookup a{};
    a.dst = keys.col[1];
    a.rank = rank ? keys.col[2] : nullptr;
    a.gs = gs.as<int32_t>();
    a.gd = gd.as<int32_t>();
    a.n = nk;
    a.row_ptr = csr.row_ptr.as<int64_t>();
    a.rows.col = csr.col.as<int32_t>();
    a.rows.col_vid = csr.col_vid.as<int64_t>();
    a.rows.erank = csr.rank.as<int64_t>();
    a.row_ok = csr.row_ok.as<uint8_t>();
    a.rows.vid_of = c.vid_of.as<int64_t>();
    a.lo = c.owned_lo();
    a.n_rows = std::min<int64_t>(csr.n_rows, c.owned_hi() - c.owned_lo());
    a.rows.window = mode == 0 ? INT64_MAX : mode == 1 ? 1 : std::max<int64_t>(1, threshold);
    a.out_src = ksrc.as<int32_t>();
    a.out_edge = kedge.as<int64_t>();
    a.flag = flag.as<uint8_t>();
    a.scanned = cnt.as<unsigned long long>() + 1;  // (word 0: the select's count)
    NBG_HIP(hipEventRecord(c.ev[6], c.stream));
    k_fetch_edge<<<grid_for(nk, kFetchThreads / kFetchGroup), kFetchThreads, 0, c.stream>>>(a);
    kernel_launched(c);
    NBG_HIP(hipEventRecord(c.ev[7], c.stream));
    keep_flagged(c, ksrc.as<int32_t>(), flag.as<uint8_t>(), rsrc.as<int32_t>(), cnt.as<uint64_t>(), nk);
    keep_flagged(c, kedge.as<int64_t>(), flag.as<uint8_t>(), redge.as<int64_t>(), cnt.as<uint64_t>(), nk);
    uint64_t h[3] = {0, 0, 0};
    NBG_HIP(hipMemcpyAsync(h, cnt.p, 24, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    c.timing.host_waits++;
    n_rows = int64_t(h[0]);
    c.timing.edges_scanned = h[1] + h[2];
    // the lookup kernel alone: its time and its algorithmic bytes: per key
    // the dst vid (+ rank), two gidx, the row_ptr pair (+ row_ok byte) and the 13 B it writes; per
    // entry scanned 4 B col (+ 8 B rank); per entry probed the 8 B dst vid (col_vid, else 4 B col +
    // 8 B vid_of) (+ 8 B rank)
    float ms = 0;
    if (hipEventElapsedTime(&ms, c.ev[6], c.ev[7]) == hipSuccess) c.timing.expand_ms = ms;
    c.timing.expand_launches = 1;
    const uint64_t rk = a.rows.erank ? 8 : 0;
    c.timing.expand_bytes = uint64_t(nk) * (8 + (a.rank ? 8 : 0) + 8 + 16 + (a.row_ok ? 1 : 0) + 13) + h[1] * (4 + rk) +
                            h[2] * ((a.rows.col_vid ? 8 : 12) + rk);
  }
  const EvalEnv env = make_env(c, es, csr, es.type);
  YieldOut y;
  yield_rows(c, progs, env, rsrc.as<int32_t>(), redge.as<int64_t>(), c.owned_lo(), n_rows,
             "fetch_edges: YIELD evaluation failed", y);
  finish_call(c, y, n_rows, distinct, keep_on_device, out);
  return NBG_OK;
}

}  // namespace

int32_t fetch_vertices_run(Ctx& c, int32_t tag_id, const int64_t* vids, size_t n, int32_t keys_on_device,
                           const uint8_t* const* yields, const size_t* yield_lens, size_t n_yields, int32_t distinct,
                           int32_t keep_on_device, nbg_rows* out) {
  PoolScope pool_scope(query_pool(c));
  if (!c.finalized) throw Error(NBG_E_STATE, "snapshot not finalized");
  check_flags(keys_on_device, distinct, keep_on_device);
  auto it = c.tags.find(tag_id);
  if (it == c.tags.end()) throw Error(NBG_E_TAG_PROP_NOT_FOUND, "fetch_vertices: unknown tag id " + std::to_string(tag_id));
  if (uint64_t(n) >= (uint64_t(1) << 32)) throw Error(NBG_E_UNSUPPORTED, "fetch_vertices: 2^32 keys or more");
  const std::vector<Program> progs = compile_yields(c, yields, yield_lens, n_yields, &it->second, nullptr);
  return run_guarded(c, [&]() {
    return fetch_vertices_impl(c, it->second, vids, n, keys_on_device != 0, progs, distinct != 0, keep_on_device != 0, out);
  });
}

int32_t fetch_edges_run(Ctx& c, int32_t edge_type, const int64_t* src, const int64_t* dst, const int64_t* rank, size_t n,
                        int32_t keys_on_device, const uint8_t* const* yields, const size_t* yield_lens, size_t n_yields,
                        int32_t distinct, int32_t keep_on_device, nbg_rows* out) {
  PoolScope pool_scope(query_pool(c));
  if (!c.finalized) throw Error(NBG_E_STATE, "snapshot not finalized");
  check_flags(keys_on_device, distinct, keep_on_device);
  if (edge_type < 0) throw Error(NBG_E_UNSUPPORTED, "fetch_edges: in-edges carry no props (a negative edge type)");
  auto it = c.edges.find(edge_type);
  if (it == c.edges.end()) throw Error(NBG_E_INVALID_ARG, "fetch_edges: edge type not in snapshot");
  if (uint64_t(n) >= (uint64_t(1) << 32)) throw Error(NBG_E_UNSUPPORTED, "fetch_edges: 2^32 keys or more");
  const std::vector<Program> progs = compile_yields(c, yields, yield_lens, n_yields, nullptr, &it->second);
  return run_guarded(c, [&]() {
    return fetch_edges_impl(c, it->second, src, dst, rank, n, keys_on_device != 0, progs, distinct != 0,
                            keep_on_device != 0, out);
  });
}

}  // namespace nbg
