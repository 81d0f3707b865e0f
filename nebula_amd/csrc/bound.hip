// bound.hip -- storage getBound / outBoundStats / inBoundStats on MI355X (gfx950).
//
// Replaces, for a whole request at once:
//   * QueryBoundProcessor (QueryBoundProcessor.cpp:19-67): the edge rows of every requested
//     (part, vid) under a push-down filter, plus the SOURCE / DEST tag props of the vertices;
//   * QueryStatsProcessor (QueryStatsProcessor.cpp:69-125): SUM / COUNT / AVG over the same rows;
//   * collectEdgeProps' firstLoop (QueryBaseProcessor.inl:349-402): on multi-version data the
//     older version a filter lets through ahead of a row's ordinary rows.
//
// The filter runs through the GO expansion (expand_flags, expand.hip): a flag byte per edge slot
// of the request's flattened adjacency; a select turns the flags into the kept rows.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "device_common.h"
#include "query_common.h"
#include "rows.h"

namespace nbg {

// request entry -> local row; a (part, vid) pair whose part does not hold the vertex's keys scans
// an empty prefix in the reference, so it gets a zero-degree stand-in (-1)
__global__ void k_bound_frontier(const int32_t* parts, const int32_t* g, int64_t n, int64_t lo, int64_t hi,
                                 const int32_t* row_part, int32_t* F) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int32_t x = g[i];
    bool ok = x >= lo && x < hi && row_part[x - lo] == parts[i];
    F[i] = ok ? int32_t(x - lo) : -1;
  }
}
__global__ void k_degrees_masked(const int32_t* F, int64_t n, const int64_t* row_ptr, int64_t* deg) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i <= n; i += int64_t(gridDim.x) * blockDim.x) {
    if (i == n) deg[i] = 0;
    else deg[i] = F[i] < 0 ? 0 : row_ptr[F[i] + 1] - row_ptr[F[i]];
  }
}
// request entries with deg 0 are removed so every frontier entry covers >= 1 edge slot
__global__ void k_slot_owner(const int64_t* kept_slots, int64_t m, const int64_t* off, int64_t nF, int64_t* owner) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    int64_t e = kept_slots[i];
    int64_t lo = 0, hi = nF;
    while (hi - lo > 1) {
      int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= e) lo = mid; else hi = mid;
    }
    owner[i] = lo;
  }
}
struct BoundCol {
  int32_t kind;  // 0 prop, 1 _dst, 2 _src, 3 _rank, 4 _type
  int32_t prop;
  int32_t type;  // NBG_T_*
  int32_t stat;  // outBoundStats: cpp2::StatType SUM 1 / COUNT 2 / AVG 3 (0: plain getBound)
  void* out;
  int64_t* str_len;  // STRING pass 1
};
constexpr int kMaxBoundCols = 32;
struct BoundCols {
  int32_t n;
  BoundCol c[kMaxBoundCols];
};
// flattened slot -> edge index of the kept rows
__global__ void k_slot_ge(const int64_t* kept_slots, const int64_t* owner, int64_t m, const int64_t* off,
                          const int32_t* F, const int64_t* row_ptr, int64_t* ge) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t k = owner[i];
    ge[i] = row_ptr[F[k]] + (kept_slots[i] - off[k]);
  }
}
// one value of a getBound column for row i: edge ge's key props, and its props either from the
// CSR (old < 0) or from the older-version side table (row old, Csr::ov_*)
__device__ inline int64_t bound_value(const BoundCol& b, int64_t ge, int64_t old, int32_t f, int64_t lo,
                                      const EvalEnv& env, const PropDev* oprops, bool& present) {
  present = true;
  switch (b.kind) {
    case 1: return env.vid_of[env.col[ge]];
    case 2: return env.vid_of[lo + f];
    case 3: return env.rank ? env.rank[ge] : 0;
    case 4: return env.etype;
    default: {
      const PropDev& p = old < 0 ? env.props[b.prop] : oprops[b.prop];
      const int64_t x = old < 0 ? ge : old;
      if (p.present && !p.present[x]) {
        present = false;
        return INT64_MIN;
      }
      if (p.type == NBG_T_STRING) return x;
      if (p.type == NBG_T_DOUBLE || p.type == NBG_T_FLOAT) return static_cast<const int64_t*>(p.data)[x];
      return load_int(p.data, p.width, x);
    }
  }
}
__global__ void k_bound_rows(const int64_t* ge_in, const int64_t* old_in, const int64_t* owner, int64_t m,
                             const int32_t* F, int64_t lo, EvalEnv env, const PropDev* oprops, BoundCols bc) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t ge = ge_in[i];
    const int64_t old = old_in ? old_in[i] : -1;
    const int32_t f = F[owner[i]];
    for (int c = 0; c < bc.n; c++) {
      const BoundCol& b = bc.c[c];
      bool present;
      const int64_t v = bound_value(b, ge, old, f, lo, env, oprops, present);
      if (b.kind == 0) {
        const PropDev& p = old < 0 ? env.props[b.prop] : oprops[b.prop];
        if (p.type == NBG_T_STRING) {
          b.str_len[i] = present ? p.str_off[v + 1] - p.str_off[v] : -1;
          continue;
        }
      }
      if (b.type == NBG_T_BOOL) static_cast<uint8_t*>(b.out)[i] = uint8_t(v != 0);
      else static_cast<int64_t*>(b.out)[i] = v;
    }
  }
}
// outBoundStats / inBoundStats (QueryStatsProcessor.cpp:69-125, StatsCollector Collector.h:66-94):
// over the kept rows, the int64 sum (wrapping, as the reference's int64 adds) and the count of
// present values of column c.  acc[2c] = sum, acc[2c+1] = count.  Doubles only count (a double
// reaching the reference's int64-initialised sum throws, reported by the caller).
__global__ void k_bound_stats(const int64_t* ge_in, const int64_t* old_in, const int64_t* owner, int64_t m,
                              const int32_t* F, int64_t lo, EvalEnv env, const PropDev* oprops, BoundCol b,
                              unsigned long long* acc) {
  unsigned long long sum = 0, cnt = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t old = old_in ? old_in[i] : -1;
    bool present;
    int64_t v = bound_value(b, ge_in[i], old, F[owner[i]], lo, env, oprops, present);
    if (b.kind == 0) {
      const int32_t t = (old < 0 ? env.props[b.prop] : oprops[b.prop]).type;
      if (t == NBG_T_STRING || t == NBG_T_DOUBLE || t == NBG_T_FLOAT || t == NBG_T_BOOL) v = 0;
    }
    if (present) {
      sum += (unsigned long long)v;
      cnt++;
    }
  }
  sum = wave_sum_u64(sum);
  cnt = wave_sum_u64(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(acc, sum);
    atomicAdd(acc + 1, cnt);
  }
}

// collectEdgeProps' firstLoop (QueryBaseProcessor.inl:349-402): until a key is emitted the scan
// does not skip a group's older versions, so when every key before it fails the filter (all
// versions of the earlier groups and the newer versions of its own group), the first older
// version that passes is emitted, ahead of the row's ordinary rows.  One thread per request
// entry (frontier entry k = local row F[k], flags of its edges at off[k]..): walks its edges in
// key order until the first kept one; per edge whose first version failed, its older versions.
// x_old[k] = the emitted older version's side-table row (-1: none), x_ge[k] = its edge.
template <int PK>
__global__ void k_first_loop(const int32_t* F, const int64_t* off, int64_t nF, const int64_t* row_ptr,
                             const uint8_t* flags, const int64_t* ov_edge, int64_t ov_n, const Program* prog,
                             EvalEnv oenv, FastArgs ofp, int64_t lo, int64_t* x_old, int64_t* x_ge) {
  for (int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; k < nF; k += int64_t(gridDim.x) * blockDim.x) {
    x_old[k] = -1;
    const int32_t f = F[k];
    const int64_t b = row_ptr[f], e = row_ptr[f + 1];
    int64_t l = 0, h = ov_n;  // first older version at or after edge b
    while (l < h) {
      const int64_t mid = (l + h) >> 1;
      if (ov_edge[mid] < b) l = mid + 1; else h = mid;
    }
    int64_t x = b;  // edges [b, x) checked: their first versions failed
    for (int64_t o = l; o < ov_n && ov_edge[o] < e;) {
      const int64_t ge = ov_edge[o];
      bool kept = false;
      for (; x <= ge && !kept; x++) kept = flags[off[k] + (x - b)] != 0;
      if (kept) break;  // an ordinary row comes first: firstLoop ends there
      bool hit = false;
      for (; o < ov_n && ov_edge[o] == ge && !hit; o++) {
        bool pass;
        if (PK == PK_FAST) {
          pass = (ofp.present && !ofp.present[o]) ? true
                                                   : fast_cmp(ofp.op, static_cast<const int64_t*>(ofp.data)[o], ofp.k);
        } else {
          const Val v = eval_program(prog, oenv, o, int32_t(lo) + f, 0);
          pass = v.t == VT_ERR ? true : as_bool(v);  // storage: an eval error keeps the edge
        }
        if (pass) {
          x_old[k] = o;
          x_ge[k] = ge;
          hit = true;
        }
      }
      if (hit) break;
    }
  }
}
// merged row list: entry k's older-version row (if any) goes first, then its kept rows.
// cx = inclusive count of entries with an older-version row.
__global__ void k_merge_kept(const int64_t* ge, const int64_t* owner, int64_t m, const int64_t* cx, int64_t* mge,
                             int64_t* mold, int64_t* mowner) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t k = owner[i];
    const int64_t pos = i + cx[k];
    mge[pos] = ge[i];
    mold[pos] = -1;
    mowner[pos] = k;
  }
}
__global__ void k_merge_old(const int64_t* x_old, const int64_t* x_ge, int64_t nF, const int64_t* owner, int64_t m,
                            const int64_t* cx, int64_t* mge, int64_t* mold, int64_t* mowner) {
  for (int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; k < nF; k += int64_t(gridDim.x) * blockDim.x) {
    if (x_old[k] < 0) continue;
    int64_t l = 0, h = m;  // kept rows of entries < k
    while (l < h) {
      const int64_t mid = (l + h) >> 1;
      if (owner[mid] < k) l = mid + 1; else h = mid;
    }
    const int64_t pos = l + cx[k] - 1;
    mge[pos] = x_ge[k];
    mold[pos] = x_old[k];
    mowner[pos] = k;
  }
}

__global__ void k_str_gather(const int64_t* ge, const int64_t* old, int64_t m, const int64_t* src_off,
                             const uint8_t* src_bytes, const int64_t* osrc_off, const uint8_t* osrc_bytes,
                             const int64_t* dst_off, uint8_t* dst) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    int64_t len = dst_off[i + 1] - dst_off[i];
    const bool o = old && old[i] >= 0;
    const uint8_t* s = o ? osrc_bytes + osrc_off[old[i]] : src_bytes + src_off[ge[i]];
    for (int64_t j = 0; j < len; j++) dst[dst_off[i] + j] = s[j];
  }
}

// tag column values of the returned vertices (gidx list): value bits, presence state, part, and
// STRING (offset, length) into the column's bytes
__global__ void k_tag_fetch(const int32_t* g, int64_t m, const int64_t* data, const uint8_t* present,
                            const int32_t* tpart, const int64_t* str_off, int64_t* val, uint8_t* state,
                            int32_t* part, int64_t* soff, int64_t* slen) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t x = g[i];
    const bool ok = x >= 0;
    val[i] = ok ? data[x] : 0;
    state[i] = ok ? present[x] : 0;
    part[i] = ok ? tpart[x] : -1;
    if (str_off) {
      soff[i] = ok ? str_off[x] : 0;
      slen[i] = ok ? str_off[x + 1] - str_off[x] : 0;
    }
  }
}
__global__ void k_bytes_gather(const int64_t* soff, const int64_t* doff, int64_t m, const uint8_t* src, uint8_t* dst) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    for (int64_t j = 0; j < doff[i + 1] - doff[i]; j++) dst[doff[i] + j] = src[soff[i] + j];
}

namespace {

// a SOURCE / DEST tag prop of the request: read from the vertex row of each returned vertex
// (tagContexts_, QueryBaseProcessor.inl:40-70; QueryBoundProcessor.cpp:19-31)
struct TagReq {
  const TagSpace* ts;
  size_t field;
  const PropCol& col() const { return ts->cols[field]; }
};

// parts not held by this rank fail with E_PART_NOT_FOUND (NebulaStore::engine, BaseProcessor.inl:14-27)
inline bool part_held(const Ctx& c, int32_t p) {
  return p >= 0 && p <= c.num_parts && owner_of_part(p, c.world) == c.rank;
}
// A vertex's tag row (k_tag_fetch: state 1 = a row of the vid's own part, 2 = of a foreign part
// only) is visible to a request entry naming part rp when it sits in rp: collectVertexProps scans
// prefix(request part, vid, tag) (QueryBaseProcessor.inl:309-333)
inline bool tag_row_visible(const Ctx& c, uint8_t state, int32_t row_part, int32_t rp, int64_t vid) {
  return (state == 1 && rp == part_of_vid(vid, c.num_parts)) || (state == 2 && rp == row_part);
}

// ends the query's device time once the stream has drained: ev[0] -> here is Timing::total_ms
void end_device_time(Ctx& c) {
  hipEventRecord(c.ev[1], c.stream);
  NBG_HIP(hipStreamSynchronize(c.stream));
  float ms = 0;
  hipEventElapsedTime(&ms, c.ev[0], c.ev[1]);
  c.timing.total_ms = ms;
}

// one cell of the stats row: SUM 1 / COUNT 2 as INT, AVG 3 as DOUBLE
void push_stat_cell(HostRows& h, int32_t stat, int64_t sum, int64_t cnt) {
  h.types.push_back(stat == 3 ? NBG_T_DOUBLE : NBG_T_INT);
  h.host.emplace_back(8);
  if (stat == 3) {
    const double avg = double(sum) / double(int32_t(cnt));  // count_ is int32 (CommonUtils.h:51)
    memcpy(h.host.back().data(), &avg, 8);
  } else {
    const int64_t v = stat == 2 ? int64_t(int32_t(cnt)) : sum;
    memcpy(h.host.back().data(), &v, 8);
  }
  h.str_off.push_back(nullptr);
}

// k_tag_fetch of one tag column at the n vertices g, copied to the host (strings: with offsets / lengths)
struct TagFetch {
  DevBuf dval, dstate, dpart, dsoff, dslen;
  std::vector<int64_t> val, soff, slen;
  std::vector<uint8_t> state;
  std::vector<int32_t> part;
  void run(Ctx& c, const TagReq& tr, const int32_t* g, int64_t n, bool strings) {
    const size_t cap = size_t(std::max<int64_t>(n, 1)), sn = size_t(n);
    const PropCol& pc = tr.col();
    for (DevBuf* d : {&dval, &dsoff, &dslen}) d->alloc(cap * 8);
    dstate.alloc(cap);
    dpart.alloc(cap * 4);
    for (auto* v : {&val, &soff, &slen}) v->resize(cap);
    state.resize(cap);
    part.resize(cap);
    if (!n) return;
    k_tag_fetch<<<grid_cap(n), 256, 0, c.stream>>>(g, n, pc.data.as<int64_t>(), pc.present.as<uint8_t>(),
                                                   tr.ts->part.as<int32_t>(), strings ? pc.str_off.as<int64_t>() : nullptr,
                                                   dval.as<int64_t>(), dstate.as<uint8_t>(), dpart.as<int32_t>(),
                                                   dsoff.as<int64_t>(), dslen.as<int64_t>());
    NBG_HIP(hipGetLastError());
    NBG_HIP(hipMemcpyAsync(val.data(), dval.p, sn * 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipMemcpyAsync(state.data(), dstate.p, sn, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipMemcpyAsync(part.data(), dpart.p, sn * 4, hipMemcpyDeviceToHost, c.stream));
    if (strings) {
      NBG_HIP(hipMemcpyAsync(soff.data(), dsoff.p, sn * 8, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipMemcpyAsync(slen.data(), dslen.p, sn * 8, hipMemcpyDeviceToHost, c.stream));
    }
    NBG_HIP(hipStreamSynchronize(c.stream));  // the caller reads the host copies next
  }
};

// Fills h->vertex_* for the returned vertices (h->vertex_ids, request parts vparts): a value is
// visible by tag_row_visible, else absent (the reference then skips the prop in the vertex row,
// RowWriter without it).
void fetch_vertex_tags(Ctx& c, HostRows* h, const std::vector<int32_t>& vparts, const std::vector<TagReq>& treq) {
  const int64_t nv = int64_t(h->vertex_ids.size());
  const size_t cap = size_t(std::max<int64_t>(nv, 1));
  DevBuf dv, dg;
  dv.alloc(cap * 8);
  dg.alloc(cap * 4);
  if (nv) {
    NBG_HIP(hipMemcpyAsync(dv.p, h->vertex_ids.data(), size_t(nv) * 8, hipMemcpyHostToDevice, c.stream));
    lookup_gidx(c, dv.as<int64_t>(), dg.as<int32_t>(), nv);
  }
  TagFetch tf;
  for (const TagReq& tr : treq) {
    const PropCol& pc = tr.col();
    const bool is_str = pc.type == NBG_T_STRING;
    tf.run(c, tr, dg.as<int32_t>(), nv, is_str);
    std::vector<uint8_t> pres(cap, 0);
    for (size_t i = 0; i < size_t(nv); i++)
      pres[i] = tag_row_visible(c, tf.state[i], tf.part[i], vparts[i], h->vertex_ids[i]);
    h->vertex_types.push_back(column_result_type(pc.type));
    h->vertex_present.push_back(pres);
    if (is_str) {
      std::vector<int64_t> offs(size_t(nv) + 1, 0);
      for (size_t i = 0; i < size_t(nv); i++) offs[i + 1] = offs[i] + (pres[i] ? tf.slen[i] : 0);
      std::vector<uint8_t> bytes(size_t(offs[size_t(nv)]) + 8);
      if (offs[size_t(nv)]) {
        DevBuf ddo, dbytes;
        ddo.alloc(size_t(nv + 1) * 8);
        dbytes.alloc(size_t(offs[size_t(nv)]) + 8);
        NBG_HIP(hipMemcpyAsync(ddo.p, offs.data(), size_t(nv + 1) * 8, hipMemcpyHostToDevice, c.stream));
        k_bytes_gather<<<grid_cap(nv), 256, 0, c.stream>>>(tf.dsoff.as<int64_t>(), ddo.as<int64_t>(), nv,
                                                           pc.str_bytes.as<uint8_t>(), dbytes.as<uint8_t>());
        NBG_HIP(hipMemcpyAsync(bytes.data(), dbytes.p, size_t(offs[size_t(nv)]), hipMemcpyDeviceToHost, c.stream));
        NBG_HIP(hipStreamSynchronize(c.stream));
      }
      h->vertex_host.push_back(std::move(bytes));
      h->vertex_host_off.push_back(std::move(offs));
    } else {
      std::vector<uint8_t> raw(cap * 8);
      if (pc.type != NBG_T_BOOL) memcpy(raw.data(), tf.val.data(), size_t(nv) * 8);
      else
        for (size_t i = 0; i < size_t(nv); i++) raw[i] = uint8_t(tf.val[i] != 0);
      h->vertex_host.push_back(std::move(raw));
      h->vertex_host_off.emplace_back();
    }
  }
}

// One getBound / boundStats request: the parsed columns, the compiled filter, the kept rows on
// the device, and the phases get_bound_run calls in order.
struct BoundQuery {
  Ctx& c;
  const int32_t* parts;  // the request entries: (parts[i], vids[i]), i < N
  const int64_t* vids;
  const int64_t N;
  const nbg_prop_def* cols;
  const size_t ncols;
  const int32_t* stats;  // boundStats: cpp2::StatType per column (null: getBound)
  nbg_rows* out;
  std::unique_ptr<HostRows> h = std::make_unique<HostRows>();

  // ---- parse_request() ----
  bool in_bound = false;
  EdgeSpace* es = nullptr;
  Csr* csr = nullptr;
  std::vector<int32_t> req_parts;  // the distinct parts, in request order
  BoundCols bc{};                  // edge columns
  std::vector<TagReq> treq;        // tag columns
  std::vector<std::pair<int, int>> sorder;  // stats: output order (retIndex), {0, bc index} or {1, treq index}
  std::vector<int32_t> tstat;               // stats: the stat type of each tag column

  // ---- compile_filter() ----
  bool has_filter = false;
  Program fprog{};
  FastPred fpk{};
  FastArgs fp{};

  // ---- build_frontier(): the request entries with >= 1 edge, as local rows ----
  int64_t lo = 0, E = 0, nF = 0;
  DevBuf dg, dcF, dcoff;        // gidx [N] of the request entries; local row [nF], first edge slot [nF + 1]
  std::vector<int64_t> centry;  // frontier entry -> request entry
  std::vector<int32_t> cF;      // host sources of dcF / dcoff (async copies: kept with the query)
  std::vector<int64_t> coff;

  // ---- scan(), first_loop(): the kept rows, in row order ----
  EvalEnv env{};
  DevBuf dprog, flags, ovtab;
  const PropDev* oprops = nullptr;  // the older versions' columns (Csr::ov_props), when read
  int64_t m = 0;
  DevBuf geb, owner, oldb;      // int64 [m]: edge index, frontier entry, older-version row (empty: none)
  std::vector<int64_t> howner;  // emit_rows(): host copy of owner

  // request-level validation fails every part of the request (QueryBaseProcessor.inl:470-477)
  int32_t fail_all(int32_t code) {
    for (auto p : req_parts) {
      h->failed_parts.push_back(p);
      h->failed_codes.push_back(code);
    }
    return hand_out(0, 0);
  }
  int32_t hand_out(int64_t nrows, int64_t scanned) {
    fill_rows(out, std::move(h), nrows, false);
    out->edges_scanned = uint64_t(scanned);
    return NBG_OK;
  }

  // Request parts, edge columns into bc, tag columns into treq, the stat order.  Returns the code
  // every part fails with (the first offending column in request order decides), or NBG_OK.
  int32_t parse_request(int32_t et) {
    for (int64_t i = 0; i < N; i++)
      if (std::find(req_parts.begin(), req_parts.end(), parts[i]) == req_parts.end()) req_parts.push_back(parts[i]);
    in_bound = et < 0;
    auto it = c.edges.find(in_bound ? -et : et);
    if (it == c.edges.end()) return NBG_E_EDGE_PROP_NOT_FOUND;
    es = &it->second;
    csr = in_bound ? &es->in : &es->out;
    for (size_t i = 0; i < ncols; i++) {
      const int32_t rc = cols[i].owner != NBG_OWNER_EDGE ? parse_tag_column(i) : parse_edge_column(i);
      if (rc != NBG_OK) return rc;
    }
    return NBG_OK;
  }
  // the last field of that name (-1: none)
  static int field_index(const std::vector<Field>& fields, const char* name) {
    int idx = -1;
    for (size_t f = 0; f < fields.size(); f++)
      if (fields[f].name == (name ? name : "")) idx = int(f);
    return idx;
  }
  // validOperation (QueryBaseProcessor.inl:18-35, 62-64): SUM / AVG need a numeric column
  static int32_t valid_stat(int32_t st, int32_t type) {
    if (st < 1 || st > 3) throw Error(NBG_E_INVALID_ARG, "stat type must be SUM 1, COUNT 2 or AVG 3");
    return st != 2 && (type == NBG_T_BOOL || type == NBG_T_STRING) ? NBG_E_IMPROPER_DATA_TYPE : NBG_OK;
  }
  int32_t parse_tag_column(size_t i) {
    auto tit = c.tags.find(cols[i].tag_id);
    if (tit == c.tags.end()) return NBG_E_TAG_PROP_NOT_FOUND;
    const int fi = field_index(tit->second.fields, cols[i].name);
    if (fi < 0) return NBG_E_IMPROPER_DATA_TYPE;
    if (stats) {
      if (valid_stat(stats[i], tit->second.fields[size_t(fi)].type) != NBG_OK) return NBG_E_IMPROPER_DATA_TYPE;
      sorder.emplace_back(1, int(treq.size()));
      tstat.push_back(stats[i]);
    }
    treq.push_back(TagReq{&tit->second, size_t(fi)});
    return NBG_OK;
  }
  int32_t parse_edge_column(size_t i) {
    const std::string name = cols[i].name ? cols[i].name : "";
    BoundCol b{};
    if (name == "_dst") b.kind = 1;
    else if (name == "_src") b.kind = 2;
    else if (name == "_rank") b.kind = 3;
    else if (name == "_type") b.kind = 4;
    if (b.kind) {
      b.type = NBG_T_INT;
    } else if (!in_bound) {
      b.prop = field_index(es->fields, cols[i].name);
      if (b.prop < 0) return NBG_E_IMPROPER_DATA_TYPE;
      b.type = column_result_type(es->fields[size_t(b.prop)].type);
    } else {
      return NBG_OK;  // "InBound has none props, skip it!"
    }
    if (stats) {
      b.stat = stats[i];
      if (valid_stat(b.stat, b.type) != NBG_OK) return NBG_E_IMPROPER_DATA_TYPE;
    }
    if (bc.n >= kMaxBoundCols) throw Error(NBG_E_UNSUPPORTED, "too many return columns");
    if (stats) sorder.emplace_back(0, bc.n);
    bc.c[bc.n++] = b;
    return NBG_OK;
  }

  int32_t compile_filter(const uint8_t* filter, size_t flen) {
    has_filter = flen != 0;
    if (has_filter) {
      std::string msg;
      int32_t rc = compile_expr(filter, flen, es->fields, false, !in_bound, &fprog, &msg, &c.tag_refs);
      if (rc == NBG_E_UNSUPPORTED) throw Error(rc, "filter: " + msg);
      if (rc != NBG_OK) return NBG_E_INVALID_FILTER;
      fpk = classify_pred(fprog, es->fields);
    }
    fp = fast_args(*csr, fpk);
    return NBG_OK;
  }

  // Request entry -> local row (k_bound_frontier) and the degree scan; entries without an edge are
  // dropped on the host (the tile owner search needs deg >= 1).  The query's Timing starts here.
  void build_frontier() {
    lo = c.owned_lo();
    for (auto p : req_parts)
      if (!part_held(c, p)) {
        h->failed_parts.push_back(p);
        h->failed_codes.push_back(NBG_E_PART_NOT_FOUND);
      }
    DevBuf dv, dp, dF, ddeg, doff;
    for (DevBuf* d : {&dv, &ddeg, &doff}) d->alloc(size_t(N + 1) * 8);
    for (DevBuf* d : {&dp, &dg, &dF}) d->alloc(size_t(N + 1) * 4);
    if (N) {
      NBG_HIP(hipMemcpyAsync(dv.p, vids, size_t(N) * 8, hipMemcpyHostToDevice, c.stream));
      NBG_HIP(hipMemcpyAsync(dp.p, parts, size_t(N) * 4, hipMemcpyHostToDevice, c.stream));
      lookup_gidx(c, dv.as<int64_t>(), dg.as<int32_t>(), N);
      k_bound_frontier<<<grid_cap(N), 256, 0, c.stream>>>(dp.as<int32_t>(), dg.as<int32_t>(), N, lo, c.owned_hi(),
                                                        csr->row_part.as<int32_t>(), dF.as<int32_t>());
    }
    k_degrees_masked<<<grid_cap(N + 1), 256, 0, c.stream>>>(dF.as<int32_t>(), N, csr->row_ptr.as<int64_t>(), ddeg.as<int64_t>());
    exclusive_scan_dev<int64_t>(c, ddeg.as<int64_t>(), doff.as<int64_t>(), N + 1);
    std::vector<int64_t> hoff(size_t(N + 1));
    NBG_HIP(hipMemcpyAsync(hoff.data(), doff.p, size_t(N + 1) * 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    E = hoff[size_t(N)];
    c.timing = Timing{};
    timing_reset(c);
    if (c.host_stage_used) NBG_HIP(hipStreamSynchronize(c.stream));  // a failed query's copies
    c.host_stage_used = 0;
    c.timing.edges_scanned = uint64_t(E);
    std::vector<int32_t> hF(static_cast<size_t>(N));
    if (N) NBG_HIP(hipMemcpy(hF.data(), dF.p, size_t(N) * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < N; i++)
      if (hoff[size_t(i + 1)] > hoff[size_t(i)]) {
        cF.push_back(hF[size_t(i)]);
        coff.push_back(hoff[size_t(i)]);
        centry.push_back(i);
      }
    coff.push_back(E);
    nF = int64_t(cF.size());
    dcF.alloc(size_t(nF + 1) * 4);
    dcoff.alloc(size_t(nF + 1) * 8);
    if (nF) NBG_HIP(hipMemcpyAsync(dcF.p, cF.data(), size_t(nF) * 4, hipMemcpyHostToDevice, c.stream));
    NBG_HIP(hipMemcpyAsync(dcoff.p, coff.data(), size_t(nF + 1) * 8, hipMemcpyHostToDevice, c.stream));
  }

  // The filter over every edge slot (flags), the select of the kept slots, then their frontier
  // entry (owner) and edge index (geb).  The query's device time starts here (ev[0]).
  void scan() {
    flags.alloc(size_t(E + 1));
    env = make_env(c, *es, *csr, in_bound ? -es->type : es->type);
    env.storage = 1;
    env.lo = lo;
    env.row_part = csr->row_part.as<int32_t>();
    dprog.alloc(sizeof(Program));
    NBG_HIP(hipMemcpyAsync(dprog.p, &fprog, sizeof(Program), hipMemcpyHostToDevice, c.stream));
    DevBuf cnts, slots, cnt;
    cnts.alloc(64);
    NBG_HIP(hipMemsetAsync(cnts.p, 0, 64, c.stream));
    hipEventRecord(c.ev[0], c.stream);
    if (E > 0) {
      ExpandArgs a{};
      a.F = dcF.as<int32_t>();
      a.nF = nF;
      a.off = dcoff.as<int64_t>();
      a.row_ptr = csr->row_ptr.as<int64_t>();
      a.col = csr->col.as<int32_t>();
      a.lo = lo;
      a.flags = flags.as<uint8_t>();
      a.err = cnts.as<unsigned long long>();
      a.storage = 1;
      expand_flags(c, a, fpk.kind, fp, dprog.as<Program>(), env, E);
      c.timing.expand_bytes += expand_bytes(nF, E, fpk.kind == PK_FAST ? fp.width : 0, EXP_FLAGS);
      slots.alloc(size_t(E + 1) * 8);
      cnt.alloc(8);
      select_dev(c, rocprim::counting_iterator<int64_t>(0), flags.as<uint8_t>(), slots.as<int64_t>(),
                 cnt.as<uint64_t>(), E);
      uint64_t hm = 0;
      NBG_HIP(hipMemcpyAsync(&hm, cnt.p, 8, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipStreamSynchronize(c.stream));
      m = int64_t(hm);
    }
    owner.alloc(size_t(m + 1) * 8);
    geb.alloc(size_t(m + 1) * 8);
    if (m) {
      k_slot_owner<<<grid_cap(m), 256, 0, c.stream>>>(slots.as<int64_t>(), m, dcoff.as<int64_t>(), nF, owner.as<int64_t>());
      k_slot_ge<<<grid_cap(m), 256, 0, c.stream>>>(slots.as<int64_t>(), owner.as<int64_t>(), m, dcoff.as<int64_t>(),
                                                   dcF.as<int32_t>(), csr->row_ptr.as<int64_t>(), geb.as<int64_t>());
      NBG_HIP(hipGetLastError());
    }
  }

  // firstLoop (multi-version data under a push-down filter): older versions emitted ahead of a
  // request entry's rows (QueryBaseProcessor.inl:349-402); the reader only exists for out-bound
  // rows with a value, so in-bound scans never evaluate the filter.  Merges them into the kept rows.
  void first_loop() {
    if (!has_filter || in_bound || csr->ov_n <= 0 || nF <= 0) return;
    std::vector<PropDev> tab;
    append_prop_devs(tab, csr->ov_props);
    ovtab.alloc(sizeof(PropDev) * std::max<size_t>(tab.size(), 1));
    if (!tab.empty()) c.h2d(ovtab.p, tab.data(), sizeof(PropDev) * tab.size());
    oprops = ovtab.as<PropDev>();
    EvalEnv oenv = env;
    oenv.props = oprops;
    FastArgs ofp{};
    if (fpk.kind == PK_FAST) {
      const PropCol& oc = csr->ov_props[size_t(fpk.col)];
      ofp = FastArgs{oc.data.p, oc.present.as<uint8_t>(), 8, fpk.op, fpk.k};
    }
    DevBuf xo, xg, cx;
    for (DevBuf* d : {&xo, &xg, &cx}) d->alloc(size_t(nF) * 8);
    auto go = [&](auto kern) {
      kern<<<grid_cap(nF), 256, 0, c.stream>>>(dcF.as<int32_t>(), dcoff.as<int64_t>(), nF, csr->row_ptr.as<int64_t>(),
                                               flags.as<uint8_t>(), csr->ov_edge.as<int64_t>(), csr->ov_n,
                                               dprog.as<Program>(), oenv, ofp, lo, xo.as<int64_t>(), xg.as<int64_t>());
    };
    if (fpk.kind == PK_FAST) go(k_first_loop<PK_FAST>);
    else go(k_first_loop<PK_VM>);
    NBG_HIP(hipGetLastError());
    auto has = rocprim::make_transform_iterator(xo.as<int64_t>(), [] __device__(int64_t v) -> int64_t { return v >= 0; });
    size_t tb = 0;
    NBG_HIP(rocprim::inclusive_scan(nullptr, tb, has, cx.as<int64_t>(), size_t(nF), rocprim::plus<int64_t>(), c.stream));
    c.ws_tmp.ensure(tb);
    NBG_HIP(rocprim::inclusive_scan(c.ws_tmp.p, tb, has, cx.as<int64_t>(), size_t(nF), rocprim::plus<int64_t>(), c.stream));
    int64_t X = 0;
    NBG_HIP(hipMemcpyAsync(&X, cx.as<int64_t>() + nF - 1, 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    if (X <= 0) return;
    DevBuf mge, mold, mown;
    for (DevBuf* d : {&mge, &mold, &mown}) d->alloc(size_t(m + X + 1) * 8);
    if (m)
      k_merge_kept<<<grid_cap(m), 256, 0, c.stream>>>(geb.as<int64_t>(), owner.as<int64_t>(), m, cx.as<int64_t>(),
                                                      mge.as<int64_t>(), mold.as<int64_t>(), mown.as<int64_t>());
    k_merge_old<<<grid_cap(nF), 256, 0, c.stream>>>(xo.as<int64_t>(), xg.as<int64_t>(), nF, owner.as<int64_t>(), m,
                                                    cx.as<int64_t>(), mge.as<int64_t>(), mold.as<int64_t>(),
                                                    mown.as<int64_t>());
    NBG_HIP(hipGetLastError());
    m += X;
    geb = std::move(mge);
    owner = std::move(mown);
    oldb = std::move(mold);
  }

  // SOURCE / DEST tag columns (QueryStatsProcessor::processVertex, QueryStatsProcessor.cpp:69-82):
  // every request entry of an owned part collects the newest version of its vertex row in that
  // part (collectVertexProps, QueryBaseProcessor.inl:309-333), when visible, into the column's
  // sum / count (StatsCollector, Collector.h:66-94); entries without the row add nothing
  void sum_tag_column(size_t t, const TagFetch& tf, int64_t& sum, int64_t& cnt) const {
    const int32_t ty = treq[t].col().type;
    for (int64_t i = 0; i < N; i++) {
      if (!part_held(c, parts[i])) continue;  // failed part
      if (!tag_row_visible(c, tf.state[size_t(i)], tf.part[size_t(i)], parts[i], vids[i])) continue;
      cnt++;
      if (ty == NBG_T_DOUBLE || ty == NBG_T_FLOAT) {
        if (tstat[t] != 2)
          throw Error(NBG_E_UNSUPPORTED, "SUM/AVG over a double prop (the reference's int64 sum throws bad_get)");
      } else if (ty != NBG_T_BOOL && ty != NBG_T_STRING) {
        sum = int64_t(uint64_t(sum) + uint64_t(tf.val[size_t(i)]));
      }
    }
  }
  // boundStats: one row, per column SUM (INT) / COUNT (INT) / AVG (DOUBLE), in request order
  // (retIndex); it carries no edges_scanned
  int32_t emit_stats() {
    // edge columns: k_bound_stats over the kept rows, ha[2i] = sum, ha[2i + 1] = count of column i
    DevBuf acc;
    std::vector<unsigned long long> ha(size_t(2 * bc.n + 2));
    acc.alloc(ha.size() * 8);
    NBG_HIP(hipMemsetAsync(acc.p, 0, ha.size() * 8, c.stream));
    if (m) {
      for (int i = 0; i < bc.n; i++)
        k_bound_stats<<<grid_cap(m, 256, 1024), 256, 0, c.stream>>>(geb.as<int64_t>(), oldb.as<int64_t>(), owner.as<int64_t>(),
                                                                    m, dcF.as<int32_t>(), lo, env, oprops, bc.c[i],
                                                                    acc.as<unsigned long long>() + 2 * i);
      NBG_HIP(hipGetLastError());
    }
    NBG_HIP(hipMemcpyAsync(ha.data(), acc.p, ha.size() * 8, hipMemcpyDeviceToHost, c.stream));
    std::vector<TagFetch> tf(treq.size());
    for (size_t t = 0; t < treq.size(); t++) tf[t].run(c, treq[t], dg.as<int32_t>(), N, false);
    end_device_time(c);
    std::vector<int64_t> tsum(treq.size(), 0), tcnt(treq.size(), 0);
    for (size_t t = 0; t < treq.size(); t++) sum_tag_column(t, tf[t], tsum[t], tcnt[t]);
    for (const auto& so : sorder) {
      if (so.first == 1) {
        push_stat_cell(*h, tstat[size_t(so.second)], tsum[size_t(so.second)], tcnt[size_t(so.second)]);
        continue;
      }
      const BoundCol& b = bc.c[so.second];
      const int64_t sum = int64_t(ha[size_t(2 * so.second)]);
      const int64_t cnt = int64_t(ha[size_t(2 * so.second + 1)]);
      if (b.stat != 2 && b.type == NBG_T_DOUBLE && cnt > 0)
        throw Error(NBG_E_UNSUPPORTED, "SUM/AVG over a double prop (the reference's int64 sum throws bad_get)");
      push_stat_cell(*h, b.stat, sum, cnt);
    }
    for (auto& hc : h->host) h->cols.push_back(hc.data());
    return hand_out(1, 0);
  }

  // The kept rows' columns: k_bound_rows writes the fixed-width ones and the STRING lengths, then
  // each column goes to the host (a STRING column's bytes through k_str_gather); absent values
  // (INT64_MIN marker / -1 length) stay absent.
  void emit_rows() {
    std::vector<DevBuf> dcols(size_t(bc.n));  // per column: its values, or a STRING column's lengths
    for (int i = 0; i < bc.n; i++) {
      BoundCol& b = bc.c[i];
      dcols[size_t(i)].alloc(size_t(m + 1) * (b.type == NBG_T_BOOL ? 1 : 8));
      if (b.type == NBG_T_STRING) b.str_len = dcols[size_t(i)].as<int64_t>();
      else b.out = dcols[size_t(i)].p;
    }
    const int64_t* oldp = oldb.as<int64_t>();
    howner.resize(static_cast<size_t>(m));
    if (m) {
      k_bound_rows<<<grid_cap(m), 256, 0, c.stream>>>(geb.as<int64_t>(), oldp, owner.as<int64_t>(), m,
                                                    dcF.as<int32_t>(), lo, env, oprops, bc);
      NBG_HIP(hipGetLastError());
      NBG_HIP(hipMemcpyAsync(howner.data(), owner.p, size_t(m) * 8, hipMemcpyDeviceToHost, c.stream));
    }
    end_device_time(c);
    for (int i = 0; i < bc.n; i++) {
      const BoundCol& b = bc.c[i];
      h->types.push_back(b.type);
      if (b.type == NBG_T_STRING) {
        std::vector<int64_t> lens(static_cast<size_t>(m));
        if (m) NBG_HIP(hipMemcpy(lens.data(), dcols[size_t(i)].p, size_t(m) * 8, hipMemcpyDeviceToHost));
        std::vector<int64_t> offs(size_t(m) + 1, 0);
        for (int64_t r = 0; r < m; r++) offs[size_t(r + 1)] = offs[size_t(r)] + std::max<int64_t>(lens[size_t(r)], 0);
        DevBuf doffs, dbytes;
        doffs.alloc(size_t(m + 1) * 8);
        dbytes.alloc(size_t(offs[size_t(m)]) + 8);
        NBG_HIP(hipMemcpy(doffs.p, offs.data(), size_t(m + 1) * 8, hipMemcpyHostToDevice));
        const PropCol& pc = csr->props[size_t(b.prop)];
        const PropCol* opc = oldp ? &csr->ov_props[size_t(b.prop)] : nullptr;
        if (m)
          k_str_gather<<<grid_cap(m), 256, 0, c.stream>>>(
              geb.as<int64_t>(), oldp, m, pc.str_off.as<int64_t>(), pc.str_bytes.as<uint8_t>(),
              opc ? opc->str_off.as<int64_t>() : nullptr, opc ? opc->str_bytes.as<uint8_t>() : nullptr,
              doffs.as<int64_t>(), dbytes.as<uint8_t>());
        NBG_HIP(hipStreamSynchronize(c.stream));
        h->host.emplace_back(size_t(offs[size_t(m)]) + 8);
        if (offs[size_t(m)]) NBG_HIP(hipMemcpy(h->host.back().data(), dbytes.p, size_t(offs[size_t(m)]), hipMemcpyDeviceToHost));
        h->host_off.push_back(offs);
        h->cols.push_back(h->host.back().data());
        h->str_off.push_back(h->host_off.back().data());
      } else {
        size_t w = b.type == NBG_T_BOOL ? 1 : 8;
        h->host.emplace_back(size_t(m) * w + 8);
        if (m) NBG_HIP(hipMemcpy(h->host.back().data(), dcols[size_t(i)].p, size_t(m) * w, hipMemcpyDeviceToHost));
        h->cols.push_back(h->host.back().data());
        h->str_off.push_back(nullptr);
      }
    }
  }

  // vertices with >= 1 row, in request order (QueryBoundProcessor.cpp:61-67), and their tag props
  void emit_vertices() {
    h->row_vertex.resize(size_t(m));
    std::vector<int32_t> vparts;  // request part of each returned vertex (its first request entry)
    int64_t last = -1;
    for (int64_t r = 0; r < m; r++) {
      int64_t k = howner[size_t(r)];
      int64_t entry = centry[size_t(k)];
      h->row_vertex[size_t(r)] = vids[entry];
      if (k != last) {
        h->vertex_ids.push_back(vids[entry]);
        h->vertex_row_offsets.push_back(r);
        vparts.push_back(parts[entry]);
        last = k;
      }
    }
    h->vertex_row_offsets.push_back(m);
    if (!treq.empty()) fetch_vertex_tags(c, h.get(), vparts, treq);
  }
};

}  // namespace

int32_t get_bound_run(Ctx& c, int32_t et, const int32_t* parts, const int64_t* vids, size_t n, const uint8_t* filter,
                      size_t flen, const nbg_prop_def* cols, size_t ncols, nbg_rows* out, const int32_t* stats) {
  PoolScope pool_scope(query_pool(c));
  if (!c.finalized) throw Error(NBG_E_STATE, "snapshot not finalized");
  BoundQuery q{c, parts, vids, int64_t(n), cols, ncols, stats, out};
  if (const int32_t rc = q.parse_request(et); rc != NBG_OK) return q.fail_all(rc);
  if (const int32_t rc = q.compile_filter(filter, flen); rc != NBG_OK) return q.fail_all(rc);
  q.build_frontier();
  q.scan();
  q.first_loop();
  if (stats) return q.emit_stats();
  q.emit_rows();
  q.emit_vertices();
  return q.hand_out(q.m, q.E);
}

}  // namespace nbg
