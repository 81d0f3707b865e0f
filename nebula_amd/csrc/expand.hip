// expand.hip -- the top-down neighbour expansion on MI355X (gfx950).
//
// Replaces, for a whole frontier at once:
//   * QueryBaseProcessor::collectEdgeProps prefix scan + filter (QueryBaseProcessor.inl:335-405)
//     -> k_expand: edge-balanced tiles over the frontier's CSR rows;
//   * GoExecutor::getDstIdsFromResp unordered_set (GoExecutor.cpp:407-431)
//     -> byte-map marks (plain stores, no atomics), compacted by frontier.hip's k_compact;
//   * processFinalResult WHERE (GoExecutor.cpp:585-782) -> the predicate fused into k_expand.
//
// Load balance (power-law degrees): the frontier's degrees are prefix-summed; each 256-thread
// workgroup takes a fixed tile of 2048 consecutive edges of that flattened space, stages the
// (<= 2048) frontier entries covering it in LDS, and each lane finds its edge's owner by a
// binary search in LDS.  Consecutive lanes read consecutive adjacency entries, so the col /
// prop loads of a tile are coalesced whatever the degree distribution (a supernode simply
// spans many tiles).
//
// Used by GO (traverse.hip) and by storage getBound (bound.hip: expand_flags, make_env, fast_args).
// The kernels' expression VM is expr_device.h.
#include <algorithm>
#include <vector>

#include "device_common.h"
#include "engine.h"
#include "expr_device.h"
#include "go_device.h"
#include "go_launch.h"
#include "program.h"
#include "qpred.h"
#include "query_common.h"

namespace nbg {

template <int MODE, int PK>
__global__ __launch_bounds__(kThreads) void k_expand(ExpandArgs a, FastArgs fp, const Program* __restrict__ prog,
                                                     EvalEnv env) {
  __shared__ int32_t s_off[kTile + 1];  // off[k] - e0 (fits: tile-relative)
  __shared__ int64_t s_rs[kTile];       // row_ptr[F[k]] - off[k]
  __shared__ int32_t s_src[kTile];      // F[k]
  __shared__ int32_t s_scan[kThreads / 64];
  int32_t* s_own = s_off;               // after the owner map is built: owner k of tile slot j
  __shared__ int64_t s_hdr[2];
  __shared__ uint32_t s_wsum[kThreads / 64];
  __shared__ unsigned long long s_base;
  const int64_t nF = a.nF;
  const int64_t E = a.off[nF];
  const int64_t ntiles = (E + kTile - 1) / kTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t e0 = t * kTile;
    const int64_t e1 = min(e0 + int64_t(kTile), E);
    if (threadIdx.x == 0 && a.tile_row) {
      int64_t i0, cnt;
      tile_entries(a.tile_row, a.off, nF, t, e1, E, i0, cnt);
      s_hdr[0] = i0;
      s_hdr[1] = cnt;
    } else if (threadIdx.x == 0) {
      // i0 = last k with off[k] <= e0 ; i1 = last k with off[k] <= e1 - 1
      int64_t lo = 0, hi = nF;  // off[lo] <= e0 < off[hi] invariant (off[0] = 0, off[nF] = E)
      while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (a.off[mid] <= e0) lo = mid; else hi = mid;
      }
      int64_t i0 = lo;
      lo = i0;
      hi = nF;
      while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (a.off[mid] <= e1 - 1) lo = mid; else hi = mid;
      }
      s_hdr[0] = i0;
      s_hdr[1] = lo - i0 + 1;
    }
    __syncthreads();
    const int64_t i0 = s_hdr[0];
    const int64_t cnt64 = s_hdr[1];
    // a run of zero-degree frontier entries can put more than kTile entries under one tile:
    // such a tile searches off[] in global memory instead of staging it in LDS
    const bool big = cnt64 > kTile;
    const int cnt = big ? 0 : int(cnt64);
    for (int k = threadIdx.x; k <= cnt && !big; k += kThreads) {
      int64_t o = a.off[i0 + k];
      s_off[k] = int32_t(min(o - e0, int64_t(kTile + 1)));
      if (k < cnt) {
        int32_t f = a.F[i0 + k];
        s_src[k] = f;
        s_rs[k] = a.row_ptr[f] - o;
      }
    }
    __syncthreads();
    if (!big) tile_owner_map<kTile, kThreads>(s_off, cnt, s_scan);
    // owner of tile slot j: its frontier row and (row_ptr - off) so that ge = rsk + e
    auto locate = [&](int j, int32_t& srck, int64_t& rsk) {
      const int64_t e = e0 + j;
      if (!big) {
        const int lo = s_own[j];
        srck = s_src[lo];
        rsk = s_rs[lo];
      } else {
        int64_t lo = i0, hi = i0 + cnt64;  // off[lo] <= e < off[hi]
        while (hi - lo > 1) {
          const int64_t mid = (lo + hi) >> 1;
          if (a.off[mid] <= e) lo = mid; else hi = mid;
        }
        srck = a.F[lo];
        rsk = a.row_ptr[srck] - a.off[lo];
      }
    };
    if constexpr (MODE == EXP_ROWS && PK == PK_NONE) {
      if (a.out_vid && a.col_vid && !big) {
        // plain dst-vid copy: all kItems loads of this thread in flight before the stores
        int64_t v[kItems];
#pragma unroll
        for (int r = 0; r < kItems; r++) {
          const int j = threadIdx.x + r * kThreads;
          v[r] = e0 + j < e1 ? __builtin_nontemporal_load(a.col_vid + s_rs[s_own[j]] + e0 + j) : 0;
        }
#pragma unroll
        for (int r = 0; r < kItems; r++) {
          const int64_t e = e0 + threadIdx.x + r * kThreads;
          if (e < e1) __builtin_nontemporal_store(v[r], a.out_vid + e);
        }
        __syncthreads();
        continue;
      }
    }
    if constexpr (MODE == EXP_MARK && PK == PK_NONE) {
      if (!a.mark_check && !a.root_next && !big) {
        // unfiltered marking: the thread's kItems col loads in flight before its byte stores
        int32_t d[kItems];
#pragma unroll
        for (int r = 0; r < kItems; r++) {
          const int j = threadIdx.x + r * kThreads;
          d[r] = e0 + j < e1 ? a.col[s_rs[s_own[j]] + e0 + j] : -1;
        }
#pragma unroll
        for (int r = 0; r < kItems; r++)
          if (d[r] >= 0) a.map[d[r]] = 1;
        __syncthreads();
        continue;
      }
    }
    uint32_t pm = 0;  // ROWS: items of this thread that pass
#pragma unroll 2
    for (int r = 0; r < kItems; r++) {
      const int j = threadIdx.x + r * kThreads;
      const int64_t e = e0 + j;
      const bool valid = e < e1;
      int32_t srck = 0;
      int64_t rsk = 0;
      if (valid) locate(j, srck, rsk);
      const int64_t ge = valid ? rsk + e : 0;
      bool pass = valid;
      int32_t d = 0;
      if (valid && (MODE != EXP_FLAGS || PK == PK_VM)) d = a.col[ge];
      if (PK == PK_FAST && valid) {
        if (fp.present && !fp.present[ge]) {
          if (a.storage) pass = true;
          else {
            atomicAdd(a.err, 1ull);
            pass = false;
          }
        } else {
          pass = fast_cmp(fp.op, load_int(fp.data, fp.width, ge), fp.k);
        }
      } else if (PK == PK_VM && valid) {
        Val v = eval_program(prog, env, ge, int32_t(a.lo) + srck, d);
        if (v.t == VT_ERR) {
          if (a.storage) pass = true;
          else {
            atomicAdd(a.err, 1ull);
            pass = false;
          }
        } else {
          pass = as_bool(v);
        }
      }
      if (MODE == EXP_ROWS && PK == PK_NONE && a.out_vid) {
        // every edge is a row: the row of flattened edge e is row e (no append, no atomics)
        if (valid) a.out_vid[e] = a.col_vid ? a.col_vid[ge] : a.vid_of[a.col[ge]];
      } else if (MODE == EXP_MARK) {
        if (pass) {
          if (a.mark_check) {
            if (a.map[d] == 0) a.map[d] = 1;
          } else {
            a.map[d] = 1;
          }
          if (a.root_next) atomicMin(a.root_next + d, a.root_cur[a.lo + srck]);
        }
      } else if (MODE == EXP_ROWS) {
        if (pass) pm |= 1u << r;
      } else {
        if (valid) a.flags[e] = pass;
      }
    }
    if (MODE == EXP_ROWS && !(PK == PK_NONE && a.out_vid)) {
      // block-aggregated append: one returning atomic per tile (a single counter serialises at
      // ~90 appends / us, so a per-wave append made row output the bottleneck)
      const uint32_t c0 = __popc(pm);
      const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
      uint32_t incl = c0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
      }
      if (lane == 63) s_wsum[wv] = incl;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < kThreads / 64; w++) {
          const uint32_t x = s_wsum[w];
          s_wsum[w] = tot;
          tot += x;
        }
        s_base = tot ? atomicAdd(a.rows_cnt, (unsigned long long)tot) : 0ull;
      }
      __syncthreads();
      unsigned long long pos = s_base + s_wsum[wv] + (incl - c0);
      while (pm) {
        const int r = __ffs(pm) - 1;
        pm &= pm - 1;
        const int j = threadIdx.x + r * kThreads;
        int32_t srck;
        int64_t rsk;
        locate(j, srck, rsk);
        if (a.out_vid) {
          const int64_t ge = rsk + e0 + j;
          a.out_vid[pos] = a.col_vid ? a.col_vid[ge] : a.vid_of[a.col[ge]];
        } else {
          a.rows_src[pos] = srck;
          a.rows_edge[pos] = rsk + e0 + j;
        }
        pos++;
      }
    }
    __syncthreads();
  }
}

// deg[i] = outdeg(F[i]); deg[nF] = 0
__global__ void k_degrees(const int32_t* F, int64_t nF, const int64_t* row_ptr, int64_t* deg) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i <= nF; i += int64_t(gridDim.x) * blockDim.x) {
    if (i == nF) {
      deg[i] = 0;
    } else {
      int32_t f = F[i];
      deg[i] = row_ptr[f + 1] - row_ptr[f];
    }
  }
}

// ------------------------------------------------------------------------------------------
// host drivers
// ------------------------------------------------------------------------------------------
// the programs' environment over csr: builds the column tables on first use
EvalEnv make_env(Ctx& c, EdgeSpace& es, Csr& csr, int32_t etype) {
  EvalEnv env{};
  env.nprops = int32_t(csr.props.size());
  auto upload = [](DevBuf& d, const std::vector<PropDev>& tab) {
    d.alloc(sizeof(PropDev) * tab.size());
    NBG_HIP(hipMemcpy(d.p, tab.data(), sizeof(PropDev) * tab.size(), hipMemcpyHostToDevice));
  };
  if (env.nprops && !csr.prop_table.p) {
    std::vector<PropDev> tab;
    append_prop_devs(tab, csr.props);
    upload(csr.prop_table, tab);
  }
  env.props = csr.prop_table.as<PropDev>();
  if (!c.tag_refs.empty() && !c.tag_table.p) {
    std::vector<PropDev> tab;
    for (auto& kv : c.tags) append_prop_devs(tab, kv.second.cols, kv.second.part.as<int32_t>());
    upload(c.tag_table, tab);
  }
  env.tprops = c.tag_table.as<PropDev>();
  env.etype = etype;
  env.vid_of = c.vid_of.as<int64_t>();
  env.col = csr.col.as<int32_t>();
  env.rank = csr.rank.as<int64_t>();
  return env;
}

// frontier degree scan: fills c.ws_off[0..nF] and returns total edges (synchronises)
// known >= 0: the caller already has the total (from a compaction's partials): no round trip
int64_t degree_scan(Ctx& c, const int32_t* F, int64_t nF, const Csr& csr, DevBuf& degbuf, int64_t known) {
  degbuf.ensure(size_t(nF + 1) * 8);
  k_degrees<<<grid_cap(nF + 1), 256, 0, c.stream>>>(F, nF, csr.row_ptr.as<int64_t>(), degbuf.as<int64_t>());
  exclusive_scan_dev<int64_t>(c, degbuf.as<int64_t>(), c.ws_off.as<int64_t>(), nF + 1);
  if (known >= 0) return known;
  int64_t E = 0;
  NBG_HIP(hipMemcpyAsync(&E, c.ws_off.as<int64_t>() + nF, 8, hipMemcpyDeviceToHost, c.stream));
  host_sync(c);
  return E;
}

template <int MODE>
void launch_expand(Ctx& c, ExpandArgs a, int pk, const FastArgs& fp, const Program* dprog, const EvalEnv& env,
                   int64_t E, bool tile_rows_ready) {
  int64_t ntiles = (E + kTile - 1) / kTile;
  int grid = int(std::max<int64_t>(1, std::min<int64_t>(ntiles, int64_t(256 * 8))));
  const size_t ia = timing_event(c);
  if (tile_rows_ready) {  // k_starts_small wrote the table
    a.tile_row = c.ws_tile_rows.as<int32_t>();
  } else if (a.nF < (int64_t(1) << 31)) {
    c.ws_tile_rows.ensure(size_t(ntiles + 2) * 4);
    a.tile_row = c.ws_tile_rows.as<int32_t>();
    k_tile_rows<kTile><<<grid_cap(a.nF), 256, 0, c.stream>>>(a.off, a.nF, c.ws_tile_rows.as<int32_t>());
  }
  switch (pk) {
    case PK_NONE: k_expand<MODE, PK_NONE><<<grid, kThreads, 0, c.stream>>>(a, fp, dprog, env); break;
    case PK_FAST: k_expand<MODE, PK_FAST><<<grid, kThreads, 0, c.stream>>>(a, fp, dprog, env); break;
    default: k_expand<MODE, PK_VM><<<grid, kThreads, 0, c.stream>>>(a, fp, dprog, env); break;
  }
  NBG_HIP(hipGetLastError());
  const size_t ib = timing_event(c);
  c.tpend.push_back(Ctx::PendingTime{ia, ib, c.timing.n_hops, 0});  // read by timing_resolve
  c.timing.expand_launches++;
}
// GO's two modes (traverse.hip); EXP_FLAGS is instantiated by expand_flags below
template void launch_expand<EXP_MARK>(Ctx&, ExpandArgs, int, const FastArgs&, const Program*, const EvalEnv&, int64_t, bool);
template void launch_expand<EXP_ROWS>(Ctx&, ExpandArgs, int, const FastArgs&, const Program*, const EvalEnv&, int64_t, bool);

void expand_flags(Ctx& c, ExpandArgs a, int pk, const FastArgs& fp, const Program* dprog, const EvalEnv& env, int64_t E) {
  launch_expand<EXP_FLAGS>(c, a, pk, fp, dprog, env, E);
}
// algorithmic bytes of one expansion (DESIGN.md "byte model"): frontier id 4 B + row_ptr pair
// 16 B + off 8 B per frontier entry; per edge: col 4 B (+ predicate column width) + the
// output it makes (1 B map mark, or 12 B row, or 1 B flag).
uint64_t expand_bytes(int64_t nF, int64_t E, int pred_width, int mode) {
  uint64_t b = uint64_t(nF) * 28 + uint64_t(E) * (4 + uint64_t(pred_width));
  b += uint64_t(E) * (mode == EXP_ROWS ? 0 : 1);
  return b;
}
// a PK_FAST predicate's typed compare on the CSR's own column (else: no arguments)
FastArgs fast_args(const Csr& csr, const FastPred& fpk) {
  if (fpk.kind != PK_FAST) return FastArgs{};
  const PropCol& pc = csr.props[size_t(fpk.col)];
  return FastArgs{pc.data.p, pc.present.as<uint8_t>(), pc.width, fpk.op, fpk.k};
}

}  // namespace nbg
