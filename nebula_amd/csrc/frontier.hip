// frontier.hip -- a GO query's frontier between its hops: the start kernels (starts -> list,
// bitmap or byte map), k_compact (byte map -> next frontier, replacing the unordered_set of
// GoExecutor::getDstIdsFromResp, GoExecutor.cpp:407-431), the exchanges of marks, bitmaps and roots
// between ranks with their collectives, the query workspaces, and the $- input index and root
// tables.  Every kernel sits behind the host function that launches it (go_launch.h).
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "device_common.h"
#include "engine.h"
#include "go_device.h"
#include "go_launch.h"
#include "query_common.h"

namespace nbg {

// Compact the owned slice [lo, lo+n) of the byte-map into a frontier list of local indices,
// clearing it.  require_deg: drop vertices without out-edges (they cannot produce rows).
// n_set counts every set byte (the reference's "starts_ non-empty" test, GoExecutor.cpp:392).
__global__ __launch_bounds__(256) void k_compact(uint8_t* map, int64_t lo, int64_t n, const int64_t* row_ptr,
                                                 const uint8_t* row_ok, int require_deg, int32_t* out,
                                                 unsigned long long* n_out, unsigned long long* partials,
                                                 uint16_t* bits, const uint32_t* __restrict__ odeg,
                                                 unsigned long long* sums = nullptr, int shards = 1,
                                                 int64_t own_lo = 0, int64_t own_hi = -1,
                                                 uint16_t* __restrict__ own_bits = nullptr, int64_t n_read = INT64_MAX) {
  // tile = 256 threads x 4 chunks of 16 bytes = 16384 vertices; one returning atomic per tile
  // (1024-thread tiles, a quarter of the atomics, measured slower: 40 -> 47 us at hop 1);
  // n_set (partials[0]), the kept out-degree sum (partials[1]) and the kept count (partials[2])
  // go to per-block partials.  out == nullptr: bitmap and counts only, no list (the list is built
  // from the bitmap later if a top-down hop needs it: the per-tile list atomics were most of
  // this kernel's time - 4096 tiles on one counter at RMAT-26).  own_lo < own_hi: the kept count
  // and out-degree sum of the vertices in [own_lo, own_hi) too (slots 3, 4: a rank's share of a
  // whole-space frontier, go_rep1; own_lo a multiple of 16), and own_bits (if set) gets that
  // range's bitmap.  n_read: past it the map is known to be zero (no dst of the hop's edge type
  // lies there: the class-ordered numbering puts the vertices without in-edges last), so those
  // chunks are not read and their bitmap words are written as zero
  __shared__ uint32_t lds[16];
  __shared__ unsigned long long lds64[kSlots * 16];
  __shared__ unsigned long long s_base;
  const int64_t nchunks = (n + 15) / 16;
  const int64_t rchunks = min(nchunks, (n_read + 15) / 16);  // chunks whose map bytes are read
  const int64_t tile = int64_t(blockDim.x) * 4;
  const int64_t ntiles = (nchunks + tile - 1) / tile;
  unsigned long long acc[5] = {0, 0, 0, 0, 0};
  const int nsum = own_lo < own_hi ? 5 : 3;
  // bitmap-only compaction (out == nullptr, the bottom-up path): the next tile's chunk loads are
  // issued with this one's (its map words stay in registers for the next round), so a block waits
  // one map latency per round of tiles, not one per tile
  const bool pre = out == nullptr;
  uint4 wn[4];
  if (pre) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int64_t ch = int64_t(blockIdx.x) * tile + q * int64_t(blockDim.x) + threadIdx.x;
      wn[q] = int64_t(blockIdx.x) < ntiles && ch < rchunks ? reinterpret_cast<const uint4*>(map + lo)[ch]
                                                            : make_uint4(0, 0, 0, 0);
    }
  }
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint32_t keep[4];
    uint32_t cnt = 0;
    // the tile's four chunk loads issued together (the clearing stores below would otherwise
    // order each load behind the previous chunk's store)
    uint4 wq[4];
    if (pre) {
      const int64_t tn = t + gridDim.x;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        wq[q] = wn[q];
        const int64_t ch = tn * tile + q * int64_t(blockDim.x) + threadIdx.x;
        wn[q] = tn < ntiles && ch < rchunks ? reinterpret_cast<const uint4*>(map + lo)[ch] : make_uint4(0, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t ch = t * tile + q * int64_t(blockDim.x) + threadIdx.x;
        wq[q] = ch < rchunks ? reinterpret_cast<const uint4*>(map + lo)[ch] : make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int64_t ch = t * tile + q * int64_t(blockDim.x) + threadIdx.x;
      const uint4 w = wq[q];
      const uint32_t words[4] = {w.x, w.y, w.z, w.w};
      uint32_t setmask = 0;
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
          if ((words[a] >> (8 * b)) & 0xff) setmask |= 1u << (a * 4 + b);
      uint32_t keepmask = setmask;
      const unsigned long long deg0 = acc[1];
      if (require_deg && setmask && odeg) {
        // out-degrees (0 where row_ok == 0) of the chunk's 16 vertices: four 16-byte loads issued
        // together, instead of a dependent row_ptr pair per set vertex (hub tiles are dense)
        uint32_t dg[16];
        if ((ch + 1) * 16 <= n) {
          const uint4* p4 = reinterpret_cast<const uint4*>(odeg + ch * 16);
#pragma unroll
          for (int a = 0; a < 4; a++) {
            const uint4 v4 = p4[a];
            dg[a * 4 + 0] = v4.x, dg[a * 4 + 1] = v4.y, dg[a * 4 + 2] = v4.z, dg[a * 4 + 3] = v4.w;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 16; j++) dg[j] = ch * 16 + j < n ? odeg[ch * 16 + j] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
          if (!((setmask >> j) & 1u)) continue;
          if (dg[j] == 0) keepmask &= ~(1u << j);
          else acc[1] += dg[j];
        }
      } else if (require_deg && setmask) {
        for (uint32_t m = setmask; m; m &= m - 1) {
          const int j = __ffs(m) - 1;
          const int64_t v = ch * 16 + j;
          const int64_t dg = row_ptr[v + 1] - row_ptr[v];
          if (dg == 0 || (row_ok && !row_ok[v])) keepmask &= ~(1u << j);
          else acc[1] += (unsigned long long)dg;
        }
      }
      if (bits && ch < nchunks) bits[ch] = uint16_t(keepmask);  // frontier bitmap for bottom-up
      if (setmask) reinterpret_cast<uint4*>(map + lo)[ch] = make_uint4(0, 0, 0, 0);
      acc[0] += __popc(setmask);
      if (ch * 16 + lo >= own_lo && ch * 16 + lo < own_hi) {
        acc[3] += __popc(keepmask), acc[4] += acc[1] - deg0;
        if (own_bits) own_bits[ch - (own_lo - lo) / 16] = uint16_t(keepmask);
      }
      keep[q] = keepmask;
      cnt += __popc(keepmask);
    }
    acc[2] += cnt;
    if (!out) continue;  // uniform: no block barrier is skipped by part of the block
    uint32_t total;
    const uint32_t pre = block_excl_scan_u32(cnt, total, lds);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(n_out, (unsigned long long)total) : 0ull;
    __syncthreads();
    unsigned long long p = s_base + pre;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int64_t ch = t * tile + q * int64_t(blockDim.x) + threadIdx.x;
      for (uint32_t m = keep[q]; m; m &= m - 1) out[p++] = int32_t(ch * 16 + (__ffs(m) - 1));
    }
    __syncthreads();
  }
  // sums (zeroed by the caller): the block sums added there, no k_reduce_partials launch
  if (sums) block_add_sums(acc, nsum, lds64, sums, shards);
  else block_store_partials(acc, nsum, lds64, partials);
}

// starts (gidx) -> deduplicated frontier: bitmap bits (set once, by a returning atomicOr) and
// list of the starts with out-edges; counts kCntList, kCntSet and kCntDegSum (the counters
// launch_compact leaves)
__global__ void k_starts_bits(const int32_t* g, int64_t n, int64_t lo, int64_t hi, const uint32_t* odeg,
                              uint32_t* bits, int32_t* out, unsigned long long* Kd) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  const int64_t rounds = (n + stride - 1) / stride;
  for (int64_t r = 0; r < rounds; r++) {
    const int64_t i = r * stride + blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    bool keep = false;
    int32_t loc = 0;
    uint32_t od = 0;
    if (i < n) {
      const int32_t x = g[i];
      if (x >= lo && x < hi) {
        loc = int32_t(x - lo);
        od = odeg[loc];
        const uint32_t bit = 1u << (loc & 31);
        keep = od && !(atomicOr(bits + (loc >> 5), bit) & bit);
      }
    }
    const int64_t s = wave_append(Kd + kCntList, keep);
    if (keep) {
      out[s] = loc;
      atomicAdd(Kd + kCntSet, 1ull);
      atomicAdd(Kd + kCntDegSum, (unsigned long long)od);
    }
  }
}

// starts (gidx) -> mark owned in the byte-map (dedup path) or list them (steps == 1 path)
// One-block start frontier for a few starts (ns <= kSmallStarts, one rank), everything the
// first top-down hop needs in one launch instead of a lookup, three memsets, the bitmap dedup, a
// degree pass, a scan and a counter round trip: zero the query counters Kd[0, 256), look the
// start vids up (gidx -> g), dedup through the start words of the frontier bitmap (only those
// words are cleared: a top-down first hop never reads the rest, k_compact rewrites it all), keep
// starts with out-edges (row_ok) as the list F, write its exclusive degree scan to off[0, ns]
// (entries past the list: degree 0, row 0) and the counts: kCntStartsN list length, kCntStartsE
// its out-degree sum, kCntHop1Rows the degree sum over every start with duplicates (hop-1 rows of
// a query without DISTINCT rescan duplicate starts, QueryBaseProcessor.inl:462-505).
// (kSmallStarts: go_launch.h)
__global__ __launch_bounds__(1024) void k_starts_small(const int64_t* __restrict__ vids, int32_t ns, const int64_t* keys,
                                                       const int32_t* vals, uint64_t mask, bool has_min,
                                                       int32_t min_gidx, int32_t* __restrict__ g, int64_t lo,
                                                       int64_t hi, const int64_t* __restrict__ row_ptr,
                                                       const uint8_t* __restrict__ row_ok, uint32_t* bits,
                                                       int32_t* __restrict__ F, int64_t* __restrict__ off,
                                                       unsigned long long* __restrict__ Kd,
                                                       int32_t* __restrict__ tile_row = nullptr) {
  __shared__ int32_t s_loc[kSmallStarts];
  __shared__ int64_t s_off[kSmallStarts];  // the kept starts' exclusive degree offsets
  __shared__ unsigned long long s_w[32];  // [0, 16): per-wave counts, [16, 32): per-wave degree sums
  __shared__ unsigned long long s_carry[2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < int(kShardStride) * kSumShards; i += blockDim.x) Kd[i] = 0ull;  // every shard
  for (int i = tid; i < ns; i += blockDim.x) {
    const int32_t x = ht_lookup(keys, vals, mask, vids[i], has_min, min_gidx);
    g[i] = x;
    int32_t loc = -1;
    if (x >= lo && x < hi && (row_ok == nullptr || row_ok[x - lo]) && row_ptr[x - lo + 1] > row_ptr[x - lo])
      loc = int32_t(x - lo);
    s_loc[i] = loc;
    if (loc >= 0) bits[loc >> 5] = 0u;
  }
  if (tid < 2) s_carry[tid] = 0ull;
  __syncthreads();
  unsigned long long scanned = 0;  // every start's degree, duplicates included
  for (int i0 = 0; i0 < ns; i0 += blockDim.x) {
    const int i = i0 + tid;
    const int32_t loc = i < ns ? s_loc[i] : -1;
    const unsigned long long d = loc >= 0 ? (unsigned long long)(row_ptr[loc + 1] - row_ptr[loc]) : 0ull;
    scanned += d;
    bool keep = false;
    if (loc >= 0) {
      const uint32_t bit = 1u << (loc & 31);
      keep = !(atomicOr(bits + (loc >> 5), bit) & bit);
    }
    // block prefix of (kept count, kept degree): wave inclusive scans, then the wave totals
    unsigned long long kc = keep ? 1ull : 0ull, kd = keep ? d : 0ull;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long a = __shfl_up(kc, o), b = __shfl_up(kd, o);
      if (lane >= o) kc += a, kd += b;
    }
    if (lane == 63) s_w[wv] = kc, s_w[16 + wv] = kd;
    __syncthreads();
    unsigned long long bc = s_carry[0], bd = s_carry[1], tc = 0, td = 0;
    for (int w = 0; w < int(blockDim.x >> 6); w++) {
      const unsigned long long wc = s_w[w], wd = s_w[16 + w];
      if (w < wv) bc += wc, bd += wd;
      tc += wc, td += wd;
    }
    if (keep) {
      const unsigned long long pos = bc + kc - 1;
      F[pos] = loc;
      off[pos] = int64_t(bd + kd - d);
      s_off[pos] = int64_t(bd + kd - d);
    }
    __syncthreads();
    if (tid == 0) s_carry[0] += tc, s_carry[1] += td;
    __syncthreads();
  }
  const unsigned long long nF = s_carry[0], E = s_carry[1];
  for (int i = int(nF) + tid; i <= ns; i += blockDim.x) {
    if (i < ns) F[i] = 0;
    off[i] = int64_t(E);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) scanned += __shfl_xor(scanned, o);
  if (lane == 0) s_w[wv] = scanned;
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < int(blockDim.x >> 6); w++) t += s_w[w];
    Kd[kCntStartsN] = nF;
    Kd[kCntStartsE] = E;
    Kd[kCntHop1Rows] = t;
  }
  // the hop-1 expansion's tile-row table (k_tile_rows' rule) from the offsets just written: one
  // launch and its gap less before the first hop.  Tile t's row is the last kept start whose
  // range begins at or before t * kTile (every kept start has out-edges, so the ranges tile
  // [0, E)): one thread per tile, a binary search of the offsets in LDS (a thread per start
  // walked a hub seed's hundreds of tiles alone)
  if (tile_row && nF > 0) {
    const int64_t nT = (int64_t(E) + kTile - 1) / kTile;
    for (int64_t t = tid; t < nT; t += blockDim.x) {
      const int64_t e0 = t * kTile;
      int k = 0;
      for (int st = kSmallStarts / 2; st > 0; st >>= 1)
        if (k + st < int(nF) && s_off[k + st] <= e0) k += st;
      tile_row[t] = k;
    }
  }
}

__global__ void k_mark_gidx(const int32_t* g, int64_t n, int64_t lo, int64_t hi, uint8_t* map) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int32_t x = g[i];
    if (x >= lo && x < hi) map[x] = 1;
  }
}
__global__ void k_list_starts(const int32_t* g, int64_t n, int64_t lo, int64_t hi, const int64_t* row_ptr,
                              const uint8_t* row_ok, int32_t* out, unsigned long long* n_out) {
  // order-preserving is not required (multiset results); wave-aggregated append
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  int64_t rounds = (n + stride - 1) / stride;
  for (int64_t r = 0; r < rounds; r++) {
    int64_t i = r * stride + blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    bool keep = false;
    int32_t loc = 0;
    if (i < n) {
      int32_t x = g[i];
      if (x >= lo && x < hi) {
        loc = int32_t(x - lo);
        keep = row_ptr[loc + 1] > row_ptr[loc] && (row_ok == nullptr || row_ok[loc]);
      }
    }
    int64_t s = wave_append(n_out, keep);
    if (keep) out[s] = loc;
  }
}
// rows the hop-1 scans return for a start list WITH its duplicates: each duplicate start rescans
// its prefix (GoExecutor.cpp:98-104 dedups the starts only under DISTINCT), so the edges scanned
// (the TEPS numerator, and what the reference's storage returns) count them, while the device
// expands the deduplicated frontier (P12 makes the next frontier a set either way)
__global__ void k_starts_degree(const int32_t* g, int64_t n, int64_t lo, int64_t hi, const int64_t* row_ptr,
                                const uint8_t* row_ok, unsigned long long* sum) {
  unsigned long long acc = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t x = g[i];
    if (x >= lo && x < hi && (row_ok == nullptr || row_ok[x - lo])) acc += (unsigned long long)(row_ptr[x - lo + 1] - row_ptr[x - lo]);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);
}

// ---- multi-rank frontier exchange ----------------------------------------------------------
// global byte-map -> 32-bit mark words (one word per thread), clearing the map
__global__ void k_map_to_bits(uint8_t* map, int64_t n, uint32_t* bits) {
  const int64_t nw = (n + 31) / 32;
  for (int64_t w = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; w < nw; w += int64_t(gridDim.x) * blockDim.x) {
    uint4* p = reinterpret_cast<uint4*>(map + w * 32);
    uint4 a = p[0], b = p[1];
    const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        if ((x[i] >> (8 * k)) & 0xff) m |= 1u << (i * 4 + k);
    bits[w] = m;
    if (m) {
      p[0] = make_uint4(0, 0, 0, 0);
      p[1] = make_uint4(0, 0, 0, 0);
    }
  }
}
// OR the [G][nw] received mark words and set the owned slice of the byte-map
__global__ void k_or_segments_to_map(const uint32_t* recv, int G, int64_t nw, uint8_t* map_lo) {
  for (int64_t w = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; w < nw; w += int64_t(gridDim.x) * blockDim.x) {
    uint32_t m = 0;
    for (int p = 0; p < G; p++) m |= recv[size_t(p) * size_t(nw) + size_t(w)];
    for (; m; m &= m - 1) map_lo[w * 32 + (__ffs(m) - 1)] = 1;
  }
}
// several ranks, a top-down hop whose next frontier goes on as a bitmap (bottom-up hops): OR the
// [G][nw] received mark words straight into the owned frontier bitmap, dropping vertices without
// out-edges, with the compaction's counts -- sums[0] vertices set, [1] kept out-degree sum,
// [2] kept vertices (k_compact's [kCntSet, kCntKept]) -- instead of writing the marks into the byte map
// and compacting it again (k_or_segments_to_map + k_compact: 6 + 29 us at RMAT-26, r12h)
__global__ __launch_bounds__(256) void k_or_segments_bits(const uint32_t* __restrict__ recv, int G, int64_t nw,
                                                          const uint32_t* __restrict__ odeg, uint32_t* bits,
                                                          unsigned long long* sums) {
  __shared__ unsigned long long lds[kSlots * 16];
  unsigned long long acc[3] = {0, 0, 0};
  for (int64_t w = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; w < nw; w += int64_t(gridDim.x) * blockDim.x) {
    uint32_t m = 0;
    for (int p = 0; p < G; p++) m |= recv[size_t(p) * size_t(nw) + size_t(w)];
    uint32_t keep = m;
    if (m) {
      // the word's 32 out-degrees as eight 16-byte loads issued together (odeg is padded to whole
      // 128-row tiles), not one dependent load per set bit (24 us at RMAT-26 one rank, r12i)
      uint32_t dg[32];
      const uint4* p4 = reinterpret_cast<const uint4*>(odeg + w * 32);
#pragma unroll
      for (int a = 0; a < 8; a++) {
        const uint4 v = p4[a];
        dg[4 * a] = v.x, dg[4 * a + 1] = v.y, dg[4 * a + 2] = v.z, dg[4 * a + 3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < 32; j++) {
        const uint32_t d = (m >> j) & 1u ? dg[j] : 0u;
        if ((m >> j) & 1u && d == 0) keep &= ~(1u << j);
        acc[1] += d;
      }
    }
    bits[w] = keep;
    acc[0] += __popc(m);
    acc[2] += __popc(keep);
  }
  block_add_sums(acc, 3, lds, sums);
}

// input table index: gidx of starts[i] -> i, the LAST row of a vid winning
// (InterimResult::buildIndex overwrites vidToRowIndex_ row by row, InterimResult.cpp:158-160)
__global__ void k_input_index(const int32_t* sg, int64_t n, int32_t* keys, int32_t* rows, uint32_t mask) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t g = sg[i];
    if (g < 0) continue;
    uint32_t h = gidx_hash(g) & mask;
    while (true) {
      const int32_t prev = atomicCAS(keys + h, -1, g);
      if (prev == -1 || prev == g) {
        atomicMax(rows + h, int32_t(i));
        break;
      }
      h = (h + 1) & mask;
    }
  }
}

// roots of the starts: rank of the start's vid among the distinct start vids (host-computed),
// so a min over ranks is the min over root vids; tab[rank] = the start's gidx
__global__ void k_root_init(const int32_t* sg, const int32_t* srank, int64_t n, int32_t* root, int32_t* tab) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t g = sg[i];
    if (g < 0) continue;
    root[g] = srank[i];
    tab[srank[i]] = g;
  }
}

// ------------------------------------------------------------------------------------------
// host drivers
// ------------------------------------------------------------------------------------------
void launch_starts_small(Ctx& c, const int64_t* vids, int64_t ns, int32_t* sg, int64_t lo, int64_t hi, const Csr& csr,
                         uint32_t* bits, int32_t* F, unsigned long long* Kd) {
  k_starts_small<<<1, 1024, 0, c.stream>>>(vids, int32_t(ns), c.ht_keys.as<int64_t>(), c.ht_vals.as<int32_t>(),
                                           uint64_t(c.ht_cap - 1), c.ht_has_min, c.ht_min_gidx, sg, lo, hi,
                                           csr.row_ptr.as<int64_t>(), csr.row_ok.as<uint8_t>(), bits, F,
                                           c.ws_off.as<int64_t>(), Kd, c.ws_tile_rows.as<int32_t>());
}
void launch_list_starts(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, const int64_t* row_ptr,
                        const uint8_t* row_ok, int32_t* F, unsigned long long* n_out) {
  k_list_starts<<<grid_cap(ns), 256, 0, c.stream>>>(sg, ns, lo, hi, row_ptr, row_ok, F, n_out);
}
void launch_starts_bits(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, const uint32_t* odeg,
                        uint32_t* bits, int32_t* F, unsigned long long* Kd) {
  k_starts_bits<<<grid_cap(ns), 256, 0, c.stream>>>(sg, ns, lo, hi, odeg, bits, F, Kd);
}
void launch_mark_gidx(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, uint8_t* map) {
  k_mark_gidx<<<grid_cap(ns), 256, 0, c.stream>>>(sg, ns, lo, hi, map);
}
void launch_starts_degree(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, const int64_t* row_ptr,
                          const uint8_t* row_ok, unsigned long long* sum) {
  k_starts_degree<<<grid_cap(ns), 256, 0, c.stream>>>(sg, ns, lo, hi, row_ptr, row_ok, sum);
}
void launch_input_index(Ctx& c, const int32_t* sg, int64_t ns, int32_t* keys, int32_t* rows, uint32_t mask) {
  k_input_index<<<grid_cap(ns), 256, 0, c.stream>>>(sg, ns, keys, rows, mask);
}
void launch_root_init(Ctx& c, const int32_t* sg, const int32_t* srank, int64_t ns, int32_t* root, int32_t* tab) {
  k_root_init<<<grid_cap(ns), 256, 0, c.stream>>>(sg, srank, ns, root, tab);
}

int64_t map_bytes(const Ctx& c) { return ((c.n_global + 63) / 64) * 64 + 64; }

void ensure_workspaces(Ctx& c, int64_t nF_cap) {
  int64_t mb = map_bytes(c);
  if (c.ws_map.bytes < size_t(mb)) {
    c.ws_map.alloc(size_t(mb));
    NBG_HIP(hipMemsetAsync(c.ws_map.p, 0, size_t(mb), c.stream));
  }
  c.ws_front[0].ensure(size_t(nF_cap + 64) * 4);
  c.ws_front[1].ensure(size_t(nF_cap + 64) * 4);
  c.ws_off.ensure(size_t(nF_cap + 2) * 8);
  c.ws_counters.ensure(kShardStride * kSumShards * 8);  // layout: CounterWord / SpecWord
  c.ws_partials.ensure(size_t(kAggBlocks) * kSlots * 8);
  c.ws_bits_send.ensure(size_t(mb / 8 + 64));
  c.ws_bits_recv.ensure(size_t(mb / 8 + 64));
  if (c.sharded) {
    c.ws_piggy.ensure(size_t(kMaxSpec) * size_t(c.world) * 16 + 64);  // spec hops' (n, e) of every rank
    c.ws_bits_glob.ensure(size_t(mb / 8 + 64));
    c.ws_bits_xchg.ensure(size_t(c.world) * size_t((c.owned_hi() - c.owned_lo()) / 8) + 64);
  }
}

// element-wise sum of a few host counters over ranks
void allsum(Ctx& c, int64_t* v, int n, unsigned long long* dscratch) {
  if (!c.sharded) return;
  {
    CommTimer t(c);
    NBG_HIP(hipMemcpyAsync(dscratch, v, size_t(n) * 8, hipMemcpyHostToDevice, c.stream));
    comm_allreduce_sum_i64(c, reinterpret_cast<int64_t*>(dscratch), size_t(n));
    NBG_HIP(hipMemcpyAsync(v, dscratch, size_t(n) * 8, hipMemcpyDeviceToHost, c.stream));
  }
  host_sync(c);
}

// device counters summed over ranks into dst (stream-ordered: a gate kernel reads the sums)
// srcs: up to 8 counter indices of K.d; dst: n consecutive words
namespace {
__global__ void k_pick_counters(const unsigned long long* K, uint64_t idx, int n, unsigned long long* dst) {
  if (threadIdx.x < unsigned(n))
    dst[threadIdx.x] = __hip_atomic_load(K + ((idx >> (8 * threadIdx.x)) & 0xffu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace
void dev_allsum(Ctx& c, const unsigned long long* K, std::initializer_list<int> idx, unsigned long long* dst) {
  uint64_t packed = 0;
  int n = 0;
  for (int i : idx) packed |= uint64_t(uint8_t(i)) << (8 * n++);
  k_pick_counters<<<1, 64, 0, c.stream>>>(K, packed, n, dst);
  NBG_HIP(hipGetLastError());
  if (!c.sharded) return;
  CommTimer t(c);
  comm_allreduce_sum_i64(c, reinterpret_cast<int64_t*>(dst), size_t(n));
}

// owned frontier bitmap -> bitmap over the whole gidx space (bottom-up hops read sources of
// every rank).  Owner ranges are padded to 64, so every segment is whole 64-bit words.
const uint32_t* global_bits(Ctx& c, const uint32_t* owned) {
  if (!c.sharded) return owned;
  CommTimer t(c);
  const size_t G = size_t(c.world);
  std::vector<size_t> rb(G), ro(G);
  for (size_t p = 0; p < G; p++) {
    rb[p] = size_t(c.base[p + 1] - c.base[p]) / 8;
    ro[p] = size_t(c.base[p]) / 8;
  }
  comm_allgatherv_bytes(c, owned, rb[size_t(c.rank)], c.ws_bits_glob.p, rb.data(), ro.data());
  c.timing.comm_bytes += uint64_t(rb[size_t(c.rank)]) * (G - 1);
  return c.ws_bits_glob.as<uint32_t>();
}

// global_bits + every rank's two counters (n, e) at cnt into all[2r, 2r + 2), one exchange
const uint32_t* global_bits_cnt(Ctx& c, const uint32_t* owned, const unsigned long long* cnt, unsigned long long* all) {
  CommTimer t(c);
  const size_t G = size_t(c.world);
  std::vector<size_t> rb(G), ro(G);
  for (size_t p = 0; p < G; p++) {
    rb[p] = size_t(c.base[p + 1] - c.base[p]) / 8;
    ro[p] = size_t(c.base[p]) / 8;
  }
  comm_allgatherv2_bytes(c, owned, rb[size_t(c.rank)], c.ws_bits_glob.p, rb.data(), ro.data(), cnt, 16, all);
  c.timing.comm_bytes += uint64_t(rb[size_t(c.rank)] + 16) * (G - 1);
  return c.ws_bits_glob.as<uint32_t>();
}

// top-down hops mark dsts of every rank in the global byte-map: ship each owner its slice as
// a bitmap and OR the received slices back into the owned range of the map
void exchange_marks(Ctx& c, uint8_t* map, uint32_t* owned_bits, const uint32_t* odeg, unsigned long long* sums) {
  if (!c.sharded) return;
  CommTimer t(c);
  const size_t G = size_t(c.world);
  const int64_t lo = c.owned_lo(), n_own = c.owned_hi() - lo;
  uint32_t* sb = c.ws_bits_glob.as<uint32_t>();
  uint32_t* rbuf = c.ws_bits_xchg.as<uint32_t>();
  int64_t nw = c.n_global / 32;
  k_map_to_bits<<<grid_cap(nw), 256, 0, c.stream>>>(map, c.n_global, sb);
  NBG_HIP(hipGetLastError());
  std::vector<size_t> sbytes(G), soff(G), rbytes(G), roff(G);
  for (size_t p = 0; p < G; p++) {
    sbytes[p] = size_t(c.base[p + 1] - c.base[p]) / 8;
    soff[p] = size_t(c.base[p]) / 8;
    rbytes[p] = size_t(n_own) / 8;
    roff[p] = p * size_t(n_own) / 8;
  }
  comm_alltoallv_bytes(c, sb, sbytes.data(), soff.data(), rbuf, rbytes.data(), roff.data());
  c.timing.comm_bytes += uint64_t(c.n_global - n_own) / 8;
  if (owned_bits) {  // the next frontier as the owned bitmap + its counts (no byte map, no compaction)
    const int grid = int(std::max<int64_t>(1, std::min<int64_t>((n_own / 32 + 255) / 256, 512)));
    k_or_segments_bits<<<grid, 256, 0, c.stream>>>(rbuf, int(G), n_own / 32, odeg, owned_bits, sums);
  } else {
    k_or_segments_to_map<<<grid_cap(n_own / 32), 256, 0, c.stream>>>(rbuf, int(G), n_own / 32, map + lo);
  }
  NBG_HIP(hipGetLastError());
}

namespace {
__global__ void k_min_segments(const int32_t* recv, int G, int64_t n, int32_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int32_t m = INT32_MAX;
    for (int g = 0; g < G; g++) m = min(m, recv[size_t(g) * size_t(n) + size_t(i)]);
    out[i] = m;
  }
}
}  // namespace

// world > 1, $- / $var props with STEPS > 1: every rank's top-down hop took the smallest root
// rank over ITS in-edges of each dst (one atomicMin per edge, any owner); the owner of a dst
// needs the minimum over all ranks' edges (GoExecutor.h:174-193's VertexBackTracker, under the
// deterministic rule of DESIGN.md divergence 6).  Each rank sends every owner its slice of the
// root array and takes the elementwise minimum of the slices it receives.
void exchange_roots(Ctx& c, int32_t* root_next) {
  if (!c.sharded) return;
  CommTimer t(c);
  const size_t G = size_t(c.world);
  const int64_t lo = c.owned_lo(), n_own = c.owned_hi() - lo;
  DevBuf rbuf;
  rbuf.alloc(std::max<size_t>(G * size_t(n_own) * 4, 4));
  std::vector<size_t> sbytes(G), soff(G), rbytes(G), roff(G);
  for (size_t p = 0; p < G; p++) {
    sbytes[p] = size_t(c.base[p + 1] - c.base[p]) * 4;
    soff[p] = size_t(c.base[p]) * 4;
    rbytes[p] = size_t(n_own) * 4;
    roff[p] = p * size_t(n_own) * 4;
  }
  comm_alltoallv_bytes(c, root_next, sbytes.data(), soff.data(), rbuf.p, rbytes.data(), roff.data());
  c.timing.comm_bytes += uint64_t(c.n_global - n_own) * 4;
  if (n_own)
    k_min_segments<<<grid_cap(n_own), 256, 0, c.stream>>>(rbuf.as<int32_t>(), int(G), n_own, root_next + lo);
  NBG_HIP(hipGetLastError());
}

void launch_compact(Ctx& c, uint8_t* map, int64_t lo, int64_t n, const int64_t* row_ptr, const uint8_t* row_ok,
                    int require_deg, int32_t* out, uint16_t* bits, unsigned long long* Kd,
                    const uint32_t* odeg, bool sums_zero, int shards, int64_t own_lo, int64_t own_hi,
                    uint16_t* own_bits, int64_t n_read) {
  // counters (CounterWord): kCntList the list length (atomic) and the sums kCntSet, kCntDegSum,
  // kCntKept (with own_lo / own_hi also kCntOwnKept, kCntOwnDegSum).
  // sums_zero: the sums' words are already zero, so the blocks add into them (bu_atomic_sums)
  unsigned long long* partials = c.ws_partials.as<unsigned long long>();
  int64_t ntiles = ((n + 15) / 16 + 1023) / 1024;
  int grid = int(std::max<int64_t>(1, std::min<int64_t>(ntiles, std::min<int64_t>(kAggBlocks, c.opt("compact_grid", 1024)))));
  const bool atomic = sums_zero && c.opt("bu_atomic_sums", 1) != 0;
  k_compact<<<grid, 256, 0, c.stream>>>(map, lo, n, row_ptr, row_ok, require_deg, out, Kd, partials, bits, odeg,
                                        atomic ? Kd + kCntSet : nullptr, atomic ? shards : 1, own_lo, own_hi, own_bits,
                                        n_read >= 0 ? n_read : n);
  if (!atomic) reduce_partials(c, partials, grid, Kd + kCntSet);
  NBG_HIP(hipGetLastError());
}

}  // namespace nbg
