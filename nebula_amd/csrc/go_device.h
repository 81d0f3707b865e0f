// go_device.h -- what the GO kernels of expand.hip, bottom_up.hip, frontier.hip and go_variants.hip
// share on the device: the expansion's tile, the block-sum helpers, the layout of a query's
// counter block and the gate of a speculated hop.  Inline and constexpr only.
#pragma once
#include "device_common.h"
#include "engine.h"
#include "qpred.h"

namespace nbg {

// the top-down expansion's tile: kTile consecutive edges of the flattened frontier per workgroup
constexpr int kThreads = 256;
constexpr int kItems = 8;
constexpr int kTile = kThreads * kItems;

// Quantised predicate on packed bottom-up words: QArgs / q_test (qpred.h).
// The kernels' copy of QArgs in scalar registers.  Read through the by-value kernel argument,
// q_test's select between `below` and `above` compiled to a per-lane select of two kernarg
// addresses and a vector load, i.e. one dependent load and a vmcnt(0) wait per slot word.
__device__ inline QArgs q_sgpr(const QArgs& a) {
  QArgs r;
  r.gmask = __builtin_amdgcn_readfirstlane(a.gmask);
  r.gbits = __builtin_amdgcn_readfirstlane(a.gbits);
  r.ulo = __builtin_amdgcn_readfirstlane(a.ulo);
  r.uhi = __builtin_amdgcn_readfirstlane(a.uhi);
  r.below = __builtin_amdgcn_readfirstlane(a.below);
  r.above = __builtin_amdgcn_readfirstlane(a.above);
  return r;
}
__device__ inline int32_t q_gidx(int32_t s, const QArgs& q) { return s & int32_t(q.gmask); }

// wave-wide exclusive prefix sum of a per-lane count
__device__ inline uint32_t wave_excl_scan(uint32_t x, uint32_t& total) {
  const int lane = threadIdx.x & 63;
  uint32_t v = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t y = __shfl_up(v, o);
    if (lane >= o) v += y;
  }
  total = __shfl(v, 63);
  return v - x;
}

// ---- block-level aggregation helpers (one atomic per block or none: a single global counter
// serialises at ~88 returning atomics/us on MI355X, MI355X_MICROARCH "dequeue") ----------------
constexpr int kAggBlocks = 8192;  // max grid of the aggregated kernels (partials are [block][kSlots])
constexpr int kSlots = 8;
constexpr int kRestMax = 2;  // bu_rest_scan: max 64- / 16-entry chunks of a rest loaded per step

__device__ inline uint32_t block_excl_scan_u32(uint32_t x, uint32_t& total, uint32_t* lds) {
  uint32_t wt;
  uint32_t pre = wave_excl_scan(x, wt);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[w] = wt;
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int i = 0; i < int(blockDim.x >> 6); i++) {
    if (i < w) off += lds[i];
    tot += lds[i];
  }
  __syncthreads();
  total = tot;
  return pre + off;
}
__device__ inline void block_store_partials(const unsigned long long* v, int k, unsigned long long* lds,
                                            unsigned long long* partials) {
  const int w = threadIdx.x >> 6;
  const int nw = int(blockDim.x >> 6);
  for (int i = 0; i < k; i++) {
    unsigned long long s = wave_sum_u64(v[i]);
    if ((threadIdx.x & 63) == 0) lds[i * 16 + w] = s;
  }
  __syncthreads();
  if (threadIdx.x < unsigned(kSlots)) {
    unsigned long long s = 0;
    if (threadIdx.x < unsigned(k))
      for (int j = 0; j < nw; j++) s += lds[threadIdx.x * 16 + j];
    partials[size_t(threadIdx.x) * kAggBlocks + blockIdx.x] = s;  // slot-major: coalesced reduce
  }
}
// ---- a GO query's counter block --------------------------------------------------------------
// Ctx::ws_counters (device, "Kd" in the kernels) and its pinned host mirror Ctx::host_counters
// (Counters::d / ::h): 256 words of 8 B, then shards 1 .. kSumShards - 1 of every word
// (block_add_sums), kShardStride words apart.  Words [0, kSpecBase) are the hop counters below,
// reused from hop to hop; [kSpecBase, 256) the speculated hops' blocks (SpecWord).
// the eight counters a bottom-up hop's two passes reduce into their `out` block
enum HopWord : int {
  kHopFound = 0,      // rows found (bits set in the next frontier)
  kHopDegSum = 1,     // ... their out-degree sum (non-final hops)
  kHopSlabWords = 2,  // slab words the first pass read
  kHopPending = 3,    // rows left pending for the rest pass
  kHopEntries = 4,    // adjacency entries the rest pass read
  kHopValues = 5,     // predicate values the rest pass read ([6] / [7]: probe statistics)
  kHopWords = 8,
};
enum CounterWord : int {
  // a list length, counted by atomics: the frontier list (k_list_starts, k_starts_bits, k_compact,
  // k_bits_compact<0>) or the DISTINCT _dst output of a host-chosen final bottom-up hop.  A
  // host-chosen non-final bottom-up hop reduces its HopWord block into [kCntList, kHopWords).
  kCntList = 0,
  kCntRows = 2,       // rows the final expansion kept (EXP_ROWS)
  kCntWhereErr = 4,   // WHERE evaluation errors (ExpandArgs::err)
  kCntYieldErr = 5,   // YIELD evaluation errors (k_materialize)
  kCntFinalHop = 8,   // [8, 16): the HopWord block of a host-chosen final bottom-up hop
  // a compaction's sums (k_compact, k_starts_bits, k_or_segments_bits), sharded when the
  // compaction runs with shards > 1:
  kCntSet = 12,     // vertices set in the byte map (found)
  kCntDegSum = 13,  // out-degree sum of the kept vertices (the next hop's E)
  kCntKept = 14,    // kept vertices (= the list length, also when no list is written)
  // go_rep1: this rank's share of the whole-space compaction (k_compact's own_lo / own_hi)
  kCntOwnKept = 15,
  kCntOwnDegSum = 16,
  kCntRed = 24,       // scratch of the cross-rank sums made through the host (allsum)
  kCntHop1Rows = 30,  // degree sum over every start, duplicates included (k_starts_degree, k_starts_small)
  kCntStartWords = 32,  // the words a fetch behind the start kernels reads: [0, kCntHop1Rows]
  kCntStartsN = 40,   // k_starts_small: the start list's length
  kCntStartsE = 41,   // ... and its out-degree sum
  kCntGlobal = 48,    // [48, 52): counters summed over ranks on the device (dev_allsum's output)
  kCntUpto = 56,      // [56, 60): the sums of a GO UPTO hop (k_upto_claim / k_upto_bu)
  kSpecBase = 64,     // the first speculated hop's block
};
// a speculated hop's block: kSpecWords words at kSpecBase + kSpecWords * (position in the chain)
enum SpecWord : int {
  // [0, kHopWords): the hop's HopWord block
  kSpecGate = 8,   // its gate (gate_open): 1 the hop ran, 0 it did nothing
  kSpecRows = 9,   // the DISTINCT _dst output count (a speculated final hop)
  kSpecSumN = 10,  // several ranks: found / next out-degree sum over ranks of the hop before --
  kSpecSumE = 11,  // ... published by this hop's gate (piggy) -- or of this hop (dev_allsum)
  kSpecLastN = 12,  // (piggy) a chain ending on a non-final hop: that hop's sums over ranks
  kSpecLastE = 13,
  kSpecWords = 16,
};
constexpr int kMaxSpec = (256 - kSpecBase) / kSpecWords;  // hops a chain can hold (12)

// the block's sums straight into out[0, k) with no-return atomics (option bu_atomic_sums: the
// bottom-up passes then need no k_reduce_partials launch; out starts at zero).
// shards > 1: block b adds into shard b % shards, kShardStride words further per shard, and every
// reader folds the shards (gate_open, k_publish): the adds of one address serialise at the memory
// side (~10 ns each), so 512 blocks ending together added ~4 us to a kernel and 1024 ~10 us
// (tools/atomic_tail, profiles/r12c_atomic_tail.jsonl); with 8 shards ~0.
__device__ inline void block_add_sums(const unsigned long long* v, int k, unsigned long long* lds,
                                      unsigned long long* out, int shards = 1) {
  if (shards > 1) out += size_t(blockIdx.x % unsigned(shards)) * kShardStride;
  const int w = threadIdx.x >> 6;
  const int nw = int(blockDim.x >> 6);
  for (int i = 0; i < k; i++) {
    unsigned long long s = wave_sum_u64(v[i]);
    if ((threadIdx.x & 63) == 0) lds[i * 16 + w] = s;
  }
  __syncthreads();
  if (threadIdx.x < unsigned(k)) {
    unsigned long long s = 0;
    for (int j = 0; j < nw; j++) s += lds[threadIdx.x * 16 + j];
    if (s) __hip_atomic_fetch_add(out + threadIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Speculative hops (go_run): the first pass of a gated hop evaluates the host's direction rule
// itself on the previous hop's device counters -- open iff the previous hop ran (pg), its next
// frontier is non-empty (*n > 0) and its out-degree sum reaches the threshold (*e >= thr) -- and
// block 0 publishes the answer at `gate` for the hop's later kernels and the host (a separate
// one-thread k_gate launch cost ~4.6 us a hop).  e == nullptr: not gated.
// Several ranks (all != nullptr): the previous hop's (n, e) of every rank arrived with this
// hop's frontier allgather (all[2r], all[2r + 1]); the gate sums them and block 0 also publishes
// the sums at its block's kSpecSumN, kSpecSumE (the host's global counts of the previous hop;
// `gate` is the block's kSpecGate word).
struct GateIn {
  const unsigned long long* e = nullptr;
  const unsigned long long* n = nullptr;
  const unsigned long long* pg = nullptr;
  unsigned long long thr = 0;
  const unsigned long long* all = nullptr;
  int world = 1;
  int shards = 1;  // e / n are sharded block sums (block_add_sums): their shards are summed
};
__device__ inline bool gate_open(const GateIn& gi, unsigned long long* gate) {
  // (plain loads: agent-scope ones at every block's start cost the C3 query 0.405 -> 0.415 ms)
  if (gi.e == nullptr && gi.all == nullptr) return gate == nullptr || *gate != 0ull;
  unsigned long long n, e;
  if (gi.all) {
    n = e = 0ull;
    for (int r = 0; r < gi.world; r++) n += gi.all[2 * r], e += gi.all[2 * r + 1];
  } else {
    n = e = 0ull;
    for (int s = 0; s < gi.shards; s++) n += gi.n[size_t(s) * kShardStride], e += gi.e[size_t(s) * kShardStride];
  }
  const bool open = (gi.pg == nullptr || *gi.pg != 0ull) && n > 0ull && e >= gi.thr;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    __hip_atomic_store(gate, open ? 1ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gi.all) {
      __hip_atomic_store(gate + (kSpecSumN - kSpecGate), n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(gate + (kSpecSumE - kSpecGate), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  return open;
}

}  // namespace nbg
