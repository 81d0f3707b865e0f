// bottom_up.hip -- the bottom-up hop of a GO query (direction-optimising BFS) on MI355X (gfx950):
// the first pass over the quad slab (k_bu_lean, or k_bu_fin on the final hop), the rest pass over
// the rows it left pending (k_bu_rest_lean), the reduction of block partials (k_reduce_partials)
// and the compaction of a frontier bitmap to a row list or to the DISTINCT _dst vids
// (k_bits_compact).  launch_bu_lean plans a hop's shape once and launches the two passes; each
// pass picks its instantiation and the name it reports from one table.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "device_common.h"
#include "engine.h"
#include "expr_device.h"
#include "go_device.h"
#include "go_launch.h"
#include "qpred.h"
#include "query_common.h"

namespace nbg {

// sums the [kSlots][kAggBlocks] partials into out[0..kSlots) (one block of 1024 threads; all
// kSlots loads of an iteration are independent, so the block has 8 loads in flight per lane
// instead of one dependent chain per slot)
// gate (speculative hops, go_run): when *gate == 0 the kernel does nothing
__global__ __launch_bounds__(1024) void k_reduce_partials(const unsigned long long* partials, int nblocks,
                                                          unsigned long long* out,
                                                          const unsigned long long* gate = nullptr) {
  if (gate && *gate == 0ull) return;
  __shared__ unsigned long long s[kSlots][16];
  unsigned long long a[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; k++) a[k] = 0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
#pragma unroll
    for (int k = 0; k < kSlots; k++) a[k] += partials[size_t(k) * kAggBlocks + b];
  }
  const int w = threadIdx.x >> 6, nw = int(blockDim.x >> 6);
#pragma unroll
  for (int k = 0; k < kSlots; k++) {
    unsigned long long v = wave_sum_u64(a[k]);
    if ((threadIdx.x & 63) == 0) s[k][w] = v;
  }
  __syncthreads();
  if (threadIdx.x < unsigned(kSlots)) {
    unsigned long long v = 0;
    for (int j = 0; j < nw; j++) v += s[threadIdx.x][j];
    out[threadIdx.x] = v;
  }
}

// The rests of a tile's rows: rows still pending after their slab slots scan [rb, re) of their
// transposed row.  Long rests (> kLongRest entries) are scanned by the whole wave, 64 entries a
// step; short ones by 16-lane groups, four rows at a time, so the tile's latency chain is paid
// once per four pending rows instead of once per row.  Both stop at the row's first hit.
template <int PK, int W, int R, typename InFront>
__device__ inline void bu_rest_scan(const bool (&pend)[R], bool (&found)[R], const int64_t (&rb)[R],
                                    const int64_t (&re)[R], const int32_t* __restrict__ tcol, const FastArgs& fp,
                                    int ru, uint32_t (&acc)[6], InFront in_front, const QArgs& q) {
  // entry test: frontier probe + predicate; a packed word settles the predicate from its bucket
  // before the probe, else the value is read after a probe hit
  auto entry = [&](int32_t raw, int64_t ex) -> bool {
    const int32_t g = q_gidx(raw, q);
    if (PK != PK_FAST) return in_front(g);
    const int t = q_test(raw, q);
    if (t == 0) return false;
    if (!in_front(g)) return false;
    if (t == 1) return true;
    acc[5]++;
    return fast_cmp(fp.op, load_w<W>(fp.data, fp.width, ex), fp.k);
  };
  const int lane = threadIdx.x & 63;
  constexpr int kLongRest = 256, GL = 16, NG = 64 / GL;
  unsigned long long pml[R], pms[R];
#pragma unroll
  for (int j = 0; j < R; j++) {
    const bool lng = pend[j] && re[j] - rb[j] > kLongRest;
    pml[j] = __ballot(lng);
    pms[j] = __ballot(pend[j] && !lng);
  }
#pragma unroll
  for (int j = 0; j < R; j++) {
    unsigned long long pm = pml[j];
    while (pm) {
      const int src = __ffsll((long long)pm) - 1;
      pm &= pm - 1;
      const int64_t b = __shfl((long long)rb[j], src), e = __shfl((long long)re[j], src);
      acc[3] += lane == 0;
      bool f = false;
      for (int64_t x = b; x < e && !f; x += 64 * ru) {
        int32_t sr[kRestMax];
#pragma unroll
        for (int u = 0; u < kRestMax; u++) {
          const int64_t ex = x + u * 64 + lane;
          sr[u] = (u < ru && ex < e) ? tcol[ex] : -1;
        }
        bool h = false;
#pragma unroll
        for (int u = 0; u < kRestMax; u++) {
          const int64_t ex = x + u * 64 + lane;
          if (sr[u] < 0) continue;
          acc[4]++;
          if (entry(sr[u], ex)) h = true;
        }
        f = __ballot(h) != 0;
      }
      if (lane == src) found[j] = f;
    }
  }
  {
    const int grp = lane / GL, gl = lane % GL;
    for (;;) {
      int my_j = -1, my_src = 0, taken = 0;
#pragma unroll
      for (int j = 0; j < R; j++) {
        while (pms[j] && taken < NG) {
          const int sidx = __ffsll((long long)pms[j]) - 1;
          if (taken == grp) {
            my_j = j;
            my_src = sidx;
          }
          pms[j] &= pms[j] - 1;
          taken++;
        }
      }
      if (taken == 0) break;
      int64_t b = 0, e = 0;
#pragma unroll
      for (int j = 0; j < R; j++) {
        const int64_t bj = __shfl((long long)rb[j], my_src), ej = __shfl((long long)re[j], my_src);
        if (my_j == j) {
          b = bj;
          e = ej;
        }
      }
      acc[3] += gl == 0 && my_j >= 0;
      bool f = false;
      for (int64_t x = b;; x += GL * ru) {
        const bool act = !f && x < e;
        if (__ballot(act) == 0) break;
        bool h = false;
        if (act) {
          int32_t sr[kRestMax];
#pragma unroll
          for (int u = 0; u < kRestMax; u++) {
            const int64_t ex = x + u * GL + gl;
            sr[u] = (u < ru && ex < e) ? tcol[ex] : -1;
          }
#pragma unroll
          for (int u = 0; u < kRestMax; u++) {
            const int64_t ex = x + u * GL + gl;
            if (sr[u] < 0) continue;
            acc[4]++;
            if (entry(sr[u], ex)) h = true;
          }
        }
        const unsigned long long hb = __ballot(h);
        if (act && ((hb >> (grp * GL)) & ((1ull << GL) - 1ull))) f = true;
      }
#pragma unroll
      for (int g = 0; g < NG; g++) {
        const int sj = __shfl(my_j, g * GL), ss = __shfl(my_src, g * GL);
        const int fg = __shfl(int(f), g * GL);
#pragma unroll
        for (int j = 0; j < R; j++)
          if (sj == j && lane == ss) found[j] = fg != 0;
      }
    }
  }
}

// Bottom-up hop (direction-optimising BFS, Beamer et al.): every owned vertex d looks for an
// in-neighbour (transposed CSR) in the frontier bitmap whose edge passes the predicate, and is
// in the next frontier iff it finds one -- the set getDstIdsFromResp builds
// (GoExecutor.cpp:407-431), with no random writes: the frontier bitmap is read-only and each
// wave writes only its own words.  Two passes: k_bu_lean over the quad slab (the first 4
// hub-first in-neighbours of every transposed row, two 8-byte halves per row), then
// k_bu_rest_lean over the rows it left pending.
// The first pass's instruction stream is cut to what the hop needs (round 2: a general slab
// kernel with per-slot branches and bounds checks was issue-bound at ~2.2 TB/s with no probes):
//  * the slab halves and the out-degrees are padded to whole 128-row tiles at build (pad slots
//    -1, degree 0), so the tile loads carry no bounds checks and no branches;
//  * a lane owns rows l and l + 64 of a 128-row tile (8-byte loads per half), so the two ballots
//    are the tile's two 64-row frontier words as they are;
//  * U tiles per iteration: every slab load of the U tiles is issued, then every probe, then the
//    bit tests (sched_barrier keeps the scheduler from pulling the consumers up to the loads,
//    which put a vmcnt(0) wait behind every probe);
//  * every probe is a buffer load whose offset is out of bounds for a non-candidate slot (the
//    hardware returns 0: no branch);
//  * a non-final hop (PK_NONE) reads the second half only for rows still pending after the
//    first (almost none: hub-first slot 0 is nearly always in a dense frontier), and only the
//    tiles below es.bu_both_tiles (the last row with an in- and an out-edge: one rank numbers
//    such vertices first, snapshot k_class_key); the tiles past it get zero words;
//  * a non-final hop reads its tile's shape word (EdgeSpace::tile_shape, option bu_lean_shape)
//    through a scalar load one tile ahead: a two-slot tile (no row has a third entry) leaves no
//    row pending, so the second half is never entered for it, and a uniform tile (every row that
//    can be found has the same out-degree) loads no per-row degree and adds degree x found rows
//    to the sum -- wave-uniform run-time branches, mixed and wide tiles run as before
//    (DESIGN.md section 6);
//  * the final hop (PK_FAST) decides each slot by two scalar compares of its packed bucket
//    (QArgs); a frontier hit in an undecided bucket and rows with more than 4 entries are left
//    pending for k_bu_rest_lean (rest_from 0).  A predicate on a column that is not the packed
//    one makes every bucket undecided: the first pass then only clears rows with no frontier
//    in-neighbour among their slots, and the rest pass reads the values.
// Outputs: next-frontier and pending words; partials [0] found, [1] their out-degree sum,
// [2] slab words read, [3] pending rows.  STATS with tile_stats (bu_probe_stats 2 / 3): [6] / [7]
// count a non-final hop's work tiles by shape (1: two-slot / uniform, 2: both / neither) instead
// of the probes.
// HUB: the block keeps the first cw words of the bitmap (the highest-out-degree vertices) in LDS
// and answers candidates there from it; the global probe of such a slot is out of bounds.
// Partials [6] / [7]: candidate probes sent to L2 / answered from LDS.
template <int PK, int U, int HUB, int STATS, int NT = 0, int SKIP = 0>
__global__ __launch_bounds__(1024, 8) void k_bu_lean(const uint2* __restrict__ lo, const uint2* __restrict__ hi,
                                                     int64_t ntiles, int64_t work_tiles,
                                                     const uint32_t* __restrict__ fbits, uint32_t fb_bytes,
                                                     unsigned long long* __restrict__ nbits,
                                                     unsigned long long* __restrict__ pbits,
                                                     const uint32_t* __restrict__ odeg, QArgs q_arg,
                                                     unsigned long long* __restrict__ partials, int cw,
                                                     const uint8_t* __restrict__ odeg8,
                                                     unsigned long long* gate, GateIn gi, int atomic_sums,
                                                     const uint32_t* __restrict__ shape, int tile_stats) {
  if (!gate_open(gi, gate)) return;  // a speculative hop that the direction choice did not take
  __shared__ unsigned long long lds[kSlots * 16];
  extern __shared__ uint32_t s_fb[];  // [0, cw): the bitmap's hub words; [cw]: a zero word
  if (HUB) hub_fill(s_fb, fbits, cw, true);
  const QArgs q = q_sgpr(q_arg);
  constexpr bool FINAL = PK == PK_FAST;
  constexpr int NS = FINAL ? 4 : 2;  // slots probed per row in the first round
  // out-of-bounds reads of the bitmap return 0: a non-candidate's probe, and an empty slot
  // (-1: its gidx bits are all ones, past every vertex, as the build guarantees)
  const __amdgpu_buffer_rsrc_t fb_rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(fbits), 0, int(fb_bytes), 0x00020000);
  const uint32_t gmask = q.gmask, ucw = uint32_t(cw);
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  uint32_t nglob = 0, nhub = 0;
  unsigned long long nfound = 0, npend = 0, nwords = 0;  // wave-uniform
  unsigned long long odsum = 0;
  unsigned long long odsum_u = 0;  // wave-uniform: the found rows of uniform tiles, degree x count
  // Non-final hops: the tile's shape word (EdgeSpace::tile_shape; shape == nullptr: every tile
  // wide and mixed, the code below as it was), a wave-uniform index, so a scalar load; past the
  // work tiles it reads the word of tile work_tiles, at most the array's padding.
  auto shape_index = [&](int64_t t) -> uint32_t {
    return __builtin_amdgcn_readfirstlane(uint32_t(min(t, work_tiles)));
  };
  auto shape_word = [&](uint32_t i) -> uint32_t { return FINAL || !shape ? kShapeWide | kShapeMixed : shape[i]; };
  uint32_t shn[U];  // asked for one iteration ahead
#pragma unroll
  for (int u = 0; u < U; u++) shn[u] = shape_word(shape_index(wave * U + u));
  // One slot word: its probe (global byte offset, out of bounds unless an L2 candidate; LDS
  // index, cw -- the zero word -- unless a hub candidate) and, final hop, its bucket's answer
  // (bit k of `pm` pass, of `um` undecided).  A failing bucket is no candidate; an undecided
  // one is probed too, so only a frontier hit there leaves the row pending.
  auto prep = [&](uint32_t sw, int k, uint32_t& goff, uint32_t& lidx, uint32_t& pm, uint32_t& um) {
    const uint32_t wi = (sw & gmask) >> 5;
    bool cand = true;
    if (FINAL) {
      const int st = q_test(int32_t(sw), q);  // below / above may be -1 (undecided) too
      const bool und = st < 0, pass = st > 0;
      cand = st != 0;
      pm |= pass ? 1u << k : 0u;
      um |= und ? 1u << k : 0u;
    }
    const bool hub = HUB && wi < ucw;
    goff = cand && !hub ? wi * 4u : 0xfffffff0u;
    lidx = cand && hub ? wi : ucw;
    if (STATS && !tile_stats) {  // (diagnostic instantiation: the counters' masks cost the hot loop registers)
      nglob += cand && !hub;
      nhub += cand && hub;
    }
  };
  auto bit = [](uint32_t w, uint32_t sw) -> uint32_t { return __builtin_amdgcn_ubfe(w, sw & 31u, 1u); };
  // (a 16-byte-lane layout, lane l holding rows 2l and 2l + 1, measured 104.7 us against 91.6)
  auto row_of = [&](int64_t t, int h) -> int64_t { return t * 128 + lane + 64 * h; };
  for (int64_t t0 = wave * U; t0 < work_tiles; t0 += nwaves * U) {
    uint2 a[U][2], b[U][2];
    uint32_t od[U][2];
    bool v[U];
    // this iteration's shape words are taken first, then the next iteration's are asked for,
    // ahead of the tiles' work: the wait is then for loads issued an iteration ago (k_bu_fin's
    // form; with the loads above it every tile waited a scalar round trip).  The empty asm ties
    // the next load's index to this iteration's word in its register: the compiler otherwise
    // sinks the word's first use, and with it the wait, below the new load.
    bool two[U], uni[U];  // wave-uniform: no row has a third entry / every row has out-degree ud
    uint32_t ud[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      uint32_t cur = shn[u];
      if (!FINAL) {
        uint32_t ni = shape_index(t0 + nwaves * U + u);
        asm volatile("" : "+s"(cur), "+s"(ni));
        __builtin_amdgcn_sched_barrier(0);
        shn[u] = shape_word(ni);
      }
      two[u] = (cur & kShapeWide) == 0u;
      ud[u] = cur & kShapeMixed;
      uni[u] = ud[u] != kShapeMixed;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      v[u] = t0 + u < work_tiles;
      const int64_t r = (v[u] ? t0 + u : t0) * 128 + lane;  // a past-the-end tile re-reads t0 (discarded)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (NT) {  // the slab and degrees are read once per hop: keep L2 for the bitmap probes
          const uint64_t x = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(lo + r + 64 * h));
          a[u][h] = make_uint2(uint32_t(x), uint32_t(x >> 32));
          if (FINAL) {
            const uint64_t y = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(hi + r + 64 * h));
            b[u][h] = make_uint2(uint32_t(y), uint32_t(y >> 32));
          }
          // 1 B per row; 255 stands for a larger degree, read from odeg where a row is found
          // (a uniform tile: the degree is in its shape word, no load)
          od[u][h] = FINAL ? 1u : ud[u];
          if (!FINAL && !uni[u]) od[u][h] = uint32_t(__builtin_nontemporal_load(odeg8 + r + 64 * h));
        } else {
          a[u][h] = lo[r + 64 * h];
          if (FINAL) b[u][h] = hi[r + 64 * h];
          od[u][h] = FINAL ? 1u : ud[u];
          if (!FINAL && !uni[u]) od[u][h] = odeg[r + 64 * h];
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t goff[U][2][NS], lidx[U][2][NS], pm[U][2], um[U][2];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        pm[u][h] = um[u][h] = 0u;
        prep(a[u][h].x, 0, goff[u][h][0], lidx[u][h][0], pm[u][h], um[u][h]);
        prep(a[u][h].y, 1, goff[u][h][1], lidx[u][h][1], pm[u][h], um[u][h]);
        if (FINAL) {
          prep(b[u][h].x, 2, goff[u][h][2], lidx[u][h][2], pm[u][h], um[u][h]);
          prep(b[u][h].y, 3, goff[u][h][3], lidx[u][h][3], pm[u][h], um[u][h]);
        }
      }
    // probes: the LDS reads first (answered in ~100 cycles), then the L2 ones, each into a
    // register of its own, OR-ed afterwards (one of the two is always 0)
    // SKIP: a probe instruction only when some lane of the wave has a candidate for it (most
    // slot registers of a tile need few or no L2 probes: the hub copy answers the hub sources)
    uint32_t lw[U][2][NS], gw[U][2][NS];
    if (HUB) {
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
          for (int k = 0; k < NS; k++) {
            if (SKIP) {
              lw[u][h][k] = 0u;
              if (__ballot(lidx[u][h][k] != ucw)) lw[u][h][k] = s_fb[lidx[u][h][k]];
            } else {
              lw[u][h][k] = s_fb[lidx[u][h][k]];
            }
          }
    }
    // SKIP bit 1 (non-final hops): rows already found through a hub word, and rows without
    // out-edges (they cannot extend the next frontier), send no L2 probe
    bool noprobe[U][2];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        noprobe[u][h] = false;
        if ((SKIP & 2) && HUB && !FINAL) {
          const uint32_t sw[2] = {a[u][h].x, a[u][h].y};
          bool hf = false;
#pragma unroll
          for (int k = 0; k < NS; k++) hf = hf || bit(lw[u][h][k], sw[k]) != 0u;
          noprobe[u][h] = hf || od[u][h] == 0u;
        }
      }
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int k = 0; k < NS; k++) {
          if (SKIP) {
            gw[u][h][k] = 0u;
            const uint32_t go = noprobe[u][h] ? 0xfffffff0u : goff[u][h][k];
            if (__ballot(go != 0xfffffff0u)) gw[u][h][k] = __builtin_amdgcn_raw_buffer_load_b32(fb_rs, go, 0, 0);
          } else {
            gw[u][h][k] = __builtin_amdgcn_raw_buffer_load_b32(fb_rs, goff[u][h][k], 0, 0);
          }
        }
    __builtin_amdgcn_sched_barrier(0);
    bool f[U][2], pend[U][2];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t sw[4] = {a[u][h].x, a[u][h].y, b[u][h].x, b[u][h].y};
        uint32_t hm = 0u;
#pragma unroll
        for (int k = 0; k < NS; k++) hm |= bit(HUB ? (lw[u][h][k] | gw[u][h][k]) : gw[u][h][k], sw[k]) << k;
        if (FINAL) {
          f[u][h] = (hm & pm[u][h]) != 0u;
          // not found: pending when a frontier hit sits in an undecided bucket, or the row has
          // a fifth entry (slot 3 present)
          pend[u][h] = v[u] && !f[u][h] && (b[u][h].y != 0xffffffffu || (hm & um[u][h]) != 0u);
        } else {
          f[u][h] = hm != 0u && od[u][h] > 0;
          // rows with a third slot to test: live, not found, slot 1 present -- none in a
          // two-slot tile (no row of it has a third entry: its pending words are zero)
          pend[u][h] = v[u] && !two[u] && hm == 0u && od[u][h] > 0 && a[u][h].y != 0xffffffffu;
        }
      }
      nwords += v[u] ? (FINAL ? 8u : 4u) * 64u : 0u;  // every lane's two rows
    }
    if (!FINAL) {
      // second half, lazily: only lanes with a pending row load it (rarely any at all)
      bool anyp = false;
#pragma unroll
      for (int u = 0; u < U; u++) anyp = anyp || pend[u][0] || pend[u][1];
      const unsigned long long anyb = __ballot(anyp);
      if (anyb) {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
          for (int h = 0; h < 2; h++) {
            b[u][h] = make_uint2(0xffffffffu, 0xffffffffu);
            if (pend[u][h]) b[u][h] = hi[row_of(t0 + u, h)];
          }
        uint64_t pc = 0;  // rows reading the second half: 2 words each
#pragma unroll
        for (int u = 0; u < U; u++) pc += uint64_t(__popcll(__ballot(pend[u][0])) + __popcll(__ballot(pend[u][1])));
        nwords += 2 * pc;
        uint32_t g2[U][2][2], l2[U][2][2];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
          for (int h = 0; h < 2; h++) {
            uint32_t d0 = 0u, d1 = 0u;
            prep(b[u][h].x, 0, g2[u][h][0], l2[u][h][0], d0, d1);
            prep(b[u][h].y, 1, g2[u][h][1], l2[u][h][1], d0, d1);
          }
        uint32_t lv[U][2][2], gv[U][2][2];
        if (HUB) {
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
              for (int k = 0; k < 2; k++) lv[u][h][k] = s_fb[l2[u][h][k]];
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
          for (int h = 0; h < 2; h++)
#pragma unroll
            for (int k = 0; k < 2; k++) gv[u][h][k] = __builtin_amdgcn_raw_buffer_load_b32(fb_rs, g2[u][h][k], 0, 0);
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const uint32_t w0 = HUB ? (lv[u][h][0] | gv[u][h][0]) : gv[u][h][0];
            const uint32_t w1 = HUB ? (lv[u][h][1] | gv[u][h][1]) : gv[u][h][1];
            const bool g = (bit(w0, b[u][h].x) | bit(w1, b[u][h].y)) != 0u;
            f[u][h] = f[u][h] || (pend[u][h] && g);
            // still pending: not found in the second half and a fifth entry may exist
            pend[u][h] = pend[u][h] && !g && b[u][h].y != 0xffffffffu;
          }
      } else {
#pragma unroll
        for (int u = 0; u < U; u++) pend[u][0] = pend[u][1] = false;
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (!v[u]) continue;  // wave-uniform
      const int64_t t = t0 + u;
      unsigned long long f0 = __ballot(f[u][0]), f1 = __ballot(f[u][1]);
      unsigned long long p0 = __ballot(pend[u][0]), p1 = __ballot(pend[u][1]);
      if (SKIP & 4) {  // one store: lane 0 the tile's two next-frontier words, lane 1 the pending ones
        if (lane < 2) {
          typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
          u64x2 vv;
          vv.x = lane ? p0 : f0;
          vv.y = lane ? p1 : f1;
          *reinterpret_cast<u64x2*>((lane ? pbits : nbits) + 2 * t) = vv;
        }
      } else if (lane < 2) {
        nbits[2 * t + lane] = lane ? f1 : f0;
        pbits[2 * t + lane] = lane ? p1 : p0;
      }
      nfound += uint64_t(__popcll(f0) + __popcll(f1));
      npend += uint64_t(__popcll(p0) + __popcll(p1));
      if (!FINAL) {
        if (uni[u]) {  // wave-uniform
          odsum_u += uint64_t(ud[u]) * uint64_t(__popcll(f0) + __popcll(f1));
        } else {
#pragma unroll
          for (int h = 0; h < 2; h++) {
            uint32_t d = f[u][h] ? od[u][h] : 0u;
            if (NT && d == 255u) d = odeg[row_of(t, h)];  // odeg8 saturates at 255
            odsum += uint64_t(d);
          }
        }
        if (STATS && tile_stats) {  // (diagnostic) the tiles by shape instead of the probes
          const bool c6 = tile_stats == 2 ? two[u] && uni[u] : two[u];
          const bool c7 = tile_stats == 2 ? !two[u] && !uni[u] : uni[u];
          nglob += lane == 0 && c6;
          nhub += lane == 0 && c7;
        }
      }
    }
  }
  // tiles past the live rows (non-final hops): nothing can be found there
  for (int64_t t = work_tiles + wave; t < ntiles; t += nwaves)
    if (lane < 2) {
      nbits[2 * t + lane] = 0ull;
      pbits[2 * t + lane] = 0ull;
    }
  // wave-uniform counters enter the block sums once, from lane 0
  if (lane != 0) nfound = npend = nwords = 0;
  if (lane == 0) odsum += odsum_u;
  unsigned long long acc64[8] = {nfound, odsum, nwords, npend, 0, 0, nglob, nhub};
  if (atomic_sums) block_add_sums(acc64, 8, lds, partials, atomic_sums);
  else block_store_partials(acc64, 8, lds, partials);
}

// Final-hop first pass with the bucket tests as unsigned range checks on the raw slot word
// (k_bu_lean's select chain cost ~19 vector instructions per slot; the r04d PMC pass showed its
// waves busy issuing, 225 VALU per 128-row tile, the HBM stream at 4 TB/s).  FinArgs, host-built
// per query (fin_args): a word is a candidate iff (w - clo) <= cr, it passes iff
// ((w - plo) <= pr) != pinv (the bucket field sits above the gidx bits, so bucket ranges are
// word ranges; the -1 pad word is a candidate of every range that reaches the top field: its
// probe, gidx 2^gbits - 1, is past the bitmap or, when n_global > 2^gbits - 32, reads a bit of
// the last word that no vertex owns and no frontier sets, see build_transpose).  A candidate's
// probe byte offset is (w >> 3) & bmask, a non-candidate's kNoProbe; the global probe reads
// through a resource based cw words into the bitmap (hub words wrap out of bounds: the hardware
// returns 0), the LDS probe reads min(offset, 4 cw) (the zero word past the hub copy).
constexpr uint32_t kNoProbe = 0x0ffffff0u;
// CLS 1: the candidates are every word from clo up and the passing ones every word from plo up
// (pinv 0): the "greater than" compares, the benchmark's.  A non-candidate's offset then comes
// from the sign of w - clo (all ones: past the bitmap and clamped to the zero word) instead of
// a compare and a select, and the pass test is one compare.  The sign test is stricter than the
// range test on the -1 pad word alone: while clo < 2^31 it sends the pad no probe at all, where
// the generic form probes the unowned bit (the same answer: that bit is never set).
// NT: non-temporal slab loads (the slab is read once per hop; the bitmap the probes hit stays
// in L2): 158 -> 148 us at C3.  Measured without gain (r04f/r04g): the next tile's slab loads
// issued behind the current tile's probes, an interleaved 16-byte slab (one load per row), two
// tiles per wave; with no probes at all the slab alone streams at 4.7 TB/s in this loop.
// Round 4 (r06h: 124.9 -> 105.8 us at C3): a probe instruction is issued only when some lane of
// the wave has an L2 candidate in that slot; one 16-byte store of the tile's next / pending
// words; rows a hub word already found send no L2 probe.  Measured without gain and removed
// (r06e-r06h): contiguous tile ranges per wave, the same skip for the LDS reads, 16-byte lanes
// (rows 2l and 2l + 1 per lane), the tile's L2 probes packed into the fewest lanes through an
// LDS scratch.  Round 5, removed in round 6: the 3-slot slab (12 B a row, slot 2 flagging a fourth
// entry in bit 31): this pass 106.9 -> 90.5 us but the rest pass 43 -> 74 us, the query 0.413 ->
// 0.425 ms (r10e).
// Two-slot tiles (wide: EdgeSpace::tile_wide, nullptr = every tile has four slots): a tile whose
// bit is clear has no row with a third entry, so its slots 2-3 are pad; the wave loads `lo`
// only and runs the pipeline for slots 0-1 (a wave-uniform run-time branch: the kernel keeps
// its two template parameters, profiles and tests go by its name).  DESIGN.md section 6.
template <int CLS, int NT>
__global__ __launch_bounds__(1024, 8) void k_bu_fin(const uint2* __restrict__ lo, const uint2* __restrict__ hi,
                                                    int64_t ntiles, int64_t work_tiles,
                                                    const uint32_t* __restrict__ fbits,
                                                    unsigned long long* __restrict__ nbits,
                                                    unsigned long long* __restrict__ pbits, FinArgs fa_arg,
                                                    unsigned long long* __restrict__ partials, int cw,
                                                    uint32_t fb_rest, unsigned long long* gate, GateIn gi,
                                                    int atomic_sums, const uint32_t* __restrict__ wide) {
  if (!gate_open(gi, gate)) return;  // a speculative hop that the direction choice did not take
  // dynamic LDS only, so the hub copy starts at address 0 and a probe's LDS address is its
  // clamped byte offset as it is: [0, cw) the bitmap's hub words, [cw] a zero word, then the
  // block's partials scratch
  extern __shared__ uint32_t s_fb[];
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(s_fb + ((cw + 2) & ~1));
  hub_fill(s_fb, fbits, cw, true);
  const uint32_t clo = __builtin_amdgcn_readfirstlane(fa_arg.clo), cr = __builtin_amdgcn_readfirstlane(fa_arg.cr);
  const uint32_t plo = __builtin_amdgcn_readfirstlane(fa_arg.plo), pr = __builtin_amdgcn_readfirstlane(fa_arg.pr);
  const bool pinv = __builtin_amdgcn_readfirstlane(fa_arg.pinv) != 0;
  const uint32_t bmask = __builtin_amdgcn_readfirstlane(fa_arg.bmask);
  const uint32_t cw4 = __builtin_amdgcn_readfirstlane(uint32_t(cw) * 4u);
  // global probes: the bitmap from word cw on (fb_rest bytes); offsets below it (hub words) wrap
  // past the end
  const __amdgpu_buffer_rsrc_t fb_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(fbits + cw), 0, int(__builtin_amdgcn_readfirstlane(fb_rest)), 0x00020000);
  // the hub copy is the kernel's only LDS (dynamic, no static arrays), at LDS address 0: a
  // probe's address is its clamped byte offset (a pointer form cost an add per probe)
  typedef const __attribute__((address_space(3))) uint32_t* lds_u32p;
  const int lane = threadIdx.x & 63;
  // (in a scalar register: the tile index picks the tile's path and its tile_wide word)
  const int64_t wave =
      int64_t(__builtin_amdgcn_readfirstlane(uint32_t((int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6)));
  const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  unsigned long long nfound = 0, npend = 0, nwords = 0;  // wave-uniform
  auto ld8 = [&](const uint2* p) -> uint2 {
    if (!NT) return *p;
    const uint64_t x = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(p));
    return make_uint2(uint32_t(x), uint32_t(x >> 32));
  };
  const uint32_t rest_b = __builtin_amdgcn_readfirstlane(fb_rest);
  // one tile, NS slots per row: 4, or 2 for a tile whose rows all have at most two entries
  // (its slots 2-3 are pad: no candidate, no hit, no fifth entry -- not loaded, not probed)
  auto tile = [&](int64_t t, auto ns_c) {
    constexpr int NS = decltype(ns_c)::value;
    uint32_t sw[2][NS];
    const int64_t r = t * 128 + lane;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint2 a = ld8(lo + r + 64 * h);
      sw[h][0] = a.x, sw[h][1] = a.y;
      if (NS == 4) {
        const uint2 b = ld8(hi + r + 64 * h);
        sw[h][NS - 2] = b.x, sw[h][NS - 1] = b.y;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t ob[2][NS];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int k = 0; k < NS; k++) {
        const uint32_t w = sw[h][k];
        if (CLS == 1)
          ob[h][k] = ((w >> 3) & bmask) | fin_skip_cls1(w, clo);
        else
          ob[h][k] = fin_candidate(w, clo, cr) ? (w >> 3) & bmask : kNoProbe;
      }
    uint32_t lw[2][NS], gw[2][NS];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int k = 0; k < NS; k++) lw[h][k] = *(lds_u32p)(size_t(min(ob[h][k], cw4)));
    // rows already found through a hub word send no L2 probe (most found rows have a hub
    // in-neighbour in the frontier: their slots' L2 probes were wasted instructions)
    bool hubf[2] = {false, false};
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int k = 0; k < NS; k++) {
        const uint32_t w = sw[h][k];
        const bool pass = CLS == 1 ? w >= plo : (w - plo <= pr) != pinv;  // qpred.h fin_pass_cls1 / fin_pass
        hubf[h] = hubf[h] || (__builtin_amdgcn_ubfe(lw[h][k], w, 1u) != 0u && pass);
      }
    // a probe instruction only when some lane of the wave has an L2 candidate in that slot
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int k = 0; k < NS; k++) {
        gw[h][k] = 0u;
        if (__ballot(ob[h][k] - cw4 < rest_b && !hubf[h]))
          gw[h][k] = __builtin_amdgcn_raw_buffer_load_b32(fb_rs, hubf[h] ? 0xfffffff0u : ob[h][k] - cw4, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    bool f[2], pend[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      bool fh = false, ah = false;
#pragma unroll
      for (int k = 0; k < NS; k++) {
        const uint32_t w = sw[h][k];
        const bool hit = __builtin_amdgcn_ubfe(lw[h][k] | gw[h][k], w, 1u) != 0u;
        const bool pass = CLS == 1 ? w >= plo : (w - plo <= pr) != pinv;  // qpred.h fin_pass_cls1 / fin_pass
        fh = fh || (hit && pass);
        ah = ah || hit;
      }
      f[h] = fh;
      // pending: no passing hit, and a hit (then in an undecided bucket) or a fifth entry
      // (slot 3 set; never in a two-slot tile)
      pend[h] = !fh && (ah || (NS == 4 && sw[h][NS - 1] != 0xffffffffu));
    }
    unsigned long long f0 = __ballot(f[0]), f1 = __ballot(f[1]);
    unsigned long long p0 = __ballot(pend[0]), p1 = __ballot(pend[1]);
    // one store instruction: lane 0 the two next-frontier words, lane 1 the two pending words
    if (lane < 2) {
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      u64x2 v;
      v.x = lane ? p0 : f0;
      v.y = lane ? p1 : f1;
      *reinterpret_cast<u64x2*>((lane ? pbits : nbits) + 2 * t) = v;
    }
    nfound += uint64_t(__popcll(f0) + __popcll(f1));
    npend += uint64_t(__popcll(p0) + __popcll(p1));
    nwords += uint64_t(2 * NS) * 64u;
  };
  // tile_wide word of tile t (wave-uniform index: a scalar load); past the work tiles it reads
  // the word of tile work_tiles, at most the bitmap's padding word.  wide == nullptr: all wide.
  auto wide_word = [&](int64_t t) -> uint32_t {
    if (!wide) return 0xffffffffu;
    return wide[__builtin_amdgcn_readfirstlane(uint32_t(min(t, work_tiles) >> 5))];
  };
  uint32_t ww = wave < work_tiles ? wide_word(wave) : 0u;
  for (int64_t t = wave; t < work_tiles; t += nwaves) {
    // this tile's bit is tested first, then the next tile's word is asked for, ahead of this
    // tile's work: the wait is then for a load issued a tile ago.  (With the load above the
    // test the wait stood behind the new load too -- scalar loads return out of order, a wait
    // is for all of them -- a round trip per tile.)
    const uint32_t wbit = __builtin_amdgcn_readfirstlane((ww >> (uint32_t(t) & 31u)) & 1u);
    __builtin_amdgcn_sched_barrier(0);
    ww = wide_word(t + nwaves);
    if (wbit)
      tile(t, std::integral_constant<int, 4>{});
    else
      tile(t, std::integral_constant<int, 2>{});
  }
  // tiles past the last row with an in-edge: nothing to find
  for (int64_t t = work_tiles + wave; t < ntiles; t += nwaves)
    if (lane < 2) {
      nbits[2 * t + lane] = 0ull;
      pbits[2 * t + lane] = 0ull;
    }
  if (lane != 0) nfound = npend = nwords = 0;
  unsigned long long acc64[8] = {nfound, 0, nwords, npend, 0, 0, 0, 0};
  if (atomic_sums) block_add_sums(acc64, 8, lds, partials, atomic_sums);
  else block_store_partials(acc64, 8, lds, partials);
}

// Second pass of a bottom-up hop: the rows k_bu_lean left pending.  A wave owns 64 pending-bit
// words spread over the row range (one per lane, nwaves apart, so every wave samples the dense
// hub end and the sparse tail alike) and ranks their pending rows (wave prefix sum of the words'
// popcounts); 64 pending rows at a time, a lane scans its row's entries [row_ptr + rest_from,
// row_ptr + 1) in aligned 8-entry chunks (two 16-byte loads): all chunk loads issued, then all
// probes (buffer loads out of bounds for non-candidates, LDS for hub words), then the tests, as
// in k_bu_lean; a value is read only for a frontier hit in an undecided bucket.  After `steps`
// chunks the rows still pending (long in-edge lists) go to bu_rest_scan (whole wave / 16-lane
// groups).  Found rows OR into the wave's 64 next-frontier words in LDS, merged into nbits by
// the owning lanes (one writer per word).  Partials [0] found, [1] their out-degree sum, [3] rows
// scanned by bu_rest_scan (counted by the first pass), [4] entries read, [5] values read.
constexpr int kLeanChunk = 8;
// The 8 entries [a, a + 8) of a transposed row's chunk, a a multiple of 4: two 16-byte loads
// (one vector-memory instruction per 4 entries instead of one per entry -- the divergent
// per-entry gathers, 64 distinct lines per instruction, held the rest passes at the L1's
// per-line rate); the second only when the row continues past a + 4.  The columns are padded
// so the first load may run past the last row.
__device__ inline void load_chunk8(const int32_t* __restrict__ tcol, int64_t a, int64_t re, bool act,
                                   int32_t (&sv)[kLeanChunk]) {
  int4 x = make_int4(-1, -1, -1, -1), y = x;
  if (act) x = *reinterpret_cast<const int4*>(tcol + a);
  if (act && a + 4 < re) y = *reinterpret_cast<const int4*>(tcol + a + 4);
  sv[0] = x.x, sv[1] = x.y, sv[2] = x.z, sv[3] = x.w;
  sv[4] = y.x, sv[5] = y.y, sv[6] = y.z, sv[7] = y.w;
}
// REC: a pending row's start, in-degree and first kRecEntries entries come from its rest record
// (EdgeSpace::brec, one 64-byte line); rows longer than that continue in tcol from there.
template <int PK, int W, int HUB, int REC>
__global__ __launch_bounds__(1024, 4) void k_bu_rest_lean(const unsigned long long* __restrict__ pbits, int64_t n,
                                                          const int64_t* __restrict__ trp,
                                                          const int32_t* __restrict__ tcol,
                                                          const uint32_t* __restrict__ fbits, uint32_t fb_bytes,
                                                          unsigned long long* nbits,
                                                          const uint32_t* __restrict__ odeg, FastArgs fp, QArgs q_arg,
                                                          unsigned long long* partials, int cw, int ru, int rest_from,
                                                          int steps, unsigned long long* dbg,
                                                          const unsigned long long* __restrict__ gate,
                                                          const uint4* __restrict__ rec, int atomic_sums) {
  if (gate && *gate == 0ull) return;
  const QArgs q = q_sgpr(q_arg);
  __shared__ unsigned long long lds[kSlots * 16];
  __shared__ unsigned long long s_found[16][64];
  extern __shared__ uint32_t s_fb[];
  const unsigned long long t_in = wall_clock64();
  if (HUB) hub_fill(s_fb, fbits, cw, false);
  const unsigned long long t_hub = wall_clock64();
  uint32_t d_rows = 0, d_batches = 0, d_steps = 0, d_scan = 0;
  unsigned long long t_scan = 0;
  const __amdgpu_buffer_rsrc_t fb_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(fbits), 0, int(__builtin_amdgcn_readfirstlane(fb_bytes)), 0x00020000);
  auto in_front = [&](int32_t g) -> bool {
    const int32_t wi = g >> 5;
    uint32_t w;
    if (HUB && wi < cw) w = s_fb[wi];
    else w = __builtin_amdgcn_raw_buffer_load_b32(fb_rs, wi * 4, 0, 0);
    return (w >> (g & 31)) & 1u;
  };
  uint32_t acc[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long odsum = 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nwords = (n + 63) / 64;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  // a wave's 64 words are spread over the whole row range (word base + l * nwaves + wave for
  // lane l): the pending rows are dense among the hub rows at the low end, and a wave of 64
  // consecutive words there held 5-6 batches while most waves had one (r04h: 57 vs 12 us)
  for (int64_t cbase = 0; cbase + wave < nwords; cbase += nwaves * 64) {
    const int64_t myw = cbase + int64_t(lane) * nwaves + wave;
    const unsigned long long pw = myw < nwords ? pbits[myw] : 0ull;
    s_found[wv][lane] = 0ull;
    uint32_t total;
    const uint32_t pre = wave_excl_scan(uint32_t(__popcll(pw)), total);
    for (uint32_t k0 = 0; k0 < total; k0 += 64) {
      // the (k0 + lane)-th pending row of the chunk: its word (binary search over the lanes'
      // exclusive prefix sums) and the matching set bit of that word
      const uint32_t p = k0 + uint32_t(lane);
      bool pend[1] = {p < total}, found[1] = {false};
      int64_t rb[1] = {0}, re[1] = {0};
      int wsel = 0;
#pragma unroll
      for (int st = 32; st > 0; st >>= 1) {
        const uint32_t pv = __shfl(pre, wsel + st);
        if (wsel + st < 64 && pv <= p) wsel += st;
      }
      const unsigned long long wbits = __shfl((long long)pw, wsel);
      const uint32_t kk = p - __shfl(pre, wsel);  // the kk-th set bit of wbits
      int bit = 0;
#pragma unroll
      for (int st = 32; st > 0; st >>= 1)
        if (uint32_t(__popcll(wbits & ((1ull << (bit + st)) - 1ull))) <= kk) bit += st;
      const int32_t r = int32_t((cbase + int64_t(wsel) * nwaves + wave) * 64 + bit);
      // the entries [base, base + 8) (those in [lo_e, hi_e) are valid): bitmap probes, then the
      // tests; a frontier hit in the constant's bucket reads its value.  Wave-uniform call.
      auto test_chunk = [&](const int32_t(&sv)[kLeanChunk], int64_t base, int64_t lo_e, int64_t hi_e, bool act,
                            bool count) __attribute__((always_inline)) -> bool {
        uint32_t w[kLeanChunk];
        int tq[kLeanChunk];
#pragma unroll
        for (int k = 0; k < kLeanChunk; k++) {
          const bool valid = act && base + k >= lo_e && base + k < hi_e;
          if (count) acc[4] += valid;  // column entries (a record's are in its line)
          tq[k] = PK == PK_FAST ? q_test(sv[k], q) : 1;
          const bool cand = valid && tq[k] != 0;
          const int32_t wi = q_gidx(sv[k], q) >> 5;
          const bool hub = HUB && wi < cw;
          const uint32_t gw = __builtin_amdgcn_raw_buffer_load_b32(fb_rs, cand && !hub ? uint32_t(wi) * 4u : 0xfffffff0u,
                                                                   0, 0);
          if (HUB) {
            const uint32_t lw = s_fb[cand && hub ? wi : 0];
            w[k] = cand && hub ? lw : gw;
          } else {
            w[k] = gw;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        bool h = false, need = false;
        uint32_t und = 0;
#pragma unroll
        for (int k = 0; k < kLeanChunk; k++) {
          const bool inf = (w[k] >> (uint32_t(sv[k]) & 31u)) & 1u;
          h = h || (inf && tq[k] > 0);
          if (PK == PK_FAST && inf && tq[k] < 0) {
            und |= 1u << k;
            need = true;
          }
        }
        if (PK == PK_FAST && __ballot(need && !h)) {
          // frontier hits in the constant's bucket: the exact value decides
          if (!h) {
#pragma unroll
            for (int k = 0; k < kLeanChunk; k++)
              if ((und >> k) & 1u) {
                acc[5]++;
                h = h || fast_cmp(fp.op, load_w<W>(fp.data, fp.width, base + k), fp.k);
              }
          }
        }
        return h;
      };
      int64_t r0 = 0;  // the row's first entry to test; chunks start at the aligned a <= r0
      if (REC) {
        // the rest record: entries [0, 8) and [8, kRecEntries), then tcol past kRecEntries
        uint4 x0 = make_uint4(0u, 0u, 0u, 0u), x1 = x0, x2 = x0, x3 = x0;
        if (pend[0]) {
          const uint4* rp = rec + size_t(r) * 4;
          x0 = rp[0], x1 = rp[1], x2 = rp[2], x3 = rp[3];
        }
        const int64_t start = int64_t(x0.x) | (int64_t(x0.y & 0xffffu) << 32);
        const uint32_t deg = x0.y >> 16;
        const int64_t rend = start + int64_t(deg < uint32_t(kRecEntries) ? deg : uint32_t(kRecEntries));
        r0 = start + rest_from;
        const int32_t sa[kLeanChunk] = {int32_t(x0.z), int32_t(x0.w), int32_t(x1.x), int32_t(x1.y),
                                        int32_t(x1.z), int32_t(x1.w), int32_t(x2.x), int32_t(x2.y)};
        bool h = test_chunk(sa, start, r0, rend, pend[0], false);
        if (__ballot(pend[0] && !h && deg > 8u)) {
          const int32_t sb[kLeanChunk] = {int32_t(x2.z), int32_t(x2.w), int32_t(x3.x), int32_t(x3.y),
                                          int32_t(x3.z), int32_t(x3.w), -1, -1};
          h = test_chunk(sb, start + 8, r0, rend, pend[0] && !h, false) || h;
        }
        if (h) found[0] = true;
        pend[0] = pend[0] && !h && deg > uint32_t(kRecEntries);
        if (pend[0]) {
          re[0] = deg < 65535u ? start + deg : trp[r + 1];
          r0 = start + kRecEntries;
          rb[0] = r0 & ~int64_t(3);
        }
      } else if (pend[0]) {
        r0 = trp[r] + rest_from;
        re[0] = trp[r + 1];
        rb[0] = r0 & ~int64_t(3);
        pend[0] = r0 < re[0];
      }
      d_batches++;
      d_rows += p < total;
      for (int step = 0; step < steps; step++) {
        if (__ballot(pend[0]) == 0) break;
        d_steps++;
        int32_t sv[kLeanChunk];
        load_chunk8(tcol, rb[0], re[0], pend[0], sv);
        __builtin_amdgcn_sched_barrier(0);
        const bool h = test_chunk(sv, rb[0], r0, re[0], pend[0], true);
        if (h) found[0] = true;
        rb[0] += kLeanChunk;
        pend[0] = pend[0] && !h && rb[0] < re[0];
      }
      const uint32_t a3 = acc[3];
      const unsigned long long ts0 = wall_clock64();
      bu_rest_scan<PK, W, 1>(pend, found, rb, re, tcol, fp, ru, acc, in_front, q);
      t_scan += wall_clock64() - ts0;
      d_scan += acc[3] - a3;
      acc[3] = a3;  // the pending rows were counted by the first pass
      if (found[0]) {
        atomicOr(&s_found[wv][wsel], 1ull << (r & 63));
        acc[0]++;
        if (odeg) odsum += odeg[r];
      }
    }
    __builtin_amdgcn_wave_barrier();
    const unsigned long long fw = s_found[wv][lane];
    if (fw) nbits[myw] |= fw;
    __builtin_amdgcn_wave_barrier();
  }
  if (dbg) {  // diagnostics: per wave timestamps (wall_clock64) and work
    const unsigned long long t_out = wall_clock64();
    uint32_t tr = d_rows, te = acc[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tr += __shfl_xor(tr, o), te += __shfl_xor(te, o);
    if (lane == 0) {
      unsigned long long* d = dbg + wave * 8;
      d[0] = t_in, d[1] = t_hub, d[2] = t_out, d[3] = tr, d[4] = d_batches << 16 | d_steps, d[5] = d_scan, d[6] = te,
      d[7] = t_scan;
    }
  }
  unsigned long long acc64[6] = {acc[0], odsum, acc[2], acc[3], acc[4], acc[5]};
  if (atomic_sums) block_add_sums(acc64, 6, lds, partials, atomic_sums);
  else block_store_partials(acc64, 6, lds, partials);
}

// bitmap -> compacted list.  mode 0: local rows (a top-down hop's frontier; the bitmaps this
// reads already exclude rows without out-edges); mode 1: vids of every set vertex (the DISTINCT
// _dst output).  A tile of 4096 words (131072 vertices) per block-iteration: the words and their
// exclusive offsets go to LDS, one returning atomic reserves the tile's output range, then each
// wave expands two words per step with one lane per bit, so consecutive set bits write
// consecutive output slots (coalesced stores, coalesced vid_of reads).
template <int MODE, int U = 4, int NT = 0>
__global__ __launch_bounds__(1024) void k_bits_compact(const uint32_t* __restrict__ bits, int64_t n, int64_t lo,
                                                       const int64_t* __restrict__ vid_of, void* out,
                                                       unsigned long long* n_out,
                                                       const unsigned long long* gate = nullptr) {
  if (gate && *gate == 0ull) return;
  // one word per thread: a 1024-thread block owns 1024 words (32 K vertices) per iteration, so
  // a 32.8 M-vertex bitmap is ~1000 blocks (4096-word tiles gave ~250: one block per CU, half
  // the resident waves this latency-bound gather needs); one counter atomic per tile
  constexpr int kTileWords = 1024;
  __shared__ uint32_t sw[kTileWords];
  __shared__ uint32_t so[kTileWords];
  __shared__ uint32_t lds[16];
  __shared__ unsigned long long s_base;
  const int64_t nwords = (n + 31) / 32;
  const int64_t ntiles = (nwords + kTileWords - 1) / kTileWords;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t w0 = t * kTileWords + int64_t(threadIdx.x);
    uint32_t x = w0 < nwords ? bits[w0] : 0u;
    // bits at or past n (a bitmap's unused tail may hold stale bits) are never listed
    if ((w0 + 1) * 32 > n && w0 < nwords) x &= (1u << uint32_t(n - w0 * 32)) - 1u;
    uint32_t total;
    const uint32_t pre = block_excl_scan_u32(__popc(x), total, lds);
    // the tile's output range: the returning atomic (serialised with every other tile's on the
    // one counter) is issued here and read only after the first step's vid_of loads are out, so
    // its wait overlaps them instead of preceding every load of the tile
    unsigned long long my_base = 0;
    if (threadIdx.x == 0 && total) my_base = atomicAdd(n_out, (unsigned long long)total);
    sw[threadIdx.x] = x;
    so[threadIdx.x] = pre;
    __syncthreads();
    if (total) {  // block-uniform
      // U word pairs per step: the step's U vid_of loads are issued before any of its stores,
      // so each lane keeps U HBM requests in flight instead of one load -> store chain per pair
      unsigned long long base = 0;
      const int half = lane >> 5, bit = lane & 31;
      const int per_wave = kTileWords / int(blockDim.x >> 6);
      for (int j = wv * per_wave; j < (wv + 1) * per_wave; j += 2 * U) {
        bool has[U];
        uint32_t rel[U];
        int64_t val[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int wi = j + 2 * u + half;
          const uint32_t xw = sw[wi];
          has[u] = (xw >> bit) & 1u;
          rel[u] = so[wi] + __popc(xw & ((1u << bit) - 1u));
          const int64_t v = (t * kTileWords + wi) * 32 + bit;
          val[u] = v;
          if (MODE == 1 && has[u]) val[u] = NT ? __builtin_nontemporal_load(vid_of + lo + v) : vid_of[lo + v];
        }
        if (j == wv * per_wave) {  // every wave's first step (same trip count in every wave)
          if (threadIdx.x == 0) s_base = my_base;
          __syncthreads();
          base = s_base;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (!has[u]) continue;
          if (MODE == 0) static_cast<int32_t*>(out)[base + rel[u]] = int32_t(val[u]);
          else if (NT) __builtin_nontemporal_store(val[u], static_cast<int64_t*>(out) + base + rel[u]);
          else static_cast<int64_t*>(out)[base + rel[u]] = val[u];
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// host drivers
// ------------------------------------------------------------------------------------------
void reduce_partials(Ctx& c, const unsigned long long* partials, int nblocks, unsigned long long* out,
                     const unsigned long long* gate) {
  k_reduce_partials<<<1, 1024, 0, c.stream>>>(partials, nblocks, out, gate);
}

// raise a kernel's dynamic LDS limit once per process (the attribute call costs a host round
// trip: done per launch it showed up as ~10 us gaps before every bottom-up pass)
static void lds_limit(const void* kern, size_t shm) {
  static std::mutex mu;
  static std::unordered_map<const void*, size_t> done;
  std::lock_guard<std::mutex> lk(mu);
  auto it = done.find(kern);
  if (it != done.end() && it->second >= shm) return;
  NBG_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(shm)));
  done[kern] = shm;
}

// QArgs of a hop on es: unpacked words, packed words whose every value is read (no typed
// compare, or one on another column than the packed one), or the bucket decisions (qpred.h).
QArgs make_qargs(const EdgeSpace& es, int pk, int fcol, const FastArgs& fp) {
  QArgs q;
  if (es.q_field < 0) return q;
  q.gmask = (1u << es.q_gbits) - 1u;
  q.gbits = es.q_gbits;
  if (pk != PK_FAST || fcol != es.q_field) return q;  // packed words, every value read
  return make_qargs_core(es.q_min, es.q_range, es.q_bits, es.q_gbits, fp.op, fp.k);
}

// the frontier as a list: the local rows of a bitmap's set bits (their count added to *n_out)
void launch_bits_list(Ctx& c, const uint32_t* bits, int64_t rows, int64_t lo, int32_t* out, unsigned long long* n_out) {
  k_bits_compact<0><<<grid_cap((rows + 31) / 32, 1024, 4096), 1024, 0, c.stream>>>(bits, rows, lo, nullptr, out, n_out);
}
// DISTINCT _dst output: the vids of a bitmap's set rows (8 word pairs per lane and step; r05
// sweep: 8 took the C3 final hop 266 -> 258 us against 4, removed in round 6)
void launch_bits_vids(Ctx& c, const uint32_t* bits, int64_t rows, int64_t lo, void* out, unsigned long long* n_out,
                      const unsigned long long* gate) {
  // non-temporal vid loads and output stores (the 173 MB of C3's output no longer pass through
  // L2 as dirty lines): 0.4048 -> 0.4001 ms a C3 query, 4 A/B pairs (+ 3: 0.403 -> 0.397)
  const int grid = grid_cap((rows + 31) / 32, 1024, 4096);
  k_bits_compact<1, 8, 1><<<grid, 1024, 0, c.stream>>>(bits, rows, lo, c.vid_of.as<int64_t>(), out, n_out, gate);
}

// bottom-up hop: the first pass (k_bu_lean) over the quad slab and the pending rows' rests in
// k_bu_rest_lean; counters reduced into out[0..8) (no synchronisation).  pk: PK_NONE (a
// non-final hop: odeg keeps found rows with out-edges and sums their degrees) or PK_FAST (the
// final hop's typed compare on transposed column fcol; decided from the packed buckets when fcol
// is the packed column, else every value of a frontier hit is read by the rest pass).
// hop_front: the frontier came out of a hop (not the starts), so on one rank with the
// class-ordered numbering (snapshot k_class_key) its bits lie below row bu_both_tiles * 128: a
// frontier vertex has an in-edge (it was found) and an out-edge (the hops keep only those).
// Probes past that bound are out of bounds of their buffer resource (the hardware answers 0
// without a memory access).
namespace {

// a kernel instantiation and the name rocprof reports for it, both from one spelling: what
// BuLaunch::k0 / k1 say is what ran (tests and bench.py match profiler rows by these names)
template <typename Fn>
struct Named {
  Fn fn;
  const char* name;
};
#define NBG_K(...) {__VA_ARGS__, "nbg::" #__VA_ARGS__}
static_assert(PK_NONE == 0 && PK_FAST == 1, "the kernel tables index by pk and spell it as a number");

// a hop's shape, derived once and read by both passes
struct BuPlan {
  QArgs q;
  bool fast = false;   // the final-hop kernels: PK_FAST, or no out-degrees (without a WHERE every bucket passes)
  int pk = PK_NONE;    // the instantiations' PK: PK_FAST iff fast
  int rest_from = 4;   // the rest pass starts past the slab slots, or rescans them (0: a slot may be undecided)
  int64_t ntiles = 0;  // 128-row tiles of the transposed rows
  int64_t work = 0;    // ... of them those that can hold a found row (the others get zero words unread)
  // first pass
  int cw = 0;          // hub words of the frontier bitmap in LDS (0: no hub copy)
  int bs = 256, grid = 1;
  size_t shm = 0;
  uint32_t fb_bytes = 0;  // the bitmap's bytes a probe may read
  int probe_stats = 0;    // partials [6] / [7]
  // 0: block partials + k_reduce_partials; else the blocks add into that many shards of `out`
  int atomic_sums = 0;
  // rest pass
  int grid2 = 512;
  int W = 0;  // predicate column width (final hop)
  int rcw = 0, ru = 1, rsteps = 4;
  size_t rshm = 4;
  int64_t rest_rows = 0;  // pending bits exist only below the work tiles
  bool use_rec = false;   // rest records cover every row the first pass can leave pending
};

BuPlan bu_plan(Ctx& c, const EdgeSpace& es, int pk, bool final, const FastArgs& fp, int fcol, bool hop_front,
               bool out_zero, int shards) {
  const Csr& tr = es.tr;
  if (pk != PK_NONE && pk != PK_FAST) throw Error(NBG_E_DEVICE, "bottom-up hop with a VM predicate");
  if (!es.pair_col[0].p) throw Error(NBG_E_DEVICE, "bottom-up hop without the quad slab");
  BuPlan p;
  // the final hop (no odeg) runs the final-hop kernels; without a WHERE every bucket passes
  p.fast = pk == PK_FAST || final;
  if (pk == PK_FAST) {
    // bu_qpred = 0 (tests): ignore the buckets, every frontier hit reads its value
    p.q = make_qargs(es, c.opt("bu_qpred", 1) != 0 ? pk : PK_NONE, fcol, fp);
  } else {
    p.q = make_qargs(es, PK_NONE, -1, fp);
    if (p.fast) p.q.ulo = p.q.uhi = INT32_MAX, p.q.below = p.q.above = 1;
  }
  // rows pending after the slab rescan it only when a slot may be undecided (a predicate)
  p.rest_from = pk == PK_FAST ? 0 : 4;
  p.pk = p.fast ? PK_FAST : PK_NONE;
  p.ntiles = (tr.n_rows + 127) / 128;
  // rows past the last one that can be found (final) or extend the next frontier (non-final)
  // get zero words without being read (exact bounds, snapshot build_transpose)
  p.work = std::min(p.ntiles, p.fast ? es.bu_in_tiles : es.bu_both_tiles);
  const int64_t waves = std::max<int64_t>(1, p.work);
  // hub words in LDS (bu_lean_lds_kb KiB, 0 = off): 1024-thread blocks, two per CU
  const int64_t fb_words = (c.n_global + 31) / 32;
  // bu_hub_cap (tests): at most that many hub words, so small graphs exercise the L2 probes too
  const int64_t hub_cap = std::max<int64_t>(0, c.opt("bu_hub_cap", 36 * 1024));
  // (final hop 72 KiB, two blocks per CU still fit: r06g/r06h 1 % faster than 64)
  p.cw = int(std::min<int64_t>(c.opt(p.fast ? "bu_lean_lds_kb_final" : "bu_lean_lds_kb", p.fast ? 72 : 64) * 256,
                               std::min<int64_t>({fb_words, int64_t(36 * 1024), hub_cap})));
  p.bs = p.cw > 0 ? 1024 : 256;
  p.grid = int(std::max<int64_t>(
      1, std::min<int64_t>((waves + p.bs / 64 - 1) / (p.bs / 64),
                           std::min<int64_t>(p.cw > 0 ? 512 : 2048, kAggBlocks / 2))));
  p.shm = size_t(p.cw + 1) * 4;  // + the zero word non-hub probes read
  p.fb_bytes = uint32_t(fb_words * 4);
  if (hop_front && !c.sharded && es.bu_both_tiles > 0)
    p.fb_bytes = uint32_t(std::min<int64_t>(p.fb_bytes, (es.bu_both_tiles * 128 + 31) / 32 * 4));
  p.probe_stats = int(c.opt("bu_probe_stats", 0));  // partials [6] / [7]
  // option bu_atomic_sums: both passes add their block sums into `out` (zeroed first unless the
  // caller's block is known zero) and no k_reduce_partials launch follows
  // (r06j: 0.4796 -> 0.4663 ms per C3 query, the two k_reduce_partials launches gone)
  // (sharded sums, shards > 1: only into a block the caller zeroed with its shards)
  p.atomic_sums =
      c.opt("bu_atomic_sums", 1) != 0 && c.opt("bu_rest_dbg", 0) == 0 ? (out_zero ? std::max(shards, 1) : 1) : 0;
  p.ru = int(std::max<int64_t>(1, std::min<int64_t>(c.opt("bu_unroll", 1), kRestMax)));
  p.W = p.fast ? int(fp.width) : 0;
  // the rest pass probes global memory only by default: its hub copy cost each block ~6 us of
  // LDS fill (r04h/r04k sweeps: 0.637 -> 0.625 ms per C3 query without it)
  p.rcw = int(std::min<int64_t>(c.opt(p.fast ? "bu_rest_lds_kb_final" : "bu_rest_lds_kb", 0) * 256,
                                std::min<int64_t>({fb_words, int64_t(36 * 1024), hub_cap})));
  p.rshm = size_t(std::max(p.rcw, 1)) * 4;
  p.rsteps = int(std::max<int64_t>(1, c.opt("bu_rest_steps", 4)));
  // pending bits exist only below the work tiles (the first pass zeroes the words past them)
  p.rest_rows = std::min(tr.n_rows, p.work * 128);
  // rest records cover every row the first pass can leave pending (rows below work tiles)
  p.use_rec = es.brec.p && es.brec_rows >= std::min(tr.n_rows, p.work * 128) && c.opt("bu_rec", 1) != 0;
  return p;
}

// the words both passes write: next-frontier bits, pending bits, their sums
struct BuOut {
  unsigned long long* nb;        // next-frontier words
  unsigned long long* pbits;     // pending words, 2 per tile
  unsigned long long* partials;  // the block partials, or `out` itself when the blocks add
  unsigned long long* gate;
};

// The first pass over the quad slab: k_bu_fin on a final hop (unless bu_fin = 0 or the probe
// statistics are on), else k_bu_lean.  Fills L.k0, od_bytes and flag_bytes.
void bu_first_pass(Ctx& c, const EdgeSpace& es, const BuPlan& p, const uint32_t* fb, const uint32_t* odeg,
                   const BuOut& o, const GateIn& gi, BuLaunch& L) {
  const uint2* lo = es.pair_col[0].as<uint2>();
  const uint2* hi = es.pair_col[1].as<uint2>();
  const int cw = p.cw;
  if (p.fast && !p.probe_stats && c.opt("bu_fin", 1) != 0) {
    using Fn = decltype(&k_bu_fin<0, 0>);
    static const Named<Fn> fin[4] = {NBG_K(k_bu_fin<0, 0>), NBG_K(k_bu_fin<1, 0>), NBG_K(k_bu_fin<0, 1>),
                                     NBG_K(k_bu_fin<1, 1>)};
    const FinArgs fa = fin_args(p.q);
    // CLS 1 ("greater than"): candidates and passing words are each one upper range
    const bool cls1 = fin_cls1_ok(fa) && c.opt("bu_fin_cls", 1) != 0;
    const size_t fshm = size_t((cw + 2) & ~1) * 4 + size_t(kSlots) * 16 * 8;
    const uint32_t rest = p.fb_bytes > uint32_t(cw) * 4u ? p.fb_bytes - uint32_t(cw) * 4u : 0u;
    const int nt = int(c.opt("bu_fin_nt", 1) != 0);
    // bu_fin_narrow = 0 (A/B runs, tests): every tile reads both halves
    const uint32_t* wide = c.opt("bu_fin_narrow", 1) != 0 ? es.tile_wide.as<uint32_t>() : nullptr;
    if (wide) L.flag_bytes = uint64_t(p.work) / 8;  // tile_wide words the final first pass read
    const Named<Fn>& k = fin[(cls1 ? 1 : 0) | nt << 1];
    if (fshm > 48 * 1024) lds_limit(reinterpret_cast<const void*>(k.fn), fshm);
    k.fn<<<p.grid, p.bs, fshm, c.stream>>>(lo, hi, p.ntiles, p.work, fb, o.nb, o.pbits, fa, o.partials, cw, rest, o.gate,
                                           gi, p.atomic_sums, wide);
    L.k0 = k.name;
    return;
  }
  // no hub copy / hub copy; their counting (diagnostic) instantiations; kHubNt the default:
  // non-temporal slab, 1 B degrees, the probe skip and hub-first L2 probes (r06j: 100.7 -> 91.6 us
  // at C3 hop 2).  Removed in round 6, each measured without gain: two tiles per iteration
  // (bu_lean_u 2), one store per tile in the non-final pass (bu_lean_skip 7), the probe skip
  // without the hub-first probes (bu_lean_skip 1).
  enum { kPlain, kHub, kPlainStats, kHubStats, kHubNt };
  using Fn = decltype(&k_bu_lean<0, 1, 0, 0, 0, 0>);
  static const Named<Fn> lean[2][5] = {
      {NBG_K(k_bu_lean<0, 1, 0, 0, 0, 0>), NBG_K(k_bu_lean<0, 1, 1, 0, 0, 0>), NBG_K(k_bu_lean<0, 1, 0, 1, 0, 0>),
       NBG_K(k_bu_lean<0, 1, 1, 1, 0, 0>), NBG_K(k_bu_lean<0, 1, 1, 0, 1, 3>)},
      {NBG_K(k_bu_lean<1, 1, 0, 0, 0, 0>), NBG_K(k_bu_lean<1, 1, 1, 0, 0, 0>), NBG_K(k_bu_lean<1, 1, 0, 1, 0, 0>),
       NBG_K(k_bu_lean<1, 1, 1, 1, 0, 0>), NBG_K(k_bu_lean<1, 1, 1, 0, 1, 3>)}};
  int sel = p.probe_stats ? (cw > 0 ? kHubStats : kPlainStats) : (cw > 0 ? kHub : kPlain);
  if (sel == kHub && (p.fast || es.odeg8.p)) sel = kHubNt;
  const Named<Fn>& k = lean[p.pk][sel];
  if (p.shm > 48 * 1024) lds_limit(reinterpret_cast<const void*>(k.fn), p.shm);
  // the shape words of a non-final hop (they describe es.odeg); bu_lean_shape = 0 (A/B runs,
  // tests): every tile runs as wide and mixed.  bu_probe_stats 2 / 3: the counting instantiations
  // count tiles by shape in [6] / [7]: two-slot / uniform, or both / neither
  const uint32_t* shape = !p.fast && odeg == es.odeg.as<uint32_t>() && c.opt("bu_lean_shape", 1) != 0
                              ? es.tile_shape.as<uint32_t>()
                              : nullptr;
  k.fn<<<p.grid, p.bs, p.shm, c.stream>>>(lo, hi, p.ntiles, p.work, fb, p.fb_bytes, o.nb, o.pbits,
                                          p.fast ? nullptr : odeg, p.q, o.partials, cw, es.odeg8.as<uint8_t>(), o.gate,
                                          gi, p.atomic_sums, shape, p.probe_stats > 1 ? p.probe_stats - 1 : 0);
  L.k0 = k.name;
  // the non-final first pass reads one out-degree per row of its work tiles: 1 B (odeg8, the
  // non-temporal instantiations) or 4 B (odeg); with the shape words 4 B per work tile and the
  // degrees of the mixed tiles only
  if (!p.fast) {
    const uint64_t od_tiles = shape ? uint64_t(p.work - std::min(p.work, es.shape_tiles[0])) : uint64_t(p.work);
    L.od_bytes = od_tiles * 128u * (sel == kHubNt ? 1u : 4u) + (shape ? uint64_t(p.work) * 4u : 0u);
  }
}

// The rest pass over the rows the first pass left pending.  Fills L.k1 and rest_rec.
void bu_rest_pass(Ctx& c, const EdgeSpace& es, const BuPlan& p, const uint32_t* fb, const uint32_t* odeg,
                  const FastArgs& fp, const BuOut& o, unsigned long long* dbg, BuLaunch& L) {
  using Fn = decltype(&k_bu_rest_lean<0, 0, 0, 0>);
  // [HUB << 1 | REC] of <PK, W>
#define NBG_REST_ROW(PKV, WV)                                                                     \
  {NBG_K(k_bu_rest_lean<PKV, WV, 0, 0>), NBG_K(k_bu_rest_lean<PKV, WV, 0, 1>), \
   NBG_K(k_bu_rest_lean<PKV, WV, 1, 0>), NBG_K(k_bu_rest_lean<PKV, WV, 1, 1>)}
  static const Named<Fn> rest_none[4] = NBG_REST_ROW(0, 0);
  // the predicate column's width: 1, 2, 4, and every other width as 8
  static const Named<Fn> rest_fast[4][4] = {NBG_REST_ROW(1, 1), NBG_REST_ROW(1, 2), NBG_REST_ROW(1, 4),
                                            NBG_REST_ROW(1, 8)};
#undef NBG_REST_ROW
  const int wi = p.W == 1 ? 0 : p.W == 2 ? 1 : p.W == 4 ? 2 : 3;
  const Named<Fn>& k = (p.fast ? rest_fast[wi] : rest_none)[(p.rcw > 0 ? 2 : 0) | (p.use_rec ? 1 : 0)];
  const Csr& tr = es.tr;
  const int32_t* tc = p.q.gbits ? es.tcol_q.as<int32_t>() : tr.col.as<int32_t>();
  const uint4* rec = p.use_rec ? es.brec.as<uint4>() : nullptr;
  if (p.rshm > 48 * 1024) lds_limit(reinterpret_cast<const void*>(k.fn), p.rshm);
  k.fn<<<p.grid2, 1024, p.rshm, c.stream>>>(o.pbits, p.rest_rows, tr.row_ptr.as<int64_t>(), tc, fb, p.fb_bytes, o.nb,
                                            odeg, fp, p.q, p.atomic_sums ? o.partials : o.partials + p.grid, p.rcw, p.ru,
                                            p.rest_from, p.rsteps, dbg, o.gate, rec, p.atomic_sums);
  L.k1 = k.name;
  L.rest_rec = p.use_rec;
}
#undef NBG_K

// diagnostics (option bu_rest_dbg): the rest pass's per-wave records appended to $NBG_DBG_FILE
void bu_rest_dbg_dump(Ctx& c, const unsigned long long* dbg, int pk, int grid2) {
  std::vector<unsigned long long> h(size_t(grid2) * 16 * 8);
  NBG_HIP(hipMemcpyAsync(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  if (const char* fn = getenv("NBG_DBG_FILE")) {
    if (FILE* f = fopen(fn, "ab")) {
      const uint64_t hdr[2] = {uint64_t(pk), uint64_t(grid2) * 16};
      fwrite(hdr, 8, 2, f);
      fwrite(h.data(), 8, h.size(), f);
      fclose(f);
    }
  }
}

}  // namespace

BuLaunch launch_bu_lean(Ctx& c, EdgeSpace& es, const uint32_t* fb, uint32_t* nbits, const uint32_t* odeg, int pk,
                        const FastArgs& fp, int fcol, unsigned long long* out, bool hop_front, unsigned long long* gate,
                        GateIn gi, bool out_zero, int shards) {
  const BuPlan p = bu_plan(c, es, pk, !odeg, fp, fcol, hop_front, out_zero, shards);
  c.ws_pend.ensure(size_t(p.ntiles * 2 + 2) * 8);  // the pending bits, 2 words per tile
  const BuOut o{reinterpret_cast<unsigned long long*>(nbits), c.ws_pend.as<unsigned long long>(),
                p.atomic_sums ? out : c.ws_partials.as<unsigned long long>(), gate};
  if (p.atomic_sums && !out_zero) NBG_HIP(hipMemsetAsync(out, 0, 8 * 8, c.stream));
  BuLaunch L;
  bu_first_pass(c, es, p, fb, odeg, o, gi, L);
  NBG_HIP(hipGetLastError());
  L.ev_first = timing_event(c);  // end of the first pass (the hop's kernel_ms)
  DevBuf dbg_buf;
  unsigned long long* dbg = nullptr;
  if (c.opt("bu_rest_dbg", 0)) {
    dbg_buf.alloc(size_t(p.grid2) * 16 * 64);
    NBG_HIP(hipMemsetAsync(dbg_buf.p, 0, size_t(p.grid2) * 16 * 64, c.stream));
    dbg = dbg_buf.as<unsigned long long>();
  }
  bu_rest_pass(c, es, p, fb, odeg, fp, o, dbg, L);
  NBG_HIP(hipGetLastError());
  if (!p.atomic_sums) reduce_partials(c, o.partials, p.grid + p.grid2, out, gate);
  NBG_HIP(hipGetLastError());
  if (dbg) bu_rest_dbg_dump(c, dbg, p.pk, p.grid2);
  return L;
}

// byte models of a bottom-up hop's two passes from their counters.
// First pass: 4 B per slab word read, the frontier bitmap once, the next-frontier and pending
// bits written, the out-degrees a non-final hop read (od_bytes: 1 B per work row from odeg8 --
// with the shape words 4 B per work tile and the bytes of the mixed tiles only;
// rounds 2-4 counted 4 B for every row, 1.5x the bytes the default kernel reads) or the
// tile_wide bits the final hop read (one per work tile; the slab words already count 4 a row
// for a two-slot tile).  Rest pass:
// a row_ptr pair (or a 64 B rest record) per pending row, 4 B per entry read, predicate values read.
uint64_t bu_first_bytes(const unsigned long long* h, int64_t n_rows, uint64_t od_bytes) {
  return h[kHopSlabWords] * 4 + 3 * (uint64_t(n_rows) / 8) + od_bytes;
}
uint64_t bu_rest_bytes(const unsigned long long* h, int pred_width, bool rec) {
  return h[kHopPending] * (rec ? 64 : 16) + h[kHopEntries] * 4 + h[kHopValues] * uint64_t(pred_width);
}

}  // namespace nbg
