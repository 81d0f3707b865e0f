// go_variants.hip -- the hop kernels of GO UPTO N STEPS and GO ... REVERSELY behind their launch
// functions, and the once-per-snapshot derived data their direction choices read: the degree
// statistics over ranks (global_degree_stats), the in-degrees of a REVERSELY query (ensure_rev)
// and the exact mirror check of the in keys against the out keys (check_mirror).
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <vector>

#include "device_common.h"
#include "edge_lookup.h"
#include "engine.h"
#include "go_device.h"
#include "go_launch.h"
#include "query_common.h"

namespace nbg {

// ---- GO UPTO N STEPS, DISTINCT: the hop kernels of the visited-pruned BFS (GoQuery::run_upto) ----
// State over the rank's owned rows, 64 rows a word: vis (vertices reached so far, the starts
// included), uni (of them those with out-edges: the union of the BFS levels B_k, the frontier of
// the one final step) and next (B_k+1: the rows first reached by this hop that have out-edges).
// One wave owns 64 consecutive rows in both kernels: it builds each word with a 64-bit ballot and
// lane 0 stores it, so no bitmap word needs an atomic and none is read by one workgroup and
// written by another inside a launch; the hops see each other's words through the stream order of
// their launches only.  sums (zeroed by the caller with their shards; one agent-scope add per
// block and word into shard block % shards, block_add_sums):
// [0] rows first reached, [1] their out-degree sum, [2] those of them with out-edges (next's
// population), [3] adjacency entries read (k_upto_bu).
//
// k_upto_claim, behind a top-down hop: mark = the owned slice of the byte map the expansion (and
// the mark exchange) wrote.  new = mark & ~vis; vis |= new; the marks are cleared.  Rows at or past
// n_read carry no mark (no in-edge: the class-ordered numbering puts them last) and are not read.
// list (optional): next as a list of local rows too, list_n its length.
__global__ __launch_bounds__(256) void k_upto_claim(uint8_t* __restrict__ mark, int64_t n, int64_t n_read,
                                                    const uint32_t* __restrict__ odeg,
                                                    unsigned long long* __restrict__ vis,
                                                    unsigned long long* __restrict__ uni,
                                                    unsigned long long* __restrict__ next, int32_t* __restrict__ list,
                                                    unsigned long long* list_n, unsigned long long* sums,
                                                    int shards) {
  __shared__ unsigned long long lds[kSlots * 16];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  const int64_t nwords = (n + 63) / 64;
  unsigned long long acc[3] = {0, 0, 0};
  // (four words a step with their mark loads issued together measured the same: 0.1037 against
  // 0.1016 ms for the hop at RMAT-26)
  for (int64_t w = wave; w < nwords; w += nwaves) {  // (wave-uniform)
    const int64_t row = w * 64 + lane;
    const bool marked = row < n && row < n_read && mark[row] != 0;
    const unsigned long long mk = __ballot(marked);
    unsigned long long keep = 0;
    if (mk) {
      const unsigned long long v = vis[w];
      const unsigned long long fresh = mk & ~v;
      const bool mine = (fresh >> lane) & 1ull;
      const uint32_t d = mine ? odeg[row] : 0u;
      keep = __ballot(mine && d > 0);
      if (marked) mark[row] = 0;
      if (lane == 0 && fresh) vis[w] = v | fresh;
      if (lane == 0 && keep) uni[w] |= keep;
      acc[0] += mine ? 1u : 0u;
      acc[1] += d;
      acc[2] += mine && d > 0 ? 1u : 0u;
      if (list && keep) {
        const int64_t s = wave_append(list_n, mine && d > 0);
        if (s >= 0) list[s] = int32_t(row);
      }
    }
    if (lane == 0) next[w] = keep;
  }
  block_add_sums(acc, 3, lds, sums, shards);
}

// k_upto_bu, a bottom-up hop over the plain transposed CSR (trp / tcol: row = owned dst, entries
// = global src index): only rows not yet in vis are scanned, and a row stops at its first
// in-neighbour in the frontier bitmap fb (over the whole gidx space, fb_bits bits).  A fixed-depth
// GO cannot skip reached rows (it must reach them again), which is why its kernels do not fit.
// Each lane scans its row's first kUptoLane entries alone; rows still open after that are scanned
// by the whole wave, 64 entries a step, so one long unreached row is not one lane's serial loop.
// Rows at or past n_scan have no in-edge: their next words are written as zero without a read.
constexpr int kUptoLane = 4;
__global__ __launch_bounds__(256) void k_upto_bu(const int64_t* __restrict__ trp, const int32_t* __restrict__ tcol,
                                                 int64_t n, int64_t n_scan, const uint32_t* __restrict__ fb,
                                                 int64_t fb_bits, const uint32_t* __restrict__ odeg,
                                                 unsigned long long* __restrict__ vis,
                                                 unsigned long long* __restrict__ uni,
                                                 unsigned long long* __restrict__ next, unsigned long long* sums,
                                                 int shards) {
  __shared__ unsigned long long lds[kSlots * 16];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  const int64_t nwords = (n + 63) / 64;
  auto in_front = [&](int32_t s) {
    return s >= 0 && int64_t(s) < fb_bits && ((fb[uint32_t(s) >> 5] >> (uint32_t(s) & 31u)) & 1u) != 0u;
  };
  unsigned long long acc[4] = {0, 0, 0, 0};
  for (int64_t w = wave; w < nwords; w += nwaves) {  // (wave-uniform)
    const int64_t row = w * 64 + lane;
    unsigned long long keep = 0;
    if (w * 64 < n_scan) {
      const unsigned long long v = vis[w];
      const bool open = row < n && row < n_scan && !((v >> lane) & 1ull);
      int64_t b = 0, e = 0;
      if (open) b = trp[row], e = trp[row + 1];
      // entry by entry: the rows are ordered hub-first, so the first entry is most often the hit,
      // and the kernel is bound by the entries it reads (loading a lane's four entries together
      // read 2.5x the entries and took 0.366 -> 0.465 ms at RMAT-26, profiles/upto_compare.md)
      bool found = false;
      for (int i = 0; i < kUptoLane; i++) {
        if (found || b + i >= e) continue;
        found = in_front(tcol[b + i]);
        acc[3]++;
      }
      unsigned long long pend = __ballot(!found && b + kUptoLane < e);
      while (pend) {
        const int l = __ffsll((long long)pend) - 1;
        pend &= pend - 1;
        const int64_t rb = __shfl(b, l) + kUptoLane, re = __shfl(e, l);
        bool hit = false;
        for (int64_t p = rb; p < re && !hit; p += 64) {
          const int64_t i = p + lane;
          bool h = false;
          if (i < re) {
            h = in_front(tcol[i]);
            acc[3]++;
          }
          hit = __ballot(h) != 0ull;
        }
        if (lane == l) found = hit;
      }
      const unsigned long long fresh = __ballot(found);
      const uint32_t d = found ? odeg[row] : 0u;
      keep = __ballot(found && d > 0);
      if (lane == 0 && fresh) vis[w] = v | fresh;
      if (lane == 0 && keep) uni[w] |= keep;
      acc[0] += found ? 1u : 0u;
      acc[1] += d;
      acc[2] += found && d > 0 ? 1u : 0u;
    }
    if (lane == 0) next[w] = keep;
  }
  block_add_sums(acc, 4, lds, sums, shards);
}

// ---- GO ... REVERSELY: the pull form of a reverse hop (GoQuery::hop_rev_pull) ----
// A reverse hop from the frontier F yields {u : some out-edge u -> v has v in F}.  The top-down
// form expands F's rows of the in CSR; when F is large this kernel scans the OUT CSR instead
// (orp / ocol: row = owned src u, entries = global dst index, in key order): every owned row with
// row_ok stops at its first dst whose bit is set in the frontier bitmap fb (over the whole gidx
// space, fb_bits bits).  Legal only where the in keys mirror the out keys (EdgeSpace::Rev::mirror).
// Modelled on k_upto_bu: one wave owns 64 consecutive rows and builds their next-frontier word by
// ballot (lane 0 stores it: no bitmap atomics); each lane scans its row's first kRevLane entries
// alone, rows still open are scanned by the whole wave, 64 entries a step, with a ballot exit.
// There is no vis (a fixed-depth GO reaches rows again).  ideg (a non-final hop): a found row is
// kept only with in-edges of its own, and the kept rows' in-degrees sum to the next hop's E;
// null (the final hop): every found row is kept.  n: the owned rows (next's words), n_rows <= n
// the rows the CSR has.  sums (zeroed by the caller with their shards; block_add_sums):
// [0] rows found, [1] in-degree sum of the kept, [2] rows kept (next's population), [3] entries
// read, [4] rows scanned (row_ok and an out-edge).
constexpr int kRevLane = 4;
__global__ __launch_bounds__(256) void k_rev_pull(const int64_t* __restrict__ orp, const int32_t* __restrict__ ocol,
                                                  const uint8_t* __restrict__ row_ok, int64_t n_rows, int64_t n,
                                                  const uint32_t* __restrict__ fb, int64_t fb_bits,
                                                  const uint32_t* __restrict__ ideg,
                                                  unsigned long long* __restrict__ next, unsigned long long* sums,
                                                  int shards) {
  __shared__ unsigned long long lds[kSlots * 16];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  const int64_t nwords = (n + 63) / 64;
  auto in_front = [&](int32_t d) {
    return d >= 0 && int64_t(d) < fb_bits && ((fb[uint32_t(d) >> 5] >> (uint32_t(d) & 31u)) & 1u) != 0u;
  };
  unsigned long long acc[5] = {0, 0, 0, 0, 0};
  for (int64_t w = wave; w < nwords; w += nwaves) {  // (wave-uniform)
    const int64_t row = w * 64 + lane;
    unsigned long long keep = 0;
    if (w * 64 < n_rows) {
      const bool open = row < n_rows && (!row_ok || row_ok[row] != 0);
      int64_t b = 0, e = 0;
      if (open) b = orp[row], e = orp[row + 1];
      acc[4] += b < e ? 1u : 0u;
      bool found = false;
      for (int i = 0; i < kRevLane; i++) {
        if (found || b + i >= e) continue;
        found = in_front(ocol[b + i]);
        acc[3]++;
      }
      unsigned long long pend = __ballot(!found && b + kRevLane < e);
      while (pend) {
        const int l = __ffsll((long long)pend) - 1;
        pend &= pend - 1;
        const int64_t rb = __shfl(b, l) + kRevLane, re = __shfl(e, l);
        bool hit = false;
        for (int64_t p = rb; p < re && !hit; p += 64) {
          const int64_t i = p + lane;
          bool h = false;
          if (i < re) {
            h = in_front(ocol[i]);
            acc[3]++;
          }
          hit = __ballot(h) != 0ull;
        }
        if (lane == l) found = hit;
      }
      const uint32_t d = found && ideg ? ideg[row] : 0u;
      const bool kept = found && (!ideg || d > 0);
      keep = __ballot(kept);
      acc[0] += found ? 1u : 0u;
      acc[1] += d;
      acc[2] += kept ? 1u : 0u;
    }
    if (lane == 0) next[w] = keep;
  }
  block_add_sums(acc, 5, lds, sums, shards);
}

// deg[v] = the row's entries, 0 where row_ok == 0; stats[0] += their sum, stats[1] = their maximum
__global__ __launch_bounds__(256) void k_row_deg(const int64_t* __restrict__ rp, const uint8_t* __restrict__ row_ok,
                                                 int64_t n, uint32_t* __restrict__ deg, unsigned long long* stats) {
  unsigned long long sum = 0, mx = 0;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
    const unsigned long long d = row_ok && !row_ok[v] ? 0ull : (unsigned long long)(rp[v + 1] - rp[v]);
    deg[v] = uint32_t(d);
    sum += d;
    mx = max(mx, d);
  }
  sum = wave_sum_u64(sum);
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, o));
  if ((threadIdx.x & 63) == 0) {
    if (sum) atomicAdd(stats, sum);
    if (mx) atomicMax(stats + 1, mx);
  }
}

// Do the in keys mirror the out keys (one rank: local row = gidx)?  One 16-lane group per in
// entry e of a row_ok in row v -- the key (v, rank, u) -- looks (rank, v) up in out row u with
// k_fetch_edge's group lookup; miss counts the entries without their out entry (an out row that
// is not row_ok holds none).  Both CSRs keep one entry per (src, rank, dst), so with equal entry
// counts over row_ok rows no miss means a bijection.
__global__ __launch_bounds__(256) void k_mirror_check(const int64_t* __restrict__ irp, const int32_t* __restrict__ icol,
                                                      const int64_t* __restrict__ irank,
                                                      const uint8_t* __restrict__ irow_ok, int64_t n_in_rows,
                                                      int64_t nnz, const int64_t* __restrict__ orp,
                                                      const uint8_t* __restrict__ orow_ok, int64_t n_out_rows,
                                                      EdgeRows out, unsigned long long* miss) {
  const int lane = threadIdx.x & (kWave - 1), sub = lane & (kLookupGroup - 1);
  const int64_t groups = int64_t(gridDim.x) * (256 / kLookupGroup);
  const int64_t g0 = (int64_t(blockIdx.x) * 256 + threadIdx.x) / kLookupGroup;
  const int64_t rounds = (nnz + groups - 1) / groups;
  unsigned long long scanned = 0, probed = 0, missed = 0;
  for (int64_t r = 0; r < rounds; r++) {  // (the same trip count in every lane: the lookup's ballots)
    const int64_t e = r * groups + g0;
    int64_t beg = 0, end = 0, rk = 0, dv = 0;
    int32_t dg = -1;
    bool key = false;
    if (e < nnz) {
      // the entry's row: the last v with irp[v] <= e
      int64_t l = 0, h = n_in_rows;
      while (h - l > 1) {
        const int64_t m = l + ((h - l) >> 1);
        if (irp[m] <= e) l = m;
        else h = m;
      }
      const int64_t v = l;
      key = !irow_ok || irow_ok[v] != 0;
      if (key) {
        const int64_t u = icol[e];
        rk = irank ? irank[e] : 0;
        dv = out.vid_of[v];
        dg = int32_t(v);
        if (u >= 0 && u < n_out_rows && (!orow_ok || orow_ok[u] != 0) && (out.erank || rk == 0))
          beg = orp[u], end = orp[u + 1];
      }
    }
    const int64_t found = group_find_edge(out, beg, end, rk, dv, dg, scanned, probed);
    missed += key && sub == 0 && found < 0;
  }
  missed = wave_sum_u64(missed);
  if (lane == 0 && missed) atomicAdd(miss, missed);
}

// ------------------------------------------------------------------------------------------
// host drivers
// ------------------------------------------------------------------------------------------
// one lane a row, at most upto_grid blocks adding their sums into the caller's shards (RMAT-26,
// UPTO 3 query: 1024 blocks 0.985 ms, 2048 / 4096 / 8192 0.799, 16384 0.925; 4096 unsharded 0.842)
static int row_grid(Ctx& c, int64_t n_own) {
  return grid_cap((n_own + 63) / 64 * 64, 256, int(std::max<int64_t>(1, c.opt("upto_grid", 4096))));
}
void launch_upto_claim(Ctx& c, uint8_t* mark, int64_t n_own, int64_t n_read, const uint32_t* odeg,
                       unsigned long long* vis, unsigned long long* uni, unsigned long long* next, int32_t* list,
                       unsigned long long* list_n, unsigned long long* sums, int shards) {
  k_upto_claim<<<row_grid(c, n_own), 256, 0, c.stream>>>(mark, n_own, n_read, odeg, vis, uni, next, list, list_n, sums,
                                                         shards);
}
void launch_upto_bu(Ctx& c, const EdgeSpace& es, int64_t n_own, int64_t n_scan, const uint32_t* fb,
                    const uint32_t* odeg, unsigned long long* vis, unsigned long long* uni, unsigned long long* next,
                    unsigned long long* sums, int shards) {
  k_upto_bu<<<row_grid(c, n_own), 256, 0, c.stream>>>(es.tr.row_ptr.as<int64_t>(), es.tr.col.as<int32_t>(),
                                                      std::min<int64_t>(n_own, es.tr.n_rows), n_scan, fb, c.n_global,
                                                      odeg, vis, uni, next, sums, shards);
}
void launch_rev_pull(Ctx& c, const EdgeSpace& es, int64_t rows, int64_t n_own, const uint32_t* fb,
                     const uint32_t* ideg, unsigned long long* next, unsigned long long* sums, int shards) {
  k_rev_pull<<<row_grid(c, n_own), 256, 0, c.stream>>>(es.out.row_ptr.as<int64_t>(), es.out.col.as<int32_t>(),
                                                       es.out.row_ok.as<uint8_t>(), rows, n_own, fb, c.n_global, ideg,
                                                       next, sums, shards);
}

// once per snapshot (collective): the out-edges summed over ranks, the largest out-degree and
// the prefix sums of the kTopDeg largest out-degrees over ranks, so that every rank takes the
// same direction decisions and a GO from a few starts knows its first hop's direction before
// it runs
constexpr int64_t kTopDeg = 4096;
// deg: this rank's u32 degrees of its n_own rows (null: no degree array, the prefix sums stay
// unknown); mine: its (entry count, largest degree, flag).  Out: the kTopDeg prefix sums and the
// entry count, the largest degree (-1: unknown on some rank) and the flags' sum over ranks.
static void gather_degree_stats(Ctx& c, const uint32_t* deg, std::array<int64_t, 3> mine, std::vector<int64_t>& top_deg,
                                int64_t& nnz_all, int64_t& max_all, int64_t& flag_all) {
  const size_t G = size_t(c.world);
  const int64_t n_own = c.owned_hi() - c.owned_lo();
  // this rank's kTopDeg largest degrees (0-padded), descending
  DevBuf top;
  top.alloc(size_t(kTopDeg) * 4 + 24);
  NBG_HIP(hipMemsetAsync(top.p, 0, size_t(kTopDeg) * 4, c.stream));
  if (deg && n_own > 0) {
    DevBuf srt;
    srt.alloc(size_t(n_own) * 4);
    size_t tb = 0;
    NBG_HIP(rocprim::radix_sort_keys_desc(nullptr, tb, deg, srt.as<uint32_t>(), size_t(n_own), 0, 32, c.stream));
    c.ws_tmp.ensure(tb);
    NBG_HIP(rocprim::radix_sort_keys_desc(c.ws_tmp.p, tb, deg, srt.as<uint32_t>(), size_t(n_own), 0, 32, c.stream));
    NBG_HIP(hipMemcpyAsync(top.p, srt.p, size_t(std::min(n_own, kTopDeg)) * 4, hipMemcpyDeviceToDevice, c.stream));
  }
  const size_t row = size_t(kTopDeg) * 4 + 24;  // the degrees, then (nnz, largest degree, flag)
  NBG_HIP(hipMemcpyAsync(top.as<uint8_t>() + size_t(kTopDeg) * 4, mine.data(), 24, hipMemcpyHostToDevice, c.stream));
  std::vector<uint8_t> all(row * G);
  DevBuf da;
  da.alloc(row * G);
  comm_allgather_bytes(c, top.p, row, da.p);
  NBG_HIP(hipMemcpyAsync(all.data(), da.p, row * G, hipMemcpyDeviceToHost, c.stream));
  host_sync(c);
  int64_t nnz = 0, mx = 0, fl = 0;
  std::vector<uint32_t> degs;
  for (size_t r = 0; r < G; r++) {
    const uint8_t* b = all.data() + r * row;
    int64_t v[3];
    memcpy(v, b + size_t(kTopDeg) * 4, 24);
    nnz += v[0];
    mx = v[1] < 0 || mx < 0 ? -1 : std::max(mx, v[1]);
    fl += v[2];
    const uint32_t* d = reinterpret_cast<const uint32_t*>(b);
    degs.insert(degs.end(), d, d + kTopDeg);
  }
  std::sort(degs.begin(), degs.end(), std::greater<uint32_t>());
  top_deg.assign(size_t(kTopDeg) + 1, 0);
  if (deg)
    for (int64_t k = 0; k < kTopDeg; k++) top_deg[size_t(k) + 1] = top_deg[size_t(k)] + int64_t(degs[size_t(k)]);
  else
    top_deg.clear();  // no degree array: unknown
  nnz_all = nnz;
  max_all = mx;
  flag_all = fl;
}
void global_degree_stats(Ctx& c, EdgeSpace& es) {
  int64_t flag = 0;
  gather_degree_stats(c, es.odeg.as<uint32_t>(), {es.out.nnz, es.max_odeg, 0}, es.top_deg, es.out_nnz_global,
                      es.max_odeg_global, flag);
}

// GO ... REVERSELY: the in-degrees of the owned rows (0 where in.row_ok == 0, padded to whole
// 128-row tiles like odeg), their statistics over ranks, and the mirror state every rank agrees
// on: known true when no rank's tuples of the type came from KV pairs (gen_rmat writes an in
// tuple per out tuple), else unknown.  Collective on several ranks.
void ensure_rev(Ctx& c, EdgeSpace& es) {
  if (es.rev.built) return;
  EdgeSpace::Rev& rv = es.rev;
  const int64_t n_own = c.owned_hi() - c.owned_lo();
  const int64_t n_rows = std::min<int64_t>(n_own, es.in.n_rows);
  const int64_t n_pad = (n_own + 127) / 128 * 128;
  rv.ideg.alloc(size_t(n_pad + 1) * 4);
  NBG_HIP(hipMemsetAsync(rv.ideg.p, 0, size_t(n_pad + 1) * 4, c.stream));
  DevBuf st;
  st.alloc(16);
  NBG_HIP(hipMemsetAsync(st.p, 0, 16, c.stream));
  if (n_rows > 0)
    k_row_deg<<<grid_cap(n_rows), 256, 0, c.stream>>>(es.in.row_ptr.as<int64_t>(), es.in.row_ok.as<uint8_t>(), n_rows,
                                                      rv.ideg.as<uint32_t>(), st.as<unsigned long long>());
  NBG_HIP(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  NBG_HIP(hipMemcpyAsync(h, st.p, 16, hipMemcpyDeviceToHost, c.stream));
  host_sync(c);
  int64_t kv_ranks = 0;
  gather_degree_stats(c, rv.ideg.as<uint32_t>(), {int64_t(h[0]), int64_t(h[1]), es.kv_loaded ? 1 : 0}, rv.top_deg,
                      rv.in_nnz_global, rv.max_ideg_global, kv_ranks);
  rv.mirror = kv_ranks == 0 ? 1 : -1;
  rv.built = true;
}

// the exact mirror check of a one-rank, non-sharded context (k_mirror_check); paid once per
// commit of the type: the answer is cached in EdgeSpace::Rev::mirror
bool check_mirror(Ctx& c, EdgeSpace& es) {
  const int64_t n = c.n_global;
  const int64_t n_in = std::min<int64_t>(n, es.in.n_rows), n_out = std::min<int64_t>(n, es.out.n_rows);
  DevBuf st, scratch;
  st.alloc(24);
  scratch.alloc(size_t(std::max<int64_t>(n_out, 1)) * 4);
  NBG_HIP(hipMemsetAsync(st.p, 0, 24, c.stream));
  if (n_out > 0)
    k_row_deg<<<grid_cap(n_out), 256, 0, c.stream>>>(es.out.row_ptr.as<int64_t>(), es.out.row_ok.as<uint8_t>(), n_out,
                                                     scratch.as<uint32_t>(), st.as<unsigned long long>());
  if (es.in.nnz > 0 && n_in > 0) {
    EdgeRows rows{};
    rows.col = es.out.col.as<int32_t>();
    rows.col_vid = es.out.col_vid.as<int64_t>();
    rows.erank = es.out.rank.as<int64_t>();
    rows.vid_of = c.vid_of.as<int64_t>();
    rows.window = 64;
    k_mirror_check<<<grid_cap(es.in.nnz, 256 / kLookupGroup), 256, 0, c.stream>>>(
        es.in.row_ptr.as<int64_t>(), es.in.col.as<int32_t>(), es.in.rank.as<int64_t>(), es.in.row_ok.as<uint8_t>(), n_in,
        es.in.nnz, es.out.row_ptr.as<int64_t>(), es.out.row_ok.as<uint8_t>(), n_out, rows,
        st.as<unsigned long long>() + 2);
  }
  NBG_HIP(hipGetLastError());
  unsigned long long h[3] = {0, 0, 0};
  NBG_HIP(hipMemcpyAsync(h, st.p, 24, hipMemcpyDeviceToHost, c.stream));
  host_sync(c);
  return int64_t(h[0]) == es.rev.in_nnz_global && h[2] == 0;
}

}  // namespace nbg
