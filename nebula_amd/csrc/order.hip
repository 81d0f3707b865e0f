// order.hip -- ORDER BY on a result table (nbg_order_by): a stable LSD radix sort in HBM.
//
// Replaces OrderByExecutor::execute / beforeExecute's std::sort over the piped rows
// (src/graph/OrderByExecutor.cpp:70-136).  DESIGN.md section 3 "ORDER BY" has the byte model.
//
// Every factor becomes one or more 64-bit keys (order_keys.h); the keys are sorted from the least
// to the most significant, 8 bits a pass, with a uint32 row index as the payload.  Per key one
// pass builds its eight 256-bin digit histograms; the host reads them (the one host wait of the
// key) and runs only the digits whose histogram has more than one non-empty bin.  A pass is
//   k_ord_count    per-tile digit counts, digit-major                       (reads the keys)
//   exclusive scan of the counts (rocprim)
//   k_ord_scatter  ranks every row inside its tile (wave ballots + per-wave counters in LDS),
//                  orders the tile in LDS and writes each digit's run contiguously
// and every dependency between workgroups is one of these kernel boundaries: no workgroup waits
// for another one.  k_ord_gather then permutes the output columns by the final index (the gather,
// the upload of a host table and the hand-out live in row_gather.h, shared with setops.hip).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "engine.h"
#include "order_keys.h"
#include "query_common.h"
#include "row_gather.h"
#include "rows.h"

namespace nbg {
namespace {

constexpr int kOrdWaves = kOrdThreads / 64;
constexpr int kHistWords = 8 * 256;
constexpr int kHistRounds = 4;
constexpr int64_t kSmallTileRows = int64_t(1) << 18;  // up to here 1024-row tiles, 4096 above
constexpr int64_t kMaxStrFactorLen = 256;

enum KeyKind : int32_t { KK_ENCODED = 0, KK_INT, KK_DOUBLE, KK_BOOL, KK_STRLEN, KK_STRCHUNK, KK_U32 };

// where element i's key comes from: encoded keys (KK_ENCODED), or a column read through the
// current index (idx == nullptr: row i) and encoded on the fly
struct KeySrc {
  const void* data;     // keys, column values or string bytes
  const int64_t* off;   // STRING offsets
  const uint32_t* idx;  // row of element i
  int32_t kind, desc;
  int64_t chunk;
};

__device__ __forceinline__ uint64_t load_key(const KeySrc& s, int64_t i) {
  if (s.kind == KK_ENCODED) return static_cast<const uint64_t*>(s.data)[i];
  const int64_t r = s.idx ? int64_t(s.idx[i]) : i;
  uint64_t k;
  switch (s.kind) {
    case KK_INT: k = okey::enc_int(static_cast<const int64_t*>(s.data)[r]); break;
    case KK_DOUBLE: k = okey::enc_double(static_cast<const double*>(s.data)[r]); break;
    case KK_BOOL: k = okey::enc_bool(static_cast<const uint8_t*>(s.data)[r]); break;
    case KK_STRLEN: k = okey::enc_str_len(s.off[r + 1] - s.off[r]); break;
    case KK_U32: k = static_cast<const uint32_t*>(s.data)[r]; break;  // GROUP BY's group ids
    default:
      k = okey::enc_str_chunk(static_cast<const uint8_t*>(s.data) + s.off[r], s.off[r + 1] - s.off[r], s.chunk);
  }
  return okey::direction(k, s.desc);
}

// One add per wave where every lane holds the same digit (the high digits of small vids, a
// constant column): 64 LDS atomics on one address would serialise.  `k` of a lane past the end
// is lane 0's key (lane 0 of a wave inside the loop is always valid), so the tail joins the vote.
__device__ __forceinline__ void wave_hist_add(uint32_t* h, uint32_t dig, bool same, bool valid, uint32_t nvalid) {
  if (same) {
    if ((threadIdx.x & 63) == 0) atomicAdd(&h[dig], nvalid);
  } else if (valid) {
    atomicAdd(&h[dig], 1u);
  }
}

// all eight digit histograms of a key in one pass over it; with key_out the encoded keys are
// written too (keys gathered through an index, string chunks).  KK_STRLEN: *max_len = the
// longest value.  hist: [digit 0..7][256] uint32 (n < 2^32).
__global__ __launch_bounds__(kOrdThreads) void k_ord_hist(KeySrc s, int64_t n, uint64_t* __restrict__ key_out,
                                                          uint32_t* __restrict__ hist,
                                                          unsigned long long* __restrict__ max_len) {
  __shared__ uint32_t h[kHistWords];
  __shared__ unsigned long long smax;
  for (int j = threadIdx.x; j < kHistWords; j += kOrdThreads) h[j] = 0;
  if (threadIdx.x == 0) smax = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  unsigned long long mx = 0;
  // a wave takes kHistRounds x 64 consecutive rows a step, every load issued before the first
  // histogram add (the adds are LDS atomics: little else hides the loads' latency)
  const int64_t stride = int64_t(gridDim.x) * kOrdThreads * kHistRounds;
  for (int64_t wb = (int64_t(blockIdx.x) * kOrdWaves + threadIdx.x / 64) * (64 * kHistRounds); wb < n; wb += stride) {
    uint64_t kk[kHistRounds];
#pragma unroll
    for (int r = 0; r < kHistRounds; r++) {
      const int64_t i = wb + r * 64 + lane;
      kk[r] = i < n ? load_key(s, i) : 0;
    }
#pragma unroll
    for (int r = 0; r < kHistRounds; r++) {
      const int64_t base = wb + r * 64;
      if (base >= n) break;  // wave-uniform
      const int64_t i = base + lane;
      const bool valid = i < n;
      uint64_t k = kk[r];
      if (valid && key_out) key_out[i] = k;
      if (valid && s.kind == KK_STRLEN) mx = max(mx, (unsigned long long)okey::direction(k, s.desc));
      const uint64_t k0 = __shfl(k, 0);
      if (!valid) k = k0;
      const uint64_t diff = k ^ k0;
      const uint32_t nvalid = uint32_t(min(int64_t(64), n - base));
#pragma unroll
      for (int d = 0; d < 8; d++) {
        const bool same = __all(((diff >> (8 * d)) & 255) == 0);
        wave_hist_add(h + d * 256, uint32_t(k >> (8 * d)) & 255u, same, valid, nvalid);
      }
    }
  }
  if (s.kind == KK_STRLEN && mx) atomicMax(&smax, mx);
  __syncthreads();
  for (int j = threadIdx.x; j < kHistWords; j += kOrdThreads)
    if (h[j]) atomicAdd(&hist[j], h[j]);
  if (threadIdx.x == 0 && smax) atomicMax(max_len, smax);
}

// Tile layout of a pass (count and scatter agree on it): tile t holds rows [t * 256 * ITEMS,
// (t + 1) * 256 * ITEMS); wave w of the workgroup takes the w-th quarter of them, 64 consecutive
// rows a round, so the input order inside a tile is (wave, round, lane).
//
// counts[d * ntiles + t] = rows of tile t whose digit is d (digit-major: the exclusive scan of
// the whole array is then each (digit, tile) run's first output position)
template <int ITEMS>
__global__ __launch_bounds__(kOrdThreads) void k_ord_count(KeySrc s, int64_t n, int shift,
                                                           uint32_t* __restrict__ counts, uint32_t ntiles) {
  __shared__ uint32_t h[kOrdWaves][256];
  for (int w = 0; w < kOrdWaves; w++) h[w][threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  const int64_t wbase = (int64_t(blockIdx.x) * kOrdWaves + wave) * (64 * ITEMS);
  for (int r = 0; r < ITEMS; r++) {
    const int64_t base = wbase + r * 64;
    if (base >= n) break;  // wave-uniform
    const int64_t i = base + lane;
    const bool valid = i < n;
    uint64_t k = valid ? load_key(s, i) : 0;
    const uint64_t k0 = __shfl(k, 0);
    if (!valid) k = k0;
    const uint32_t dig = uint32_t(k >> shift) & 255u;
    const bool same = __all(dig == (uint32_t(k0 >> shift) & 255u));
    wave_hist_add(h[wave], dig, same, valid, uint32_t(min(int64_t(64), n - base)));
  }
  __syncthreads();
  uint32_t c = 0;
  for (int w = 0; w < kOrdWaves; w++) c += h[w][threadIdx.x];
  counts[size_t(threadIdx.x) * ntiles + blockIdx.x] = c;
}

// One pass: row i of the tile goes to scanned[digit * ntiles + tile] + (rows of the tile before
// it with the same digit).  Payload: idx_in[i], or i itself (the first pass of the sort).
// key_out == nullptr: the key's last pass (only the index goes on); idx_out == nullptr: keys only.
// decode = 1: the keys-only sort's last pass writes the int64 values back (dec_int).
template <int ITEMS>
__global__ __launch_bounds__(kOrdThreads) void k_ord_scatter(KeySrc s, const uint32_t* __restrict__ idx_in, int64_t n,
                                                             int shift, const uint32_t* __restrict__ scanned,
                                                             uint32_t ntiles, uint64_t* __restrict__ key_out,
                                                             uint32_t* __restrict__ idx_out, int32_t decode,
                                                             int32_t decode_desc) {
  constexpr int TILE = kOrdThreads * ITEMS;
  __shared__ uint64_t sk[TILE];
  __shared__ uint32_t si[TILE];
  __shared__ uint32_t wcnt[kOrdWaves][256];
  __shared__ uint32_t texcl[256];  // first tile-local position of each digit
  __shared__ uint32_t goff[256];   // its first global position minus texcl
  __shared__ uint32_t wsum[kOrdWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid / 64;
  for (int w = 0; w < kOrdWaves; w++) wcnt[w][tid] = 0;
  __syncthreads();

  const int64_t tbase = int64_t(blockIdx.x) * TILE;
  const int64_t wbase = tbase + int64_t(wave) * (64 * ITEMS);
  const uint64_t lt = (uint64_t(1) << lane) - 1;
  uint64_t key[ITEMS];
  uint32_t pay[ITEMS], lrank[ITEMS];
  // every load of the tile is issued before the ranking starts
#pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    const int64_t i = wbase + r * 64 + lane;
    const bool valid = i < n;
    key[r] = valid ? load_key(s, i) : 0;
    pay[r] = valid ? (idx_in ? idx_in[i] : uint32_t(i)) : 0;
  }
#pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    const int64_t i = wbase + r * 64 + lane;
    const bool valid = i < n;
    const uint64_t k = key[r];
    const uint32_t dig = uint32_t(k >> shift) & 255u;
    // the lanes of this round that hold the same digit (8 ballots, one per digit bit)
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (dig >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t rank = uint32_t(__popcll(peers & lt));
    // the wave's running count of the digit: every peer reads it, the first one adds the round's
    // count (a wave executes the two LDS accesses in order; the barriers keep the compiler from
    // moving them)
    const uint32_t prev = valid ? wcnt[wave][dig] : 0;
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) wcnt[wave][dig] = prev + uint32_t(__popcll(peers));
    __builtin_amdgcn_wave_barrier();
    lrank[r] = prev + rank;
  }
  __syncthreads();

  // thread d: digit d's per-wave counts -> exclusive offsets over the waves, the tile's count ->
  // an exclusive scan over the 256 digits
  {
    uint32_t total = 0;
    for (int w = 0; w < kOrdWaves; w++) {
      const uint32_t c = wcnt[w][tid];
      wcnt[w][tid] = total;
      total += c;
    }
    uint32_t v = total;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(v, o);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    uint32_t add = 0;
    for (int w = 0; w < wave; w++) add += wsum[w];
    const uint32_t excl = v - total + add;
    texcl[tid] = excl;
    goff[tid] = scanned[size_t(tid) * ntiles + blockIdx.x] - excl;
  }
  __syncthreads();

#pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    const int64_t i = wbase + r * 64 + lane;
    if (i < n) {
      const uint32_t dig = uint32_t(key[r] >> shift) & 255u;
      const uint32_t pos = texcl[dig] + wcnt[wave][dig] + lrank[r];
      sk[pos] = key[r];
      si[pos] = pay[r];
    }
  }
  __syncthreads();

  const int nv = int(min(int64_t(TILE), n - tbase));
  for (int j = tid; j < nv; j += kOrdThreads) {
    const uint64_t k = sk[j];
    const uint32_t g = goff[uint32_t(k >> shift) & 255u] + uint32_t(j);
    if (key_out) key_out[g] = decode ? uint64_t(okey::dec_int(okey::direction(k, decode_desc))) : k;
    if (idx_out) idx_out[g] = si[j];
  }
}

// the sort of one call: workspace, current index, counters
struct OrderSort {
  Ctx& c;
  const int64_t n;
  const int items;  // rows per thread of a tile (4 or 16)
  const uint32_t ntiles;
  DevBuf keys[2], idxs[2], counts, hist;
  HostBuf hist_host;
  const uint32_t* idx = nullptr;  // current order (nullptr: the input order)
  int idx_next = 0;               // the index buffer the next pass writes
  int passes = 0;

  OrderSort(Ctx& c_, int64_t n_)
      : c(c_), n(n_), items(n_ <= kSmallTileRows ? 4 : 16),
        ntiles(uint32_t((n_ + kOrdThreads * items - 1) / (kOrdThreads * items))) {
    counts.alloc(size_t(ntiles) * 256 * 4);
    hist.alloc(kHistWords * 4 + 8);
    hist_host.alloc(c.host_pool, kHistWords * 4 + 8);
  }
  void launched() { kernel_launched(c); }
  uint64_t* key_buf(int which) {
    if (!keys[which].p) keys[which].alloc(size_t(n) * 8);
    return keys[which].as<uint64_t>();
  }
  uint32_t* idx_buf(int which) {
    if (!idxs[which].p) idxs[which].alloc(size_t(n) * 4);
    return idxs[which].as<uint32_t>();
  }

  // the key's histograms on the host (the key's one host wait); returns the digits to run
  std::vector<int> histograms(const KeySrc& s, uint64_t* key_out, int64_t* max_len) {
    NBG_HIP(hipMemsetAsync(hist.p, 0, kHistWords * 4 + 8, c.stream));
    // (four workgroups a CU at most: each one ends with up to 2048 global adds)
    k_ord_hist<<<grid_for(n, kOrdThreads * kHistRounds * 4, 1024), kOrdThreads, 0, c.stream>>>(
        s, n, key_out, hist.as<uint32_t>(), reinterpret_cast<unsigned long long*>(hist.as<uint8_t>() + kHistWords * 4));
    launched();
    NBG_HIP(hipMemcpyAsync(hist_host.p, hist.p, kHistWords * 4 + 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    c.timing.host_waits++;
    const uint32_t* h = static_cast<const uint32_t*>(hist_host.p);
    if (max_len) memcpy(max_len, static_cast<const uint8_t*>(hist_host.p) + kHistWords * 4, 8);
    std::vector<int> run;
    for (int d = 0; d < 8; d++) {
      int bins = 0;
      for (int b = 0; b < 256 && bins < 2; b++) bins += h[d * 256 + b] != 0;
      if (bins > 1) run.push_back(d);  // one non-empty bin: the pass would move nothing
    }
    return run;
  }

  void pass(const KeySrc& s, int digit, uint64_t* key_out, uint32_t* idx_out, int32_t decode, int32_t decode_desc) {
    const int shift = 8 * digit;
    uint32_t* cnt = counts.as<uint32_t>();
    const size_t ncnt = size_t(ntiles) * 256;
    if (items == 4) k_ord_count<4><<<ntiles, kOrdThreads, 0, c.stream>>>(s, n, shift, cnt, ntiles);
    else k_ord_count<16><<<ntiles, kOrdThreads, 0, c.stream>>>(s, n, shift, cnt, ntiles);
    launched();
    exclusive_scan_dev<uint32_t>(c, cnt, cnt, int64_t(ncnt));
    c.timing.launches++;
    if (items == 4)
      k_ord_scatter<4><<<ntiles, kOrdThreads, 0, c.stream>>>(s, idx, n, shift, cnt, ntiles, key_out, idx_out, decode,
                                                             decode_desc);
    else
      k_ord_scatter<16><<<ntiles, kOrdThreads, 0, c.stream>>>(s, idx, n, shift, cnt, ntiles, key_out, idx_out, decode,
                                                              decode_desc);
    launched();
    passes++;
    c.timing.steps_run = passes;
  }

  // stable sort of the current order by one 64-bit key.  `direct`: the key is read from its
  // column at every use (a fixed-width column in input order); otherwise the histogram pass
  // materialises it.  Returns the longest value for KK_STRLEN.
  int64_t sort_key(KeySrc s, bool direct) {
    int64_t max_len = 0;
    s.idx = idx;
    uint64_t* mat = direct ? nullptr : key_buf(0);
    const std::vector<int> run = histograms(s, mat, s.kind == KK_STRLEN ? &max_len : nullptr);
    KeySrc cur = s;
    int kb = 1;  // the key buffer the next pass writes (materialised keys sit in buffer 0)
    if (!direct) {
      cur = KeySrc{mat, nullptr, nullptr, KK_ENCODED, 0, 0};
    } else {
      kb = 0;
    }
    for (size_t p = 0; p < run.size(); p++) {
      const bool last = p + 1 == run.size();
      uint64_t* ko = last ? nullptr : key_buf(kb);
      uint32_t* io = idx_buf(idx_next);
      pass(cur, run[p], ko, io, 0, 0);
      idx = io;
      idx_next ^= 1;
      if (!last) {
        cur = KeySrc{ko, nullptr, nullptr, KK_ENCODED, 0, 0};
        kb ^= 1;
      }
    }
    return max_len;
  }

  // keys only (a one-column int table ordered by that column): no index; the last pass decodes
  // into `out`.  Returns false when no pass ran (the column is constant: out is not written).
  bool sort_keys_only(KeySrc s, uint64_t* out) {
    const std::vector<int> run = histograms(s, nullptr, nullptr);
    KeySrc cur = s;
    int kb = 0;
    for (size_t p = 0; p < run.size(); p++) {
      const bool last = p + 1 == run.size();
      uint64_t* ko = last ? out : key_buf(kb);
      pass(cur, run[p], ko, nullptr, last ? 1 : 0, s.desc);
      cur = KeySrc{ko, nullptr, nullptr, KK_ENCODED, 0, 0};
      kb ^= 1;
    }
    return !run.empty();
  }
};

int32_t order_by_impl(Ctx& c, const nbg_rows& in, const std::vector<std::pair<int32_t, int32_t>>& factors,
                      bool keep_on_device, nbg_rows* out) {
  const int64_t n = in.n_rows;
  const size_t ncols = size_t(in.n_cols);
  NBG_HIP(hipEventRecord(c.ev[0], c.stream));

  // ---- the input columns in HBM (a host table is uploaded; a device table is read in place) ----
  std::vector<DevBuf> up;
  const std::vector<InCol> cols = upload_table(c, in, up, "order_by");

  auto h = std::make_unique<HostRows>();
  for (size_t k = 0; k < ncols; k++) h->types.push_back(cols[k].type);
  std::vector<DevBuf> out_off(ncols);  // STRING columns' new offsets
  h->dev.resize(ncols);

  if (n > 0) {
    OrderSort srt(c, n);
    const bool keys_only = ncols == 1 && factors.size() == 1 && int_like(cols[0].type);
    if (keys_only) {
      // ---- one int column ordered by itself: sort the keys, decode them into the output ----
      h->dev[0].alloc(size_t(n) * 8);
      const KeySrc s{cols[0].data, nullptr, nullptr, KK_INT, factors[0].second, 0};
      if (!srt.sort_keys_only(s, h->dev[0].as<uint64_t>()))
        NBG_HIP(hipMemcpyAsync(h->dev[0].p, cols[0].data, size_t(n) * 8, hipMemcpyDeviceToDevice, c.stream));
    } else {
      // ---- LSD over the factors: the last one first ----
      for (size_t f = factors.size(); f-- > 0;) {
        const InCol& ic = cols[size_t(factors[f].first)];
        const int32_t desc = factors[f].second;
        if (ic.type == NBG_T_STRING) {
          // least significant first: the length, then the chunks from the last to the first
          const int64_t max_len = srt.sort_key(KeySrc{ic.data, ic.off, nullptr, KK_STRLEN, desc, 0}, false);
          if (max_len > kMaxStrFactorLen)
            throw Error(NBG_E_UNSUPPORTED, "order_by: a STRING factor's values may be at most 256 bytes, found " +
                                               std::to_string(max_len));
          for (int64_t ch = okey::str_chunks(max_len); ch-- > 0;)
            srt.sort_key(KeySrc{ic.data, ic.off, nullptr, KK_STRCHUNK, desc, ch}, false);
        } else {
          const int32_t kind = ic.type == NBG_T_DOUBLE ? KK_DOUBLE : ic.type == NBG_T_BOOL ? KK_BOOL : KK_INT;
          srt.sort_key(KeySrc{ic.data, nullptr, nullptr, kind, desc, 0}, srt.idx == nullptr);
        }
      }
      // ---- the output columns, permuted by the final index ----
      gather_rows(c, cols, srt.idx, n, h->dev, out_off);
    }
  } else {
    for (size_t k = 0; k < ncols; k++) h->dev[k].alloc(8);
  }
  NBG_HIP(hipEventRecord(c.ev[1], c.stream));
  c.total_pending = true;

  // ---- hand out: device blocks, or host copies through the pinned result blocks ----
  std::vector<int64_t> str_bytes(ncols);
  for (size_t k = 0; k < ncols; k++) str_bytes[k] = cols[k].str_bytes;
  hand_out_rows(c, std::move(h), out_off, str_bytes, n, keep_on_device, out);
  out->edges_scanned = in.edges_scanned;
  return NBG_OK;
}

}  // namespace

// GROUP BY's ordered path (group.hip): the rows in a stable order by their 32-bit group id, with
// the sort above (one key, so one host wait; the digits no id differs in are skipped).  Returns
// false when no pass ran: every id is the same and the input order is the answer.
bool order_rows_by_u32(Ctx& c, const uint32_t* keys, int64_t n, DevBuf& idx) {
  OrderSort srt(c, n);
  srt.sort_key(KeySrc{keys, nullptr, nullptr, KK_U32, 0, 0}, true);
  if (!srt.idx) return false;
  idx = std::move(srt.idxs[srt.idx_next ^ 1]);  // the buffer the last pass wrote
  return true;
}

int32_t order_by_run(Ctx& c, const nbg_rows& in, const int32_t* fcols, const int32_t* fdesc, size_t n_factors,
                     int32_t keep_on_device, nbg_rows* out) {
  check_plain_table(in, "order_by");
  // factor 0 is the most significant; a column's later repeats decide nothing
  std::vector<std::pair<int32_t, int32_t>> factors;
  for (size_t f = 0; f < n_factors; f++) {
    if (fcols[f] < 0 || fcols[f] >= in.n_cols) throw Error(NBG_E_INVALID_ARG, "order_by: column index out of range");
    if (fdesc[f] != 0 && fdesc[f] != 1) throw Error(NBG_E_INVALID_ARG, "order_by: desc must be 0 or 1");
    bool seen = false;
    for (auto& p : factors) seen |= p.first == fcols[f];
    if (!seen) factors.emplace_back(fcols[f], fdesc[f]);
  }
  if (uint64_t(in.n_rows) >= (uint64_t(1) << 32)) throw Error(NBG_E_UNSUPPORTED, "order_by: 2^32 rows or more");

  PoolScope pool_scope(query_pool(c));
  c.timing = Timing{};
  timing_reset(c);
  c.total_pending = false;
  try {
    return order_by_impl(c, in, factors, keep_on_device != 0, out);
  } catch (...) {
    // no launch or copy may still use a block this call frees on the way out
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
}

}  // namespace nbg
