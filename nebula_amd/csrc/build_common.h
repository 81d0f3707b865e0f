// build_common.h -- what the snapshot build's translation units share (snapshot.hip: staging, the
// vertex map and the finalize / commit drivers; csr_build.hip: the CSR and transpose builders;
// rmat_stream.hip: the streamed RMAT build): launch sizing, the rocprim sort / unique wrappers,
// device scalars read on the host, small collectives, and the entry points that cross files.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <array>
#include <vector>

#include "device_common.h"
#include "engine.h"
#include "query_common.h"

namespace nbg {

template <typename T>
__global__ void k_fill(T* p, T v, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    p[i] = v;
}
static int grid_for(int64_t n, int block = 256) {
  int64_t g = (n + block - 1) / block;
  return int(std::max<int64_t>(1, std::min<int64_t>(g, 2048 * 8)));
}
template <typename T>
static void fill(Ctx& c, T* p, T v, int64_t n) {
  if (n <= 0) return;
  k_fill<T><<<grid_for(n), 256, 0, c.stream>>>(p, v, n);
}

// grows b to at least `need` bytes keeping its contents: exactly `need` (the caller sized it), or
// 1.25x the old size when that is larger (amortised appends of many small batches)
static void grow_copy(Ctx& c, DevBuf& b, size_t need, bool exact = false) {
  if (need <= b.bytes) return;
  DevBuf nb;
  nb.alloc(exact ? need : std::max(need, b.bytes + b.bytes / 4));
  if (b.bytes) NBG_HIP(hipMemcpyAsync(nb.p, b.p, b.bytes, hipMemcpyDeviceToDevice, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  b = std::move(nb);
}

// bits that index x values: the smallest b >= 1 with 2^b >= x
inline int bits_for(int64_t x) {
  int b = 1;
  while ((int64_t(1) << b) < std::max<int64_t>(x, 2)) b++;
  return b;
}
// the smallest floor * 2^k >= x
inline int64_t pow2_at_least(int64_t x, int64_t floor) {
  int64_t cap = floor;
  while (cap < x) cap <<= 1;
  return cap;
}

// N device words of type T that the host initialises and reads back: read() is the copy and the
// one stream wait of its site
template <typename T, int N>
struct DevWords {
  DevBuf b;
  std::array<T, N> init{};  // set()'s source: pageable, so it lives as long as the copy may run
  DevWords() { b.alloc(sizeof(T) * N); }
  template <typename U = T>
  U* dev() const {
    static_assert(sizeof(U) == sizeof(T), "same-width view only");
    return b.as<U>();
  }
  void zero(Ctx& c) { NBG_HIP(hipMemsetAsync(b.p, 0, sizeof(T) * N, c.stream)); }
  void set(Ctx& c, const std::array<T, N>& v) {
    init = v;
    NBG_HIP(hipMemcpyAsync(b.p, init.data(), sizeof(T) * N, hipMemcpyHostToDevice, c.stream));
  }
  std::array<T, N> read(Ctx& c) const {
    std::array<T, N> h;
    NBG_HIP(hipMemcpyAsync(h.data(), b.p, sizeof(T) * N, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    return h;
  }
};

template <typename K, typename V>
static void radix_pairs(Ctx& c, K* kin, K* kout, V* vin, V* vout, int64_t n, int bits) {
  size_t tb = 0;
  NBG_HIP(rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, size_t(n), 0, bits, c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::radix_sort_pairs(c.ws_tmp.p, tb, kin, kout, vin, vout, size_t(n), 0, bits, c.stream));
}
template <typename K>
static void radix_keys(Ctx& c, K* kin, K* kout, int64_t n, int bits) {
  size_t tb = 0;
  NBG_HIP(rocprim::radix_sort_keys(nullptr, tb, kin, kout, size_t(n), 0, bits, c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::radix_sort_keys(c.ws_tmp.p, tb, kin, kout, size_t(n), 0, bits, c.stream));
}
// unique of a sorted array; returns count
template <typename T>
static int64_t unique_sorted(Ctx& c, T* in, T* out, int64_t n) {
  DevWords<uint64_t, 1> cnt;
  size_t tb = 0;
  NBG_HIP(rocprim::unique(nullptr, tb, in, out, cnt.dev(), size_t(n), rocprim::equal_to<T>(), c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::unique(c.ws_tmp.p, tb, in, out, cnt.dev(), size_t(n), rocprim::equal_to<T>(), c.stream));
  return int64_t(cnt.read(c)[0]);
}

// mine[0, k) of every rank, rank-major (world * k values; one stream wait)
inline std::vector<int64_t> allgather_i64(Ctx& c, const std::vector<int64_t>& mine) {
  const size_t k = mine.size(), G = size_t(c.world);
  DevBuf dm, da;
  dm.alloc(k * 8);
  da.alloc(G * k * 8);
  NBG_HIP(hipMemcpyAsync(dm.p, mine.data(), k * 8, hipMemcpyHostToDevice, c.stream));
  comm_allgather_bytes(c, dm.p, k * 8, da.p);
  std::vector<int64_t> all(G * k);
  NBG_HIP(hipMemcpyAsync(all.data(), da.p, G * k * 8, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  return all;
}
inline std::vector<int64_t> allgather_i64(Ctx& c, int64_t mine) {
  return allgather_i64(c, std::vector<int64_t>(1, mine));
}
// every rank's set (sizes[r] entries of `width` bytes; this rank's: mine[0, n)) end to end in rank
// order.  The sets travel padded to the longest (an allgather of equal blocks) and are compacted;
// compact = false returns them as received, rank r's at r * the longest size.
inline DevBuf allgather_padded(Ctx& c, const DevBuf& mine, int64_t n, const std::vector<int64_t>& sizes,
                               int64_t width, bool compact = true) {
  const size_t w = size_t(width);
  const int64_t mx = *std::max_element(sizes.begin(), sizes.end());
  DevBuf sendb, recvb, all;
  sendb.alloc(size_t(std::max<int64_t>(mx, 1)) * w);
  recvb.alloc(size_t(std::max<int64_t>(mx, 1)) * w * size_t(c.world));
  if (n) NBG_HIP(hipMemcpyAsync(sendb.p, mine.p, size_t(n) * w, hipMemcpyDeviceToDevice, c.stream));
  comm_allgather_bytes(c, sendb.p, size_t(mx) * w, recvb.p);
  if (!compact) return recvb;
  int64_t tot = 0;
  for (auto s : sizes) tot += s;
  all.alloc(size_t(std::max<int64_t>(tot, 1)) * w);
  int64_t at = 0;
  for (int r = 0; r < c.world; r++) {
    if (sizes[size_t(r)])
      NBG_HIP(hipMemcpyAsync(all.as<uint8_t>() + size_t(at) * w, recvb.as<uint8_t>() + size_t(r) * size_t(mx) * w,
                             size_t(sizes[size_t(r)]) * w, hipMemcpyDeviceToDevice, c.stream));
    at += sizes[size_t(r)];
  }
  return all;
}

// ---- snapshot.hip: the vertex map ---------------------------------------------------------
// The vid -> gidx table (Ctx::ht_*; open addressing, INT64_MIN the empty key, so the vid
// INT64_MIN itself is kept beside the table: ht_min_gidx).  reset sizes it for n_slots_for gidx
// slots (a power of two at least twice that, at least 1024) and empties it; insert adds
// vids[0, n) as gidx base.. and notes in dmin (set to -1 by the caller) the gidx of INT64_MIN if
// it is among them; publish_min reads dmin back (the site's one stream wait).
void vid_hash_reset(Ctx& c, int64_t n_slots_for);
void vid_hash_insert(Ctx& c, const int64_t* vids, int64_t n, int64_t base, DevWords<int32_t, 1>& dmin);
void vid_hash_publish_min(Ctx& c, const DevWords<int32_t, 1>& dmin);
// bytewise order rank of every gidx (RocksDB key order of the dst bytes; holes sort anywhere)
DevBuf bytewise_ranks(Ctx& c);
// vertex numbering keys (k_class_key) of n vertices; idx (or null) indexes the degree counts
constexpr int kClassKeyBits = 36;
void class_keys(Ctx& c, const uint32_t* odeg, const uint32_t* ideg, const uint32_t* idx, int64_t n, uint64_t* key);

// ---- csr_build.hip ------------------------------------------------------------------------
// One CSR from a staging area (out = Csr() first).  consume: the staged tuples are freed; else
// ord (writable snapshots) keeps the sorted order for a later merge commit.  merge: sort only the
// tuples behind ord->n and merge them into the committed order.
void build_csr(Ctx& c, Staging& s, const std::vector<Field>& fields, bool with_props, Csr& out,
               const uint32_t* byterank, bool consume = true, EdgeSpace::Order* ord = nullptr, bool merge = false);
// the transposed CSR of es.out with its slabs, bounds and rest records (collective on several ranks)
void build_transpose(Ctx& c, EdgeSpace& es);
// es.odeg of es.out's rows (0 for rows with row_ok clear); dmax (device, or null) takes the maximum
void build_out_degrees(Ctx& c, EdgeSpace& es, const uint8_t* row_ok, unsigned int* dmax);
// {min, max} of an INT column of width 1/2/4/8 bytes (n = 0: {LLONG_MAX, LLONG_MIN}; one stream wait)
std::array<long long, 2> minmax_w(Ctx& c, const void* data, int width, int64_t n);
// row_part[i] = the hash part of vids[i]
void row_part_by_hash(Ctx& c, const int64_t* vids, int64_t n, int32_t* row_part);

// ---- rmat_stream.hip ----------------------------------------------------------------------
void finalize_rmat_stream(Ctx& c, EdgeSpace& es);

// ---- synthetic RMAT (definition shared with oracle/refcpu.cpp) --------------------
constexpr uint32_t kTA = 2448131358u;    // floor(0.57 * 2^32)
constexpr uint32_t kTAB = 3264175144u;   // floor(0.76 * 2^32)
constexpr uint32_t kTABC = 4080218931u;  // floor(0.95 * 2^32)

__device__ inline void rmat_pick(uint32_t r, uint64_t& u, uint64_t& v) {
  uint64_t bu = (r >= kTAB) ? 1 : 0;
  uint64_t bv = ((r >= kTA && r < kTAB) || r >= kTABC) ? 1 : 0;
  u = (u << 1) | bu;
  v = (v << 1) | bv;
}
__device__ inline int64_t rmat_vid(uint64_t idx, uint64_t smix) {
  const uint64_t M = (1ull << 63) - 1;
  uint64_t x = (idx + smix) & M;
  x ^= x >> 29;
  x = (x * 0xBF58476D1CE4E5B9ull) & M;
  x ^= x >> 32;
  x = (x * 0x94D049BB133111EBull) & M;
  x ^= x >> 29;
  return int64_t(x);
}

// sample i of the generator: (u, v) in the index space [0, 2^scale)
__device__ inline void rmat_sample(uint64_t i, int32_t scale, uint64_t seed, uint64_t& u, uint64_t& v) {
  u = 0;
  v = 0;
  for (int32_t l = 0; l < scale; l += 2) {
    uint64_t h = splitmix64(seed ^ (0xD6E8FEB86659FD93ull * (i + 1)) ^ (0xA0761D6478BD642Full * uint64_t(l + 1)));
    rmat_pick(uint32_t(h >> 32), u, v);
    if (l + 1 < scale) rmat_pick(uint32_t(h), u, v);
  }
}
// the edge prop of sample (s, d): follow.weight (same value for every duplicate of the pair)
__device__ inline int64_t rmat_weight(int64_t s, int64_t d, uint64_t seed) {
  const uint64_t du = uint64_t(d);
  return int64_t(splitmix64(uint64_t(s) ^ ((du << 32) | (du >> 32)) ^ seed) % 1000);
}

}  // namespace nbg
