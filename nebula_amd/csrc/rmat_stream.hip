// rmat_stream.hip -- the streamed RMAT build (one rank): the generator re-run per phase and per
// bucket instead of staged as tuples (snapshot_gen_rmat only records the parameters).
#include <climits>

#include <rocprim/iterator/counting_iterator.hpp>

#include "build_common.h"

namespace nbg {

// ------------------------------------------------------------------------------------------
// Streamed RMAT build (one rank).  The tuple stage holds 40+ bytes per sample in each CSR
// direction and indexes tuples with 32-bit permutations, so RMAT-28 (2^32 samples) cannot pass
// through it.  Here the generator is re-run instead of stored: one counting pass gives the vertex
// set and the per-vertex sample counts, the vertex numbering is the staged build's (vids sorted,
// then by descending sample out-degree), and each CSR direction is built in src-gidx buckets of
// at most rmat_bucket samples: regenerate, keep the bucket's samples as 64-bit keys
// (local src << 32 | bytewise rank of dst), radix sort, unique (= the version / identical-key
// collapse of a generator that writes one version of rank 0), and emit row_ptr, col, the dst-vid
// column and the weight (a function of (src, dst), recomputed).  Same CSR as the staged build.
// ------------------------------------------------------------------------------------------
__global__ void k_rmat_count(int64_t lo, int64_t hi, int32_t scale, uint64_t seed, uint8_t* present,
                             uint32_t* odeg_u, uint32_t* ideg_u) {
  for (int64_t i = lo + blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < hi; i += int64_t(gridDim.x) * blockDim.x) {
    uint64_t u, v;
    rmat_sample(uint64_t(i), scale, seed, u, v);
    present[u] = 1;  // idempotent byte stores
    present[v] = 1;
    atomicAdd(odeg_u + u, 1u);
    atomicAdd(ideg_u + v, 1u);
  }
}
__global__ void k_rmat_vkeys(const uint32_t* idx, int64_t n, uint64_t smix, uint64_t* key) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    key[i] = uint64_t(rmat_vid(idx[i], smix)) ^ (1ull << 63);
}
// gidx g <-> index u; vid_of; per-gidx sample counts of both directions
__global__ void k_rmat_number(const uint32_t* idx, int64_t n, uint64_t smix, const uint32_t* odeg_u,
                              const uint32_t* ideg_u, int32_t* gidx_of_u, int64_t* vid_of, int64_t* ocnt,
                              int64_t* icnt) {
  for (int64_t g = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; g < n; g += int64_t(gridDim.x) * blockDim.x) {
    const uint32_t u = idx[g];
    gidx_of_u[u] = int32_t(g);
    vid_of[g] = rmat_vid(u, smix);
    ocnt[g] = odeg_u[u];
    icnt[g] = ideg_u[u];
  }
}
// brank_u[u] = bytewise rank of u's vid; gidx_of_rank = its inverse over the gidx space
__global__ void k_rmat_rank_maps(const uint32_t* idx, int64_t n, const uint32_t* brank, uint32_t* brank_u,
                                 int32_t* gidx_of_rank) {
  for (int64_t g = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; g < n; g += int64_t(gridDim.x) * blockDim.x) {
    brank_u[idx[g]] = brank[g];
    gidx_of_rank[brank[g]] = int32_t(g);
  }
}
// bucket starts: row g opens bucket excl[g] / cap when that differs from row g - 1's
__global__ void k_rmat_cuts(const int64_t* excl, int64_t n, int64_t cap, int64_t* cut) {
  for (int64_t g = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; g < n; g += int64_t(gridDim.x) * blockDim.x) {
    const int64_t k = excl[g] / cap;
    if (g == 0 || excl[g - 1] / cap != k) cut[k] = g;
  }
}
// the samples of bucket [ga, gb) of one direction (out: key src u, in: key src v) as sort keys
__global__ void k_rmat_bucket(int64_t lo, int64_t hi, int32_t scale, uint64_t seed, int32_t dir,
                              const int32_t* gidx_of_u, const uint32_t* brank_u, int64_t ga, int64_t gb, uint64_t* keys,
                              unsigned long long* cnt, int64_t cap) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  const int64_t rounds = (hi - lo + stride - 1) / stride;
  for (int64_t r = 0; r < rounds; r++) {
    const int64_t i = lo + r * stride + blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    bool take = false;
    uint64_t key = 0;
    if (i < hi) {
      uint64_t u, v;
      rmat_sample(uint64_t(i), scale, seed, u, v);
      const uint64_t sidx = dir ? v : u, didx = dir ? u : v;
      const int64_t g = gidx_of_u[sidx];
      take = g >= ga && g < gb;
      if (take) key = (uint64_t(g - ga) << 32) | brank_u[didx];
    }
    const int64_t slot = wave_append(cnt, take);
    if (take && slot < cap) keys[slot] = key;
  }
}
// CSR rows [ga, gb) from the bucket's sorted unique keys (entries base .. base + m)
__global__ void k_rmat_emit(const uint64_t* keys, int64_t m, int64_t ga, int64_t nrows, int64_t base,
                            const int32_t* gidx_of_rank, const int64_t* vid_of, uint64_t seed, int64_t* row_ptr,
                            int32_t* col, int64_t* col_vid, int16_t* w16) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i <= m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t prev = i == 0 ? -1 : int64_t(keys[i - 1] >> 32);
    const int64_t cur = i == m ? nrows : int64_t(keys[i] >> 32);
    for (int64_t r = prev + 1; r <= cur; r++) row_ptr[ga + r] = base + i;
    if (i == m) continue;
    const int32_t d = gidx_of_rank[uint32_t(keys[i])];
    col[base + i] = d;
    if (col_vid) {
      const int64_t dv = vid_of[d];
      col_vid[base + i] = dv;
      w16[base + i] = int16_t(rmat_weight(vid_of[ga + cur], dv, seed));
    }
  }
}
__global__ void k_i16_to_i8(const int16_t* in, int8_t* out, int64_t m) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = int8_t(in[i]);
}

struct RmatStream {
  Ctx& c;
  EdgeSpace& es;
  const int32_t scale;
  const uint64_t seed;
  const int64_t E, NU;  // samples, index space
  const uint64_t smix;
  static constexpr int64_t chunk = int64_t(1) << 28;  // samples per generator launch
  DevBuf present, odeg_u, ideg_u;   // per index: referenced, sample counts of both directions
  DevBuf idxA, idxB;
  const uint32_t* order = nullptr;  // index of every gidx (in idxA or idxB)
  int64_t n = 0;                    // vertices
  DevBuf gidx_of_u, ocnt, icnt;     // gidx of every index; per-gidx sample counts
  DevBuf brank_u, gidx_of_rank;     // bytewise rank of every index; its inverse over the gidx space
  int64_t bucket_cap = 0;

  RmatStream(Ctx& ctx, EdgeSpace& e)
      : c(ctx), es(e), scale(e.rmat_scale), seed(e.rmat_seed), E(int64_t(e.rmat_ef) << e.rmat_scale),
        NU(int64_t(1) << e.rmat_scale), smix(splitmix64(e.rmat_seed) & ((1ull << 63) - 1)) {}

  static int sample_grid(int64_t k) { return int(std::max<int64_t>(1, std::min<int64_t>((k + 255) / 256, 256 * 64))); }

  // counting pass: the referenced indices and their sample counts
  void count_samples() {
    present.alloc(size_t(NU));
    odeg_u.alloc(size_t(NU) * 4);
    ideg_u.alloc(size_t(NU) * 4);
    NBG_HIP(hipMemsetAsync(present.p, 0, size_t(NU), c.stream));
    NBG_HIP(hipMemsetAsync(odeg_u.p, 0, size_t(NU) * 4, c.stream));
    NBG_HIP(hipMemsetAsync(ideg_u.p, 0, size_t(NU) * 4, c.stream));
    for (int64_t lo = 0; lo < E; lo += chunk) {
      const int64_t hi = std::min(E, lo + chunk);
      k_rmat_count<<<sample_grid(hi - lo), 256, 0, c.stream>>>(lo, hi, scale, seed, present.as<uint8_t>(),
                                                               odeg_u.as<uint32_t>(), ideg_u.as<uint32_t>());
    }
    NBG_HIP(hipGetLastError());
  }
  // vertex set in the staged build's numbering: vids ascending (signed), then stable by
  // descending sample out-degree (order_by_degree), unless degree_order = 0
  void number_vertices() {
    idxA.alloc(size_t(NU) * 4);
    DevWords<uint64_t, 1> cntb;
    select_dev(c, rocprim::counting_iterator<uint32_t>(0), present.as<uint8_t>(), idxA.as<uint32_t>(), cntb.dev(),
               int64_t(NU));
    n = int64_t(cntb.read(c)[0]);
    present.release();
    if (n == 0) throw Error(NBG_E_INVALID_ARG, "empty RMAT graph");
    idxB.alloc(size_t(n) * 4);
    {
      DevBuf k1, k2;
      k1.alloc(size_t(n) * 8);
      k2.alloc(size_t(n) * 8);
      k_rmat_vkeys<<<grid_for(n), 256, 0, c.stream>>>(idxA.as<uint32_t>(), n, smix, k1.as<uint64_t>());
      radix_pairs<uint64_t, uint32_t>(c, k1.as<uint64_t>(), k2.as<uint64_t>(), idxA.as<uint32_t>(), idxB.as<uint32_t>(),
                                      n, 64);
    }
    order = idxB.as<uint32_t>();
    if (c.opt("degree_order", 1)) {
      // the staged build's key (k_class_key; this builder runs on one rank)
      DevBuf d1, d2;
      d1.alloc(size_t(n) * 8);
      d2.alloc(size_t(n) * 8);
      class_keys(c, odeg_u.as<uint32_t>(), ideg_u.as<uint32_t>(), idxB.as<uint32_t>(), n, d1.as<uint64_t>());
      radix_pairs<uint64_t, uint32_t>(c, d1.as<uint64_t>(), d2.as<uint64_t>(), idxB.as<uint32_t>(), idxA.as<uint32_t>(),
                                      n, kClassKeyBits);
      order = idxA.as<uint32_t>();
    }
  }
  // vertex map (one rank: base = [0, n padded to 64]), per-gidx sample counts and the hash table
  void publish_vertex_map() {
    c.counts.assign(1, n);
    c.base.assign(2, 0);
    c.base[1] = (n + 63) / 64 * 64;
    c.n_global = c.base[1];
    c.n_vertices = n;
    if (c.n_global >= (int64_t(1) << 31)) throw Error(NBG_E_UNSUPPORTED, "more than 2^31 vertices");
    c.vid_of.alloc(size_t(c.n_global) * 8);
    fill<int64_t>(c, c.vid_of.as<int64_t>(), INT64_MIN, c.n_global);
    gidx_of_u.alloc(size_t(NU) * 4);
    ocnt.alloc(size_t(c.n_global + 1) * 8);
    icnt.alloc(size_t(c.n_global + 1) * 8);
    NBG_HIP(hipMemsetAsync(ocnt.p, 0, size_t(c.n_global + 1) * 8, c.stream));
    NBG_HIP(hipMemsetAsync(icnt.p, 0, size_t(c.n_global + 1) * 8, c.stream));
    k_rmat_number<<<grid_for(n), 256, 0, c.stream>>>(order, n, smix, odeg_u.as<uint32_t>(), ideg_u.as<uint32_t>(),
                                                     gidx_of_u.as<int32_t>(), c.vid_of.as<int64_t>(), ocnt.as<int64_t>(),
                                                     icnt.as<int64_t>());
    odeg_u.release();
    ideg_u.release();
    vid_hash_reset(c, c.n_global);
    DevWords<int32_t, 1> dmin;
    dmin.set(c, {-1});
    vid_hash_insert(c, c.vid_of.as<int64_t>(), n, 0, dmin);
    vid_hash_publish_min(c, dmin);
  }
  // bytewise rank of every vertex (row order = RocksDB key order), per index and inverted
  void rank_maps() {
    DevBuf brank = bytewise_ranks(c);
    brank_u.alloc(size_t(NU) * 4);
    gidx_of_rank.alloc(size_t(c.n_global) * 4);
    k_rmat_rank_maps<<<grid_for(n), 256, 0, c.stream>>>(order, n, brank.as<uint32_t>(), brank_u.as<uint32_t>(),
                                                        gidx_of_rank.as<int32_t>());
    order = nullptr;
    idxA.release();
    idxB.release();
  }

  // src-gidx buckets of at most bucket_cap samples (a row of more is a bucket of its own)
  struct Buckets {
    std::vector<int64_t> starts;  // first row of every bucket, then n_rows
    std::vector<int64_t> sb;      // samples before starts[k] (differences: upper bounds of the unique keys)
    int64_t maxb = 0;             // the largest bucket's samples
  };
  Buckets bucket_cuts(int dir) {
    const int64_t n_rows = c.n_global;
    Buckets b;
    DevBuf excl;
    excl.alloc(size_t(n_rows + 1) * 8);
    exclusive_scan_dev<int64_t>(c, (dir ? icnt : ocnt).as<int64_t>(), excl.as<int64_t>(), n_rows + 1);
    int64_t total = 0;
    NBG_HIP(hipMemcpyAsync(&total, excl.as<int64_t>() + n_rows, 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    if (total != E) throw Error(NBG_E_UNKNOWN, "streamed RMAT: sample counts do not add up");
    const int64_t nb = (total + bucket_cap - 1) / bucket_cap;
    DevBuf dcut;
    dcut.alloc(size_t(nb + 1) * 8);
    NBG_HIP(hipMemsetAsync(dcut.p, 0xff, size_t(nb + 1) * 8, c.stream));
    k_rmat_cuts<<<grid_for(n_rows), 256, 0, c.stream>>>(excl.as<int64_t>(), n_rows, bucket_cap, dcut.as<int64_t>());
    std::vector<int64_t> cut(size_t(nb + 1));
    NBG_HIP(hipMemcpyAsync(cut.data(), dcut.p, size_t(nb) * 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    for (int64_t k = 0; k < nb; k++)
      if (cut[size_t(k)] >= 0) b.starts.push_back(cut[size_t(k)]);
    b.starts.push_back(n_rows);
    b.sb.resize(b.starts.size());
    for (size_t k = 0; k < b.starts.size(); k++)
      NBG_HIP(hipMemcpyAsync(&b.sb[k], excl.as<int64_t>() + b.starts[k], 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    for (size_t k = 0; k + 1 < b.starts.size(); k++) b.maxb = std::max(b.maxb, b.sb[k + 1] - b.sb[k]);
    return b;
  }
  // one CSR direction, bucket by bucket: regenerate, keep the bucket's samples as keys, sort,
  // unique, emit; returns the out direction's weights as 16-bit values (for narrow_weight)
  DevBuf build_direction(int dir) {
    const int64_t n_rows = c.n_global;
    Csr& out = dir ? es.in : es.out;
    out = Csr();
    out.n_rows = n_rows;
    const Buckets b = bucket_cuts(dir);
    // final arrays sized for every sample (trimmed nnz is known only at the end; the tail stays unused)
    out.row_ptr.alloc(size_t(n_rows + 1) * 8);
    NBG_HIP(hipMemsetAsync(out.row_ptr.p, 0, 8, c.stream));
    out.col.alloc(size_t(E) * 4 + 64);  // padded: aligned 16-byte loads past the last entry
    const bool with_props = dir == 0;
    DevBuf w16;
    if (with_props) {
      if (c.opt("rows_vid_col", 1)) out.col_vid.alloc(size_t(E) * 8 + 8);
      w16.alloc(size_t(E) * 2 + 16);
    }
    DevBuf kA, kB;
    kA.alloc(size_t(std::max<int64_t>(b.maxb, 1)) * 8);
    kB.alloc(size_t(std::max<int64_t>(b.maxb, 1)) * 8);
    DevWords<unsigned long long, 1> bc;
    int64_t base = 0;
    for (size_t k = 0; k + 1 < b.starts.size(); k++) {
      const int64_t ga = b.starts[k], gb = b.starts[k + 1], want = b.sb[k + 1] - b.sb[k];
      if (want == 0) {  // rows without samples (a run of zero-degree rows)
        k_rmat_emit<<<1, 64, 0, c.stream>>>(kB.as<uint64_t>(), 0, ga, gb - ga, base, gidx_of_rank.as<int32_t>(),
                                            c.vid_of.as<int64_t>(), seed, out.row_ptr.as<int64_t>(),
                                            out.col.as<int32_t>(), nullptr, nullptr);
        continue;
      }
      bc.zero(c);
      for (int64_t lo = 0; lo < E; lo += chunk) {
        const int64_t hi = std::min(E, lo + chunk);
        k_rmat_bucket<<<sample_grid(hi - lo), 256, 0, c.stream>>>(lo, hi, scale, seed, dir, gidx_of_u.as<int32_t>(),
                                                                  brank_u.as<uint32_t>(), ga, gb, kA.as<uint64_t>(),
                                                                  bc.dev(), want);
      }
      radix_keys<uint64_t>(c, kA.as<uint64_t>(), kB.as<uint64_t>(), want, std::min(32 + bits_for(gb - ga), 64));
      const int64_t m = unique_sorted<uint64_t>(c, kB.as<uint64_t>(), kA.as<uint64_t>(), want);
      k_rmat_emit<<<grid_for(m + 1), 256, 0, c.stream>>>(kA.as<uint64_t>(), m, ga, gb - ga, base,
                                                         gidx_of_rank.as<int32_t>(), c.vid_of.as<int64_t>(), seed,
                                                         out.row_ptr.as<int64_t>(), out.col.as<int32_t>(),
                                                         with_props ? out.col_vid.as<int64_t>() : nullptr,
                                                         with_props ? w16.as<int16_t>() : nullptr);
      NBG_HIP(hipGetLastError());
      base += m;
    }
    out.nnz = base;
    // row_part by the hash rule (every generated key sits in hash(vid)'s part: row_ok stays empty)
    out.row_part.alloc(size_t(n_rows + 1) * 4);
    row_part_by_hash(c, c.vid_of.as<int64_t>(), n_rows, out.row_part.as<int32_t>());
    return w16;
  }
  // weight: narrowed to the width its range needs, as gather_props does
  void narrow_weight(Csr& out, DevBuf& w16) {
    const int64_t base = out.nnz;
    PropCol pc;
    pc.name = es.fields[0].name;
    pc.type = es.fields[0].type;
    const auto hm = minmax_w(c, w16.p, 2, base);
    pc.minv = base ? hm[0] : 0;
    pc.maxv = base ? hm[1] : 0;
    if (pc.minv >= INT8_MIN && pc.maxv <= INT8_MAX) {
      pc.width = 1;
      pc.data.alloc(size_t(base) + 16);
      if (base) k_i16_to_i8<<<grid_for(base), 256, 0, c.stream>>>(w16.as<int16_t>(), pc.data.as<int8_t>(), base);
    } else {
      pc.width = 2;
      pc.data = std::move(w16);
    }
    out.props.push_back(std::move(pc));
  }
};

void finalize_rmat_stream(Ctx& c, EdgeSpace& es) {
  if (c.sharded) throw Error(NBG_E_UNSUPPORTED, "streamed RMAT build on more than one rank");
  if (c.edges.size() != 1 || !c.tags.empty())
    throw Error(NBG_E_UNSUPPORTED, "streamed RMAT must be the snapshot's only edge type, without tags");
  RmatStream b(c, es);
  b.count_samples();
  b.number_vertices();
  b.publish_vertex_map();
  b.rank_maps();
  b.bucket_cap = std::max<int64_t>(c.opt("rmat_bucket", int64_t(1) << 30), 1 << 16);
  for (int dir = 0; dir < 2; dir++) {
    DevBuf w16 = b.build_direction(dir);
    if (dir == 0) b.narrow_weight(es.out, w16);
    NBG_HIP(hipStreamSynchronize(c.stream));
  }
  // out-degrees (compaction's degree reads); no transposed CSR: GO runs top-down here
  build_out_degrees(c, es, nullptr, nullptr);
  es.has_tr = false;
  NBG_HIP(hipStreamSynchronize(c.stream));
  NBG_HIP(hipGetLastError());
}

}  // namespace nbg
