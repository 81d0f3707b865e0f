// csr_build.hip -- the snapshot build's CSR builders: one CSR from a stage of decoded tuples
// (build_csr: the reference's key order, the bytewise-first version of every (src, rank, dst),
// narrowed SoA prop columns; or a sorted batch merged into the committed order), and the
// transposed CSR of the out CSR with what the bottom-up hops read beside it (build_transpose:
// hub-first rows, the quantised pack, the pair slab, tile_wide, live bounds, rest records).
#include <climits>

#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>

#include "build_common.h"
#include "qpred.h"

namespace nbg {

__global__ void k_iota_rev_u32(uint32_t* p, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    p[i] = uint32_t(n - 1 - i);
}
__global__ void k_iota_u32(uint32_t* p, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    p[i] = uint32_t(i);
}
// edge sort key (single-pass case): (src_local << 32) | byterank(dst)
__global__ void k_edge_keys(const int64_t* src, const int64_t* dst, int64_t n, const int64_t* keys_ht,
                            const int32_t* vals_ht, uint64_t mask, bool has_min, int32_t min_gidx,
                            int64_t lo, int64_t hi, const uint32_t* byterank, uint64_t* keys,
                            uint32_t* perm, int32_t* dst_g, unsigned long long* err) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int32_t sg = ht_lookup(keys_ht, vals_ht, mask, src[i], has_min, min_gidx);
    int32_t dg = ht_lookup(keys_ht, vals_ht, mask, dst[i], has_min, min_gidx);
    if (sg < lo || sg >= hi || dg < 0) {
      atomicAdd(err, 1ull);
      sg = int32_t(lo);
      dg = 0;
    }
    keys[i] = (uint64_t(uint32_t(sg - lo)) << 32) | uint64_t(byterank[dg]);
    perm[i] = uint32_t(i);
    dst_g[i] = dg;
  }
}
__global__ void k_seq_desc_keys(const int64_t* seq, int64_t n, uint64_t* keys) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    keys[i] = ~uint64_t(seq[i]);
}
// multi-pass LSD helpers: gather a 64-bit key through the current permutation
__global__ void k_gather_key_bswap(const int64_t* vals, const uint32_t* perm, uint64_t* keys, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    keys[i] = bswap64(uint64_t(vals[perm[i]]));
}
__global__ void k_gather_key_src(const uint64_t* srckey, const uint32_t* perm, uint64_t* keys, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    keys[i] = srckey[perm[i]] >> 32;
}

// keep-first flags in sorted order: (src, rank, dst) differs from predecessor
__global__ void k_dedup_flags(const uint64_t* skey, const uint32_t* perm, const int64_t* rank,
                              const int32_t* dst_g, int64_t n, uint8_t* keep) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    bool k = true;
    if (i > 0) {
      uint32_t a = perm[i - 1], b = perm[i];
      bool same = (skey[a] >> 32) == (skey[b] >> 32) && dst_g[a] == dst_g[b] &&
                  (rank == nullptr || rank[a] == rank[b]);
      k = !same;
    }
    keep[i] = k;
  }
}

// row_ptr from row keys sorted ascending (no atomics): row_ptr[v] = first i with key[i] >= v
// row_ptr[0, n] from the sorted row keys of m entries: entry i (i = m: the end) opens the rows
// (keys[i - 1], keys[i]].  A run of more than kRowRun rows (rows without entries: with the
// class-ordered numbering the in-only class of an out CSR is one run of millions) goes to a list
// filled by k_rowptr_runs, one block per run -- one thread storing it row by row took 10 ms at
// RMAT-22 and most of a merge commit at RMAT-26.
constexpr int64_t kRowRun = 64;
__global__ void k_rowptr_sorted(const uint32_t* keys, int64_t m, int64_t n, int64_t* row_ptr, int64_t* runs,
                                unsigned long long* nruns, int64_t cap) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i <= m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t prev = i == 0 ? -1 : int64_t(keys[i - 1]);
    const int64_t cur = i == m ? n : int64_t(keys[i]);
    if (cur - prev > kRowRun) {
      const unsigned long long slot = atomicAdd(nruns, 1ull);
      if (int64_t(slot) < cap) {
        runs[3 * slot] = prev + 1, runs[3 * slot + 1] = cur, runs[3 * slot + 2] = i;
        continue;
      }
    }
    for (int64_t v = prev + 1; v <= cur; v++) row_ptr[v] = i;
  }
}
__global__ void k_rowptr_runs(const int64_t* runs, const unsigned long long* nruns, int64_t cap, int64_t* row_ptr) {
  const int64_t nr = int64_t(*nruns) < cap ? int64_t(*nruns) : cap;
  for (int64_t r = blockIdx.x; r < nr; r += gridDim.x) {
    const int64_t a = runs[3 * r], b = runs[3 * r + 1], val = runs[3 * r + 2];
    for (int64_t v = a + threadIdx.x; v <= b; v += blockDim.x) row_ptr[v] = val;
  }
}
static void rowptr_from_sorted(Ctx& c, const uint32_t* keys, int64_t m, int64_t n, int64_t* row_ptr) {
  // every listed run holds more than kRowRun of the n + 1 rows
  const int64_t cap = (n + 1) / kRowRun + 1;
  DevBuf runs, cnt;
  runs.alloc(size_t(cap) * 24);
  cnt.alloc(8);
  NBG_HIP(hipMemsetAsync(cnt.p, 0, 8, c.stream));
  k_rowptr_sorted<<<grid_for(m + 1), 256, 0, c.stream>>>(keys, m, n, row_ptr, runs.as<int64_t>(),
                                                        cnt.as<unsigned long long>(), cap);
  k_rowptr_runs<<<1024, 256, 0, c.stream>>>(runs.as<int64_t>(), cnt.as<unsigned long long>(), cap, row_ptr);
  NBG_HIP(hipGetLastError());
}
__global__ void k_kept_src(const uint64_t* skey, const uint32_t* kept, int64_t m, uint32_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = uint32_t(skey[kept[i]] >> 32);
}
__global__ void k_row_part_default(const int64_t* vid_of_lo, int64_t n, int32_t parts, int32_t* row_part) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    row_part[i] = dev_part_of(vid_of_lo[i], parts);
}
__global__ void k_row_part_scatter(const uint64_t* skey, const uint32_t* kept_perm, int64_t m, const int32_t* part,
                                   int32_t* row_part) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    uint32_t t = kept_perm[i];
    row_part[skey[t] >> 32] = part[t];
  }
}
__global__ void k_row_ok(const int64_t* vid_of_lo, int64_t n, int32_t parts, const int32_t* row_part, uint8_t* ok,
                         unsigned long long* bad) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    bool g = row_part[i] == dev_part_of(vid_of_lo[i], parts);
    ok[i] = g;
    if (!g) atomicAdd(bad, 1ull);
  }
}
__global__ void k_row_counts(const uint64_t* skey, const uint32_t* kept_perm, int64_t m, int64_t* counts) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    atomicAdd(reinterpret_cast<unsigned long long*>(counts + (skey[kept_perm[i]] >> 32)), 1ull);
}
template <typename T>
__global__ void k_gather_w(const T* in, const uint32_t* perm, T* out, int64_t m) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = in[perm[i]];
}
template <typename T>
static void gather(Ctx& c, const T* in, const uint32_t* perm, T* out, int64_t m) {
  k_gather_w<T><<<grid_for(m), 256, 0, c.stream>>>(in, perm, out, m);
}
__global__ void k_col_vid(const int32_t* col, const int64_t* vid_of, int64_t m, int64_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = vid_of[col[i]];
}
template <typename T>
__global__ void k_narrow(const int64_t* in, T* out, int64_t m) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = T(in[i]);
}
__global__ void k_str_lengths(const int64_t* lens, const uint8_t* present, int64_t m, int64_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = (present == nullptr || present[i]) ? lens[i] : 0;
}
__global__ void k_str_copy(const uint8_t* heap, const int64_t* offs_src, const int64_t* dst_off, int64_t m,
                           uint8_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    int64_t len = dst_off[i + 1] - dst_off[i];
    const uint8_t* s = heap + offs_src[i];
    uint8_t* d = out + dst_off[i];
    for (int64_t j = 0; j < len; j++) d[j] = s[j];
  }
}

// (a rocprim reduce, not k_minmax_w: it is what the staged build has always run on its 8-byte
// columns, and the build's device code stays as it is)
static void minmax_i64(Ctx& c, const int64_t* d, int64_t n, int64_t& mn, int64_t& mx) {
  DevBuf r;
  r.alloc(16);
  size_t tb = 0;
  NBG_HIP(rocprim::reduce(nullptr, tb, d, r.as<int64_t>(), INT64_MAX, size_t(n), rocprim::minimum<int64_t>(), c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::reduce(c.ws_tmp.p, tb, d, r.as<int64_t>(), INT64_MAX, size_t(n), rocprim::minimum<int64_t>(), c.stream));
  tb = 0;
  NBG_HIP(rocprim::reduce(nullptr, tb, d, r.as<int64_t>() + 1, INT64_MIN, size_t(n), rocprim::maximum<int64_t>(), c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::reduce(c.ws_tmp.p, tb, d, r.as<int64_t>() + 1, INT64_MIN, size_t(n), rocprim::maximum<int64_t>(), c.stream));
  int64_t h[2];
  NBG_HIP(hipMemcpyAsync(h, r.p, 16, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  mn = h[0];
  mx = h[1];
}

// older-version flags over the sorted tuples: not kept (a later version of a kept group) and
// not an overwritten identical key (same version as its predecessor: WriteBatch last write wins
// puts the visible write first).  escan[i] = keep[i] (inclusive-scanned by the caller -> the
// group's edge index + 1).
__global__ void k_old_version_flags(const uint32_t* perm, const uint8_t* keep, const int64_t* ver, int64_t n,
                                    uint8_t* ov, uint32_t* escan, unsigned long long* count) {
  unsigned long long c = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    escan[i] = keep[i];
    const bool o = !keep[i] && i > 0 && ver[perm[i]] != ver[perm[i - 1]];
    ov[i] = o;
    c += o;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}
// the older versions' group edge indices: inclusive keep-scan - 1, widened
__global__ void k_ov_edges(const uint32_t* e, int64_t n, int64_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = int64_t(e[i]) - 1;
}
// SoA prop columns of the staged tuples kp[0..m) (in that order): INT-like values narrowed to
// the smallest width holding [min, max] when `narrow`, DOUBLE as bits, STRING as offsets + bytes
static void gather_props(Ctx& c, Staging& s, const std::vector<Field>& fields, const uint32_t* kp, int64_t m,
                         bool narrow, std::vector<PropCol>& props_out) {
  DevBuf tmp;
  tmp.alloc(size_t(m) * 8 + 8);
  for (size_t f = 0; f < fields.size(); f++) {
    PropCol pc;
    pc.name = fields[f].name;
    pc.type = fields[f].type;
    gather<int64_t>(c, s.props[f].as<int64_t>(), kp, tmp.as<int64_t>(), m);
    bool has_present = f < s.present.size() && s.present[f].p != nullptr;
    if (has_present) {
      pc.present.alloc(size_t(m) + 1);
      gather<uint8_t>(c, s.present[f].as<uint8_t>(), kp, pc.present.as<uint8_t>(), m);
    }
    if (pc.type == NBG_T_STRING) {
      DevBuf lens, offs_src;
      lens.alloc(size_t(m) * 8 + 8);
      offs_src.alloc(size_t(m) * 8 + 8);
      gather<int64_t>(c, s.str_len[f].as<int64_t>(), kp, lens.as<int64_t>(), m);
      NBG_HIP(hipMemcpyAsync(offs_src.p, tmp.p, size_t(m) * 8, hipMemcpyDeviceToDevice, c.stream));
      DevBuf l2;
      l2.alloc(size_t(m + 1) * 8);
      k_str_lengths<<<grid_for(m), 256, 0, c.stream>>>(lens.as<int64_t>(),
                                                             has_present ? pc.present.as<uint8_t>() : nullptr,
                                                             m, l2.as<int64_t>());
      NBG_HIP(hipMemsetAsync(l2.as<int64_t>() + m, 0, 8, c.stream));
      pc.str_off.alloc(size_t(m + 1) * 8);
      exclusive_scan_dev<int64_t>(c, l2.as<int64_t>(), pc.str_off.as<int64_t>(), m + 1);
      int64_t total = 0;
      NBG_HIP(hipMemcpyAsync(&total, pc.str_off.as<int64_t>() + m, 8, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipStreamSynchronize(c.stream));
      pc.str_bytes.alloc(size_t(total) + 8);
      k_str_copy<<<grid_for(m), 256, 0, c.stream>>>(c.heap.as<uint8_t>(), offs_src.as<int64_t>(),
                                                           pc.str_off.as<int64_t>(), m, pc.str_bytes.as<uint8_t>());
      pc.width = 0;
    } else if (pc.type == NBG_T_DOUBLE || pc.type == NBG_T_FLOAT) {
      pc.width = 8;
      pc.data.alloc(size_t(m) * 8 + 8);
      NBG_HIP(hipMemcpyAsync(pc.data.p, tmp.p, size_t(m) * 8, hipMemcpyDeviceToDevice, c.stream));
    } else {
      // INT / VID / TIMESTAMP / BOOL: narrow to the smallest width holding [min, max]
      int64_t mn = 0, mx = 0;
      if (m) minmax_i64(c, tmp.as<int64_t>(), m, mn, mx);
      pc.minv = mn;
      pc.maxv = mx;
      int w = 8;
      if (mn >= INT8_MIN && mx <= INT8_MAX) w = 1;
      else if (mn >= INT16_MIN && mx <= INT16_MAX) w = 2;
      else if (mn >= INT32_MIN && mx <= INT32_MAX) w = 4;
      if (!narrow) w = 8;
      pc.width = w;
      pc.data.alloc(size_t(m) * size_t(w) + 16);
      int g = grid_for(m);
      switch (w) {
        case 1: k_narrow<int8_t><<<g, 256, 0, c.stream>>>(tmp.as<int64_t>(), pc.data.as<int8_t>(), m); break;
        case 2: k_narrow<int16_t><<<g, 256, 0, c.stream>>>(tmp.as<int64_t>(), pc.data.as<int16_t>(), m); break;
        case 4: k_narrow<int32_t><<<g, 256, 0, c.stream>>>(tmp.as<int64_t>(), pc.data.as<int32_t>(), m); break;
        default: NBG_HIP(hipMemcpyAsync(pc.data.p, tmp.p, size_t(m) * 8, hipMemcpyDeviceToDevice, c.stream));
      }
    }
    props_out.push_back(std::move(pc));
  }
}

// (src, rank bytes, dst bytes, version bytes) order of two tuples: the merge commit's key (the
// sort's last key, load sequence descending, is implied: a batch is newer than every committed
// tuple and the merge puts it first among equals)
struct GroupLess {
  const uint64_t* skey;
  const int64_t* rank;  // null: constant
  const int64_t* ver;   // null: constant
  __device__ bool operator()(uint32_t a, uint32_t b) const {
    const uint64_t ka = skey[a], kb = skey[b];
    if ((ka >> 32) != (kb >> 32)) return (ka >> 32) < (kb >> 32);
    if (rank) {
      const uint64_t ra = bswap64(uint64_t(rank[a])), rb = bswap64(uint64_t(rank[b]));
      if (ra != rb) return ra < rb;
    }
    if (uint32_t(ka) != uint32_t(kb)) return uint32_t(ka) < uint32_t(kb);
    if (ver) {
      const uint64_t va = bswap64(uint64_t(ver[a])), vb = bswap64(uint64_t(ver[b]));
      if (va != vb) return va < vb;
    }
    return false;
  }
};
__global__ void k_iota_off_u32(uint32_t* p, int64_t n, int64_t off) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    p[i] = uint32_t(off + i);
}

// One CSR from a non-empty stage, phase by phase (build_csr calls them in order).  The sort
// scratch and the final permutation are members so that each is freed where the build is done
// with it, not at the end.
struct CsrBuild {
  Ctx& c;
  Staging& s;
  const std::vector<Field>& fields;
  const bool with_props;
  Csr& out;
  const uint32_t* byterank;
  EdgeSpace::Order* ord;
  const int64_t n, lo, hi;
  const int srcbits;
  const int64_t n0;    // tuples of the committed order
  const bool merging;  // merge commit: sort the batch [n0, n) only and merge it in
  DevWords<unsigned long long, 1> err;
  DevBuf skey;                 // (src_local << 32 | byterank(dst)) by tuple index
  DevBuf dstg;                 // dst gidx by tuple index
  DevBuf keyB, permA, permB;   // sort scratch
  DevBuf perm;                 // the tuples in key order
  DevBuf keep, kept, ovp;
  uint64_t m = 0;  // kept edges

  CsrBuild(Ctx& ctx, Staging& st, const std::vector<Field>& f, bool props, Csr& o, const uint32_t* br,
           EdgeSpace::Order* od, bool merge)
      : c(ctx), s(st), fields(f), with_props(props), out(o), byterank(br), ord(od), n(st.n), lo(ctx.owned_lo()),
        hi(ctx.owned_hi()), srcbits(bits_for(o.n_rows)), n0(od ? od->n : 0),
        merging(merge && od && n0 > 0 && n0 < n && od->perm.p && st.seq.bytes >= size_t(n) * 8) {
    err.zero(c);
  }

  // sort keys and dst gidx of the whole stage, or (merging) of the batch behind the committed ones
  void edge_keys() {
    const int64_t first = merging ? n0 : 0, cnt = n - first;
    if (merging) {
      // the committed keys grow in place when their (pool-rounded) block has room for the batch
      auto grow = [&](DevBuf& dst, DevBuf& old, size_t w) {
        if (old.bytes >= size_t(n) * w) {
          dst = std::move(old);
        } else {
          dst.alloc(size_t(n) * w);
          NBG_HIP(hipMemcpyAsync(dst.p, old.p, size_t(n0) * w, hipMemcpyDeviceToDevice, c.stream));
        }
      };
      grow(skey, ord->skey, 8);
      grow(dstg, ord->dstg, 4);
      keyB.alloc(size_t(cnt) * 8);
      permA.alloc(size_t(cnt) * 4);
      permB.alloc(size_t(cnt) * 4);
    } else {
      skey.alloc(size_t(n) * 8);
      keyB.alloc(size_t(n) * 8);
      permA.alloc(size_t(n) * 4);
      permB.alloc(size_t(n) * 4);
      dstg.alloc(size_t(n) * 4);
    }
    k_edge_keys<<<grid_for(cnt), 256, 0, c.stream>>>(
        s.src.as<int64_t>() + first, s.dst.as<int64_t>() + first, cnt, c.ht_keys.as<int64_t>(), c.ht_vals.as<int32_t>(),
        uint64_t(c.ht_cap - 1), c.ht_has_min, c.ht_min_gidx, lo, hi, byterank, skey.as<uint64_t>() + first,
        permA.as<uint32_t>(), dstg.as<int32_t>() + first, err.dev());
  }
  // the one stream wait of the ordering phases: every key named an owned src and a known dst
  void check_keys() {
    NBG_HIP(hipGetLastError());
    if (err.read(c)[0]) throw Error(NBG_E_PART_NOT_FOUND, "edge source not owned by this rank / unknown vertex");
  }

  // permA = the tuples [first, first + cnt) by load sequence descending
  void newest_first(int64_t first, int64_t cnt) {
    DevBuf keyC;
    keyC.alloc(size_t(cnt) * 8);
    if (first) k_iota_off_u32<<<grid_for(cnt), 256, 0, c.stream>>>(permB.as<uint32_t>(), cnt, first);
    else k_iota_u32<<<grid_for(cnt), 256, 0, c.stream>>>(permB.as<uint32_t>(), cnt);
    k_seq_desc_keys<<<grid_for(cnt), 256, 0, c.stream>>>(s.seq.as<int64_t>() + first, cnt, keyC.as<uint64_t>());
    radix_pairs<uint64_t, uint32_t>(c, keyC.as<uint64_t>(), keyB.as<uint64_t>(), permB.as<uint32_t>(),
                                    permA.as<uint32_t>(), cnt, 64);
  }
  // LSD passes over the cnt tuples listed in permA (global tuple indices, already ordered by load
  // sequence descending): version bytes, dst bytes, rank bytes, then src; the result is in permA
  void lsd_passes(int64_t cnt) {
    DevBuf keyC;
    keyC.alloc(size_t(cnt) * 8);
    auto sort_pass = [&](int bits) {
      radix_pairs<uint64_t, uint32_t>(c, keyC.as<uint64_t>(), keyB.as<uint64_t>(), permA.as<uint32_t>(),
                                      permB.as<uint32_t>(), cnt, bits);
      std::swap(permA, permB);
    };
    auto pass_bswap = [&](const DevBuf& vals) {
      k_gather_key_bswap<<<grid_for(cnt), 256, 0, c.stream>>>(vals.as<int64_t>(), permA.as<uint32_t>(),
                                                              keyC.as<uint64_t>(), cnt);
      sort_pass(64);
    };
    if (!s.ver_const) pass_bswap(s.ver);
    pass_bswap(s.dst);
    if (!s.rank_const) pass_bswap(s.rank);
    k_gather_key_src<<<grid_for(cnt), 256, 0, c.stream>>>(skey.as<uint64_t>(), permA.as<uint32_t>(), keyC.as<uint64_t>(),
                                                          cnt);
    sort_pass(srcbits);
  }

  // single pass on (src_local, byterank(dst)) == the reference key order (constant rank and version)
  void order_full() {
    check_keys();
    radix_pairs<uint64_t, uint32_t>(c, skey.as<uint64_t>(), keyB.as<uint64_t>(), permA.as<uint32_t>(),
                                    permB.as<uint32_t>(), n, 32 + srcbits);
    perm = std::move(permB);
  }
  void order_lsd() {
    check_keys();
    // start from reverse load order: stable passes then put the LAST write of identical keys
    // first, so keep-first implements WriteBatch last-write-wins (RocksEngine.cpp:216-230).
    // The decode stage appends tuples in wave order, not load order, so the start permutation
    // is the staged load sequence numbers sorted descending.
    if (s.seq.bytes >= size_t(n) * 8) newest_first(0, n);
    else k_iota_rev_u32<<<grid_for(n), 256, 0, c.stream>>>(permA.as<uint32_t>(), n);
    lsd_passes(n);
    perm = std::move(permA);
  }
  // merge commit: the batch sorted on its own (LSD, load sequence descending first), then merged
  // into the committed order -- the batch first among equal groups (it is newer), which is the
  // full sort's order
  void order_merge() {
    const int64_t mb = n - n0;
    newest_first(n0, mb);
    lsd_passes(mb);
    perm.alloc(size_t(n) * 4);
    const GroupLess less{skey.as<uint64_t>(), s.rank_const ? nullptr : s.rank.as<int64_t>(),
                         s.ver_const ? nullptr : s.ver.as<int64_t>()};
    size_t tb = 0;
    NBG_HIP(rocprim::merge(nullptr, tb, permA.as<uint32_t>(), ord->perm.as<uint32_t>(), perm.as<uint32_t>(), size_t(mb),
                           size_t(n0), less, c.stream));
    c.ws_tmp.ensure(tb);
    NBG_HIP(rocprim::merge(c.ws_tmp.p, tb, permA.as<uint32_t>(), ord->perm.as<uint32_t>(), perm.as<uint32_t>(),
                           size_t(mb), size_t(n0), less, c.stream));
    ord->perm.release();
    ord->skey.release();
    ord->dstg.release();
    check_keys();  // (the batch's sort and the merge are queued ahead of this stream wait)
  }

  // keep the first (= bytewise-smallest version) of every (src, rank, dst)
  void dedup() {
    keep.alloc(size_t(n));
    const int64_t* rank_ptr = s.rank_const ? nullptr : s.rank.as<int64_t>();
    k_dedup_flags<<<grid_for(n), 256, 0, c.stream>>>(skey.as<uint64_t>(), perm.as<uint32_t>(), rank_ptr,
                                                     dstg.as<int32_t>(), n, keep.as<uint8_t>());
    kept.alloc(size_t(n) * 4);
    DevWords<uint64_t, 1> cnt;
    select_dev(c, perm.as<uint32_t>(), keep.as<uint8_t>(), kept.as<uint32_t>(), cnt.dev(), n);
    m = cnt.read(c)[0];
    out.nnz = int64_t(m);
  }
  // older versions (multi-version data): tuples that are neither kept nor an overwritten
  // identical key, with the edge index of their group (the firstLoop side table, Csr::ov_*)
  void older_versions() {
    out.ov_n = 0;
    out.ov_edge.release();
    out.ov_props.clear();
    if (!(with_props && !s.ver_const && int64_t(m) < n)) return;
    DevBuf ovf, escan, ove;
    ovf.alloc(size_t(n));
    escan.alloc(size_t(n) * 4);
    DevWords<unsigned long long, 1> ocnt;
    ocnt.zero(c);
    k_old_version_flags<<<grid_for(n), 256, 0, c.stream>>>(perm.as<uint32_t>(), keep.as<uint8_t>(), s.ver.as<int64_t>(),
                                                           n, ovf.as<uint8_t>(), escan.as<uint32_t>(), ocnt.dev());
    const uint64_t no = ocnt.read(c)[0];
    if (!no) return;
    // buffers sized by the older-version count (kept edges < 2^32: 32-bit scan)
    size_t tb2 = 0;
    NBG_HIP(rocprim::inclusive_scan(nullptr, tb2, escan.as<uint32_t>(), escan.as<uint32_t>(), size_t(n),
                                    rocprim::plus<uint32_t>(), c.stream));
    c.ws_tmp.ensure(tb2);
    NBG_HIP(rocprim::inclusive_scan(c.ws_tmp.p, tb2, escan.as<uint32_t>(), escan.as<uint32_t>(), size_t(n),
                                    rocprim::plus<uint32_t>(), c.stream));
    ovp.alloc(size_t(no) * 4 + 4);
    ove.alloc(size_t(no) * 4 + 4);
    select_dev(c, perm.as<uint32_t>(), ovf.as<uint8_t>(), ovp.as<uint32_t>(), ocnt.dev<uint64_t>(), n);
    select_dev(c, escan.as<uint32_t>(), ovf.as<uint8_t>(), ove.as<uint32_t>(), ocnt.dev<uint64_t>(), n);
    out.ov_n = int64_t(no);
    out.ov_edge.alloc(size_t(no) * 8 + 8);
    k_ov_edges<<<grid_for(int64_t(no)), 256, 0, c.stream>>>(ove.as<uint32_t>(), int64_t(no), out.ov_edge.as<int64_t>());
  }
  // the sort is over: only the final permutation (for keep_order) and the kept list stay
  void release_sort_scratch() {
    keyB.release();
    permA.release();
    permB.release();
    keep.release();
  }

  // row_ptr (kept edges are sorted by src)
  void emit_row_ptr() {
    DevBuf ks;
    ks.alloc(size_t(m + 1) * 4);
    k_kept_src<<<grid_for(int64_t(m)), 256, 0, c.stream>>>(skey.as<uint64_t>(), kept.as<uint32_t>(), int64_t(m),
                                                           ks.as<uint32_t>());
    rowptr_from_sorted(c, ks.as<uint32_t>(), int64_t(m), out.n_rows, out.row_ptr.as<int64_t>());
    NBG_HIP(hipStreamSynchronize(c.stream));
  }
  // row_part: hash rule by default, the key's part where the staging recorded it
  void emit_row_part() {
    out.row_part.alloc(size_t(out.n_rows + 1) * 4);
    row_part_by_hash(c, c.vid_of.as<int64_t>() + lo, out.n_rows, out.row_part.as<int32_t>());
    if (!s.part.p) return;
    DevWords<unsigned long long, 1> bad;
    bad.zero(c);
    k_row_part_scatter<<<grid_for(int64_t(m)), 256, 0, c.stream>>>(skey.as<uint64_t>(), kept.as<uint32_t>(), int64_t(m),
                                                                   s.part.as<int32_t>(), out.row_part.as<int32_t>());
    out.row_ok.alloc(size_t(out.n_rows + 1));
    k_row_ok<<<grid_for(out.n_rows), 256, 0, c.stream>>>(c.vid_of.as<int64_t>() + lo, out.n_rows, c.num_parts,
                                                         out.row_part.as<int32_t>(), out.row_ok.as<uint8_t>(), bad.dev());
    if (bad.read(c)[0] == 0) out.row_ok.release();
  }
  // col, col_vid, rank and the prop columns, in kept order
  void emit_columns() {
    const uint32_t* kp = kept.as<uint32_t>();
    out.col.alloc(size_t(m) * 4 + 64);  // padded: aligned 16-byte loads past the last entry
    gather<int32_t>(c, dstg.as<int32_t>(), kp, out.col.as<int32_t>(), int64_t(m));
    // the out CSR's dst vids as a column of their own: a plain GO's rows (YIELD _dst) stream it
    // instead of gathering vid_of[col[e]] (one random line per row)
    if (with_props && c.opt("rows_vid_col", 1) && m) {
      out.col_vid.alloc(size_t(m) * 8 + 8);
      k_col_vid<<<grid_for(int64_t(m)), 256, 0, c.stream>>>(out.col.as<int32_t>(), c.vid_of.as<int64_t>(), int64_t(m),
                                                            out.col_vid.as<int64_t>());
    }
    if (!s.rank_const) {
      out.rank.alloc(size_t(m) * 8 + 8);
      gather<int64_t>(c, s.rank.as<int64_t>(), kp, out.rank.as<int64_t>(), int64_t(m));
      int64_t mn, mx;
      minmax_i64(c, out.rank.as<int64_t>(), int64_t(m), mn, mx);
      if (mn == 0 && mx == 0) out.rank.release();
    } else if (s.rank_value != 0) {
      out.rank.alloc(size_t(m) * 8 + 8);
      fill<int64_t>(c, out.rank.as<int64_t>(), s.rank_value, int64_t(m));
    }
    if (with_props) gather_props(c, s, fields, kp, int64_t(m), true, out.props);
    // older versions of multi-version groups (firstLoop side table, selected above)
    if (out.ov_n) gather_props(c, s, fields, ovp.as<uint32_t>(), out.ov_n, false, out.ov_props);
    NBG_HIP(hipStreamSynchronize(c.stream));
    NBG_HIP(hipGetLastError());
  }
  // the sorted order for a later merge commit (writable snapshots only)
  void keep_order(bool consume) {
    if (!ord) return;
    ord->perm.release();
    ord->skey.release();
    ord->dstg.release();
    ord->n = 0;
    if (!consume && perm.p) {
      ord->perm = std::move(perm);
      ord->skey = std::move(skey);
      ord->dstg = std::move(dstg);
      ord->n = n;
    }
  }
  // a writable snapshot keeps its decoded tuples (the write log) for the next commit
  void consume_stage() {
    s.src.release();
    s.dst.release();
    s.rank.release();
    s.ver.release();
    s.part.release();
    s.props.clear();
    s.present.clear();
    s.str_len.clear();
    s.n = 0;
    s.cap = 0;
  }
};

void build_csr(Ctx& c, Staging& s, const std::vector<Field>& fields, bool with_props, Csr& out,
               const uint32_t* byterank, bool consume, EdgeSpace::Order* ord, bool merge) {
  out = Csr();  // a commit retried after a failed build must not extend a half-built CSR
  out.n_rows = c.owned_hi() - c.owned_lo();
  out.row_ptr.alloc(size_t(out.n_rows + 1) * 8);
  if (s.n == 0) {
    NBG_HIP(hipMemsetAsync(out.row_ptr.p, 0, size_t(out.n_rows + 1) * 8, c.stream));
    out.nnz = 0;
    for (auto& f : fields)
      if (with_props) {
        PropCol pc;
        pc.name = f.name;
        pc.type = f.type;
        out.props.push_back(std::move(pc));
      }
    return;
  }
  if (s.n >= (int64_t(1) << 32)) throw Error(NBG_E_UNSUPPORTED, "more than 2^32 edges on one rank");
  CsrBuild b(c, s, fields, with_props, out, byterank, ord, merge);
  b.edge_keys();
  if (b.merging) b.order_merge();
  else if (s.rank_const && s.ver_const) b.order_full();
  else b.order_lsd();
  b.dedup();
  b.older_versions();
  b.release_sort_scratch();
  b.emit_row_ptr();
  b.emit_row_part();
  b.emit_columns();
  b.keep_order(consume);
  if (consume) b.consume_stage();
}

__global__ void k_edge_src(const int64_t* row_ptr, int64_t n_rows, int32_t* esrc) {
  for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r < n_rows; r += int64_t(gridDim.x) * blockDim.x)
    for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) esrc[e] = int32_t(r);
}
__global__ void k_tr_col(const uint32_t* t_eid, const int32_t* esrc, int64_t m, int64_t lo, int32_t* tcol) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    tcol[i] = int32_t(lo) + esrc[t_eid[i]];
}
__global__ void k_sorted_bounds(const uint32_t* keys, int64_t m, const int64_t* bounds, int nb, int64_t* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  int64_t lo = 0, hi = m, x = bounds[i];  // first index with key >= x
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (int64_t(keys[mid]) < x) lo = mid + 1; else hi = mid;
  }
  out[i] = lo;
}
__global__ void k_src_global(const uint32_t* perm, const int32_t* esrc, int64_t m, int64_t lo, int32_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = int32_t(lo) + esrc[perm[i]];
}
__global__ void k_sub_lo(const int32_t* in, int64_t m, int64_t lo, uint32_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = uint32_t(in[i] - lo);
}
static void gather_width(Ctx& c, const void* in, const uint32_t* perm, void* out, int64_t m, int w) {
  switch (w) {
    case 1: gather(c, static_cast<const int8_t*>(in), perm, static_cast<int8_t*>(out), m); break;
    case 2: gather(c, static_cast<const int16_t*>(in), perm, static_cast<int16_t*>(out), m); break;
    case 4: gather(c, static_cast<const int32_t*>(in), perm, static_cast<int32_t*>(out), m); break;
    default: gather(c, static_cast<const int64_t*>(in), perm, static_cast<int64_t*>(out), m);
  }
}
static bool copy_prop(const PropCol& p) {
  bool intlike = p.type == NBG_T_INT || p.type == NBG_T_VID || p.type == NBG_T_TIMESTAMP || p.type == NBG_T_BOOL;
  return intlike && !p.present.p;
}


// out[0] = 1 + the last row with an in-edge (transposed row), out[1] = 1 + the last row with
// an in-edge and an out-edge
__global__ void k_live_bounds(const int64_t* trp, const uint32_t* odeg, int64_t n, unsigned long long* out) {
  unsigned long long a = 0, b = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    if (trp[i + 1] > trp[i]) {
      a = (unsigned long long)(i + 1);
      if (odeg[i]) b = (unsigned long long)(i + 1);
    }
  for (int o = 32; o > 0; o >>= 1) {
    a = max(a, (unsigned long long)__shfl_xor((long long)a, o));
    b = max(b, (unsigned long long)__shfl_xor((long long)b, o));
  }
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicMax(out, a);
    if (b) atomicMax(out + 1, b);
  }
}
__global__ void k_odeg8(const uint32_t* deg, int64_t n, uint8_t* d8) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    d8[i] = uint8_t(min(deg[i], 255u));
}
__global__ void k_out_deg(const int64_t* row_ptr, const uint8_t* row_ok, int64_t n, uint32_t* deg,
                          unsigned int* maxd) {
  unsigned int m = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    uint32_t d = uint32_t(row_ptr[i + 1] - row_ptr[i]);
    if (row_ok && !row_ok[i]) d = 0;
    deg[i] = d;
    m = d > m ? d : m;
  }
  if (maxd) atomicMax(maxd, m);
}
// hub-first key: sources with larger out-degree sort first inside a transposed row
__global__ void k_hub_key(const int32_t* tsrc, int64_t m, const uint32_t* gdeg, uint32_t maxd, uint32_t* key) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
    key[i] = maxd - gdeg[tsrc[i]];
}
// min / max of a narrowed INT column (width 1/2/4/8)
__global__ void k_minmax_w(const void* data, int w, int64_t m, long long* mm) {
  long long lo = LLONG_MAX, hi = LLONG_MIN;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    long long v = w == 1 ? static_cast<const int8_t*>(data)[i]
                : w == 2 ? static_cast<const int16_t*>(data)[i]
                : w == 4 ? static_cast<const int32_t*>(data)[i]
                         : static_cast<const int64_t*>(data)[i];
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const long long a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
  }
}
// packed transposed column: (bucket << gbits) | src gidx
__global__ void k_pack_col(const int32_t* col, const void* data, int w, int64_t m, int64_t vmin, uint64_t range,
                           int gbits, int qbits, int32_t* out) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t v = w == 1 ? static_cast<const int8_t*>(data)[i]
                    : w == 2 ? static_cast<const int16_t*>(data)[i]
                    : w == 4 ? static_cast<const int32_t*>(data)[i]
                             : static_cast<const int64_t*>(data)[i];
    out[i] = int32_t((q_bucket(v, vmin, range, qbits) << gbits) | uint32_t(col[i]));
  }
}
// quad slab: row d's first 4 entries as two row-major halves (slots 0-1 in lo, 2-3 in hi)
template <typename T>
__global__ void k_build_pair(const int64_t* trp, const T* src, int64_t n, T* lo, T* hi, T none) {
  for (int64_t d = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; d < n; d += int64_t(gridDim.x) * blockDim.x) {
    const int64_t b = trp[d], e = trp[d + 1];
#pragma unroll
    for (int q = 0; q < 4; q++) (q < 2 ? lo : hi)[size_t(d) * 2 + (q & 1)] = b + q < e ? src[b + q] : none;
  }
}

// EdgeSpace::tile_wide: bit t set iff a row of 128-row tile t has at least 3 entries (slots 2-3 of
// the tile's other rows are all pad).  A wave covers 64 consecutive rows per step: one atomic
// per half tile with such a row.  `wide` is zeroed by the caller.
__global__ void k_tile_wide(const int64_t* trp, int64_t n, uint32_t* wide) {
  const int lane = threadIdx.x & 63;
  for (int64_t b = blockIdx.x * int64_t(blockDim.x) + threadIdx.x - lane; b < n; b += int64_t(gridDim.x) * blockDim.x) {
    const int64_t d = b + lane;
    const bool w = d < n && trp[d + 1] - trp[d] >= 3;
    const int64_t t = b >> 7;
    if (__ballot(w) != 0ull && lane == 0) atomicOr(wide + (t >> 5), 1u << (uint32_t(t) & 31u));
  }
}

// EdgeSpace::tile_shape: one word per 128-row tile, a wave per tile (a lane owns rows l and l + 64,
// as in the first pass).  Bit 31: the tile_wide bit.  Bits 0-30: the out-degree that every row of
// the tile with an in-edge has, or kShapeMixed when they differ (or no row has one, or the degree
// does not fit below it).  Rows without an in-edge do not count: the pass can never find them, so
// it never uses their degree -- the rows past the last vertex (the owned range is padded to 64)
// and a run of out-edge-only rows behind the last live one are such rows.
__global__ void k_tile_shape(const int64_t* trp, const uint32_t* odeg, int64_t n, int64_t ntiles, uint32_t* shape) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t t = wave; t < ntiles; t += nwaves) {
    bool wide = false, has[2];
    uint32_t o[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int64_t d = t * 128 + lane + 64 * h;
      const int64_t ind = d < n ? trp[d + 1] - trp[d] : 0;
      wide = wide || ind >= 3;
      has[h] = ind > 0;
      o[h] = has[h] ? odeg[d] : 0u;
    }
    // the degree of the tile's first row with an in-edge; none: mixed
    const unsigned long long b0 = __ballot(has[0]), b1 = __ballot(has[1]);
    uint32_t d0 = kShapeMixed;
    if (b0) d0 = uint32_t(__shfl(int(o[0]), __ffsll((long long)b0) - 1));
    else if (b1) d0 = uint32_t(__shfl(int(o[1]), __ffsll((long long)b1) - 1));
    const bool mixed = (has[0] && o[0] != d0) || (has[1] && o[1] != d0);
    const bool w = __ballot(wide) != 0ull, m = __ballot(mixed) != 0ull || d0 >= kShapeMixed;
    if (lane == 0) shape[t] = (w ? kShapeWide : 0u) | (m ? kShapeMixed : d0);
  }
}
// out[0] uniform tiles, out[1] two-slot tiles, out[2] tiles that are both, out[3] uniform tiles of
// out-degree 0, among the first nt tiles
__global__ void k_shape_count(const uint32_t* shape, int64_t nt, unsigned long long* out) {
  unsigned long long a[4] = {0, 0, 0, 0};
  for (int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; t < nt; t += int64_t(gridDim.x) * blockDim.x) {
    const uint32_t s = shape[t];
    const bool uni = (s & kShapeMixed) != kShapeMixed, two = !(s & kShapeWide);
    a[0] += uni, a[1] += two, a[2] += uni && two, a[3] += (s & kShapeMixed) == 0u;
  }
  for (int k = 0; k < 4; k++) {
    for (int o = 32; o > 0; o >>= 1) a[k] += (unsigned long long)__shfl_xor((long long)a[k], o);
    if ((threadIdx.x & 63) == 0 && a[k]) atomicAdd(out + k, a[k]);
  }
}

// rest records (EdgeSpace::brec): row d's start and clamped in-degree, then its first
// kRecEntries entries of src, as one 64-byte line (four 16-byte stores)
__global__ void k_build_rec(const int64_t* trp, const int32_t* src, int64_t n, uint4* rec) {
  for (int64_t d = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; d < n; d += int64_t(gridDim.x) * blockDim.x) {
    const int64_t b = trp[d], e = trp[d + 1];
    const uint64_t deg = uint64_t(e - b) < 65535u ? uint64_t(e - b) : 65535u;
    uint32_t w[16];
    w[0] = uint32_t(uint64_t(b));
    w[1] = uint32_t(uint64_t(b) >> 32) | uint32_t(deg << 16);
#pragma unroll
    for (int k = 0; k < kRecEntries; k++) w[2 + k] = b + k < e ? uint32_t(src[b + k]) : 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 4; j++) rec[size_t(d) * 4 + j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
  }
}

std::array<long long, 2> minmax_w(Ctx& c, const void* data, int width, int64_t n) {
  DevWords<long long, 2> mm;
  mm.set(c, {LLONG_MAX, LLONG_MIN});
  if (n) k_minmax_w<<<grid_for(n), 256, 0, c.stream>>>(data, width, n, mm.dev());
  return mm.read(c);
}

void build_out_degrees(Ctx& c, EdgeSpace& es, const uint8_t* row_ok, unsigned int* dmax) {
  // padded to whole 128-row tiles (k_bu_lean loads two rows per lane without bounds checks)
  const int64_t n = es.out.n_rows, n_pad = (n + 127) / 128 * 128;
  es.odeg.alloc(size_t(n_pad + 1) * 4);
  NBG_HIP(hipMemsetAsync(es.odeg.p, 0, size_t(n_pad + 1) * 4, c.stream));
  k_out_deg<<<grid_for(n), 256, 0, c.stream>>>(es.out.row_ptr.as<int64_t>(), row_ok, n, es.odeg.as<uint32_t>(), dmax);
}

void row_part_by_hash(Ctx& c, const int64_t* vids, int64_t n, int32_t* row_part) {
  k_row_part_default<<<grid_for(n), 256, 0, c.stream>>>(vids, n, c.num_parts, row_part);
}

// Transpose of the out CSR for bottom-up hops: rows = owned dst, entries = global src index,
// plus copies of the INT-like props in transpose order.  With several ranks every out-edge is
// shipped to the owner of its dst (one build-time all-to-all), so each rank can run bottom-up
// hops over its own vertices against the allgathered frontier bitmap.
//
// Inside a row the sources are ordered hub-first (descending out-degree): in a dense frontier
// the first in-neighbour checked is then almost always a frontier member, and the first K
// entries of every row are copied into a slot-major slab, so the common case of a bottom-up hop
// reads 4 coalesced bytes per row instead of one scattered cache line per row.
struct TransposeBuild {
  Ctx& c;
  EdgeSpace& es;
  Csr& o;
  Csr& t;
  const int64_t m, lo, n_own;
  const int G;
  DevBuf gdeg;                       // world > 1: every rank's out-degrees
  const uint32_t* gdegp = nullptr;   // out-degrees of the gidx space
  uint32_t maxd = 0;
  // the transposed edge list, in the order the props come in: tdst (local row), tsrc (global)
  DevBuf tdst, tsrc;
  int64_t R = 0;
  std::vector<const PropCol*> cp;    // the out props copied into the transpose (else null)
  std::vector<DevBuf> rprops;        // world > 1: received prop columns
  std::vector<const void*> psrc;     // where prop f of the list is read from
  DevBuf perm;                       // list position of every transposed entry

  TransposeBuild(Ctx& ctx, EdgeSpace& e)
      : c(ctx), es(e), o(e.out), t(e.tr), m(e.out.nnz), lo(ctx.owned_lo()), n_own(ctx.owned_hi() - ctx.owned_lo()),
        G(ctx.world), rprops(e.out.props.size()), psrc(e.out.props.size(), nullptr) {
    for (const PropCol& p : o.props) cp.push_back(copy_prop(p) ? &p : nullptr);
  }

  // out-degrees (0 for rows outside hash(vid)'s part) of every vertex of the gidx space
  void out_degrees() {
    const int64_t n_pad = (n_own + 127) / 128 * 128;
    DevWords<unsigned int, 4> dmax;
    dmax.zero(c);
    build_out_degrees(c, es, o.row_ok.as<uint8_t>(), dmax.dev());
    es.odeg8.alloc(size_t(n_pad + 64));
    k_odeg8<<<grid_for(n_pad + 1), 256, 0, c.stream>>>(es.odeg.as<uint32_t>(), n_pad + 1, es.odeg8.as<uint8_t>());
    gdegp = es.odeg.as<uint32_t>();
    if (G > 1) {
      gdeg.alloc(size_t(c.n_global + 1) * 4);
      std::vector<size_t> rb(static_cast<size_t>(G)), ro(static_cast<size_t>(G));
      for (int p = 0; p < G; p++) {
        rb[size_t(p)] = size_t(c.base[size_t(p) + 1] - c.base[size_t(p)]) * 4;
        ro[size_t(p)] = size_t(c.base[size_t(p)]) * 4;
      }
      comm_allgatherv_bytes(c, es.odeg.p, size_t(n_own) * 4, gdeg.p, rb.data(), ro.data());
      gdegp = gdeg.as<uint32_t>();
    }
    maxd = dmax.read(c)[0];
    es.max_odeg = int64_t(maxd);
    if (G > 1) maxd = UINT32_MAX;  // other ranks' degrees may exceed the local maximum
  }

  // src row of every out entry
  DevBuf edge_sources() {
    DevBuf esrc;
    esrc.alloc(size_t(m + 1) * 4);
    if (m) k_edge_src<<<grid_for(o.n_rows), 256, 0, c.stream>>>(o.row_ptr.as<int64_t>(), o.n_rows, esrc.as<int32_t>());
    return esrc;
  }
  // one rank: the out entries as they stand
  void transposed_edges_local() {
    R = m;
    tsrc = edge_sources();  // lo == 0: local == global
    tdst.alloc(size_t(m + 1) * 4);
    if (m) NBG_HIP(hipMemcpyAsync(tdst.p, o.col.p, size_t(m) * 4, hipMemcpyDeviceToDevice, c.stream));
    for (size_t f = 0; f < cp.size(); f++) psrc[f] = cp[f] ? cp[f]->data.p : nullptr;
  }
  // several ranks: ship every out-edge to its dst's owner: sort by dst gidx, cut at the owner bases
  void transposed_edges_exchange() {
    DevBuf esrc = edge_sources();
    DevBuf keysB, iota, sperm;
    keysB.alloc(size_t(m + 1) * 4);
    iota.alloc(size_t(m + 1) * 4);
    sperm.alloc(size_t(m + 1) * 4);
    if (m) {
      k_iota_u32<<<grid_for(m), 256, 0, c.stream>>>(iota.as<uint32_t>(), m);
      radix_pairs<uint32_t, uint32_t>(c, o.col.as<uint32_t>(), keysB.as<uint32_t>(), iota.as<uint32_t>(),
                                      sperm.as<uint32_t>(), m, bits_for(c.n_global));
    }
    iota.release();
    DevBuf dbase, dcut;
    dbase.alloc(size_t(G + 1) * 8);
    dcut.alloc(size_t(G + 1) * 8);
    NBG_HIP(hipMemcpyAsync(dbase.p, c.base.data(), size_t(G + 1) * 8, hipMemcpyHostToDevice, c.stream));
    k_sorted_bounds<<<1, 64, 0, c.stream>>>(keysB.as<uint32_t>(), m, dbase.as<int64_t>(), G + 1, dcut.as<int64_t>());
    std::vector<int64_t> cut(static_cast<size_t>(G + 1));
    NBG_HIP(hipMemcpyAsync(cut.data(), dcut.p, size_t(G + 1) * 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    cut[size_t(G)] = m;
    DevBuf ssrc;
    ssrc.alloc(size_t(m + 1) * 4);
    if (m) k_src_global<<<grid_for(m), 256, 0, c.stream>>>(sperm.as<uint32_t>(), esrc.as<int32_t>(), m, lo, ssrc.as<int32_t>());
    esrc.release();
    // every rank's send counts to every rank
    const size_t ng = static_cast<size_t>(G);
    std::vector<int64_t> mine(ng);
    for (size_t h = 0; h < ng; h++) mine[h] = cut[h + 1] - cut[h];
    const std::vector<int64_t> all = allgather_i64(c, mine);
    std::vector<int64_t> roff(ng + 1, 0);
    for (size_t p = 0; p < ng; p++) roff[p + 1] = roff[p] + all[p * ng + size_t(c.rank)];
    R = roff[ng];
    auto exchange = [&](const void* send, void* recv, int w) {
      std::vector<size_t> sb(ng), so(ng), rb(ng), ro(ng);
      for (size_t p = 0; p < ng; p++) {
        sb[p] = size_t(mine[p]) * size_t(w);
        so[p] = size_t(cut[p]) * size_t(w);
        rb[p] = size_t(roff[p + 1] - roff[p]) * size_t(w);
        ro[p] = size_t(roff[p]) * size_t(w);
      }
      comm_alltoallv_bytes(c, send, sb.data(), so.data(), recv, rb.data(), ro.data());
    };
    DevBuf rdst;
    tsrc.alloc(size_t(R + 1) * 4);
    rdst.alloc(size_t(R + 1) * 4);
    exchange(ssrc.p, tsrc.p, 4);
    exchange(keysB.p, rdst.p, 4);
    tdst.alloc(size_t(R + 1) * 4);
    if (R) k_sub_lo<<<grid_for(R), 256, 0, c.stream>>>(rdst.as<int32_t>(), R, lo, tdst.as<uint32_t>());
    for (size_t f = 0; f < o.props.size(); f++) {
      if (!cp[f]) continue;
      int w = cp[f]->width;
      DevBuf sp;
      sp.alloc(size_t(m + 1) * size_t(w));
      rprops[f].alloc(size_t(R + 1) * size_t(w));
      if (m) gather_width(c, cp[f]->data.p, sperm.as<uint32_t>(), sp.p, m, w);
      exchange(sp.p, rprops[f].p, w);
      psrc[f] = rprops[f].p;
    }
    NBG_HIP(hipStreamSynchronize(c.stream));
  }

  // order: stable sort by hub key, then stable sort by row -> rows hub-first; emits t's row_ptr,
  // col and prop columns
  void hub_first_order() {
    t.n_rows = n_own;
    t.nnz = R;
    t.props.clear();
    for (const PropCol& p : o.props) {
      PropCol q;
      q.name = p.name;
      q.type = p.type;
      q.width = p.width;
      t.props.push_back(std::move(q));
    }
    t.row_ptr.alloc(size_t(t.n_rows + 1) * 8);
    t.col.alloc(size_t(R) * 4 + 64);  // padded: the rest passes load whole aligned 16-byte groups
    perm.alloc(size_t(R + 1) * 4);
    if (R) {
      DevBuf key, keyS, iota, perm1;
      key.alloc(size_t(R) * 4);
      keyS.alloc(size_t(R) * 4);
      iota.alloc(size_t(R) * 4);
      perm1.alloc(size_t(R) * 4);
      k_hub_key<<<grid_for(R), 256, 0, c.stream>>>(tsrc.as<int32_t>(), R, gdegp, maxd, key.as<uint32_t>());
      k_iota_u32<<<grid_for(R), 256, 0, c.stream>>>(iota.as<uint32_t>(), R);
      radix_pairs<uint32_t, uint32_t>(c, key.as<uint32_t>(), keyS.as<uint32_t>(), iota.as<uint32_t>(),
                                      perm1.as<uint32_t>(), R, G > 1 ? 32 : bits_for(int64_t(maxd) + 1));
      iota.release();
      gather<uint32_t>(c, tdst.as<uint32_t>(), perm1.as<uint32_t>(), key.as<uint32_t>(), R);
      radix_pairs<uint32_t, uint32_t>(c, key.as<uint32_t>(), keyS.as<uint32_t>(), perm1.as<uint32_t>(),
                                      perm.as<uint32_t>(), R, bits_for(n_own));
      gather<int32_t>(c, tsrc.as<int32_t>(), perm.as<uint32_t>(), t.col.as<int32_t>(), R);
      rowptr_from_sorted(c, keyS.as<uint32_t>(), R, t.n_rows, t.row_ptr.as<int64_t>());
    } else {
      NBG_HIP(hipMemsetAsync(t.row_ptr.p, 0, size_t(t.n_rows + 1) * 8, c.stream));
    }
    tsrc.release();
    tdst.release();
    for (size_t f = 0; f < o.props.size(); f++) {
      if (!cp[f]) continue;
      int w = cp[f]->width;
      t.props[f].data.alloc(size_t(R) * size_t(w) + 16);
      if (R) gather_width(c, psrc[f], perm.as<uint32_t>(), t.props[f].data.p, R, w);
      rprops[f].release();
    }
    if (G == 1) {
      es.t_eid = std::move(perm);
      es.has_t_eid = true;
    } else {
      es.has_t_eid = false;
    }
  }

  // the column the bottom-up first pass reads (k_bu_lean), packed with the quantised bucket of
  // the first INT-like transposed prop when the gidx leaves >= 3 spare bits below bit 31
  void pack_quantised() {
    es.q_field = -1;
    es.q_gbits = es.q_bits = 0;
    es.tcol_q.release();
    if (R <= 0) return;
    // 2^gb > n_global: an empty slot (-1) decodes to gidx 2^gb - 1, past every vertex.  Its bitmap
    // probe is out of bounds (and answers 0) unless n_global > 2^gb - 32; then it is in bounds
    // (n_global = 2^gb - 1: bit 31 of the last word) and reads a bit no vertex owns, which no
    // frontier bitmap ever has set: the start bitmap and the top-down marks set bits of real gidx
    // only, and a bottom-up hop finds a row only through a set bit, so the pad rows of the last
    // tile (all slots empty) stay unfound (k_bu_lean, k_bu_fin and k_bu_rest_lean rely on it)
    const int gb = bits_for(c.n_global + 1);
    const int qb = std::min(8, 31 - gb);
    int f = -1;
    for (size_t i = 0; i < t.props.size() && f < 0; i++)
      if (t.props[i].data.p) f = int(i);
    if (qb < 3 || f < 0) return;
    const PropCol& pc = t.props[size_t(f)];
    const auto h = minmax_w(c, pc.data.p, pc.width, R);
    es.q_field = f;
    es.q_gbits = gb;
    es.q_bits = qb;
    es.q_min = h[0];
    es.q_range = uint64_t(h[1]) - uint64_t(h[0]) + 1;  // 0 = the whole 2^64 range
    es.tcol_q.alloc(size_t(R) * 4 + 64);
    k_pack_col<<<grid_for(R), 256, 0, c.stream>>>(t.col.as<int32_t>(), pc.data.p, pc.width, R, es.q_min, es.q_range, gb,
                                                  qb, es.tcol_q.as<int32_t>());
    NBG_HIP(hipGetLastError());
  }
  const int32_t* first_pass_col() const { return es.q_field >= 0 ? es.tcol_q.as<int32_t>() : t.col.as<int32_t>(); }

  // the quad slab of the bottom-up first pass and tile_wide
  void pair_slab() {
    // padded to whole 128-row tiles with empty slots (-1)
    const int64_t n_pad = (n_own + 127) / 128 * 128;
    for (int h = 0; h < 2; h++) {
      es.pair_col[h].alloc(size_t(n_pad) * 8 + 16);
      NBG_HIP(hipMemsetAsync(es.pair_col[h].as<uint8_t>() + size_t(n_own) * 8, 0xff, size_t(n_pad - n_own) * 8 + 16,
                             c.stream));
    }
    if (n_own)
      k_build_pair<int32_t><<<grid_for(n_own), 256, 0, c.stream>>>(t.row_ptr.as<int64_t>(), first_pass_col(), n_own,
                                                                   es.pair_col[0].as<int32_t>(),
                                                                   es.pair_col[1].as<int32_t>(), -1);
    // one bit per tile: some row of it has a third entry (from the row_ptr the slab was cut from,
    // so exact whatever the numbering); a word of padding past the last tile's, k_bu_fin reads
    // its next tile's word ahead
    const int64_t nt = n_pad / 128;
    es.tile_wide.alloc(size_t(nt / 32 + 2) * 4);
    NBG_HIP(hipMemsetAsync(es.tile_wide.p, 0, size_t(nt / 32 + 2) * 4, c.stream));
    if (n_own)
      k_tile_wide<<<grid_for(n_own), 256, 0, c.stream>>>(t.row_ptr.as<int64_t>(), n_own, es.tile_wide.as<uint32_t>());
    // the non-final first pass's word per tile (wide bit + common out-degree), two words of
    // padding (wide, mixed): k_bu_lean reads its next tile's word ahead
    es.tile_shape.alloc(size_t(nt + 2) * 4);
    NBG_HIP(hipMemsetAsync(es.tile_shape.p, 0xff, size_t(nt + 2) * 4, c.stream));
    if (n_own)
      k_tile_shape<<<grid_for(nt * 64), 256, 0, c.stream>>>(t.row_ptr.as<int64_t>(), es.odeg.as<uint32_t>(), n_own, nt,
                                                           es.tile_shape.as<uint32_t>());
  }
  // the shares of the non-final first pass's tiles (byte model); a uniform tile of out-degree 0
  // below bu_both_tiles -- which the class-ordered numbering rules out, and a stale numbering is
  // not known to produce -- turns the shape words off for this edge space
  void shape_shares() {
    DevWords<unsigned long long, 4> sc;
    sc.zero(c);
    if (es.bu_both_tiles > 0)
      k_shape_count<<<grid_for(es.bu_both_tiles), 256, 0, c.stream>>>(es.tile_shape.as<uint32_t>(), es.bu_both_tiles,
                                                                      sc.dev());
    const auto h = sc.read(c);
    for (int k = 0; k < 3; k++) es.shape_tiles[k] = int64_t(h[size_t(k)]);
    if (h[3]) {
      es.tile_shape.release();
      es.shape_tiles[0] = es.shape_tiles[1] = es.shape_tiles[2] = 0;
    }
  }
  // exact row bounds of the bottom-up hops: past the last row with an in-edge nothing can be
  // found (final hop), past the last one with an in-edge and an out-edge nothing can extend
  // the next frontier (non-final hops); the class-ordered numbering makes both short prefixes
  void live_bounds() {
    DevWords<unsigned long long, 2> lb;
    lb.zero(c);
    if (n_own)
      k_live_bounds<<<grid_for(n_own), 256, 0, c.stream>>>(t.row_ptr.as<int64_t>(), es.odeg.as<uint32_t>(), n_own,
                                                           lb.dev());
    const auto h = lb.read(c);
    es.bu_in_tiles = int64_t((h[0] + 127) / 128);
    es.bu_both_tiles = int64_t((h[1] + 127) / 128);
  }
  // rest records for the rows a bottom-up hop reads (bu_rec_mb: at most that many MiB, else
  // the rest pass reads row_ptr and the columns)
  void rest_records() {
    es.brec.release();
    es.brec_rows = 0;
    const int64_t rows = std::min(n_own, es.bu_in_tiles * 128);
    const int64_t cap_mb = c.opt("bu_rec_mb", 8192);
    if (rows > 0 && c.opt("bu_rec", 1) != 0 && rows * 64 <= (cap_mb << 20)) {
      es.brec.alloc(size_t(rows) * 64);
      k_build_rec<<<grid_for(rows), 256, 0, c.stream>>>(t.row_ptr.as<int64_t>(), first_pass_col(), rows,
                                                        es.brec.as<uint4>());
      NBG_HIP(hipGetLastError());
      es.brec_rows = rows;
    }
  }
};

void build_transpose(Ctx& c, EdgeSpace& es) {
  TransposeBuild b(c, es);
  b.out_degrees();
  if (b.G == 1) b.transposed_edges_local();
  else b.transposed_edges_exchange();
  b.hub_first_order();
  for (int h = 0; h < 2; h++) es.pair_col[h].release();
  es.tile_wide.release();
  es.tile_shape.release();
  b.pack_quantised();
  b.pair_slab();
  b.live_bounds();
  b.shape_shares();
  b.rest_records();
  NBG_HIP(hipStreamSynchronize(c.stream));
  NBG_HIP(hipGetLastError());
  es.has_tr = true;
}

}  // namespace nbg
