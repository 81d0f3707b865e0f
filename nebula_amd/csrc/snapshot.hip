// snapshot.hip -- snapshot builder: reference KV bytes (or synthetic RMAT tuples) -> GPU CSR.
//
// Stage 1 (decode, per loaded part): one thread per KV pair parses the 40-byte edge key
//   (NebulaKeyUtils.h:14-21: part i32 | src i64 | type i32 | rank i64 | dst i64 | ver i64, LE)
//   and, for out-edges, the RowWriter row (RowWriter.cpp:49-75: header byte, schema version,
//   block offsets every 16 fields, INT = LEB128 varint, VID/TIMESTAMP 8 B, DOUBLE 8 B, FLOAT
//   4 B, BOOL 1 B, STRING varint length + bytes).  Field offsets follow RowReader::skipToField
//   (RowReader.cpp:276-368), including the stored block offsets.  Output: SoA tuples.
// Stage 2 (finalize): vertex set, vid<->gidx map, sort each rank's tuples into the reference's
//   key order, keep the bytewise-first version of every (src, rank, dst)
//   (QueryBaseProcessor.inl:349-362, P3), emit CSR + narrowed SoA property columns.
//
// This file holds staging and decode, the load / write / commit entry points, the RMAT tuple
// generator, the vertex map (numbering, hash table, bytewise ranks), the tag columns and the
// finalize and merge-commit drivers.  The CSR and transpose builders are in csr_build.hip, the
// streamed RMAT build in rmat_stream.hip; build_common.h declares what crosses the three.
#include <algorithm>
#include <numeric>

#include "build_common.h"

namespace nbg {

constexpr int kMaxFields = 64;
struct SchemaDev {
  int32_t nfields;
  int32_t types[kMaxFields];
};

// the context's build-time block cache (option build_pool_gb, 0 = plain hipMalloc / hipFree)
static std::shared_ptr<BufPool> build_pool(Ctx& c) {
  const int64_t gb = c.opt("build_pool_gb", 128);
  if (gb <= 0) return nullptr;
  c.build_pool->limit = size_t(gb) << 30;
  return c.build_pool;
}

__global__ void k_hash_part(const int64_t* src, int32_t* part, int64_t n, int32_t parts) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    part[i] = int32_t(uint64_t(src[i]) % uint64_t(parts) + 1);
}

// A device-generated stage (snapshot_gen_rmat) keeps rank / version as constants, the key part
// implicit (hash rule), no sequence numbers and no present bytes.  Before decoded KV tuples are
// appended behind it (a write batch), spell those columns out: the generated tuples precede every
// later write (sequence 0), their part is the hash part of the key's vertex.
static void materialize_stage(Ctx& c, Staging& s, size_t nfields, bool with_props) {
  if (s.n == 0 || s.seq.p) return;
  const int64_t n = s.n;
  const size_t cap = std::max(s.cap, size_t(n));
  s.rank.alloc(cap * 8);
  s.ver.alloc(cap * 8);
  s.part.alloc(cap * 4);
  s.seq.alloc(cap * 8);
  fill<int64_t>(c, s.rank.as<int64_t>(), s.rank_value, n);
  fill<int64_t>(c, s.ver.as<int64_t>(), s.ver_value, n);
  fill<int64_t>(c, s.seq.as<int64_t>(), 0, n);
  k_hash_part<<<grid_for(n), 256, 0, c.stream>>>(s.src.as<int64_t>(), s.part.as<int32_t>(), n, c.num_parts);
  NBG_HIP(hipGetLastError());
  if (with_props) {
    s.present.resize(std::max(s.present.size(), nfields));
    for (size_t f = 0; f < nfields; f++)
      if (!s.present[f].p) {
        s.present[f].alloc(cap);
        fill<uint8_t>(c, s.present[f].as<uint8_t>(), 1, n);
      }
  }
  s.rank_const = s.ver_const = false;
  s.cap = cap;
  c.load_seq = std::max<int64_t>(c.load_seq, 1);
  NBG_HIP(hipStreamSynchronize(c.stream));
}

static void stage_reserve(Ctx& c, Staging& s, size_t nfields, size_t extra, bool with_props,
                          const std::vector<Field>& fields) {
  materialize_stage(c, s, nfields, with_props);
  size_t need = size_t(s.n) + extra;
  if (need <= s.cap) return;
  // 1.25x growth: a write batch appended behind a device-sized stage must not double it
  size_t cap = std::max(need, s.cap + s.cap / 4);
  grow_copy(c, s.src, cap * 8, true);
  grow_copy(c, s.dst, cap * 8, true);
  grow_copy(c, s.rank, cap * 8, true);
  grow_copy(c, s.ver, cap * 8, true);
  grow_copy(c, s.part, cap * 4, true);
  grow_copy(c, s.seq, cap * 8, true);
  if (with_props) {
    s.props.resize(nfields);
    s.present.resize(nfields);
    s.str_len.resize(nfields);
    for (size_t f = 0; f < nfields; f++) {
      grow_copy(c, s.props[f], cap * 8, true);
      grow_copy(c, s.present[f], cap, true);
      if (fields[f].type == NBG_T_STRING) grow_copy(c, s.str_len[f], cap * 8, true);
    }
  }
  s.cap = cap;
}

// ------------------------------------------------------------------------------------------
// Stage 1a: KV decode
// ------------------------------------------------------------------------------------------
struct StageOut {
  int32_t* part;
  int64_t* src;
  int64_t* dst;
  int64_t* rank;
  int64_t* ver;
  int64_t* seq;
  int64_t* props[kMaxFields];
  uint8_t* present[kMaxFields];
  int64_t* str_len[kMaxFields];
};

template <typename T>
__device__ inline T ld_unaligned(const uint8_t* p) {
  T v;
  __builtin_memcpy(&v, p, sizeof(T));
  return v;
}

__device__ inline int dev_varint(const uint8_t* p, int64_t avail, uint64_t& out) {
  uint64_t v = 0;
  for (int i = 0; i < 10 && i < avail; i++) {
    v |= uint64_t(p[i] & 0x7f) << (7 * i);
    if (!(p[i] & 0x80)) {
      out = v;
      return i + 1;
    }
  }
  return -1;
}

// Decodes one row into field slots.  Mirrors RowReader: header (RowReader.cpp:218-263),
// sequential skip (skipToNext :276-341), stored block offsets for fields 16k (:239-249).
__device__ void decode_row(const uint8_t* row, int64_t len, const SchemaDev& sch, int64_t heap_off,
                           const StageOut& o, int64_t slot, unsigned long long* err) {
  int nf = sch.nfields;
  if (len <= 0) {
    for (int f = 0; f < nf; f++) o.present[f][slot] = 0;
    return;
  }
  uint8_t h = row[0];
  int offBytes = (h & 7) + 1;
  int verBytes = h >> 5;
  int numOffsets = nf >> 4;
  int64_t hdr = 1 + verBytes + int64_t(offBytes) * numOffsets;
  if (hdr > len) {  // "Rowe data is too short": reader is invalid, no props
    for (int f = 0; f < nf; f++) o.present[f][slot] = 0;
    atomicAdd(err, 1ull);
    return;
  }
  const uint8_t* data = row + hdr;
  int64_t dlen = len - hdr;
  int64_t pos = 0;
  bool broken = false;
  for (int f = 0; f < nf; f++) {
    if (f > 0 && (f & 15) == 0) {
      int64_t bo = 0;
      const uint8_t* ob = row + 1 + verBytes + int64_t(offBytes) * ((f >> 4) - 1);
      for (int j = 0; j < offBytes; j++) bo |= int64_t(uint64_t(ob[j]) << (8 * j));
      pos = bo;
      broken = false;
    }
    int64_t v = 0;
    int64_t next = -1;
    if (!broken && pos >= 0 && pos <= dlen) {
      switch (sch.types[f]) {
        case NBG_T_BOOL:
          if (pos + 1 <= dlen) { v = data[pos] != 0; next = pos + 1; }
          break;
        case NBG_T_INT: {
          uint64_t u;
          int n = dev_varint(data + pos, dlen - pos, u);
          if (n > 0) { v = int64_t(u); next = pos + n; }
          break;
        }
        case NBG_T_VID:
        case NBG_T_TIMESTAMP:
          if (pos + 8 <= dlen) { v = ld_unaligned<int64_t>(data + pos); next = pos + 8; }
          break;
        case NBG_T_FLOAT:
          if (pos + 4 <= dlen) {
            double d = double(ld_unaligned<float>(data + pos));
            v = __double_as_longlong(d);
            next = pos + 4;
          }
          break;
        case NBG_T_DOUBLE:
          if (pos + 8 <= dlen) { v = ld_unaligned<int64_t>(data + pos); next = pos + 8; }
          break;
        case NBG_T_STRING: {
          uint64_t sl;
          int n = dev_varint(data + pos, dlen - pos, sl);
          if (n > 0 && pos + n + int64_t(sl) <= dlen) {
            v = heap_off + hdr + pos + n;
            o.str_len[f][slot] = int64_t(sl);
            next = pos + n + int64_t(sl);
          }
          break;
        }
        default: break;
      }
    }
    if (next < 0) {
      broken = true;
      o.present[f][slot] = 0;
      o.props[f][slot] = 0;
    } else {
      o.present[f][slot] = 1;
      o.props[f][slot] = v;
      pos = next;
    }
  }
}

__global__ void k_decode_kv(const uint8_t* __restrict__ kb, const uint64_t* __restrict__ koff,
                            const uint8_t* __restrict__ vb, const uint64_t* __restrict__ voff,
                            int64_t n, int32_t etype, int32_t sver, SchemaDev sch, int64_t heap_base,
                            int64_t seq0, StageOut outS, unsigned long long* out_cnt, StageOut inS,
                            unsigned long long* in_cnt, unsigned long long* err, int32_t req_part, int32_t parts,
                            int32_t world, int32_t my_rank) {
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  int64_t n_rounds = (n + stride - 1) / stride;
  for (int64_t r = 0; r < n_rounds; r++) {
    int64_t i = r * stride + blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    bool is_out = false, is_in = false;
    int64_t src = 0, dst = 0, rank = 0, ver = 0;
    int32_t kpart = 0;
    if (i < n) {
      uint64_t k0 = koff[i], k1 = koff[i + 1];
      if (k1 - k0 == 40) {
        const uint8_t* k = kb + k0;
        int32_t type = ld_unaligned<int32_t>(k + 12);
        if (type == etype || type == -etype) {
          kpart = ld_unaligned<int32_t>(k);
          src = ld_unaligned<int64_t>(k + 4);
          rank = ld_unaligned<int64_t>(k + 16);
          dst = ld_unaligned<int64_t>(k + 24);
          ver = ld_unaligned<int64_t>(k + 32);
          is_out = type == etype;
          is_in = !is_out;
          // a part holds only keys of its own prefix, and with several ranks this rank can only
          // host rows of the vertices it owns (err[2]: the whole batch is refused)
          if (kpart != req_part || (world > 1 && dev_owner(src, parts, world) != my_rank)) atomicAdd(err + 2, 1ull);
        }
      }
    }
    int64_t so = wave_append(out_cnt, is_out);
    int64_t si = wave_append(in_cnt, is_in);
    if (is_out) {
      outS.part[so] = kpart;
      outS.src[so] = src;
      outS.dst[so] = dst;
      outS.rank[so] = rank;
      outS.ver[so] = ver;
      outS.seq[so] = seq0 + i;
      uint64_t v0 = voff[i], v1 = voff[i + 1];
      const uint8_t* row = vb + v0;
      int64_t len = int64_t(v1 - v0);
      if (len > 0) {
        // schema version from the row header (RowReader.cpp:173-199)
        int verBytes = row[0] >> 5;
        int32_t rv = 0;
        if (verBytes > 0 && verBytes + 1 <= len)
          for (int b = 0; b < verBytes; b++) rv |= int32_t(uint32_t(row[1 + b]) << (8 * b));
        if (rv != sver) atomicAdd(err + 1, 1ull);
      }
      decode_row(row, len, sch, heap_base + int64_t(v0), outS, so, err);
    }
    if (is_in) {
      inS.part[si] = kpart;
      inS.src[si] = src;
      inS.dst[si] = dst;
      inS.rank[si] = rank;
      inS.ver[si] = ver;
      inS.seq[si] = seq0 + i;
    }
  }
}

// Vertex keys (NebulaKeyUtils.h:14-17: part i32 | vid i64 | tag i32 | ver i64, 24 bytes) of one
// tag -> staged (vid, ver, part, load sequence) + decoded row fields.
__global__ void k_decode_vkv(const uint8_t* __restrict__ kb, const uint64_t* __restrict__ koff,
                             const uint8_t* __restrict__ vb, const uint64_t* __restrict__ voff, int64_t n,
                             int32_t tag, int32_t sver, SchemaDev sch, int64_t heap_base, int64_t seq0,
                             StageOut o, unsigned long long* cnt, unsigned long long* err, int32_t req_part) {
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  int64_t n_rounds = (n + stride - 1) / stride;
  for (int64_t r = 0; r < n_rounds; r++) {
    int64_t i = r * stride + blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    bool hit = false;
    if (i < n && koff[i + 1] - koff[i] == 24) hit = ld_unaligned<int32_t>(kb + koff[i] + 12) == tag;
    int64_t so = wave_append(cnt, hit);
    if (!hit) continue;
    const uint8_t* k = kb + koff[i];
    if (ld_unaligned<int32_t>(k) != req_part) atomicAdd(err + 2, 1ull);
    o.part[so] = ld_unaligned<int32_t>(k);
    o.src[so] = ld_unaligned<int64_t>(k + 4);
    o.ver[so] = ld_unaligned<int64_t>(k + 16);
    o.seq[so] = seq0 + i;
    const uint8_t* row = vb + voff[i];
    int64_t len = int64_t(voff[i + 1] - voff[i]);
    if (len > 0) {
      int verBytes = row[0] >> 5;
      int32_t rv = 0;
      if (verBytes > 0 && verBytes + 1 <= len)
        for (int b = 0; b < verBytes; b++) rv |= int32_t(uint32_t(row[1 + b]) << (8 * b));
      if (rv != sver) atomicAdd(err + 1, 1ull);
    }
    decode_row(row, len, sch, heap_base + int64_t(voff[i]), o, so, err);
  }
}

static StageOut stage_ptrs(Staging& s, size_t nf) {
  StageOut o{};
  o.part = s.part.as<int32_t>();
  o.src = s.src.as<int64_t>();
  o.dst = s.dst.as<int64_t>();
  o.rank = s.rank.as<int64_t>();
  o.ver = s.ver.as<int64_t>();
  o.seq = s.seq.as<int64_t>();
  for (size_t f = 0; f < nf && f < size_t(kMaxFields); f++) {
    o.props[f] = f < s.props.size() ? s.props[f].as<int64_t>() : nullptr;
    o.present[f] = f < s.present.size() ? s.present[f].as<uint8_t>() : nullptr;
    o.str_len[f] = f < s.str_len.size() ? s.str_len[f].as<int64_t>() : nullptr;
  }
  return o;
}

static void decode_part(Ctx& c, int32_t part, const uint8_t* kb, const uint64_t* koff,
                        const uint8_t* vb, const uint64_t* voff, size_t n) {
  if (part < 0 || part > c.num_parts) throw Error(NBG_E_PART_NOT_FOUND, "part out of range");
  if (owner_of_part(part, c.world) != c.rank)
    throw Error(NBG_E_PART_NOT_FOUND, "part " + std::to_string(part) + " is not owned by this rank");
  if (c.edges.empty() && c.tags.empty()) throw Error(NBG_E_STATE, "no edge or tag schema registered");
  if (n == 0) return;
  double t0 = now_s();
  size_t kbytes = koff[n], vbytes = voff[n];
  DevBuf dk, dko, dvo;
  dk.alloc(kbytes + 8);
  dko.alloc((n + 1) * 8);
  dvo.alloc((n + 1) * 8);
  NBG_HIP(hipMemcpyAsync(dk.p, kb, kbytes, hipMemcpyHostToDevice, c.stream));
  NBG_HIP(hipMemcpyAsync(dko.p, koff, (n + 1) * 8, hipMemcpyHostToDevice, c.stream));
  NBG_HIP(hipMemcpyAsync(dvo.p, voff, (n + 1) * 8, hipMemcpyHostToDevice, c.stream));
  // value bytes go to the string heap (kept until finalize for STRING props)
  int64_t heap_base = int64_t(c.heap_used);
  grow_copy(c, c.heap, c.heap_used + vbytes + 8);
  if (vbytes) NBG_HIP(hipMemcpyAsync(c.heap.as<uint8_t>() + heap_base, vb, vbytes, hipMemcpyHostToDevice, c.stream));
  c.heap_used += vbytes;
  DevBuf cnt;
  cnt.alloc(64);
  // A RocksDB write batch for one part is all or nothing: remember where every stage ended, and
  // on any refusal roll them (and the value heap) back.  The load sequence advances either way,
  // so a later batch never reuses this one's numbers (identical-key order stays unambiguous).
  struct Mark {
    Staging* s;
    int64_t n;
  };
  std::vector<Mark> marks;
  for (auto& kvp : c.edges) {
    marks.push_back(Mark{&kvp.second.out_stage, kvp.second.out_stage.n});
    marks.push_back(Mark{&kvp.second.in_stage, kvp.second.in_stage.n});
  }
  for (auto& kvp : c.tags) marks.push_back(Mark{&kvp.second.stage, kvp.second.stage.n});
  const size_t heap_mark = size_t(heap_base);
  try {
  for (auto& kvp : c.edges) {
    EdgeSpace& es = kvp.second;
    size_t nf = es.fields.size();
    if (nf > size_t(kMaxFields)) throw Error(NBG_E_UNSUPPORTED, "more than 64 edge fields");
    SchemaDev sch{};
    sch.nfields = int32_t(nf);
    for (size_t f = 0; f < nf; f++) sch.types[f] = es.fields[f].type;
    stage_reserve(c, es.out_stage, nf, n, true, es.fields);
    stage_reserve(c, es.in_stage, 0, n, false, es.fields);
    NBG_HIP(hipMemsetAsync(cnt.p, 0, 64, c.stream));
    unsigned long long* d = cnt.as<unsigned long long>();
    NBG_HIP(hipMemcpyAsync(d, &es.out_stage.n, 8, hipMemcpyHostToDevice, c.stream));
    NBG_HIP(hipMemcpyAsync(d + 1, &es.in_stage.n, 8, hipMemcpyHostToDevice, c.stream));
    StageOut so = stage_ptrs(es.out_stage, nf);
    StageOut si = stage_ptrs(es.in_stage, 0);
    k_decode_kv<<<grid_for(int64_t(n)), 256, 0, c.stream>>>(
        dk.as<uint8_t>(), dko.as<uint64_t>(), c.heap.as<uint8_t>() + heap_base, dvo.as<uint64_t>(),
        int64_t(n), es.type, es.schema_ver, sch, heap_base, c.load_seq, so, d, si, d + 1, d + 2, part, c.num_parts,
        c.world, c.rank);
    NBG_HIP(hipGetLastError());
    unsigned long long h[5];
    NBG_HIP(hipMemcpyAsync(h, d, 40, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    // (REVERSELY: KV pairs need not come in out / in pairs, as gen_rmat's tuples do)
    if (int64_t(h[0]) != es.out_stage.n || int64_t(h[1]) != es.in_stage.n) es.kv_loaded = true;
    es.out_stage.n = int64_t(h[0]);  // the marks roll back a refused batch
    es.in_stage.n = int64_t(h[1]);
    if (h[3] != 0)
      throw Error(NBG_E_UNSUPPORTED, "row schema version differs from the registered version");
    if (h[4] != 0)
      throw Error(NBG_E_PART_NOT_FOUND, "edge key of another part, or of a vertex another rank owns");
    es.out_stage.rank_const = es.out_stage.ver_const = false;
    es.in_stage.rank_const = es.in_stage.ver_const = false;
  }
  for (auto& kvp : c.tags) {
    TagSpace& ts = kvp.second;
    size_t nf = ts.fields.size();
    SchemaDev sch{};
    sch.nfields = int32_t(nf);
    for (size_t f = 0; f < nf; f++) sch.types[f] = ts.fields[f].type;
    stage_reserve(c, ts.stage, nf, n, true, ts.fields);
    NBG_HIP(hipMemsetAsync(cnt.p, 0, 64, c.stream));
    unsigned long long* d = cnt.as<unsigned long long>();
    NBG_HIP(hipMemcpyAsync(d, &ts.stage.n, 8, hipMemcpyHostToDevice, c.stream));
    k_decode_vkv<<<grid_for(int64_t(n)), 256, 0, c.stream>>>(
        dk.as<uint8_t>(), dko.as<uint64_t>(), c.heap.as<uint8_t>() + heap_base, dvo.as<uint64_t>(), int64_t(n),
        ts.id, ts.schema_ver, sch, heap_base, c.load_seq, stage_ptrs(ts.stage, nf), d, d + 2, part);
    NBG_HIP(hipGetLastError());
    unsigned long long h[5];
    NBG_HIP(hipMemcpyAsync(h, d, 40, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    ts.stage.n = int64_t(h[0]);
    if (h[3] != 0) throw Error(NBG_E_UNSUPPORTED, "tag row schema version differs from the registered version");
    if (h[4] != 0) throw Error(NBG_E_PART_NOT_FOUND, "vertex key of another part");
  }
  } catch (...) {
    for (auto& m : marks) m.s->n = m.n;
    c.heap_used = heap_mark;
    c.load_seq += int64_t(n);
    throw;
  }
  c.load_seq += int64_t(n);
  c.build_seconds += now_s() - t0;
}

void snapshot_load_part(Ctx& c, int32_t part, const uint8_t* kb, const uint64_t* koff,
                        const uint8_t* vb, const uint64_t* voff, size_t n) {
  PoolScope build_scope(build_pool(c));  // staged tuples
  if (c.finalized) throw Error(NBG_E_STATE, "snapshot already finalized");
  decode_part(c, part, kb, koff, vb, voff, n);
}

// ------------------------------------------------------------------------------------------
// Write path.  AddEdgesProcessor / AddVerticesProcessor turn a request into one
// batch of KV puts per part (AddEdgesProcessor.cpp:15-31, AddVerticesProcessor.cpp:16-38; the
// version in the key is INT64_MAX - now_us, so a newer write of the same edge sorts first and
// an identical key overwrites).  A writable snapshot keeps the decoded tuples of everything
// loaded so far (the stages, read-only to the CSR build: the "log") next to the CSRs; a write
// batch is decoded by the same k_decode_kv /
// k_decode_vkv behind the log with later load sequence numbers, so the CSR build's version
// dedup (bytewise-first key, last write of an identical key) gives exactly what the prefix scan
// of the written RocksDB part returns.  nbg_snapshot_commit rebuilds the vertex map, CSRs,
// transposes and tag columns from the log on the device -- nothing is re-uploaded -- and until
// then queries keep reading the previous commit (a RocksDB snapshot's view).
// ------------------------------------------------------------------------------------------
// drop what build_transpose derives from the out CSRs of every rank
static void reset_transpose_derived(EdgeSpace& es) {
  es.rep_out = Csr();
  es.rep_in = Csr();
  es.has_rep = es.has_rep_out = false;
  es.rep_odeg.release();
  es.tr = Csr();
  es.t_eid.release();
  es.has_tr = es.has_t_eid = false;
  es.out_nnz_global = -1;
  es.tcol_q.release();
  es.q_field = -1;
  es.q_gbits = es.q_bits = 0;
  for (int h = 0; h < 2; h++) es.pair_col[h].release();
  es.tile_wide.release();
  es.tile_shape.release();
  es.odeg.release();
  es.odeg8.release();
  es.max_odeg = -1;
  es.max_odeg_global = -1;
  es.top_deg.clear();
  es.bu_in_tiles = es.bu_both_tiles = 0;
  es.brec.release();
  es.brec_rows = 0;
  es.rev = EdgeSpace::Rev();  // (REVERSELY: in-degrees, their statistics and the mirror state)
}

// drop everything snapshot_finalize derives from the staged tuples
static void reset_edge_derived(EdgeSpace& es) {
  es.out = Csr();
  es.in = Csr();
  reset_transpose_derived(es);
}

static void reset_derived(Ctx& c) {
  c.brank.release();
  for (auto& kv : c.edges)
    for (auto& o : kv.second.ord) {
      o.perm.release();
      o.skey.release();
      o.dstg.release();
      o.n = 0;
    }
  c.vid_of.release();
  c.ht_keys.release();
  c.ht_vals.release();
  c.ht_cap = 0;
  c.ht_has_min = false;
  c.ht_min_gidx = -1;
  c.tag_table.release();
  for (auto& kv : c.edges) reset_edge_derived(kv.second);
  for (auto& kv : c.tags) {
    kv.second.cols.clear();
    kv.second.part.release();
  }
  c.sp_dist[0].release();
  c.sp_dist[1].release();
  c.sp_dist_bytes = 0;
  c.sp_dirty = false;
  c.sp = Ctx::SpWork();
}

// Merge commit: each edge CSR merges its sorted batch into the committed order (build_csr merge
// mode) and the transposed CSR is rebuilt from the new out CSRs.  One rank: new vertices extend
// the numbering (appended gidx) and tag writes rebuild the tag columns.  Several ranks: batches
// of edges and tag rows merge on every rank together; a batch with a new vertex anywhere takes
// the full rebuild (appending to one rank's gidx range would move every later rank's).  Returns
// false when the batch needs the full rebuild.
static bool commit_merge(Ctx& c);

void snapshot_write_part(Ctx& c, int32_t part, const uint8_t* kb, const uint64_t* koff,
                         const uint8_t* vb, const uint64_t* voff, size_t n) {
  PoolScope build_scope(build_pool(c));  // staged tuples
  if (!c.finalized) {  // before the first commit a write batch is one more loaded batch
    decode_part(c, part, kb, koff, vb, voff, n);
    return;
  }
  if (!c.has_log) throw Error(NBG_E_STATE, "snapshot is not writable (set option writable=1 before finalize)");
  decode_part(c, part, kb, koff, vb, voff, n);  // behind the kept tuples; the CSRs are untouched
  c.pending_writes = true;
}

void snapshot_commit(Ctx& c) {
  if (!c.finalized) {
    // first finalize, or a retry after a commit whose rebuild failed half-way (e.g. E_NOMEM):
    // whatever that attempt derived is dropped before building again
    NBG_HIP(hipStreamSynchronize(c.stream));
    reset_derived(c);
    snapshot_finalize(c);
    return;
  }
  if (!c.has_log) throw Error(NBG_E_STATE, "snapshot is not writable (set option writable=1 before finalize)");
  // collective when world > 1: every rank rebuilds, with or without writes of its own
  NBG_HIP(hipStreamSynchronize(c.stream));
  if (commit_merge(c)) {
    c.pending_writes = false;
    c.commits++;
    c.merge_commits++;
    return;
  }
  reset_derived(c);
  c.pending_writes = false;
  c.finalized = false;
  snapshot_finalize(c);
  c.commits++;
}

// ------------------------------------------------------------------------------------------
// Stage 1b: synthetic RMAT (definition in build_common.h, shared with oracle/refcpu.cpp)
// ------------------------------------------------------------------------------------------
__global__ void k_gen_rmat(int64_t lo, int64_t hi, int32_t scale, uint64_t seed, uint64_t smix,
                           int32_t parts, int32_t world, int32_t rank, int64_t* osrc, int64_t* odst,
                           int64_t* oweight, unsigned long long* ocnt, int64_t* isrc, int64_t* idst,
                           unsigned long long* icnt, int64_t cap) {
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  int64_t n = hi - lo;
  int64_t rounds = (n + stride - 1) / stride;
  for (int64_t r = 0; r < rounds; r++) {
    int64_t j = r * stride + blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    bool valid = j < n;
    int64_t s = 0, d = 0;
    if (valid) {
      uint64_t u, v;
      rmat_sample(uint64_t(lo + j), scale, seed, u, v);
      s = rmat_vid(u, smix);
      d = rmat_vid(v, smix);
    }
    bool is_out = valid && (world == 1 || dev_owner(s, parts, world) == rank);
    bool is_in = valid && (world == 1 || dev_owner(d, parts, world) == rank);
    int64_t so = wave_append(ocnt, is_out);
    int64_t si = wave_append(icnt, is_in);
    if (is_out && so < cap) {  // counts keep growing past cap: the host re-runs with the exact size
      osrc[so] = s;
      odst[so] = d;
      oweight[so] = rmat_weight(s, d, seed);
    }
    if (is_in && si < cap) {  // in-edge key (dst, -type, rank, src): key src = d, key dst = s
      isrc[si] = d;
      idst[si] = s;
    }
  }
}

void snapshot_gen_rmat(Ctx& c, int32_t scale, int32_t ef, uint64_t seed, int32_t et) {
  PoolScope build_scope(build_pool(c));  // staged tuples
  if (c.finalized) throw Error(NBG_E_STATE, "snapshot already finalized");
  auto it = c.edges.find(et);
  if (it == c.edges.end()) throw Error(NBG_E_INVALID_ARG, "edge type not registered");
  EdgeSpace& es = it->second;
  if (es.fields.size() != 1 || es.fields[0].type != NBG_T_INT)
    throw Error(NBG_E_INVALID_ARG, "RMAT edge schema must be (weight int)");
  if (scale < 1 || scale > 31 || ef < 1) throw Error(NBG_E_INVALID_ARG, "bad RMAT scale");
  double t0 = now_s();
  int64_t E = int64_t(ef) << scale;
  int64_t expect = !c.sharded ? E : E / c.world + E / (4 * c.world) + (1 << 20);
  Staging& so = es.out_stage;
  Staging& si = es.in_stage;
  if (so.n != 0 || si.n != 0 || es.rmat_stream) throw Error(NBG_E_STATE, "RMAT must be the only source of this edge type");
  // streamed build: forced with rmat_stream = 1, automatic on one rank once the tuple stage
  // would pass its 2^32 cap (2^31 samples and up: two CSR directions of 40+ B tuples)
  const int64_t stream_opt = c.opt("rmat_stream", -1);
  if (!c.sharded && (stream_opt > 0 || (stream_opt < 0 && E >= (int64_t(1) << 31)))) {
    if (c.opt("writable", 0)) throw Error(NBG_E_UNSUPPORTED, "streamed RMAT snapshot is read-only (writable = 1)");
    es.rmat_stream = true;
    es.rmat_scale = scale;
    es.rmat_ef = ef;
    es.rmat_seed = seed;
    return;
  }
  auto alloc_stage = [&](Staging& s, int64_t cap, bool props) {
    s.src.alloc(size_t(cap) * 8);
    s.dst.alloc(size_t(cap) * 8);
    s.rank.release();
    s.ver.release();
    s.part.release();
    s.seq.release();
    s.rank_const = s.ver_const = true;
    s.rank_value = 0;
    s.ver_value = INT64_MAX - 1;
    if (props) {
      s.props.resize(1);
      s.present.resize(1);
      s.str_len.resize(1);
      s.props[0].alloc(size_t(cap) * 8);
      s.present[0].release();  // all present
    }
    s.cap = size_t(cap);
  };
  DevBuf cnt;
  cnt.alloc(16);
  unsigned long long* d = cnt.as<unsigned long long>();
  uint64_t smix = splitmix64(seed) & ((1ull << 63) - 1);
  const int64_t chunk = int64_t(1) << 26;
  unsigned long long h[2];
  for (int attempt = 0; attempt < 2; attempt++) {
    alloc_stage(so, expect, true);
    alloc_stage(si, expect, false);
    NBG_HIP(hipMemsetAsync(cnt.p, 0, 16, c.stream));
    for (int64_t lo = 0; lo < E; lo += chunk) {
      int64_t hi = std::min(E, lo + chunk);
      k_gen_rmat<<<grid_for(hi - lo), 256, 0, c.stream>>>(lo, hi, scale, seed, smix, c.num_parts, c.world,
                                                        c.rank, so.src.as<int64_t>(), so.dst.as<int64_t>(),
                                                        so.props[0].as<int64_t>(), d, si.src.as<int64_t>(),
                                                        si.dst.as<int64_t>(), d + 1, expect);
      NBG_HIP(hipGetLastError());
    }
    NBG_HIP(hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    if (int64_t(std::max(h[0], h[1])) <= expect) break;
    expect = int64_t(std::max(h[0], h[1]));  // skewed ownership: regenerate with the exact size
  }
  so.n = int64_t(h[0]);
  si.n = int64_t(h[1]);
  c.build_seconds += now_s() - t0;
}

// ------------------------------------------------------------------------------------------
// Stage 2: finalize
// ------------------------------------------------------------------------------------------
// key transform for signed int64 sort order: flip the sign bit
__global__ void k_flip_copy(const int64_t* in, uint64_t* out, int64_t n, int world, int parts, int rank,
                            int filter_owner) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int64_t v = in[i];
    out[i] = uint64_t(v) ^ (1ull << 63);
  }
}
__global__ void k_unflip(const uint64_t* in, int64_t* out, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = int64_t(in[i] ^ (1ull << 63));
}

__global__ void k_ht_insert(int64_t* keys, int32_t* vals, uint64_t mask, const int64_t* vids, int64_t n,
                            int64_t gbase, int32_t* min_gidx) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int64_t v = vids[i];
    if (v == INT64_MIN) {
      *min_gidx = int32_t(gbase + i);
      continue;
    }
    uint64_t h = ht_hash(v) & mask;
    while (true) {
      unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(keys + h),
                                          (unsigned long long)INT64_MIN, (unsigned long long)v);
      if (prev == (unsigned long long)INT64_MIN || int64_t(prev) == v) {
        vals[h] = int32_t(gbase + i);
        break;
      }
      h = (h + 1) & mask;
    }
  }
}
__global__ void k_ht_lookup(const int64_t* keys, const int32_t* vals, uint64_t mask, bool has_min,
                            int32_t min_gidx, const int64_t* vids, int32_t* out, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = ht_lookup(keys, vals, mask, vids[i], has_min, min_gidx);
}

void lookup_gidx(Ctx& c, const int64_t* d_vids, int32_t* d_gidx, int64_t n) {
  if (n <= 0) return;
  k_ht_lookup<<<grid_for(n), 256, 0, c.stream>>>(c.ht_keys.as<int64_t>(), c.ht_vals.as<int32_t>(),
                                                uint64_t(c.ht_cap - 1), c.ht_has_min, c.ht_min_gidx,
                                                d_vids, d_gidx, n);
  NBG_HIP(hipGetLastError());
}

// bytewise order rank of every vertex: position of gidx in the order of bswap(vid)
__global__ void k_bswap_keys(const int64_t* vid_of, uint64_t* keys, uint32_t* idx, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    keys[i] = bswap64(uint64_t(vid_of[i]));
    idx[i] = uint32_t(i);
  }
}
__global__ void k_scatter_rank(const uint32_t* sorted_idx, uint32_t* byterank, int64_t n) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    byterank[sorted_idx[i]] = uint32_t(i);
}

// an emptied open-addressing table that n_slots_for entries fill at most half; returns its capacity
static int64_t ht_reset(Ctx& c, DevBuf& keys, DevBuf& vals, int64_t n_slots_for) {
  const int64_t cap = pow2_at_least(2 * n_slots_for, 1024);
  keys.alloc(size_t(cap) * 8);
  vals.alloc(size_t(cap) * 4);
  fill<int64_t>(c, keys.as<int64_t>(), INT64_MIN, cap);
  return cap;
}
static void ht_insert(Ctx& c, DevBuf& keys, DevBuf& vals, int64_t cap, const int64_t* vids, int64_t n, int64_t base,
                      DevWords<int32_t, 1>& dmin) {
  if (n <= 0) return;
  k_ht_insert<<<grid_for(n), 256, 0, c.stream>>>(keys.as<int64_t>(), vals.as<int32_t>(), uint64_t(cap - 1), vids, n, base,
                                                 dmin.dev());
}
void vid_hash_reset(Ctx& c, int64_t n_slots_for) {
  c.ht_cap = ht_reset(c, c.ht_keys, c.ht_vals, n_slots_for);
  c.ht_has_min = false;
  c.ht_min_gidx = -1;
}
void vid_hash_insert(Ctx& c, const int64_t* vids, int64_t n, int64_t base, DevWords<int32_t, 1>& dmin) {
  ht_insert(c, c.ht_keys, c.ht_vals, c.ht_cap, vids, n, base, dmin);
}
void vid_hash_publish_min(Ctx& c, const DevWords<int32_t, 1>& dmin) {
  const int32_t mg = dmin.read(c)[0];
  if (mg >= 0) {
    c.ht_has_min = true;
    c.ht_min_gidx = mg;
  }
}

__global__ void k_owned_only(const uint64_t* in, int64_t n, int parts, int world, int rank, uint8_t* flag) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int64_t v = int64_t(in[i] ^ (1ull << 63));
    flag[i] = dev_owner(v, parts, world) == rank;
  }
}

// out-degree (pre-collapse multiplicity is fine: it only orders vertices) via a provisional table
__global__ void k_count_deg(const int64_t* src, int64_t n, const int64_t* keys, const int32_t* vals, uint64_t mask,
                            bool has_min, int32_t min_idx, unsigned int* deg) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t g = ht_lookup(keys, vals, mask, src[i], has_min, min_idx);
    if (g >= 0) atomicAdd(deg + g, 1u);
  }
}
// Vertex numbering key (sorted ascending, stable over vids ascending): the degree class above
// the complemented out-degree.  Classes: 0 both in- and out-edges, 1 in-edges only, 2 out-edges
// only, 3 none (ideg null: every vertex class 0, plain descending out-degree); below the
// out-degree, two bits of descending min(in-degree, 3), so the rows with at most two in-edges
// -- nearly all of them in the long equal-out-degree runs, class 1 whole among them -- gather
// at the end of their run and fill whole tiles whose slots 2-3 are pad (tile_wide clear; the
// hubs, of distinct out-degrees, keep their places).  A bottom-up hop
// then works on a prefix of the rows: a non-final hop on class 0 (a row needs an in-edge to be
// found and an out-edge to matter), the final hop on classes 0-1 (snapshot: bu_both_tiles,
// bu_in_tiles, exact bounds whatever the order).  idx (streamed RMAT build): counts are indexed
// through it.
__global__ void k_class_key(const unsigned int* odeg, const unsigned int* ideg, const uint32_t* idx, int64_t n,
                            uint64_t* key) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t u = idx ? int64_t(idx[i]) : i;
    const uint32_t od = odeg[u];
    if (ideg) {
      const uint32_t id = ideg[u];
      const uint64_t cls = id ? (od ? 0 : 1) : (od ? 2 : 3);
      key[i] = (cls << 34) | (uint64_t(~od) << 2) | uint64_t(3u - min(id, 3u));
    } else {
      key[i] = uint64_t(~od);
    }
  }
}

void class_keys(Ctx& c, const uint32_t* odeg, const uint32_t* ideg, const uint32_t* idx, int64_t n, uint64_t* key) {
  k_class_key<<<grid_for(n), 256, 0, c.stream>>>(odeg, ideg, idx, n, key);
}

// Degree-ordered vertex numbering: a rank's owned gidx range lists its vertices by descending
// out-degree (ties by vid), one rank: within the degree classes of k_class_key.  The hubs -- the sources a bottom-up hop finds first (hub-first
// transposed rows) -- then share a few cache lines of every frontier bitmap instead of being
// scattered over all of it.  `owned` holds sign-flipped vids, sorted ascending on entry.
static void order_by_degree(Ctx& c, DevBuf& owned, int64_t n_owned) {
  if (n_owned <= 1) return;
  // a provisional table vid -> position in `owned`
  DevBuf keys, vals, vids, deg;
  const int64_t cap = ht_reset(c, keys, vals, n_owned);
  vids.alloc(size_t(n_owned) * 8);
  deg.alloc(size_t(n_owned) * 4);
  DevWords<int32_t, 1> dmin;
  dmin.set(c, {-1});
  NBG_HIP(hipMemsetAsync(deg.p, 0, size_t(n_owned) * 4, c.stream));
  k_unflip<<<grid_for(n_owned), 256, 0, c.stream>>>(owned.as<uint64_t>(), vids.as<int64_t>(), n_owned);
  ht_insert(c, keys, vals, cap, vids.as<int64_t>(), n_owned, 0, dmin);
  const int32_t min_idx = dmin.read(c)[0];
  // in-degrees too, for the degree classes of class_key: one rank counts the dsts of its out-edge
  // stage (every in-edge of an owned vertex is there); several ranks count the in-edge keys
  // (dst, -type, rank, src) their parts hold -- the dst owner's, P5 -- so each rank's range is
  // class-ordered too and its bottom-up hops stop at its own bu_both_tiles / bu_in_tiles
  DevBuf ideg;
  ideg.alloc(size_t(n_owned) * 4);
  NBG_HIP(hipMemsetAsync(ideg.p, 0, size_t(n_owned) * 4, c.stream));
  auto count = [&](const DevBuf& col, int64_t n, DevBuf& into) {
    k_count_deg<<<grid_for(n), 256, 0, c.stream>>>(col.as<int64_t>(), n, keys.as<int64_t>(), vals.as<int32_t>(),
                                                   uint64_t(cap - 1), min_idx >= 0, min_idx, into.as<unsigned int>());
  };
  for (auto& kv : c.edges) {
    const Staging& st = kv.second.out_stage;
    if (!st.n) continue;
    count(st.src, st.n, deg);
    if (!c.sharded) count(st.dst, st.n, ideg);
    const Staging& si = kv.second.in_stage;
    if (c.sharded && si.n) count(si.src, si.n, ideg);
  }
  keys.release();
  vals.release();
  DevBuf key, keyS, sorted;
  key.alloc(size_t(n_owned) * 8);
  keyS.alloc(size_t(n_owned) * 8);
  sorted.alloc(size_t(n_owned) * 8);
  class_keys(c, deg.as<uint32_t>(), ideg.as<uint32_t>(), nullptr, n_owned, key.as<uint64_t>());
  radix_pairs<uint64_t, uint64_t>(c, key.as<uint64_t>(), keyS.as<uint64_t>(), owned.as<uint64_t>(),
                                 sorted.as<uint64_t>(), n_owned, kClassKeyBits);
  NBG_HIP(hipMemcpyAsync(owned.p, sorted.p, size_t(n_owned) * 8, hipMemcpyDeviceToDevice, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  NBG_HIP(hipGetLastError());
}

// Tag columns over the gidx space.  Winner per vertex = the first key of the prefix
// (part, vid, tag) in RocksDB bytewise order: smallest LE version bytes, and among identical keys
// the last write (WriteBatch last-write-wins, RocksEngine.cpp:216-230).  Rows stored in a part
// other than the vid's own are never reached by the prefix scan (the request part is
// hash(vid), StorageClient.cpp:238-243), and vids outside every edge have no gidx: both dropped.
__global__ void k_tag_gather(const int32_t* win, const uint8_t* state, int64_t ng, const int64_t* props,
                             const uint8_t* present, int64_t* data, uint8_t* pres_out) {
  for (int64_t g = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; g < ng; g += int64_t(gridDim.x) * blockDim.x) {
    int32_t w = win[g];
    bool ok = w >= 0 && present[w] != 0;
    data[g] = ok ? props[w] : 0;
    pres_out[g] = ok ? state[g] : 0;
  }
}
__global__ void k_tag_str_len(const int32_t* win, int64_t ng, const uint8_t* present, const int64_t* lens,
                              int64_t* out) {
  for (int64_t g = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; g <= ng; g += int64_t(gridDim.x) * blockDim.x) {
    int32_t w = g < ng ? win[g] : -1;
    out[g] = (w >= 0 && present[w]) ? lens[w] : 0;
  }
}
__global__ void k_tag_str_copy(const int32_t* win, int64_t ng, const uint8_t* heap, const int64_t* heap_off,
                               const int64_t* off, uint8_t* out) {
  for (int64_t g = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; g < ng; g += int64_t(gridDim.x) * blockDim.x) {
    int64_t len = off[g + 1] - off[g];
    if (len <= 0) continue;
    const uint8_t* s = heap + heap_off[win[g]];
    for (int64_t j = 0; j < len; j++) out[off[g] + j] = s[j];
  }
}

// world > 1: every rank fills its owned gidx slice [base[r], base[r+1]); allgather the slices
// so each rank holds the whole column ($$ props of dsts owned elsewhere)
static void replicate_owned(Ctx& c, DevBuf& col, size_t w) {
  std::vector<size_t> rb(size_t(c.world)), ro(size_t(c.world));
  for (int r = 0; r < c.world; r++) {
    ro[size_t(r)] = size_t(c.base[size_t(r)]) * w;
    rb[size_t(r)] = size_t(c.base[size_t(r) + 1] - c.base[size_t(r)]) * w;
  }
  DevBuf send;
  send.alloc(std::max<size_t>(rb[size_t(c.rank)], 8));
  if (rb[size_t(c.rank)])
    NBG_HIP(hipMemcpyAsync(send.p, col.as<uint8_t>() + ro[size_t(c.rank)], rb[size_t(c.rank)], hipMemcpyDeviceToDevice,
                           c.stream));
  comm_allgatherv_bytes(c, send.p, rb[size_t(c.rank)], col.p, rb.data(), ro.data());
}

static void build_tag_columns(Ctx& c) {
  c.tag_refs.clear();
  const int64_t ng = c.n_global;
  for (auto& kvp : c.tags) {
    TagSpace& ts = kvp.second;
    const int64_t n = ts.stage.n;
    std::vector<int32_t> win(size_t(std::max<int64_t>(ng, 1)), -1);
    std::vector<uint8_t> wstate(size_t(std::max<int64_t>(ng, 1)), 0);  // 1 own part, 2 foreign part
    std::vector<int32_t> tpart(size_t(std::max<int64_t>(ng, 1)), 0);
    std::vector<int64_t> tail_vids;
    if (n > 0) {
      DevBuf dg;
      dg.alloc(size_t(n) * 4);
      const size_t nn = static_cast<size_t>(n);
      std::vector<int32_t> g(nn, -1), part(nn);
      std::vector<int64_t> vid(nn), ver(nn), seq(nn);
      if (ng > 0) {  // (no edge at all: no vertex map, every row is a tail row)
        lookup_gidx(c, ts.stage.src.as<int64_t>(), dg.as<int32_t>(), n);
        NBG_HIP(hipMemcpyAsync(g.data(), dg.p, size_t(n) * 4, hipMemcpyDeviceToHost, c.stream));
      }
      NBG_HIP(hipMemcpyAsync(part.data(), ts.stage.part.p, size_t(n) * 4, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipMemcpyAsync(vid.data(), ts.stage.src.p, size_t(n) * 8, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipMemcpyAsync(ver.data(), ts.stage.ver.p, size_t(n) * 8, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipMemcpyAsync(seq.data(), ts.stage.seq.p, size_t(n) * 8, hipMemcpyDeviceToHost, c.stream));
      NBG_HIP(hipStreamSynchronize(c.stream));
      // candidate order: rows of the vid's own part first (GO reads those), else the smallest
      // foreign part (a getBound request naming that part reads it); then the prefix scan's
      // first key (smallest LE version bytes), identical keys by last write
      auto foreign = [&](int64_t i) { return part[size_t(i)] != part_of_vid(vid[size_t(i)], c.num_parts); };
      // world > 1: a rank keeps only its owned slice (replicate_owned gathers slices); a row in a
      // foreign part held by another rank is not visible there (getBound on that part only)
      const int64_t olo = c.owned_lo(), ohi = c.owned_hi();
      // vids outside every edge have no gidx: their own-part rows (on the rank owning that part)
      // go to the tag's tail under the same winner rule (FETCH PROP ON reads them)
      std::map<int64_t, int32_t> orphan;
      for (int64_t i = 0; i < n; i++) {
        int32_t gi = g[size_t(i)];
        if (gi < 0) {
          if (foreign(i) || (c.sharded && owner_of_part(part[size_t(i)], c.world) != c.rank)) continue;
          auto ins = orphan.emplace(vid[size_t(i)], int32_t(i));
          if (ins.second) continue;
          int32_t& w = ins.first->second;
          uint64_t a = __builtin_bswap64(uint64_t(ver[size_t(i)])), b = __builtin_bswap64(uint64_t(ver[size_t(w)]));
          if (a < b || (a == b && seq[size_t(i)] > seq[size_t(w)])) w = int32_t(i);
          continue;
        }
        if (c.sharded && (gi < olo || gi >= ohi)) continue;
        int32_t& w = win[size_t(gi)];
        if (w < 0) {
          w = int32_t(i);
          continue;
        }
        const bool fi = foreign(i), fw = foreign(w);
        if (fi != fw) {
          if (!fi) w = int32_t(i);
          continue;
        }
        if (fi && part[size_t(i)] != part[size_t(w)]) {
          if (part[size_t(i)] < part[size_t(w)]) w = int32_t(i);
          continue;
        }
        uint64_t a = __builtin_bswap64(uint64_t(ver[size_t(i)])), b = __builtin_bswap64(uint64_t(ver[size_t(w)]));
        if (a < b || (a == b && seq[size_t(i)] > seq[size_t(w)])) w = int32_t(i);
      }
      for (int64_t gi = 0; gi < ng; gi++) {
        const int32_t w = win[size_t(gi)];
        if (w < 0) continue;
        wstate[size_t(gi)] = foreign(w) ? 2 : 1;
        tpart[size_t(gi)] = part[size_t(w)];
      }
      // the tail: entry ng + k = the k-th orphan vid in ascending order
      win.resize(size_t(ng));
      wstate.resize(size_t(ng));
      tpart.resize(size_t(ng));
      for (const auto& o : orphan) {
        tail_vids.push_back(o.first);
        win.push_back(o.second);
        wstate.push_back(1);
        tpart.push_back(part[size_t(o.second)]);
      }
      if (win.empty()) {
        win.push_back(-1);
        wstate.push_back(0);
        tpart.push_back(0);
      }
    }
    const int64_t nt = int64_t(tail_vids.size());
    const int64_t nx = ng + nt;  // the columns' entries: the gidx space, then the tail
    const size_t nx1 = size_t(std::max<int64_t>(nx, 1));
    ts.n_tail = nt;
    ts.tail_vids.alloc(size_t(std::max<int64_t>(nt, 1)) * 8);
    if (nt) NBG_HIP(hipMemcpyAsync(ts.tail_vids.p, tail_vids.data(), size_t(nt) * 8, hipMemcpyHostToDevice, c.stream));
    DevBuf dwin;
    dwin.alloc(nx1 * 4);
    ts.state.alloc(nx1);
    ts.part.alloc(nx1 * 4);
    NBG_HIP(hipMemcpyAsync(dwin.p, win.data(), nx1 * 4, hipMemcpyHostToDevice, c.stream));
    NBG_HIP(hipMemcpyAsync(ts.state.p, wstate.data(), nx1, hipMemcpyHostToDevice, c.stream));
    NBG_HIP(hipMemcpyAsync(ts.part.p, tpart.data(), nx1 * 4, hipMemcpyHostToDevice, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));  // host vectors are pageable
    ts.cols.clear();
    for (size_t f = 0; f < ts.fields.size(); f++) {
      PropCol pc;
      pc.name = ts.fields[f].name;
      pc.type = ts.fields[f].type;
      pc.width = 8;
      pc.data.alloc(nx1 * 8);
      pc.present.alloc(nx1);
      if (n == 0 || nx == 0) {
        NBG_HIP(hipMemsetAsync(pc.data.p, 0, pc.data.bytes, c.stream));
        NBG_HIP(hipMemsetAsync(pc.present.p, 0, pc.present.bytes, c.stream));
      } else {
        k_tag_gather<<<grid_for(nx), 256, 0, c.stream>>>(dwin.as<int32_t>(), ts.state.as<uint8_t>(), nx,
                                                          ts.stage.props[f].as<int64_t>(),
                                                          ts.stage.present[f].as<uint8_t>(), pc.data.as<int64_t>(),
                                                          pc.present.as<uint8_t>());
      }
      if (pc.type == NBG_T_STRING) {
        DevBuf lens;
        lens.alloc(size_t(nx + 1) * 8);
        pc.str_off.alloc(size_t(nx + 1) * 8);
        if (n == 0 || nx == 0) {
          NBG_HIP(hipMemsetAsync(lens.p, 0, lens.bytes, c.stream));
        } else {
          k_tag_str_len<<<grid_for(nx + 1), 256, 0, c.stream>>>(dwin.as<int32_t>(), nx, ts.stage.present[f].as<uint8_t>(),
                                                                 ts.stage.str_len[f].as<int64_t>(), lens.as<int64_t>());
        }
        exclusive_scan_dev<int64_t>(c, lens.as<int64_t>(), pc.str_off.as<int64_t>(), nx + 1);
        int64_t total = 0;
        NBG_HIP(hipMemcpyAsync(&total, pc.str_off.as<int64_t>() + nx, 8, hipMemcpyDeviceToHost, c.stream));
        NBG_HIP(hipStreamSynchronize(c.stream));
        pc.str_bytes.alloc(size_t(total) + 8);
        if (total > 0)
          k_tag_str_copy<<<grid_for(nx), 256, 0, c.stream>>>(dwin.as<int32_t>(), nx, c.heap.as<uint8_t>(),
                                                              ts.stage.props[f].as<int64_t>(), pc.str_off.as<int64_t>(),
                                                              pc.str_bytes.as<uint8_t>());
        if (c.sharded) {
          // lengths of every rank's owned slice -> global offsets; bytes by owner block
          // (the tail is rank-local: its lengths stay behind the gathered slices, and its bytes,
          // which sit behind this rank's owned slice here, move behind every rank's)
          replicate_owned(c, lens, 8);
          exclusive_scan_dev<int64_t>(c, lens.as<int64_t>(), pc.str_off.as<int64_t>(), nx + 1);
          std::vector<int64_t> goff(size_t(nx) + 1);
          NBG_HIP(hipMemcpyAsync(goff.data(), pc.str_off.p, size_t(nx + 1) * 8, hipMemcpyDeviceToHost, c.stream));
          NBG_HIP(hipStreamSynchronize(c.stream));
          std::vector<size_t> rb(size_t(c.world)), ro(size_t(c.world));
          for (int r = 0; r < c.world; r++) {
            ro[size_t(r)] = size_t(goff[size_t(c.base[size_t(r)])]);
            rb[size_t(r)] = size_t(goff[size_t(c.base[size_t(r) + 1])]) - ro[size_t(r)];
          }
          DevBuf all;
          all.alloc(size_t(goff[size_t(nx)]) + 8);
          const size_t own_bytes = rb[size_t(c.rank)];
          comm_allgatherv_bytes(c, pc.str_bytes.p, own_bytes, all.p, rb.data(), ro.data());
          if (size_t(total) > own_bytes)
            NBG_HIP(hipMemcpyAsync(all.as<uint8_t>() + goff[size_t(ng)], pc.str_bytes.as<uint8_t>() + own_bytes,
                                   size_t(total) - own_bytes, hipMemcpyDeviceToDevice, c.stream));
          pc.str_bytes = std::move(all);
        }
      }
      if (c.sharded) {
        replicate_owned(c, pc.data, 8);
        replicate_owned(c, pc.present, 1);
      }
      NBG_HIP(hipGetLastError());
      c.tag_refs.push_back(TagFieldRef{ts.name, pc.name, pc.type});
      ts.cols.push_back(std::move(pc));
    }
    if (c.sharded) {
      replicate_owned(c, ts.part, 4);
      replicate_owned(c, ts.state, 1);
    }
    NBG_HIP(hipStreamSynchronize(c.stream));
    if (!c.opt("writable", 0)) ts.stage = Staging{};
  }
}

__global__ void k_count_unknown(const int64_t* src, const int64_t* dst, int64_t n, const int64_t* keys_ht,
                                const int32_t* vals_ht, uint64_t mask, bool has_min, int32_t min_gidx,
                                unsigned long long* cnt) {
  unsigned long long u = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    u += (ht_lookup(keys_ht, vals_ht, mask, src[i], has_min, min_gidx) < 0) +
         (ht_lookup(keys_ht, vals_ht, mask, dst[i], has_min, min_gidx) < 0);
  for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o);
  if ((threadIdx.x & 63) == 0 && u) atomicAdd(cnt, u);
}

// vids of a batch's endpoints that are not in the vertex map (sign-flipped for an unsigned sort)
__global__ void k_collect_unknown(const int64_t* src, const int64_t* dst, int64_t n, const int64_t* keys_ht,
                                  const int32_t* vals_ht, uint64_t mask, bool has_min, int32_t min_gidx,
                                  uint64_t* out, unsigned long long* cnt) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  const int64_t rounds = (n + stride - 1) / stride;
  for (int64_t r = 0; r < rounds; r++) {
    const int64_t i = r * stride + blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    int64_t a = 0, b = 0;
    bool ua = false, ub = false;
    if (i < n) {
      a = src[i];
      b = dst[i];
      ua = ht_lookup(keys_ht, vals_ht, mask, a, has_min, min_gidx) < 0;
      ub = ht_lookup(keys_ht, vals_ht, mask, b, has_min, min_gidx) < 0;
    }
    const int64_t sa = wave_append(cnt, ua);
    if (ua) out[sa] = uint64_t(a) ^ (1ull << 63);
    const int64_t sb = wave_append(cnt, ub);
    if (ub) out[sb] = uint64_t(b) ^ (1ull << 63);
  }
}
// committed sort keys under new bytewise ranks: the src half stays, the dst rank is re-read
__global__ void k_rekey(uint64_t* skey, const int32_t* dstg, int64_t n, const uint32_t* brank) {
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    skey[i] = (skey[i] & 0xffffffff00000000ull) | uint64_t(brank[dstg[i]]);
}

DevBuf bytewise_ranks(Ctx& c) {
  DevBuf brank;
  const int64_t ng = std::max<int64_t>(c.n_global, 1);
  DevBuf k1, k2, i1, i2;
  k1.alloc(size_t(ng) * 8);
  k2.alloc(size_t(ng) * 8);
  i1.alloc(size_t(ng) * 4);
  i2.alloc(size_t(ng) * 4);
  brank.alloc(size_t(ng) * 4);
  if (c.n_global) {
    k_bswap_keys<<<grid_for(c.n_global), 256, 0, c.stream>>>(c.vid_of.as<int64_t>(), k1.as<uint64_t>(), i1.as<uint32_t>(),
                                                             c.n_global);
    radix_pairs<uint64_t, uint32_t>(c, k1.as<uint64_t>(), k2.as<uint64_t>(), i1.as<uint32_t>(), i2.as<uint32_t>(),
                                    c.n_global, 64);
    k_scatter_rank<<<grid_for(c.n_global), 256, 0, c.stream>>>(i2.as<uint32_t>(), brank.as<uint32_t>(), c.n_global);
  }
  return brank;
}

// the endpoint vids of every pending batch that are not in the vertex map, sign-flipped, sorted
// and unique in uniq; returns their count (unknown_bound: k_count_unknown's count of them)
static int64_t collect_unknown_vids(Ctx& c, int64_t unknown_bound, DevBuf& uniq) {
  DevBuf raw;
  raw.alloc(size_t(std::max<int64_t>(unknown_bound, 1)) * 8);
  DevWords<unsigned long long, 1> cnt;
  cnt.zero(c);
  for (auto& kv : c.edges) {
    EdgeSpace& es = kv.second;
    for (int d = 0; d < 2; d++) {
      const Staging& st = d ? es.in_stage : es.out_stage;
      const int64_t n0 = es.ord[d].n;
      if (st.n > n0)
        k_collect_unknown<<<grid_for(st.n - n0), 256, 0, c.stream>>>(
            st.src.as<int64_t>() + n0, st.dst.as<int64_t>() + n0, st.n - n0, c.ht_keys.as<int64_t>(),
            c.ht_vals.as<int32_t>(), uint64_t(c.ht_cap - 1), c.ht_has_min, c.ht_min_gidx, raw.as<uint64_t>(), cnt.dev());
    }
  }
  const unsigned long long nraw = cnt.read(c)[0];
  if (int64_t(nraw) > unknown_bound) throw Error(NBG_E_UNKNOWN, "merge commit: unknown-vertex count changed");
  DevBuf sorted;
  sorted.alloc(size_t(std::max<uint64_t>(nraw, 1)) * 8);
  uniq.alloc(size_t(std::max<uint64_t>(nraw, 1)) * 8);
  if (!nraw) return 0;
  radix_keys<uint64_t>(c, raw.as<uint64_t>(), sorted.as<uint64_t>(), int64_t(nraw), 64);
  return unique_sorted<uint64_t>(c, sorted.as<uint64_t>(), uniq.as<uint64_t>(), int64_t(nraw));
}

// after new vertices: the bytewise ranks recomputed, and the committed sort keys re-read their
// dst rank
static void rerank_committed_orders(Ctx& c) {
  c.brank = bytewise_ranks(c);
  for (auto& kv : c.edges)
    for (auto& o : kv.second.ord)
      if (o.n > 0 && o.skey.p)
        k_rekey<<<grid_for(o.n), 256, 0, c.stream>>>(o.skey.as<uint64_t>(), o.dstg.as<int32_t>(), o.n,
                                                    c.brank.as<uint32_t>());
  NBG_HIP(hipGetLastError());
}

// Merge commit with new vertices (one rank): the batch's unknown endpoint vids, sorted, take
// the gidx after the committed ones (the padding first, then a grown range), the vertex map and
// hash table grow in place (the table is rebuilt when it would pass half full), the bytewise
// ranks are recomputed and the committed sort keys re-read their dst rank -- the committed
// order itself stays sorted, since inserting vids into the bytewise order moves no committed
// vid past another.  Existing gidx never change, so every committed tuple keeps its place.
static void extend_vertex_map(Ctx& c, int64_t unknown_bound) {
  DevBuf uniq;
  const int64_t k = collect_unknown_vids(c, unknown_bound, uniq);
  const int64_t n0 = c.n_vertices, n1 = n0 + k;
  const int64_t ng1 = (n1 + 63) / 64 * 64;
  if (ng1 >= (int64_t(1) << 31)) throw Error(NBG_E_UNSUPPORTED, "more than 2^31 vertices");
  if (ng1 > c.n_global) {
    DevBuf nv;
    nv.alloc(size_t(ng1) * 8);
    fill<int64_t>(c, nv.as<int64_t>(), INT64_MIN, ng1);
    NBG_HIP(hipMemcpyAsync(nv.p, c.vid_of.p, size_t(c.n_global) * 8, hipMemcpyDeviceToDevice, c.stream));
    c.vid_of = std::move(nv);
  }
  if (k) k_unflip<<<grid_for(k), 256, 0, c.stream>>>(uniq.as<uint64_t>(), c.vid_of.as<int64_t>() + n0, k);
  DevWords<int32_t, 1> dmin;
  dmin.set(c, {-1});
  if (2 * ng1 > c.ht_cap) {  // past half full: a table of the grown size, every vertex inserted
    vid_hash_reset(c, ng1);
    vid_hash_insert(c, c.vid_of.as<int64_t>(), n1, 0, dmin);
  } else {
    vid_hash_insert(c, c.vid_of.as<int64_t>() + n0, k, n0, dmin);
  }
  vid_hash_publish_min(c, dmin);
  c.n_vertices = n1;
  c.counts.assign(1, n1);
  c.base.assign(2, 0);
  c.base[1] = ng1;
  c.n_global = ng1;
  rerank_committed_orders(c);
}

// Merge commit with new vertices on several ranks.  Every rank sends the unknown endpoint vids
// of its batch (sorted, unique) to all; the union, sorted, is the same on every rank, and each
// owner's new vertices (vid % parts + 1 on rank part % world, pickHosts) take the next gidx of
// its growth room in vid order -- every rank computes every assignment itself, so the
// replicated vertex map and hash table stay identical without a second exchange.  Returns false
// (on every rank alike) when some owner's room is too small: the caller then rebuilds fully.
struct NewVertexPlan {
  std::vector<int64_t> vids;  // the union, sorted
  std::vector<std::vector<int64_t>> per_owner;
};
static bool plan_new_vertices_ranks(Ctx& c, int64_t unknown_bound, NewVertexPlan& plan) {
  DevBuf uniq;
  const int64_t k = collect_unknown_vids(c, unknown_bound, uniq);
  // every rank's list to every rank
  const size_t G = size_t(c.world);
  const std::vector<int64_t> ks = allgather_i64(c, k);
  std::vector<size_t> rb(G), ro(G);
  size_t tot = 0;
  for (size_t r = 0; r < G; r++) {
    rb[r] = size_t(ks[r]) * 8;
    ro[r] = tot;
    tot += rb[r];
  }
  DevBuf recv;
  recv.alloc(std::max<size_t>(tot, 8));
  comm_allgatherv_bytes(c, uniq.p, size_t(k) * 8, recv.p, rb.data(), ro.data());
  std::vector<uint64_t> flipped(tot / 8);
  if (tot) NBG_HIP(hipMemcpyAsync(flipped.data(), recv.p, tot, hipMemcpyDeviceToHost, c.stream));
  NBG_HIP(hipStreamSynchronize(c.stream));
  std::sort(flipped.begin(), flipped.end());
  flipped.erase(std::unique(flipped.begin(), flipped.end()), flipped.end());
  plan.vids.resize(flipped.size());
  plan.per_owner.assign(G, {});
  for (size_t i = 0; i < flipped.size(); i++) {  // sign-flipped order = signed vid order
    const int64_t v = int64_t(flipped[i] ^ (1ull << 63));
    plan.vids[i] = v;
    plan.per_owner[size_t(dev_owner(v, c.num_parts, c.world))].push_back(v);
  }
  for (size_t q = 0; q < G; q++)
    if (c.counts[q] + int64_t(plan.per_owner[q].size()) > c.base[q + 1] - c.base[q]) return false;
  return true;
}

// applies a plan: each owner's new vertices at base + counts onward, in the replicated vertex map
// and hash table; bytewise ranks recomputed and the committed sort keys re-read their dst rank
static void extend_vertex_map_ranks(Ctx& c, const NewVertexPlan& plan) {
  DevWords<int32_t, 1> dmin;
  dmin.set(c, {-1});
  DevBuf dv;
  dv.alloc(std::max<size_t>(plan.vids.size(), 1) * 8);
  size_t off = 0;
  for (size_t q = 0; q < plan.per_owner.size(); q++) {
    const auto& l = plan.per_owner[q];
    if (l.empty()) continue;
    const int64_t g0 = c.base[q] + c.counts[q];
    NBG_HIP(hipMemcpyAsync(dv.as<int64_t>() + off, l.data(), l.size() * 8, hipMemcpyHostToDevice, c.stream));
    NBG_HIP(hipMemcpyAsync(c.vid_of.as<int64_t>() + g0, dv.as<int64_t>() + off, l.size() * 8, hipMemcpyDeviceToDevice,
                           c.stream));
    vid_hash_insert(c, dv.as<int64_t>() + off, int64_t(l.size()), g0, dmin);
    off += l.size();
  }
  vid_hash_publish_min(c, dmin);  // (its stream wait also covers the pageable host lists)
  for (size_t q = 0; q < plan.per_owner.size(); q++) c.counts[q] += int64_t(plan.per_owner[q].size());
  c.n_vertices += int64_t(plan.vids.size());
  rerank_committed_orders(c);
}

// option build_trace: per-phase wall time and hipMalloc count on stderr (the stream drained at
// each mark)
struct BuildTrace {
  Ctx& c;
  const char* tag;  // "build" or "merge"
  const bool on;
  double tmark;
  BuildTrace(Ctx& ctx, const char* t, double t0) : c(ctx), tag(t), on(ctx.opt("build_trace", 0) != 0), tmark(t0) {}
  void operator()(const char* name) {
    if (!on) return;
    NBG_HIP(hipStreamSynchronize(c.stream));
    const double t = now_s();
    const int64_t an = g_alloc_clock.alloc_ns.exchange(0), fn = g_alloc_clock.free_ns.exchange(0);
    const int64_t na = g_alloc_clock.allocs.exchange(0);
    fprintf(stderr, "[nbg %s] %-22s %8.3f s  (hipMalloc %lld x %.3f s, hipFree %.3f s)\n", tag, name, t - tmark,
            (long long)na, an * 1e-9, fn * 1e-9);
    tmark = t;
  }
};

// The merge commit in steps.  flags: what the ranks agree on by one sum -- [0] some rank must
// rebuild, [1] endpoints not in the vertex map, [2] tag writes, then per edge space whether the
// out / in stage grew (a rank without writes of its own still rebuilds its transposed rows when
// another rank's out-edges changed).
struct MergeCommit {
  Ctx& c;
  unsigned long long unknown = 0;  // this rank's count
  std::vector<int64_t> flags;
  NewVertexPlan plan;
  explicit MergeCommit(Ctx& ctx) : c(ctx), flags(3 + 2 * ctx.edges.size(), 0) {}

  // can every changed stage merge (a committed order to merge into, load sequences), and how many
  // batch endpoints are new vertices
  void local_checks() {
    bool tag_writes = false;
    for (auto& kv : c.tags) tag_writes |= kv.second.stage.n != kv.second.committed_n;
    bool refuse = false;
    DevWords<unsigned long long, 1> cnt;
    cnt.zero(c);
    for (auto& kv : c.edges) {
      EdgeSpace& es = kv.second;
      if (es.rmat_stream) refuse = true;
      for (int d = 0; d < 2 && !refuse; d++) {
        const Staging& st = d ? es.in_stage : es.out_stage;
        const int64_t n0 = es.ord[d].n;
        if (st.n == n0) continue;
        if (n0 <= 0 || !es.ord[d].perm.p || st.n < n0 || st.seq.bytes < size_t(st.n) * 8) {
          refuse = true;
          break;
        }
        k_count_unknown<<<grid_for(st.n - n0), 256, 0, c.stream>>>(
            st.src.as<int64_t>() + n0, st.dst.as<int64_t>() + n0, st.n - n0, c.ht_keys.as<int64_t>(),
            c.ht_vals.as<int32_t>(), uint64_t(c.ht_cap - 1), c.ht_has_min, c.ht_min_gidx, cnt.dev());
      }
    }
    unknown = cnt.read(c)[0];
    if (!refuse && unknown) {
      // new vertices extend the numbering (extend_vertex_map); every CSR direction then needs
      // rows for them, which the merge builds only where the batch has tuples: other batches
      // (and the off switch) take the full rebuild
      // (several ranks: the new vertices land in rows every CSR already has, the growth room)
      for (auto& kv : c.edges)
        for (int d = 0; d < 2 && !c.sharded; d++)
          if ((d ? kv.second.in_stage.n : kv.second.out_stage.n) == kv.second.ord[d].n) refuse = true;
    }
    size_t i = 3;
    for (auto& kv : c.edges) {
      flags[i++] = kv.second.out_stage.n != kv.second.ord[0].n;
      flags[i++] = kv.second.in_stage.n != kv.second.ord[1].n;
    }
    flags[0] = refuse, flags[1] = int64_t(unknown), flags[2] = tag_writes;
  }
  // several ranks: the choice is collective (every rank merges or every rank rebuilds)
  void agree() {
    if (!c.sharded) return;
    DevBuf f;
    f.alloc(flags.size() * 8);
    NBG_HIP(hipMemcpyAsync(f.p, flags.data(), flags.size() * 8, hipMemcpyHostToDevice, c.stream));
    comm_allreduce_sum_i64(c, f.as<int64_t>(), flags.size());
    NBG_HIP(hipMemcpyAsync(flags.data(), f.p, flags.size() * 8, hipMemcpyDeviceToHost, c.stream));
    NBG_HIP(hipStreamSynchronize(c.stream));
    // new vertices: placed in the owners' growth rooms when they fit on every rank (collective:
    // the same union and decision everywhere), else the full rebuild
    if (!flags[0] && flags[1] > 0 && !plan_new_vertices_ranks(c, int64_t(unknown), plan)) flags[0] = 1;
  }
  bool can_merge() const { return !flags[0]; }

  void vertex_map(BuildTrace& phase) {
    const bool new_vertices = c.sharded ? !plan.vids.empty() : unknown > 0;
    if (new_vertices) {
      if (c.sharded) extend_vertex_map_ranks(c, plan);
      else extend_vertex_map(c, int64_t(unknown));
      phase("vertex map (new vertices)");
    }
    if (new_vertices || flags[2] > 0) {
      // tag columns span the gidx space and pick winners over every staged row: rebuilt (on every
      // rank when any has tag writes: the owned slices are allgathered)
      c.tag_table.release();
      for (auto& kv : c.tags) {
        kv.second.cols.clear();
        kv.second.part.release();
      }
      build_tag_columns(c);
      for (auto& kv : c.tags) kv.second.committed_n = kv.second.stage.n;
      phase("tag columns");
    }
  }
  // one edge space: the changed CSRs merged, the transpose rebuilt; out_any / in_any: on some rank
  void edge_space(EdgeSpace& es, bool out_any, bool in_any, BuildTrace& phase) {
    const bool out_changed = es.out_stage.n != es.ord[0].n, in_changed = es.in_stage.n != es.ord[1].n;
    if (out_changed) {
      Csr keep_in = std::move(es.in);  // an unchanged in CSR survives the reset
      reset_edge_derived(es);          // out CSR and everything derived from it (transpose, slabs)
      es.in = std::move(keep_in);
      build_csr(c, es.out_stage, es.fields, true, es.out, c.brank.as<uint32_t>(), false, &es.ord[0], true);
      phase("out CSR (merge)");
    } else if (out_any) {
      reset_transpose_derived(es);  // another rank's out-edges land in this rank's transposed rows
    }
    if (in_changed) build_csr(c, es.in_stage, es.fields, false, es.in, c.brank.as<uint32_t>(), false, &es.ord[1], true);
    phase("in CSR (merge)");
    if (out_any || in_any) {
      // replicated CSRs (FIND SHORTEST PATH on several ranks) are rebuilt on first use
      es.rep_out = Csr();
      es.rep_in = Csr();
      es.has_rep = es.has_rep_out = false;
      es.rep_odeg.release();
      es.rev = EdgeSpace::Rev();  // the type's keys changed on some rank: in-degrees and mirror state too
    }
    if (out_any && c.opt("bottom_up", 1)) build_transpose(c, es);  // collective on several ranks
    phase("transpose + slabs");
  }
};

static bool commit_merge(Ctx& c) {
  // (the option and c.brank (writable) agree on every rank)
  if (c.opt("merge_commit", 1) == 0 || !c.brank.p) return false;
  MergeCommit mc(c);
  mc.local_checks();
  mc.agree();
  if (!mc.can_merge()) return false;
  PoolScope build_scope(build_pool(c));
  c.finalized = false;  // a merge that throws leaves the next commit a full rebuild
  const double t0 = now_s();
  BuildTrace phase(c, "merge", t0);
  phase("checks");
  mc.vertex_map(phase);
  size_t fi = 3;
  for (auto& kv : c.edges) {
    mc.edge_space(kv.second, mc.flags[fi] > 0, mc.flags[fi + 1] > 0, phase);
    fi += 2;
  }
  c.ws_tmp.release();
  NBG_HIP(hipStreamSynchronize(c.stream));
  c.finalized = true;
  c.build_seconds += now_s() - t0;
  return true;
}

// The vertex set and numbering of a full build, step by step (snapshot_finalize calls them in
// order): the vids the staged tuples reference, the ones this rank owns (degree-ordered by
// order_by_degree in between), every rank's gidx range, the replicated vid_of and hash table.
struct VertexMapBuild {
  Ctx& c;
  const bool keep;  // writable snapshot
  DevBuf refs;      // sign-flipped vids, sorted unique
  int64_t nuniq = 0;
  DevBuf owned;     // the same of the vertices this rank owns
  int64_t n_owned = 0;
  std::vector<int64_t> counts;  // owned vertices of every rank

  // referenced vids (src/dst of every staged tuple), sign-flipped for an unsigned sort.  One
  // staged column at a time is sorted, deduplicated and merged into the running set, so the peak
  // is 16 B per tuple of the largest column (not 16 B per vid reference of the whole snapshot:
  // 69 GB for a writable RMAT-26, whose stages stay resident beside it)
  void referenced_vids() {
    for (auto& kv : c.edges) {
      for (Staging* s : {&kv.second.out_stage, &kv.second.in_stage}) {
        if (s->n == 0) continue;
        for (const DevBuf* colp : {&s->src, &s->dst}) {
          const int64_t n = s->n;
          DevBuf t1, t2;
          t1.alloc(size_t(n) * 8);
          t2.alloc(size_t(n) * 8);
          k_flip_copy<<<grid_for(n), 256, 0, c.stream>>>(colp->as<int64_t>(), t1.as<uint64_t>(), n, 0, 0, 0, 0);
          radix_keys<uint64_t>(c, t1.as<uint64_t>(), t2.as<uint64_t>(), n, 64);
          const int64_t m = unique_sorted<uint64_t>(c, t2.as<uint64_t>(), t1.as<uint64_t>(), n);
          t2.release();
          if (nuniq == 0) {
            refs = std::move(t1);
            nuniq = m;
            continue;
          }
          DevBuf cat, srt;
          cat.alloc(size_t(nuniq + m) * 8);
          srt.alloc(size_t(nuniq + m) * 8);
          NBG_HIP(hipMemcpyAsync(cat.p, refs.p, size_t(nuniq) * 8, hipMemcpyDeviceToDevice, c.stream));
          NBG_HIP(hipMemcpyAsync(cat.as<uint64_t>() + nuniq, t1.p, size_t(m) * 8, hipMemcpyDeviceToDevice, c.stream));
          t1.release();
          refs.release();
          radix_keys<uint64_t>(c, cat.as<uint64_t>(), srt.as<uint64_t>(), nuniq + m, 64);
          nuniq = unique_sorted<uint64_t>(c, srt.as<uint64_t>(), cat.as<uint64_t>(), nuniq + m);
          refs = std::move(cat);
        }
      }
    }
    if (!refs.p) refs.alloc(8);
  }
  // the referenced vids this rank owns
  void owned_vids() {
    n_owned = nuniq;
    if (!c.sharded) {
      owned = std::move(refs);
      return;
    }
    // every rank sends the vids it references to their owners; owners union.  (Simple form:
    // allgather the unique referenced sets, filter by owner; fine for build-time volumes.)
    const std::vector<int64_t> sizes = allgather_i64(c, nuniq);
    DevBuf all = allgather_padded(c, refs, nuniq, sizes, 8);
    int64_t tot = 0;
    for (auto s : sizes) tot += s;
    // keep owned, sort + unique
    DevBuf flag, sel;
    flag.alloc(size_t(std::max<int64_t>(tot, 1)));
    sel.alloc(size_t(std::max<int64_t>(tot, 1)) * 8);
    DevWords<uint64_t, 1> cnt;
    k_owned_only<<<grid_for(tot), 256, 0, c.stream>>>(all.as<uint64_t>(), tot, c.num_parts, c.world, c.rank, flag.as<uint8_t>());
    select_dev(c, all.as<uint64_t>(), flag.as<uint8_t>(), sel.as<uint64_t>(), cnt.dev(), tot);
    const uint64_t ns = cnt.read(c)[0];
    DevBuf s2;
    s2.alloc(size_t(std::max<uint64_t>(ns, 1)) * 8);
    radix_keys<uint64_t>(c, sel.as<uint64_t>(), s2.as<uint64_t>(), int64_t(ns), 64);
    owned.alloc(size_t(std::max<uint64_t>(ns, 1)) * 8);
    n_owned = ns ? unique_sorted<uint64_t>(c, s2.as<uint64_t>(), owned.as<uint64_t>(), int64_t(ns)) : 0;
    refs.release();
  }
  // counts -> base (rank-major gidx ranges), n_global, n_vertices
  void assign_ranges() {
    counts = c.sharded ? allgather_i64(c, n_owned) : std::vector<int64_t>(1, n_owned);
    // owner ranges padded to 64 vertices: every rank's slice of a frontier bitmap starts on a
    // 64-bit word, so bitmap slices are exchanged without shifting (holes have no edges)
    // A writable snapshot on several ranks also reserves growth room in every owner range (option
    // grow_room_pct of the rank's vertices, at least 1024): a merge commit places new vertices
    // there without moving any rank's range (extend_vertex_map_ranks); a batch that overflows
    // some rank's room takes the full rebuild, which reserves room again.
    const int64_t room_pct = keep && c.sharded ? std::max<int64_t>(0, c.opt("grow_room_pct", 10)) : 0;
    c.base.assign(size_t(c.world) + 1, 0);
    c.counts = counts;
    for (int r = 0; r < c.world; r++) {
      const int64_t room = room_pct ? std::max<int64_t>(1024, counts[size_t(r)] * room_pct / 100) : 0;
      c.base[size_t(r) + 1] = c.base[size_t(r)] + ((counts[size_t(r)] + room + 63) / 64) * 64;
    }
    c.n_global = c.base[size_t(c.world)];
    c.n_vertices = 0;
    for (auto x : counts) c.n_vertices += x;
    if (c.n_global >= (int64_t(1) << 31)) throw Error(NBG_E_UNSUPPORTED, "more than 2^31 vertices");
  }
  // vid_of: every rank's owned table at its base (within a rank by descending out-degree, or by
  // vid with degree_order=0), holes INT64_MIN
  void publish_vertex_map() {
    c.vid_of.alloc(size_t(std::max<int64_t>(c.n_global, 1)) * 8);
    fill<int64_t>(c, c.vid_of.as<int64_t>(), INT64_MIN, c.n_global);
    if (!c.sharded) {
      if (n_owned) k_unflip<<<grid_for(n_owned), 256, 0, c.stream>>>(owned.as<uint64_t>(), c.vid_of.as<int64_t>(), n_owned);
    } else {
      const int64_t mx = *std::max_element(counts.begin(), counts.end());
      DevBuf recv = allgather_padded(c, owned, n_owned, counts, 8, false);
      for (int r = 0; r < c.world; r++)
        if (counts[size_t(r)])
          k_unflip<<<grid_for(counts[size_t(r)]), 256, 0, c.stream>>>(recv.as<uint64_t>() + size_t(r) * size_t(mx),
                                                                       c.vid_of.as<int64_t>() + c.base[size_t(r)],
                                                                       counts[size_t(r)]);
    }
    owned.release();
  }
  // hash table vid -> gidx
  void build_hash() {
    vid_hash_reset(c, c.n_global);
    DevWords<int32_t, 1> dmin;
    dmin.set(c, {-1});
    for (int r = 0; r < c.world; r++)
      vid_hash_insert(c, c.vid_of.as<int64_t>() + c.base[size_t(r)], counts[size_t(r)], c.base[size_t(r)], dmin);
    vid_hash_publish_min(c, dmin);
  }
};

void snapshot_finalize(Ctx& c) {
  if (c.finalized) throw Error(NBG_E_STATE, "snapshot already finalized");
  PoolScope build_scope(build_pool(c));
  struct TrimAfter {  // a read-only snapshot has no further builds: give the cache back
    Ctx& c;
    ~TrimAfter() {
      if (!c.opt("writable", 0)) c.build_pool->trim();
    }
  } trim_after{c};
  double t0 = now_s();
  const bool keep = c.opt("writable", 0) != 0;
  BuildTrace phase(c, "build", t0);
  if (phase.on) {
    g_alloc_clock.alloc_ns = 0;
    g_alloc_clock.free_ns = 0;
    g_alloc_clock.allocs = 0;
  }
  for (auto& kv : c.edges)
    if (kv.second.rmat_stream) {
      finalize_rmat_stream(c, kv.second);
      c.has_log = false;
      c.ws_tmp.release();
      c.finalized = true;
      c.build_seconds += now_s() - t0;
      return;
    }
  VertexMapBuild v{c, keep};
  v.referenced_vids();
  phase("vertex set");
  v.owned_vids();
  order_by_degree(c, v.owned, v.n_owned);
  phase("degree order");
  v.assign_ranges();
  v.publish_vertex_map();
  v.build_hash();
  phase("vertex map + hash");
  build_tag_columns(c);
  phase("tag columns");
  // bytewise order rank of every vertex (for CSR row order = RocksDB key order)
  DevBuf brank = bytewise_ranks(c);
  phase("bytewise ranks");
  for (auto& kv : c.edges) {
    EdgeSpace& es = kv.second;
    build_csr(c, es.out_stage, es.fields, true, es.out, brank.as<uint32_t>(), !keep, &es.ord[0]);
    phase("out CSR");
    build_csr(c, es.in_stage, es.fields, false, es.in, brank.as<uint32_t>(), !keep, &es.ord[1]);
    phase("in CSR");
    if (c.opt("bottom_up", 1)) build_transpose(c, es);
    phase("transpose + slabs");
  }
  if (!keep) {
    c.heap.release();
    c.heap_used = 0;
  } else {
    c.brank = std::move(brank);  // the batch keys of a merge commit
    for (auto& kv : c.tags) kv.second.committed_n = kv.second.stage.n;
  }
  c.has_log = keep;
  c.ws_tmp.release();
  NBG_HIP(hipStreamSynchronize(c.stream));
  c.finalized = true;
  c.build_seconds += now_s() - t0;
}

}  // namespace nbg
