// row_gather.h -- the row-table plumbing nbg_order_by, nbg_set_op and nbg_group_by share (included
// by order.hip, setops.hip and group.hip; every definition is translation-unit local):
//   check_plain_table  the argument checks of a plain row table
//   upload_table       a host table's columns to HBM (a device table is read in place)
//   gather_rows        output columns = input columns permuted / selected by a uint32 row index
//                      (k_ord_gather; STRING columns k_ord_str_lens -> scan -> k_ord_str_copy)
//   hand_out_rows      device blocks, or host copies through the pinned result blocks
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "query_common.h"
#include "rows.h"

namespace nbg {
namespace {

constexpr int kOrdThreads = 256;

constexpr int kGatherCols = 16;
struct GatherCols {
  const void* src[kGatherCols];
  void* dst[kGatherCols];
  int32_t width[kGatherCols];  // 8 or 1 bytes per value
  int32_t n;
};

// dst[c][i] = src[c][idx[i]] for every fixed-width column; a thread takes four consecutive
// output rows (one 16-byte load of the index, 32-byte / 4-byte stores per column)
__global__ __launch_bounds__(kOrdThreads) void k_ord_gather(GatherCols g, const uint32_t* __restrict__ idx, int64_t n) {
  const int64_t quads = (n + 3) / 4;
  for (int64_t q = int64_t(blockIdx.x) * kOrdThreads + threadIdx.x; q < quads; q += int64_t(gridDim.x) * kOrdThreads) {
    const int64_t i0 = q * 4;
    uint32_t r[4];
    const int m = int(min(int64_t(4), n - i0));
    if (m == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(idx + i0);
      r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
    } else {
      for (int e = 0; e < 4; e++) r[e] = e < m ? idx[i0 + e] : 0;
    }
    for (int c = 0; c < g.n; c++) {
      if (g.width[c] == 8) {
        const uint64_t* src = static_cast<const uint64_t*>(g.src[c]);
        uint64_t* dst = static_cast<uint64_t*>(g.dst[c]);
        uint64_t v[4];
        for (int e = 0; e < 4; e++) v[e] = e < m ? src[r[e]] : 0;
        if (m == 4) {
          *reinterpret_cast<ulonglong2*>(dst + i0) = make_ulonglong2(v[0], v[1]);
          *reinterpret_cast<ulonglong2*>(dst + i0 + 2) = make_ulonglong2(v[2], v[3]);
        } else {
          for (int e = 0; e < m; e++) dst[i0 + e] = v[e];
        }
      } else {
        const uint8_t* src = static_cast<const uint8_t*>(g.src[c]);
        uint8_t* dst = static_cast<uint8_t*>(g.dst[c]);
        uint8_t v[4];
        for (int e = 0; e < 4; e++) v[e] = e < m ? src[r[e]] : 0;
        if (m == 4) {
          *reinterpret_cast<uchar4*>(dst + i0) = make_uchar4(v[0], v[1], v[2], v[3]);
        } else {
          for (int e = 0; e < m; e++) dst[i0 + e] = v[e];
        }
      }
    }
  }
}

// STRING output: the permuted lengths (lens[n] = 0, so the scan's last word is the byte total) ...
__global__ void k_ord_str_lens(const int64_t* __restrict__ off, const uint32_t* __restrict__ idx, int64_t n,
                               int64_t* __restrict__ lens) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += int64_t(gridDim.x) * blockDim.x) {
    if (i == n) {
      lens[i] = 0;
    } else {
      const int64_t r = idx ? int64_t(idx[i]) : i;
      lens[i] = off[r + 1] - off[r];
    }
  }
}
// ... and the bytes: 16 lanes copy one value
__global__ void k_ord_str_copy(const uint8_t* __restrict__ src, const int64_t* __restrict__ off,
                               const uint32_t* __restrict__ idx, int64_t n, const int64_t* __restrict__ new_off,
                               uint8_t* __restrict__ dst) {
  const int sub = threadIdx.x & 15;
  for (int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / 16; i < n; i += int64_t(gridDim.x) * blockDim.x / 16) {
    const int64_t r = idx ? int64_t(idx[i]) : i;
    const int64_t a = off[r], len = off[r + 1] - a, b = new_off[i];
    for (int64_t j = sub; j < len; j += 16) dst[b + j] = src[a + j];
  }
}

int grid_for(int64_t work_items, int per_block, int64_t cap = 4096) {
  return int(std::max<int64_t>(1, std::min<int64_t>((work_items + per_block - 1) / per_block, cap)));
}

struct InCol {
  int32_t type = 0;
  const void* data = nullptr;    // device
  const int64_t* off = nullptr;  // device, STRING
  int64_t str_bytes = 0;
};

bool int_like(int32_t t) { return t == NBG_T_INT || t == NBG_T_VID || t == NBG_T_TIMESTAMP; }

void kernel_launched(Ctx& c) {
  NBG_HIP(hipGetLastError());
  c.timing.launches++;
}

void scan_i64(Ctx& c, const int64_t* in, int64_t* out, int64_t n) {
  exclusive_scan_dev<int64_t>(c, in, out, n);
  c.timing.launches++;
}

// `who`: the call's name in the messages ("order_by", "set_op")
void check_plain_table(const nbg_rows& in, const std::string& who) {
  if (in.n_rows < 0 || in.n_cols < 0 || (in.n_cols && (!in.col_types || !in.cols)))
    throw Error(NBG_E_INVALID_ARG, who + ": malformed input table");
  if (in.row_vertex || in.n_vertices || in.vertex_ids || in.n_failed || in.path_offsets || in.path_vids ||
      in.n_vertex_cols)
    throw Error(NBG_E_INVALID_ARG, who + ": the input must be a plain row table (no get_bound / path parts)");
  for (int32_t k = 0; k < in.n_cols; k++) {
    const int32_t t = in.col_types[k];
    if (t != NBG_T_BOOL && t != NBG_T_INT && t != NBG_T_VID && t != NBG_T_DOUBLE && t != NBG_T_STRING &&
        t != NBG_T_TIMESTAMP)
      throw Error(NBG_E_INVALID_ARG, who + ": unknown column type");
    if (in.n_rows > 0 && (!in.cols[k] || (t == NBG_T_STRING && (!in.str_offsets || !in.str_offsets[k]))))
      throw Error(NBG_E_INVALID_ARG, who + ": null column");
  }
}

// the input columns in HBM (a host table is uploaded into `up`; a device table is read in place)
std::vector<InCol> upload_table(Ctx& c, const nbg_rows& in, std::vector<DevBuf>& up, const std::string& who) {
  const int64_t n = in.n_rows;
  const size_t ncols = size_t(in.n_cols);
  std::vector<InCol> cols(ncols);
  for (size_t k = 0; k < ncols; k++) {
    InCol& ic = cols[k];
    ic.type = in.col_types[k];
    const size_t w = ic.type == NBG_T_BOOL ? 1 : 8;
    if (ic.type == NBG_T_STRING) {
      if (n == 0) continue;
      if (in.on_device) {
        ic.data = in.cols[k];
        ic.off = in.str_offsets[k];
        int64_t total = 0;
        NBG_HIP(hipMemcpyAsync(&total, ic.off + n, 8, hipMemcpyDeviceToHost, c.stream));
        NBG_HIP(hipStreamSynchronize(c.stream));
        c.timing.host_waits++;
        ic.str_bytes = total;
      } else {
        const int64_t* ho = in.str_offsets[k];
        if (ho[0] != 0 || ho[n] < 0) throw Error(NBG_E_INVALID_ARG, who + ": STRING offsets must start at 0");
        ic.str_bytes = ho[n];
        DevBuf o, b;
        o.alloc(size_t(n + 1) * 8);
        b.alloc(size_t(ic.str_bytes) + 8);
        NBG_HIP(hipMemcpyAsync(o.p, ho, size_t(n + 1) * 8, hipMemcpyHostToDevice, c.stream));
        if (ic.str_bytes) NBG_HIP(hipMemcpyAsync(b.p, in.cols[k], size_t(ic.str_bytes), hipMemcpyHostToDevice, c.stream));
        ic.off = o.as<int64_t>();
        ic.data = b.p;
        up.push_back(std::move(o));
        up.push_back(std::move(b));
      }
    } else if (in.on_device || n == 0) {
      ic.data = in.cols[k];
    } else {
      DevBuf b;
      b.alloc(size_t(n) * w);
      NBG_HIP(hipMemcpyAsync(b.p, in.cols[k], size_t(n) * w, hipMemcpyHostToDevice, c.stream));
      ic.data = b.p;
      up.push_back(std::move(b));
    }
  }
  return cols;
}

// dev[k] (allocated here) = column k's rows idx[0, n_out), n_out > 0; out_off[k] = a STRING
// column's new offsets.  idx == nullptr: the rows in input order (n_out = the input's rows), a copy.
// A STRING column's block holds the input's bytes (str_bytes: no output has more).
void gather_rows(Ctx& c, const std::vector<InCol>& cols, const uint32_t* idx, int64_t n_out, std::vector<DevBuf>& dev,
                 std::vector<DevBuf>& out_off) {
  const int64_t n = n_out;
  GatherCols g{};
  auto flush = [&]() {
    if (!g.n) return;
    k_ord_gather<<<grid_for(n, kOrdThreads * 4), kOrdThreads, 0, c.stream>>>(g, idx, n);
    kernel_launched(c);
    g.n = 0;
  };
  for (size_t k = 0; k < cols.size(); k++) {
    const InCol& ic = cols[k];
    if (ic.type == NBG_T_STRING) {
      DevBuf lens;
      lens.alloc(size_t(n + 1) * 8);
      out_off[k].alloc(size_t(n + 1) * 8);
      k_ord_str_lens<<<grid_for(n + 1, 256), 256, 0, c.stream>>>(ic.off, idx, n, lens.as<int64_t>());
      kernel_launched(c);
      scan_i64(c, lens.as<int64_t>(), out_off[k].as<int64_t>(), n + 1);
      dev[k].alloc(size_t(ic.str_bytes) + 8);
      if (ic.str_bytes) {
        k_ord_str_copy<<<grid_for(n, 16), 256, 0, c.stream>>>(static_cast<const uint8_t*>(ic.data), ic.off, idx, n,
                                                             out_off[k].as<int64_t>(), dev[k].as<uint8_t>());
        kernel_launched(c);
      }
      continue;
    }
    const size_t w = ic.type == NBG_T_BOOL ? 1 : 8;
    dev[k].alloc(size_t(n) * w);
    if (!idx) {  // nothing moved (no factor, or constant factors): a copy
      NBG_HIP(hipMemcpyAsync(dev[k].p, ic.data, size_t(n) * w, hipMemcpyDeviceToDevice, c.stream));
      continue;
    }
    g.src[g.n] = ic.data;
    g.dst[g.n] = dev[k].p;
    g.width[g.n] = int32_t(w);
    if (++g.n == kGatherCols) flush();
  }
  flush();
}

// hand out h (types and dev filled, n rows): device blocks, or host copies through the pinned
// result blocks.  str_bytes[k]: the bytes of STRING column k to copy (at least its offsets' last
// word; its block holds that many).  Ends with the call's last stream synchronisation.
void hand_out_rows(Ctx& c, std::unique_ptr<HostRows> h, std::vector<DevBuf>& out_off, const std::vector<int64_t>& str_bytes,
                   int64_t n, bool keep_on_device, nbg_rows* out) {
  const size_t ncols = h->types.size();
  for (size_t k = 0; k < ncols; k++) {
    const bool is_str = h->types[k] == NBG_T_STRING;
    if (keep_on_device) {
      h->cols.push_back(h->dev[k].p);
      if (is_str && n > 0) {
        h->str_off.push_back(out_off[k].as<int64_t>());
        h->dev.push_back(std::move(out_off[k]));
      } else {
        h->str_off.push_back(nullptr);
      }
      continue;
    }
    if (is_str) {
      h->host_off.emplace_back(size_t(n) + 1, 0);
      h->host.emplace_back(size_t(str_bytes[k]) + 8);
      if (n > 0) {
        NBG_HIP(hipMemcpyAsync(h->host_off.back().data(), out_off[k].p, size_t(n + 1) * 8, hipMemcpyDeviceToHost, c.stream));
        if (str_bytes[k])
          NBG_HIP(hipMemcpyAsync(h->host.back().data(), h->dev[k].p, size_t(str_bytes[k]), hipMemcpyDeviceToHost,
                                 c.stream));
      }
      h->cols.push_back(h->host.back().data());
      h->str_off.push_back(h->host_off.back().data());
      continue;
    }
    const size_t w = h->types[k] == NBG_T_BOOL ? 1 : 8;
    h->hpin.emplace_back();
    if (h->hpin.size() == 1) host_pool_cap(c);
    h->hpin.back().alloc(c.host_pool, size_t(n) * w + 8);
    if (n > 0) NBG_HIP(hipMemcpyAsync(h->hpin.back().p, h->dev[k].p, size_t(n) * w, hipMemcpyDeviceToHost, c.stream));
    h->cols.push_back(h->hpin.back().p);
    h->str_off.push_back(nullptr);
  }
  NBG_HIP(hipStreamSynchronize(c.stream));  // the result is complete, and uploaded inputs may be released
  c.timing.host_waits++;
  if (!keep_on_device) h->dev.clear();
  fill_rows(out, std::move(h), n, keep_on_device);
}

}  // namespace
}  // namespace nbg
