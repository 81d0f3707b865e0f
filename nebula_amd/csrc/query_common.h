// query_common.h -- host-side helpers the .hip translation units share: grid sizing, the rocprim
// scan / select wrappers, and the entry points of the expansion (expand.hip) and the YIELD
// materialiser (yield.hip) that bound.hip and fetch.hip call.
#pragma once
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <vector>

#include "engine.h"
#include "expr_device.h"

namespace nbg {

inline int grid_cap(int64_t n, int block = 256, int cap = 256 * 16) {
  int64_t g = (n + block - 1) / block;
  return int(std::max<int64_t>(1, std::min<int64_t>(g, cap)));
}

template <typename T>
void exclusive_scan_dev(Ctx& c, const T* in, T* out, int64_t n) {
  size_t tb = 0;
  NBG_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, T(0), size_t(n), rocprim::plus<T>(), c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::exclusive_scan(c.ws_tmp.p, tb, in, out, T(0), size_t(n), rocprim::plus<T>(), c.stream));
}

// the same over bytes (keep flags): out[i] = in[0] + ... + in[i - 1] as uint32
inline void exclusive_scan_dev(Ctx& c, const uint8_t* in, uint32_t* out, int64_t n) {
  size_t tb = 0;
  NBG_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, uint32_t(0), size_t(n), rocprim::plus<uint32_t>(), c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::exclusive_scan(c.ws_tmp.p, tb, in, out, uint32_t(0), size_t(n), rocprim::plus<uint32_t>(), c.stream));
}

// rocprim::select in its two calls (size query, run): in[i] with flags[i] != 0 to out, in order;
// their count to *cnt (device)
template <typename In, typename Flags, typename Out>
void select_dev(Ctx& c, In in, Flags flags, Out out, uint64_t* cnt, int64_t n) {
  size_t tb = 0;
  NBG_HIP(rocprim::select(nullptr, tb, in, flags, out, cnt, size_t(n), c.stream));
  c.ws_tmp.ensure(tb);
  NBG_HIP(rocprim::select(c.ws_tmp.p, tb, in, flags, out, cnt, size_t(n), c.stream));
}

// device descriptors of a column list, appended to tab (part: TagSpace::part of tag columns)
inline void append_prop_devs(std::vector<PropDev>& tab, const std::vector<PropCol>& cols, const int32_t* part = nullptr) {
  for (const PropCol& p : cols)
    tab.push_back(PropDev{p.type, p.width, p.data.p, p.present.as<uint8_t>(), p.str_off.as<int64_t>(),
                          p.str_bytes.as<uint8_t>(), part});
}

enum ExpMode : int { EXP_MARK = 0, EXP_ROWS = 1, EXP_FLAGS = 2 };

struct ExpandArgs {
  const int32_t* F;
  int64_t nF;
  const int64_t* off;      // exclusive degree scan, off[nF] = total edges
  const int64_t* row_ptr;
  const int32_t* col;
  int64_t lo;              // gidx of local row 0
  uint8_t* map;            // EXP_MARK
  int32_t* rows_src;       // EXP_ROWS: local row index
  int64_t* rows_edge;      //           global edge index into the CSR
  unsigned long long* rows_cnt;
  uint8_t* flags;          // EXP_FLAGS: one byte per flattened edge slot
  unsigned long long* err; // eval errors (GO semantics)
  int32_t storage;         // 1: eval error keeps the edge (QueryBaseProcessor.inl:391-396)
  int32_t mark_check;      // read the byte before storing it
  int64_t* out_vid;        // EXP_ROWS fused YIELD _dst: write vid_of[dst] instead of (src, edge)
  const int64_t* vid_of;
  const int64_t* col_vid;  // per-edge dst vid (Csr::col_vid) or null: vid_of[col[e]]
  const int32_t* tile_row; // [ntiles + 1]: frontier entry holding the first slot of each tile
                           // (k_tile_rows), or null: binary search of off[]
  // multi-step $- / $var (VertexBackTracker, GoExecutor.h:174-193): root start of every marked
  // dst = the smallest (by vid rank) root of its in-edges' srcs this hop, or null
  const int32_t* root_cur;
  int32_t* root_next;
};

// ---- defined in expand.hip ----
EvalEnv make_env(Ctx& c, EdgeSpace& es, Csr& csr, int32_t etype);  // builds the column tables on first use
FastArgs fast_args(const Csr& csr, const FastPred& fpk);
uint64_t expand_bytes(int64_t nF, int64_t E, int pred_width, int mode);
// the EXP_FLAGS expansion: a.flags[slot] = the edge at that slot passes the predicate
void expand_flags(Ctx& c, ExpandArgs a, int pk, const FastArgs& fp, const Program* dprog, const EvalEnv& env, int64_t E);

// ---- defined in yield.hip ----
// the type a stored column is returned as: FLOAT widens to DOUBLE, VID and TIMESTAMP are INTs
int32_t column_result_type(int32_t t);
// the YIELD materialiser (k_materialize, k_str_pack) over n rows (rows_src[i] + lo = the row's src
// gidx, rows_edge[i] = its edge in env's CSR; rows_edge == nullptr: vertex rows, whose programs hold
// only P_SRCTAG and constants).  out: one column per program, STRING columns as packed bytes + n + 1
// offsets, ready for hand_out_rows.  An evaluation error on any row throws NBG_E_EVAL (err_what).
constexpr int kMaxYieldCols = 16;  // YieldArgs::cols (go_launch.h kMaxYields)
struct YieldOut {
  std::vector<int32_t> types;  // NBG_T_*
  std::vector<DevBuf> dev, off;
  std::vector<int64_t> str_bytes;
};
void yield_rows(Ctx& c, const std::vector<Program>& progs, const EvalEnv& env, const int32_t* rows_src,
                const int64_t* rows_edge, int64_t lo, int64_t n, const char* err_what, YieldOut& out);

// ---- defined in setops.hip ----
// one column of a table in HBM (row_gather.h's InCol for callers in another translation unit)
struct TableCol {
  int32_t type;  // NBG_T_*
  const void* data;
  const int64_t* off;  // STRING
  int64_t str_bytes;
};
// the first row of every class of equal rows (nbg_set_op's row equality), as row numbers in input
// order in idx: UNION DISTINCT's hash build and probe over one table.  n > 0; returns their count
// (one host wait)
int64_t distinct_first_rows(Ctx& c, const std::vector<TableCol>& cols, int64_t n, DevBuf& idx);

// ---- defined in order.hip ----
// idx = the row numbers [0, n) in a stable ascending order of keys[row] (ORDER BY's radix sort,
// one host wait); false, and idx untouched, when every key is the same.  n > 0
bool order_rows_by_u32(Ctx& c, const uint32_t* keys, int64_t n, DevBuf& idx);

}  // namespace nbg
