// expr_device.h -- the device expression VM: the value model, the column loads and the postfix
// evaluator of a compiled Program (program.h), plus the typed-compare fast path.  Shared by the
// query translation units (expand.hip, yield.hip, bound.hip); everything here is inlined into
// their kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nebula_amd.h"
#include "program.h"
#include "qpred.h"

namespace nbg {

// ------------------------------------------------------------------------------------------
// device value model (boost::variant<int64,double,bool,string> + error)
// ------------------------------------------------------------------------------------------
struct Val {
  int64_t b;
  int32_t t;
  int32_t len;
};

struct PropDev {
  int32_t type;
  int32_t width;
  const void* data;
  const uint8_t* present;
  const int64_t* str_off;
  const uint8_t* str_bytes;
  const int32_t* part;  // tag columns: the part of each vertex's row (TagSpace::part)
};
struct EvalEnv {
  const PropDev* props;  // device table, one entry per schema field (Csr::prop_table)
  int32_t nprops;
  int32_t etype;
  const int64_t* vid_of;
  const int32_t* col;
  const int64_t* rank;
  const PropDev* tprops;  // tag columns over the gidx space (Ctx::tag_refs order), or null
  // $- / $var input table: open-addressing index src gidx -> its last input row, and columns
  const int32_t* in_keys;
  const int32_t* in_rows;
  uint32_t in_mask;
  const PropDev* iprops;
  // STEPS > 1: root start (vid rank) of every final-frontier vertex and rank -> start gidx
  const int32_t* in_root;
  const int32_t* in_root_tab;
  // storage (getBound) filters: a $^ tag row is visible when it sits in the request's part,
  // which for an edge row is the part of the row's keys (Csr::row_part, local row = src - lo)
  int32_t storage;
  int64_t lo;
  const int32_t* row_part;
};
__device__ inline uint32_t gidx_hash(int32_t g) { return uint32_t(g) * 2654435761u; }
// row of the input table whose FROM vid is gidx g (-1: none)
__device__ inline int32_t input_row(const EvalEnv& env, int32_t g) {
  uint32_t h = gidx_hash(g) & env.in_mask;
  for (uint32_t probe = 0; probe <= env.in_mask; probe++) {
    const int32_t k = env.in_keys[h];
    if (k == g) return env.in_rows[h];
    if (k < 0) return -1;
    h = (h + 1) & env.in_mask;
  }
  return -1;
}

__device__ inline int64_t load_int(const void* data, int width, int64_t i) {
  switch (width) {
    case 1: return int64_t(static_cast<const int8_t*>(data)[i]);
    case 2: return int64_t(static_cast<const int16_t*>(data)[i]);
    case 4: return int64_t(static_cast<const int32_t*>(data)[i]);
    default: return static_cast<const int64_t*>(data)[i];
  }
}

// compile-time width variant (W = 0: runtime width)
template <int W>
__device__ inline int64_t load_w(const void* data, int width, int64_t i) {
  if (W == 1) return int64_t(static_cast<const int8_t*>(data)[i]);
  if (W == 2) return int64_t(static_cast<const int16_t*>(data)[i]);
  if (W == 4) return int64_t(static_cast<const int32_t*>(data)[i]);
  if (W == 8) return static_cast<const int64_t*>(data)[i];
  return load_int(data, width, i);
}

__device__ inline Val load_prop(const PropDev& p, int64_t ge) {
  Val v;
  v.len = 0;
  if (p.present && !p.present[ge]) {
    v.t = VT_ERR;
    v.b = 0;
    return v;
  }
  switch (p.type) {
    case NBG_T_DOUBLE:
    case NBG_T_FLOAT:
      v.t = VT_DOUBLE;
      v.b = static_cast<const int64_t*>(p.data)[ge];
      break;
    case NBG_T_BOOL:
      v.t = VT_BOOL;
      v.b = load_int(p.data, p.width, ge) != 0;
      break;
    case NBG_T_STRING: {
      int64_t o = p.str_off[ge];
      v.t = VT_STR;
      v.b = int64_t(reinterpret_cast<uintptr_t>(p.str_bytes + o));
      v.len = int32_t(p.str_off[ge + 1] - o);
      break;
    }
    default:
      v.t = VT_INT;
      v.b = load_int(p.data, p.width, ge);
  }
  return v;
}

__device__ inline double as_d(const Val& v) { return v.t == VT_INT ? double(v.b) : __longlong_as_double(v.b); }
__device__ inline bool as_bool(const Val& v) {
  switch (v.t) {
    case VT_INT: return v.b != 0;
    case VT_DOUBLE: return __longlong_as_double(v.b) != 0.0;
    case VT_BOOL: return v.b != 0;
    default: return v.len == 0;  // string -> empty() (Expressions.h:172-173)
  }
}
__device__ inline int str_cmp(const Val& a, const Val& b) {
  const uint8_t* x = reinterpret_cast<const uint8_t*>(uintptr_t(a.b));
  const uint8_t* y = reinterpret_cast<const uint8_t*>(uintptr_t(b.b));
  int n = a.len < b.len ? a.len : b.len;
  for (int i = 0; i < n; i++)
    if (x[i] != y[i]) return x[i] < y[i] ? -1 : 1;
  return a.len == b.len ? 0 : (a.len < b.len ? -1 : 1);
}
// boost::variant operator< : index first, then value
__device__ inline bool v_lt(const Val& a, const Val& b) {
  if (a.t != b.t) return a.t < b.t;
  switch (a.t) {
    case VT_INT: return a.b < b.b;
    case VT_DOUBLE: return __longlong_as_double(a.b) < __longlong_as_double(b.b);
    case VT_BOOL: return a.b < b.b;
    default: return str_cmp(a, b) < 0;
  }
}
__device__ inline bool v_eq(const Val& a, const Val& b) {
  if (a.t != b.t) return false;
  switch (a.t) {
    case VT_INT:
    case VT_BOOL: return a.b == b.b;
    case VT_DOUBLE: return __longlong_as_double(a.b) == __longlong_as_double(b.b);
    default: return str_cmp(a, b) == 0;
  }
}
__device__ inline Val mk(int32_t t, int64_t b) {
  Val v;
  v.t = t;
  v.b = b;
  v.len = 0;
  return v;
}
__device__ inline Val mkd(double d) { return mk(VT_DOUBLE, __double_as_longlong(d)); }

__device__ inline Val eval_program(const Program* __restrict__ P, const EvalEnv& env, int64_t ge, int32_t src_g,
                                   int32_t dst_g) {
  Val st[kMaxStack];
  int sp = 0;
  const int n = P->n;
  for (int pc = 0; pc < n; pc++) {
    Ins in = P->ins[pc];
    switch (in.op) {
      case P_CONST: {
        Val v;
        v.t = P->ctype[in.arg];
        v.b = P->cbits[in.arg];
        v.len = P->clen[in.arg];
        if (v.t == VT_STR) v.b = int64_t(reinterpret_cast<uintptr_t>(P->cstr + P->cbits[in.arg]));
        st[sp++] = v;
        break;
      }
      case P_PROP: st[sp++] = load_prop(env.props[in.arg], ge); break;
      case P_DST: st[sp++] = mk(VT_INT, env.vid_of[dst_g]); break;
      case P_SRC: st[sp++] = mk(VT_INT, env.vid_of[src_g]); break;
      case P_RANK: st[sp++] = mk(VT_INT, env.rank ? env.rank[ge] : 0); break;
      case P_TYPE: st[sp++] = mk(VT_INT, env.etype); break;
      case P_SRCTAG:
      case P_DSTTAG: {
        // only a row of the vertex's own part is visible to GO (presence byte 1; 2 = a row that
        // only a getBound naming its foreign part reads)
        const PropDev& tp = env.tprops[in.arg];
        const int32_t g = in.op == P_SRCTAG ? src_g : dst_g;
        const bool vis = env.storage ? tp.present[g] != 0 && tp.part[g] == env.row_part[src_g - env.lo]
                                     : tp.present[g] == 1;
        st[sp++] = vis ? load_prop(tp, g) : mk(VT_ERR, 0);
        break;
      }
      case P_INPUT: {
        int32_t g0 = src_g;
        if (env.in_root) {  // multi-step: the input row of the vertex's root start
          const int32_t r = env.in_root[src_g];
          g0 = r == INT32_MAX ? -1 : env.in_root_tab[r];
        }
        const int32_t row = g0 < 0 ? -1 : input_row(env, g0);
        st[sp++] = row < 0 ? mk(VT_ERR, 0) : load_prop(env.iprops[in.arg], row);
        break;
      }
      case P_UNARY: {
        Val& a = st[sp - 1];
        if (a.t == VT_ERR) break;
        if (in.sub == 0) break;  // PLUS
        if (in.sub == 1) {       // NEGATE
          if (a.t == VT_INT) a.b = int64_t(0ull - uint64_t(a.b));
          else if (a.t == VT_DOUBLE) a.b = __double_as_longlong(-__longlong_as_double(a.b));
          else a.t = VT_ERR;
        } else {
          a = mk(VT_BOOL, !as_bool(a));
        }
        break;
      }
      case P_ARITH: {
        Val r = st[--sp];
        Val l = st[sp - 1];
        Val o;
        if (l.t == VT_ERR) o = l;
        else if (r.t == VT_ERR) o = r;
        else {
          bool ar = (l.t == VT_INT || l.t == VT_DOUBLE) && (r.t == VT_INT || r.t == VT_DOUBLE);
          bool dbl = l.t == VT_DOUBLE || r.t == VT_DOUBLE;
          o = mk(VT_ERR, 0);
          switch (in.sub) {
            case 0:
              if (ar) o = dbl ? mkd(as_d(l) + as_d(r)) : mk(VT_INT, int64_t(uint64_t(l.b) + uint64_t(r.b)));
              break;
            case 1:
              if (ar) o = dbl ? mkd(as_d(l) - as_d(r)) : mk(VT_INT, int64_t(uint64_t(l.b) - uint64_t(r.b)));
              break;
            case 2:
              if (ar) o = dbl ? mkd(as_d(l) * as_d(r)) : mk(VT_INT, int64_t(uint64_t(l.b) * uint64_t(r.b)));
              break;
            case 3:
              if (ar) {
                if (dbl) o = mkd(as_d(l) / as_d(r));
                else if (r.b == 0) o = mk(VT_ERR, 0);
                else if (r.b == -1) o = mk(VT_INT, int64_t(0ull - uint64_t(l.b)));
                else o = mk(VT_INT, l.b / r.b);
              }
              break;
            default:
              if (l.t == VT_INT && r.t == VT_INT) {
                if (r.b == 0) o = mk(VT_ERR, 0);
                else if (r.b == -1) o = mk(VT_INT, 0);
                else o = mk(VT_INT, l.b % r.b);
              }
          }
        }
        st[sp - 1] = o;
        break;
      }
      case P_REL: {
        Val r = st[--sp];
        Val l = st[sp - 1];
        Val o;
        if (l.t == VT_ERR) o = l;
        else if (r.t == VT_ERR) o = r;
        else {
          bool res;
          bool mixed = (l.t == VT_INT || l.t == VT_DOUBLE) && (r.t == VT_INT || r.t == VT_DOUBLE) &&
                       (l.t == VT_DOUBLE || r.t == VT_DOUBLE);
          switch (in.sub) {
            case 0: res = v_lt(l, r); break;
            case 1: res = !v_lt(r, l); break;
            case 2: res = v_lt(r, l); break;
            case 3: res = !v_lt(l, r); break;
            case 4: res = mixed ? fabs(as_d(l) - as_d(r)) < 1e-8 : v_eq(l, r); break;
            default: res = mixed ? !(fabs(as_d(l) - as_d(r)) < 1e-8) : !v_eq(l, r); break;
          }
          o = mk(VT_BOOL, res);
        }
        st[sp - 1] = o;
        break;
      }
      case P_LOGIC: {
        Val r = st[--sp];
        Val l = st[sp - 1];
        Val o;
        if (l.t == VT_ERR) o = l;
        else if (r.t == VT_ERR) o = r;
        else if (in.sub == 0) o = mk(VT_BOOL, as_bool(l) ? as_bool(r) : false);
        else o = mk(VT_BOOL, as_bool(l) ? true : as_bool(r));
        st[sp - 1] = o;
        break;
      }
    }
  }
  return st[0];
}

// how a kernel evaluates its predicate (FastPred::kind): none, one typed compare, or the VM
enum PredKind : int { PK_NONE = 0, PK_FAST = 1, PK_VM = 2 };

// PK_FAST: column `data` (int, `width` bytes) `op` constant k; an absent value is an eval error
struct FastArgs {
  const void* data;
  const uint8_t* present;
  int32_t width;
  int32_t op;
  int64_t k;
};
// the compare itself: fast_cmp (qpred.h)

}  // namespace nbg
