// qpred.h -- the arithmetic of the typed compare (PK_FAST) and of the quantised predicate on
// packed bottom-up words (host and device).
//
// A packed word is (bucket << gbits) | src gidx, the bucket that of the packed column's value:
//   q_bucket     value -> bucket, floor((v - min) * 2^bits / range)             (csr_build.hip)
//   make_qargs_core (min, range, bits, gbits, op, k) -> QArgs: which buckets the compare decides
//   q_test       word -> 1 pass / 0 fail / -1 undecided        (k_bu_lean, k_bu_rest_lean, k_expand)
//   fin_args     QArgs -> FinArgs: the same decisions as unsigned word ranges           (k_bu_fin)
//   fin_candidate / fin_pass and their CLS-1 forms: k_bu_fin's two tests of a word
// Plain functions only: tests/cpp/qpred_test.cpp compiles this header with the host compiler.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NBG_HD __host__ __device__ inline
#else
#define NBG_HD inline
#endif

namespace nbg {

// PK_FAST: value `a` `op` constant k (op: 0 < 1 <= 2 > 3 >= 4 == 5 !=)
NBG_HD bool fast_cmp(int op, int64_t a, int64_t k) {
  switch (op) {
    case 0: return a < k;
    case 1: return a <= k;
    case 2: return a > k;
    case 3: return a >= k;
    case 4: return a == k;
    default: return a != k;
  }
}

// the quantised bucket of v: floor((v - min) * 2^bits / range) (range 0 = 2^64)
NBG_HD uint32_t q_bucket(int64_t v, int64_t vmin, uint64_t range, int bits) {
  const unsigned __int128 d = (unsigned __int128)(uint64_t(v) - uint64_t(vmin)) << bits;
  const unsigned __int128 r = range ? (unsigned __int128)range : ((unsigned __int128)1 << 64);
  return uint32_t(d / r);
}

// Quantised predicate on packed bottom-up words (EdgeSpace::q_*): the low gbits bits are the
// source gidx, the bits above the bucket of the predicate column's value.  The compare decides
// every bucket below ulo (`below`: 1 pass, 0 fail) and above uhi (`above`); buckets in
// [ulo, uhi] hold the constant and need the exact value (-1).  Host-built per query
// (make_qargs_core); all scalars, so the test is two compares, no table loads.  Unpacked words:
// gmask all ones, ulo 0, uhi INT_MAX (every word undecided).
struct QArgs {
  uint32_t gmask = 0xffffffffu;
  int32_t gbits = 0;
  int32_t ulo = 0, uhi = INT32_MAX;
  int32_t below = -1, above = -1;
};
// 1 pass, 0 fail, -1 undecided (load the value)
NBG_HD int q_test(int32_t s, const QArgs& q) {
  const int32_t b = int32_t(uint32_t(s) >> q.gbits);
  int r = -1;
  r = b > q.uhi ? q.above : r;
  r = b < q.ulo ? q.below : r;
  return r;
}

// first offset of bucket b from the column's minimum: ceil(b * range / 2^bits) (range 0 = 2^64)
inline unsigned __int128 q_edge(uint64_t b, uint64_t range, int bits) {
  using u128 = unsigned __int128;
  const u128 R = range ? u128(range) : (u128(1) << 64);
  return ((u128(b) * R) + ((u128(1) << bits) - 1)) >> bits;  // ceil
}

// QArgs of `packed column op k` on words packed with (vmin, range, bits, gbits).  Bucket b holds the
// values min + [ceil(b * range / 2^bits), ceil((b + 1) * range / 2^bits) - 1]; it passes (fails)
// when every value in it passes (fails) the compare, else the kernels read the exact value.
inline QArgs make_qargs_core(int64_t vmin, uint64_t range, int bits, int gbits, int op, int64_t k) {
  QArgs q;
  q.gmask = (1u << gbits) - 1u;
  q.gbits = gbits;
  using u128 = unsigned __int128;
  const int nb = 1 << bits;
  // per bucket: 1 pass, 0 fail, -1 undecided, 2 empty (no value lands there: either answer)
  std::vector<int> dec(size_t(nb), 2);
  for (int b = 0; b < nb; b++) {
    const u128 o0 = q_edge(uint64_t(b), range, bits), o1 = q_edge(uint64_t(b) + 1, range, bits);
    if (o0 >= o1) continue;
    const int64_t lo = int64_t(uint64_t(vmin) + uint64_t(o0));
    const int64_t hi = int64_t(uint64_t(vmin) + uint64_t(o1 - 1));
    bool pass, fail;
    if (op == 4) {  // ==
      pass = lo == k && hi == k;
      fail = k < lo || k > hi;
    } else if (op == 5) {  // !=
      pass = k < lo || k > hi;
      fail = lo == k && hi == k;
    } else {  // monotone compares: both ends decide the bucket
      const bool x = fast_cmp(op, lo, k), z = fast_cmp(op, hi, k);
      pass = x && z;
      fail = !x && !z;
    }
    dec[size_t(b)] = pass ? 1 : fail ? 0 : -1;
  }
  // below: the first non-empty bucket's answer, up to the first bucket answering otherwise;
  // above: the last one's, down to the last bucket answering otherwise; between: undecided
  int first = 2, last = 2;
  for (int b = 0; b < nb && first == 2; b++) first = dec[size_t(b)];
  for (int b = nb - 1; b >= 0 && last == 2; b--) last = dec[size_t(b)];
  if (first == 2) return q;  // no values at all
  int ulo = nb, uhi = nb - 1;
  for (int b = 0; b < nb; b++)
    if (dec[size_t(b)] != 2 && dec[size_t(b)] != first) {
      ulo = b;
      break;
    }
  for (int b = nb - 1; b >= 0; b--)
    if (dec[size_t(b)] != 2 && dec[size_t(b)] != last) {
      uhi = b;
      break;
    }
  q.ulo = ulo;
  q.uhi = ulo == nb ? nb - 1 : uhi;
  q.below = first;
  q.above = ulo == nb ? first : last;
  return q;
}

// k_bu_fin's tests of a raw slot word w as unsigned range checks: a candidate (a bitmap probe is
// sent) iff (w - clo) <= cr, passing iff ((w - plo) <= pr) != pinv.  A candidate's probe byte
// offset is (w >> 3) & bmask.
struct FinArgs {
  uint32_t clo = 0, cr = 0xffffffffu, plo = 0, pr = 0xffffffffu;
  uint32_t pinv = 0, bmask = 0xfffffffcu;
};
// k_bu_fin holds the fields in scalar registers and calls the scalar forms of the candidate tests.
// Its pass test (`const bool pass = CLS == 1 ? w >= plo : (w - plo <= pr) != pinv;`, twice in the
// tile loop) stays written out: through fin_pass / fin_pass_cls1 the compiler swapped operands of
// the mask ANDs / ORs around it; the two functions restate that line.
NBG_HD bool fin_candidate(uint32_t w, uint32_t clo, uint32_t cr) { return w - clo <= cr; }
NBG_HD bool fin_pass(uint32_t w, uint32_t plo, uint32_t pr, bool pinv) { return (w - plo <= pr) != pinv; }
NBG_HD bool fin_candidate(uint32_t w, const FinArgs& f) { return fin_candidate(w, f.clo, f.cr); }
NBG_HD bool fin_pass(uint32_t w, const FinArgs& f) { return fin_pass(w, f.plo, f.pr, f.pinv != 0); }
// CLS 1: the candidates are every word from clo up and the passing ones every word from plo up
// (pinv 0): the "greater than" compares.  The candidate test is then the sign of w - clo, which
// k_bu_fin ORs into the probe offset as a mask: all ones (past the bitmap) for a non-candidate.
NBG_HD uint32_t fin_skip_cls1(uint32_t w, uint32_t clo) { return uint32_t(int32_t(w - clo) >> 31); }
NBG_HD bool fin_candidate_cls1(uint32_t w, uint32_t clo) { return fin_skip_cls1(w, clo) == 0u; }  // int32_t(w - clo) >= 0
NBG_HD bool fin_pass_cls1(uint32_t w, uint32_t plo) { return w >= plo; }
NBG_HD bool fin_candidate_cls1(uint32_t w, const FinArgs& f) { return fin_candidate_cls1(w, f.clo); }
NBG_HD bool fin_pass_cls1(uint32_t w, const FinArgs& f) { return fin_pass_cls1(w, f.plo); }
// May k_bu_fin<CLS = 1> run these ranges?  Both sets are upper ranges [lo, 2^32), and lo <= 2^31
// makes the sign of w - clo the range test for every word below 2^31 (bit 31 is clear in every
// real slot word: gbits + bits <= 31).  The -1 pad word is the one word they differ on: the range
// test takes it (it then probes gidx 2^gbits - 1, a bit no vertex owns), the sign test does not
// while clo < 2^31 (no probe at all); both leave the pad row unfound, and the pass tests agree.
NBG_HD bool fin_cls1_ok(const FinArgs& f) {
  return f.pinv == 0 && f.cr == ~f.clo && f.pr == ~f.plo && f.clo <= 0x80000000u && f.plo <= 0x80000000u;
}

// k_bu_fin's word ranges from a query's bucket decisions (q_test: buckets below ulo answer
// `below`, above uhi `above`, the rest are undecided).  The field above the gidx bits is the
// bucket; every decision region is a contiguous field range, so each set is one word range.
inline FinArgs fin_args(const QArgs& q) {
  FinArgs f;
  const int gb = q.gbits;
  f.bmask = (q.gmask >> 3) & ~3u;
  if (gb <= 0) {  // unpacked words: no buckets (every word undecided, or no predicate at all)
    f.clo = 0, f.cr = 0xffffffffu;
    const bool all_pass = q.below == 1 && q.above == 1;
    f.plo = 0, f.pr = 0xffffffffu, f.pinv = all_pass ? 0u : 1u;
    return f;
  }
  const int64_t B = (int64_t(1) << (32 - gb)) - 1;  // largest field value (the -1 pad's)
  const int64_t lo_end = std::min<int64_t>(std::max<int64_t>(q.ulo, 0), B + 1);  // [0, lo_end): below
  const int64_t u_end = std::min<int64_t>(std::max<int64_t>(q.uhi, lo_end - 1), B);  // [lo_end, u_end]: undecided
  auto word_lo = [&](int64_t a) { return uint32_t(uint64_t(a) << gb); };
  auto word_hi = [&](int64_t b) { return uint32_t(((uint64_t(b) + 1) << gb) - 1); };
  auto set_range = [&](int64_t a, int64_t b, uint32_t& lo, uint32_t& r) {  // field range [a, b], a <= b
    lo = word_lo(a);
    r = word_hi(b) - lo;
  };
  const bool c0 = q.below != 0, c2 = q.above != 0;  // below / above regions are candidates
  if (c0 && c2) set_range(0, B, f.clo, f.cr);
  else if (c0) set_range(0, u_end, f.clo, f.cr);
  else if (c2) set_range(lo_end, B, f.clo, f.cr);
  else if (lo_end <= u_end) set_range(lo_end, u_end, f.clo, f.cr);
  else f.clo = 0xffffffffu, f.cr = 0;  // no candidate but the pad word
  const bool p0 = q.below == 1 && lo_end > 0, p2 = q.above == 1 && u_end < B;
  f.pinv = 0;
  if (p0 && p2) {
    if (lo_end <= u_end) set_range(lo_end, u_end, f.plo, f.pr), f.pinv = 1;  // all but the undecided
    else f.plo = 0, f.pr = 0xffffffffu;
  } else if (p0) {
    set_range(0, lo_end - 1, f.plo, f.pr);
  } else if (p2) {
    set_range(u_end + 1, B, f.plo, f.pr);
  } else {
    f.plo = 0, f.pr = 0xffffffffu, f.pinv = 1;  // nothing passes
  }
  return f;
}

}  // namespace nbg
