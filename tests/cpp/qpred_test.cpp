// qpred_test.cpp -- host check of nebula_amd/csrc/qpred.h (tests/test_qpred.py builds and runs
// it): the quantised predicate of the packed bottom-up words must never answer a compare wrongly.
// Over a grid of (bucket bits, gidx bits, column minimum, column range, op, constant) it checks
// q_bucket against the bucket edges make_qargs_core uses, q_test against the exact compare,
// that at most the bucket holding the constant is undecided, fin_args' word ranges against
// q_test, and k_bu_fin's CLS-1 forms against the generic ones wherever fin_cls1_ok allows them.
// Reference arithmetic is signed 128-bit, independent of the header's unsigned wrap-around.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "qpred.h"

using namespace nbg;
typedef __int128 i128;
typedef unsigned __int128 u128;

static long failures = 0;
static unsigned long long checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    checks++;                                              \
    if (!(cond)) {                                         \
      if (failures++ < 40) {                               \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, "\n");                             \
      }                                                    \
    }                                                      \
  } while (0)

static const i128 kI64Min = i128(INT64_MIN), kI64Max = i128(INT64_MAX);
static bool fits(i128 v) { return v >= kI64Min && v <= kI64Max; }
static long long ll(i128 v) { return (long long)v; }

// the compare on Python-like integers
static bool P(int op, i128 v, i128 k) {
  switch (op) {
    case 0: return v < k;
    case 1: return v <= k;
    case 2: return v > k;
    case 3: return v >= k;
    case 4: return v == k;
    default: return v != k;
  }
}

struct Col {
  int64_t vmin;
  uint64_t range;  // 0 = 2^64
  int bits;
  i128 R, vmax;
  std::vector<i128> lo, hi;     // per bucket; lo > hi: empty
  std::vector<int64_t> V;       // the value sample, ascending
  std::vector<uint32_t> VB;     // q_bucket of V
};

static uint32_t bucket(const Col& c, int64_t v) { return q_bucket(v, c.vmin, c.range, c.bits); }

static void add_clipped(std::vector<int64_t>& out, const Col& c, i128 v) {
  if (v >= i128(c.vmin) && v <= c.vmax) out.push_back(int64_t(v));
}

// property 1 and the value sample
static void build_col(Col& c) {
  const int nb = 1 << c.bits;
  c.R = c.range ? i128(c.range) : (i128(1) << 64);
  c.vmax = i128(c.vmin) + c.R - 1;
  c.lo.assign(size_t(nb), 0);
  c.hi.assign(size_t(nb), -1);
  CHECK(q_edge(0, c.range, c.bits) == 0, "edge(0) != 0");
  CHECK(i128(q_edge(uint64_t(nb), c.range, c.bits)) == c.R, "edge(2^bits) != range");
  for (int b = 0; b < nb; b++) {
    const i128 o0 = i128(q_edge(uint64_t(b), c.range, c.bits)), o1 = i128(q_edge(uint64_t(b) + 1, c.range, c.bits));
    CHECK(o0 <= o1, "edges decrease at bucket %d", b);
    // the ceil: the smallest offset o with o * 2^bits >= b * range
    CHECK((o0 << c.bits) >= i128(b) * c.R && (o0 == 0 || ((o0 - 1) << c.bits) < i128(b) * c.R),
          "edge(%d) is not ceil(b * range / 2^bits): min %lld range %llu bits %d", b, (long long)c.vmin,
          (unsigned long long)c.range, c.bits);
    c.lo[size_t(b)] = i128(c.vmin) + o0;
    c.hi[size_t(b)] = i128(c.vmin) + o1 - 1;
  }
  std::vector<int64_t>& V = c.V;
  if (c.R <= 4096) {
    for (i128 v = c.vmin; v <= c.vmax; v++) V.push_back(int64_t(v));
  } else {
    add_clipped(V, c, c.vmin);
    add_clipped(V, c, c.vmax);
    for (int b = 0; b < nb; b++) {
      if (c.lo[size_t(b)] > c.hi[size_t(b)]) continue;
      add_clipped(V, c, c.lo[size_t(b)]);
      add_clipped(V, c, c.hi[size_t(b)]);
      add_clipped(V, c, c.lo[size_t(b)] - 1);
    }
  }
  std::sort(V.begin(), V.end());
  V.erase(std::unique(V.begin(), V.end()), V.end());
  uint32_t prev = 0;
  for (int64_t v : V) {
    const uint32_t b = bucket(c, v);
    CHECK(b < uint32_t(nb), "bucket %u out of range: v %lld min %lld range %llu bits %d", b, (long long)v,
          (long long)c.vmin, (unsigned long long)c.range, c.bits);
    CHECK(b >= prev, "bucket decreases at v %lld: min %lld range %llu bits %d", (long long)v, (long long)c.vmin,
          (unsigned long long)c.range, c.bits);
    // the value lies between the edges of its bucket
    if (b < uint32_t(nb))
      CHECK(i128(v) >= c.lo[b] && i128(v) <= c.hi[b], "v %lld outside the edges of its bucket %u: min %lld range %llu bits %d",
            (long long)v, b, (long long)c.vmin, (unsigned long long)c.range, c.bits);
    prev = b;
    c.VB.push_back(b);
  }
  CHECK(bucket(c, c.vmin) == 0, "bucket(min) != 0");
  for (int b = 0; b < nb; b++) {
    if (c.lo[size_t(b)] > c.hi[size_t(b)]) continue;
    CHECK(bucket(c, int64_t(c.lo[size_t(b)])) == uint32_t(b) && bucket(c, int64_t(c.hi[size_t(b)])) == uint32_t(b),
          "bucket %d: its edges [%lld, %lld] land in %u / %u: min %lld range %llu bits %d", b, ll(c.lo[size_t(b)]),
          ll(c.hi[size_t(b)]), bucket(c, int64_t(c.lo[size_t(b)])), bucket(c, int64_t(c.hi[size_t(b)])),
          (long long)c.vmin, (unsigned long long)c.range, c.bits);
    if (c.lo[size_t(b)] > i128(c.vmin))
      CHECK(bucket(c, int64_t(c.lo[size_t(b)] - 1)) < uint32_t(b), "bucket %d: the value below its first is not below", b);
  }
}

static std::vector<int64_t> constants(const Col& c) {
  const int nb = 1 << c.bits;
  std::vector<i128> ks = {kI64Min, kI64Max, i128(c.vmin) - 1, c.vmin, i128(c.vmin) + 1, c.vmax - 1, c.vmax, c.vmax + 1};
  const i128 mid = i128(c.vmin) + c.R / 2;
  ks.push_back(mid), ks.push_back(mid - 1), ks.push_back(mid + 1);
  // the first, the last and two middle non-empty buckets
  std::vector<int> ne;
  for (int b = 0; b < nb; b++)
    if (c.lo[size_t(b)] <= c.hi[size_t(b)]) ne.push_back(b);
  const size_t n = ne.size();
  for (size_t i : {size_t(0), n / 2 ? n / 2 - 1 : 0, n / 2, n - 1}) {
    ks.push_back(c.lo[size_t(ne[std::min(i, n - 1)])]);
    ks.push_back(c.hi[size_t(ne[std::min(i, n - 1)])]);
  }
  std::vector<int64_t> out;
  for (i128 k : ks)
    if (fits(k)) out.push_back(int64_t(k));
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return out;
}

// properties 4 and 5 for one word
static void check_word(uint32_t w, int t, const FinArgs& fa, bool cls1, const char* what, long long a, long long b) {
  const bool cand = fin_candidate(w, fa), pass = fin_pass(w, fa);
  if (t == 1) CHECK(cand && pass, "%s: word %08x passes (q_test 1) but candidate %d pass %d (%lld, %lld)", what, w, cand, pass, a, b);
  if (t == -1) CHECK(cand && !pass, "%s: word %08x undecided but candidate %d pass %d (%lld, %lld)", what, w, cand, pass, a, b);
  if (t == 0) CHECK(!pass, "%s: word %08x fails (q_test 0) but passes the range test (%lld, %lld)", what, w, a, b);
  if (cls1) {
    CHECK(fin_candidate_cls1(w, fa) == cand, "%s: word %08x CLS-1 candidate %d, generic %d (clo %08x)", what, w,
          fin_candidate_cls1(w, fa), cand, fa.clo);
    CHECK((fin_skip_cls1(w, fa.clo) == 0xffffffffu) == !cand && (fin_skip_cls1(w, fa.clo) == 0u) == cand,
          "%s: word %08x CLS-1 skip mask %08x, candidate %d", what, w, fin_skip_cls1(w, fa.clo), cand);
    CHECK(fin_pass_cls1(w, fa) == pass, "%s: word %08x CLS-1 pass %d, generic %d (plo %08x)", what, w,
          fin_pass_cls1(w, fa), pass, fa.plo);
  }
}
// The -1 pad word (an empty slot).  4: it is no candidate, or its probe reads the bit of gidx gmask.
// 5: its pass tests agree.  Its candidate tests cannot: for an upper range [clo, 2^32) the range
// test always takes 0xffffffff, the sign test never does while clo < 2^31 (0xffffffff - clo keeps
// bit 31).  That is the safe side (k_bu_fin<1> sends the pad no probe at all); what must hold is
// that CLS 1 never makes a candidate of a pad word the range test refuses.
static unsigned long long n_pad_stricter = 0;
static void check_pad(const QArgs& q, const FinArgs& fa, bool cls1, const char* what) {
  const uint32_t w = 0xffffffffu;
  const bool cand = fin_candidate(w, fa);
  CHECK(!cand || ((w >> 3) & fa.bmask) == ((q.gmask >> 3) & fa.bmask), "%s: the pad word's probe offset", what);
  CHECK(fa.bmask == ((q.gmask >> 3) & ~3u), "%s: bmask %08x for gmask %08x", what, fa.bmask, q.gmask);
  if (cls1) {
    CHECK(!fin_candidate_cls1(w, fa) || cand, "%s: pad word a CLS-1 candidate but no generic one (clo %08x)", what, fa.clo);
    CHECK((fin_skip_cls1(w, fa.clo) == 0u) == fin_candidate_cls1(w, fa), "%s: pad word skip mask", what);
    n_pad_stricter += !fin_candidate_cls1(w, fa) && cand;
    CHECK(fin_pass_cls1(w, fa) == fin_pass(w, fa), "%s: pad word CLS-1 pass, generic %d (plo %08x)", what,
          fin_pass(w, fa), fa.plo);
  }
}

static unsigned long long n_q = 0, n_undecided = 0, n_cls1 = 0;

// properties 2 to 5 for one column, packing and compare
static void check_query(const Col& c, int gbits, int op, int64_t k) {
  const int nb = 1 << c.bits;
  const QArgs q = make_qargs_core(c.vmin, c.range, c.bits, gbits, op, k);
  const FinArgs fa = fin_args(q);
  const bool cls1 = fin_cls1_ok(fa);
  n_q++;
  n_cls1 += cls1;
  const uint32_t gmask = (1u << gbits) - 1u;
  CHECK(q.gmask == gmask && q.gbits == gbits, "gmask / gbits");
  // 3: only the bucket straddling k may be undecided
  int undecided = 0;
  for (int b = 0; b < nb; b++)
    if (c.lo[size_t(b)] <= c.hi[size_t(b)] && q_test(int32_t(uint32_t(b) << gbits), q) == -1) undecided++;
  n_undecided += uint64_t(undecided);
  CHECK(undecided <= 1, "%d undecided buckets: min %lld range %llu bits %d op %d k %lld", undecided, (long long)c.vmin,
        (unsigned long long)c.range, c.bits, op, (long long)k);
  if (i128(k) < i128(c.vmin) - 1 || i128(k) > c.vmax + 1)
    CHECK(undecided == 0, "k outside the range but %d undecided buckets: min %lld range %llu bits %d op %d k %lld", undecided,
          (long long)c.vmin, (unsigned long long)c.range, c.bits, op, (long long)k);
  auto value = [&](int64_t v, uint32_t b) {
    const bool want = P(op, v, k);
    CHECK(fast_cmp(op, v, k) == want, "fast_cmp(%d, %lld, %lld)", op, (long long)v, (long long)k);
    for (uint32_t g : {0u, gmask}) {
      const uint32_t w = (b << gbits) | g;
      const int t = q_test(int32_t(w), q);
      // 2: decided buckets answer the compare
      CHECK(t == -1 || t == int(want), "q_test %d, compare %d: v %lld min %lld range %llu bits %d gbits %d op %d k %lld", t,
            int(want), (long long)v, (long long)c.vmin, (unsigned long long)c.range, c.bits, gbits, op, (long long)k);
      check_word(w, t, fa, cls1, "query", (long long)v, (long long)k);
    }
  };
  for (size_t i = 0; i < c.V.size(); i++) value(c.V[i], c.VB[i]);
  if (c.R > 4096)
    for (i128 v : {i128(k) - 1, i128(k), i128(k) + 1})
      if (v >= i128(c.vmin) && v <= c.vmax) value(int64_t(v), bucket(c, int64_t(v)));
  check_pad(q, fa, cls1, "query");
}

// property 6: the final hop without a predicate, and unpacked words
static void check_no_predicate() {
  for (int gbits : {1, 9, 10, 13, 23, 28}) {
    QArgs q;
    q.gmask = (1u << gbits) - 1u;
    q.gbits = gbits;
    q.ulo = q.uhi = INT32_MAX, q.below = q.above = 1;
    const FinArgs fa = fin_args(q);
    const bool cls1 = fin_cls1_ok(fa);
    if (gbits > 1) CHECK(cls1, "no predicate: not CLS 1 at gbits %d", gbits);  // (gbits 1: INT32_MAX is the pad's field)
    const uint32_t top = (1u << (31 - gbits)) - 1u;  // the largest bucket field of a real word
    for (uint32_t b : {0u, 1u, top / 2, top}) {
      for (uint32_t g : {0u, q.gmask}) {
        const uint32_t w = (b << gbits) | g;
        CHECK(q_test(int32_t(w), q) == 1, "no predicate: q_test");
        check_word(w, 1, fa, cls1, "no predicate", b, g);
      }
    }
    check_pad(q, fa, cls1, "no predicate");
  }
  for (int all_pass = 0; all_pass < 2; all_pass++) {
    QArgs q;  // unpacked: gbits 0
    if (all_pass) q.ulo = q.uhi = INT32_MAX, q.below = q.above = 1;
    const FinArgs fa = fin_args(q);
    const bool cls1 = fin_cls1_ok(fa);
    for (uint32_t w : {0u, 1u, 7u, 8u, 510u, 511u, 512u, 123456789u, 0x7ffffffdu, 0x7ffffffeu}) {  // a gidx is below INT32_MAX
      const int t = q_test(int32_t(w), q);
      CHECK(t == (all_pass ? 1 : -1), "unpacked: q_test %d", t);
      check_word(w, t, fa, cls1, "unpacked", w, all_pass);
    }
    check_pad(q, fa, cls1, "unpacked");
  }
}

// property 5 on word ranges make_qargs_core does not produce: whatever ranges fin_cls1_ok accepts,
// the sign test must equal the range test on every real slot word (bit 31 clear); the pad word as
// in check_pad
static void check_cls1_ranges() {
  const uint32_t los[] = {0u, 1u, 0x200u, 0x12345600u, 0x7ffffe00u, 0x7fffffffu, 0x80000000u,
                          0x80000001u, 0x80000200u, 0xc0000000u, 0xfffffe00u, 0xffffffffu};
  std::vector<uint32_t> words = {0u, 1u, 0x1ffu, 0x200u, 0x201u, 0x123455ffu, 0x12345600u, 0x12345601u, 0x3fffffffu,
                                 0x40000000u, 0x7ffffdffu, 0x7ffffe00u, 0x7ffffffeu, 0x7fffffffu};
  unsigned accepted = 0;
  for (uint32_t clo : los)
    for (uint32_t plo : los)
      for (uint32_t pinv : {0u, 1u}) {
        FinArgs fa;
        fa.clo = clo, fa.cr = ~clo, fa.plo = plo, fa.pr = ~plo, fa.pinv = pinv;
        if (!fin_cls1_ok(fa)) continue;
        accepted++;
        for (uint32_t w : words) {
          CHECK(fin_candidate_cls1(w, fa) == fin_candidate(w, fa), "ranges: word %08x clo %08x: CLS-1 candidate %d, generic %d", w,
                clo, fin_candidate_cls1(w, fa), fin_candidate(w, fa));
          CHECK(fin_pass_cls1(w, fa) == fin_pass(w, fa), "ranges: word %08x plo %08x: CLS-1 pass %d, generic %d", w, plo,
                fin_pass_cls1(w, fa), fin_pass(w, fa));
        }
        QArgs q;  // (only gmask is read)
        fa.bmask = (q.gmask >> 3) & ~3u;
        check_pad(q, fa, true, "ranges");
      }
  CHECK(accepted >= 49, "fin_cls1_ok accepted only %u of the upper ranges", accepted);  // 7 x 7 with lo <= 2^31
}

int main() {
  const int gbits_all[] = {1, 9, 13, 23, 28};
  const i128 two31 = i128(1) << 31;
  const i128 mins[] = {0, 1, -1, -128, -129, -32768, -two31, -two31 - 1, kI64Min, kI64Max - 5, i128(1) << 40};
  const uint64_t ranges[] = {1, 2, 3, 255, 256, 257, 1000, (1ull << 16) + 1, 1ull << 32, 1ull << 63, ~0ull, 0};
  unsigned cols = 0;
  for (int bits = 3; bits <= 8; bits++)
    for (i128 vmin : mins)
      for (uint64_t range : ranges) {
        const i128 R = range ? i128(range) : (i128(1) << 64);
        if (!fits(vmin + R - 1)) continue;
        if (range == 0 && vmin != kI64Min) continue;
        Col c;
        c.vmin = int64_t(vmin), c.range = range, c.bits = bits;
        build_col(c);
        cols++;
        const std::vector<int64_t> ks = constants(c);
        for (int gbits : gbits_all) {
          if (gbits + bits > 31) continue;
          for (int op = 0; op < 6; op++)
            for (int64_t k : ks) check_query(c, gbits, op, k);
        }
      }
  check_no_predicate();
  check_cls1_ranges();
  // the grid is not vacuous: some queries leave a bucket undecided, and some run as CLS 1
  CHECK(n_undecided > 0 && n_undecided < n_q, "undecided buckets in %llu of %llu queries", n_undecided, n_q);
  CHECK(n_cls1 > 0 && n_cls1 < n_q, "CLS 1 in %llu of %llu queries", n_cls1, n_q);
  if (failures) {
    fprintf(stderr, "%ld checks failed\n", failures);
    return 1;
  }
  printf("qpred ok: %u columns, %llu queries (%llu with an undecided bucket, %llu CLS 1), %llu checks\n", cols, n_q,
         n_undecided, n_cls1, checks);
  printf("pad word: a generic candidate but no CLS-1 candidate in %llu CLS-1 cases\n", n_pad_stricter);
  return 0;
}
