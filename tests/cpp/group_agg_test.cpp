// group_agg_test.cpp -- TEST PROGRAM: the arithmetic of GROUP BY's aggregates on the host.
//
// Compiled against nebula_amd/csrc/group_agg.h with the host compiler (its own main, no HIP, no
// GPU; tests/test_group_agg.py builds it with AddressSanitizer + UBSan where it can).  Checks:
//   the MIN / MAX key round trip (enc_int / dec_int at the int64 extremes, enc_double / dec_double
//   at both zeros, both infinities, NaN payloads and denormals, enc_bool / dec_bool);
//   the identities of the four operators;
//   the wrapped integer sum at INT64_MAX + 1 and the AVG divisions;
//   the segment tree on lengths 0, 1, 2, 16, 17, 63, 64, 65, 1025, 4096, 4097, 5000, 16384, 16385
//   and 50000 against a scalar restatement written here from the header's comment, not from its
//   code.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "group_agg.h"

using namespace nbg;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      failures++;                                                \
    }                                                            \
  } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
static double from_bits(uint64_t b) {
  double v;
  memcpy(&v, &b, 8);
  return v;
}

static void test_round_trip() {
  const int64_t ints[] = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX};
  for (int64_t v : ints) CHECK(okey::dec_int(okey::enc_int(v)) == v);
  for (size_t i = 0; i + 1 < sizeof(ints) / sizeof(ints[0]); i++) CHECK(okey::enc_int(ints[i]) < okey::enc_int(ints[i + 1]));
  CHECK(agg::dec_bool(okey::enc_bool(0)) == 0 && agg::dec_bool(okey::enc_bool(1)) == 1 && agg::dec_bool(okey::enc_bool(7)) == 1);

  const double inf = std::numeric_limits<double>::infinity();
  const double keep[] = {-inf, -1.7976931348623157e308, -1.5, -2.2250738585072014e-308, -4.9406564584124654e-324,
                         4.9406564584124654e-324, 2.2250738585072014e-308, 1.0, 1.7976931348623157e308, inf};
  for (double v : keep) CHECK(bits(agg::dec_double(okey::enc_double(v))) == bits(v));  // its own bits
  for (size_t i = 0; i + 1 < sizeof(keep) / sizeof(keep[0]); i++) CHECK(okey::enc_double(keep[i]) < okey::enc_double(keep[i + 1]));
  // both zeros are one class, and it decodes to +0.0
  CHECK(okey::enc_double(-0.0) == okey::enc_double(0.0));
  CHECK(bits(agg::dec_double(okey::enc_double(-0.0))) == 0);
  CHECK(bits(agg::dec_double(okey::enc_double(0.0))) == 0);
  CHECK(okey::enc_double(-4.9406564584124654e-324) < okey::enc_double(0.0));
  CHECK(okey::enc_double(0.0) < okey::enc_double(4.9406564584124654e-324));
  // every NaN is one class after +inf, and it decodes to the quiet NaN
  const uint64_t nans[] = {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0x7ff8000000000abcull,
                           0xffffffffffffffffull};
  for (uint64_t nb : nans) {
    CHECK(okey::enc_double(from_bits(nb)) == okey::enc_double(from_bits(nans[0])));
    CHECK(okey::enc_double(from_bits(nb)) > okey::enc_double(inf));
    CHECK(bits(agg::dec_double(okey::enc_double(from_bits(nb)))) == okey::kQuietNan);
  }
}

static void test_identities() {
  const uint64_t words[] = {0, 1, 0x8000000000000000ull, 0x7fffffffffffffffull, ~uint64_t(0), bits(1.5), bits(-0.0), bits(0.0)};
  for (int32_t op : {agg::OP_ADD_I64, agg::OP_MIN_U64, agg::OP_MAX_U64}) {
    for (uint64_t w : words) {
      CHECK(agg::combine(op, agg::identity(op), w) == w);
      CHECK(agg::combine(op, w, agg::identity(op)) == w);
    }
  }
  // the double sum's identity is -0.0: it keeps even a -0.0 (the +0.0 would not)
  const double ds[] = {-0.0, 0.0, 1.5, -1.5, 4.9406564584124654e-324, std::numeric_limits<double>::infinity(),
                       -std::numeric_limits<double>::infinity()};
  for (double d : ds) {
    CHECK(agg::combine(agg::OP_ADD_F64, agg::identity(agg::OP_ADD_F64), bits(d)) == bits(d));
    CHECK(agg::combine(agg::OP_ADD_F64, bits(d), agg::identity(agg::OP_ADD_F64)) == bits(d));
  }
  CHECK(agg::combine(agg::OP_ADD_F64, bits(0.0), bits(-0.0)) == bits(0.0));
  CHECK(std::isnan(from_bits(agg::combine(agg::OP_ADD_F64, agg::identity(agg::OP_ADD_F64), okey::kQuietNan))));
  CHECK(agg::identity(agg::OP_MIN_U64) == ~uint64_t(0) && agg::identity(agg::OP_MAX_U64) == 0);
}

static void test_sums_and_avg() {
  CHECK(agg::wrap_add(INT64_MAX, 1) == INT64_MIN);
  CHECK(agg::wrap_add(INT64_MIN, -1) == INT64_MAX);
  CHECK(agg::wrap_add(INT64_MIN, INT64_MIN) == 0);
  CHECK(agg::wrap_add(-5, 7) == 2);
  CHECK(int64_t(agg::combine(agg::OP_ADD_I64, uint64_t(INT64_MAX), 1)) == INT64_MIN);
  // AVG of the wrapped sum: INT64_MAX + 1 over two rows is INT64_MIN / 2
  CHECK(agg::avg_int(agg::wrap_add(INT64_MAX, 1), 2) == -4611686018427387904.0);
  CHECK(agg::avg_int(7, 2) == 3.5);
  CHECK(agg::avg_int(-7, 2) == -3.5);
  CHECK(agg::avg_double(1.0, 3) == 1.0 / 3.0);
  CHECK(std::isnan(agg::avg_double(from_bits(okey::kQuietNan), 3)));
}

// ---- the scalar restatement of the tree (from the header's comment) -----------------------------
static double lane_sum(const std::vector<double>& x, size_t first, size_t step) {
  double s = -0.0;
  for (size_t j = first; j < x.size(); j += step) s = s + x[j];
  return s;
}
static double halve(std::vector<double> p) {  // 64 partial sums
  for (size_t o = 32; o >= 1; o /= 2)
    for (size_t l = 0; l < o; l++) p[l] = p[l] + p[l + o];
  return p[0];
}
static double block_sum(const std::vector<double>& x) {  // the 256-thread tree
  double w[4];
  for (size_t wv = 0; wv < 4; wv++) {
    std::vector<double> p(64);
    for (size_t l = 0; l < 64; l++) p[l] = lane_sum(x, wv * 64 + l, 256);
    w[wv] = halve(p);
  }
  return (w[0] + w[1]) + (w[2] + w[3]);
}
static double tree_sum(const std::vector<double>& x) {
  if (x.size() <= 16) return lane_sum(x, 0, 1);
  if (x.size() <= 4096) {
    std::vector<double> p(64);
    for (size_t l = 0; l < 64; l++) p[l] = lane_sum(x, l, 64);
    return halve(p);
  }
  std::vector<double> chunks;  // chunks of 16384 values, a block each; their sums, a block again
  for (size_t at = 0; at < x.size(); at += 16384)
    chunks.push_back(block_sum(std::vector<double>(x.begin() + at, x.begin() + std::min(x.size(), at + 16384))));
  return block_sum(chunks);
}

static void test_segment_tree() {
  CHECK(agg::seg_class(0) == 0 && agg::seg_class(16) == 0 && agg::seg_class(17) == 1 && agg::seg_class(4096) == 1 &&
        agg::seg_class(4097) == 2);
  uint64_t state = 0x9e3779b97f4a7c15ull;
  for (size_t len : {size_t(0), size_t(1), size_t(2), size_t(16), size_t(17), size_t(63), size_t(64), size_t(65),
                     size_t(1025), size_t(4096), size_t(4097), size_t(5000), size_t(16384), size_t(16385),
                     size_t(50000)}) {
    // values of very different magnitudes: another association order changes the low bits
    std::vector<double> x(len);
    for (double& v : x) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      const int e = int((state >> 20) % 40) - 20;
      v = std::ldexp(double(int64_t(state >> 11) % 1000003) / 1000003.0, e);
    }
    std::vector<uint64_t> w(len);
    for (size_t j = 0; j < len; j++) w[j] = bits(x[j]);
    const uint64_t* wp = w.data();
    const uint64_t got = agg::seg_reduce(agg::OP_ADD_F64, [wp](int64_t j) { return wp[j]; }, int64_t(len));
    CHECK(got == bits(tree_sum(x)));
    if (len == 0) CHECK(got == bits(-0.0));
    // the exact operators give what a plain loop gives, whatever the tree
    uint64_t sum = 0, mn = ~uint64_t(0), mx = 0;
    for (uint64_t v : w) sum += v, mn = v < mn ? v : mn, mx = v > mx ? v : mx;
    CHECK(agg::seg_reduce(agg::OP_ADD_I64, [wp](int64_t j) { return wp[j]; }, int64_t(len)) == sum);
    CHECK(agg::seg_reduce(agg::OP_MIN_U64, [wp](int64_t j) { return wp[j]; }, int64_t(len)) == mn);
    CHECK(agg::seg_reduce(agg::OP_MAX_U64, [wp](int64_t j) { return wp[j]; }, int64_t(len)) == mx);
  }
  // a segment of -0.0s sums to -0.0 in every class
  for (size_t len : {size_t(3), size_t(100), size_t(5000)}) {
    std::vector<uint64_t> w(len, bits(-0.0));
    const uint64_t* wp = w.data();
    CHECK(agg::seg_reduce(agg::OP_ADD_F64, [wp](int64_t j) { return wp[j]; }, int64_t(len)) == bits(-0.0));
  }
}

int main() {
  test_round_trip();
  test_identities();
  test_sums_and_avg();
  test_segment_tree();
  if (failures) {
    printf("group_agg: %d check(s) failed\n", failures);
    return 1;
  }
  printf("group_agg ok\n");
  return 0;
}
