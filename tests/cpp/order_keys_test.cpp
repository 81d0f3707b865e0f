// order_keys_test.cpp -- host check of nebula_amd/csrc/order_keys.h (tests/test_order_keys.py
// builds and runs it): the uint64 keys nbg_order_by sorts by must order and tie exactly as the
// values do under ColumnValue::operator< (src/graph/OrderByExecutor.cpp:14-68), with the
// engine's own rules for -0.0 and NaN (DESIGN.md divergence 8).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "order_keys.h"

using namespace nbg::okey;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      failures++;                        \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);      \
      fprintf(stderr, "\n");             \
    }                                    \
  } while (0)

// -1 / 0 / 1 of the values under the ORDER BY rules
static int cmp_int(int64_t a, int64_t b) { return a < b ? -1 : a > b ? 1 : 0; }
static int cmp_double(double a, double b) {
  const bool na = std::isnan(a), nb = std::isnan(b);
  if (na || nb) return na && nb ? 0 : na ? 1 : -1;  // NaNs tie, after +inf
  return a < b ? -1 : a > b ? 1 : 0;                // -0.0 == +0.0
}
static int cmp_key(uint64_t a, uint64_t b) { return a < b ? -1 : a > b ? 1 : 0; }

static double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// the key sequence of a string factor, most significant first: the chunks, then the length
static std::vector<uint64_t> str_keys(const std::string& s, int64_t max_len, int desc) {
  std::vector<uint64_t> k;
  for (int64_t c = 0; c < str_chunks(max_len); c++)
    k.push_back(direction(enc_str_chunk(reinterpret_cast<const uint8_t*>(s.data()), int64_t(s.size()), c), desc));
  k.push_back(direction(enc_str_len(int64_t(s.size())), desc));
  return k;
}
static int cmp_seq(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
  for (size_t i = 0; i < a.size(); i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}

int main() {
  const int64_t ints[] = {std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::min() + 1, -(int64_t(1) << 32),
                          -256, -1, 0, 1, 255, 256, (int64_t(1) << 26) - 1, int64_t(1) << 32,
                          std::numeric_limits<int64_t>::max() - 1, std::numeric_limits<int64_t>::max()};
  for (int desc = 0; desc < 2; desc++)
    for (int64_t a : ints)
      for (int64_t b : ints) {
        const int want = desc ? -cmp_int(a, b) : cmp_int(a, b);
        CHECK(cmp_key(direction(enc_int(a), desc), direction(enc_int(b), desc)) == want, "int %lld %lld desc %d",
              (long long)a, (long long)b, desc);
        CHECK(dec_int(enc_int(a)) == a, "int round trip %lld", (long long)a);
      }

  const double inf = std::numeric_limits<double>::infinity();
  const double doubles[] = {-inf, -std::numeric_limits<double>::max(), -1.5, -std::numeric_limits<double>::min(),
                            -std::numeric_limits<double>::denorm_min(), -0.0, 0.0,
                            std::numeric_limits<double>::denorm_min(), 2 * std::numeric_limits<double>::denorm_min(),
                            std::numeric_limits<double>::min(), 1.0, 1.5, std::numeric_limits<double>::max(), inf,
                            from_bits(0x7ff8000000000000ull),   // quiet NaN
                            from_bits(0xfff8000000000001ull),   // negative NaN with a payload
                            from_bits(0x7ff0000000000123ull)};  // signalling NaN with a payload
  for (int desc = 0; desc < 2; desc++)
    for (double a : doubles)
      for (double b : doubles) {
        const int want = desc ? -cmp_double(a, b) : cmp_double(a, b);
        CHECK(cmp_key(direction(enc_double(a), desc), direction(enc_double(b), desc)) == want, "double %a %a desc %d", a,
              b, desc);
      }
  CHECK(enc_double(-0.0) == enc_double(0.0), "-0.0 ties with +0.0");
  CHECK(enc_double(from_bits(0xfff8000000000001ull)) > enc_double(inf), "NaN after +inf");

  for (int desc = 0; desc < 2; desc++)
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2; b++) {
        const int want = desc ? -cmp_int(a, b) : cmp_int(a, b);
        CHECK(cmp_key(direction(enc_bool(uint8_t(a)), desc), direction(enc_bool(uint8_t(b)), desc)) == want,
              "bool %d %d desc %d", a, b, desc);
      }
  CHECK(enc_bool(7) == enc_bool(1), "any non-zero byte is true");

  // strings: std::string order (unsigned bytes, a proper prefix first, embedded NULs legal)
  std::vector<std::string> strs = {
      "", "a", std::string("a\0", 2), std::string("a\0\0", 3), "ab", "b", std::string("\0", 1),
      "abcdefgh",                          // 8 bytes
      "abcdefgi",                          // 8, differs in the last byte of the chunk
      "abcdefgh0",                         // 9, shares the 8-byte prefix
      "abcdefgh1",                         // 9
      std::string("abcdefgh\0", 9),        // 9, a NUL right behind the chunk
      "abcdefghijklmnop",                  // 16
      "abcdefghijklmnoq",                  // 16
      "abcdefghijklmnopq",                 // 17, shares the 16-byte prefix
      "abcdefghijklmnopr",                 // 17
      std::string("abcdefghijklmnop\0", 17),
      "\x80", "\xff", "a\x80", "a\x7f", "\xff\xff\xff\xff\xff\xff\xff\xff", "\xff\xff\xff\xff\xff\xff\xff\xff\x01",
      "Z", "z",
  };
  int64_t max_len = 0;
  for (auto& s : strs) max_len = std::max<int64_t>(max_len, int64_t(s.size()));
  CHECK(str_chunks(0) == 0 && str_chunks(1) == 1 && str_chunks(8) == 1 && str_chunks(9) == 2 && str_chunks(256) == 32,
        "chunk counts");
  for (int desc = 0; desc < 2; desc++)
    for (auto& a : strs)
      for (auto& b : strs) {
        const int c = a.compare(b);
        const int want0 = c < 0 ? -1 : c > 0 ? 1 : 0;
        const int want = desc ? -want0 : want0;
        // padded to the set's longest value, and to a longer bound: extra zero chunks decide nothing
        for (int64_t ml : {max_len, max_len + 8, int64_t(256)})
          CHECK(cmp_seq(str_keys(a, ml, desc), str_keys(b, ml, desc)) == want, "string #%zu vs #%zu desc %d max %lld",
                size_t(&a - &strs[0]), size_t(&b - &strs[0]), desc, (long long)ml);
      }

  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("order_keys ok\n");
  return 0;
}
