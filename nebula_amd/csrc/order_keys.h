// order_keys.h -- order-preserving uint64 keys of ORDER BY factors (host and device).
//
// nbg_order_by sorts rows with an LSD radix sort over unsigned 64-bit keys, so every factor is
// first turned into keys whose unsigned order is the factor's order (ColumnValue::operator<,
// src/graph/OrderByExecutor.cpp:14-68):
//   INT / VID / TIMESTAMP   signed int64         -> the sign bit flipped
//   BOOL                    false < true         -> 0 / 1
//   DOUBLE                  numeric              -> the usual total-order transform, after -0.0
//                                                   became +0.0 (they tie: the reference tests ==
//                                                   first) and every NaN the one quiet NaN (all
//                                                   NaNs tie and sort after +inf; DESIGN.md
//                                                   divergence 8)
//   STRING                  std::string order    -> a SEQUENCE of keys, most significant first:
//                                                   the 8-byte big-endian chunks of the value,
//                                                   zero-padded, then the length.  Two values that
//                                                   differ only in trailing NUL bytes have equal
//                                                   chunks, and the shorter (a proper prefix)
//                                                   sorts first by its length.
// DESC is the bitwise complement of the ASC key: the exact reverse order, and equal keys stay
// equal, so a stable sort keeps ties in input order under either direction.
// Plain functions only: tests/cpp/order_keys_test.cpp compiles this header with the host compiler.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NBG_HD __host__ __device__ inline
#else
#define NBG_HD inline
#endif

namespace nbg {
namespace okey {

constexpr uint64_t kSign = uint64_t(1) << 63;
constexpr uint64_t kQuietNan = 0x7ff8000000000000ull;

NBG_HD uint64_t enc_int(int64_t v) { return uint64_t(v) ^ kSign; }
NBG_HD int64_t dec_int(uint64_t k) { return int64_t(k ^ kSign); }

NBG_HD uint64_t enc_bool(uint8_t b) { return b ? 1u : 0u; }

NBG_HD uint64_t enc_double(double v) {
  uint64_t b;
  if (v != v) {
    b = kQuietNan;
  } else if (v == 0.0) {
    b = 0;
  } else {
    memcpy(&b, &v, 8);
  }
  return (b & kSign) ? ~b : (b | kSign);
}

// keys of one string factor: str_keys(len) of them, index 0 the most significant
NBG_HD int64_t str_chunks(int64_t max_len) { return (max_len + 7) / 8; }
NBG_HD uint64_t enc_str_len(int64_t len) { return uint64_t(len); }
// bytes [8 * chunk, 8 * chunk + 8) of the value as one big-endian word, zero past its end
NBG_HD uint64_t enc_str_chunk(const uint8_t* p, int64_t len, int64_t chunk) {
  uint64_t k = 0;
  const int64_t at = chunk * 8;
  for (int64_t j = 0; j < 8; j++) {
    const int64_t i = at + j;
    k = (k << 8) | uint64_t(i < len ? p[i] : 0);
  }
  return k;
}

NBG_HD uint64_t direction(uint64_t key, int32_t desc) { return desc ? ~key : key; }

}  // namespace okey
}  // namespace nbg
