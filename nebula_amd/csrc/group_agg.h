// group_agg.h -- the arithmetic of GROUP BY's aggregates (host and device).
//
// nbg_group_by keeps every accumulator as one uint64 word and combines two words with one of four
// operators:
//   OP_ADD_I64   COUNT and the integer SUM: a 64-bit add, two's-complement wrap-around
//   OP_MIN_U64   MIN: the unsigned minimum of order_keys.h keys (enc_int, enc_bool, enc_double)
//   OP_MAX_U64   MAX: the unsigned maximum of the same keys
//   OP_ADD_F64   the DOUBLE SUM: an IEEE add of the two words' doubles
// The first three are associative, commutative and exact, so the atomic path (any arrival order)
// and the ordered path (a fixed tree) give the same word.  OP_ADD_F64 is neither, so it only ever
// runs through the fixed tree below, whose shape depends on the segment's length alone:
//   len <= kSegLane   one lane adds the values from the first to the last
//   len <= kSegWave   64 lanes: lane l adds values l, l + 64, l + 128, ... in that order, then
//                     the 64 partial sums are halved 32, 16, ... 1 (p[l] += p[l + o])
//   longer            the segment is cut into chunks of kSegChunk values (the last one shorter);
//                     a workgroup reduces a chunk: thread t of 256 adds values t, t + 256, ...,
//                     each wave of 64 halves its partial sums as above, and the four wave sums
//                     join as (w0 + w1) + (w2 + w3).  The chunks' words, in order, are reduced by
//                     that same 256-thread tree
// A lane without a value holds the operator's identity.  For OP_ADD_F64 that is -0.0, the one
// double x with x + v == v bit for bit for every v (+0.0 would turn a sum of -0.0s into +0.0).
// Plain functions only: tests/cpp/group_agg_test.cpp compiles this header with the host compiler.
#pragma once
#include <cstdint>
#include <cstring>

#include "order_keys.h"

namespace nbg {
namespace agg {

enum Op : int32_t { OP_ADD_I64 = 0, OP_MIN_U64 = 1, OP_MAX_U64 = 2, OP_ADD_F64 = 3 };

constexpr int64_t kSegLane = 16;
constexpr int64_t kSegWave = 4096;
constexpr int64_t kSegChunk = 16384;
constexpr int kWaveLanes = 64;
constexpr int kBlockLanes = 256;

NBG_HD uint64_t dbits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
NBG_HD double dval(uint64_t b) {
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// combine(op, identity(op), w) == w for every word w
NBG_HD uint64_t identity(int32_t op) {
  return op == OP_MIN_U64 ? ~uint64_t(0) : op == OP_ADD_F64 ? okey::kSign /* -0.0 */ : 0;
}

NBG_HD uint64_t combine(int32_t op, uint64_t a, uint64_t b) {
  switch (op) {
    case OP_ADD_I64: return a + b;
    case OP_MIN_U64: return a < b ? a : b;
    case OP_MAX_U64: return a > b ? a : b;
    default: return dbits(dval(a) + dval(b));
  }
}

// the integer SUM: int64 with wrap-around (signed overflow is undefined, so through uint64)
NBG_HD int64_t wrap_add(int64_t a, int64_t b) { return int64_t(uint64_t(a) + uint64_t(b)); }

// okey::enc_double back to a double: the canonical value of the key's class (+0.0 for a zero, the
// quiet NaN for a NaN, every other value its own bits)
NBG_HD double dec_double(uint64_t k) { return dval((k & okey::kSign) ? (k ^ okey::kSign) : ~k); }
NBG_HD uint8_t dec_bool(uint64_t k) { return k ? 1 : 0; }

// AVG: the `sum / count` of nbg_bound_stats (count > 0: a group has a row)
NBG_HD double avg_int(int64_t wrapped_sum, uint64_t count) { return double(wrapped_sum) / double(count); }
NBG_HD double avg_double(double sum, uint64_t count) { return sum / double(count); }

// 0: a lane, 1: a wave, 2: chunks, a workgroup each
NBG_HD int seg_class(int64_t len) { return len <= kSegLane ? 0 : len <= kSegWave ? 1 : 2; }
NBG_HD int64_t seg_chunks(int64_t len) { return (len + kSegChunk - 1) / kSegChunk; }

// what lane `lane` of `width` lanes holds after its own adds: values lane, lane + width, ...
// get(j): value j of the segment as a word
template <typename Get>
NBG_HD uint64_t strided_partial(int32_t op, const Get& get, int64_t len, int lane, int width) {
  uint64_t acc = identity(op);
  for (int64_t j = lane; j < len; j += width) acc = combine(op, acc, get(j));
  return acc;
}

// the halving of 64 partial words (what the wave's shuffles compute for lane 0); p is overwritten
NBG_HD uint64_t halve64(int32_t op, uint64_t* p) {
  for (int o = kWaveLanes / 2; o >= 1; o >>= 1)
    for (int l = 0; l < o; l++) p[l] = combine(op, p[l], p[l + o]);
  return p[0];
}

// the 256-thread tree over `len` words in scalar code
template <typename Get>
NBG_HD uint64_t block_reduce(int32_t op, const Get& get, int64_t len) {
  uint64_t p[kWaveLanes], w[kBlockLanes / kWaveLanes];
  for (int wv = 0; wv < kBlockLanes / kWaveLanes; wv++) {
    for (int l = 0; l < kWaveLanes; l++) p[l] = strided_partial(op, get, len, wv * kWaveLanes + l, kBlockLanes);
    w[wv] = halve64(op, p);
  }
  return combine(op, combine(op, w[0], w[1]), combine(op, w[2], w[3]));
}

// the whole tree in scalar code: what the device returns for a segment of `len` values
template <typename Get>
NBG_HD uint64_t seg_reduce(int32_t op, const Get& get, int64_t len) {
  const int cls = seg_class(len);
  if (cls == 0) return strided_partial(op, get, len, 0, 1);
  if (cls == 1) {
    uint64_t p[kWaveLanes];
    for (int l = 0; l < kWaveLanes; l++) p[l] = strided_partial(op, get, len, l, kWaveLanes);
    return halve64(op, p);
  }
  // (block_reduce asks for every chunk's word exactly once)
  const auto chunk_word = [&](int64_t c) {
    const int64_t at = c * kSegChunk, clen = len - at < kSegChunk ? len - at : kSegChunk;
    return block_reduce(op, [&](int64_t j) { return get(at + j); }, clen);
  };
  return block_reduce(op, chunk_word, seg_chunks(len));
}

}  // namespace agg
}  // namespace nbg
