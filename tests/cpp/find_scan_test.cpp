// find_scan_test.cpp -- nebula_amd/csrc/find_scan.h (the arithmetic of FIND's column scan) against
// scalar restatements, on the host: no HIP, no GPU.  tests/test_find_scan.py builds and runs it.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "find_scan.h"

using namespace nbg;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (++failures <= 20) {                  \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                   \
        printf("\n");                          \
      }                                        \
    }                                          \
  } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// scalar restatement: the fast_cmp table written out
static bool cmp_ref(int op, int64_t a, int64_t k) {
  return op == 0 ? a < k : op == 1 ? a <= k : op == 2 ? a > k : op == 3 ? a >= k : op == 4 ? a == k : a != k;
}

template <typename T>
static void pack(const T* v, uint64_t* w) {  // 8 elements as the column stores them (little-endian)
  memcpy(w, v, 8 * sizeof(T));
}

template <typename T, int W>
static void check_width(int64_t tmin, int64_t tmax) {
  static_assert(sizeof(T) == W, "width");
  std::vector<int64_t> interesting = {tmin, tmin + 1, -1, 0, 1, tmax - 1, tmax};
  // constants: each column's min and max, just inside, and just outside them where int64 has room
  std::vector<int64_t> consts = {tmin, tmin + 1, tmax - 1, tmax, 0, -1, 1, 499};
  if (tmin > INT64_MIN) consts.push_back(tmin - 1);
  if (tmax < INT64_MAX) consts.push_back(tmax + 1);
  consts.push_back(INT64_MIN);
  consts.push_back(INT64_MAX);
  for (int round = 0; round < 400; round++) {
    T v[8];
    for (int k = 0; k < 8; k++) {
      const uint64_t r = rnd();
      v[k] = (r & 3) == 0 ? T(interesting[(r >> 8) % interesting.size()]) : T(r >> 16);
    }
    uint64_t w[W];
    pack<T>(v, w);
    for (int k = 0; k < 8; k++)
      CHECK(find_elem<W>(w, k) == int64_t(v[k]), "W=%d elem %d: %lld != %lld", W, k, (long long)find_elem<W>(w, k),
            (long long)v[k]);
    for (int op = 0; op < 6; op++)
      for (int64_t c : consts)
        for (int nvalid = 0; nvalid <= 8; nvalid += (round % 8 == 0 ? 1 : 8)) {
          uint32_t want = 0;
          for (int k = 0; k < nvalid; k++)
            if (cmp_ref(op, int64_t(v[k]), c)) want |= 1u << k;
          const uint32_t m = find_lane_mask<W>(w, op, c, nvalid);
          CHECK(m == want, "W=%d op=%d c=%lld nvalid=%d: mask %x != %x", W, op, (long long)c, nvalid, m, want);
        }
  }
}

static void check_masks_and_ranks() {
  // every one of the 256 pass patterns, as a lane of 0 / 1 values compared with > 0
  for (uint32_t pat = 0; pat < 256; pat++) {
    int8_t v8[8];
    int64_t v64[8];
    uint8_t pres[8];
    for (int k = 0; k < 8; k++) {
      v8[k] = (pat >> k) & 1 ? 1 : 0;
      v64[k] = (pat >> k) & 1 ? INT64_MAX : INT64_MIN;
      pres[k] = (pat >> k) & 1 ? 0 : uint8_t(1 + k);  // absent where the pattern has a bit
    }
    uint64_t w1[1], w8[8], p;
    pack<int8_t>(v8, w1);
    pack<int64_t>(v64, w8);
    memcpy(&p, pres, 8);
    CHECK(find_lane_mask<1>(w1, 2, 0) == pat, "pattern %x W=1", pat);
    CHECK(find_lane_mask<8>(w8, 2, 0) == pat, "pattern %x W=8", pat);
    CHECK(find_lane_mask<1>(w1, 4, 0) == (~pat & 0xffu), "pattern %x ==", pat);
    CHECK(find_absent_mask(p) == pat, "absent pattern %x", pat);
    for (int nv = 0; nv <= 8; nv++) CHECK(find_absent_mask(p, nv) == (pat & ((1u << nv) - 1u)), "absent %x nvalid %d", pat, nv);
    // ranks: the passers of the lane count 0, 1, 2, ... in entry order
    int seen = 0;
    for (int k = 0; k < 8; k++) {
      CHECK(find_rank(pat, k) == seen, "rank pattern %x k %d", pat, k);
      seen += (pat >> k) & 1;
    }
  }
}

static void check_tail_bounds() {
  const int64_t sizes[] = {0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, 4101};
  for (int64_t nnz : sizes) {
    const int64_t tiles = find_tiles(nnz);
    CHECK(tiles == (nnz + 2047) / 2048, "tiles of %lld", (long long)nnz);
    CHECK(tiles * kFindTile >= nnz && (tiles == 0 || (tiles - 1) * int64_t(kFindTile) < nnz), "tile cover %lld", (long long)nnz);
    int64_t covered = 0;
    for (int64_t t = 0; t < tiles; t++) {
      const int64_t e1 = find_tile_end(t, nnz);
      CHECK(e1 > t * kFindTile && e1 <= nnz && e1 <= (t + 1) * int64_t(kFindTile), "tile end %lld of %lld", (long long)t, (long long)nnz);
      for (int lane = 0; lane < kFindThreads; lane++) {
        const int64_t e0 = t * kFindTile + int64_t(lane) * kFindItems;
        const int nv = find_lane_valid(e0, nnz);
        int want = 0;
        for (int k = 0; k < kFindItems; k++) want += e0 + k < nnz;
        CHECK(nv == want, "valid nnz=%lld e0=%lld: %d != %d", (long long)nnz, (long long)e0, nv, want);
        // a wide lane reads entries e0 .. e0 + 7: all of them must exist
        CHECK(find_lane_wide(e0, nnz) == (e0 + 7 < nnz), "wide nnz=%lld e0=%lld", (long long)nnz, (long long)e0);
        CHECK(!find_lane_wide(e0, nnz) || nv == 8, "wide implies 8 valid");
        covered += nv;
      }
    }
    CHECK(covered == nnz, "lanes cover %lld entries of %lld", (long long)covered, (long long)nnz);
    CHECK(find_lane_valid(nnz, nnz) == 0 && find_lane_valid(nnz + 8, nnz) == 0, "past the end");
  }
}

static int64_t row_ref(const std::vector<int64_t>& rp, int64_t e) {  // linear: the row whose range holds e
  for (size_t r = 0; r + 1 < rp.size(); r++)
    if (rp[r] <= e && e < rp[r + 1]) return int64_t(r);
  return -1;
}

static void check_row_search() {
  // degree lists with leading, trailing and interior runs of empty rows
  const std::vector<std::vector<int>> shapes = {
      {1},
      {5},
      {0, 0, 0, 3},
      {3, 0, 0, 0},
      {2, 0, 0, 0, 4},
      {0, 1, 0, 1, 0, 1, 0},
      {0, 0, 7, 0, 0, 0, 1, 0, 0, 2500, 0, 1, 0, 0},
      {1, 1, 1, 1, 1, 1, 1, 1, 1},
      {0, 0, 0, 0, 0, 0, 0, 0, 1},
      {4099, 1, 1},
  };
  std::vector<std::vector<int>> all = shapes;
  for (int round = 0; round < 200; round++) {
    std::vector<int> d(1 + rnd() % 40);
    for (int& x : d) x = (rnd() & 3) ? 0 : int(rnd() % 9);
    d[rnd() % d.size()] += 1;  // at least one entry
    all.push_back(d);
  }
  for (const auto& d : all) {
    std::vector<int64_t> rp(d.size() + 1, 0);
    for (size_t r = 0; r < d.size(); r++) rp[r + 1] = rp[r] + d[r];
    const int64_t n_rows = int64_t(d.size()), nnz = rp.back();
    auto get = [&](int64_t r) { return rp[size_t(r)]; };
    for (int64_t e = 0; e < nnz; e++) {
      const int64_t want = row_ref(rp, e);
      const int64_t r = find_row(get, 0, n_rows, e);
      CHECK(r == want, "row of %lld: %lld != %lld", (long long)e, (long long)r, (long long)want);
      CHECK(d[size_t(r)] > 0, "an empty row was returned");
      // any bracket [lo, hi) with rp(lo) <= e < rp(hi) gives the same row: a tile's slice
      for (int t = 0; t < 4; t++) {
        int64_t lo = int64_t(rnd() % uint64_t(want + 1)), hi = want + 1 + int64_t(rnd() % uint64_t(n_rows - want));
        while (hi <= n_rows && rp[size_t(hi)] <= e) hi++;
        CHECK(find_row(get, lo, hi, e) == want, "bracket [%lld, %lld) of %lld", (long long)lo, (long long)hi, (long long)e);
      }
    }
  }
}

int main() {
  check_width<int8_t, 1>(INT8_MIN, INT8_MAX);
  check_width<int16_t, 2>(INT16_MIN, INT16_MAX);
  check_width<int32_t, 4>(INT32_MIN, INT32_MAX);
  check_width<int64_t, 8>(INT64_MIN, INT64_MAX);
  check_masks_and_ranks();
  check_tail_bounds();
  check_row_search();
  if (failures) {
    printf("find_scan: %d failures\n", failures);
    return 1;
  }
  printf("find_scan ok\n");
  return 0;
}
