// go_launch.h -- the host-side seams between the GO translation units: the structs that cross
// them and the prototypes of the launch and exchange functions, each kernel behind the one host
// function that owns its grid, block and dynamic LDS.  traverse.hip (GoQuery) calls them; what
// bound.hip, fetch.hip and paths.hip need is in query_common.h and engine.h.
#pragma once
#include <initializer_list>
#include <string>
#include <vector>

#include "engine.h"
#include "expr_device.h"
#include "go_device.h"
#include "query_common.h"

namespace nbg {

// a query's counter block (CounterWord / SpecWord index both)
struct Counters {
  unsigned long long* d;  // device counters
  unsigned long long* h;  // pinned host mirror (256 entries)
};

// YIELD materialisation: one program per output column
struct ColOut {
  void* data;
  int32_t type;  // VT_*
  int64_t* len;  // VT_STR: byte length per row (`data` holds the device address of the bytes)
};
constexpr int kMaxYields = 16;
struct YieldArgs {
  int32_t ncols;
  ColOut cols[kMaxYields];
};

// ---- counters.hip ---------------------------------------------------------------------------
// a host wait of the engine on the device (Timing::host_waits counts them; waits inside the
// transport are not the engine's)
void host_sync_at(Ctx& c, const char* file, int line);
#define host_sync(c) host_sync_at((c), __FILE_NAME__, __LINE__)
// records a pooled timing event on the query stream; returns its pool index
constexpr size_t kNoEvent = ~size_t(0);
// an event recorded on the engine stream for deferred hop timing (kNoEvent: hop_timing off)
size_t timing_event(Ctx& c);
// time of the exchanges between ranks: an event pair around each, read after the query (a host
// wait per collective here would serialise the stream-ordered transport)
struct CommTimer {
  Ctx& c;
  size_t a;
  explicit CommTimer(Ctx& cc) : c(cc), a(timing_event(cc)) {}
  ~CommTimer() {
    const size_t b = timing_event(c);
    if (a != ~size_t(0) && b != ~size_t(0)) c.tpend.push_back(Ctx::PendingTime{a, b, -1, 2});
  }
};

// ---- expand.hip -----------------------------------------------------------------------------
// frontier degree scan: fills c.ws_off[0..nF] and returns total edges (synchronises)
// known >= 0: the caller already has the total (from a compaction's partials): no round trip
int64_t degree_scan(Ctx& c, const int32_t* F, int64_t nF, const Csr& csr, DevBuf& degbuf, int64_t known);
// one expansion of the frontier a.F over E flattened edges (k_tile_rows unless the table is
// ready, then k_expand<MODE, pk>), between two timing events; MODE: EXP_MARK, EXP_ROWS, EXP_FLAGS
template <int MODE>
void launch_expand(Ctx& c, ExpandArgs a, int pk, const FastArgs& fp, const Program* dprog, const EvalEnv& env,
                   int64_t E, bool tile_rows_ready = false);

// ---- bottom_up.hip --------------------------------------------------------------------------
// sums the [kSlots][kAggBlocks] block partials of nblocks blocks into out[0, kSlots)
// (k_reduce_partials, one block); gate: a speculated hop's gate word, 0 = do nothing
void reduce_partials(Ctx& c, const unsigned long long* partials, int nblocks, unsigned long long* out,
                     const unsigned long long* gate = nullptr);
// QArgs of a hop on es: unpacked words, packed words whose every value is read (no typed
// compare, or one on another column than the packed one), or the bucket decisions (qpred.h).
QArgs make_qargs(const EdgeSpace& es, int pk, int fcol, const FastArgs& fp);
// the frontier list of a bitmap: the local rows of its set bits to out, their count added to
// *n_out (k_bits_compact<0>)
void launch_bits_list(Ctx& c, const uint32_t* bits, int64_t rows, int64_t lo, int32_t* out, unsigned long long* n_out);
// DISTINCT _dst output: the vids of a bitmap's set rows (k_bits_compact<1, 8, 1>)
void launch_bits_vids(Ctx& c, const uint32_t* bits, int64_t rows, int64_t lo, void* out, unsigned long long* n_out,
                      const unsigned long long* gate);
// what a bottom-up hop's launch ran
struct BuLaunch {
  size_t ev_first = kNoEvent;  // timing event at the end of the first pass (the hop's kernel_ms)
  std::string k0, k1;          // rocprof names of the first-pass and the rest-pass kernel
  bool rest_rec = false;       // the rest pass read the rest records
  uint64_t od_bytes = 0;       // out-degree bytes and tile_shape words the first pass read (non-final hop)
  uint64_t flag_bytes = 0;     // tile_wide bytes the first pass read (final hop, bu_fin_narrow)
};
// bottom-up hop: the first pass over the quad slab and the pending rows' rests; counters reduced
// into out[0..8) (no synchronisation)
BuLaunch launch_bu_lean(Ctx& c, EdgeSpace& es, const uint32_t* fb, uint32_t* nbits, const uint32_t* odeg, int pk,
                        const FastArgs& fp, int fcol, unsigned long long* out, bool hop_front,
                        unsigned long long* gate = nullptr, GateIn gi = GateIn{}, bool out_zero = false,
                        int shards = 1);
// byte models of a bottom-up hop's two passes from their counters
uint64_t bu_first_bytes(const unsigned long long* h, int64_t n_rows, uint64_t od_bytes);
uint64_t bu_rest_bytes(const unsigned long long* h, int pred_width, bool rec);

// ---- frontier.hip ---------------------------------------------------------------------------
constexpr int kSmallStarts = 4096;  // k_starts_small: at most that many starts
int64_t map_bytes(const Ctx& c);    // the byte map's size (64 B past the padded vertex space)
// the query workspaces of Ctx for a frontier of at most nF_cap entries (first use: allocates)
void ensure_workspaces(Ctx& c, int64_t nF_cap);
// element-wise sum of a few host counters over ranks
void allsum(Ctx& c, int64_t* v, int n, unsigned long long* dscratch);
// device counters summed over ranks into dst (stream-ordered: a gate kernel reads the sums)
void dev_allsum(Ctx& c, const unsigned long long* K, std::initializer_list<int> idx, unsigned long long* dst);
// owned frontier bitmap -> bitmap over the whole gidx space
const uint32_t* global_bits(Ctx& c, const uint32_t* owned);
// global_bits + every rank's two counters (n, e) at cnt into all[2r, 2r + 2), one exchange
const uint32_t* global_bits_cnt(Ctx& c, const uint32_t* owned, const unsigned long long* cnt, unsigned long long* all);
// top-down hops mark dsts of every rank in the global byte-map: ship each owner its slice as
// a bitmap and OR the received slices back into the owned range of the map
void exchange_marks(Ctx& c, uint8_t* map, uint32_t* owned_bits = nullptr, const uint32_t* odeg = nullptr,
                    unsigned long long* sums = nullptr);
// multi-step $- / $var roots: the elementwise minimum over ranks of every owned dst's root
void exchange_roots(Ctx& c, int32_t* root_next);
// the byte map's owned slice -> frontier list / bitmap and the counters kCntList, kCntSet,
// kCntDegSum, kCntKept (k_compact, then the partials' reduction unless the blocks add)
void launch_compact(Ctx& c, uint8_t* map, int64_t lo, int64_t n, const int64_t* row_ptr, const uint8_t* row_ok,
                    int require_deg, int32_t* out, uint16_t* bits, unsigned long long* Kd,
                    const uint32_t* odeg = nullptr, bool sums_zero = false, int shards = 1, int64_t own_lo = 0,
                    int64_t own_hi = -1, uint16_t* own_bits = nullptr, int64_t n_read = -1);
// the start kernels (starts' gidx sg[0, ns), owned range [lo, hi)):
// one block: lookup, dedup, list F, degree scan (c.ws_off), tile rows (c.ws_tile_rows), counters
void launch_starts_small(Ctx& c, const int64_t* vids, int64_t ns, int32_t* sg, int64_t lo, int64_t hi, const Csr& csr,
                         uint32_t* bits, int32_t* F, unsigned long long* Kd);
// the starts with out-edges as the list F, duplicates kept; their count added to *n_out
void launch_list_starts(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, const int64_t* row_ptr,
                        const uint8_t* row_ok, int32_t* F, unsigned long long* n_out);
// dedup through the frontier bitmap: bits, list F and the counters launch_compact leaves
void launch_starts_bits(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, const uint32_t* odeg,
                        uint32_t* bits, int32_t* F, unsigned long long* Kd);
// the owned starts marked in the byte map
void launch_mark_gidx(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, uint8_t* map);
// *sum += the out-degrees of every owned start, duplicates included
void launch_starts_degree(Ctx& c, const int32_t* sg, int64_t ns, int64_t lo, int64_t hi, const int64_t* row_ptr,
                          const uint8_t* row_ok, unsigned long long* sum);
// $- input table index: gidx of starts[i] -> i in the hash table (keys, rows) of mask + 1 slots
void launch_input_index(Ctx& c, const int32_t* sg, int64_t ns, int32_t* keys, int32_t* rows, uint32_t mask);
// root[gidx of start i] = srank[i], tab[srank[i]] = that gidx
void launch_root_init(Ctx& c, const int32_t* sg, const int32_t* srank, int64_t ns, int32_t* root, int32_t* tab);

// ---- go_variants.hip ------------------------------------------------------------------------
// once per snapshot (collective): the out-degree statistics over ranks (EdgeSpace::top_deg, ...)
void global_degree_stats(Ctx& c, EdgeSpace& es);
// the exact mirror check of a one-rank, non-sharded context (k_mirror_check)
bool check_mirror(Ctx& c, EdgeSpace& es);
// GO UPTO's hops over the n_own owned rows (at most upto_grid blocks, sums into `shards` shards):
// the claim behind a top-down hop (mark: the owned slice of the byte map) ...
void launch_upto_claim(Ctx& c, uint8_t* mark, int64_t n_own, int64_t n_read, const uint32_t* odeg,
                       unsigned long long* vis, unsigned long long* uni, unsigned long long* next, int32_t* list,
                       unsigned long long* list_n, unsigned long long* sums, int shards);
// ... and the bottom-up hop over es.tr (rows at or past n_scan have no in-edge)
void launch_upto_bu(Ctx& c, const EdgeSpace& es, int64_t n_own, int64_t n_scan, const uint32_t* fb,
                    const uint32_t* odeg, unsigned long long* vis, unsigned long long* uni, unsigned long long* next,
                    unsigned long long* sums, int shards);
// REVERSELY's pull hop over the first `rows` out rows of es (ideg null: the final hop)
void launch_rev_pull(Ctx& c, const EdgeSpace& es, int64_t rows, int64_t n_own, const uint32_t* fb,
                     const uint32_t* ideg, unsigned long long* next, unsigned long long* sums, int shards);

// ---- yield.hip ------------------------------------------------------------------------------
// the NBG_T_* column type of a program's VT_* result
int32_t result_type(int32_t vt);
// the YIELD programs over n (src, edge) rows into ya's columns (rows_edge null: vertex rows);
// evaluation errors counted at *err
void launch_materialize(Ctx& c, const int32_t* rows_src, const int64_t* rows_edge, int64_t n, const Program* progs,
                        const YieldArgs& ya, const EvalEnv& env, int64_t lo, unsigned long long* err);
// the default YIELD: out[i] = the vid of row i's dst
void launch_yield_dst(Ctx& c, const int64_t* rows_edge, int64_t n, const int32_t* col, int64_t* out);
// gidx list (local indices + lo) -> vids
void launch_local_to_vid(Ctx& c, const int32_t* loc, int64_t n, int64_t lo, int64_t* out);
// a STRING column in two steps that only enqueue; the caller waits between them.  First: off[0, n]
// = the exclusive scan of len[0, n] (len[n] = 0), and off[n], the byte total, copied to *total
void str_offsets(Ctx& c, const int64_t* len, int64_t n, DevBuf& off, int64_t* total);
// then: the rows' bytes (addr[i], off[i + 1] - off[i]) packed into `bytes` (allocated here);
// false: nothing to pack, no launch
bool str_pack(Ctx& c, const int64_t* addr, const int64_t* off, int64_t n, int64_t total, DevBuf& bytes);
// DISTINCT with several ranks: every row goes to rank hash(row) % G (all copies of a row meet
// on one rank), then the local dedup runs as with one rank.  Returns the received row count.
int64_t shuffle_rows(Ctx& c, YieldArgs& ya, std::vector<DevBuf>& cols, int64_t n);
// DISTINCT over whole rows: a hash table keeps one row of each value, then every column (and
// STRING length column in slen) is compacted by the keep flags.  Returns the kept row count.
int64_t dedup_rows(Ctx& c, YieldArgs& ya, std::vector<DevBuf>& cols, std::vector<DevBuf>& slen, int64_t nrows);

}  // namespace nbg
