// traverse.hip -- GO N STEPS on the host: GoQuery (one query's compiled programs, counter block,
// frontier and speculation state, and its phases) and go_run, which calls the phases in order.
// It launches no kernel itself; every device step is a named function of go_launch.h:
//   expand.hip       the top-down expansion (k_expand) and the frontier's degree scan
//   bottom_up.hip    the bottom-up hop's two passes, bitmap -> list / vids
//   frontier.hip     start kernels, compaction, the exchanges between ranks, workspaces
//   go_variants.hip  GO UPTO's and REVERSELY's hops, the once-per-snapshot degree statistics
//   yield.hip        YIELD materialisation, STRING packing, DISTINCT over rows
//   counters.hip     counter publication (fetch_counters) and query timing
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "expr_device.h"
#include "go_launch.h"
#include "program.h"
#include "qpred.h"
#include "query_common.h"
#include "rows.h"

namespace nbg {

namespace {

// a lone YIELD _dst (also the default YIELD): no YIELD program runs, the rows are dst vids
bool is_lone_dst(const std::vector<Program>& yields) {
  return yields.size() == 1 && yields[0].n == 1 && yields[0].ins[0].op == P_DST;
}
// the predicate can run bottom-up: only when it cannot error (the reference fails the query on
// any row's eval error, so every row must be evaluated when errors are possible) -- none, or a
// typed compare on a column without absent values that the transposed CSR carries
bool pred_runs_bottom_up(const FastPred& fpk, const FastArgs& fp, const EdgeSpace& es) {
  return fpk.kind == PK_NONE || (fpk.kind == PK_FAST && fp.present == nullptr &&
                                 es.tr.props.size() > size_t(fpk.col) && es.tr.props[size_t(fpk.col)].data.p);
}

// One GO query: its compiled programs, counter block, frontier and speculation state, and the
// phases go_run calls in order.
struct GoQuery {
  Ctx& c;
  const nbg_go_spec& s;
  EdgeSpace& es;
  // GO ... REVERSELY (edge_type < 0): the hops expand the in keys.  The direction's view, chosen
  // once: csr (es.out / es.in) and D (the forward view aliases the out-degree fields, so forward
  // queries run the launches they always ran; the reverse view is EdgeSpace::rev).  REVERSELY is
  // host-driven, one counter fetch per hop: no k_starts_small first hop, no go_rep1, no
  // speculation chain, no host_direct; its bottom-up form is the pull hop (hop_rev_pull).
  const bool rev;
  Csr& csr;
  struct Dir {
    const uint32_t* deg = nullptr;            // es.odeg / es.rev.ideg
    const std::vector<int64_t>* top = nullptr;  // es.top_deg / es.rev.top_deg
    int64_t max_deg_global = -1, nnz_global = 0;
  } D;
  nbg_rows* out;
  // the query's device-time events too are instrumentation: with hop_timing off none is recorded
  // (an event between two launches leaves ~5.5 us between them on the device)
  const bool tot_ev;

  // ---- compile() ----
  Program where{};
  std::vector<Program> yields;
  std::vector<Field> in_fields;  // $- / $var input table columns
  const bool has_where, default_yield;
  // GO UPTO N STEPS (nbg_go_spec::upto with steps > 1; UPTO 1 STEPS is GO 1 STEPS): run_upto
  const bool upto;
  // compile errors are deferred to the final step, as the reference only reports them when the
  // final getNeighbors request is actually sent
  int32_t deferred = NBG_OK;
  std::string deferred_msg;
  bool uses_input = false, lone_dst = false;  // lone_dst: is_lone_dst(yields)
  // the WHERE's class and its typed compare, classified once (no deferred error): read by the
  // speculated final hop and by the final step
  FastPred fpk{};
  FastArgs fp{};
  bool pred_bu = false;    // pred_runs_bottom_up
  const FastArgs no_fp{};  // the non-final hops evaluate no predicate

  // ---- resolve_starts() ----
  int64_t lo = 0, hi = 0, n_own = 0, ns = 0;
  Counters K{};
  DevBuf degbuf;
  uint8_t* map = nullptr;
  const int64_t* row_ptr = nullptr;
  const uint8_t* row_ok = nullptr;  // rows whose keys sit outside hash(vid)'s part
  bool bu_ok = false;
  int64_t bu_div = 4, bu_force = 0;  // bottom-up when E >= nnz / bu_div; force 1: always, -1: never
  int32_t* d_sg = nullptr;           // the starts' gidx
  // a first hop that is certainly top-down (no transposed CSR, or even the ns largest
  // out-degrees sum below the bottom-up threshold) from a few starts: one launch builds its
  // frontier and degree scan (k_starts_small) and the hop runs without a round trip (the
  // expansion reads the frontier size from the scan; the counts come back with the compaction's)
  // (with several ranks each rank's k_starts_small keeps its own starts; the hop-1 marks are
  // exchanged before the compaction)
  bool fast1 = false;
  bool multi = false;  // counters summed over ranks on the device (dev_allsum) land at kCntGlobal
  // several ranks (option go_rep1): every rank runs the whole first hop -- every start, over a
  // replica of the out CSR (ensure_rep_out, built on first use) -- into a frontier bitmap over the
  // whole gidx space, so the hop needs no mark exchange and the second hop no frontier allgather:
  // one collective a C3 query instead of three.  (The same branch on every rank: ns, the degree
  // statistics and the options are the same everywhere.)
  bool rep1 = false;
  const Csr* csr1 = nullptr;  // the first hop's rows (rep1: the replica)
  int64_t max_odeg1 = -1;
  // the marks of a top-down hop over this edge type are its dsts: rows with an in-edge, the
  // first bu_in_tiles tiles of the owned range (class-ordered numbering); the compactions read
  // the byte map that far and write the bitmap past it as zero
  int64_t map_bound = 0;
  int64_t hop1_scanned = -1;  // hop-1 rows with duplicate starts rescanned (k_starts_degree)
  int64_t Eg_known = -1;      // several ranks: the start frontier's out-degree sum over ranks
  // one rank: the hop-1 compaction and the speculated hops add their block sums into kSumShards
  // shards (option sum_shards; block_add_sums), folded by their readers -- the gates and the
  // counter fetches.  Shards are zero at the query start (k_starts_small / the memset);
  // clean_shards zeroes them again before any later dense use of the same words.
  int ks = 1;
  bool shards_dirty = false;
  // a host-chosen bottom-up hop's HopWord block lies over [kCntList, kHopWords) (kCntWhereErr too)
  bool hop_words_stale = false;

  // ---- frontier state: a list of local rows (top-down) and/or a bitmap (bottom-up) ----
  int32_t* F = nullptr;
  int64_t nF = 0;
  int cur = 0;
  bool have_list = true, off_ready = false;
  // E = sum of the frontier's out-degrees = the adjacency entries the hop scans (TEPS numerator,
  // SURVEY 8d); E_known: when a compaction already produced it; Eg: over all ranks
  int64_t E = -1, E_known = -1, Eg = 0;
  int64_t list_n = -1;      // length of the list the bitmap will compact to, when already counted
  int64_t nset_global = 0;  // "starts_ non-empty" (GoExecutor.cpp:93-97)
  uint32_t *bitsA = nullptr, *bitsB = nullptr;  // the frontier bitmap (k_compact / bottom-up hops) and the next

  // ---- bind_inputs() ----
  ExpandArgs a{};
  EvalEnv env{};
  DevBuf in_keys, in_rows, in_tab;
  std::vector<DevBuf> in_cols;
  // STEPS > 1: graphd maps every dst of a non-final step back to a start (VertexBackTracker,
  // GoExecutor.h:174-193, GoExecutor.cpp:420-424) in RPC response order, last write winning --
  // order-dependent whenever a vertex is reached from several starts.  The build's rule
  // (DESIGN.md): each hop reads the previous hop's roots and a dst takes the smallest root vid
  // among its in-edges' srcs; it is the reference's answer whenever the root is unique.
  bool multi_root = false;
  DevBuf root_buf[2], root_tab;
  int root_cur = 0;

  // ---- the speculation chain ----
  // Speculative bottom-up hops.  A direction choice needs the previous hop's counters on the
  // host, one round trip per hop; instead, right after a top-down hop's compaction, the
  // remaining hops are enqueued as bottom-up hops gated on the device (GateIn: the same rule as
  // want_bu, on the same counters) before the one counter fetch.  A hop whose gate is 0 does
  // nothing (every kernel returns at once), and the host continues from there as before: the
  // direction never changes a hop's result, only its cost.  The final step is speculated only
  // as the DISTINCT _dst bottom-up hop (a predicate that cannot error, no deferred compile
  // error).  Each hop has a SpecWord block in the counters.
  // (several ranks: each gate reads counters summed over ranks on the device, dev_allsum, and
  // every rank enqueues the same chain of collectives, so every rank takes the same branches)
  struct Spec {
    int32_t hop;  // Timing::hops index it will take
    bool final;
    BuLaunch L;  // what its own launch ran
  };
  std::vector<Spec> spec;
  bool spec_ok = false, fin_spec = false;  // hops / the final step can be speculated
  unsigned long long spec_thr = 1;
  bool spec_blocks_used = false;
  // several ranks (piggy): every speculated hop's frontier allgather carries the previous hop's
  // (n, e) of every rank to its gate (GateIn::all), one exchange per hop instead of an allgather
  // and an all-reduce
  bool piggy_used = false;
  // option host_direct: a DISTINCT _dst result that goes to the host is written by the bottom-up
  // output kernel straight into pinned host memory (mapped into the device's address space), so
  // the hand-out copies nothing
  // (r06j: stores from the device reach 54.6 GB/s into pinned host memory, hipMemcpyAsync 29.7:
  // C3's 173 MB hand-out 7.4 -> 3.8 ms end to end)
  bool host_direct = false;
  DevBuf spec_vids;
  HostBuf spec_hvids;
  // the speculated final hop that ran (spec_replay): its block and launch
  unsigned long long fin_h[kSpecWords] = {};
  BuLaunch fin_L;
  bool fin_done = false;

  // ---- the final step ----
  DevBuf dprog;  // the WHERE program, then the YIELD programs
  std::unique_ptr<HostRows> rows;
  int64_t nrows = 0;
  std::vector<DevBuf> slen;          // STRING yield columns: byte length per row
  std::map<size_t, bool> host_cols;  // columns already in pinned host memory (host_direct)

  GoQuery(Ctx& c_, const nbg_go_spec& s_, EdgeSpace& es_, nbg_rows* out_)
      : c(c_), s(s_), es(es_), rev(s_.edge_type < 0), csr(s_.edge_type < 0 ? es_.in : es_.out), out(out_),
        tot_ev(c_.hop_timing), has_where(s_.where_len > 0),
        default_yield(s_.n_yields == 0), upto(s_.upto == 1 && s_.steps > 1) {}

  // WHERE / YIELD programs, the input table's columns (validated here, uploaded once the starts
  // are resolved) and the predicate's class
  void compile() {
    std::string msg;
    if (s.n_inputs) {
      if (!s.input_names || !s.input_types || !s.input_cols) throw Error(NBG_E_INVALID_ARG, "input table");
      for (size_t i = 0; i < s.n_inputs; i++) {
        const int32_t t = s.input_types[i];
        if (t != NBG_T_VID && t != NBG_T_INT && t != NBG_T_DOUBLE && t != NBG_T_BOOL && t != NBG_T_STRING)
          throw Error(NBG_E_UNSUPPORTED, "input column type");
        if (t == NBG_T_STRING && (!s.input_str_offsets || !s.input_str_offsets[i]))
          throw Error(NBG_E_INVALID_ARG, "input STRING column without offsets");
        in_fields.push_back(Field{s.input_names[i] ? s.input_names[i] : "", t});
      }
    }
    const std::vector<Field>* inf = in_fields.empty() ? nullptr : &in_fields;
    if (has_where) {
      int32_t rc = compile_expr(s.where, s.where_len, es.fields, true, !rev, &where, &msg, &c.tag_refs, inf);
      if (rc == NBG_E_UNSUPPORTED || rc == NBG_E_INVALID_ARG) throw Error(rc, "WHERE: " + msg);
      if (rc != NBG_OK) {
        deferred = rc;
        deferred_msg = "WHERE: " + msg;
      }
    }
    if (default_yield) {
      yields.push_back(program_dst());
    } else {
      if (s.n_yields > size_t(kMaxYields)) throw Error(NBG_E_UNSUPPORTED, "too many YIELD columns");
      for (size_t i = 0; i < s.n_yields; i++) {
        Program p{};
        int32_t rc = compile_expr(s.yields[i], s.yield_lens[i], es.fields, true, !rev, &p, &msg, &c.tag_refs, inf);
        if (rc == NBG_E_UNSUPPORTED || rc == NBG_E_INVALID_ARG) throw Error(rc, "YIELD: " + msg);
        if (rc != NBG_OK && deferred == NBG_OK) {
          deferred = rc;
          deferred_msg = "YIELD: " + msg;
        }
        if (rc == NBG_OK && p.result_type == VT_STR && s.distinct && c.sharded)
          throw Error(NBG_E_UNSUPPORTED, "DISTINCT over STRING YIELD columns across ranks");
        yields.push_back(p);
      }
    }
    for (int i = 0; i < where.n && has_where; i++) uses_input |= where.ins[i].op == P_INPUT;
    for (auto& p : yields)
      for (int i = 0; i < p.n; i++) uses_input |= p.ins[i].op == P_INPUT;
    lone_dst = is_lone_dst(yields);
    if (upto && uses_input)
      throw Error(NBG_E_UNSUPPORTED, "GO UPTO with $- / $var properties in WHERE or YIELD is not supported");
    if (deferred == NBG_OK) {
      fpk = has_where ? classify_pred(where, es.fields) : FastPred{};
      fp = fast_args(csr, fpk);
      // (REVERSELY: a legal WHERE reads vertex or input props only; the pull hop evaluates none)
      pred_bu = rev ? !has_where : pred_runs_bottom_up(fpk, fp, es);
      fin_spec = s.distinct && lone_dst && pred_bu;
    }
  }

  void clean_shards() {
    if (!shards_dirty) return;
    NBG_HIP(hipMemsetAsync(K.d + kShardStride, 0, kShardStride * size_t(ks - 1) * 8, c.stream));
    shards_dirty = false;
  }

  // starts -> gidx -> the start frontier: the fast1 and rep1 decisions, then k_starts_small, or
  // the list / bitmap / byte-map paths with their counter fetch
  void resolve_starts() {
    lo = c.owned_lo(), hi = c.owned_hi();
    n_own = hi - lo;
    ensure_workspaces(c, std::max<int64_t>({n_own, int64_t(s.n_starts), 1}));
    K = Counters{c.ws_counters.as<unsigned long long>(), c.host_counters};
    map = c.ws_map.as<uint8_t>();
    bitsA = c.ws_bits_send.as<uint32_t>();
    bitsB = c.ws_bits_recv.as<uint32_t>();
    uint16_t* bits16 = c.ws_bits_send.as<uint16_t>();  // frontier bitmap written by k_compact
    row_ptr = csr.row_ptr.as<int64_t>();
    if (rev) {
      ensure_rev(c, es);
      if (c.opt("rev_mirror_recheck", 0) != 0 && !c.sharded) es.rev.mirror = -1;  // (measurement)
    }
    // (REVERSELY: the pull hop needs mirrored keys -- known, or checked on one rank by want_bu)
    bu_ok = (rev ? es.rev.mirror == 1 || (es.rev.mirror < 0 && !c.sharded) : es.has_tr) && c.opt("bottom_up", 1) != 0;
    bu_div = std::max<int64_t>(1, rev ? c.opt("rev_bu_div", 4) : c.opt("bu_div", 4));
    bu_force = c.opt("bu_force", 0);
    row_ok = csr.row_ok.as<uint8_t>();
    ns = int64_t(s.n_starts);
    c.ws_starts.ensure(size_t(std::max<int64_t>(ns, 1)) * 12 + 64);
    int64_t* d_starts = c.ws_starts.as<int64_t>();
    d_sg = reinterpret_cast<int32_t*>(d_starts + std::max<int64_t>(ns, 1));
    if (!rev && es.out_nnz_global < 0) global_degree_stats(c, es);
    if (rev) D = Dir{es.rev.ideg.as<uint32_t>(), &es.rev.top_deg, es.rev.max_ideg_global, es.rev.in_nnz_global};
    else D = Dir{es.odeg.as<uint32_t>(), &es.top_deg, es.max_odeg_global, es.out_nnz_global};
    // a first hop from ns starts is certainly top-down when even the ns largest out-degrees sum
    // below the bottom-up threshold
    const int64_t deg_bound = ns < int64_t(D.top->size()) ? (*D.top)[size_t(ns)]
                              : D.max_deg_global >= 0     ? ns * D.max_deg_global
                                                          : INT64_MAX;
    const bool td1_certain = !bu_ok || bu_force < 0 || (bu_force == 0 && deg_bound < D.nnz_global / bu_div);
    fast1 = ns > 0 && ns <= kSmallStarts && s.steps >= 2 && td1_certain && !(uses_input && s.steps > 1) &&
            c.opt("starts_small", 1) != 0 && !upto && !rev;
    multi = c.sharded;
    ks = multi ? 1 : int(std::min<int64_t>(std::max<int64_t>(c.opt("sum_shards", kSumShards), 1), kSumShards));
    // the small-start path's one block reads the starts from coherent pinned host memory (the
    // stream's previous query finished before this one was enqueued): no copy between queries
    const int64_t* k_starts = d_starts;
    if (ns && fast1 && c.starts_host) {
      memcpy(c.starts_host, s.starts, size_t(ns) * 8);
      k_starts = c.starts_host;
    } else if (ns) {
      c.h2d(d_starts, s.starts, size_t(ns) * 8);
      if (!fast1) lookup_gidx(c, d_starts, d_sg, ns);
    }
    F = c.ws_front[0].as<int32_t>();
    nset_global = ns;
    // (REVERSELY: the marks are srcs, rows with an out-edge: the owned range)
    map_bound = !rev && es.has_tr && es.bu_in_tiles > 0 ? std::min<int64_t>(n_own, es.bu_in_tiles * 128) : n_own;
    rep1 = fast1 && multi && bu_ok && c.opt("compact_list", 0) == 0 && es.odeg.p && c.opt("go_rep1", 1) != 0;
    csr1 = rep1 ? &es.rep_out : &csr;
    if (rep1) {
      ensure_rep_out(c, es);
      c.ws_bits_rep1.ensure(size_t(map_bytes(c) / 8 + 64));
    }
    max_odeg1 = rep1 ? es.max_odeg_global : es.max_odeg;
    if (fast1) {
      // the hop-1 expansion's tile-row table is written by k_starts_small (sized for the degree bound)
      const int64_t eb = std::max<int64_t>(1, max_odeg1 >= 0 ? int64_t(ns) * max_odeg1 : csr1->nnz);
      c.ws_tile_rows.ensure(size_t(std::min<int64_t>(eb, csr1->nnz + 1) / kTile + 4) * 4);
      launch_starts_small(c, k_starts, ns, d_sg, rep1 ? 0 : lo, rep1 ? c.n_global : hi, *csr1,
                          rep1 ? c.ws_bits_rep1.as<uint32_t>() : bitsA, F, K.d);
      NBG_HIP(hipGetLastError());
      nF = ns;  // an upper bound: the entries past the list have degree 0
      return;
    }
    NBG_HIP(hipMemsetAsync(K.d, 0, kShardStride * kSumShards * 8, c.stream));
    if (!ns) return;
    const bool counted = !(s.steps == 1 && !s.distinct);
    if (!counted) {
      launch_list_starts(c, d_sg, ns, lo, hi, row_ptr, row_ok, F, K.d);
    } else {
      if (!c.sharded && D.deg) {
        // one rank: dedup the starts through the frontier bitmap itself (a few hundred atomics)
        // instead of marking the byte map and compacting the whole vertex space
        NBG_HIP(hipMemsetAsync(bits16, 0, c.ws_bits_send.bytes, c.stream));
        launch_starts_bits(c, d_sg, ns, lo, hi, D.deg, bitsA, F, K.d);
      } else {
        launch_mark_gidx(c, d_sg, ns, lo, hi, map);
        launch_compact(c, map, lo, n_own, row_ptr, row_ok, 1, F, bits16, K.d, D.deg);
      }
      if (!s.distinct) launch_starts_degree(c, d_sg, ns, lo, hi, row_ptr, row_ok, K.d + kCntHop1Rows);
    }
    NBG_HIP(hipGetLastError());
    if (multi && counted) dev_allsum(c, K.d, {kCntDegSum}, K.d + kCntGlobal);
    fetch_counters(c, K.d, multi && counted ? kCntGlobal + 4 : kCntStartWords, K.h);
    nF = int64_t(K.h[kCntList]);
    if (counted) {
      E_known = int64_t(K.h[kCntDegSum]);
      if (multi) Eg_known = int64_t(K.h[kCntGlobal]);
      if (!s.distinct) hop1_scanned = int64_t(K.h[kCntHop1Rows]);
    }
  }

  // the empty result: the single exit of every early return
  int32_t finish_empty() {
    auto h = std::make_unique<HostRows>();
    for (auto& p : yields) {
      h->types.push_back(result_type(p.result_type));
      h->cols.push_back(nullptr);
      h->str_off.push_back(nullptr);
    }
    fill_rows(out, std::move(h), 0, s.keep_on_device != 0);
    hipEventRecord(c.ev[1], c.stream);
    hipEventSynchronize(c.ev[1]);
    float ms = 0;
    hipEventElapsedTime(&ms, c.ev[0], c.ev[1]);
    c.timing.total_ms = ms;
    out->edges_scanned = c.timing.edges_scanned;
    return NBG_OK;
  }

  // the expansions' arguments, the multi-step roots and the $- input table's upload; then the
  // speculation's conditions (they depend on multi_root)
  void bind_inputs() {
    a.row_ptr = row_ptr;
    a.col = csr.col.as<int32_t>();
    a.lo = lo;
    a.map = map;
    a.err = K.d + kCntWhereErr;
    a.storage = 0;
    a.mark_check = 0;
    env = make_env(c, es, csr, s.edge_type);
    multi_root = uses_input && s.steps > 1;
    if (multi_root) {
      // rank of every start's vid among the distinct start vids
      std::vector<int64_t> u(s.starts, s.starts + ns);
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      std::vector<int32_t> rk(size_t(std::max<int64_t>(ns, 1)));
      for (int64_t i = 0; i < ns; i++)
        rk[size_t(i)] = int32_t(std::lower_bound(u.begin(), u.end(), s.starts[i]) - u.begin());
      DevBuf drk;
      drk.alloc(rk.size() * 4);
      NBG_HIP(hipMemcpyAsync(drk.p, rk.data(), rk.size() * 4, hipMemcpyHostToDevice, c.stream));
      for (auto& b : root_buf) {
        b.alloc(size_t(c.n_global + 1) * 4);
        NBG_HIP(hipMemsetAsync(b.p, 0x7f, size_t(c.n_global + 1) * 4, c.stream));  // > every rank
      }
      root_tab.alloc(std::max<size_t>(u.size(), 1) * 4);
      if (ns) launch_root_init(c, d_sg, drk.as<int32_t>(), ns, root_buf[0].as<int32_t>(), root_tab.as<int32_t>());
      host_sync(c);  // rk is pageable host memory
    }
    if (uses_input) {
      uint32_t cap = 64;
      while (cap < uint32_t(2 * std::max<int64_t>(ns, 1))) cap <<= 1;
      in_keys.alloc(size_t(cap) * 4);
      in_rows.alloc(size_t(cap) * 4);
      NBG_HIP(hipMemsetAsync(in_keys.p, 0xff, size_t(cap) * 4, c.stream));
      NBG_HIP(hipMemsetAsync(in_rows.p, 0xff, size_t(cap) * 4, c.stream));
      if (ns) launch_input_index(c, d_sg, ns, in_keys.as<int32_t>(), in_rows.as<int32_t>(), cap - 1);
      NBG_HIP(hipGetLastError());
      std::vector<PropDev> tab;
      for (size_t i = 0; i < s.n_inputs; i++) {
        const int32_t t = s.input_types[i];
        const size_t w = t == NBG_T_BOOL ? 1 : 8;
        DevBuf col, off;
        PropDev pd{t, int32_t(w), nullptr, nullptr, nullptr, nullptr};
        if (t != NBG_T_STRING) {
          col.alloc(std::max<size_t>(size_t(ns) * w, 8));
          if (ns) NBG_HIP(hipMemcpyAsync(col.p, s.input_cols[i], size_t(ns) * w, hipMemcpyHostToDevice, c.stream));
          pd.data = col.p;
        } else {
          const int64_t* ho = s.input_str_offsets[i];
          off.alloc(size_t(ns + 1) * 8);
          NBG_HIP(hipMemcpyAsync(off.p, ho, size_t(ns + 1) * 8, hipMemcpyHostToDevice, c.stream));
          col.alloc(size_t(ho[ns]) + 8);
          if (ho[ns]) NBG_HIP(hipMemcpyAsync(col.p, s.input_cols[i], size_t(ho[ns]), hipMemcpyHostToDevice, c.stream));
          pd = PropDev{t, 8, nullptr, nullptr, off.as<int64_t>(), col.as<uint8_t>()};
        }
        tab.push_back(pd);
        in_cols.push_back(std::move(col));
        in_cols.push_back(std::move(off));
      }
      in_tab.alloc(sizeof(PropDev) * tab.size());
      NBG_HIP(hipMemcpyAsync(in_tab.p, tab.data(), sizeof(PropDev) * tab.size(), hipMemcpyHostToDevice, c.stream));
      host_sync(c);  // `tab` is pageable host memory
      env.in_keys = in_keys.as<int32_t>();
      env.in_rows = in_rows.as<int32_t>();
      env.in_mask = cap - 1;
      env.iprops = in_tab.as<PropDev>();
    }
    host_direct = !s.keep_on_device && c.opt("host_direct", 1) != 0 && !rev;
    spec_ok = bu_ok && !multi_root && bu_force >= 0 && c.opt("bu_spec", 1) != 0 && !upto && !rev;
    spec_thr = bu_force > 0 ? 1ull : (unsigned long long)std::max<int64_t>(1, D.nnz_global / bu_div);
  }

  // the frontier as a list: compacts the bitmap when only that exists
  void ensure_list() {
    if (have_list) return;
    cur ^= 1;
    F = c.ws_front[cur].as<int32_t>();
    NBG_HIP(hipMemsetAsync(K.d, 0, 8, c.stream));
    launch_bits_list(c, bitsA, n_own, lo, F, K.d + kCntList);
    if (list_n >= 0) {
      nF = list_n;  // counted by the compaction that wrote the bitmap: no round trip
    } else {
      fetch_counters(c, K.d, kCntList + 1, K.h);
      nF = int64_t(K.h[kCntList]);
    }
    list_n = -1;
    have_list = true;
    off_ready = false;
  }
  // ... and its degree scan
  void ensure_off() {
    ensure_list();
    if (off_ready) return;
    E = nF ? degree_scan(c, F, nF, csr, degbuf, E_known) : 0;
    E_known = E;
    off_ready = true;
  }
  // direction choice is global (every rank must take the same branch: bottom-up allgathers)
  // (REVERSELY: bottom-up is the pull hop, for mirrored keys only -- an unknown mirror state is
  // settled here, at the first query that would pull, on one rank -- and never under UPTO)
  bool want_bu(int64_t eg) {  // (multi-step roots need every in-edge: top-down only)
    const bool w = eg > 0 && bu_ok && !multi_root && bu_force >= 0 && (bu_force > 0 || eg >= D.nnz_global / bu_div);
    if (!w || !rev) return w;
    if (upto) return false;
    if (es.rev.mirror < 0) es.rev.mirror = !c.sharded && check_mirror(c, es) ? 1 : 0;
    return es.rev.mirror == 1;
  }
  // the start frontier's degree scan and its out-degree sum over ranks
  void first_degrees() {
    if (fast1) {
      off_ready = true;  // k_starts_small wrote the scan; E is counted on the device
      return;
    }
    ensure_off();
    Eg = E;
    if (Eg_known >= 0) Eg = Eg_known;
    else allsum(c, &Eg, 1, K.d + kCntRed);
  }
  // where a DISTINCT _dst output goes: a pinned host block (host_direct) or a device block
  void* vid_block(DevBuf& d, HostBuf& hb) {
    if (host_direct) {
      host_pool_cap(c);
      hb.release();  // (a second speculation chain in one query replaces the first's block)
      hb.alloc(c.host_pool, size_t(c.n_global + 64) * 8);
      return hb.p;
    }
    d.alloc(size_t(c.n_global + 64) * 8);
    return d.p;
  }

  // a bottom-up hop's launches between two timing events; the hop's and its first pass's times
  // are read later (timing_resolve) into Timing::hops[hop]
  template <typename Fn>
  BuLaunch timed_bu(int32_t hop, Fn launch) {
    const size_t ia = timing_event(c);
    BuLaunch L = launch();
    const size_t ib = timing_event(c);
    c.tpend.push_back(Ctx::PendingTime{ia, ib, hop, 0});
    c.tpend.push_back(Ctx::PendingTime{ia, L.ev_first, hop, 1});
    return L;
  }
  // the statistics of a bottom-up hop that ran, from its HopWord block h and its launch; a final
  // hop (DISTINCT _dst, out_rows rows) adds its output (k_bits_compact<1>): next bits once, vid_of
  // read + vid written
  void record_bu_hop(const unsigned long long* h, const BuLaunch& L, bool final = false, int64_t out_rows = 0) {
    c.timing.expand_launches++;
    c.timing.bu_steps++;
    const int pw = final && fpk.kind == PK_FAST ? fp.width : 0;
    const uint64_t kb = bu_first_bytes(h, es.tr.n_rows, L.od_bytes + L.flag_bytes), hb = kb + bu_rest_bytes(h, pw, L.rest_rec);
    c.timing.expand_bytes += hb + (final ? uint64_t(es.tr.n_rows) / 8 + uint64_t(out_rows) * 16 : 0);
    c.timing.hop(1, final, 0.0, h, 0.0, kb);
    c.timing.name_last_hop(L.k0, L.k1, final ? "nbg::k_bits_compact<1, 8, 1>" : nullptr);
  }
  // the next frontier is the bitmap a bottom-up hop wrote (its HopWord block h); list_len: the
  // bitmap's population when the hop's counts give it (ensure_list then needs no round trip)
  void adopt_bu(const unsigned long long* h, int64_t list_len, int64_t n_global, int64_t e_global) {
    std::swap(bitsA, bitsB);
    have_list = false;
    list_n = list_len;
    off_ready = false;
    E = int64_t(h[kHopDegSum]);
    E_known = E;
    nset_global = n_global;
    Eg = e_global;
  }
  // the next frontier is what a compaction left (counters fetched): the list, or with lazy only
  // the bitmap and its counted length.  whole_space (go_rep1): the compaction ran over every
  // rank's rows, its sums are global and this rank's share sits at kCntOwnKept / kCntOwnDegSum.
  // Several ranks otherwise: the global counts come from the first speculated hop's gate
  // (piggy) or from dev_allsum's words.
  void adopt_compaction(bool lazy, bool whole_space) {
    int64_t ng = int64_t(K.h[kCntSet]), eg = int64_t(K.h[kCntDegSum]);
    if (multi && !whole_space) {
      const unsigned long long* g = piggy_used ? K.h + kSpecBase + kSpecSumN : K.h + kCntGlobal;
      ng = int64_t(g[0]), eg = int64_t(g[1]);
    }
    nF = lazy ? 0 : int64_t(K.h[kCntList]);
    list_n = lazy ? int64_t(K.h[whole_space ? kCntOwnKept : kCntKept]) : -1;
    E = int64_t(K.h[whole_space ? kCntOwnDegSum : kCntDegSum]);
    E_known = E;
    nset_global = ng;
    Eg = eg;
    have_list = !lazy;
    if (lazy) cur ^= 1;  // ensure_list flips to the list buffer again
    off_ready = false;
  }

  // enqueue the gated hops from step `first` on; the compaction behind them left its counts at
  // (e, n) and its bitmap in bitsA; hop0 = the Timing::hops index of the first one
  // several ranks (piggy): instead of (e, n), cnt = this rank's (n, e) of the compaction behind
  // the first hop; every hop's frontier allgather carries the previous hop's (n, e) of every rank
  // to its gate (GateIn::all)
  // fb_first (several ranks, go_rep1): the first hop reads this whole-space frontier and (e, n)
  // summed over ranks already; the hops after it exchange as with cnt
  void spec_enqueue(int32_t first, const unsigned long long* e, const unsigned long long* n, int32_t hop0,
                    const unsigned long long* cnt = nullptr, const uint32_t* fb_first = nullptr) {
    spec.clear();
    if (!spec_ok) return;
    unsigned long long* const SPd = K.d + kSpecBase;
    // the blocks start at zero (query start); a second chain in one query reuses them
    if (spec_blocks_used) {
      clean_shards();
      NBG_HIP(hipMemsetAsync(SPd, 0, kSpecWords * kMaxSpec * 8, c.stream));
    }
    spec_blocks_used = true;
    if (ks > 1) shards_dirty = true;
    const uint32_t* in = bitsA;
    uint32_t* outb = bitsB;
    const unsigned long long* pg = nullptr;
    unsigned long long* last_blk = nullptr;
    for (int32_t st = first; st <= s.steps && spec.size() < size_t(kMaxSpec); st++) {
      const bool fin = st == s.steps;
      if (fin && !fin_spec) break;
      unsigned long long* blk = SPd + kSpecWords * spec.size();
      // the hop's first pass evaluates its gate (GateIn) and publishes it at kSpecGate
      GateIn gi;
      gi.e = e, gi.n = n, gi.pg = pg, gi.thr = spec_thr;
      gi.shards = ks;  // (several ranks: ks = 1)
      const int32_t hop = hop0 + int32_t(spec.size());
      // several ranks: the frontier bitmaps of every rank (the exchange runs whatever the gate
      // says: every rank enqueued it)
      const uint32_t* fb;
      if (fb_first && spec.empty()) {
        fb = fb_first;
      } else if (cnt) {
        unsigned long long* all = c.ws_piggy.as<unsigned long long>() + spec.size() * size_t(c.world) * 2;
        fb = global_bits_cnt(c, in, cnt, all);
        gi.e = gi.n = nullptr;
        gi.all = all;
        gi.world = c.world;
      } else {
        fb = global_bits(c, in);
      }
      BuLaunch L = timed_bu(hop, [&] {
        BuLaunch l;
        if (!fin) {
          l = launch_bu_lean(c, es, fb, outb, es.odeg.as<uint32_t>(), PK_NONE, no_fp, -1, blk, true, blk + kSpecGate,
                             gi, true, ks);
        } else {
          FastArgs tfp = fp;
          if (fpk.kind == PK_FAST) tfp.data = es.tr.props[size_t(fpk.col)].data.p;
          l = launch_bu_lean(c, es, fb, outb, nullptr, fpk.kind, tfp, fpk.kind == PK_FAST ? fpk.col : -1, blk, true,
                             blk + kSpecGate, gi, true, ks);
          void* vout = vid_block(spec_vids, spec_hvids);
          launch_bits_vids(c, outb, es.tr.n_rows, lo, vout, blk + kSpecRows, blk + kSpecGate);
        }
        NBG_HIP(hipGetLastError());
        return l;
      });
      spec.push_back(Spec{hop, fin, std::move(L)});
      e = blk + kHopDegSum;
      n = blk + kHopFound;
      last_blk = fin ? nullptr : blk;
      if (cnt || fb_first) {
        cnt = blk;  // the next hop's exchange carries this hop's (n, e)
      } else if (multi && !fin) {
        dev_allsum(c, blk, {kHopFound, kHopDegSum}, blk + kSpecSumN);
        e = blk + kSpecSumE;
        n = blk + kSpecSumN;
      }
      pg = blk + kSpecGate;
      const uint32_t* t = in;
      in = outb;
      outb = const_cast<uint32_t*>(t);
    }
    // (piggy) a chain ending on a non-final hop: its global counts for the host
    if (cnt && last_blk) dev_allsum(c, last_blk, {kHopFound, kHopDegSum}, last_blk + kSpecLastN);
  }
  // several ranks: the global (n, e) of speculated hop j after the fetch -- piggy: published by
  // hop j + 1's gate (its block's kSpecSumN / kSpecSumE) or, for the chain's last hop, at
  // kSpecLastN / kSpecLastE; else its own block's kSpecSumN / kSpecSumE
  void spec_global(size_t j, unsigned long long& ng, unsigned long long& eg) const {
    const unsigned long long* hh = K.h + kSpecBase + kSpecWords * j;
    if (!piggy_used) {
      ng = hh[kSpecSumN], eg = hh[kSpecSumE];
    } else if (j + 1 < spec.size()) {
      ng = hh[kSpecWords + kSpecSumN], eg = hh[kSpecWords + kSpecSumE];
    } else {
      ng = hh[kSpecLastN], eg = hh[kSpecLastE];
    }
  }
  // the words a fetch behind an enqueued chain reads (base: without one)
  int spec_words(int base) const { return spec.empty() ? base : kSpecBase + kSpecWords * int(spec.size()); }
  // (the device work ends at the fetch when the speculated final hop runs: ev[1] ahead of it)
  hipEvent_t spec_final_event() const { return !spec.empty() && spec.back().final && tot_ev ? c.ev[1] : nullptr; }
  // after the fetch: record the hops that ran, as hop_bottom_up does; stops at the first gate
  // that was 0 (its timings dropped).  Returns the steps consumed; fin_done when the final step
  // ran (its block copied to fin_h)
  int32_t spec_replay() {
    int32_t used = 0;
    for (size_t j = 0; j < spec.size(); j++) {
      const unsigned long long* hh = K.h + kSpecBase + kSpecWords * j;
      if (hh[kSpecGate] == 0) {
        const int32_t cut = spec[j].hop;
        c.tpend.erase(std::remove_if(c.tpend.begin(), c.tpend.end(),
                                     [cut](const Ctx::PendingTime& p) { return p.hop >= cut; }),
                      c.tpend.end());
        break;
      }
      c.timing.spec_hops++;
      if (spec[j].final) {
        std::copy(hh, hh + kSpecWords, fin_h);
        fin_L = spec[j].L;
        fin_done = true;
        break;
      }
      c.timing.steps_run++;
      c.timing.edges_scanned += uint64_t(E);
      record_bu_hop(hh, spec[j].L);
      unsigned long long ng = hh[kHopFound], eg = hh[kHopDegSum];
      if (multi) spec_global(j, ng, eg);
      adopt_bu(hh, -1, int64_t(ng), int64_t(eg));
      used++;
      if (nset_global == 0) break;  // the caller returns the empty result
    }
    spec.clear();
    return used;
  }

  // hop 1 of a small start set: top-down from k_starts_small's list (nF = ns bounds it),
  // compaction, then one round trip for the start counts and the next frontier's together.
  // false: every start lacks out-edges (the empty result)
  bool hop1_small() {
    frontier_args();
    const int64_t e_bound = std::max<int64_t>(1, max_odeg1 >= 0 ? ns * max_odeg1 : csr1->nnz);
    ExpandArgs a1 = a;
    if (rep1) a1.row_ptr = csr1->row_ptr.as<int64_t>(), a1.col = csr1->col.as<int32_t>(), a1.lo = 0;
    // (the tile-row table: written by k_starts_small)
    launch_expand<EXP_MARK>(c, a1, PK_NONE, no_fp, nullptr, env, std::min<int64_t>(e_bound, csr1->nnz + 1), true);
    cur ^= 1;
    F = c.ws_front[cur].as<int32_t>();
    const bool lazy = bu_ok && c.opt("compact_list", 0) == 0;
    // (the counter block is zero: k_starts_small cleared it)
    if (rep1) {
      // the whole-space frontier and its counts (the same on every rank), plus this rank's share
      // (kCntOwnKept, kCntOwnDegSum) and its owned slice in bitsA (for a host-chosen top-down hop
      // 2).  (Block partials + a reduce launch instead of the block atomics measured the same:
      // 0.4255 vs 0.4243 ms a one-rank RCCL query, profiles/r13b_*)
      launch_compact(c, map, 0, c.n_global, csr1->row_ptr.as<int64_t>(), csr1->row_ok.as<uint8_t>(), 1, nullptr,
                     c.ws_bits_rep1.as<uint16_t>(), K.d, es.rep_odeg.as<uint32_t>(), true, 1, lo, hi,
                     reinterpret_cast<uint16_t*>(bitsA));
    } else if (multi && lazy && es.odeg.p) {
      // several ranks: every owner ORs the marks it receives straight into its frontier bitmap
      exchange_marks(c, map, bitsA, es.odeg.as<uint32_t>(), K.d + kCntSet);
    } else {
      exchange_marks(c, map);  // several ranks: every owner receives the marks of its vertices
      launch_compact(c, map, lo, n_own, row_ptr, row_ok, 1, lazy ? nullptr : F, reinterpret_cast<uint16_t*>(bitsA),
                     K.d, es.odeg.as<uint32_t>(), true, ks, 0, -1, nullptr, map_bound);
      if (ks > 1) shards_dirty = true;
    }
    // several ranks: the counts over ranks -- piggy: carried by the first speculated hop's
    // frontier exchange (its gate publishes them); else found, next out-degree sum and hop-1
    // entries summed into [kCntGlobal, kCntGlobal + 3)
    piggy_used = multi && spec_ok && (rep1 || c.opt("comm_piggy", 1) != 0);
    if (multi && !piggy_used) dev_allsum(c, K.d, {kCntSet, kCntDegSum, kCntStartsE}, K.d + kCntGlobal);
    if (rep1)
      spec_enqueue(2, K.d + kCntDegSum, K.d + kCntSet, c.timing.n_hops + 1, nullptr, c.ws_bits_rep1.as<uint32_t>());
    else
      spec_enqueue(2, K.d + (multi ? kCntGlobal + 1 : kCntDegSum), K.d + (multi ? kCntGlobal : kCntSet),
                   c.timing.n_hops + 1, piggy_used ? K.d + kCntSet : nullptr);  // (hop 1: below)
    if (piggy_used && spec.empty()) {  // nothing speculated (steps == 2 without the final): sum here
      piggy_used = false;
      if (!rep1) dev_allsum(c, K.d, {kCntSet, kCntDegSum, kCntStartsE}, K.d + kCntGlobal);
    }
    fetch_counters(c, K.d, spec_words(multi ? kCntGlobal + 4 : kCntStartsE + 1), K.h, spec_final_event(), ks);
    const int64_t nF1 = int64_t(K.h[kCntStartsN]), E1 = int64_t(K.h[kCntStartsE]);
    if (!s.distinct) hop1_scanned = int64_t(K.h[kCntHop1Rows]);
    // (go_rep1: every rank ran the whole hop; rank 0 counts it, so the ranks' sum is the hop's)
    if (!rep1 || c.rank == 0) c.timing.edges_scanned += uint64_t(hop1_scanned >= 0 ? hop1_scanned : E1);
    if (E1 > 0) c.timing.expand_bytes += expand_bytes(nF1, E1, 0, EXP_MARK);
    record_td_hop(false, 0.0, nF1, E1);
    // hop 1's entries over ranks (go_rep1: whole-space counts, already the sums)
    int64_t E1g = E1;
    if (multi && !rep1)  // (piggy: no marks anywhere iff no start has out-edges: the empty result either way)
      E1g = int64_t(piggy_used ? K.h[kSpecBase + kSpecSumN] : K.h[kCntGlobal + 2]);
    if (E1g == 0) return false;
    adopt_compaction(lazy, rep1);
    return true;
  }

  // a host-chosen bottom-up hop: frontier bitmap in, next frontier bitmap out
  void hop_bottom_up(int32_t step) {
    if (rev) return hop_rev_pull();
    const uint32_t* fb = global_bits(c, bitsA);
    const BuLaunch L = timed_bu(c.timing.n_hops, [&] {
      return launch_bu_lean(c, es, fb, bitsB, es.odeg.as<uint32_t>(), PK_NONE, no_fp, -1, K.d, step > 1);
    });
    hop_words_stale = true;
    if (multi) dev_allsum(c, K.d, {kHopFound, kHopDegSum}, K.d + kCntGlobal);
    fetch_counters(c, K.d, multi ? kCntGlobal + 2 : kHopWords, K.h);
    record_bu_hop(K.h, L);
    // one rank: the found rows the two passes counted are the new bitmap's population (every
    // found row sets one bit; pending rows are disjoint from the first pass's found rows), so
    // ensure_list needs no round trip; several ranks: the local population is read back
    if (multi) adopt_bu(K.h, -1, int64_t(K.h[kCntGlobal]), int64_t(K.h[kCntGlobal + 1]));
    else adopt_bu(K.h, int64_t(K.h[kHopFound]), int64_t(K.h[kHopFound]), int64_t(K.h[kHopDegSum]));
  }

  // REVERSELY: a pull hop (k_rev_pull over the out rows): frontier bitmap in, next frontier bitmap
  // out, one counter fetch.  final (DISTINCT _dst): every found row is kept and its vid written to
  // vout (launch_bits_vids, as final_distinct_dst's bottom-up branch does); returns the row count.
  // The hop's sums land sharded at [kCntUpto, kCntUpto + 5), the output count at kCntList.
  int64_t rev_pull(bool final, void* vout) {
    const uint32_t* fb = global_bits(c, bitsA);
    NBG_HIP(hipMemsetAsync(K.d, 0, kShardStride * size_t(ks) * 8, c.stream));
    if (ks > 1) shards_dirty = true;
    hop_words_stale = false;  // (the memset cleared the block)
    const int64_t rows = std::min<int64_t>(n_own, es.out.n_rows);
    const size_t ia = timing_event(c);
    launch_rev_pull(c, es, rows, n_own, fb, final ? nullptr : D.deg, reinterpret_cast<unsigned long long*>(bitsB),
                    K.d + kCntUpto, ks);
    NBG_HIP(hipGetLastError());
    const size_t ik = timing_event(c);
    if (final) {
      launch_bits_vids(c, bitsB, n_own, lo, vout, K.d + kCntList, nullptr);
      NBG_HIP(hipGetLastError());
    }
    const size_t ib = final ? timing_event(c) : ik;
    c.tpend.push_back(Ctx::PendingTime{ia, ib, c.timing.n_hops, 0});
    c.tpend.push_back(Ctx::PendingTime{ia, ik, c.timing.n_hops, 1});
    if (multi && !final) dev_allsum(c, K.d, {kCntUpto, kCntUpto + 1}, K.d + kCntGlobal);
    fetch_counters(c, K.d, kCntUpto + 5, K.h, nullptr, ks);
    const unsigned long long* h = K.h + kCntUpto;
    const int64_t n_out = final ? int64_t(K.h[kCntList]) : 0;
    c.timing.expand_launches++;
    c.timing.bu_steps++;
    // the byte model: a row_ptr pair (+ the row_ok byte) per owned row, 4 B per entry
    // read, the in-degree of every found row (non-final), the next word per 64 rows; the frontier
    // words are gathered (not counted: they stay in cache); final: + the output (next bits once,
    // vid_of read + vid written)
    const uint64_t kb = uint64_t(rows) * (8 + (es.out.row_ok.p ? 1 : 0)) + h[3] * 4 + (final ? 0 : h[0] * 4) +
                        uint64_t(n_own) / 8;
    c.timing.expand_bytes += kb + (final ? uint64_t(n_own) / 8 + uint64_t(n_out) * 16 : 0);
    const unsigned long long hs[8] = {h[0], h[1], 0, h[4], h[3], 0, 0, 0};
    c.timing.hop(6, final, 0.0, hs, 0.0, kb);
    c.timing.name_last_hop("nbg::k_rev_pull", "", final ? "nbg::k_bits_compact<1, 8, 1>" : nullptr);
    return n_out;
  }
  void hop_rev_pull() {
    rev_pull(false, nullptr);
    const unsigned long long* h = K.h + kCntUpto;
    std::swap(bitsA, bitsB);
    have_list = false;
    list_n = int64_t(h[2]);  // the kept rows are the new bitmap's population
    off_ready = false;
    E = E_known = int64_t(h[1]);
    nset_global = multi ? int64_t(K.h[kCntGlobal]) : int64_t(h[0]);
    Eg = multi ? int64_t(K.h[kCntGlobal + 1]) : E;
  }

  // the frontier list and its degree scan as the expansion's arguments
  void frontier_args() {
    a.F = F;
    a.nF = nF;
    a.off = c.ws_off.as<int64_t>();
  }
  // a top-down hop's statistics (frontier entries, edges, rows out)
  void record_td_hop(bool final, double ms, int64_t n, int64_t e, int64_t rows_out = 0) {
    const unsigned long long hs[8] = {(unsigned long long)n, (unsigned long long)e, uint64_t(rows_out), 0, 0, 0, 0, 0};
    c.timing.hop(0, final, ms, hs);
  }
  // a top-down expansion into the byte map, the marks exchanged to their owners; the final one
  // evaluates the WHERE, the others carry the multi-step roots along
  void expand_marks(bool final) {
    ensure_off();
    frontier_args();
    const double ms0 = c.timing.expand_ms;
    const bool roots = multi_root && !final;
    if (roots) {
      NBG_HIP(hipMemsetAsync(root_buf[root_cur ^ 1].p, 0x7f, size_t(c.n_global + 1) * 4, c.stream));
      a.root_cur = root_buf[root_cur].as<int32_t>();
      a.root_next = root_buf[root_cur ^ 1].as<int32_t>();
    }
    if (E > 0) {
      if (final) launch_expand<EXP_MARK>(c, a, fpk.kind, fp, dprog.as<Program>(), env, E);
      else launch_expand<EXP_MARK>(c, a, PK_NONE, no_fp, nullptr, env, E);
      c.timing.expand_bytes += expand_bytes(nF, E, final ? pred_w() : 0, EXP_MARK);
    }
    if (roots) {
      exchange_roots(c, a.root_next);
      root_cur ^= 1;
      a.root_cur = nullptr;
      a.root_next = nullptr;
    }
    record_td_hop(final, c.timing.expand_ms - ms0, nF, E);
    exchange_marks(c, map);
  }

  // a top-down hop: expansion into the byte map, compaction to the next frontier, and the
  // remaining hops speculated behind it
  void hop_top_down(int32_t step) {
    expand_marks(false);
    // next frontier = set of dsts (P12): compact, drop rows without out-edges, bitmap too
    cur ^= 1;
    F = c.ws_front[cur].as<int32_t>();
    NBG_HIP(hipMemsetAsync(K.d, 0, 32, c.stream));
    // when the next hop may go bottom-up it reads the bitmap alone: the list is left to
    // ensure_list (option compact_list = 1 always writes it here).  One rank only: this
    // bitmap is slice-relative, ensure_list's input is the bottom-up's global-indexed one
    const bool lazy = bu_ok && !multi_root && c.opt("compact_list", 0) == 0;
    launch_compact(c, map, lo, n_own, row_ptr, row_ok, 1, lazy ? nullptr : F, reinterpret_cast<uint16_t*>(bitsA),
                   K.d, D.deg, false, 1, 0, -1, nullptr, map_bound);
    piggy_used = multi && lazy && spec_ok && c.opt("comm_piggy", 1) != 0;
    if (multi && !piggy_used) dev_allsum(c, K.d, {kCntSet, kCntDegSum}, K.d + kCntGlobal);
    if (lazy)
      spec_enqueue(step + 1, K.d + (multi ? kCntGlobal + 1 : kCntDegSum), K.d + (multi ? kCntGlobal : kCntSet),
                   c.timing.n_hops, piggy_used ? K.d + kCntSet : nullptr);
    if (piggy_used && spec.empty()) {
      piggy_used = false;
      dev_allsum(c, K.d, {kCntSet, kCntDegSum}, K.d + kCntGlobal);
    }
    fetch_counters(c, K.d, spec_words(multi ? kCntGlobal + 2 : kCntOwnKept + 1), K.h, spec_final_event(), ks);
    adopt_compaction(lazy, false);
  }

  int pred_w() const { return fpk.kind == PK_FAST ? fp.width : 0; }
  // WHERE / YIELD evaluation errors of the final step (summed over ranks): the reference fails
  // the query on any row's error
  void check_eval_errors(int word, const char* what) {
    if (multi) dev_allsum(c, K.d, {word}, K.d + kCntGlobal);
    fetch_counters(c, K.d, multi ? kCntGlobal + 1 : kCntYieldErr + 1, K.h);
    if (K.h[multi ? kCntGlobal : word]) throw Error(NBG_E_EVAL, what);
  }

  // the final step begins: the deferred compile error, the programs' upload, the result's owner
  void begin_final() {
    if (multi_root) {
      env.in_root = root_buf[root_cur].as<int32_t>();
      env.in_root_tab = root_tab.as<int32_t>();
    }
    if (deferred != NBG_OK) throw Error(deferred, deferred_msg);
    // DISTINCT _dst reads no YIELD program (and the WHERE program only on the VM path)
    if (!dprog.p && (fpk.kind == PK_VM || (!default_yield && !(s.distinct && lone_dst)))) {
      dprog.alloc(sizeof(Program) * (yields.size() + 1));
      c.h2d(dprog.p, &where, sizeof(Program));
      c.h2d(dprog.as<Program>() + 1, yields.data(), sizeof(Program) * yields.size());
    }
    c.timing.edges_scanned += uint64_t(E);
    rows = std::make_unique<HostRows>();
    slen.resize(yields.size());
  }

  // DISTINCT e._dst: mark surviving dsts, compact the whole vertex space (no deg filter).
  // Bottom-up only when the predicate cannot error (pred_runs_bottom_up).
  void final_distinct_dst() {
    const int pk = fpk.kind;
    const bool bu = pred_bu && want_bu(Eg);
    DevBuf vids;
    HostBuf hvids;
    if (fin_done) {
      // the speculated final hop ran (spec_replay): its counters, rows and kernel names
      vids = std::move(spec_vids);
      hvids = std::move(spec_hvids);
      nrows = int64_t(fin_h[kSpecRows]);
      record_bu_hop(fin_h, fin_L, true, nrows);
    } else if (bu && rev) {
      vids.alloc(size_t(c.n_global + 64) * 8);
      nrows = rev_pull(true, vids.p);
    } else if (bu) {
      FastArgs tfp = fp;
      if (pk == PK_FAST) tfp.data = es.tr.props[size_t(fpk.col)].data.p;
      NBG_HIP(hipMemsetAsync(K.d, 0, 8, c.stream));
      const uint32_t* fb = global_bits(c, bitsA);
      const BuLaunch L = timed_bu(c.timing.n_hops, [&] {
        BuLaunch l = launch_bu_lean(c, es, fb, bitsB, nullptr, pk, tfp, pk == PK_FAST ? fpk.col : -1,
                                    K.d + kCntFinalHop, s.steps > 1 && !upto);
        void* vout = vid_block(vids, hvids);
        launch_bits_vids(c, bitsB, es.tr.n_rows, lo, vout, K.d + kCntList, nullptr);
        NBG_HIP(hipGetLastError());
        return l;
      });
      fetch_counters(c, K.d, kCntFinalHop + kHopWords, K.h);
      nrows = int64_t(K.h[kCntList]);
      record_bu_hop(K.h + kCntFinalHop, L, true, nrows);
    } else {
      vids.alloc(size_t(c.n_global + 64) * 8);
      // a host-chosen bottom-up hop before this one left its HopWord block in [0, kHopWords):
      // kHopEntries is this word (else it is still zero: nothing else writes it before here)
      if (hop_words_stale) NBG_HIP(hipMemsetAsync(K.d + kCntWhereErr, 0, 8, c.stream));
      hop_words_stale = false;
      expand_marks(true);
      DevBuf lst;
      lst.alloc(size_t(n_own + 64) * 4);
      NBG_HIP(hipMemsetAsync(K.d, 0, kCntRows * 8, c.stream));  // keep the eval-error counter (kCntWhereErr)
      launch_compact(c, map, lo, n_own, row_ptr, nullptr, 0, lst.as<int32_t>(), nullptr, K.d);
      check_eval_errors(kCntWhereErr, "WHERE evaluation failed");
      nrows = int64_t(K.h[kCntList]);
      if (nrows) launch_local_to_vid(c, lst.as<int32_t>(), nrows, lo, vids.as<int64_t>());
    }
    HostRows* h = rows.get();
    h->types.push_back(NBG_T_VID);
    if (hvids.p) {  // already on the host (host_direct)
      host_cols[h->dev.size()] = true;
      h->hpin.push_back(std::move(hvids));
    }
    h->dev.push_back(std::move(vids));
  }

  // rows (src, edge) passing WHERE; a lone YIELD _dst (the default) is written directly as
  // vids by the expansion (no row list, no materialisation pass)
  void final_rows() {
    HostRows* h = rows.get();
    const int pk = fpk.kind;
    ensure_off();
    frontier_args();
    DevBuf fused;
    int64_t* rows_edge = nullptr;
    int32_t* rows_src = nullptr;
    if (lone_dst) {
      fused.alloc(size_t(E + 64) * 8);
      a.out_vid = fused.as<int64_t>();
      a.vid_of = c.vid_of.as<int64_t>();
      a.col_vid = csr.col_vid.as<int64_t>();
    } else {
      c.ws_rows.ensure(size_t(E + 64) * 12);
      rows_edge = c.ws_rows.as<int64_t>();
      rows_src = reinterpret_cast<int32_t*>(rows_edge + E + 32);
    }
    a.rows_edge = rows_edge;
    a.rows_src = rows_src;
    a.rows_cnt = K.d + kCntRows;
    NBG_HIP(hipMemsetAsync(K.d, 0, (kCntYieldErr + 1) * 8, c.stream));
    const double ms0 = c.timing.expand_ms;
    if (E > 0) launch_expand<EXP_ROWS>(c, a, pk, fp, dprog.as<Program>(), env, E);
    check_eval_errors(kCntWhereErr, "WHERE evaluation failed");
    const bool direct = lone_dst && pk == PK_NONE;  // every edge is a row, written at its index
    nrows = direct ? E : int64_t(K.h[kCntRows]);
    // the hop's bytes: frontier entries + per edge the col (+ predicate);
    // per row its 8 B vid write and where the vid comes from: the 8 B dst-vid column read
    // instead of col (direct rows), else an 8 B vid_of gather behind the col read (a 4 B
    // (src) + 8 B (edge) row pair without the fused _dst)
    if (E > 0) {
      if (direct && csr.col_vid.p)
        c.timing.expand_bytes += uint64_t(nF) * 28 + uint64_t(E) * 16;
      else
        c.timing.expand_bytes += expand_bytes(nF, E, pred_w(), EXP_ROWS) + uint64_t(nrows) * (lone_dst ? 16 : 12);
    }
    record_td_hop(true, c.timing.expand_ms - ms0, nF, E, nrows);
    YieldArgs ya{};
    ya.ncols = int32_t(yields.size());
    for (auto& p : yields) {
      int32_t t = p.result_type;
      DevBuf b;
      if (lone_dst) b = std::move(fused);
      else b.alloc(size_t(nrows + 1) * (t == VT_BOOL ? 1 : 8));
      const size_t k = h->types.size();
      if (t == VT_STR) slen[k].alloc(size_t(nrows + 1) * 8);
      ya.cols[k] = ColOut{b.p, t, slen[k].as<int64_t>()};
      h->types.push_back(result_type(t));
      h->dev.push_back(std::move(b));
    }
    if (nrows && !lone_dst) {
      if (default_yield) launch_yield_dst(c, rows_edge, nrows, csr.col.as<int32_t>(), h->dev[0].as<int64_t>());
      else launch_materialize(c, rows_src, rows_edge, nrows, dprog.as<Program>() + 1, ya, env, lo, K.d + kCntYieldErr);
      NBG_HIP(hipGetLastError());
    }
    // (the fused _dst rows evaluate nothing: no error count to read)
    if (!lone_dst) check_eval_errors(kCntYieldErr, "YIELD evaluation failed");
    if (s.distinct && c.sharded) nrows = shuffle_rows(c, ya, h->dev, nrows);
    if (s.distinct && nrows) nrows = dedup_rows(c, ya, h->dev, slen, nrows);
  }

  // STRING columns: (address, length) rows -> packed bytes + n+1 offsets; then the stream is
  // drained where the hand-out needs it.  Returns per column the index of its offsets in
  // rows->dev (-1: not a STRING)
  std::vector<int64_t> pack_strings() {
    HostRows* h = rows.get();
    const size_t ncols_out = h->types.size();
    std::vector<int64_t> soff_dev_idx(ncols_out, -1);
    for (size_t cc = 0; cc < ncols_out; cc++) {
      if (h->types[cc] != NBG_T_STRING) continue;
      DevBuf off, bytes;
      NBG_HIP(hipMemsetAsync(slen[cc].as<int64_t>() + nrows, 0, 8, c.stream));
      int64_t total = 0;
      str_offsets(c, slen[cc].as<int64_t>(), nrows, off, &total);
      host_sync(c);
      str_pack(c, h->dev[cc].as<int64_t>(), off.as<int64_t>(), nrows, total, bytes);
      h->dev[cc] = std::move(bytes);
      soff_dev_idx[cc] = int64_t(h->dev.size());
      h->dev.push_back(std::move(off));
    }
    // the result is complete before it is handed out: a host copy waits for its own copies
    // (hand_out); device columns need the stream drained, which the counter fetch of a speculated
    // final hop already saw (nothing was enqueued after it)
    // (STRING columns and very large ones are copied with the blocking hipMemcpy, which does not
    // order behind the engine stream: drained first)
    bool drain = s.keep_on_device ? !fin_done : false;
    for (size_t cc = 0; cc < ncols_out && !s.keep_on_device; cc++) {
      const size_t w = h->types[cc] == NBG_T_BOOL ? 1 : 8;
      drain |= soff_dev_idx[cc] >= 0 ||
               size_t(nrows) * w + 8 > size_t(std::max<int64_t>(0, c.opt("host_pinned_mb", 4096))) << 20;
    }
    if (drain && hipStreamQuery(c.stream) != hipSuccess) host_sync(c);
    if (s.keep_on_device || drain) c.host_stage_used = 0;  // the query's input copies have completed
    return soff_dev_idx;
  }

  // the columns' pointers for the caller: device blocks (keep_on_device), the pinned block the
  // output kernel wrote (host_direct), or host copies
  void fill_columns(const std::vector<int64_t>& soff_dev_idx) {
    HostRows* h = rows.get();
    const bool on_dev = s.keep_on_device != 0;
    for (size_t cc = 0; cc < soff_dev_idx.size(); cc++) {
      if (soff_dev_idx[cc] >= 0) {  // STRING
        DevBuf& off = h->dev[size_t(soff_dev_idx[cc])];
        if (on_dev) {
          h->cols.push_back(h->dev[cc].p);
          h->str_off.push_back(off.as<int64_t>());
        } else {
          h->host_off.emplace_back(size_t(nrows) + 1);
          NBG_HIP(hipMemcpy(h->host_off.back().data(), off.p, size_t(nrows + 1) * 8, hipMemcpyDeviceToHost));
          const size_t total = size_t(h->host_off.back()[size_t(nrows)]);
          h->host.emplace_back(total + 8);
          if (total) NBG_HIP(hipMemcpy(h->host.back().data(), h->dev[cc].p, total, hipMemcpyDeviceToHost));
          h->cols.push_back(h->host.back().data());
          h->str_off.push_back(h->host_off.back().data());
        }
        continue;
      }
      h->str_off.push_back(nullptr);
      if (host_cols.count(cc)) {  // written into pinned host memory by the output kernel
        // the block spans the vertex space (n_global vids): a result far smaller than it is copied
        // into a right-sized pinned block, so a result the caller keeps pins about its own size (the
        // large block returns to the context's pinned cache, whose cap bounds what stays held)
        HostBuf& big = h->hpin.back();
        const size_t need = size_t(nrows) * 8 + 8;
        if (need * 4 < big.bytes && need <= (size_t(64) << 20)) {
          HostBuf small;
          small.alloc(c.host_pool, need);
          if (nrows) memcpy(small.p, big.p, size_t(nrows) * 8);
          big = std::move(small);
        }
        h->cols.push_back(h->hpin.back().p);
      } else if (on_dev) {
        h->cols.push_back(h->dev[cc].p);
      } else {
        size_t w = h->types[cc] == NBG_T_BOOL ? 1 : 8;
        const size_t bytes = size_t(nrows) * w + 8;
        if (bytes <= size_t(std::max<int64_t>(0, c.opt("host_pinned_mb", 4096))) << 20) {
          h->hpin.emplace_back();
          if (h->hpin.size() == 1) host_pool_cap(c);
          h->hpin.back().alloc(c.host_pool, bytes);
          if (nrows)
            NBG_HIP(hipMemcpyAsync(h->hpin.back().p, h->dev[cc].p, size_t(nrows) * w, hipMemcpyDeviceToHost, c.stream));
          h->cols.push_back(h->hpin.back().p);
        } else {  // very large results (RMAT-28's 21 GB of rows): pageable, through the driver
          h->host.emplace_back(bytes);
          if (nrows) NBG_HIP(hipMemcpy(h->host.back().data(), h->dev[cc].p, size_t(nrows) * w, hipMemcpyDeviceToHost));
          h->cols.push_back(h->host.back().data());
        }
      }
    }
    if (!on_dev) {
      host_sync(c);  // the pinned copies above (and with them the whole query)
      c.host_stage_used = 0;
      h->dev.clear();
    }
  }
  // hand the columns out (a failed pinned allocation or copy frees the rows and rethrows)
  int32_t hand_out(const std::vector<int64_t>& soff_dev_idx) {
    try {
      fill_columns(soff_dev_idx);
    } catch (...) {
      // no copy may still target a block freed with the rows (their owner frees them after this)
      (void)hipStreamSynchronize(c.stream);
      throw;
    }
    fill_rows(out, std::move(rows), nrows, s.keep_on_device != 0);
    out->edges_scanned = c.timing.edges_scanned;
    return NBG_OK;
  }

  // ---- GO UPTO N STEPS (DESIGN.md divergence 7): the rows of GO 1 .. N STEPS together ----
  // Host-driven, no speculation chain, no fast1 / rep1.  Called behind first_degrees with a
  // non-empty start list.  GO 1 STEPS reports a deferred compile error at its only step, so here
  // it comes before any hop.
  int32_t run_upto() {
    if (deferred != NBG_OK) throw Error(deferred, deferred_msg);
    return s.distinct ? upto_distinct() : upto_rows();
  }
  // the query's end behind the final step(s): ev[1] ends the device time (read when asked for)
  int32_t upto_hand_out() {
    if (tot_ev) hipEventRecord(c.ev[1], c.stream);
    c.total_pending = tot_ev;
    return hand_out(pack_strings());
  }

  // DISTINCT: the result depends only on the set of vertices that are in some step's frontier,
  // U = starts + everything reached within N - 1 hops (with out-edges), so a visited-pruned BFS
  // builds U expanding each vertex once (levels B_k) and ONE final step runs over U.
  int32_t upto_distinct() {
    if (!D.deg) throw Error(NBG_E_STATE, "GO UPTO: the snapshot has no out-degree array");
    const size_t bm = size_t(map_bytes(c) / 8 + 64);
    c.ws_vis.ensure(2 * bm);
    auto* vis = c.ws_vis.as<unsigned long long>();
    auto* uni = reinterpret_cast<unsigned long long*>(c.ws_vis.as<uint8_t>() + bm);
    // B_1: the frontier bitmap resolve_starts left (the distinct starts with out-edges; a start
    // without them yields nothing at any step, and reaching it again is harmless)
    const size_t wb = size_t((n_own + 63) / 64) * 8;
    NBG_HIP(hipMemcpyAsync(vis, bitsA, wb, hipMemcpyDeviceToDevice, c.stream));
    NBG_HIP(hipMemcpyAsync(uni, bitsA, wb, hipMemcpyDeviceToDevice, c.stream));
    const uint32_t* odeg = D.deg;  // (REVERSELY: in-degrees)
    unsigned long long* const S = K.d + kCntUpto;
    // a level's successor is certainly expanded top-down: the claim writes it as a list too
    const bool td_certain = rev || !bu_ok || bu_force < 0;  // (REVERSELY: never k_upto_bu, which reads es.tr)
    const int64_t n_scan = std::min<int64_t>(n_own, es.bu_in_tiles * 128);  // rows with an in-edge lie below
    int64_t bn = nF;                     // |B_k| on this rank
    int64_t un = nF, ue = E, ueg = Eg;   // |U|, outdeg(U) on this rank, outdeg(U) over ranks
    for (int32_t step = 1; step < s.steps && Eg > 0; step++) {
      c.timing.steps_run++;
      c.timing.edges_scanned += uint64_t(E);
      c.timing.expand_launches++;
      const bool bu = want_bu(Eg);  // (global: every rank takes the same branch)
      if (!bu) ensure_off();  // (may count the list at kCntList: ahead of the hop's zeroing)
      NBG_HIP(hipMemsetAsync(K.d, 0, kShardStride * size_t(ks) * 8, c.stream));  // the hop's sums and kCntList
      if (ks > 1) shards_dirty = true;
      int32_t* nl = nullptr;
      if (bu) {
        const uint32_t* fb = global_bits(c, bitsA);
        const size_t ia = timing_event(c);
        launch_upto_bu(c, es, n_own, n_scan, fb, odeg, vis, uni, reinterpret_cast<unsigned long long*>(bitsB), S, ks);
        NBG_HIP(hipGetLastError());
        c.tpend.push_back(Ctx::PendingTime{ia, timing_event(c), c.timing.n_hops, 0});
        c.timing.bu_steps++;
      } else {
        frontier_args();
        if (E > 0) {
          launch_expand<EXP_MARK>(c, a, PK_NONE, no_fp, nullptr, env, E);
          c.timing.expand_bytes += expand_bytes(nF, E, 0, EXP_MARK);
        }
        exchange_marks(c, map);  // several ranks: every owner receives the marks of its vertices
        if (td_certain) nl = c.ws_front[cur ^ 1].as<int32_t>();
        const size_t ia = timing_event(c);
        launch_upto_claim(c, map + lo, n_own, map_bound, odeg, vis, uni, reinterpret_cast<unsigned long long*>(bitsB), nl,
                          K.d + kCntList, S, ks);
        NBG_HIP(hipGetLastError());
        c.tpend.push_back(Ctx::PendingTime{ia, timing_event(c), c.timing.n_hops, 0});
      }
      if (multi) dev_allsum(c, K.d, {kCntUpto, kCntUpto + 1}, K.d + kCntGlobal);
      fetch_counters(c, K.d, kCntUpto + 4, K.h, nullptr, ks);
      const unsigned long long* h = K.h + kCntUpto;
      const int64_t read = bu ? int64_t(h[3]) : E;
      // bottom-up: 4 B per entry read, a row_ptr pair per open row (not counted: unknown), vis,
      // frontier and next words; claim: the mark bytes read, vis / uni / next words
      c.timing.expand_bytes += bu ? uint64_t(h[3]) * 4 + 3 * uint64_t(n_scan / 8) : uint64_t(map_bound) + 2 * uint64_t(n_own / 8);
      const unsigned long long hs[8] = {h[0], h[1], (unsigned long long)bn, (unsigned long long)read, 0, 0, 0, 0};
      c.timing.hop(bu ? 1 : 0, false, 0.0, hs);
      c.timing.name_last_hop(bu ? "nbg::k_upto_bu" : "nbg::k_upto_claim", bu ? "" : "nbg::k_expand");
      // the next level: the bitmap the kernel wrote (and the claim's list)
      std::swap(bitsA, bitsB);
      bn = int64_t(h[2]);
      E = E_known = int64_t(h[1]);
      Eg = multi ? int64_t(K.h[kCntGlobal + 1]) : E;
      off_ready = false;
      if (nl) {
        cur ^= 1;
        F = nl;
        nF = int64_t(K.h[kCntList]);
        have_list = true;
        list_n = -1;
      } else {
        have_list = false;
        list_n = bn;
      }
      un += bn, ue += E, ueg += Eg;
      if ((multi ? K.h[kCntGlobal] : h[0]) == 0) break;  // nothing new anywhere: U is complete
    }
    // ---- the final step over U.  U holds the starts, which need no in-edge: no consumer may
    // assume a hop's output here (launch_bu_lean's hop_front, map_bound on the frontier) ----
    c.timing.steps_run++;
    clean_shards();  // dense counters from here on
    bitsA = reinterpret_cast<uint32_t*>(uni);
    have_list = false;
    list_n = un;
    off_ready = false;
    E = E_known = ue;
    Eg = ueg;
    begin_final();
    if (lone_dst) final_distinct_dst();
    else final_rows();
    return upto_hand_out();
  }

  // Without DISTINCT multiplicity matters: the frontiers are the unpruned F_k of the existing
  // hops.  Each step's frontier first yields its rows (final_rows), then advances (one expansion
  // each; no step is re-run from the starts); the steps' columns stay on the device and are
  // concatenated at the end.  The general path: existing kernels, not a tuned one.
  int32_t upto_rows() {
    struct StepRows {
      std::vector<DevBuf> cols, slen;
      int64_t n = 0;
    };
    std::vector<StepRows> parts;
    for (int32_t step = 1; step <= s.steps && Eg > 0; step++) {
      c.timing.steps_run++;
      // step 1 rescans duplicate starts exactly as GO 1 STEPS does (k_list_starts); the advance
      // below uses the de-duplicated frontier
      const bool dup = step == 1 && hop1_scanned >= 0 && hop1_scanned != E;
      int32_t* const keepF = F;
      const int64_t keepN = nF, keepE = E;
      DevBuf dl;
      if (dup) {
        dl.alloc(size_t(ns + 64) * 4);
        NBG_HIP(hipMemsetAsync(K.d + kCntList, 0, 8, c.stream));
        launch_list_starts(c, d_sg, ns, lo, hi, row_ptr, row_ok, dl.as<int32_t>(), K.d + kCntList);
        NBG_HIP(hipGetLastError());
        fetch_counters(c, K.d, kCntList + 1, K.h);
        F = dl.as<int32_t>();
        nF = int64_t(K.h[kCntList]);
        E = E_known = hop1_scanned;  // the list's out-degree sum (k_starts_degree)
        off_ready = false;
      }
      begin_final();  // (counts the step's E entries as scanned)
      final_rows();
      StepRows sr;
      sr.cols = std::move(rows->dev);
      sr.slen = std::move(slen);
      sr.n = nrows;
      parts.push_back(std::move(sr));
      if (dup) {
        F = keepF, nF = keepN, E = E_known = keepE;
        off_ready = false;
      }
      if (step == s.steps) break;
      if (want_bu(Eg)) hop_bottom_up(step);
      else hop_top_down(step);
      if (nset_global == 0) break;  // the frontier died: the rows of the steps so far
    }
    if (parts.empty()) return finish_empty();  // no start has out-edges
    int64_t total = 0;
    for (auto& p : parts) total += p.n;
    rows = std::make_unique<HostRows>();
    slen.clear();
    slen.resize(yields.size());
    for (size_t k = 0; k < yields.size(); k++) {
      const int32_t t = yields[k].result_type;
      const size_t w = t == VT_BOOL ? 1 : 8;
      DevBuf b;
      b.alloc(size_t(total + 1) * w);
      if (t == VT_STR) slen[k].alloc(size_t(total + 1) * 8);
      int64_t at = 0;
      for (auto& p : parts) {
        if (p.n) {
          NBG_HIP(hipMemcpyAsync(b.as<uint8_t>() + size_t(at) * w, p.cols[k].p, size_t(p.n) * w, hipMemcpyDeviceToDevice,
                                 c.stream));
          if (t == VT_STR)
            NBG_HIP(hipMemcpyAsync(slen[k].as<int64_t>() + at, p.slen[k].p, size_t(p.n) * 8, hipMemcpyDeviceToDevice,
                                   c.stream));
        }
        at += p.n;
      }
      rows->types.push_back(result_type(t));
      rows->dev.push_back(std::move(b));
    }
    nrows = total;
    return upto_hand_out();
  }
};

}  // namespace

int32_t go_run(Ctx& c, const nbg_go_spec& s, nbg_rows* out) {
  PoolScope pool_scope(query_pool(c));
  if (!c.finalized) throw Error(NBG_E_STATE, "snapshot not finalized");
  if (s.steps < 1) throw Error(NBG_E_INVALID_ARG, "steps must be >= 1");
  if (s.upto != 0 && s.upto != 1) throw Error(NBG_E_INVALID_ARG, "upto must be 0 or 1");
  // edge_type < 0: GO ... OVER -edge_type REVERSELY, the convention of nbg_get_bound
  if (s.edge_type == 0 || s.edge_type == INT32_MIN) throw Error(NBG_E_INVALID_ARG, "edge_type must not be 0");
  auto it = c.edges.find(s.edge_type < 0 ? -s.edge_type : s.edge_type);
  if (it == c.edges.end()) throw Error(NBG_E_INVALID_ARG, "edge type not in snapshot");
  if (s.edge_type < 0 && !it->second.in.row_ptr.p)
    throw Error(NBG_E_UNSUPPORTED, "GO ... REVERSELY: the edge type has no in CSR");
  c.timing = Timing{};
  timing_reset(c);
  // per-hop event pairs (hop stats); bench.py's timed loop turns them off like a production
  // caller would, its statistics loop on
  c.hop_timing = c.opt("hop_timing", 1) != 0;
  if (c.host_stage_used) host_sync(c);  // a failed query's copies
  c.host_stage_used = 0;
  c.total_pending = false;
  GoQuery q(c, s, it->second, out);
  if (q.tot_ev) hipEventRecord(c.ev[0], c.stream);
  q.compile();
  q.resolve_starts();
  if (q.nset_global == 0) return q.finish_empty();
  q.bind_inputs();
  q.first_degrees();
  if (q.upto) return q.run_upto();
  for (int32_t step = 1; step < s.steps; step++) {
    c.timing.steps_run++;
    q.clean_shards();  // (the speculated hops' sums were fetched: dense counters from here on)
    if (q.fast1 && step == 1) {
      if (!q.hop1_small()) return q.finish_empty();  // every start lacks out-edges
    } else {
      c.timing.edges_scanned += uint64_t(step == 1 && q.hop1_scanned >= 0 ? q.hop1_scanned : q.E);
      if (q.Eg == 0) return q.finish_empty();  // every frontier vertex lacks out-edges
      if (q.want_bu(q.Eg)) q.hop_bottom_up(step);
      else q.hop_top_down(step);
    }
    if (q.nset_global == 0) return q.finish_empty();  // onEmptyInputs (GoExecutor.cpp:392-395)
    step += q.spec_replay();  // the speculated hops that ran behind this one
    if (q.nset_global == 0) return q.finish_empty();
    if (q.fin_done) break;
  }
  // ---- final step ----
  c.timing.steps_run++;
  if (!q.fin_done) q.clean_shards();
  q.begin_final();
  if (s.distinct && q.lone_dst) q.final_distinct_dst();
  else q.final_rows();
  // ev[1] ends the device time; not waited for here (resolve_total reads it when asked): a
  // speculated final hop recorded it ahead of its counter fetch, after which nothing was enqueued
  if (q.tot_ev && !q.fin_done) hipEventRecord(c.ev[1], c.stream);
  c.total_pending = q.tot_ev;
  return q.hand_out(q.pack_strings());
}

void free_rows_impl(void* impl) { delete static_cast<HostRows*>(impl); }

}  // namespace nbg
