/*
 * nebula_amd.h -- C ABI of the MI355X neighbour-expansion engine.
 *
 * This is the drop-in boundary for the reference's getBound / GO hot path (Nebula Graph
 * v1.0.0-beta).  Every entry point is plain C (pointers + sizes, no C++/torch types), so a
 * storaged/graphd built from the reference can bind it directly (see INTEGRATION.md for the
 * C++ operator shapes that wrap it).  Each function names the reference interface it replaces.
 *
 * Error convention: functions return 0 on success or a negative code.  Codes -1..-100 are the
 * reference's storage::cpp2::ErrorCode values (src/interface/storage.thrift:13-35); codes
 * <= -1000 are engine errors.  nbg_last_error() gives the message for the calling context.
 * All calls on one context are serialised internally (the reference's processors may call
 * from many RPC worker threads: QueryBaseProcessor.inl:407-423).
 */
#ifndef NEBULA_AMD_H_
#define NEBULA_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (storage.thrift:13-35 + engine range) -------------------------------- */
#define NBG_OK 0
#define NBG_E_LEADER_CHANGED (-11)
#define NBG_E_SPACE_NOT_FOUND (-13)
#define NBG_E_PART_NOT_FOUND (-14)
#define NBG_E_EDGE_PROP_NOT_FOUND (-21)
#define NBG_E_TAG_PROP_NOT_FOUND (-22)
#define NBG_E_IMPROPER_DATA_TYPE (-23)
#define NBG_E_INVALID_FILTER (-31)
#define NBG_E_UNKNOWN (-100)
#define NBG_E_DEVICE (-1000)      /* HIP runtime / kernel failure                          */
#define NBG_E_INVALID_ARG (-1001) /* bad argument (null pointer, unknown edge type, ...)   */
#define NBG_E_STATE (-1002)       /* call out of order (query before snapshot finalize)   */
#define NBG_E_UNSUPPORTED (-1003) /* expression / column shape the engine does not run    */
#define NBG_E_EVAL (-1004)        /* expression evaluation error at the final GO step
                                     (GoExecutor.cpp:754-758 fails the whole query)       */
#define NBG_E_COMM (-1005)        /* RCCL failure                                          */
#define NBG_E_NOMEM (-1006)       /* device allocation failed                              */

/* cpp2::SupportedType values (src/interface/common.thrift:30-46) */
#define NBG_T_BOOL 1
#define NBG_T_INT 2
#define NBG_T_VID 3
#define NBG_T_FLOAT 4
#define NBG_T_DOUBLE 5
#define NBG_T_STRING 6
#define NBG_T_TIMESTAMP 21

/* cpp2::PropOwner (storage.thrift:37-41) */
#define NBG_OWNER_SOURCE 1
#define NBG_OWNER_DEST 2
#define NBG_OWNER_EDGE 3

typedef struct nbg_ctx nbg_ctx;

/* ---- context ------------------------------------------------------------------------------
 * One context = one space on one GPU (one rank of `world_size`).  Replaces the storaged's
 * KVStore* + SchemaManager* pair handed to QueryBoundProcessor::instance
 * (src/storage/QueryBoundProcessor.h:23-28) and graphd's StorageClient for that space.
 * num_parts: the space's partition count (CreateSpaceProcessor.cpp:10-11); a vid lives in part
 * (uint64)vid % num_parts + 1 (StorageClient.cpp:10-11) and part p on rank p % world_size
 * (pickHosts, CreateSpaceProcessor.cpp:77-90).                                              */
nbg_ctx* nbg_ctx_create(int32_t device, int32_t num_parts, int32_t rank, int32_t world_size);
void nbg_ctx_destroy(nbg_ctx* ctx);
const char* nbg_last_error(const nbg_ctx* ctx);

/* Multi-GPU: RCCL communicator over xGMI.  Rank 0 calls nbg_comm_unique_id and the launcher
 * broadcasts the 128 bytes (e.g. via torch.distributed's store); every rank then calls
 * nbg_comm_init.  Replaces StorageClient::collectResponse's RPC scatter/gather
 * (src/storage/client/StorageClient.inl:74-159) with a per-step all-to-all.                 */
int32_t nbg_comm_unique_id(uint8_t out[128]);
int32_t nbg_comm_init(nbg_ctx* ctx, const uint8_t unique_id[128]);
/* Test transport: contexts of ONE process (one per rank, any device) with the same group_key
 * form a group whose collectives are device-to-device copies; the sharded algorithm then runs
 * unchanged with world_size ranks on a single GPU.  Each rank must call from its own thread. */
int32_t nbg_comm_init_local(nbg_ctx* ctx, int64_t group_key);
/* The context's communicator as the transport itself reports it: *ranks = ncclCommCount of
 * the RCCL communicator (the LocalComm group size; 1 without one), *transport = 0 none,
 * 1 RCCL, 2 LocalComm.  Lets a multi-GPU bench line show the rank count RCCL really formed.  */
int32_t nbg_comm_info(nbg_ctx* ctx, int32_t* ranks, int32_t* transport);

/* ABI version of this header's structs and signatures.  Caller-allocated structs (nbg_timing,
 * nbg_hop_stat, nbg_snapshot_info, nbg_go_spec, nbg_rows) change layout between versions: an
 * integration compares nbg_abi_version() with the NBG_ABI_VERSION it was built against and
 * refuses to run on a mismatch (INTEGRATION.md "ABI versioning").                          */
#define NBG_ABI_VERSION 7
int32_t nbg_abi_version(void);
/* sizeof of the caller-allocated structs as the library was built: 0 nbg_timing, 1
 * nbg_hop_stat, 2 nbg_snapshot_info, 3 nbg_go_spec, 4 nbg_rows, 5 nbg_prop_def; -1 otherwise */
int64_t nbg_struct_size(int32_t which);

/* pure arithmetic helpers (host, no GPU needed) */
int32_t nbg_part_of(int64_t vid, int32_t num_parts);          /* StorageClient.cpp:238-243 */
int32_t nbg_rank_of_part(int32_t part, int32_t world_size);   /* CreateSpaceProcessor.cpp:77-90 */

/* ---- schema (meta SchemaManager::getEdgeSchema, src/meta/SchemaManager.h:38) ------------ */
int32_t nbg_schema_set_edge(nbg_ctx* ctx, int32_t edge_type, int32_t schema_ver,
                            int32_t nfields, const char* const* names, const int32_t* types);

/* Vertex tag schema (SchemaManager::getTagSchema, src/meta/SchemaManager.h:32-36) plus the tag's
 * name, which graphd resolves $^.tag.prop / $$.tag.prop with (SchemaManager::toTagID,
 * GoExecutor.cpp:475-478).  Vertex keys of registered tags (NebulaKeyUtils.h:14-17, 24 bytes) are
 * decoded by nbg_snapshot_load_part into per-vertex columns used by GO's $^ / $$ props.       */
int32_t nbg_schema_set_tag(nbg_ctx* ctx, int32_t tag_id, const char* tag_name, int32_t schema_ver,
                           int32_t nfields, const char* const* names, const int32_t* types);

/* ---- snapshot builder --------------------------------------------------------------------
 * Consumes a partition's KV pairs in the reference byte layout (NebulaKeyUtils.h:14-21 keys,
 * dataman RowWriter rows) -- what RocksEngine::prefix iterates (RocksEngine.cpp:191-200) --
 * and builds the GPU-resident CSR + SoA property columns.  Keys/values are concatenated blobs
 * with n+1 offsets.  Keys of unregistered tags / edge types are ignored.  Call once per part (any
 * order), then nbg_snapshot_finalize.                                                       */
int32_t nbg_snapshot_load_part(nbg_ctx* ctx, int32_t part, const uint8_t* key_bytes,
                               const uint64_t* key_offsets, const uint8_t* val_bytes,
                               const uint64_t* val_offsets, size_t n);
/* Synthetic RMAT graph generated on the device (definition in DESIGN.md): the KV the
 * reference's INSERT EDGE path would write (out-edge + empty in-edge, rank 0, one version),
 * produced directly in the decoded-tuple stage of the same builder.                        */
int32_t nbg_snapshot_gen_rmat(nbg_ctx* ctx, int32_t scale, int32_t edge_factor, uint64_t seed,
                              int32_t edge_type);
int32_t nbg_snapshot_finalize(nbg_ctx* ctx);
/* Write path.  nbg_snapshot_write_part takes one part's batch of the KV puts
 * AddEdgesProcessor::process / AddVerticesProcessor::process hand to doPut
 * (AddEdgesProcessor.cpp:15-31, AddVerticesProcessor.cpp:16-38: keys carry version
 * INT64_MAX - now_us; an identical key overwrites) in the same blob layout as load_part.
 * Before the first finalize it is load_part.  After it the snapshot must have been finalized
 * with option "writable" = 1 (which keeps the decoded tuples on the device); the batch is
 * decoded behind them and becomes visible at nbg_snapshot_commit, which rebuilds the CSRs from
 * the device-resident tuples (queries in between read the previous commit).  Commit is
 * collective when world > 1.  Errors: NBG_E_STATE (not writable), NBG_E_PART_NOT_FOUND.     */
int32_t nbg_snapshot_write_part(nbg_ctx* ctx, int32_t part, const uint8_t* key_bytes,
                                const uint64_t* key_offsets, const uint8_t* val_bytes,
                                const uint64_t* val_offsets, size_t n);
int32_t nbg_snapshot_commit(nbg_ctx* ctx);

typedef struct {
  int64_t num_vertices;     /* global vertex count (vertices appearing in any edge)          */
  int64_t local_vertices;   /* vertices owned by this rank                                    */
  int64_t local_out_edges;  /* out-edges (after version / multi-edge collapse) on this rank   */
  int64_t local_in_edges;
  int64_t device_bytes;     /* HBM held by the snapshot on this rank                          */
  double build_seconds;
  int64_t commits;          /* commits applied since finalize                                 */
  int64_t merge_commits;    /* of them, merged into the committed order (no full rebuild)     */
} nbg_snapshot_info;
int32_t nbg_snapshot_info_get(nbg_ctx* ctx, int32_t edge_type, nbg_snapshot_info* out);
/* CSR export for tests: out-degree of vid (-1 if unknown) */
int64_t nbg_snapshot_out_degree(nbg_ctx* ctx, int32_t edge_type, int64_t vid);

/* ---- result rows ------------------------------------------------------------------------
 * Column-major, typed.  col_types: NBG_T_VID (int64; every integer of a GO result is a VID,
 * GoExecutor.cpp:596-600), NBG_T_INT (int64, storage rows), NBG_T_DOUBLE, NBG_T_BOOL (1 byte),
 * NBG_T_STRING (int64 offsets n+1 + bytes).  Memory is owned by the engine until
 * nbg_rows_free.  `on_device` = 1: column pointers are device pointers.                    */
typedef struct {
  int64_t n_rows;
  int32_t n_cols;
  int32_t on_device;
  int32_t* col_types;
  void** cols;            /* per column: int64_t* / double* / uint8_t* / uint8_t* bytes    */
  int64_t** str_offsets;  /* per column: n_rows+1 offsets for STRING columns, else NULL     */
  int64_t* row_vertex;    /* get_bound: vid of the vertex a row belongs to (else NULL)      */
  /* get_bound response parts (QueryResponse, storage.thrift:207-228) */
  int64_t n_vertices;     /* vertices returned (only those with >= 1 edge row, QBP.cpp:61-67) */
  int64_t* vertex_ids;
  int64_t* vertex_row_offsets; /* n_vertices+1 */
  int32_t n_failed;       /* ResultCode list (BaseProcessor.h:64-71) */
  int32_t* failed_parts;
  int32_t* failed_codes;
  uint64_t edges_scanned; /* adjacency entries read (TEPS numerator)            */
  /* nbg_shortest_path: path of row i = path_vids[path_offsets[i] .. path_offsets[i+1])
   * (empty when the pair is unreachable); host memory.  NULL for other calls.              */
  int64_t* path_offsets;  /* n_rows+1 */
  int64_t* path_vids;
  void* _impl;
  /* get_bound SOURCE/DEST tag props (VertexData.vertex_data, QueryBoundProcessor.cpp:19-31): one
   * value per vertex_ids entry and requested tag prop, in request order; host memory.  Types as
   * for the edge columns (STRING: vertex_str_offsets[c] has n_vertices+1 offsets).
   * vertex_col_present[c][i] = 0 when the vertex has no row of that tag in the request's part
   * (the reference then leaves the prop out of the vertex row).                              */
  int32_t n_vertex_cols;
  int32_t* vertex_col_types;
  void** vertex_cols;
  int64_t** vertex_str_offsets;
  uint8_t** vertex_col_present;
} nbg_rows;
void nbg_rows_free(nbg_rows* rows);

/* ---- getBound ------------------------------------------------------------------------------
 * Replaces QueryBoundProcessor::process(GetNeighborsRequest) for OUT_BOUND / IN_BOUND
 * (src/storage/QueryBaseProcessor.inl:462-505, QueryBoundProcessor.cpp:16-106).
 * parts/vids: the request's parts map flattened (pair i = (parts[i], vids[i])).
 * edge_type < 0: in-bound scan (StorageClient.cpp:118).  filter: Expression::encode bytes or
 * empty.  Return columns are EDGE-owned props (key props _src/_dst/_rank/_type or schema props)
 * and SOURCE/DEST tag props (tag_id + name; returned per vertex in vertex_cols; unknown tag ->
 * E_TAG_PROP_NOT_FOUND, unknown prop -> E_IMPROPER_DATA_TYPE on every part).  $^ tag props in
 * the push-down filter read the request part's vertex row ($$ -> E_INVALID_FILTER, as checkExp,
 * QueryBaseProcessor.inl:160-238).  Request-level errors are
 * reported per part in failed_codes (QueryBaseProcessor.inl:470-477), not as the return.    */
typedef struct {
  const char* name;
  int32_t owner;
  int32_t tag_id;
} nbg_prop_def;
int32_t nbg_get_bound(nbg_ctx* ctx, int32_t edge_type, const int32_t* parts,
                      const int64_t* vids, size_t n, const uint8_t* filter, size_t filter_len,
                      const nbg_prop_def* cols, size_t ncols, nbg_rows* out);

/* ---- outBoundStats / inBoundStats ---------------------------------------------------------
 * Replaces QueryStatsProcessor::process (src/storage/QueryStatsProcessor.cpp:16-125,
 * StorageServiceHandler.cpp:40-53): the getBound scan with the same filter push-down, reduced
 * on the device to one row.  stat_types[i] = cpp2::StatType of cols[i] (SUM 1, COUNT 2, AVG 3,
 * storage.thrift:51-55).  Columns in request order: SUM -> INT (int64 sum), COUNT -> INT,
 * AVG -> DOUBLE (sum / count, NaN without rows); in-bound requests skip edge props.  SUM / AVG
 * over BOOL / STRING fail every part with E_IMPROPER_DATA_TYPE (validOperation,
 * QueryBaseProcessor.inl:18-35); SUM / AVG over DOUBLE values return NBG_E_UNSUPPORTED (the
 * reference's int64-initialised sum throws boost::bad_get).  SOURCE / DEST tag props
 * (tag_id + name) reduce over the request entries of owned parts whose vertex row sits in the
 * entry's part (collectVertexProps, QueryBaseProcessor.inl:309-333; QueryStatsProcessor.cpp:
 * 69-82), duplicates counted per entry; unknown tag -> E_TAG_PROP_NOT_FOUND, unknown prop or
 * SUM / AVG over BOOL / STRING -> E_IMPROPER_DATA_TYPE on every part.                        */
int32_t nbg_bound_stats(nbg_ctx* ctx, int32_t edge_type, const int32_t* parts, const int64_t* vids,
                        size_t n, const uint8_t* filter, size_t filter_len, const nbg_prop_def* cols,
                        const int32_t* stat_types, size_t ncols, nbg_rows* out);

/* ---- GO N STEPS ---------------------------------------------------------------------------
 * Replaces GoExecutor's stepOut -> getNeighbors -> onStepOutResponse -> getDstIdsFromResp loop
 * and its final processFinalResult / setupInterimResult (src/graph/GoExecutor.cpp:80-106,
 * 334-431, 585-782) with one device-resident call.  starts: literal or piped vids (duplicates
 * kept unless distinct, GoExecutor.cpp:98-104).  where/yields: Expression::encode bytes as the
 * graphd AST would encode them.  n_yields = 0 means the default YIELD e._dst AS id.
 * With world_size > 1 every rank passes the same spec; rows come back sharded by owner.
 *
 * GO UPTO N STEPS (upto = 1; the reference parses it, parser.yy:455, and refuses to run it,
 * GoExecutor.cpp:121-123; semantics owned by this build, DESIGN.md divergence 7): the rows of
 * GO 1 STEPS, GO 2 STEPS, ... GO N STEPS with the same starts, edge type, WHERE and YIELD,
 * concatenated (row order unspecified); distinct = 1 removes duplicates over the whole
 * concatenation.  A frontier that becomes empty at step k ends the query with the rows of steps
 * 1 .. k-1 (not the empty result of plain GO N STEPS).  A WHERE / YIELD evaluation error at any
 * step fails the query (NBG_E_EVAL).  upto = 1 with steps = 1 is GO 1 STEPS.  $- / $var
 * properties in WHERE or YIELD are not supported under UPTO (NBG_E_UNSUPPORTED; piped starts
 * without input properties work); upto outside {0, 1} is NBG_E_INVALID_ARG.
 * edges_scanned: without distinct the (step, adjacency entry) pairs examined; with distinct the
 * engine runs a visited-pruned BFS and one final step: sum over k < N of outdeg(B_k), B_k the
 * vertices first reached at hop k-1 (B_1 the distinct starts), plus outdeg(union of the B_k).
 *
 * GO ... OVER t REVERSELY (edge_type = -t, t a registered type: the convention of nbg_get_bound;
 * the reference parses it, parser.yy:512-521, and refuses to run it, GoExecutor.cpp:203-205;
 * DESIGN.md divergence 11).  edge_type = 0 is NBG_E_INVALID_ARG, -t with t not in the snapshot
 * NBG_E_INVALID_ARG "edge type not in snapshot", a type without an in CSR NBG_E_UNSUPPORTED.  A
 * hop expands a frontier vertex v over the in keys (part(v), v, -t, rank, u) of v's own part:
 * e._src = v, e._dst = u (the far end, the edge's original source), e._rank = the key's rank,
 * e._type = the alias as always; $^.tag.prop reads v, $$.tag.prop reads u; the default YIELD is
 * e._dst.  In-bound keys carry no edge schema props: one in WHERE or YIELD is
 * NBG_E_IMPROPER_DATA_TYPE "in-bound edges have no props", reported like an unknown edge prop of
 * a forward GO, when the final step runs.  DISTINCT, duplicate starts, $- / $var inputs and the
 * smallest-root rule, the empty-frontier endings, keep_on_device, sharding by owner and UPTO
 * (the concatenation of GO k STEPS ... REVERSELY, k = 1 .. N) carry over unchanged.
 * edges_scanned: as above with in-degrees (the sum of the frontiers' in-degrees; under UPTO
 * DISTINCT indeg(B_k) and indeg(union)), whichever kernel ran a hop.
 * Pull hops: a reverse hop from a large frontier scans the out rows instead (nbg::k_rev_pull, hop
 * mode 6) -- non-final hops, and the final hop of DISTINCT with the lone e._dst yield and no
 * WHERE -- when the frontier's in-degree sum E over ranks is >= in-entries / rev_bu_div (option,
 * default 4).  Options bottom_up = 0 or bu_force = -1: never pull; bu_force = 1: always pull
 * where legal.  Never with $- / $var inputs at steps > 1, nor under UPTO.  A pull is legal only
 * when the in keys mirror the out keys, one in key (v, -t, rank, u) per out key (u, t, rank, v):
 * known after gen_rmat; unknown after KV loads and after a commit that changed the type, then
 * checked exactly on a one-rank context at the first query that would pull (cached until the
 * next such commit); a sharded KV-loaded space stays unknown and runs top-down.  Without the
 * mirror bu_force = 1 still runs top-down: the result never depends on these options.          */
typedef struct {
  int32_t edge_type;      /* < 0: GO ... OVER -edge_type REVERSELY                              */
  int32_t steps;
  const int64_t* starts;
  size_t n_starts;
  const uint8_t* where;
  size_t where_len;
  const uint8_t* const* yields;
  const size_t* yield_lens;
  size_t n_yields;
  int32_t distinct;
  int32_t keep_on_device; /* 1: leave result columns in HBM (bench / chained queries)        */
  /* $-.prop / $var.prop (GoExecutor::getPropFromInterim, GoExecutor.cpp:831-838): the piped or
   * variable input rows, one per starts[i] (the FROM column).  A start vid's props come from its
   * LAST row (InterimResult::buildIndex, InterimResult.cpp:146-160).  Column types NBG_T_VID /
   * NBG_T_INT / NBG_T_DOUBLE (int64 / double arrays), NBG_T_BOOL (uint8) or NBG_T_STRING (bytes
   * + n_starts+1 int64 offsets).  With steps > 1 the final step reads the input row of each
   * dst's root start, as graphd's VertexBackTracker (GoExecutor.h:174-193) does; a dst reached
   * from several starts takes the smallest root vid among its in-edge srcs (the reference's
   * answer there depends on RPC response order; DESIGN.md divergence 6).
   * n_inputs = 0: no input table (zero-initialised specs stay valid).                        */
  size_t n_inputs;
  const char* const* input_names;
  const int32_t* input_types;
  const void* const* input_cols;
  const int64_t* const* input_str_offsets;
  int32_t upto;           /* 1: GO UPTO `steps` STEPS (ABI 7; last, so zeroed specs stay valid) */
} nbg_go_spec;
int32_t nbg_go(nbg_ctx* ctx, const nbg_go_spec* spec, nbg_rows* out);

/* ---- FIND SHORTEST PATH (no reference implementation: FindExecutor.cpp:20-22) ------------
 * Definition (owned by this build): the unweighted hop distance from src to
 * dst over edge_type out-edges, -1 when dst is not reached within max_steps hops; the path is
 * the lexicographically smallest vid sequence among the shortest paths.  Distances toward dst
 * follow the -edge_type in-edge keys (P5: INSERT EDGE writes both), so parity with the oracle
 * assumes the in-edge keys mirror the out-edge keys, as the write path guarantees.
 * Runs as batched bidirectional BFS (pairs in batches, option "sp_batch").
 * out: 3 VID columns [src, dst, hops] per pair, in input order; paths in path_offsets /
 * path_vids (src ... dst, hops+1 vids).  src == dst gives hops 0 and the path [src].        */
int32_t nbg_shortest_path(nbg_ctx* ctx, int32_t edge_type, const int64_t* src,
                          const int64_t* dst, size_t npairs, int32_t max_steps, nbg_rows* out);

/* ---- ORDER BY -----------------------------------------------------------------------------
 * Replaces OrderByExecutor::execute (src/graph/OrderByExecutor.cpp:104-136: std::sort of the
 * piped rows under the factor comparator) on a result table: `GO ... | ORDER BY $-.col [ASC|DESC],
 * ...`.  in: a plain row table as nbg_go hands it out, host-resident (its columns are uploaded)
 * or device-resident (on_device = 1, produced on this context); it is neither consumed nor
 * modified, and the caller frees both in and out.  A table carrying row_vertex, vertices, failed
 * parts or paths is NBG_E_INVALID_ARG.  Factor f orders by column cols[f], descending when
 * desc[f] = 1; factor 0 is the most significant.  Resolving `$-.name` to an index, and dropping
 * names the input does not have (OrderByExecutor.cpp:91-101), is the caller's job.  n_factors = 0
 * returns the rows in input order (OrderByTest.WrongFactor); a column's later repeats decide
 * nothing.  A column index out of range or desc outside {0, 1} is NBG_E_INVALID_ARG.
 * Order (ColumnValue::operator<, OrderByExecutor.cpp:14-68): VID / INT / TIMESTAMP as signed
 * int64, BOOL false < true, DOUBLE numeric, STRING as std::string (unsigned bytes, a proper prefix
 * first, embedded NUL bytes legal).  DESC is the exact reverse.  Owned by this build (DESIGN.md
 * divergence 8): the sort is stable (rows equal under every factor keep their input order; the
 * reference's std::sort leaves it open), -0.0 ties with +0.0, every NaN ties with every NaN and
 * sorts after +inf under ASC.
 * out: the same column types, in HBM when keep_on_device = 1, else on the host (STRING columns as
 * packed bytes + n_rows+1 offsets); zero input rows give zero rows.  edges_scanned is copied.
 * NBG_E_UNSUPPORTED: a STRING factor with a value longer than 256 bytes; 2^32 rows or more.
 * NBG_E_NOMEM: the workspace (24 B per row + the output) did not fit; the input is untouched.
 * Works on any context (no snapshot needed).  Rank-local: with world_size > 1 each rank orders
 * the rows it holds and no collective is issued; merging the ranks' runs stays with the caller.
 * nbg_last_timing then reports total_ms (a host table's upload, the sort and the output
 * permutation; the copies to the host behind them are not in it), launches (kernels; a scan counts as one), steps_run (radix
 * passes that ran), host_waits (one per 64-bit key sorted, plus the hand-out) and n_hops = 0.   */
int32_t nbg_order_by(nbg_ctx* ctx, const nbg_rows* in, const int32_t* cols, const int32_t* desc,
                     size_t n_factors, int32_t keep_on_device, nbg_rows* out);

/* ---- UNION / INTERSECT / MINUS -----------------------------------------------------------------
 * Replaces SetExecutor (src/graph/SetExecutor.cpp:143-328: doUnion / doDistinct's sort + unique,
 * and the nested row loops of doIntersect / doMinus) on two result tables: `A UNION [ALL|DISTINCT]
 * B`, `A INTERSECT B`, `A MINUS B`.  left / right: plain row tables as nbg_go / nbg_order_by hand
 * them out, each one host-resident (uploaded) or device-resident on this context (read in place);
 * neither is consumed or modified, and the caller frees left, right and out.  A table carrying
 * row_vertex, vertices, failed parts or paths is NBG_E_INVALID_ARG.
 * Schema (checkSchema, SetExecutor.cpp:188-218): the column counts must match, else
 * NBG_E_INVALID_ARG "Field count not match."; a side with n_cols = 0 and n_rows = 0 is the
 * reference's nullptr result and takes the other side's schema.  The output's column types are the
 * left's.  VID / INT / TIMESTAMP are one integer type; where the types otherwise differ the right
 * column is first cast to the left's type (doCasting, SetExecutor.cpp:220-234;
 * InterimResult::castTo, InterimResult.cpp:215-347): int <-> double by static_cast, int / double ->
 * bool by != 0, bool -> int / double as 0 / 1.  double -> int of NaN or of a value outside int64 is
 * undefined in the reference: here it saturates, and NaN becomes 0.  A cast to or from STRING is
 * NBG_E_UNSUPPORTED.
 * Row equality (owned by this build, DESIGN.md divergence 9): integers, bools and strings by value
 * (strings as bytes plus length, embedded NUL bytes legal); doubles under ORDER BY's tie rule:
 * -0.0 == +0.0 and every NaN equals every NaN (the reference's == never matches a NaN).  An output
 * row carries the bits of the input row it came from.
 *   NBG_SET_UNION, distinct = 0   the left rows, then the right rows (after any cast), each side in
 *                                 input order (doUnion, SetExecutor.cpp:143-186)
 *   NBG_SET_UNION, distinct = 1   of that concatenation the first occurrence of every distinct row,
 *                                 in concatenation order.  doDistinct (SetExecutor.cpp:237-241)
 *                                 leaves the rows sorted; this call does not sort (chain
 *                                 nbg_order_by over every column for that order).  A side without
 *                                 rows is an empty set, and the other side is still deduplicated
 *                                 (the reference returns it as it is, SetExecutor.cpp:145-157)
 *   NBG_SET_INTERSECT             every left row equal to some right row, in left order, with the
 *                                 left's multiplicity (doIntersect, SetExecutor.cpp:269-277, moves
 *                                 matched right rows out and compares against the moved-from rows
 *                                 afterwards; on tables without duplicates the two agree)
 *   NBG_SET_MINUS                 every left row equal to no right row, in left order, multiplicity
 *                                 kept: doMinus (SetExecutor.cpp:283-328)
 * distinct is ignored for INTERSECT / MINUS, as in the reference.  op outside {1, 2, 3} or distinct
 * outside {0, 1} is NBG_E_INVALID_ARG.  The output is deterministic: the same inputs give the same
 * rows in the same order on every run.
 * out: in HBM when keep_on_device = 1, else on the host (STRING columns as packed bytes + n_rows+1
 * offsets).  edges_scanned = left's + right's.
 * NBG_E_UNSUPPORTED: left.n_rows + right.n_rows >= 2^32.
 * NBG_E_NOMEM: the workspace did not fit; the inputs are untouched.  Per row, besides the output
 * and a host table's upload: INTERSECT / MINUS 8 B (hash) per left and right row, 16 to 32 B (the
 * table: 8 B x the power of two >= 2 x rows) per right row and 9 B (keep byte, position, index) per
 * left row; UNION DISTINCT the concatenated columns plus 8 + 9 + 16 to 32 B per row of both sides;
 * UNION ALL nothing; a right column under a cast adds its cast copy.
 * Works on any context (no snapshot needed).  Rank-local: with world_size > 1 each rank combines
 * the rows it holds and no collective is issued; bringing equal rows to the same rank first stays
 * with the caller.
 * nbg_last_timing then reports total_ms (uploads, kernels and the output gather; the copies to the
 * host behind them are not in it), launches (kernels; a scan counts as one), host_waits and
 * n_hops = 0.  host_waits: 2 (the fetch of the output row count, and the hand-out) for INTERSECT /
 * MINUS with left rows and for UNION DISTINCT with rows; 1 (the hand-out) otherwise, where the
 * count needs no device; plus one per STRING column of a device-resident input with rows (its
 * byte total).
 * Engine option "set_hash_bits" (default 64; tests): the row hash is masked to its low k bits, so
 * 0 makes every row collide.                                                                   */
#define NBG_SET_UNION 1
#define NBG_SET_INTERSECT 2
#define NBG_SET_MINUS 3
int32_t nbg_set_op(nbg_ctx* ctx, int32_t op, const nbg_rows* left, const nbg_rows* right,
                   int32_t distinct, int32_t keep_on_device, nbg_rows* out);

/* ---- GROUP BY ----------------------------------------------------------------------------------
 * `... | GROUP BY $-.a YIELD $-.a, COUNT(*), SUM($-.b)` on a result table.  The reference
 * (v1.0.0-beta) has no GROUP BY; the later nGQL releases do, and the semantics below are owned by
 * this build (DESIGN.md divergence 13).  in: a plain row table as nbg_go / nbg_order_by /
 * nbg_set_op hand it out, host-resident (uploaded) or device-resident on this context (read in
 * place); it is neither consumed nor modified, and the caller frees both in and out.  A table
 * carrying row_vertex, vertices, failed parts or paths is NBG_E_INVALID_ARG.
 * Output columns: the n_keys key columns first, in key_cols order and with their input types (a
 * key column may repeat: the repeat decides nothing and is output again), then the n_aggs
 * aggregates: agg_fns[i] over column agg_cols[i].
 *   NBG_AGG_COUNT   the group's row count, NBG_T_INT; agg_cols[i] is ignored (-1 included)
 *   NBG_AGG_SUM     over VID / INT / TIMESTAMP the int64 sum with two's-complement wrap-around,
 *                   NBG_T_INT; over DOUBLE an IEEE sum of the group's values, NBG_T_DOUBLE, whose
 *                   association order is fixed by the input alone: the same input gives the same
 *                   bits on every run, but it is not defined to equal a left-to-right sum
 *   NBG_AGG_AVG     NBG_T_DOUBLE: double(that wrapped sum) / double(count) over integers (the
 *                   `sum / count` of nbg_bound_stats), that double sum / count over DOUBLE
 *   NBG_AGG_MIN / NBG_AGG_MAX   the column's own type, under ORDER BY's order: integers as signed
 *                   int64, false < true, doubles numerically with NaN after +inf.  For doubles
 *                   the value is canonical: a zero extreme is +0.0, a NaN extreme is the quiet NaN
 *                   0x7ff8000000000000, every other value keeps its own bits
 * SUM / AVG over BOOL or STRING is NBG_E_IMPROPER_DATA_TYPE (validOperation, as nbg_bound_stats);
 * MIN / MAX over STRING is NBG_E_UNSUPPORTED (STRING key columns are fully supported).
 * Groups: one output row per distinct key tuple under nbg_set_op's row equality (integers and bools
 * by value, strings as bytes plus length with embedded NUL bytes legal, -0.0 == +0.0, every NaN
 * equals every NaN).  The key columns of an output row carry the bits of the group's first input
 * row, and the groups come in first-occurrence order (the order UNION DISTINCT leaves;
 * deterministic; chain nbg_order_by for another one).  n_keys = 0 puts every row into one group
 * (`| YIELD COUNT(*), SUM($-.x)`); n_aggs = 0 with keys is a DISTINCT projection of the key
 * columns; both zero is NBG_E_INVALID_ARG.  Zero input rows give zero output rows with the
 * output's column count and types, for n_keys = 0 too (there is no NULL to put into MIN).
 * NBG_E_INVALID_ARG: a null ctx, in or out; a null array with a count > 0; a column index out of
 * range; a function outside 1..5; keep_on_device outside {0, 1}.
 * NBG_E_UNSUPPORTED: n_keys + n_aggs > 16 (a result has at most 16 columns); 2^32 rows or more.
 * NBG_E_NOMEM: the workspace did not fit; the input is untouched.  Besides the output and a host
 * table's upload, with keys: per row 8 B (hash), 16 to 32 B (the table: 8 B x the power of two
 * >= 2 x rows), 4 B (group id), 1 B + 4 B (first-occurrence byte and its scan); per group 4 B (first
 * row).  The aggregates add, on the atomic path, per group 8 B x (1 + the aggregates other than
 * COUNT); on the ordered path per row 8 B (the order: two row indices) and up to 16 B (radix keys),
 * per group 12 B (segment offsets, chunk numbers) and 8 B per aggregate for every 16384 rows of a
 * group of more than 4096.
 * out: in HBM when keep_on_device = 1, else on the host (STRING columns as packed bytes + n_rows+1
 * offsets).  edges_scanned is copied from in.
 * Works on any context (no snapshot needed).  Rank-local: with world_size > 1 each rank groups the
 * rows it holds and no collective is issued; INTEGRATION.md has the rule by which a caller merges
 * the ranks' partial tables.
 * Two paths, the same table from both wherever both are defined.  Atomic (no SUM / AVG over
 * DOUBLE): 64-bit integer atomics per row, through LDS first when the groups are few.  Ordered (a
 * SUM / AVG over DOUBLE, or engine option "group_sorted" = 1): the rows in a stable order by group,
 * each segment reduced in a tree fixed by its length; no float atomics anywhere.
 * nbg_last_timing then reports total_ms (uploads and kernels; the copies to the host behind them
 * are not in it), launches (kernels; a scan counts as one), host_waits and n_hops = 0.
 * host_waits, independent of the row and group counts: 1 (the hand-out) for zero input rows or
 * n_keys = 0; with keys and rows 2 (the fetch of the group count, and the hand-out) on the atomic
 * path and for n_aggs = 0, 3 on the ordered path (one more for the order's digit histogram) unless
 * there is one group only (2); plus one per STRING column of a device-resident input with rows
 * (its byte total).
 * Engine options (tests, measurement): "group_sorted" (default 0), "group_lds_max" (default 1024:
 * the atomic path accumulates in LDS when the group count is at most this and groups x (1 +
 * aggregates other than COUNT) <= 4096 words), "set_hash_bits" (masks the key hash as in
 * nbg_set_op).  No option changes a result.                                                     */
#define NBG_AGG_SUM 1    /* cpp2::StatType values, as nbg_bound_stats takes them */
#define NBG_AGG_COUNT 2
#define NBG_AGG_AVG 3
#define NBG_AGG_MIN 4
#define NBG_AGG_MAX 5
int32_t nbg_group_by(nbg_ctx* ctx, const nbg_rows* in, const int32_t* key_cols, size_t n_keys,
                     const int32_t* agg_fns, const int32_t* agg_cols, size_t n_aggs,
                     int32_t keep_on_device, nbg_rows* out);

/* ---- FETCH PROP ON (FetchVerticesExecutor / FetchEdgesExecutor) ---------------------------
 * FETCH PROP ON tag vid, ... [YIELD [DISTINCT] ...] and FETCH PROP ON edge src->dst[@rank], ...:
 * the device replacement of FetchVerticesExecutor::fetchVertices / processResult
 * (src/graph/FetchVerticesExecutor.cpp:84-196) over QueryVertexPropsProcessor
 * (src/storage/QueryVertexPropsProcessor.cpp) and of FetchEdgesExecutor::fetchEdges / processResult
 * (src/graph/FetchEdgesExecutor.cpp:221-330) over QueryEdgePropsProcessor::collectEdgesProps
 * (src/storage/QueryEdgePropsProcessor.cpp:17-40): a point lookup of every key in the resident
 * snapshot instead of one RocksDB prefix scan per key.
 * Keys: n vids, or n (src, dst, rank) triples (rank == NULL: every key has rank 0).  With
 * keys_on_device = 1 the key arrays are device pointers on this context (columns of a
 * keep_on_device result of nbg_go, nbg_order_by, nbg_set_op or of these calls); they are read in
 * place and neither consumed nor modified.
 * Yields: Expression::encode bytes as for nbg_go.  Only the alias.prop form is legal
 * (FetchExecutor::prepareYield, FetchExecutor.cpp:13-50): a $^ / $$ / $- / $var node or an
 * edge-key function (_src(e), ...) is NBG_E_INVALID_ARG ("Only support form of alias.prop in fetch
 * sentence."), as is a yield list without any prop ("No props declared.").  Vertices: the alias must
 * be the tag's name (else NBG_E_INVALID_ARG) and prop one of its fields.  Edges: the alias is
 * ignored, as nbg_go ignores it; prop is a schema field or _src / _dst / _rank, the key props
 * QueryEdgePropsProcessor::addDefaultProps returns (QueryEdgePropsProcessor.cpp:42-48); _type is
 * NBG_E_UNSUPPORTED.  An unknown prop is NBG_E_IMPROPER_DATA_TYPE.  Arithmetic, relational and
 * logical operators and constants over the props run on the device VM unchanged.  n_yields = 0:
 * every field of the tag / edge schema in schema order (FetchExecutor::setupColumns,
 * FetchExecutor.cpp:52-80).  More than 16 yields: NBG_E_UNSUPPORTED.
 * A vid yields a row iff the tag has a row for it in the vid's own part (StorageClient sends the
 * request to part hash(vid), StorageClient.cpp:238-243); a vid without one is skipped
 * (FetchVerticesExecutor.cpp:136-145).  This includes vertices no edge names (INSERT VERTEX alone).
 * With several versions of the row the bytewise-first one is read (collectVertexProps,
 * QueryBaseProcessor.inl:309-333).  An edge key yields a row iff src's out-edges of edge_type hold
 * (src, rank, dst) in a row nbg_go would expand (the keys sit in src's own part); of several
 * versions the bytewise-first one is read ("only use the latest version",
 * QueryEdgePropsProcessor.cpp:26).  A key with an unknown vid is skipped.
 * Row order (owned by this build, DESIGN.md divergence 10): the rows come in key input order; the
 * reference's order is the order its storage RPC responses arrive in.
 * distinct = 1: the keys are deduplicated first, keeping first occurrences (getDistinctVIDs,
 * FetchVerticesExecutor.cpp:248-250; EdgeKeyHashSet, FetchEdgesExecutor.cpp:144-172); then the
 * output rows by value, first occurrence kept, in order (uniqResult, FetchVerticesExecutor.cpp:134-176, FetchEdgesExecutor.cpp:270-312)
 * under nbg_set_op's row equality.
 * out: column types are the yields' static result types as for nbg_go (every integer is
 * NBG_T_VID).  Zero keys or zero matches give n_rows = 0 with n_cols = the yield count and those
 * types.  In HBM when keep_on_device = 1, else on the host; STRING columns as packed bytes +
 * n_rows + 1 offsets.  An evaluation error on any emitted row (a field the row lacks included)
 * fails the call with NBG_E_EVAL, as in nbg_go (GoExecutor.cpp:754-758).
 * Errors: NBG_E_STATE before finalize; NBG_E_TAG_PROP_NOT_FOUND unknown tag_id; NBG_E_INVALID_ARG
 * unknown edge type, null pointers with n > 0, a flag outside {0, 1}; NBG_E_UNSUPPORTED 2^32 keys
 * or more, a negative edge_type (in-edges carry no props).
 * world_size > 1: every rank passes the same keys and emits the rows of the keys it owns (the
 * vid's part owner; src's part owner for edges); no collective is issued, and the row-level
 * DISTINCT is rank-local as in nbg_set_op.
 * nbg_last_timing then reports total_ms, launches, host_waits and n_hops = 0.  edges_scanned: 0
 * for vertices; for edges the adjacency entries the lookup read (informational).  host_waits: 3
 * with keys (the match count, the materialiser's error count together with its STRING byte
 * totals, the hand-out; the second is skipped without matches), 1 without keys; distinct adds one
 * for the key dedup and one for the row dedup (more than one row).
 * Engine option "fetch_search" (tests, measurement): 0 = every row is scanned, 1 = every row is
 * searched, unset = the hybrid: rows of up to 64 entries are scanned, longer rows are searched
 * down to a window of 64 entries, which is scanned; option
 * "fetch_threshold" replaces the 64 (measurement).                                             */
int32_t nbg_fetch_vertices(nbg_ctx* ctx, int32_t tag_id, const int64_t* vids, size_t n,
                           int32_t keys_on_device, const uint8_t* const* yields,
                           const size_t* yield_lens, size_t n_yields, int32_t distinct,
                           int32_t keep_on_device, nbg_rows* out);
int32_t nbg_fetch_edges(nbg_ctx* ctx, int32_t edge_type, const int64_t* src, const int64_t* dst,
                        const int64_t* rank, size_t n, int32_t keys_on_device,
                        const uint8_t* const* yields, const size_t* yield_lens, size_t n_yields,
                        int32_t distinct, int32_t keep_on_device, nbg_rows* out);

/* ---- FIND props FROM tag / edge WHERE (FindSentence) ----------------------------------------
 * FIND prop_list FROM name_label where_clause: the reference parses the sentence (parser.yy:565-571,
 * FindSentence, src/parser/TraverseSentences.h:83-113) and FindExecutor::prepare answers "Does not
 * support" (src/graph/FindExecutor.cpp:20-22).  The semantics below are this build's (DESIGN.md
 * section 5, divergence 12): a scan of the resident columns that returns the vertices / edges whose
 * props satisfy WHERE, the start vids of a later GO.
 * Vertices: the candidates are every vid with a row of tag_id in the vid's own part that this rank
 * owns, vertices no edge names included; of several versions of the row the bytewise-first is read:
 * the row nbg_fetch_vertices returns for that vid.  Column 0 is the vid (NBG_T_VID, "VertexID");
 * the yields follow.
 * Edges: the candidates are every entry of the edge_type out-CSR in a row nbg_go would expand (the
 * keys sit in src's own part), each the bytewise-first version of its (src, rank, dst) group.
 * Columns 0..2 are _src, _dst, _rank (NBG_T_VID); the yields follow.  A negative edge_type is
 * NBG_E_UNSUPPORTED (in-edges carry no props), a type not in the snapshot NBG_E_INVALID_ARG.
 * A candidate is selected when WHERE is true; where_len = 0 selects every candidate, and a WHERE
 * without any prop node is legal.  A WHERE whose value is not a bool counts as nbg_go counts it
 * (asBool: int != 0, double != 0.0, a string iff empty).
 * WHERE and yields: Expression::encode bytes, compiled under FETCH PROP ON's rule.  Vertices: the
 * legal prop node is alias.prop with alias = the tag's name (another alias: NBG_E_INVALID_ARG).
 * Edges: alias.prop with any alias, and the key props _src, _dst, _rank; _type is
 * NBG_E_UNSUPPORTED.  A $^ / $$ / $- / $var node or an edge-key function (_src(e), ...) is
 * NBG_E_INVALID_ARG ("Only support form of alias.prop in fetch sentence."); an unknown prop is
 * NBG_E_IMPROPER_DATA_TYPE.  Arithmetic, relational, logical and unary operators and constants
 * over these nodes run on the device VM as in nbg_go (graphd semantics, not storage's).
 * n_yields = 0 returns the key columns alone (the form a pipe into GO wants; not FETCH's "every
 * field", not an error).  More than 15 yields (vertices) / 13 yields (edges): NBG_E_UNSUPPORTED
 * (a result has at most 16 columns).
 * Evaluation: a WHERE evaluation error on any candidate (a field its row lacks included) fails the
 * call with NBG_E_EVAL, as does a YIELD evaluation error on any selected row.  What is no
 * candidate is never evaluated and cannot fail the call: a row of a foreign part, a vid of another
 * rank.
 * Row order: deterministic, otherwise unspecified: ascending by position in the scanned structure
 * (edges: out-CSR entry order; vertices: column index order, vertices without edges last), the
 * same on every run and for every value of the option below.  Chain nbg_order_by for a meaningful
 * order.
 * out: column types as for nbg_fetch_*; in HBM when keep_on_device = 1, else on the host; STRING
 * columns as packed bytes + n_rows + 1 offsets.  A device result feeds nbg_order_by, nbg_set_op
 * and nbg_fetch_* (keys_on_device) in place; nbg_go takes host starts, so FIND | GO copies column 0
 * to the host.
 * Errors: NBG_E_STATE before finalize; NBG_E_TAG_PROP_NOT_FOUND unknown tag_id; NBG_E_INVALID_ARG
 * null pointers with lengths > 0, keep_on_device outside {0, 1}; NBG_E_UNSUPPORTED 2^32 selected
 * rows or more.
 * world_size > 1: every rank scans what it owns and emits those rows; no collective is issued.
 * After nbg_snapshot_commit the scan reads the new commit.
 * nbg_last_timing then reports total_ms, launches, host_waits and n_hops = 0; expand_ms,
 * expand_launches and expand_bytes describe the scan kernels alone (edges);
 * edges_scanned: the entries of the out-CSR the edge scan went over, 0 for vertices.
 * host_waits: 3 with selected rows (the match count together with the WHERE error count, the
 * materialiser's error count together with its STRING byte totals, the hand-out), 2 without
 * (no materialiser; nbg_find_vertices with n_yields = 0 has none either), 1 when there is nothing
 * to scan (no entry of the type / no row of the tag).
 * launches, edges with a typed compare (below): 3 (count, scan of the tile counts, emit; 2 without
 * selected rows), plus 1 on the first such call on a type after finalize / a commit (the table of
 * each tile's first row).  Edges otherwise: 4 (frontier, tile rows, expansion, select), plus 1 with
 * selected rows (slot -> entry), plus 2 when foreign-part rows exist (visible degrees, their scan).
 * Vertices: 2 (flags, select), plus 1 with selected rows (the vid column).  All: plus the
 * materialiser's with selected rows and yields: 1, and 2 per STRING column (1 if all are empty).
 * Engine option "find_fast" (tests, measurement): the edge scan of a WHERE of the form
 * `int prop REL int constant` reads the prop's column alone, 8 entries per lane in 8- / 16-byte
 * loads (k_find_count / k_find_emit); every other WHERE runs nbg_go's expansion kernel over all
 * rows.  0 forces the latter for every WHERE, 1 or unset takes the former wherever eligible.     */
int32_t nbg_find_vertices(nbg_ctx* ctx, int32_t tag_id, const uint8_t* where, size_t where_len,
                          const uint8_t* const* yields, const size_t* yield_lens, size_t n_yields,
                          int32_t keep_on_device, nbg_rows* out);
int32_t nbg_find_edges(nbg_ctx* ctx, int32_t edge_type, const uint8_t* where, size_t where_len,
                       const uint8_t* const* yields, const size_t* yield_lens, size_t n_yields,
                       int32_t keep_on_device, nbg_rows* out);

/* ---- timing of the last call (HIP events on the engine stream) --------------------------- */
/* one hop of the last nbg_go: mode 0 = top-down expansion of a frontier list, 1 = bottom-up
 * over the transposed CSR.  c[]: top-down {frontier, entries, next frontier, 0, 0, 0};
 * bottom-up {found, next-hop out-degree sum, slab words read, rows scanned past the slab,
 * entries read past the slab, predicate values read past the slab, first-pass frontier probes
 * answered by L2, first-pass probes answered from the LDS hub copy}.
 * A hop of a GO UPTO ... DISTINCT's pruned BFS (final_hop = 0; kernels names nbg::k_upto_claim,
 * mode 0, or nbg::k_upto_bu, mode 1): c[] = {vertices first reached, their out-degree sum, size
 * of the level expanded, adjacency entries read, 0, 0, 0, 0}; its final step records as above.
 * mode 6 = a pull hop of GO ... REVERSELY over the out rows (kernels names nbg::k_rev_pull):
 * c[] = {found, next-hop in-degree sum, 0, rows scanned, entries read, 0, 0, 0}.
 * nbg_shortest_path records one entry per launch instead: mode 2 = BFS expansion, 3 = meet
 * probe, 4 = sweep; c[] = {tuples, adjacency entries, claims, meets so far, iteration,
 * active pairs, 0, 0}; 5 = walk scan (device-driven batches), c[] = {chunks, adjacency
 * entries, 0, meets, walk step, 0, 0, 0}.                                                   */
typedef struct {
  int32_t mode;
  int32_t final_hop;
  double ms;         /* HIP-event time of the hop's expansion kernels                      */
  uint64_t bytes;    /* their algorithmic bytes                       */
  uint64_t c[8];
  double kernel_ms;      /* the hop's dominant kernel alone (first pass of a bottom-up hop)  */
  uint64_t kernel_bytes; /* that kernel's algorithmic bytes                                  */
  char kernels[160];     /* rocprof names of the hop's kernels, dominant first, "; "-separated
                            (empty: a top-down hop, nbg::k_expand)                          */
} nbg_hop_stat;
#define NBG_MAX_HOP_STATS 16
typedef struct {
  double total_ms;        /* device time of the last nbg_go / nbg_get_bound (events around the
                             whole call; 0 for nbg_go with option hop_timing = 0, which records
                             no event at all)                                                  */
  double expand_ms;       /* summed time of the expansion kernels                            */
  int64_t expand_launches;
  uint64_t edges_scanned;
  uint64_t expand_bytes;  /* algorithmic bytes of the expansion kernels          */
  int32_t steps_run;
  int32_t bu_steps;       /* steps that ran bottom-up over the transposed CSR               */
  double comm_ms;         /* time in frontier exchanges / reductions between ranks          */
  uint64_t comm_bytes;    /* bytes this rank sent to other ranks                            */
  int32_t n_hops;         /* entries of hops[] filled (nbg_go, nbg_shortest_path)            */
  nbg_hop_stat hops[NBG_MAX_HOP_STATS];
  int32_t host_waits;     /* times the engine waited on the host for the device in the last
                             call (counter fetches, stream synchronisations; waits inside the
                             LocalComm / RCCL transport not included)                          */
  int32_t spec_hops;      /* nbg_go: hops that ran speculatively behind a device gate;
                             nbg_shortest_path: batches that ran device-driven (the others ran
                             host-driven: option sp_dev = 0, or a list overflow re-ran them)   */
  int32_t launches;       /* nbg_shortest_path: kernel launches of its device-driven batches
                             (ABI 5); nbg_order_by / nbg_set_op: their kernel launches; 0 for
                             other calls                                                     */
  int32_t comm_calls;     /* collectives this rank issued through its communicator in the last
                             call (ABI 6; comm_ms / comm_calls = the mean time of one on the
                             engine stream, enqueue to completion)                              */
} nbg_timing;
int32_t nbg_last_timing(nbg_ctx* ctx, nbg_timing* out);
/* engine option key = value (tuning knobs); value INT64_MIN removes the key, so the
 * engine default applies again                                                              */
int32_t nbg_set_option(nbg_ctx* ctx, const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* NEBULA_AMD_H_ */
