/*
 * linkteller_hip.h -- C ABI of the MI355X (gfx950) implementation of LinkTeller's
 * influence-analysis hot path.
 *
 * The reference (AI-secure/LinkTeller) is pure Python/PyTorch and has no FFI/plugin layer
 * (SURVEY.md section 8b): its "operator interface" for this path is four PyTorch call
 * sites.  Each entry point below names the reference call site it stands in for
 * (file:line relative to the reference tree); INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (LT_OK) or a negative lt_status; nothing throws across the
 *     boundary; lt_last_error() returns a thread-local description of the last failure.
 *   - "device" pointers are borrowed HIP device pointers (e.g. torch tensor data_ptr());
 *     the caller keeps them alive until the stream has drained.  All matrices are
 *     row-major fp32 with an explicit leading dimension in elements.
 *   - kernels are enqueued on the caller's stream (a hipStream_t passed as void*; NULL =
 *     the default stream) and never synchronise; workspaces are caller-provided so that
 *     the launch functions are hipGraph-capturable.
 *   - handles are not thread-safe: one handle per host thread / per rank.
 */
#ifndef LINKTELLER_HIP_H
#define LINKTELLER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_ABI_VERSION 5   /* 5: lt_influence_rows_f64 (the probes' blocks write the float64 matrix themselves), lt_influence_matrix_host (the same, synchronous, packed), the on-demand pre-activation by
                            row list (lt_baseline_form / gather / scatter_rows_fp64: hub rows shared between ranks); every version-4 entry
                            point is unchanged.  4: lt_export_rows_f64 (the matrix leaves the device once, as float64), node ids checked on the device
                            (LT_ERR_INDEX, lt_node_check), lt_profile_calls; every version-3 entry point is unchanged.  2: lt_baseline_refresh launches nothing (lazy recomputation on the first reader's stream); fp64 shard entry points;
                            profile classes 9-11.  3: lt_influence_rows_vec + lt_wide_combine (layers wider than one pass of the fused
                            kernels), lt_spmm_gather_ceiling (measurement support); every version-2 entry point is unchanged.
                            Additive within 5: training of the 2-layer GCN (lt_gcn2_trainer_*) and lt_adam_step; no entry point changed.
                            Additive within 5: training of the 3-layer GCN (lt_gcn3_trainer_*); no entry point changed.
                            Additive within 5: edge recovery (lt_top_pairs_lower, profile classes 12-13); no entry point changed.
                            Additive within 5: attack metrics (lt_score_curve, profile classes 14-15); no entry point changed.
                            Additive within 5: the attack's node pairs (lt_sample_square_labels, lt_group_pairs, lt_upper_edge_count,
                            lt_sample_balanced_philox); no entry point changed.
                            Additive within 5: the baseline attacks' scores (lt_corr_square, lt_corr_pairs); no entry point changed.
                            Additive within 5: validation every epoch (lt_eval_head, lt_early_stop_*, lt_gcn*_trainer_attach_validation /
                            _run_validated / _val_state / _restore_best / _val_logits); no entry point changed.
                            Additive within 5: evaluation over a row list (lt_eval_head_rows, lt_eval_head_rows_workspace_bytes,
                            lt_gcn*_trainer_attach_validation_rows); no entry point changed.
                            Additive within 5: the wide head of the 2-layer trainer (lt_gcn2_trainer_create_wide, _counts, _hidden,
                            _attach_validation_wide, lt_eval_head_wide, lt_eval_head_wide_workspace_bytes); no entry point changed.
                            Additive within 5: the wide head of the 3-layer trainer (lt_gcn3_trainer_create_wide, _counts,
                            _attach_validation_wide); no entry point changed.
                            Additive within 5: edge recovery over rows that arrive in chunks (lt_top_stream_*) and lt_pairs_present;
                            no entry point changed.
                            Additive within 5: the pair list of the 3-layer model (lt_influence3_pairs, _workspace_bytes); no entry
                            point changed.
                            Additive within 5: the 2-layer model with a wide class layer through one handle (lt_baseline2w_*,
                            lt_influence2w_*); no entry point changed.
                            Additive within 5: minibatch training of the feature-only MLP baselines (lt_mlp_trainer_*,
                            lt_mlp_forward, lt_mlp_forward_workspace_bytes); no entry point changed.
                            Additive within 5: row bands of the baseline attacks' square (lt_corr_rows_prepare, lt_corr_rows,
                            lt_corr_rows_workspace_bytes); no entry point changed */

typedef enum lt_status {
    LT_OK = 0,
    LT_ERR_INVALID = -1,     /* bad argument / malformed CSR                          */
    LT_ERR_HIP = -2,         /* a HIP runtime call failed (message has the HIP error) */
    LT_ERR_UNSUPPORTED = -3, /* shape outside what the kernels are built for          */
    LT_ERR_WORKSPACE = -4,   /* caller workspace too small / misaligned               */
    LT_ERR_NOMEM = -5,
    LT_ERR_INDEX = -6        /* a node id of an EARLIER call's device lists was out of range (see lt_node_check) */
} lt_status;

/* how lt_influence_rows evaluates a probe (all three give the reference's quantity
 * || (f(X + d*e_v x_v^T) - f(X))[u] ||_2 / d, attacker.py:100-108,227-229)            */
typedef enum lt_influence_mode {
    LT_MODE_FULL = 0,   /* every probe: perturbed row GEMV + full SpMM over all N rows + ReLU + W2
                           + layer-2 SpMM on the observed rows, then the fp32 finite difference */
    LT_MODE_SPARSE = 1, /* bit-identical to FULL, but only rows whose value can differ from the
                           baseline (the 1-/2-hop set of the probe) are recomputed             */
    LT_MODE_DELTA = 2   /* propagates the perturbation itself (piecewise-linear through ReLU):
                           no cancellation, agrees with an fp64 evaluation of the reference
                           (within 1e-5 of the largest score on the value domain stated at
                           lt_baseline_enable_fp64)                                              */
} lt_influence_mode;

typedef struct lt_graph lt_graph;       /* device-resident normalised adjacency (CSR + CSC) */
typedef struct lt_baseline lt_baseline; /* unperturbed forward state of a 2-layer GCN       */

const char *lt_last_error(void);
int lt_abi_version(void);
/* number of visible HIP devices (0 on a CPU-only box; never initialises a context) */
int lt_device_count(int *count);

/* ---- tuning knobs (no reference counterpart) ---------------------------------------------------
 * Every setting gives bit-identical results unless its entry says otherwise (the entries that choose another fp64 summation order
 * or storage form for LT_MODE_DELTA's product: results then agree to < 1e-6 of the largest score); the knobs choose between kernel
 * routes and are what the tests use to run each route on small inputs.  Defaults come from LT_* environment variables read once.
 *   "tiled_min_bytes"     S of at least this many bytes takes the tiled SpMM / layer-1 route (default 32 MiB)
 *   "chunk_budget_bytes"  per-call scratch budget that decides the probe chunking (default 1 GiB)
 *   "full_p"              probes per wave of FULL stage A: 8 / 16 / 32, 0 = from the probe count
 *   "long_par"            hub rows in FULL stage A: 1 = segments in separate waves, 0 = one wave per row
 *   "overlap"             hub-row kernels on the baseline's side stream (1) or on the caller's (0)
 *   "item_bits"           SPARSE / DELTA stage B membership bitmap on (1) / off (0)
 *   "hub_short_side"      SPARSE / DELTA stage B on observed hub rows: 1 = the members of row(u) and R_v are found from the
 *                         shorter list, 0 = every entry is tested against every probe, negative = by whether the call has a
 *                         bitmap row per probe (default)
 *   "bits_max_bytes"      SPARSE / DELTA stage B keeps a membership bitmap row per probe while a chunk's rows fit this many
 *                         bytes (default 128 MiB); larger calls give rows to their big probes only
 *   "pair_marks"          SPARSE / DELTA stage B: calls of at least this many (probe, observed) pairs per chunk -- and every
 *                         call too large for a membership bitmap -- find the affected pairs through a join over the
 *                         middle nodes; 0 = always, negative = never (default 2^22)
 *   "wide_min_hp"         smallest padded hidden width served by the batched stage-A kernel
 *   "tiled_big"           1 = the tiled SpMM uses its 64-bit gather offsets on any graph (test hook; default: S >= 4 GiB)
 *   "feature_delta"       fp64 product X*W1 of LT_MODE_DELTA from the differences of the feature rows to one reference row
 *                         (one pass over X when every column holds two values, as standardised indicator features do;
 *                         exact for any X): 0 = never, 1 = always try, negative = when lt_baseline_enable_fp64 found the
 *                         features to be of that kind (default).  The only knob that changes fp64 summation ORDER (the
 *                         results agree to ~1e-16 relative before the final rounding to fp32).
 *   "s1_f32"              feature-difference route with "defer_cref": 1 = the fp64-accumulated product rows are stored as 32-bit
 *                         fixed point with one scale per row (31 bits against the row's largest value; half the bytes the fp64
 *                         SpMM gathers) and the pre-activation in fp32 (default), 0 = both in fp64.  Moves `delta` results by
 *                         < 1e-6 of the largest score (plain fp32 rows moved them by up to 7e-5: DESIGN.md 5d)
 *   "delta_fused"         LT_MODE_DELTA on a graph with incidence records (lt_graph_create builds them for graphs of n <= 65534 nodes
 *                         without hub rows), calls whose pre-activation is formed on all rows: 1 = stage A and stage B of a probe in
 *                         ONE block, from the probe node's record matched against the observed list inside the pre-activation's
 *                         launch (default), 0 = the item kernels.  Bit-identical
 *   "records_early"       "delta_fused" route: 1 = the record blocks of a call's first probe chunk ride in the launch that forms the fp64
 *                         product rows whenever that launch runs (a refreshed baseline on the feature-difference route: CU slots to
 *                         spare, seven times the duration) (default), 0 = in the pre-activation's launch.  Bit-identical
 *   "feature_ring"        feature-difference route: the product rows by the persistent LDS-ring kernel (two workgroups per CU, a row in
 *                         flight by LDS-DMA ahead of the row a wave works on, rows claimed from counters; rows 8-byte aligned, W1 16-byte aligned,
 *                         H % 4 == 0, 2046 <= F <= 3326): 0 = never (one wave per row; default -- the ring form measured 25.6 us
 *                         against 22.0 at twitch size, profiles/r06_ring_lab.txt), 1 = whenever the shapes allow, negative = when
 *                         they do and the matrix has at least "feature_ring_min_rows" rows.  fp64 summation order only (as with
 *                         the "feature_delta" knob); a probe chunk's record blocks then ride in the pre-activation's launch
 *   "feature_ring_min_rows"   see "feature_ring" (default 1024, >= 2)
 *   "pair_list"           SPARSE / DELTA stage B on calls that find their affected pairs by the join over the middle nodes ("pair_marks"): 1 = the
 *                         marked pairs are compacted into a list, the result rows zero-filled, and the pair kernel walks the list (default;
 *                         calls whose list would exceed 256 MiB keep the other form), 0 = every pair's lane group reads its own mark.
 *                         Bit-identical
 *   "i8_split"            the fp64 product X*W1 of LT_MODE_DELTA on DENSE features (n >= 256, F >= 256, H a multiple of 64): 1 = as an
 *                         error-free integer split on the int8 matrix cores (X five, W1 four signed base-256 digits, fourteen digit
 *                         pairs, exact integer sums, one rounding per K slice: rows within 5e-10 of their largest value of the fp64
 *                         product; default), 0 = on the f64 matrix cores.  Results agree to < 1e-6 of the largest score
 *   "gcn3_product_gather" lt_influence3_rows, LT_MODE_DELTA: 1 = the probes' fp64 product rows X[v] W1 are read off the product the baseline
 *                         already holds for every row (default), 0 = formed again on the f64 matrix cores (as on the aggregate-first
 *                         route).  fp64 summation order / storage only: results agree to < 1e-6 of the largest score
 *   "export_sparse"       lt_influence_rows_f64 on the fused LT_MODE_DELTA route, calls that find the baseline refreshed: 1 = the first
 *                         rows of dst are zero-filled by a few waves riding in the launch that forms the fp64 product rows and in the
 *                         pre-activation's (np.zeros of attacker.py:216 crossing PCIe under those launches) and their probes' blocks
 *                         write the touched positions only; the other rows are widened whole by their blocks (default), 0 = all rows
 *                         are.  Bit-identical; so are the four keys below
 *   "export_zero_share"   per cent of dst's rows zero-filled under the product rows' launch (default 35; 0 .. 100)
 *   "export_zero_share2"  per cent of dst's rows, the next ones, zero-filled under the pre-activation's launch (default 15; 0 .. 100)
 *   "export_zero_blocks"  waves that zero-fill in each of the two launches (default 16; 1 .. 4096: more of them, or more stores in
 *                         flight, and the writes queued for the link hold up the loads of the kernels beside them)
 *   "export_zero_inflight"   1-KiB stores each such wave keeps in flight (default 4; 1 .. 64)
 *   "export_compact"      lt_influence_matrix_host on the fused LT_MODE_DELTA route: 1 = the touched values travel packed into pinned
 *                         staging (their indices into dst from the probes' record blocks, early in the step; their fp32 values from the
 *                         probes' blocks) while the host zero-fills dst, and the host places them after the stream wait, when the
 *                         graph's mean touched share of a row is below 0.25 (default), 0 = never (the route of
 *                         lt_influence_rows_f64), 2 = always.  Bit-identical
 *   "export_early"        ... packed calls of one probe chunk: 1 = after zero-filling dst the host looks (bounded by hipStreamQuery,
 *                         never waiting) for the index run the GPU publishes early in the step and, if it is there, walks it and asks
 *                         for the destination lines before the stream wait, 0 = everything after the wait (default: the look
 *                         shortens the section behind the wait by 1.6 us and costs the twitch-RU step 2.4), 2 = as 1, and the
 *                         indices the early look saw are compared with the finished run (lt_host_landing_stats).  Bit-identical.
 *                         Under "host_poll" = 1 the indices are always consumed before any wait; 1 then adds the walk ahead that
 *                         asks for the destination lines while the values are still out, 2 the comparison (and its wait)
 *   "host_poll"           ... packed calls of one probe chunk: 1 = the host places every value as soon as its word in the staging
 *                         block stops reading as the sentinel, and a call that consumed them all returns without the stream wait
 *                         (default; see lt_influence_matrix_host), 0 = the values are placed behind the wait.  Bit-identical
 *   "host_poll_sentinel"  the sentinel's 32-bit pattern (default 0xFFFFFFFF, a NaN no score is).  For tests: with the pattern of a
 *                         score the matrix holds, the call runs out of stall budget, waits for the stream and is still exact
 *   "feature_stagger"     feature-difference route, one wave per row: the row blocks start in (value & 255) groups, (value >> 8) x 10 ns
 *                         apart, so that a group walks its lists while the next one's rows arrive; 0 = all together.  Bit-identical
 *   "xf64_blocks"         aggregate-first route: blocks per XCD that walk the compacted work items of the rows a call reaches (default 96;
 *                         1 .. 4096).  Bit-identical
 *   "feature_lists"       feature-difference route, one wave per row: 1 = a refresh reads each row's differing columns from the lists
 *                         lt_baseline_enable_fp64 built (default: no pass over X), 0 = it lists them from X again (LT_FEATURE_LISTS)
 *   "feature_flags"       feature-difference route, one wave per row: 1 = a row's differing columns are found as flag bits (plain VALU)
 *                         and listed level by level (default: the kernel is bound by the issue of its compare steps), 0 = by a
 *                         ballot per value as in round 5.  Changes the order of a row's list: fp64 summation order only
 *   "defer_cref"          feature-difference route: 1 = the reference vector's product m W1 is formed by extra blocks of the rows'
 *                         launch and added by the readers of S1d (the fp64 SpMM, stage A) (default), 0 = formed first and added
 *                         by the rows kernel.  fp64 summation order only, like "feature_delta"
 *   "z_on_demand"         LT_MODE_DELTA on the S1d routes: 1 = the fp64 pre-activation is formed only on the rows a call's items
 *                         read (they stay valid until the next refresh), 0 = on all rows at the first call after a refresh,
 *                         negative = by the call's size (default: on demand when probes x average column length < n / 2 and the
 *                         whole fp64 SpMM is worth avoiding, nnz x hidden width >= 2.5e8: below that it is a 10 us launch)
 *   "stageb_rows"         SPARSE / DELTA stage B of calls with a membership bitmap and no pair marks: 1 = one block per (observed
 *                         node, slice of the probes), the observed row staged in LDS (default), 0 = one 8-lane group per pair
 *   "aggregate_first"     fp64 pre-activation of LT_MODE_DELTA as Z1d[r] = (A_hat X)[r] W1 + b1, computed only on the rows the
 *                         probes of a call reach (no n x F x H product): 0 = never, 1 = whenever the shapes allow (F <= 2 Hp,
 *                         F <= 512; set it before lt_baseline_enable_fp64 allocates), negative = then and when the features
 *                         are not sparse differences (default).  Like "feature_delta" it changes fp64 summation order only.
 *   "profile_every"       lt_profile_enable brackets every N-th launch group of an enabled class with events (default 1 = all of them)
 *   "probe_kslice"        K-slice of the perturbed-row GEMM; 0 = the slicing of the baseline X*W1 (default: S1'[v] and
 *                         S1[v] then share one summation order, like the reference's two torch.mm calls)
 * value = LT_TUNING_DEFAULT restores the default. */
#define LT_TUNING_DEFAULT (-0x7fffffffffffffffLL - 1)
int lt_set_tuning(const char *key, long long value);

/* ---- graph ------------------------------------------------------------------------------
 * Stands in for utils/load.py:552-559 (sparse_mx_to_torch_sparse_tensor) + the .cuda() at
 * worker.py:665-678: takes the normalised adjacency A_hat as HOST CSR (int32 indices,
 * fp32 values, columns strictly increasing inside each row), validates it, and uploads it
 * to the current device together with its transpose (CSC) used by the sparse/delta modes.
 * Graphs of up to 65534 nodes without hub rows (rows of more than 128 entries) also get their per-node incidence records
 * (LT_MODE_DELTA's fused route, "delta_fused"): sum over the nodes of |column| x the columns' lengths entries of 8 bytes,
 * built on the host in this call (twitch-RU: 1.5 M entries, 25 MB); skipped when a node has more than 4096 (dense clusters: the item kernels are faster there) or they pass 256 MB. */
int lt_graph_create(int32_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col,
                    const float *val, lt_graph **out);
int lt_graph_destroy(lt_graph *g);
int lt_graph_info(const lt_graph *g, int32_t *n, int64_t *nnz, int32_t *max_row_nnz);
/* The rows of at least min_entries entries that the probe nodes reach in one hop ({r : A_hat[r, v] != 0 for a probe v}), each once,
 * in no particular order: rows[0 .. *count) (device; capacity n), flags: device scratch of n int32 (overwritten).  What the ranks
 * of a multi-GPU run agree on (every rank runs it on the WHOLE probe list and sorts the result) before they split the hub rows
 * of the on-demand pre-activation between them (lt_baseline_form_rows_fp64 below). */
int lt_graph_reached_rows(const lt_graph *g, const int32_t *probes, int32_t n_probe, int32_t min_entries, int32_t *flags,
                          int32_t *rows, int32_t *count, void *stream);
/* Host only (no device call): the incidence records lt_graph_create would build for this CSR -- what tests/test_records.py pins
 * against a plain restatement.  meta [4 n]: per node (offset into rec in 32-bit words, items, touched nodes, incidences);
 * rec (may be NULL: sizes only): per node its items (row r, A_hat[r, v] as bits), then the touched nodes (u, first entry |
 * entries << 16), u ascending, then the entries (A_hat[u, r] as bits, item << 16 | position in row u) node by node in entry
 * order.  *rec_words: the words the records take.  LT_ERR_UNSUPPORTED when the graph gets none (hub rows, more than 65534
 * nodes, a node beyond the incidence cap, more than 256 MB), LT_ERR_WORKSPACE when rec_capacity (words) is too small. */
int lt_graph_records_host(int32_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col, const float *val,
                          int32_t *meta, int32_t *rec, int64_t rec_capacity, int64_t *rec_words);
/* The same graph from a CSR that already lies in DEVICE memory of the current device (d_rowptr [n + 1], d_col / d_val [nnz]): read in
 * stream order on `stream`, validated (the refusals and messages of lt_graph_create; rowptr is checked completely before anything
 * is read through it, a malformed input is refused and never dereferenced) and copied, so the graph owns its arrays.  Every derived
 * table is built by kernels; only rowptr, the column totals, the first column of each long-row segment and four counts per node visit
 * the host.  The call synchronises `stream` and returns a graph that equals lt_graph_create's for the same CSR word for word:
 * every kernel, baseline and trainer runs on it unchanged. */
int lt_graph_create_device(int32_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_col, const float *d_val, void *stream,
                           lt_graph **out);
/* Read-back of one table of a graph, for tests and tools (synchronous).  dst == NULL: *bytes = the table's size only; an optional
 * table the graph does not have reports 0 bytes; LT_ERR_WORKSPACE when capacity_bytes is too small.  All tables are int32 except
 * val / tval (float), cv (pairs of col, val bits) and LT_TABLE_SCALARS (LT_TABLE_SCALAR_COUNT doubles: n, nnz, max_row_nnz,
 * max_col_nnz, local_frac, hot_frac, p_n_long, p_n_seg, q_n_long, q_n_seg, w_n, dl_max_t, dl_max_tu, dl_touch_frac, tpos present,
 * cv present, records present).  col, val, tpos and cv carry their 16 zero pad entries; trow / tval hold nnz entries. */
typedef enum lt_graph_table_id {
    LT_TABLE_ROWPTR = 0,
    LT_TABLE_COL = 1,
    LT_TABLE_VAL = 2,
    LT_TABLE_TPTR = 3,
    LT_TABLE_TROW = 4,
    LT_TABLE_TVAL = 5,
    LT_TABLE_TPOS = 6,
    LT_TABLE_CV = 7,
    LT_TABLE_DL_META = 8,
    LT_TABLE_DL_REC = 9,
    LT_TABLE_P_LONG_ROW = 10,
    LT_TABLE_P_LONG_SEGPTR = 11,
    LT_TABLE_P_SEG_LONG = 12,
    LT_TABLE_P_SEG_BEGIN = 13,
    LT_TABLE_Q_LONG_ROW = 14,
    LT_TABLE_Q_LONG_SEGPTR = 15,
    LT_TABLE_Q_SEG_LONG = 16,
    LT_TABLE_Q_SEG_BEGIN = 17,
    LT_TABLE_W_E0 = 18,
    LT_TABLE_W_CNT = 19,
    LT_TABLE_W_DST = 20,
    LT_TABLE_SCALARS = 21,
    LT_TABLE_COUNT = 22
} lt_graph_table_id;
#define LT_TABLE_SCALAR_COUNT 17
int lt_graph_table(const lt_graph *g, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes);

/* ---- dense GEMM C[M,N] = A[M,K] * B[K,N]  (torch.mm at gcn/layers.py:31) ----------------
 * exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): each output is the ordered sum of k-ordered fmaf chains of 128 terms
 * (one chain per 128 k's, each started from +0: the rounding of a K = 3170 product stays at the level of a blocked CPU
 * sgemm, which is what keeps the fp32 finite difference of FULL / SPARSE inside the reference's own noise). */
int lt_gemm_f32(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                int32_t M, int32_t N, int32_t K, void *stream);

/* ---- SpMM out[n,ncols] = A_hat * S (+ bias) (ReLU)  (torch.spmm + bias at
 * gcn/layers.py:32-36, F.relu at gcn/models.py:20) ---------------------------------------
 * Any ncols (the reference has no width limit): columns are independent chains, so wide layers are served in slices of
 * 256 columns; the 16-byte vector path takes what is aligned (S / out / bias 16-byte aligned, lds and ldo multiples of
 * 4), a tail of ncols % 4 columns and unaligned operands go through an 8-lane kernel, 8 columns per launch.
 * Row-owned, fixed-order fmaf chains: deterministic and run-to-run reproducible.
 * lt_spmm_route: 1 when the call takes the tiled (column-sliced work-item) route on this graph, 0 for the row kernels. */
int lt_spmm_csr_f32(const lt_graph *g, const float *S, int64_t lds, int32_t ncols,
                    const float *bias_or_null, int32_t relu, float *out, int64_t ldo,
                    void *stream);
int lt_spmm_route(const lt_graph *g, int32_t ncols);

/* ---- 2-layer GCN forward (GCN.forward, gcn/models.py:19-24, eval mode) ------------------
 * logits[n,C] = A_hat * (relu(A_hat * (X*W1) + b1) * W2) + b2.   H <= 256, C <= 8.
 * logits is written with leading dimension ldl >= C (columns C .. ldl - 1 are left as they are).
 * lt_gcn2_workspace_bytes: size of the scratch the call needs (S1, S2, split-K partials). */
size_t lt_gcn2_workspace_bytes(int32_t n, int32_t F, int32_t H, int32_t C);
int lt_gcn2_forward(const lt_graph *g, const float *X, int64_t ldx, int32_t F,
                    const float *W1, const float *b1, int32_t H,
                    const float *W2, const float *b2, int32_t C,
                    float *logits, int64_t ldl, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ---- baseline state for the probe loop --------------------------------------------------
 * The reference recomputes model(features, adj) for every probe (attacker.py:106); it is
 * loop-invariant, so it is computed once here: S1 = X*W1, Z1 = A_hat*S1 + b1,
 * S2 = relu(Z1)*W2, OUT = A_hat*S2 + b2 -- lazily, by the first call that reads them (see lt_baseline_refresh).
 * Owns those four device buffers, the scratch of its hub rows and the side stream / events lt_influence_rows forks
 * hub-row work onto; borrows X, W1, b1, W2, b2 (needed again for the perturbed rows X'[v]*W1). */
int lt_baseline_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F,
                       const float *W1, const float *b1, int32_t H,
                       const float *W2, const float *b2, int32_t C,
                       void *stream, lt_baseline **out);
/* Adds an fp64-accumulated copy of the pre-activation Z1 (one more X*W1 on the f64 matrix cores +
 * one fp64 SpMM; redone after every lt_baseline_refresh when next needed).  LT_MODE_DELTA then evaluates the ReLU kink
 * test on it, which is what brings it within 1e-6 of an fp64 run of the reference; without it the
 * delta mode still works but entries that cross a kink carry ~1e-4 relative error.
 * Value domain: by default the product rows are kept as 31-bit fixed point against each ROW's largest value (dense and
 * feature-difference routes) and the int8 split cuts X / W1 to 39 / 31 bits against the largest value of a (row, K slice) /
 * (column, K slice); a stored error reaches a unit that crosses its kink divided by the perturbation.  Measured
 * (tests/test_value_domain_gpu.py): within 1e-5 of the largest score up to a 2^12 scale imbalance between hidden units or range
 * between feature columns; with a whole row of units at their kinks up to 4x (16x: up to 2.7e-5).  The aggregate-first
 * route keeps fp64 and has no such limit; "s1_f32" = 0 with "i8_split" = 0 lifts it on every route (<= 2.5e-7 at 2^20). */
int lt_baseline_enable_fp64(lt_baseline *b, void *stream);
/* The borrowed weights (same pointers) changed, e.g. once per benchmark step -- and so may have the contents of X, EXCEPT for a
 * baseline with the fp64 pre-activation on the feature-difference route (lt_baseline_fp64_route == 1): that baseline keeps the
 * lists of the columns in which each row of X differs from its reference vector, built by lt_baseline_enable_fp64, and changed
 * contents of X are announced to it by lt_baseline_features_changed instead.  Launches nothing: everything
 * derived from them is marked stale and recomputed by the first call that reads it, on THAT call's stream (a caller that
 * uses several streams orders them itself) -- S1 = X*W1 by LT_MODE_FULL / LT_MODE_SPARSE rows and lt_baseline_logits;
 * Z1 / S2 / OUT by SPARSE rows and lt_baseline_logits (FULL rows never need them: their stage A yields the unperturbed
 * layer as a by-product and stage B forms the baseline logits of the observed nodes itself); the fp64 pre-activation by
 * LT_MODE_DELTA rows, which then read nothing fp32 of the baseline (the probe's S1 row comes off the fp64 product). */
int lt_baseline_refresh(lt_baseline *b, void *stream);
/* The contents of X changed (same pointer, same shape): builds the difference lists of the feature-difference route again -- may
 * synchronise and allocate, like lt_baseline_enable_fp64 -- and marks stale everything lt_baseline_refresh marks stale.  Correct
 * on every route and without the fp64 pre-activation (it is then lt_baseline_refresh).  Additive within ABI 5. */
int lt_baseline_features_changed(lt_baseline *b, void *stream);
/* *entries = the number of (column, difference) entries in the baseline's difference lists, -1 when it keeps none (fp64 not
 * enabled, another route, a row with more differing columns than a wave's list holds, lists beyond a quarter of X's bytes). */
int lt_baseline_feature_list_entries(const lt_baseline *b, int64_t *entries);
/* Multi-GPU: the loop-invariant X*W1 sharded over ranks instead of replicated.
 * lt_baseline_attach_s1: the baseline reads S1 = X*W1 from caller-owned storage from now on ([>= n, Hp] fp32 with
 *   Hp = H rounded up to 4, ld == Hp; e.g. the torch tensor the ranks' all-gather writes); the current S1 is copied in.
 * lt_baseline_refresh_rows: like lt_baseline_refresh, but computes only rows [row_begin, row_end) of X*W1, into
 *   dst[row_end - row_begin, Hp] (typically the rank's send buffer of the all-gather).  Rows carry the same bits
 *   whichever rank computed them (the split-K slicing is that of the full product).  The rest of S1 is the caller's
 *   job; Z1 / S2 / OUT are marked stale exactly as by lt_baseline_refresh. */
int lt_baseline_attach_s1(lt_baseline *b, float *S1, int64_t ld, void *stream);
int lt_baseline_refresh_rows(lt_baseline *b, int32_t row_begin, int32_t row_end, float *dst, void *stream);
/* The fp64 twins (LT_MODE_DELTA with lt_baseline_enable_fp64 on): lt_baseline_attach_s1d hands the library caller-owned
 * storage for S1d = X*W1 in fp64 ([>= n, Hp] doubles, ld == Hp, 16-byte aligned: the output of the ranks' all-gather) and
 * switches the baseline to "S1d arrives from outside"; lt_baseline_refresh_rows_fp64 computes rows [row_begin, row_end)
 * of the fp64 product into dst[row_end - row_begin, Hp] (the rank's send buffer).  Same K slicing whatever the range, so a
 * row carries the same bits whichever rank computed it.  lt_baseline_fp64_route: 1 when the baseline's features were
 * found to be sparse differences to a reference row (two-valued columns, as standardised indicator features are) and
 * the fp64 product therefore costs one pass over X -- then sharding it buys nothing -- 0 when it runs on the f64
 * matrix cores, 2 when the pre-activation is formed aggregate-first on the rows a call needs (no S1d at all), -1 when fp64 is
 * not enabled. */
int lt_baseline_attach_s1d(lt_baseline *b, double *S1d, int64_t ld, void *stream);
int lt_baseline_refresh_rows_fp64(lt_baseline *b, int32_t row_begin, int32_t row_end, double *dst, void *stream);
int lt_baseline_fp64_route(const lt_baseline *b, int32_t *route);
/* For tests of the kernels that form them: the fp64 arrays of the S1d routes as they stand, copied on `stream` to caller buffers the
 * device can write.  LT_ERR_UNSUPPORTED on the aggregate-first route (no product rows), and while the product is stale: between
 * lt_baseline_refresh and the next call that re-forms it (any LT_MODE_DELTA call).  lt_baseline_enable_fp64 forms the product itself,
 * so straight after it the call succeeds with the product rows and cref in place and NO pre-activation row formed yet (forms[2] = 0,
 * every state word 0); the pre-activation is formed by the LT_MODE_DELTA calls, for all rows or for the rows a call reads.
 * product: [n, Hp] the product rows -- forms[0] = 1: 32-bit fixed point (int32) with the rows' scales in scales[n], forms[0] = 0:
 * doubles (scales untouched); size it for doubles.  preact: [n, Hp] the pre-activation -- forms[1] = 1: fp32, 0: doubles; size it
 * for doubles.  row_state: [n] the rows' state words (1 = the row of preact is valid), meaningful when forms[2] = 0; forms[2] = 1:
 * every row of preact is valid.  forms[3] = 1: the product rows lack the reference vector's product (deferred cref).  cref: [Hp]
 * that product m W1 of the feature-difference route as the refresh formed it, forms[4] = 1 (0 on the other route: cref untouched).
 * forms: int32[5], host memory, written before the call returns.  Additive within ABI 5. */
int lt_baseline_fp64_arrays(const lt_baseline *b, void *product, double *scales, double *cref, void *preact, int32_t *row_state,
                            int32_t *forms, void *stream);
/* The on-demand route by ROW LIST (lt_baseline_fp64_route == 2; LT_ERR_UNSUPPORTED otherwise): a call of lt_influence_rows forms
 * the fp64 pre-activation Z1d on the rows ITS probes reach.  On a heavy-tailed graph most of that work lies in hub rows every
 * rank's probes reach (BASELINE configs[4], 8 ranks x 512 probes: ~3 800 rows of >= 1 024 entries hold 84 % of a rank's gathers,
 * and they are the same rows on every rank).  Every rank knows the whole probe list (attacker.py:220: one list), so the ranks
 * can split those rows: each forms its share (lt_baseline_form_rows_fp64: the listed rows now; rows valid since the last refresh
 * are skipped), packs it (lt_baseline_gather_rows_fp64: dst[i, 0 .. Hp) = Z1d[rows[i]], the send buffer of ONE all-gather) and
 * adopts everybody's (lt_baseline_scatter_rows_fp64: Z1d[rows[i]] = src[i, 0 .. Hp), marked valid).  The calls of
 * lt_influence_rows that follow skip valid rows.  A row's bits do not depend on who formed it.  rows: device int32 lists (ids out
 * of range are skipped); dst / src: device, [n_rows, Hp] doubles, 16-byte aligned; Hp = H rounded up to 4. */
int lt_baseline_form_rows_fp64(lt_baseline *b, const int32_t *rows, int32_t n_rows, void *stream);
int lt_baseline_gather_rows_fp64(lt_baseline *b, const int32_t *rows, int32_t n_rows, double *dst, void *stream);
int lt_baseline_scatter_rows_fp64(lt_baseline *b, const int32_t *rows, int32_t n_rows, const double *src, void *stream);
int lt_baseline_destroy(lt_baseline *b);
/* copies the baseline logits OUT [n, C] (dense, ld = C) to a device buffer */
int lt_baseline_logits(const lt_baseline *b, float *dst, void *stream);

/* ---- the probe primitive: rows of the influence matrix ----------------------------------
 * Stands in for Attacker.get_gradient_eps_mat + the inner j-loop of
 * link_prediction_attack_efficient (attacker.py:100-108, 220-229):
 *   out[i*ldo + j] = || (f(X + delta * e_v x_v^T) - f(X))[u_j] ||_2 / delta,
 *   v = probe_nodes[i], u_j = observe_nodes[j]
 * probe_nodes / observe_nodes / out are device pointers.  One call handles any n_probe
 * (internally chunked so the workspace stays bounded); no host synchronisation. */
size_t lt_influence_workspace_bytes(const lt_baseline *b, int32_t n_probe, int32_t n_obs,
                                    int32_t mode);
int lt_influence_rows(const lt_baseline *b, const int32_t *probe_nodes, int32_t n_probe,
                      const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode,
                      float *out, int64_t ldo, void *workspace, size_t workspace_bytes,
                      void *stream);

/* Node ids arrive as DEVICE lists, which the host side of this ABI cannot read: the first kernel of a call that touches a list
 * checks every id against [0, n) -- where the reference raises IndexError at grad_mat[test_nodes[j]] / features[v]
 * (attacker.py:103, 226-229) -- replaces an id out of range by node 0 for the rest of the call (no out-of-bounds access;
 * the rows / columns of such ids are meaningless) and raises a flag in mapped host memory.  The flag is reported
 *   - by lt_node_check: *bad_probe / *bad_observe (may be NULL) = 1 when a list of a call whose kernels have COMPLETED held such
 *     an id (call it after synchronising the stream); clears the flag; returns LT_ERR_INDEX when either is set;
 *   - by the next lt_influence_rows / _vec / lt_influence3_rows* call that finds it set: LT_ERR_INDEX, nothing enqueued. */
int lt_node_check(int32_t *bad_probe, int32_t *bad_observe);

/* ---- the probe primitive over a LIST of pairs -------------------------------------------------------------------------
 * Stands in for Attacker.get_gradient_eps + the loops of link_prediction_attack (attacker.py:89-97, 143-163) and for the
 * per-node partner lists of link_prediction_attack_efficient_balanced (attacker.py:250-284): callers that read a few dozen
 * pairs per probe, not a rectangle.  Pairs are grouped by probe: probe i = probe_nodes[i] owns
 * pair_obs[pair_ptr[i] .. pair_ptr[i + 1]), and
 *   out[k] = || (f(X + delta * e_v x_v^T) - f(X))[u] ||_2 / delta,   v = the probe that owns k, u = pair_obs[k]
 * -- the value lt_influence_rows writes at (v, u) for the same mode, bit for bit.  A probe may own no pair, probes may
 * repeat, u == v is allowed, a pair may be listed twice.  probe_nodes / pair_obs / out are device pointers; out holds n_pairs
 * floats.  pair_ptr is a HOST array of n_probe + 1 offsets: the call reads it while it runs -- it is validated before anything
 * is launched (pair_ptr[0] == 0, non-decreasing, pair_ptr[n_probe] == n_pairs, not NULL unless n_pairs == 0: LT_ERR_INVALID)
 * and gives every probe chunk its range of pairs by value -- and sends it to the device with one stream-ordered copy: pageable
 * memory may be released when the call returns, pinned memory once the stream has passed that copy.
 * Everything else follows lt_influence_rows: enqueue only; node ids checked on the device (LT_ERR_INDEX / lt_node_check;
 * bad_observe covers pair_obs); probes chunked by "chunk_budget_bytes".  The workspace holds the item tables of one probe
 * chunk, the checked lists and the offsets -- nothing of the size of n_probe x (nodes observed) -- and out is sized by the list.
 * Modes: LT_MODE_DELTA as in lt_influence_rows (the fp64 kink test with lt_baseline_enable_fp64 on); LT_MODE_SPARSE;
 * LT_MODE_FULL is accepted and EVALUATED AS LT_MODE_SPARSE -- the two are bit-identical (see above), and a pair list has no use
 * for FULL's all-rows stage A.  n_pairs == 0 or n_probe == 0: LT_OK, nothing launched.  At most 2^31 - 65537 pairs per call.
 * The 2-layer lt_baseline only (H <= 256, C <= 8). */
size_t lt_influence_pairs_workspace_bytes(const lt_baseline *b, int32_t n_probe, int64_t n_pairs, int32_t mode);
int lt_influence_pairs(const lt_baseline *b, const int32_t *probe_nodes, int32_t n_probe,
                       const int64_t *pair_ptr, const int32_t *pair_obs, int64_t n_pairs,
                       float delta, int32_t mode, float *out, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---- the finished rows, once, as float64 ------------------------------------------------------------------------------
 * Stands in for influence_val = np.zeros((n_test, n_test)) (float64, attacker.py:216) and the n_test^2 `.norm().item()` host
 * round trips that fill it (attacker.py:227-229): dst[i * ldd + j] = (double)src[i * lds + j] by one launch.  src: device
 * [rows, lds] fp32 (what lt_influence_rows wrote).  dst: device memory, or PINNED host memory (hipHostMalloc /
 * hipHostRegister, e.g. a torch tensor with pin_memory=True): the kernel then writes over PCIe through the buffer's
 * device-side alias -- no staging copy, no second operation on the stream; the bytes are valid on the host once the stream has
 * drained.  Pageable host pointers are refused (LT_ERR_INVALID). */
int lt_export_rows_f64(const float *src, int64_t lds, int32_t rows, int32_t cols, double *dst, int64_t ldd, void *stream);

/* lt_influence_rows and lt_export_rows_f64 in ONE call: out ([n_probe, ldo] fp32, device) is written as by lt_influence_rows, and
 * dst[i * ldd + j] = (double)out[i * ldo + j] -- the reference's influence_val (attacker.py:216, 227-229) -- in device memory or
 * PINNED host memory (as lt_export_rows_f64).  On the fused LT_MODE_DELTA route (graphs with incidence records) every probe's
 * block writes its own finished row into dst and no export launch follows; when the call also recomputes the baseline (it
 * follows an lt_baseline_refresh) the first half of dst's rows is zero-filled by a few waves riding in the launches that form
 * the fp64 product rows and the pre-activation -- np.zeros crossing PCIe under kernels that do not touch the link -- and the
 * blocks of those rows send their touched positions only (tuning keys "export_sparse", "export_zero_*").  Every other route
 * ends with the launch lt_export_rows_f64 makes.  Same values as the two calls, bit for bit. */
int lt_influence_rows_f64(const lt_baseline *b, const int32_t *probe_nodes, int32_t n_probe,
                          const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode,
                          float *out, int64_t ldo, double *dst, int64_t ldd, void *workspace, size_t workspace_bytes,
                          void *stream);

/* lt_influence_rows_f64 into PINNED host memory, and the wait: returns once dst[i * ldd + j] holds the float64 matrix (the
 * reference's influence_val, attacker.py:213 -> 231); columns n_obs .. ldd - 1 are left as they are.  Same arguments, checks and
 * LT_ERR_INDEX behaviour as lt_influence_rows_f64; out is written as by lt_influence_rows.  On the fused LT_MODE_DELTA route
 * ("export_compact") the matrix's zeros do not cross PCIe: the touched values travel packed into a pinned staging block the
 * baseline owns (allocated on first use, worst-case size, freed by lt_baseline_destroy) -- 4 bytes of index per value early in
 * the step, as soon as the probes' records are matched, 4 bytes of value from the probes' blocks at its end -- the host zero-fills
 * dst while the GPU computes and, in a call of one probe chunk ("host_poll"), places each value as it lands: the value words of
 * the staging block hold a sentinel between calls, every touched position gets exactly one 4-byte store, so a word that no
 * longer reads as the sentinel is final.  A call that consumed the whole run this way returns WITHOUT waiting for the stream:
 *   - dst holds the complete matrix, and a node-id flag raised by the call's lists is in host memory (lt_node_check may follow);
 *   - the stream may still be retiring the last launch's tail: `out` is ordered for later users by the stream, as after
 *     lt_influence_rows, and an asynchronous error of that tail surfaces at the stream's next wait, not from this call.
 *   - so what was safe only because the call used to be fully synchronous no longer is: the next call on this baseline must go
 *     to the SAME stream (or behind a wait of the caller's own), and `out` or the workspace may be freed only by a stream-ordered
 *     allocator or behind such a wait -- else it races with the last launch's tail.  "host_poll" = 0 restores the old behaviour.
 * The host's stalls are bounded (200 us in all, counted in looks and clock reads): beyond that the call waits for the stream
 * once, reports its error, and places the rest behind the wait -- so does a call of several chunks or with "host_poll" = 0, and a
 * score that happens to equal the sentinel costs that one wait and nothing else.  Every call that is not packed is
 * lt_influence_rows_f64 followed by the wait.  Same values, bit for bit.  Like every call on a baseline handle, not thread-safe. */
int lt_influence_matrix_host(const lt_baseline *b, const int32_t *probe_nodes, int32_t n_probe,
                             const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode,
                             float *out, int64_t ldo, double *dst, int64_t ldd, void *workspace, size_t workspace_bytes,
                             void *stream);

/* One host-landed step in ONE call: lt_baseline_refresh (on request), lt_influence_matrix_host and lt_node_check.  The arguments
 * of lt_influence_matrix_host, then
 *   flags        LT_STEP_REFRESH: mark the baseline stale exactly as lt_baseline_refresh does -- behind every check that stands in
 *                front of the first launch (arguments, a pending node-id flag, the workspace, dst): a call refused by one of
 *                those enqueued nothing and marked nothing.  (The grid-limit checks of the probe chunks come later: a call
 *                they refuse has run the launches that recompute the baseline, and the refresh is spent.)
 *                LT_STEP_DST_PINNED: the caller vouches that dst is pinned host memory it allocated.  On the packed route only
 *                the host touches dst, and the runtime is then not asked what kind of pointer it is; on every route where
 *                the GPU writes dst it is resolved as lt_influence_matrix_host resolves it, flag or no flag.
 *   bad_probe, bad_observe   optional: behind the wait (or, in a call that placed its values by look and did not wait, behind the
 *                last value: the launches that raise the flag had ended by then) the node-id flag is read and cleared as by lt_node_check.  A flag raised
 *                by THIS call's lists returns LT_ERR_INDEX from this call with the two words filled (1 = that list held an id
 *                outside [0, n)); the matrix of such a call is meaningless.  Both are 0 after any other return -- also when
 *                the call is refused on entry with LT_ERR_INDEX because an EARLIER call left its flag uncollected (that
 *                report clears the flag, as in every probe call; nothing was enqueued).
 * LT_ERR_WORKSPACE: nothing was enqueued and nothing marked stale; lt_last_error names the size needed.  Counted by
 * lt_host_landing_stats like lt_influence_matrix_host.  Same values as the three calls, bit for bit.  Additive in ABI 5. */
#define LT_STEP_REFRESH 1
#define LT_STEP_DST_PINNED 2
int lt_influence_step_host(const lt_baseline *b, const int32_t *probe_nodes, int32_t n_probe,
                           const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode,
                           float *out, int64_t ldo, double *dst, int64_t ldd, void *workspace, size_t workspace_bytes,
                           void *stream, int32_t flags, int32_t *bad_probe, int32_t *bad_observe);

/* The packed calls of lt_influence_matrix_host / lt_influence_step_host on this baseline so far: out4[0] = calls that made the
 * "export_early" look (the index run walked ahead of its values), [1] = the other packed calls, [2] = nanoseconds the host spent
 * placing -- between the wait's return and the matrix being complete, or, for a call that placed by look ("host_poll"), from the
 * end of its zero-fill to the complete matrix -- summed over both, [3] = ("export_early" = 2) index words the early look saw
 * differently from the finished run -- anything but 0 means the publication is broken.  Additive in ABI 5. */
int lt_host_landing_stats(const lt_baseline *b, int64_t *out4);
/* ... and of those calls: out4[0] = calls that placed their values by look ("host_poll"), [1] = those of them that ran out of
 * stall budget and finished behind the stream wait, [2] = stalled looks (loads that found the ready word or a value word not
 * yet there; in the rounds over the entries passed over: every entry a round rescanned and left pending), [3] = entries whose
 * first look found them not yet there.  The stall budget is coarse: the clock is read every 1 024 looks, and while entries are
 * pending it runs on all time, placing included -- about 250 us pass before a fallback.  Additive in ABI 5. */
int lt_host_landing_stats2(const lt_baseline *b, int64_t *out4);

/* ---- measurement support: the gather ceiling of the tiled SpMM ------------------------------------------------------
 * The tiled (column-sliced work-item) kernel of lt_spmm_csr_f32 with everything but its gathers removed: the same work
 * items, order, column stream, slice placement and piece size, `in_flight` (8 = the kernel's own, or 16) gathers per lane;
 * no values, no arithmetic, no result rows.  Its duration bounds from below ANY row-gather SpMM that issues this index
 * stream -- what bench.py reports as roofline_spmm.gather_ceiling next to the kernel it bounds.  `sink`: device scratch
 * of lt_spmm_gather_ceiling_bytes(g) bytes (one word per item and slice keeps the loads alive).  `out` != NULL ([n, ldo]
 * fp32): the result rows are stored as the real kernel stores them (their content is meaningless): gathers + result stores. */
size_t lt_spmm_gather_ceiling_bytes(const lt_graph *g);
int lt_spmm_gather_ceiling(const lt_graph *g, const float *S, int64_t lds, int32_t ncols, int32_t in_flight,
                           void *sink, size_t sink_bytes, float *out, int64_t ldo, void *stream);

/* ---- layers wider than one pass of the fused kernels (hidden > 256 or > 8 classes) ------------------------------------
 * The reference has no width limit (gcn/layers.py:14-36, main.py:30 --hidden).  The perturbation's effect on the logits is
 * a SUM over the hidden units, so a wide model is served slice by slice: for every slice s of <= 256 hidden units and every
 * slice t of <= 8 classes a baseline on (W1[:, s], b1[s], W2[s, t], b2[t]) and one
 *   lt_influence_rows_vec   = lt_influence_rows that also writes the pair's difference VECTOR, unscaled:
 *                             vec[(i * ldo + j) * C_t + c] = (f_s(X + d e_v x_v^T) - f_s(X))[u_j, c]   (LT_MODE_SPARSE: the fp32
 *                             finite difference of the slice's own forward; LT_MODE_DELTA: the propagated difference; exact zeros
 *                             outside the probe's 2-hop set in both).  FULL has no vector form (it names SPARSE's bits).
 * and per class slice one
 *   lt_wide_combine         d_c = (vec_0 + vec_1 + ... )[c] / delta in slice order, ss = fma(d_c, d_c, ss) in class order on top of
 *                             the running ss[pair] of the previous class slices (first != 0: start from 0), and on the last class
 *                             slice (last != 0) ss[pair] <- sqrt(ss[pair]): the influence score of attacker.py:227-229.
 * vecs: HOST array of n_vec device pointers, each [n_pairs, C] dense.  Launch count per matrix: ~5 per (s, t) + one per t,
 * independent of n_probe (the round-3 route looped ~5 launches per PROBE). */
int lt_influence_rows_vec(const lt_baseline *b, const int32_t *probe_nodes, int32_t n_probe,
                          const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode,
                          float *out, int64_t ldo, float *vec, void *workspace, size_t workspace_bytes,
                          void *stream);
int lt_wide_combine(const float *const *vecs, int32_t n_vec, int64_t n_pairs, int32_t C, float delta,
                    float *ss, int32_t first, int32_t last, void *stream);

/* ---- the same for the 3-layer model (GCN3, gcn/models.py:28-46; --n-layer 3, gcn_trainer.py:81-86) -------------
 *   logits = A (relu(A (relu(A (X W1) + b1) W2) + b2) W3) + b3,   H1, H2 <= 256, C <= 8 (C <= 256: lt_baseline3_create_wide).
 * lt_baseline3_create owns the unperturbed forward (S1, H1, S2, Z2, S3, OUT) and borrows X and the six parameter tensors;
 * lt_baseline3_refresh marks everything stale and launches nothing: the next reader recomputes what IT reads on its own stream
 * (a LT_MODE_DELTA build the fp64 pre-activations only, the fp32 modes and lt_baseline3_logits the fp32 forward).  lt_influence3_rows evaluates the
 * reference's fp32 finite difference (f(X + d e_v x_v^T) - f(X))[u] / d only where it can be non-zero: the rows a
 * probe reaches in 1, 2 and 3 hops, each recomputed with the arithmetic of the baseline forward, so unreachable
 * pairs are exactly 0.  The conventions of lt_influence_rows (enqueue only, no host synchronisation: the item
 * count that sizes the level-2 GEMM stays on the device). */
typedef struct lt_baseline3 lt_baseline3;
int lt_baseline3_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F,
                        const float *W1, const float *b1, int32_t H1,
                        const float *W2, const float *b2, int32_t H2,
                        const float *W3, const float *b3, int32_t C,
                        void *stream, lt_baseline3 **out);
/* The same handle for a WIDE class layer (reddit's 41 classes, ppi's 121 labels: what lt_gcn3_trainer_create_wide trains):
 * H1, H2 <= 256 and 1 <= C <= 256; same arguments, same handle type, LT_ERR_UNSUPPORTED beyond.  refresh, features_changed,
 * enable_fp64 and destroy work as on a narrow handle (the fp64 pre-activations do not depend on C); lt_baseline3_logits forms
 * the last layer by the unfused product and SpMM (lt_gemm_f32 / lt_spmm_csr_f32's kernels: fp32 rounding only).
 * MODE RULE of a wide handle: lt_influence3_rows_mode serves LT_MODE_DELTA alone -- levels 1 and 2 of the narrow chain, then
 * dS3x = dH2x W3 as one MFMA product over the level-2 items (their count stays on the device) and the observed rows with a
 * lane group across the class columns.  LT_MODE_SPARSE / LT_MODE_FULL and lt_influence3_rows return LT_ERR_UNSUPPORTED and
 * enqueue nothing: the fp32 finite difference of these shapes is the caller's loop over lt_gemm_f32 / lt_spmm_csr_f32.  A cell
 * depends on (probe, observed, model, graph) alone, not on the chunking or the other nodes of the call; no floating-point
 * atomics.  Everything else as for a narrow handle: enqueue only, ids checked on the device (lt_node_check), probes chunked
 * by "chunk_budget_bytes" -- the level-2 tables are sized by n rows per probe, so a large graph gets small chunks.
 * C <= 8 is allowed here and takes the wide kernels all the same. */
int lt_baseline3_create_wide(const lt_graph *g, const float *X, int64_t ldx, int32_t F,
                             const float *W1, const float *b1, int32_t H1,
                             const float *W2, const float *b2, int32_t H2,
                             const float *W3, const float *b3, int32_t C,
                             void *stream, lt_baseline3 **out);
int lt_baseline3_refresh(lt_baseline3 *b, void *stream);
/* lt_baseline_features_changed for the inner 2-layer baseline, and everything lt_baseline3_refresh marks stale. */
int lt_baseline3_features_changed(lt_baseline3 *b, void *stream);
int lt_baseline3_destroy(lt_baseline3 *b);
int lt_baseline3_logits(const lt_baseline3 *b, float *dst, void *stream);
size_t lt_influence3_workspace_bytes(const lt_baseline3 *b, int32_t n_probe, int32_t n_obs);
int lt_influence3_rows(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe,
                       const int32_t *observe_nodes, int32_t n_obs, float delta,
                       float *out, int64_t ldo, void *workspace, size_t workspace_bytes, void *stream);
/* The same with a mode: LT_MODE_SPARSE (= LT_MODE_FULL here: lt_influence3_rows, the fp32 finite difference on the 3-hop set)
 * or LT_MODE_DELTA -- the perturbation propagated exactly through the three layers (no subtraction of nearly equal numbers;
 * the two ReLU kink tests read fp64-accumulated pre-activations), which needs lt_baseline3_enable_fp64 first: an fp64 copy of
 * the first two layers' pre-activations (the layer-1 product takes the routes of lt_baseline_enable_fp64), recomputed after
 * every lt_baseline3_refresh when next needed. */
int lt_baseline3_enable_fp64(lt_baseline3 *b, void *stream);
int lt_influence3_rows_mode(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe,
                            const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode,
                            float *out, int64_t ldo, void *workspace, size_t workspace_bytes, void *stream);

/* The probe primitive of the 3-layer model over a LIST of pairs: the contract of lt_influence_pairs for a lt_baseline3 handle.
 * Pairs are grouped by probe: probe i = probe_nodes[i] owns pair_obs[pair_ptr[i] .. pair_ptr[i + 1]), and out[k] is the value
 * lt_influence3_rows_mode writes at (the probe that owns k, pair_obs[k]) for the same mode, BIT FOR BIT -- levels 1 and 2 of a
 * probe chunk are the launches of the rows call, and the observed-row kernels run the same per-cell device function for pair k
 * that the rectangle kernels run for cell (b, j); a lane group finds its probe by a binary search in the chunk's offsets.  A
 * probe may own no pair, probes may repeat, u == v is allowed, a pair may be listed twice.  probe_nodes / pair_obs / out are
 * device pointers; out holds n_pairs floats.  pair_ptr is a HOST array of n_probe + 1 int64 offsets: it is validated before
 * anything is launched (pair_ptr[0] == 0, non-decreasing, pair_ptr[n_probe] == n_pairs, not NULL unless n_pairs == 0:
 * LT_ERR_INVALID, nothing launched or written), gives every probe chunk its range of pairs by value, and reaches the device by
 * one stream-ordered copy: pageable memory may be released when the call returns, pinned memory once the stream has passed that
 * copy.  Modes as in lt_influence3_rows_mode: a narrow handle serves LT_MODE_SPARSE, LT_MODE_DELTA and LT_MODE_FULL (evaluated
 * as SPARSE: the same quantity for this model); a wide handle LT_MODE_DELTA alone (LT_ERR_UNSUPPORTED otherwise, nothing
 * enqueued); DELTA needs lt_baseline3_enable_fp64.  n_pairs == 0 or n_probe == 0: LT_OK, nothing launched.  At most
 * 2^31 - 65537 pairs per call.  Enqueue only, no host synchronisation; node ids checked on the device (LT_ERR_INDEX /
 * lt_node_check; bad_observe covers pair_obs; a pending flag of an earlier call refuses this one); probes chunked by
 * "chunk_budget_bytes" exactly as the rows call chunks them.  A chunk whose probes own no pair launches NOTHING: its levels 1
 * and 2 are skipped with its observed rows.  The workspace holds the level-1 / level-2 tables of one probe chunk, the two checked
 * lists and the offsets -- nothing of the size of n_probe x (nodes observed):
 *   lt_influence3_pairs_workspace_bytes(b, P, M) <= lt_influence3_workspace_bytes(b, P, 1) + 4 M + 8 (P + 1) + 512,
 * whatever nodes the list names.  The query returns 0 for invalid arguments. */
size_t lt_influence3_pairs_workspace_bytes(const lt_baseline3 *b, int32_t n_probe, int64_t n_pairs);
int lt_influence3_pairs(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe,
                        const int64_t *pair_ptr, const int32_t *pair_obs, int64_t n_pairs,
                        float delta, int32_t mode, float *out, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ---- the 2-layer model with a WIDE class layer (GCN, gcn/models.py:8-25, with reddit's 41 classes or ppi's 121 labels: what
 * lt_gcn2_trainer_create_wide trains) through one handle ----------------------------------------------------------------------
 *   logits = A (relu(A (X W1) + b1) W2) + b2,   H <= 256 and 1 <= C <= 256 (LT_ERR_UNSUPPORTED beyond, *out = NULL).
 * C <= 8 is allowed and takes the wide kernels all the same.  The handle borrows X and the four parameter tensors and owns,
 * from creation, the fp64 parts LT_MODE_DELTA reads: an inner lt_baseline over (X, W1, b1) whose fp64 pre-activation and product
 * rows take the routes of lt_baseline_enable_fp64 -- there is no enable call.  lt_baseline2w_refresh marks everything stale and
 * launches nothing: the next reader re-forms what IT reads on its own stream (the probe calls the fp64 pre-activation alone,
 * lt_baseline2w_logits the fp32 forward: the unfused product and SpMM, lt_gemm_f32 / lt_spmm_csr_f32's kernels, allocated by
 * its first call).  lt_baseline2w_features_changed is lt_baseline_features_changed for the inner baseline.
 * MODE RULE: LT_MODE_DELTA alone.  For two layers the class width enters only behind the single ReLU kink test, so the chain is
 * the wide chain of lt_baseline3_create_wide with one level removed: per probe chunk the probes' fp64 product rows, the level-1
 * bitmap with positions, dH1 = relu(Z1 + A[r,v] d S1[v]) - relu(Z1) piecewise on the fp64 pre-activation, dS2x = dH1x W2 as ONE
 * MFMA product over the items (their count stays on the device; rows of stride C rounded up to 4) and the observed rows with a
 * lane group across the class columns -- the wide chain's own kernels, handed the level-1 tables: row u's entries in entry
 * order, the members of R1 add fma(a, dS2x[pos][c], acc), / delta, the squares in one fixed order, sqrt.  No floating-point
 * atomics; a cell no path reaches is exactly +0; the pad columns are carried along and never enter the squares.
 * LT_MODE_SPARSE / LT_MODE_FULL return LT_ERR_UNSUPPORTED and enqueue nothing: the fp32 finite difference of these shapes
 * stays lt_influence_rows_vec + lt_wide_combine over class slices.
 * lt_influence2w_rows: the contract of lt_influence3_rows_mode -- enqueue only, no host synchronisation; a cell depends on
 * (probe, observed, model, graph) alone, not on the chunking, the other nodes of the call or the run; node ids checked on the
 * device into copies (lt_node_check / LT_ERR_INDEX; a bad id is replaced, never dereferenced); probes chunked by
 * "chunk_budget_bytes" -- the per-probe tables are sized by the longest column of A_hat, not by n, so chunks are large;
 * n_probe == 0 or n_obs == 0: LT_OK, nothing launched; a short or misaligned workspace: LT_ERR_WORKSPACE.
 * lt_influence2w_pairs: the contract of lt_influence3_pairs -- out[k] is, BIT FOR BIT, what the rows call writes at (the probe
 * that owns k, pair_obs[k]); pair_ptr is a HOST array of n_probe + 1 int64 offsets validated before anything is launched
 * (LT_ERR_INVALID, nothing written); a chunk whose probes own no pair launches nothing; n_pairs == 0: LT_OK; and
 *   lt_influence2w_pairs_workspace_bytes(b, P, M) <= lt_influence2w_workspace_bytes(b, P, 1) + 4 M + 8 (P + 1) + 512.
 * The workspace queries return 0 for invalid arguments.  lt_baseline2w_logits writes a dense [n, C] matrix. */
typedef struct lt_baseline2w lt_baseline2w;
int lt_baseline2w_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F,
                         const float *W1, const float *b1, int32_t H,
                         const float *W2, const float *b2, int32_t C,
                         void *stream, lt_baseline2w **out);
int lt_baseline2w_refresh(lt_baseline2w *b, void *stream);
int lt_baseline2w_features_changed(lt_baseline2w *b, void *stream);
int lt_baseline2w_destroy(lt_baseline2w *b);
int lt_baseline2w_logits(const lt_baseline2w *b, float *dst, void *stream);
size_t lt_influence2w_workspace_bytes(const lt_baseline2w *b, int32_t n_probe, int32_t n_obs);
int lt_influence2w_rows(const lt_baseline2w *b, const int32_t *probe_nodes, int32_t n_probe,
                        const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode,
                        float *out, int64_t ldo, void *workspace, size_t workspace_bytes, void *stream);
size_t lt_influence2w_pairs_workspace_bytes(const lt_baseline2w *b, int32_t n_probe, int64_t n_pairs);
int lt_influence2w_pairs(const lt_baseline2w *b, const int32_t *probe_nodes, int32_t n_probe,
                         const int64_t *pair_ptr, const int32_t *pair_obs, int64_t n_pairs,
                         float delta, int32_t mode, float *out, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ---- LapGraph cell selection (worker.py:302-335: A += noise, the n_keep largest cells of the strict lower
 * triangle by a 50-way np.argpartition) --------------------------------------------------------------------------------
 * The noise stays numpy's (stream compatibility with --noise-seed): the host draws the N x N float64 matrix and uploads
 * it as `cells` (device, [n, n], only j < i is read; overwritten with adjacency + noise).  lower_rowptr / lower_col:
 * device CSR of the 0/1 adjacency (entries with j >= i are ignored).  The call adds 1.0 on the edges (the reference's fp64
 * add), radix-selects the n_keep-th largest key and writes the flat indices i * n + j of the selected cells to out_idx
 * ([n_keep] int64, device, unordered).  work: >= 4096 bytes of device scratch.  threshold_out (host, may be NULL): the
 * n_keep-th largest value.  Synchronises the stream.  The selected set equals np.argpartition's unless the threshold
 * value is tied; a threshold <= 0 (the selection would reach the zero cells of the upper triangle, where the reference
 * asserts) returns LT_ERR_UNSUPPORTED. */
int lt_lapgraph_select(int32_t n, const int32_t *lower_rowptr, const int32_t *lower_col, double *cells, int64_t n_keep,
                       int64_t *out_idx, void *work, size_t work_bytes, double *threshold_out, void *stream);

/* ---- edge-DP noise from a counter-based stream: LapGraph and EdgeRand without an N x N matrix ------------
 * lt_lapgraph_select above needs numpy's N x N draw.  The functions below evaluate a documented Philox4x32-10 stream per cell on
 * the device instead: the noise is never stored, the selection needs O(kept edges) memory.  A given seed gives a DIFFERENT
 * graph than numpy's stream does; the stream is this contract, as the dropout mask is the trainers':
 *   cell      a strict-lower-triangle pair (i, j), j < i, with the linear index t = i (i - 1) / 2 + j (64 bits)
 *   block     q = t >> 1; counter (q & 0xffffffff, q >> 32, stream, 0), key (seed & 0xffffffff, seed >> 32) -> words w[0 .. 3];
 *             cell t takes a = w[2 (t & 1)] and b = w[2 (t & 1) + 1]
 *   stream    0: LapGraph's cell noise, 1: LapGraph's edge-count draw (cell 0 only; drawn by the host), 2: EdgeRand
 *             (3: the non-edge draws of lt_sample_balanced_philox, which are indexed by draw and not by cell; stated there)
 *   uniform   k = (a << 20) | (b >> 12) (52 bits); u = (2 k + 1) 2^-53, exact, in (0, 1); coin = b & 1 (not a bit of k)
 *   LapGraph  g = 2 u if k < 2^51, else 1 / (2 (1 - u)); key = g c for an edge cell, g otherwise, with c = exp(eps2) computed once
 *             by the caller (`edge_factor`).  The key is exp((a_ij + Laplace(1 / eps2)) eps2) for the inverse-CDF Laplace draw of
 *             u: ranking by key is ranking by adjacency + noise.  One multiply and at most one divide, each correctly rounded
 *             (the library is built with -ffp-contract=off and no fast-math): numpy and the device agree bit for bit.
 *   order     total: key descending, then t ascending (equally: flat index i * n + j ascending).  The selection is the first
 *             n_keep cells of that order.
 *   EdgeRand  a cell is re-drawn iff k < s_threshold = floor(s 2^52), s = 2 / (e^eps + 1); coin 1 sets the pair, 0 clears it.
 * The adjacency is a device CSR (int32; columns sorted and unique within a row; entries j >= i are ignored; d_col must be a
 * valid pointer even for a graph without entries).  Cells are reported as flat indices i * n + j (int64).
 *
 * lt_philox_cells_scan: every cell of rows [row_begin, row_end) whose key is >= key_min, as (out_cell[p], out_key[p]) in no
 * particular order.  *d_count (device int64) receives the number found, also when it exceeds `capacity`; nothing is written
 * past `capacity`.  Enqueue only.  LT_ERR_INVALID before anything is enqueued: NULL pointers, n < 2, rows outside
 * 0 <= row_begin <= row_end <= n, capacity < 0, edge_factor negative or not finite, key_min negative or NaN.
 *
 * lt_lapgraph_philox: the first n_keep cells of the order above, to out_idx ([n_keep] int64, device, unordered).  It scans with
 * a key_min from the closed-form tail of the key distribution (or key_hint when > 0) into a buffer of 3 n_keep + 4096
 * candidates, scans again with a moved key_min if fewer than n_keep or more than the buffer came back, and selects exactly among
 * the candidates (a radix select over the key bits, the tied group resolved by ascending t).  The result does not depend on
 * key_hint or on the number of passes.  info (HOST int64 [8]): [0] the threshold key's bit pattern, [1] candidates of the last
 * scan, [2] scan passes, [3] cells above the threshold key, [4] cells tied at it that were taken, [5] cells tied at it in
 * total ([3] + [4] == n_keep), [6] the last key_min's bit pattern, [7] 0.  Synchronises the stream (it reads the counts back).
 * Any 1 <= n_keep <= n (n - 1) / 2 and any finite edge_factor >= 0.  LT_ERR_INVALID before any device call: NULL pointers,
 * n < 2, n_keep out of range, a bad edge_factor, a workspace smaller than lt_lapgraph_philox_workspace reports or not 8-byte
 * aligned.  LT_ERR_UNSUPPORTED: more cells are tied at one key around the threshold than the candidate buffer holds (only
 * edge_factor == 0 on a graph of more than 3 n_keep + 4096 edges can do that).  The workspace is linear in n_keep (it does
 * not depend on n or nnz); nothing is O(n^2).
 *
 * lt_edgerand_philox: the re-drawn cells of rows [row_begin, row_end) with their coins (out_coin uint8), same count / capacity
 * contract as the scan; needs no adjacency.  s_threshold <= 2^52.  Additive in ABI 5. */
int lt_philox_cells_scan(int32_t n, int32_t row_begin, int32_t row_end, const int32_t *d_rowptr, const int32_t *d_col,
                         uint64_t seed, double edge_factor, double key_min, int64_t *out_cell, double *out_key,
                         int64_t capacity, int64_t *d_count, void *stream);
int lt_lapgraph_philox_workspace(int32_t n, int64_t nnz, int64_t n_keep, size_t *bytes);
int lt_lapgraph_philox(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, uint64_t seed, double edge_factor,
                       int64_t n_keep, double key_hint, int64_t *out_idx, int64_t *info, void *ws, size_t ws_bytes,
                       void *stream);
int lt_edgerand_philox(int32_t n, int32_t row_begin, int32_t row_end, uint64_t seed, uint64_t s_threshold, int64_t *out_cell,
                       uint8_t *out_coin, int64_t capacity, int64_t *d_count, void *stream);

/* ---- a DP graph stays on the device: listed cells -> symmetric CSR -> normalised CSR --------------------
 * lt_sym_csr_from_cells.  cells[k] = i * n + j with j < i (int64, device, any order: what lt_lapgraph_philox and
 * lt_edgerand_philox write).  Coin 1 sets the unordered pair {i, j}, coin 0 clears it; without coins (coins_or_null == NULL) every
 * cell sets.  The base is a device CSR (int32, columns sorted and unique per row, both triangles stored) or absent (both pointers
 * NULL, base_nnz == 0).  Row r of the result is
 *     {c in base row r : the pair {r, c} is not listed with coin 0}  u  {c : the pair {r, c} is listed with coin 1},
 * columns strictly increasing; diagonal entries of the base pass through untouched.  LapGraph is base = NULL without coins,
 * EdgeRand is base = the clean adjacency with coins.
 * d_info (device int64 [4]): [0] the nnz of the result, [1] the cells that are not a strict-lower-triangle cell of an n x n
 * matrix, [2] the listed cells that repeat a cell listed before them (m minus the distinct cells), [3] 0.  With [1] or [2]
 * non-zero the result is unspecified, but no access leaves the buffers.  Nothing is written past out_capacity (entries of
 * out_col); [0] is reported all the same, the capacity contract of lt_philox_cells_scan.  base_nnz + 2 m always suffices.
 * out_rowptr: [n + 1].  The base's row offsets are taken as given (clamped to [0, base_nnz]); they are not validated.
 * Enqueue only, no host round trip: the 2 m directed entries are sorted by (row, col) with two stable LSD radix sorts (the kernels
 * of lt_graph_create_device's transpose), row extents come from a bisection of the sorted rows, every base and listed entry finds
 * its place in its row's merged order by a bisection of the other side, and an ordered compaction (flags, scan, write) keeps what
 * the rule above keeps.  Stream order is the only barrier between blocks.  The output is a pure function of the input: two calls
 * give identical bytes, whatever the order of the cells.
 * LT_ERR_INVALID before anything is enqueued: NULL pointers other than the two _or_null (and the base pair, which is given or
 * absent as a pair), n < 2, m < 0, base_nnz < 0, out_capacity < 0, base_nnz + 2 m >= 2^31 - 1, a workspace smaller than
 * lt_sym_csr_workspace_bytes(n, base_nnz, m) or not 8-byte aligned.  m == 0 with a base copies the base; m == 0 without one
 * gives the empty graph.  The query returns 0 for invalid arguments; it is linear in base_nnz + m plus O(n) words.
 *
 * lt_normalize_csr: the six normalisers of the reference (utils/load.py:562-627) on a UNIT PATTERN -- every stored entry counts as
 * 1, what a DP graph is -- in the float64 arithmetic numpy gives an integer adjacency, narrowed once to float32:
 *   a_rc = 1, plus 1 on the diagonal for LT_NORM_AUG_NORM_ADJ, LT_NORM_AUG_RWALK and LT_NORM_BINGGE (a missing diagonal entry is
 *          inserted, one that is present becomes 2);   s_r = stored entries of row r, plus 1 for those three;   d_r = inv_pow[s_r]
 *   value = fl64(fl64(d_r * a_rc) * d_c) for the power -1/2 forms (FIRST_ORDER_GCN, BINGGE, NORM_ADJ, AUG_NORM_ADJ),
 *           fl64(d_r * a_rc) for the two random-walk forms (RWALK, AUG_RWALK);
 *   then + 1.0 on the diagonal in float64 for FIRST_ORDER_GCN and BINGGE (the entry is inserted if absent);
 *   then one round-to-nearest-even narrowing to float32.
 * inv_pow (device double [n + 2]) is the caller's: inv_pow[s] = s^p as numpy's np.power(np.arange(n + 2.0), p) gives it, p = -1/2
 * with the infinity at s = 0 replaced by 0 for the four power -1/2 forms, p = -1 with the infinity kept for the two random-walk
 * forms.  The table makes the values numpy's bit for bit without leaning on the device's pow.
 * out_rowptr [n + 1], out_col / out_val: out_capacity entries; nnz + n always suffices and nothing is written past it.
 * d_info (device int64 [4]): [0] the nnz written (nnz + n - diagonals present for the four identity-adding forms, nnz for the
 * others), [1] the rows whose columns are not strictly increasing or not in [0, n); with [1] non-zero the output is unspecified,
 * but in bounds.  rowptr is taken as given (clamped to [0, nnz]).  Enqueue only: row lengths, a one-block scan, a fill with a
 * quarter wave per row.  LT_ERR_INVALID before anything is enqueued: NULL pointers, n < 1, nnz < 0 or >= 2^31 - 1 - n, an unknown
 * norm, negative capacity.  Both are additive in ABI 5. */
typedef enum lt_norm {
    LT_NORM_FIRST_ORDER_GCN = 0, /* I + D^-1/2 A D^-1/2                  */
    LT_NORM_BINGGE = 1,          /* (D+I)^-1/2 (A+I) (D+I)^-1/2 + I      */
    LT_NORM_NORM_ADJ = 2,        /* D^-1/2 A D^-1/2                      */
    LT_NORM_AUG_RWALK = 3,       /* (D+I)^-1 (A+I)                       */
    LT_NORM_RWALK = 4,           /* D^-1 A                               */
    LT_NORM_AUG_NORM_ADJ = 5     /* (D+I)^-1/2 (A+I) (D+I)^-1/2          */
} lt_norm;
size_t lt_sym_csr_workspace_bytes(int32_t n, int64_t base_nnz, int64_t m);
int lt_sym_csr_from_cells(int32_t n, const int32_t *base_rowptr_or_null, const int32_t *base_col_or_null, int64_t base_nnz,
                          const int64_t *cells, const uint8_t *coins_or_null, int64_t m, int32_t *out_rowptr, int32_t *out_col,
                          int64_t out_capacity, int64_t *d_info, void *ws, size_t ws_bytes, void *stream);
int lt_normalize_csr(int32_t n, const int32_t *rowptr, const int32_t *col, int64_t nnz, int32_t norm, const double *inv_pow,
                     int32_t *out_rowptr, int32_t *out_col, float *out_val, int64_t out_capacity, int64_t *d_info, void *stream);

/* ---- edge recovery: the m highest-scoring pairs of sampled nodes (attack_stats_all.py:106-116: n_pos = ceil(ratio * n_total),
 * ind = np.argpartition(pred, -n_pos)[-n_pos:] over the saved score list, then precision / recall / F1 of y[ind]) -----------
 * scores: device [n, lds] fp32, what lt_influence_rows / lt_influence3_rows* wrote for probes == observed == the sampled nodes.
 * Only the cells (i, j) with j < i are read -- row = perturbed node, column = observed node, the cells the reference scores
 * its sampled pairs from (attacker.py:235-245); the diagonal, the upper triangle and columns n .. lds - 1 are never read.
 * The cells are ranked by the total order "value descending, then flat index i * n + j ascending", in which -0.0 counts as
 * +0.0 (the key is taken of v + 0.0f; negative values and +-inf rank as numbers).  out_idx[0 .. m): the flat indices i * n + j
 * of the m first cells in that order, written in ASCENDING flat index; out_score[k]: the value at out_idx[k], bit for bit as
 * stored (a stored -0.0 stays -0.0).  out_info (int64 [4], device): [0] the bit pattern of the m-th value (of v + 0.0f,
 * zero-extended), [1] the cells strictly above it, [2] the cells tied at it that were taken (the first so many in flat order),
 * [3] the cells tied at it in total; [1] + [2] == m.  The output is a pure function of the input: two calls give identical
 * bytes (np.argpartition picks among tied values as its partition happens to leave them).  A matrix holding NaNs gives an
 * unspecified set; exactly m in-region indices are written all the same.
 * Enqueue only, no synchronisation, no host round trip: a radix select by four digit histograms (the pick of each digit is the
 * prologue of the next launch), then count / scan / write launches of an ordered compaction; stream order is the only barrier
 * between blocks.  LT_ERR_INVALID before anything is enqueued: NULL pointers, n < 2, lds < n, m outside [1, n (n - 1) / 2], a
 * workspace smaller than lt_top_pairs_workspace_bytes(n, m) or not 8-byte aligned.  The query returns 0 for invalid arguments.
 * Additive in ABI 5. */
size_t lt_top_pairs_workspace_bytes(int32_t n, int64_t m);
int lt_top_pairs_lower(const float *scores, int64_t lds, int32_t n, int64_t m, int64_t *out_idx, float *out_score,
                       int64_t *out_info, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the same selection over rows that arrive in chunks: a whole graph's edge list without the n x n matrix ------------------
 * A handle selects the m first cells of the strict lower triangle of an n x n score matrix that is never formed: the caller
 * pushes rows [row_begin, row_begin + n_rows) as lt_influence_rows / lt_influence3_rows* wrote them for those probes, then
 * finishes.  Total order, out_idx, out_score and out_info are exactly those of lt_top_pairs_lower on the assembled matrix: the
 * result is a pure function of the matrix, whatever the cut into pushes, slack_cells, the compactions that fired or the order in
 * which waves appended.
 * lt_top_stream_create: n >= 2, 1 <= m <= min(n (n - 1) / 2, 2^30), max_push_rows >= 1 (the largest n_rows a push may bring; no
 *   storage depends on it), slack_cells = 0 for the default max(2 (n - 1), 2^22) or a value in [2 (n - 1), 2^31]: the candidate
 *   buffers hold m + slack_cells entries, and a push is cut into slabs of whole rows of at most slack_cells / 2 cells.  Allocates
 *   lt_top_stream_bytes device bytes, A(x) = x rounded up to 256:
 *     25600 + A(8 cap) + A(16 cap) + 4 A(4 m) + A(1024 nblk),  cap = m + slack_cells,
 *     nblk = ceil(m / (256 r)), r the smallest of 4, 8, 16 ... with ceil(m / (256 r)) <= 4096
 *   -- linear in m + slack_cells; nothing is O(n^2) or O(n max_push_rows).  Synchronises the device once (its header is cleared).
 * lt_top_stream_push: rows = device [n_rows, lds] fp32.  Of row i only columns 0 .. i - 1 are read, so lds >= row_begin + n_rows - 1
 *   is enough (a chunk may be formed against the first row_begin + n_rows observed nodes only); nothing else is touched.  Rows
 *   arrive contiguously, in ascending order, from row 0, each once: the handle keeps the next expected row.  LT_ERR_INVALID
 *   before anything is enqueued (the handle stays as it was): NULL, n_rows outside [1, max_push_rows], another row_begin than the
 *   next row, rows beyond n, lds too small, a finished handle.
 * lt_top_stream_finish: out_idx int64 [m], out_score fp32 [m], out_info int64 [4], device.  LT_ERR_INVALID before row n - 1 was
 *   pushed, and on a handle that was finished already.
 * push and finish only enqueue on `stream`: no synchronisation, no host read of device memory, no spinning in a kernel; all
 *   running state (held count, threshold key, cells seen) lives in device memory and stream order is the only barrier.  In front
 *   of every slab a predicated chain of 6 + P launches (P = bytes of n * n - 1) is enqueued; its blocks return at once unless the
 *   held count exceeds m + slack_cells / 2, in which case exactly the m first held entries are kept and the threshold key rises.
 *   A failed HIP call inside push / finish leaves the handle's content undefined until lt_top_stream_reset.
 * lt_top_stream_reset: enqueues the clear of the state; the handle then takes another matrix of the same (n, m).
 * lt_top_stream_stats: enqueues a copy of 16 state words to d_out (device int64 [16]): [0], [1] entries in the two buffers,
 *   [2] the current buffer, [5] threshold key, [6] whether one is set, [7] cells tied at it that were dropped, [8] cells scanned,
 *   [9] chains that fired in front of the first slab of a push (between pushes), [10] in front of a later slab (inside a push),
 *   [11] slabs scanned; the others are internal.  One handle serves one stream at a time.  Additive in ABI 5. */
typedef struct lt_top_stream lt_top_stream;
int lt_top_stream_create(int32_t n, int64_t m, int32_t max_push_rows, int64_t slack_cells, lt_top_stream **out);
int lt_top_stream_bytes(const lt_top_stream *s, size_t *device_bytes);
int lt_top_stream_push(lt_top_stream *s, const float *rows, int64_t lds, int32_t row_begin, int32_t n_rows, void *stream);
int lt_top_stream_finish(lt_top_stream *s, int64_t *out_idx, float *out_score, int64_t *out_info, void *stream);
int lt_top_stream_reset(lt_top_stream *s, void *stream);
int lt_top_stream_stats(const lt_top_stream *s, int64_t *d_out, void *stream);
int lt_top_stream_destroy(lt_top_stream *s);

/* lt_pairs_present: out[k] (uint8, device) = 1 iff column v[k] is stored in row u[k] of the device CSR pattern (sorted columns, as
 * the attack's samplers take it), else 0: a binary search per pair.  u, v: device int32 [m].  d_info (device int64 [1]) is
 * cleared and then counts the pairs with an id outside [0, n); such a pair gets out[k] = 0 and reads nothing.  The node-id flag of
 * the probe primitives is not involved.  Enqueue only.  Additive in ABI 5. */
int lt_pairs_present(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, const int32_t *u, const int32_t *v, int64_t m,
                     uint8_t *out, int64_t *d_info, void *stream);

/* ---- attack metrics: the table behind roc_curve / precision_recall_curve / average_precision_score (attacker.py:378-389) --------
 * Item k (of n_items) has label labels[k] (uint8, 0 or 1) and score scores[index[k]], or scores[k] when index_or_null is NULL.
 * With an index, n_scores is the extent of scores in ELEMENTS and every index must lie in [0, n_scores): the index addresses storage,
 * so a strided score matrix is read through i * lds + j, an element may be listed twice, and the diagonal and the padding are
 * simply never listed.  Without one, n_scores >= n_items.  Every pointer is device memory.
 * Values are ordered as lt_top_pairs_lower orders them: -0.0 counts as +0.0, subnormals are kept as they are.  With
 * v_1 > v_2 > ... > v_D the distinct values, entries [0, D) of the three output arrays (capacity n_items each) are written:
 *   thresholds[d] = v_d (the zero group reports +0.0), tps[d] = #{k : y_k = 1, s_k >= v_d}, fps[d] = #{k : y_k = 0, s_k >= v_d}
 * -- sklearn's _binary_clf_curve for float32 scores -- and summary (int64 [8]):
 *   [0] D   [1] P = all positives   [2] N = all negatives
 *   [3] auc2 = sum_d neg_d (2 tps[d - 1] + pos_d), tps[-1] = 0, pos_d / neg_d the counts AT v_d: AUC = auc2 / (2 P N) exactly
 *   [4] the bit pattern of the float64 AP = sum_d (pos_d / P) (tps[d] / (tps[d] + fps[d])), summed in ONE fixed order (thread order
 *       inside a block, then block order): two calls give the same bits; 0 when P = 0
 *   [5] items whose score is NaN or +-Inf   [6] items whose index is outside [0, n_scores)   [7] items whose label is > 1
 * When [5], [6] or [7] is non-zero the other outputs are unspecified; no access leaves the buffers all the same (a bad index is
 * replaced by 0 before the load).  Every output is a function of the multiset of (value, label) pairs: item order does not show.
 * Enqueue only, no synchronisation, no host round trip: one gather pass, an LSD radix sort of 32-bit keys (8 bits a pass, the label
 * as payload), run ends + two scans + a compaction to D entries, a last pass for auc2 and AP; stream order is the only barrier
 * between blocks.  LT_ERR_INVALID before anything is enqueued: a NULL pointer other than index_or_null, n_items outside
 * [1, 2^31 - 1], n_scores < 1, a NULL index with n_scores < n_items, a workspace smaller than lt_score_curve_workspace_bytes(n_items)
 * or not 8-byte aligned.  The query returns 0 for an invalid n_items.  Additive in ABI 5. */
size_t lt_score_curve_workspace_bytes(int64_t n_items);
int lt_score_curve(const float *scores, int64_t n_scores, const int64_t *index_or_null,
                   const uint8_t *labels, int64_t n_items,
                   float *thresholds, int64_t *tps, int64_t *fps, int64_t *summary,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- the attack's node pairs: which pairs are scored and which of them are edges -------------------------
 * The adjacency of the four functions is a device CSR of int32 (d_rowptr [n + 1], d_col, nnz stored entries) whose columns are
 * sorted and unique within a row.  A stored entry counts whatever its value: structural presence, what the reference's
 * _get_edge_sets_among_nodes (utils/load.py:304-326) and construct_balanced_edge_sets (utils/load.py:219-249) read.  d_col must be
 * a valid pointer even for a graph without entries.  Row offsets are taken as given (clamped to [0, nnz]).
 *
 * lt_sample_square_labels: all pairs of a node sample.  nodes[k]: int32, device, distinct ids in [0, n), in ANY order (a sample is
 * not sorted).  Pair (i, j), i < j, of POSITIONS has slot p = i (2 k - i - 1) / 2 + (j - i - 1) -- row-major over the strict upper
 * triangle, the reference's enumeration order -- of T = k (k - 1) / 2:
 *   out_labels[p] (uint8) = 1 iff nodes[j] is stored in row nodes[i] (directed, as in the reference), else 0
 *   out_index_or_null[p] (int64) = j * lds + i: the storage element of the cell "perturb nodes[j], observe nodes[i]" in score rows
 *                                  of stride lds >= k (what lt_score_curve takes as its index)
 *   d_info (device int64 [4]): [0] labels set, [1] nodes outside [0, n), [2] nodes that repeat an earlier one, [3] 0.  With [1] or
 *                              [2] non-zero the outputs are unspecified, but no access leaves the buffers.
 * Enqueue only, no host round trip: a position map pos[node] in the workspace is cleared, scattered and checked back; one block
 * per position i clears its stretch of labels and writes its stretch of the index, then walks row nodes[i] block-wide (a hub row
 * costs its length / 256 trips) and sets the label of every column c with pos[c] > i.  The count is an integer atomic.
 * LT_ERR_INVALID before anything is enqueued: NULL pointers other than the index, n < 1, k < 2, lds < k, nnz outside [0, 2^31 - 1),
 * a workspace smaller than lt_sample_square_workspace_bytes(n, k) or not 8-byte aligned.  The query returns 0 for invalid arguments.
 *
 * lt_group_pairs: probe[m], observed[m] (int32, device, ids in [0, n)) -> the grouped layout of lt_influence_pairs:
 *   out_order [m] int32    the STABLE sort of the pairs by probe (the pairs of one probe keep their input order, repeats are kept)
 *   out_obs   [m] int32    observed[out_order[p]]
 *   out_nodes [m] int32    entries [0, G): the distinct probes, ascending
 *   out_ptr   [m + 1] int64, DEVICE   entries [0, G]: group g is [out_ptr[g], out_ptr[g + 1]) of out_obs
 *   d_info (device int64 [4]): [0] G, [1] ids (of either list) outside [0, n): the result is then unspecified, but in bounds; [2], [3] 0
 * Enqueue only: the stable LSD radix sort of lt_graph_create_device (the digit passes that order [0, n - 1], the pair's index as
 * payload), run ends, a scan, a compaction of the group heads.  LT_ERR_INVALID before anything is enqueued: NULL pointers, n < 1,
 * m outside [1, 2^31 - 2], a workspace smaller than lt_group_pairs_workspace_bytes(m) or not 8-byte aligned.
 *
 * lt_upper_edge_count: *d_count (device int64) = E, the stored entries with col > row.  Enqueue only.
 *
 * lt_sample_balanced_philox: the `balanced-full` pair lists as two int32 device arrays out_u, out_v of 2 E entries.
 *   [0, E)    the edges: every stored entry with col > row as (row, col), rows ascending, columns ascending within a row
 *   [E, 2 E)  the non-edges: the first E ACCEPTED draws of STREAM 3 of the Philox contract above, in draw order:
 *               draw t = 0, 1, 2, ... (64 bits); counter (t & 0xffffffff, t >> 32, 3, 0), key (seed & 0xffffffff, seed >> 32)
 *               -> words w[0 .. 3];  u = (uint64(w[0]) * n) >> 32,  v = (uint64(w[1]) * n) >> 32;  w[2], w[3] are unused.
 *               n < 2^31; the multiply-shift favours an id over another by at most n 2^-32 in probability.
 *             A draw is accepted iff v is not stored in row u AND u is not stored in row v.  The reference's quirks are kept:
 *             u == v is accepted unless (u, u) is stored, repeated pairs are kept, both directions are tested.  Like the DP
 *             streams, a seed gives a DIFFERENT sample than numpy's generator would.
 * Draws are evaluated in rounds of round_draws consecutive t (0: a default near 9 E / 8, at most 2^22; at most 2^24): flags (two
 * bisections of sorted rows per draw), a scan, an ordered write of the accepted draws that still fit.  The host reads the running
 * count after each round, so the call SYNCHRONISES the stream, as lt_lapgraph_philox does.  The result is a pure function of
 * (graph, seed): it depends on neither round_draws nor the number of rounds.  E is the caller's, from lt_upper_edge_count; max_draws
 * bounds t (0: 64 E + 4096).  info (HOST int64 [8]): [0] E, [1] draws consumed (t of the last accepted draw + 1), [2] rounds,
 * [3] accepted draws with u == v, the rest 0.  E == 0 writes nothing and succeeds.
 * LT_ERR_INVALID: NULL pointers, n < 1, E outside [0, 2^30), nnz outside [0, 2^31 - 1), max_draws < 0, round_draws outside
 * [0, 2^24], a workspace smaller than lt_sample_balanced_workspace_bytes(n, E, round_draws) or not 8-byte aligned -- all before any
 * device call -- and an E that is not the graph's (after one count).  LT_ERR_UNSUPPORTED: fewer than E draws were accepted within
 * max_draws (the message names the counts; the reference's loop would not end on such a graph); [1] is then the draws evaluated.
 * All additive in ABI 5. */
size_t lt_sample_square_workspace_bytes(int32_t n, int32_t k);
int lt_sample_square_labels(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, int64_t nnz, const int32_t *nodes, int32_t k,
                            int64_t lds, uint8_t *out_labels, int64_t *out_index_or_null, int64_t *d_info, void *ws, size_t ws_bytes,
                            void *stream);
size_t lt_group_pairs_workspace_bytes(int64_t m);
int lt_group_pairs(int32_t n, const int32_t *probe, const int32_t *observed, int64_t m, int32_t *out_nodes, int64_t *out_ptr,
                   int32_t *out_obs, int32_t *out_order, int64_t *d_info, void *ws, size_t ws_bytes, void *stream);
int lt_upper_edge_count(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, int64_t nnz, int64_t *d_count, void *stream);
size_t lt_sample_balanced_workspace_bytes(int32_t n, int64_t E, int64_t round_draws);
int lt_sample_balanced_philox(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, int64_t nnz, int64_t E, uint64_t seed,
                              int64_t max_draws, int64_t round_draws, int32_t *out_u, int32_t *out_v, int64_t *info, void *ws,
                              size_t ws_bytes, void *stream);

/* ---- the baseline attacks' scores (LSA2-post / LSA2-attr, attacker.py:287-375): correlation of mean-centred rows ---------------------
 * V: device [n, ldv] fp32 (posteriors or features), ldv >= D, any 4-byte alignment.  The score of two rows is
 *   corr(a, b) = <x_a - m, x_b - m> / ||x_a - m|| / ||x_b - m||
 * with the fp32 inputs widened exactly and the mean m, the centring, every product and every sum in fp64; ONE rounding to fp32
 * happens at the store.  No floating-point atomics: column sums go through a fixed partition of the rows (a function of the row
 * count alone) added in partition order, the Gram's K slices (a function of (k, D) alone) are added in slice order; two calls
 * give equal bits.
 * lt_corr_square: out[i * ldo + j] = corr(nodes[i], nodes[j]), i, j < k; m = the column mean over the k listed rows (a repeated
 *   id counts as often as it is listed).  The full k x k square is written and equals its transpose bit for bit (every lower
 *   64 x 64 tile is formed once on v_mfma_f64_16x16x4_f64 and stored twice); words j >= k of a row are left alone.  The norms are
 *   the square roots of the reduced Gram's own diagonal.
 * lt_corr_pairs: out[p] = corr(u[p], v[p]), p < m; the mean is taken over ALL n rows; u[p] == v[p] is allowed (the reference's
 *   balanced-full sample produces it).
 * nodes, u, v: device int32.  info (device int64 [4]): [0] rows (square) / pairs (pair list) with a zero-norm row -- a row whose
 * centred vector is zero; every cell it touches is NaN, as the reference's 0 / 0 is; [1] node ids outside [0, n): such an id is
 * never used as an address, every cell it touches is NaN, and the square's mean is taken over the valid listed rows; [2], [3] 0.
 * Enqueue only, no synchronisation.  LT_ERR_INVALID before any device call: NULL pointers, n < 1, D < 1, k < 0, m outside
 * [0, 2^31 - 1], ldv < D, ldo < k, a workspace smaller than lt_corr_workspace_bytes(n, D, k, 0) / (n, D, 0, m) or not 8-byte
 * aligned.  k == 0 / m == 0: a successful no-op.  The query serves both calls (the larger need) and returns 0 for invalid
 * arguments.  Additive in ABI 5. */
size_t lt_corr_workspace_bytes(int32_t n, int32_t D, int32_t k, int64_t n_pairs);
int lt_corr_square(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *nodes, int32_t k, float *out, int64_t ldo,
                   int64_t *info, void *ws, size_t ws_bytes, void *stream);
int lt_corr_pairs(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *u, const int32_t *v, int64_t m, float *out,
                  int64_t *info, void *ws, size_t ws_bytes, void *stream);

/* ---- row bands of lt_corr_square's square: the square is never formed, rows arrive a band at a time (edge recovery over a whole
 * graph: lt_top_stream_push consumes them) ---------------------------------------------------------------------------------------
 * lt_corr_rows_prepare leaves the column mean over the k listed rows and the norm of every listed row in the head of ws and
 *   fills info exactly as lt_corr_square does ([0] zero-norm rows, [1] ids outside [0, n)): one four-word copy tells the caller
 *   about NaN rows before any row is formed.  The layout inside ws is the library's own; the caller keeps ws, V and nodes
 *   untouched until the last rows call.
 * lt_corr_rows writes out[i * ldo + j] = corr(nodes[row_begin + i], nodes[j]) for i < n_rows, j < n_cols; words j >= n_cols of a
 *   row are left alone.  n_cols < k asks for the lower trapezoid only (the stream reads columns 0 .. i - 1 of row i): 64-column
 *   blocks wholly at or right of n_cols are not computed.
 * Bit contract: every cell written has the bits lt_corr_square writes at that cell for the same (V, nodes), for any row_begin,
 *   n_rows, n_cols (bands need not start on a multiple of 64): the same tile arithmetic on v_mfma_f64_16x16x4_f64, the K slice
 *   plan of the WHOLE list (a function of (k, D)), slices added in slice order from 0.0, norms = square roots of the Gram's own
 *   diagonal (prepare forms the k / 64 diagonal tiles only), one rounding.  The two divisions round separately and do not
 *   commute: the square forms a cell in its lower position, g / n_row / n_col with row >= col, and mirrors the bits; so a cell
 *   (i, j) is g / n_max(i,j) / n_min(i,j) of list positions, above the diagonal too.  No floating-point atomics.
 * Workspace: 8 * (D' + (P D)' + k' + part) bytes, x' = x rounded up to even, P = ceil(k / max(32, ceil(k / 1024))) column-sum
 *   partitions; part = S * ceil(max_rows / 64) * ceil(k / 64) * 4096 words of per-slice partial tiles when the slice plan has
 *   S > 1 slices (k below about 2000), 0 when it has one (the finish is then the Gram kernel's epilogue).  At least 16 bytes;
 *   nothing grows with k^2.  lt_corr_rows_prepare needs the head (max_rows = 0).  Returns 0 for invalid arguments (n < 1, D < 1,
 *   k < 0, max_rows < 0).
 * Both calls enqueue only.  LT_ERR_INVALID before any device call: NULL pointers, n < 1, D < 1, k < 0, ldv < D, ldo < n_cols,
 * row_begin < 0, n_rows < 0, row_begin + n_rows > k, n_cols outside [0, k], n_rows > 4 194 240 (65 535 row blocks of 64: one
 * launch's grid; a longer band is several calls), a workspace smaller than
 * lt_corr_rows_workspace_bytes(n, D, k, n_rows) -- that is n_rows above the max_rows it was sized for, where the size depends on
 * it -- or not 8-byte aligned.  n_rows == 0 or n_cols == 0: a successful no-op.  A bad node id is never an address; its cells are
 * NaN.  Additive in ABI 5. */
size_t lt_corr_rows_workspace_bytes(int32_t n, int32_t D, int32_t k, int32_t max_rows);
int lt_corr_rows_prepare(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *nodes, int32_t k, int64_t *info, void *ws,
                         size_t ws_bytes, void *stream);
int lt_corr_rows(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *nodes, int32_t k, int32_t row_begin,
                 int32_t n_rows, int32_t n_cols, float *out, int64_t ldo, void *ws, size_t ws_bytes, void *stream);

/* ---- training of the 2-layer GCN (reference gcn_trainer.py:144-170 train_one_epoch + optim.Adam) ----
 * lt_gcn2_trainer_create borrows the graph, X [n, ldx], labels (int32 [n], device, each in [0, C)) and the four parameter
 * tensors (W1 [F, H], b1 [H], W2 [H, C], b2 [C], dense fp32 device buffers), which every epoch updates IN PLACE; it owns
 * the Adam moments and every intermediate.  H <= 256 and C <= 8 (the fused forward's limits), dropout in [0, 1]; anything
 * else is LT_ERR_INVALID.  One epoch, with e = the epochs run since creation:
 *   S1 = X W1; Z1 = A S1 + b1; H1d = dropout_p(relu(Z1)); S2 = H1d W2; Z2 = A S2 + b2  (the launches of lt_gcn2_forward:
 *        with dropout 0 the first epoch's Z2 equals lt_gcn2_forward's logits bit for bit)
 *   loss = mean_r CE(Z2[r], y[r]); dZ2 = (softmax(Z2) - onehot(y)) / n; dS2 = A^T dZ2 (the CSC: A need not be symmetric)
 *   dW2 = H1d^T dS2, db2 = sum_r dZ2, dZ1 = [H1d > 0] (dS2 W2^T) / (1 - p), db1 = sum_r dZ1, dS1 = A^T dZ1, dW1 = X^T dS1
 *   one Adam step (torch.optim.Adam: betas (0.9, 0.999), eps 1e-8, weight decay added to the gradient), step = e + 1
 * Dropout: element (r, h) has i = r * H + h; it is kept iff word (i & 3) of Philox4x32-10 with counter
 * (q & 0xffffffff, q >> 32, e, 0), q = i >> 2, and key (seed & 0xffffffff, seed >> 32) is >= floor(p * 2^32); kept
 * elements are scaled by (float)(1 / (1 - p)).  p = 0 draws nothing; p = 1 keeps nothing.
 * lt_gcn2_trainer_run enqueues n_epochs epochs on `stream`, no host synchronisation; record (device, [n_epochs, 2] fp32):
 * per epoch the mean training loss and the number of rows whose first argmax equals the label.  Every reduction has a
 * fixed order: the same inputs and seed give the same bits, and run(40) equals four run(10).
 * lt_gcn2_trainer_grads / _logits: the LAST epoch's gradients (before weight decay) and its train-mode logits Z2 (before
 * that epoch's update) -- for tests, as lt_spmm_gather_ceiling is for measurement.  lt_gcn2_trainer_epoch: epochs run. */
typedef struct lt_gcn2_trainer lt_gcn2_trainer;
int lt_gcn2_trainer_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const int32_t *labels, int32_t H,
                           int32_t C, float *W1, float *b1, float *W2, float *b2, double lr, double weight_decay,
                           double dropout, uint64_t seed, void *stream, lt_gcn2_trainer **out);
int lt_gcn2_trainer_run(lt_gcn2_trainer *t, int32_t n_epochs, float *record, void *stream);
int lt_gcn2_trainer_grads(const lt_gcn2_trainer *t, float *dW1, float *db1, float *dW2, float *db2, void *stream);
int lt_gcn2_trainer_logits(const lt_gcn2_trainer *t, float *Z2, int64_t ldz, void *stream);
int lt_gcn2_trainer_epoch(const lt_gcn2_trainer *t, int64_t *epoch);
int lt_gcn2_trainer_destroy(lt_gcn2_trainer *t);
/* ---- training of the 3-layer GCN (reference gcn/models.py:28-46 GCN3 under the same train_one_epoch) ----
 * Ownership, validation and stream semantics of lt_gcn2_trainer_*: the graph, X [n, ldx], labels and the six parameter tensors
 * (W1 [F, H1], b1 [H1], W2 [H1, H2], b2 [H2], W3 [H2, C], b3 [C], dense fp32 device buffers) are borrowed and the parameters
 * are updated IN PLACE; the trainer owns every intermediate and the Adam moments.  H1, H2 <= 256 and C <= 8 (the limits of
 * lt_baseline3_create), dropout in [0, 1], lr and weight_decay >= 0; anything else is LT_ERR_INVALID.  One epoch, with e =
 * the epochs run since creation, A the graph as given (not symmetric in general), scale = (float)(1 / (1 - p)):
 *   S1 = X W1;   Z1 = A S1 + b1; H1d = drop_0(relu(Z1))   [n, H1]
 *   S2 = H1d W2; Z2 = A S2 + b2; H2d = drop_1(relu(Z2))   [n, H2]
 *   S3 = H2d W3; Z3 = A S3 + b3                           [n, C]
 *   loss = mean_r CE(Z3[r], y[r]); dZ3 = (softmax(Z3) - onehot(y)) / n; db3 = sum_r dZ3
 *   dS3 = A^T dZ3; dW3 = H2d^T dS3; dZ2 = [H2d > 0] scale (dS3 W3^T); db2 = sum_r dZ2
 *   dS2 = A^T dZ2; dW2 = H1d^T dS2; dZ1 = [H1d > 0] scale (dS2 W2^T); db1 = sum_r dZ1
 *   dW1 = X^T (A^T dZ1)
 *   one Adam step (lt_adam_step's op order, weight decay added to the gradient) over W1 | b1 | W2 | b2 | W3 | b3, step = e + 1
 * Dropout: for hidden layer k in {0, 1}, element (r, h) has i = r * H_{k+1} + h; it is kept iff word (i & 3) of
 * Philox4x32-10 with counter (q & 0xffffffff, q >> 32, e, k), q = i >> 2, and key (seed & 0xffffffff, seed >> 32) is
 * >= floor(p * 2^32).  Layer 0 is exactly the 2-layer trainer's mask; the layer word keeps the two masks apart when
 * H1 = H2.  p = 0 draws nothing; p = 1 keeps nothing.
 * lt_gcn3_trainer_run enqueues without a host synchronisation; record [n_epochs, 2] = (mean loss, correct count) per epoch.
 * No float atomics and every reduction in a fixed order: run(a + b) equals run(a); run(b) bit for bit, and two trainers
 * with the same inputs give the same bits.
 * lt_gcn3_trainer_grads / _logits / _hidden are test accessors for the LAST epoch: its six gradients (before weight decay),
 * its train-mode logits Z3 [n, ldz] and its H1d (layer 1, [n, H1]) or H2d (layer 2, [n, H2]) after ReLU and dropout, written
 * with leading dimension ld. */
typedef struct lt_gcn3_trainer lt_gcn3_trainer;
int lt_gcn3_trainer_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const int32_t *labels,
                           int32_t H1, int32_t H2, int32_t C,
                           float *W1, float *b1, float *W2, float *b2, float *W3, float *b3,
                           double lr, double weight_decay, double dropout, uint64_t seed, void *stream,
                           lt_gcn3_trainer **out);
int lt_gcn3_trainer_run(lt_gcn3_trainer *t, int32_t n_epochs, float *record, void *stream);
int lt_gcn3_trainer_grads(const lt_gcn3_trainer *t, float *dW1, float *db1, float *dW2, float *db2,
                          float *dW3, float *db3, void *stream);
int lt_gcn3_trainer_logits(const lt_gcn3_trainer *t, float *Z3, int64_t ldz, void *stream);
int lt_gcn3_trainer_hidden(const lt_gcn3_trainer *t, int32_t layer /* 1 | 2 */, float *dst, int64_t ld, void *stream);
int lt_gcn3_trainer_epoch(const lt_gcn3_trainer *t, int64_t *epoch);
int lt_gcn3_trainer_destroy(lt_gcn3_trainer *t);
/* One Adam step over n fp32 elements in place (the trainer's update, exported so it is tested on its own):
 * torch/optim/adam.py _single_tensor_adam op by op in fp32 with correctly rounded sqrt and division, and fused multiply-adds
 * where torch's CPU kernels fuse (the weight-decay add, lerp_, addcmul_) --
 *   g' = fma(p, wd, g); m = fma(w1, g' - m, m) (lerp_, w1 = 1 - beta1); v = v beta2; v = fma(w2 g', g', v) (w2 = 1 - beta2);
 *   p = p + (-lr / bc1 * m) / (sqrt(v) / sqrt(bc2) + eps),  bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 * -- the scalars formed in double and rounded once to float, as torch does with Python scalars.  step >= 1 is the step
 * count after this update. */
int lt_adam_step(int64_t n, float *p, const float *g, float *m, float *v, int64_t step, double lr, double beta1,
                 double beta2, double eps, double weight_decay, void *stream);

/* ---- validation every epoch: evaluation head, early-stopping state, best-model snapshot (reference gcn_trainer.py:167-174,
 * 195-196, 235-238 and utils/early_stopping.py).  Additive within ABI 5; everything is opt-in.
 *
 * lt_eval_head: mean cross-entropy and confusion matrix of logits Z [n, ldz] (fp32, device) against labels (int32 [n], device),
 * enqueue-only, in two launches.  Row stage: one thread per row, ceil(n / 256) blocks, the training head's per-row arithmetic
 * (loss_r = (max + logf(sum expf(z - max))) - z[y], predicted class = first argmax); each block reduces its 256 row losses
 * with a fixed tree and counts its C x C cells as integers.  Finish stage: one block adds the blocks' partials in a fixed
 * order.  loss (device, one float) = the sum / n; confusion (device, int32 [C, C], row = true class, column = predicted
 * class), whose trace is the correct count.  No float atomics: the outputs are a pure function of the inputs.  A label
 * outside [0, C) counts in no cell (its row's loss reads z[y] as 0, as the training head does): checking labels is the
 * caller's job here, lt_gcn*_trainer_attach_validation does it.  LT_ERR_INVALID before any launch: n <= 0, C outside
 * [1, 8], ldz < C, a NULL pointer; LT_ERR_WORKSPACE: workspace (device, 4-byte aligned) smaller than
 * lt_eval_head_workspace_bytes(n, C) (0 for unsupported n / C).
 *
 * The early-stopping state is 8 int32 words of device memory the caller owns:
 *   [0] best_loss (the fp32 bits)  [1] best_epoch  [2] counter  [3] stop_epoch (-1 while running)
 *   [4] improved (the last update's flag)  [5] seen (1 once an epoch has been applied)  [6], [7] 0
 * lt_early_stop_reset writes the initial state (best_epoch = stop_epoch = -1, the rest 0).  lt_early_stop_update applies one
 * epoch's loss (a device word) -- EarlyStopping.__call__ with delta = 0:
 *   stop_epoch >= 0:  improved = 0, nothing else changes (the state is frozen)
 *   seen && loss > best_loss:  ++counter, improved = 0; if (patience > 0 && counter >= patience) stop_epoch = epoch
 *   otherwise:  best_loss = loss, best_epoch = epoch, counter = 0, improved = 1
 * so a tie is an improvement, and a NaN loss (or a NaN best) compares false and becomes the best, as `score < best_score`
 * does in the reference.  patience = 0: keep the best, never stop.  Both calls are enqueue-only (one launch).
 * LT_ERR_INVALID before the launch: a NULL pointer, patience < 0, epoch < 0.
 *
 * Per trainer (`gcn2` and `gcn3` alike):
 * lt_gcn*_trainer_attach_validation borrows the held-out graph g2, X2 [n2, ldx2] and labels2 (int32 [n2], device); the
 * trainer allocates the forward's buffers at n2 rows (with split-K slabs chosen for n2), the head's partials, the state
 * block and, with keep_best = 1, a snapshot buffer of the parameters' size.  It synchronises (labels2 is read back and
 * checked).  LT_ERR_INVALID, with nothing allocated or launched: a second attach; a NULL argument; n2 != the graph's node
 * count or an empty graph; ldx2 < F; a label outside [0, C); keep_best outside {0, 1}; patience < 0; g2, X2 or labels2 not in
 * device memory of the device the trainer's X lives on.
 * lt_gcn*_trainer_run_validated enqueues n_epochs epochs, no host synchronisation.  Per epoch e (0-based, counted since the
 * trainer was created): the training epoch of lt_gcn*_trainer_run, unchanged; then, with the updated parameters, the
 * forward's launches with dropout off on (g2, X2) -- for gcn2 the launches of lt_gcn2_forward, hence its bits -- the
 * evaluation head, the state update (inside the finish launch) and, with keep_best, one predicated launch that copies the
 * live parameters into the snapshot when `improved` is set and returns at once when it is not.  record [n_epochs, 2] as
 * lt_gcn*_trainer_run; val_loss [n_epochs] fp32; val_counts [n_epochs, C * C] int32 (device).  Epochs enqueued after a stop
 * still run and still fill their rows of the three outputs; they change the live parameters and nothing else: state and
 * snapshot are frozen, so the selected model does not depend on how many epochs were enqueued past the stop.
 * LT_ERR_INVALID before any launch: no validation attached, n_epochs < 0, a NULL output with n_epochs > 0.
 * lt_gcn*_trainer_run on a trainer with validation attached keeps its meaning: no validation.
 * lt_gcn*_trainer_val_state copies the 8 state words to `state` (host) and synchronises the stream.
 * lt_gcn*_trainer_restore_best (keep_best only, else LT_ERR_INVALID) enqueues the copy of the snapshot into the live
 * parameters (nothing happens before the first validated epoch); the padded copies follow at the next run, as always.
 * lt_gcn*_trainer_val_logits: test accessor, the last validation logits [n2, C] written with leading dimension ldz >= C.
 *
 * Row lists (datasets with one graph and a split of its nodes: reference gcn_trainer.py:183-196, 354-383; DESIGN.md section
 * 10.3).  Additive within ABI 5.
 * lt_eval_head_rows: lt_eval_head over a list.  rows (int32 [m], device) holds node ids in any order, repeats allowed, each
 * occurrence counting; list entry i scores logits row rows[i] against labels[rows[i]] with lt_eval_head's per-row arithmetic
 * (the same operations in the same order, first argmax).  Entry i belongs to block i / 256; block tree and finish stage are
 * lt_eval_head's, in two launches (and one 4-byte memset when n_bad is given).  loss = the sum / m; confusion covers the listed
 * entries only.  An id outside [0, n) is never dereferenced: it contributes nothing, the divisor stays m, and it is counted in
 * *n_bad (int32, device; may be NULL).  With rows = 0 .. n - 1 the outputs are lt_eval_head's bits.  Enqueue-only, no float
 * atomics, a pure function of the inputs.  LT_ERR_INVALID before any launch: m <= 0, n <= 0, C outside [1, 8], ldz < C, a NULL
 * pointer other than n_bad; LT_ERR_WORKSPACE: workspace (device, 4-byte aligned) smaller than
 * lt_eval_head_rows_workspace_bytes(m, C) (0 for unsupported m / C).
 * lt_gcn*_trainer_attach_validation_rows is lt_gcn*_trainer_attach_validation plus the list: rows (int32 [m], device, the
 * trainer's device) is borrowed, read back once and checked on the host -- m <= 0, a NULL list or an id outside [0, n2) is
 * LT_ERR_INVALID (the message names the first offender), with nothing allocated.  lt_gcn*_trainer_run_validated then applies
 * the head to the list: val_loss, val_counts, the early-stopping state and the snapshot follow the listed rows; everything
 * else in its contract is unchanged.  lt_eval_head and lt_gcn*_trainer_attach_validation keep every bit and every launch. */
size_t lt_eval_head_workspace_bytes(int32_t n, int32_t C);
int lt_eval_head(const float *Z, int64_t ldz, const int32_t *labels, int32_t n, int32_t C, float *loss, int32_t *confusion,
                 void *workspace, size_t workspace_bytes, void *stream);
#define LT_EARLY_STOP_WORDS 8
int lt_early_stop_reset(int32_t *state, void *stream);
int lt_early_stop_update(const float *loss, int32_t patience, int32_t epoch, int32_t *state, void *stream);
int lt_gcn2_trainer_attach_validation(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                                      const int32_t *labels2, int32_t keep_best, int32_t patience, void *stream);
int lt_gcn2_trainer_run_validated(lt_gcn2_trainer *t, int32_t n_epochs, float *record, float *val_loss, int32_t *val_counts,
                                  void *stream);
int lt_gcn2_trainer_val_state(const lt_gcn2_trainer *t, int32_t *state, void *stream);
int lt_gcn2_trainer_restore_best(lt_gcn2_trainer *t, void *stream);
int lt_gcn2_trainer_val_logits(const lt_gcn2_trainer *t, float *Z, int64_t ldz, void *stream);
int lt_gcn3_trainer_attach_validation(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                                      const int32_t *labels2, int32_t keep_best, int32_t patience, void *stream);
int lt_gcn3_trainer_run_validated(lt_gcn3_trainer *t, int32_t n_epochs, float *record, float *val_loss, int32_t *val_counts,
                                  void *stream);
int lt_gcn3_trainer_val_state(const lt_gcn3_trainer *t, int32_t *state, void *stream);
int lt_gcn3_trainer_restore_best(lt_gcn3_trainer *t, void *stream);
int lt_gcn3_trainer_val_logits(const lt_gcn3_trainer *t, float *Z, int64_t ldz, void *stream);
size_t lt_eval_head_rows_workspace_bytes(int32_t m, int32_t C);
int lt_eval_head_rows(const float *Z, int64_t ldz, const int32_t *labels, int32_t n, int32_t C, const int32_t *rows, int32_t m,
                      float *loss, int32_t *confusion, int32_t *n_bad, void *workspace, size_t workspace_bytes, void *stream);
int lt_gcn2_trainer_attach_validation_rows(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                                           const int32_t *labels2, int32_t keep_best, int32_t patience, const int32_t *rows,
                                           int32_t m, void *stream);
int lt_gcn3_trainer_attach_validation_rows(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                                           const int32_t *labels2, int32_t keep_best, int32_t patience, const int32_t *rows,
                                           int32_t m, void *stream);

/* ---- the wide head of the 2-layer trainer: class width 1 <= C <= 256, cross-entropy or multi-label BCE (reference
 * gcn_trainer.py:27-28, 41-45, 258-262) ----
 * lt_gcn2_trainer_create_wide is lt_gcn2_trainer_create with the class layer run as matrix products at the padded width and
 * the loss head of lt_train_wide.hip.h.  loss_kind LT_LOSS_CE: labels int32 [n] (ldy is not read), mean cross-entropy;
 * LT_LOSS_BCE: labels uint8 [n, ldy] holding 0 / 1 (any other byte counts as 1), loss = sum over all n C elements of
 * max(z, 0) - z y + log1p(exp(-|z|)), divided by n C (F.binary_cross_entropy_with_logits, mean).  The handle is a
 * lt_gcn2_trainer: _run, _grads, _logits, _epoch, _destroy, _run_validated, _val_state, _restore_best and _val_logits work on
 * it.  record [n_epochs, 2] = (loss, sum over the classes of tp): for CE the correct count, as lt_gcn2_trainer_run's.  The
 * mask contract is the 2-layer trainer's (layer word 0).  No float atomics, every reduction in a fixed order: run(a + b)
 * equals run(a); run(b) and two trainers agree bit for bit.  Against lt_gcn2_trainer_create at C <= 8 the results agree to
 * rounding, not bit for bit: the class layer's sums are associated differently.  LT_ERR_INVALID with a message naming the
 * value, nothing allocated: H > 256, C > 256, an unknown loss_kind, ldy < C for LT_LOSS_BCE.
 * lt_gcn2_trainer_counts: the LAST epoch's counts, int32 [C, 3] = (tp, fp, fn) per class (device); wide trainers only.  CE: a
 * row with first argmax a and label y adds tp[y] when a == y, else fp[a] and fn[y].  BCE: element (r, c) is predicted positive
 * iff z > 0 (the reference's sigmoid(z) > 0.5 in fp32 differs only where |z| < 2^-22).
 * lt_gcn2_trainer_hidden: test accessor, the last epoch's H1d = drop(relu(A X W1 + b1)) [n, H] with leading dimension ld >= H;
 * any 2-layer trainer.
 * lt_gcn2_trainer_attach_validation_wide: lt_gcn2_trainer_attach_validation(_rows) for a wide trainer; labels2 as the
 * trainer's labels (ldy2 for BCE), rows may be NULL (all n2 rows).  lt_gcn2_trainer_run_validated then writes val_counts as
 * [n_epochs, C, 3]; the state rule, the snapshot and the accessors keep their meaning.  The attach entry points of the narrow
 * head called on a wide trainer, and this one on a narrow trainer, are LT_ERR_INVALID.
 * lt_eval_head_wide: the head's loss and counts [C, 3] of logits Z [n, ldz] over all rows (rows == NULL; m is not read) or
 * the m listed ones, with lt_eval_head_rows' rules: repeats count, an id outside [0, n) is never dereferenced and is counted
 * in *n_bad (may be NULL), the divisor stays m (times C for BCE); with rows = 0 .. n - 1 the bits of the call without a list.
 * Workspace: lt_eval_head_wide_workspace_bytes(entries scored, C) (0 for unsupported values). */
enum { LT_LOSS_CE = 0, LT_LOSS_BCE = 1 };
int lt_gcn2_trainer_create_wide(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const void *labels, int64_t ldy,
                                int32_t loss_kind, int32_t H, int32_t C, float *W1, float *b1, float *W2, float *b2, double lr,
                                double weight_decay, double dropout, uint64_t seed, void *stream, lt_gcn2_trainer **out);
int lt_gcn2_trainer_counts(const lt_gcn2_trainer *t, int32_t *counts, void *stream);
int lt_gcn2_trainer_hidden(const lt_gcn2_trainer *t, float *H1d, int64_t ld, void *stream);
int lt_gcn2_trainer_attach_validation_wide(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                                           const void *labels2, int64_t ldy2, int32_t keep_best, int32_t patience,
                                           const int32_t *rows, int32_t m, void *stream);
size_t lt_eval_head_wide_workspace_bytes(int32_t m, int32_t C);
int lt_eval_head_wide(const float *Z, int64_t ldz, const void *labels, int64_t ldy, int32_t n, int32_t C, int32_t loss_kind,
                      const int32_t *rows, int32_t m, float *loss, int32_t *counts, int32_t *n_bad, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ---- the wide head on the 3-layer trainer.  Additive within ABI 5. ----
 * lt_gcn3_trainer_create_wide is lt_gcn3_trainer_create with the class layer and the loss head of
 * lt_gcn2_trainer_create_wide behind the two hidden layers: labels, ldy and loss_kind as there, widths H1, H2 <= 256 and
 * C <= 256.  The handle is a lt_gcn3_trainer: _run, _run_validated, _grads, _logits, _hidden, _epoch, _val_state,
 * _restore_best, _val_logits and _destroy work on it.  record [n_epochs, 2] = (loss, sum over the classes of tp).  The mask
 * contract is GCN3's (layer words 0 and 1): a narrow and a wide GCN3 trainer of one seed draw the same masks.  No float
 * atomics: run(a + b) equals run(a); run(b) and two trainers agree bit for bit.  LT_ERR_INVALID with a message naming the
 * value, nothing allocated: H1 or H2 > 256, C > 256, an unknown loss_kind, ldy < C for LT_LOSS_BCE, a NULL pointer.
 * lt_gcn3_trainer_counts: lt_gcn2_trainer_counts for a wide 3-layer trainer.
 * lt_gcn3_trainer_attach_validation_wide: lt_gcn2_trainer_attach_validation_wide for a wide 3-layer trainer; val_counts are
 * [n_epochs, C, 3].  The narrow attach entry points on a wide trainer, and this one on a narrow trainer, are
 * LT_ERR_INVALID with a message naming the right call. */
int lt_gcn3_trainer_create_wide(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const void *labels, int64_t ldy,
                                int32_t loss_kind, int32_t H1, int32_t H2, int32_t C, float *W1, float *b1, float *W2, float *b2,
                                float *W3, float *b3, double lr, double weight_decay, double dropout, uint64_t seed, void *stream,
                                lt_gcn3_trainer **out);
int lt_gcn3_trainer_counts(const lt_gcn3_trainer *t, int32_t *counts, void *stream);
int lt_gcn3_trainer_attach_validation_wide(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                                           const void *labels2, int64_t ldy2, int32_t keep_best, int32_t patience,
                                           const int32_t *rows, int32_t m, void *stream);

/* ---- training on a listed subset of the rows: transductive training.  Additive within ABI 5. ----
 * The reference's loss on the datasets whose adj_train is the whole graph (gcn_trainer.py:150-156:
 * model(features_train, adj_train)[idx_train] against labels_train[idx_train]): the whole graph is forwarded, the loss is taken
 * over m listed rows.  rows: HOST int32 [m], distinct ids in [0, n), any order; the library checks the list, copies it to the
 * device and owns the copy (the caller's array is its own again when the call returns).  m = 0 (rows NULL or not) restores
 * "all rows".  May be called between runs on either head, before or after attach_validation*; it waits for `stream` (a setup
 * call, like lt_graph_create) and zeroes the trainer's dZc on it: pass the stream the trainer's runs use, or call it when the
 * last run has completed (the zeroing must not overtake an epoch in flight).  Replacing or clearing a list waits for the
 * whole device before the old copy is freed.  LT_ERR_INVALID with a message naming the position and the
 * value, the trainer unchanged: an id outside [0, n), a repeated id, m < 0, m > n, rows NULL with m > 0.
 * With a list set: loss = the mean over the listed rows (CE: / m, BCE: / (m C)); record[1] and lt_gcn*_trainer_counts count
 * the listed rows only; dZc has the all-rows formula with m in place of n on the listed rows and is +0 on every other row;
 * the class-bias gradient is the sum of dZc over the list in list order (thread t of the narrow head's reduce takes positions
 * t, t + 256, ...; the wide head's blocks take their tiles of positions in order).  Everything behind dZc -- A^T dZc, the
 * hidden layers' backward, the TN products, Adam, the mirrors -- is the unchanged chain over all n rows, and validation,
 * snapshots and early stopping do not see the list.  The per-row arithmetic is the all-rows head's, operation for
 * operation: the list 0 .. n - 1 trains the bits of a trainer without a list.  The head costs O(m) per epoch. */
int lt_gcn2_trainer_set_train_rows(lt_gcn2_trainer *t, const int32_t *rows, int32_t m, void *stream);
int lt_gcn3_trainer_set_train_rows(lt_gcn3_trainer *t, const int32_t *rows, int32_t m, void *stream);

/* ---- the feature-only baselines, trained in minibatches.  Additive within ABI 5. ----
 * The reference's OneLayerMLP / SingleHiddenLayerMLP (gcn/models.py:91-120) under MLPTrainer (mlp_trainer.py): no graph.
 *   depth 2: Z1 = X_b W1 + b1, H1d = dropout_p(relu(Z1)), Z2 = H1d W2 + b2      (W1 [F, H], b1 [H], W2 [H, C], b2 [C])
 *   depth 1: Z = X_b W + b, no hidden layer, no dropout                                (W1 = W [F, C], b1 = b [C]; W2, b2, H not read)
 * X_b = the rows of the borrowed X [n, ldx] one batch of the epoch's row order names; it is never materialised.
 * lt_mlp_trainer_create borrows X, labels and the parameter tensors (device, project layout [in, out], updated in place) and
 * owns the Adam moments and every intermediate.  loss_kind / labels / ldy as lt_gcn2_trainer_create_wide, taken over the
 * batch's own rows: a batch of b rows divides by b (CE) or b C (BCE), the last, shorter batch of an epoch by its own size.
 * LT_ERR_INVALID with a message naming the value, nothing allocated: depth other than 1 / 2, H outside [1, 256] (depth 2), C
 * outside [1, 256], batch_size < 1, n < 1, F < 1, ldx < F, an unknown loss_kind, ldy < C for LT_LOSS_BCE, dropout outside
 * [0, 1], lr or weight_decay < 0, a NULL pointer.
 * One step (s = optimiser steps since creation): forward, loss head (the step's loss and the sum of tp: for CE the correct
 * count), dZ2, dW2 = H1d^T dZ2, db2, dZ1 = [H1d > 0] (dZ2 W2^T) / (1 - p), db1, dW1 = X_b^T dZ1, then one Adam step under
 * lt_adam_step's contract with step number s + 1 (betas 0.9 / 0.999, eps 1e-8, weight decay added to the gradient).
 * Dropout: element (j, h), j = the row's position inside its batch, i = j H + h, is kept iff word (i & 3) of Philox4x32-10
 * with counter (q lo, q hi, s, 0), q = i >> 2, key (seed lo, seed hi) is >= floor(p 2^32); kept values are scaled by
 * (float)(1 / (1 - p)); p = 0 draws nothing, p = 1 keeps nothing.
 * lt_mlp_trainer_run enqueues every step of n_epochs epochs on `stream`, no host synchronisation: epoch e's batches are
 * order[e, 0 .. B), [B .. 2 B), ..., the last one n - (ceil(n / B) - 1) B rows.  order: device int32 [n_epochs, n], one
 * permutation per epoch (not checked to be one: a repeated row counts twice), or NULL for the Philox shuffle: the key of row r
 * in epoch e (e = epochs since creation) is word 0 of Philox4x32-10 with counter (r, 0, e, 2), key (seed lo, seed hi); the
 * epoch's order is the rows sorted ascending by (key, r).  An id outside [0, n) is never used as an address (row 0 stands in)
 * and raises the probe-list flag of lt_node_check: LT_ERR_INDEX from it, or from the next call that finds it.  batch_size >= n
 * with the identity order is the reference's full-batch branch.  record: device fp32 [n_epochs ceil(n / B), 2] = (loss, sum of
 * tp) per step, or NULL.  No float atomics, every sum in a fixed order that depends on the step's shapes alone: two trainers
 * given the same inputs agree bit for bit and run(a + b) equals run(a); run(b).
 * lt_mlp_trainer_step enqueues ONE step over the b rows rows[0 .. b) (device int32, 1 <= b <= min(batch_size, n), ids checked
 * as above): the step lt_mlp_trainer_run takes for that batch, bit for bit; it advances the step count, not the epoch count.
 * record: device fp32 [2] or NULL.
 * Test accessors: lt_mlp_trainer_grads -- the LAST step's gradients before weight decay (depth 1: dW1 = dW, db1 = db, the other
 * two not written); lt_mlp_trainer_logits -- its train-mode logits [rows of that step, ldz], rows in batch order;
 * lt_mlp_trainer_counts -- steps and epochs run and the last step's row count (any may be NULL); lt_mlp_trainer_order -- the
 * last Philox order, int32 [n] (LT_ERR_INVALID before any epoch ran under it).
 * lt_mlp_forward: eval-mode logits Z [m, ldz] of rows[0 .. m) of any X2 [n2, ldx2] (rows == NULL: all n2 rows, m not read),
 * through the trainer's forward kernels with the mask off: with p = 0 a step's logits are these bits.  Row ids are checked
 * as above.  workspace: device, 16-byte aligned, lt_mlp_forward_workspace_bytes(rows scored, F, depth, H, C) bytes (0 for
 * unsupported values), else LT_ERR_WORKSPACE. */
typedef struct lt_mlp_trainer lt_mlp_trainer;
int lt_mlp_trainer_create(const float *X, int64_t ldx, int32_t n, int32_t F, const void *labels, int64_t ldy, int32_t loss_kind,
                          int32_t depth, int32_t H, int32_t C, float *W1, float *b1, float *W2, float *b2, int32_t batch_size,
                          double lr, double weight_decay, double dropout, uint64_t seed, void *stream, lt_mlp_trainer **out);
int lt_mlp_trainer_run(lt_mlp_trainer *t, int32_t n_epochs, const int32_t *order, float *record, void *stream);
int lt_mlp_trainer_step(lt_mlp_trainer *t, const int32_t *rows, int32_t b, float *record, void *stream);
int lt_mlp_trainer_grads(const lt_mlp_trainer *t, float *dW1, float *db1, float *dW2, float *db2, void *stream);
int lt_mlp_trainer_logits(const lt_mlp_trainer *t, float *Z, int64_t ldz, void *stream);
int lt_mlp_trainer_counts(const lt_mlp_trainer *t, int64_t *steps, int64_t *epochs, int32_t *last_rows);
int lt_mlp_trainer_order(const lt_mlp_trainer *t, int32_t *order, void *stream);
int lt_mlp_trainer_destroy(lt_mlp_trainer *t);
size_t lt_mlp_forward_workspace_bytes(int32_t m, int32_t F, int32_t depth, int32_t H, int32_t C);
int lt_mlp_forward(const float *X2, int64_t ldx2, int32_t n2, int32_t F, int32_t depth, int32_t H, int32_t C, const float *W1,
                   const float *b1, const float *W2, const float *b2, const int32_t *rows, int32_t m, float *Z, int64_t ldz,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- per-kernel timing (used by bench.py for the roofline object) --------------------------
 * lt_profile_enable(mask): bit k of mask set = launches of kernel class k are bracketed by a pair of
 * hipEvents on the caller's stream (mask 0 = off, -1 = every class; an event pair costs a few
 * microseconds of stream time, so a timed region should enable only what it reports -- and may sample:
 * lt_set_tuning("profile_every", N) brackets only every N-th launch group of an enabled class).
 * lt_profile_summary synchronises on the recorded events and returns the summed duration and
 * launch count of one kernel class.  No reference counterpart (the reference only
 * has wall-clock prints, attacker.py:213,231). */
typedef enum lt_kernel_id {
    LT_K_GEMM = 0,        /* k_gemm_f32_mfma                           */
    LT_K_LAYER1 = 1,      /* k_layer1 (baseline fused SpMM1+ReLU+W2)   */
    LT_K_LAYER2 = 2,      /* k_layer2 (baseline SpMM2 + b2)            */
    LT_K_PERTURB = 3,     /* (unused since the perturbation moved into the probe-row GEMM's loads; id kept) */
    LT_K_FULL_A = 4,      /* k_full_stageA / k_full_stageA_lds: batched perturbed SpMM1+ReLU+W2 */
    LT_K_FULL_B = 5,      /* k_full_stageB: SpMM2 on observed rows + diff + norm    */
    LT_K_ITEM_A = 6,      /* k_item_stageA (sparse / delta)            */
    LT_K_ITEM_B = 7,      /* k_item_stageB (sparse / delta)            */
    LT_K_SPMM = 8,        /* k_spmm_rows / k_spmm_narrow               */
    LT_K_FP64_PRODUCT = 9,/* S1d = X*W1 in fp64: k_s1d_feature_rows (+ the reference row's product), or k_gemm_f64acc_128 + k_sum_slabs_f64 */
    LT_K_FP64_SPMM = 10,  /* Z1d = A_hat*S1d + b1: k_spmm_f64 / k_rows_tiled_f64 (+ long-row combine) */
    LT_K_ITEM_BITS = 11,  /* k_item_bits (+ the pair-mark kernels): item offsets, (probe, row) table, membership bitmap */
    LT_K_SELECT_HIST = 12,    /* lt_top_pairs_lower: the clear of its workspace header + the four k_sel_hist digit passes */
    LT_K_SELECT_COLLECT = 13, /* lt_top_pairs_lower: k_sel_count + k_sel_scan + k_sel_write (the ordered compaction) */
    LT_K_METRICS_SORT = 14,   /* lt_score_curve: the clear of its workspace header, k_mc_keys and the four hist / scan / scatter passes */
    LT_K_METRICS_CURVE = 15,  /* lt_score_curve: k_mc_count + k_mc_block_scan + k_mc_write + k_mc_terms + k_mc_summary */
    LT_K_COUNT = 16
} lt_kernel_id;
int lt_profile_enable(int mask);
int lt_profile_reset(void);
int lt_profile_summary(int kernel_id, double *total_ms, int64_t *launches);
/* "profile_every" = N samples whole CALLS of lt_influence_rows* (every scope of a sampled call is bracketed, none of the others):
 * the number of calls sampled since lt_profile_enable -- a class's time per call = its total / this, however many scopes it opens */
int lt_profile_calls(int64_t *calls_sampled);

#ifdef __cplusplus
}
#endif
#endif /* LINKTELLER_HIP_H */
