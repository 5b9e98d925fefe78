/*
 * gem_hip.h -- C ABI of libgem_hip.so, the MI355X (gfx950) backend for the
 * learn_embedding() hot path of GEM's HOPE / GraphFactorization / node2vec.
 *
 * Plain C: pointers, sizes and opaque handles only.  No torch types.
 * Conventions
 *   - every function returns 0 on success, <0 on error (GEMHIP_E_*); the message
 *     is available from gemhip_last_error() (thread-local, valid until the next
 *     failing call on that thread);
 *   - the CALLER owns every host buffer; the library keeps no host pointer after
 *     a call returns.  Device state lives in opaque handles that the caller
 *     destroys;
 *   - `stream` arguments are a hipStream_t passed as void* (NULL = the null
 *     stream).  Calls taking a stream only ENQUEUE work; everything else is
 *     blocking;
 *   - row-major everywhere; embeddings are float32 [n][d] on the device
 *     (the Python layer returns float64 like the reference does).
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the GEM repository).  INTEGRATION.md shows the ctypes stub a GEM maintainer
 * would add.
 */
#ifndef GEM_HIP_H
#define GEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEMHIP_VERSION 100 /* 0.1.0 */

#define GEMHIP_OK 0
#define GEMHIP_E_INVALID (-1)  /* bad argument */
#define GEMHIP_E_HIP (-2)      /* HIP runtime error (no device, OOM, launch failure) */
#define GEMHIP_E_UNSUPPORTED (-3)
#define GEMHIP_E_NOTCONVERGED (-4)

/* ------------------------------------------------------------------ runtime */
int gemhip_version(void);
const char *gemhip_last_error(void);
int gemhip_device_count(int *n);
int gemhip_set_device(int device);
/* device-side helpers so a host (numpy / torch) can hand over or fetch buffers */
int gemhip_malloc(void **dptr, int64_t bytes);
int gemhip_free(void *dptr);
int gemhip_memcpy_h2d(void *dst_dev, const void *src_host, int64_t bytes);
int gemhip_memcpy_d2h(void *dst_host, const void *src_dev, int64_t bytes);
int gemhip_synchronize(void *stream);
/* Where the wall time of the LAST one-shot call on this thread went (gemhip_gf_train, gemhip_n2v_train, gemhip_hope: the drop-ins
 * for gf.py:55-72, node2vec.py:35-48 and hope.py:28-36, whose callers time `learn_embedding` as a whole -- SURVEY 8d "API wall"):
 * out[8] = {total_seconds, host_prepare_seconds (CSR sort, alias / unigram tables, plans), h2d_seconds, kernel_seconds (HIP events),
 * d2h_seconds, 0, 0, 0}.  gemhip_cc_labels and gemhip_lcc (the drop-in for graph_util.py:29-34, get_lcc) fill it too: host_prepare is their
 * validation of the arc list, kernel_seconds the sum gemhip_cc_last_kernel_ms splits. */
int gemhip_last_call_phases(double *out);

/* ------------------------------------------------- Graph Factorization (GF)
 * Replaces: gem/embedding/gf.py:81-101 (GraphFactorization.learn_embedding,
 * hot loop :93-100) and the native executable it shells out to,
 * gem/c_src/gf.cpp:130-169 (`gf <graph> <emb> <verbose> <weighted> <d> <eta>
 * <regu> <max_iter> <print_step>`, gf.py:54-72).
 *
 * The edge list is the wire format of that executable (gf.cpp:54-92 /
 * gem/utils/graph_util.py:129-134): m triples (src, dst, w) in the order
 * graph.edges() yields them.  Semantics are the reference's: sequential
 * (Gauss-Seidel) sweeps, only edges with dst > src update, only row `src` is
 * written.  The device schedule reproduces that order exactly (level-scheduled
 * rows + double-buffered table) -- results differ from the fp32
 * CPU loop only by dot-product summation order.
 *
 * PRECONDITION (checked; GEMHIP_E_INVALID otherwise): every firing edge
 * (dst > src) reads a row that, in file order, has had either all or none of
 * its updates of the sweep -- always true when a source's edges are contiguous
 * (what graph.edges() and saveGraphToEdgeListTxt produce).  gf.cpp:152-164
 * processes an arbitrary file strictly in file order; a list such as
 * (1,2),(0,1),(1,3), where row 0 must see row 1 between its two updates, needs
 * a third version of a row and is rejected rather than silently regrouped.
 */
typedef struct gemhip_gf_plan *gemhip_gf_plan_t;

/* One-shot drop-in for `gf` / GraphFactorization.learn_embedding.
 * X_inout: [n][d] float32, in = initial embedding (gf.cpp:41-52 draws
 * 0.01*N(0,1)), out = trained embedding.  stats (optional, 4 doubles):
 * {kernel_seconds, updates_per_sweep, rows_per_sweep, levels}. */
int gemhip_gf_train(int64_t n, int64_t m, const int32_t *src, const int32_t *dst,
                    const float *w /* NULL = all 1.0 */, int32_t d, float eta,
                    float regu, int32_t max_iter, float *X_inout, double *stats);

/* Staged form (graph resident in HBM across calls; used by bench.py and the
 * multi-GPU driver).  [row_begin,row_end) restricts the plan to the source
 * rows this rank owns (source-node sharding); pass 0,n for all. */
int gemhip_gf_plan_create(int64_t n, int64_t m, const int32_t *src,
                          const int32_t *dst, const float *w, int32_t d,
                          int64_t row_begin, int64_t row_end,
                          gemhip_gf_plan_t *out);
int gemhip_gf_plan_destroy(gemhip_gf_plan_t plan);
/* Use caller-provided DEVICE buffers [n][d] float32 for the two table copies
 * (e.g. torch tensors, so RCCL can all-gather them).  Both must hold the same
 * initial embedding.  Without this call the plan allocates its own. */
int gemhip_gf_plan_bind(gemhip_gf_plan_t plan, void *dX_a, void *dX_b);
int gemhip_gf_plan_set_embedding(gemhip_gf_plan_t plan, const float *X_host);
/* 0.01*N(0,1)-style init on the device (Philox4x32-10 + Box-Muller), same
 * distribution as gf.cpp:41-52 / gf.py:92. */
int gemhip_gf_plan_init_embedding(gemhip_gf_plan_t plan, uint64_t seed, float scale);
/* Enqueue `nsweeps` sweeps (one sweep = gf.cpp:152-164 over all edges). */
int gemhip_gf_plan_sweeps(gemhip_gf_plan_t plan, int32_t nsweeps, float eta,
                          float regu, void *stream);
/* Source rows a wavefront trains back to back inside one sweep launch (1 = one row per wavefront, gf_sweep_kernel; K > 1 =
 * gf_sweep_rows_kernel, which has the next row's inputs in flight while a row is trained); 0 = auto (by level size).  Every
 * setting gives bit-identical tables -- rows of a level are independent.  No reference counterpart (gf.cpp is one thread). */
int gemhip_gf_plan_set_rows_per_wave(gemhip_gf_plan_t plan, int32_t rows_per_wave);
/* Sweeps per COOPERATIVE launch (gf_sweeps_coop_kernel: a resident grid, sweeps separated by a grid barrier instead of a kernel boundary): 0 = off
 * (default: one launch per sweep and level), k > 1 = up to k sweeps per launch on single-level plans without hub rows (others keep the launch loop);
 * max_grid caps the workgroups of that launch (0 = what the occupancy allows).  Bit-identical tables either way.  No reference counterpart. */
int gemhip_gf_plan_set_fused_sweeps(gemhip_gf_plan_t plan, int32_t sweeps_per_launch, int32_t max_grid);
/* Blocked hub rows: 0 = off (default), 1 = on; anything else is GEMHIP_E_INVALID.  On, the rows the plan marks as hub rows (GEMHIP_GF_HUB_EDGES
 * firing edges or more, default 1024) apply their edges B at a time -- one Gram matrix of the B neighbour rows on the fp32 matrix units, B scalar
 * steps, one GEMV -- instead of B dependent dot-and-axpy steps (gf_hub_block_kernel; DESIGN.md "GF: blocked hub rows").  NOT bit-identical to the row
 * kernels: the same updates in another association of the same fp32 operations.  The bound it meets is the one the row kernels meet: every entry
 * within 2e-5 of max|X| of the sequential fp32 loop of gf.cpp:152-164 (tests/test_gf_hub_block_gpu.py).  Deterministic: a row's result depends only on
 * its edge list and inputs.  All other rows are computed exactly as with the switch off.  No effect on plans without hub rows; accepted without
 * effect on a unit plan.  GEMHIP_GF_HUB_BLOCK=1 in the environment sets the initial value of every plan at its creation (so it reaches
 * gemhip_gf_train and gemhip_gf_train_multi).  No reference counterpart. */
int gemhip_gf_plan_set_hub_block(gemhip_gf_plan_t plan, int32_t on);
/* block = the B in effect (0 when the switch is off, and on a unit plan), hub_rows = the hub rows of the plan (all levels). */
int gemhip_gf_plan_hub_block(gemhip_gf_plan_t plan, int32_t *block, int64_t *hub_rows);
int gemhip_gf_plan_get_embedding(gemhip_gf_plan_t plan, float *X_host);
/* Device pointer of the CURRENT table (the one holding the latest sweep). */
int gemhip_gf_plan_current(gemhip_gf_plan_t plan, void **dX);
/* info (8 int64): {updates_per_sweep, rows_per_sweep, levels, n, d,
 * algorithmic_bytes_per_sweep, rows per wavefront of the largest level's launch, 1 on a unit schedule
 * (gemhip_gf_plan_create_any_order; rows_per_sweep then counts units) else 0} */
int gemhip_gf_plan_info(gemhip_gf_plan_t plan, int64_t *info);
/* Any edge order, exactly as gf.cpp:152-164 walks it (DESIGN.md "GF: any edge order").  A list gemhip_gf_plan_create accepts gets exactly that
 * plan (all rows; same levels, kernels and speed).  Any other list -- a shuffled file, two sorted files concatenated, edges appended later -- gets a
 * UNIT schedule: a unit is a run of one row's edges that one wavefront applies in file order (gf_sweep_units_kernel), units are placed in levels so
 * that two edges touching a row one of them writes run in file order; one launch per level, in stream order.  flags bit 0 forces the unit schedule
 * on a list the row schedule represents (tests, A/B); the tables are bit-identical either way.  The plan works with every gemhip_gf_plan_* call;
 * on a unit plan gemhip_gf_plan_info reports {.., units, levels, .., info[6] = 1, info[7] = 1}, and set_rows_per_wave / set_fused_sweeps are accepted
 * and change nothing.  A unit schedule covers all rows of one device (no row range).  Like every plan it needs the two tables to agree on the rows
 * that never fire: set_embedding / init_embedding fill both tables (own or bound) with the same values; after gemhip_gf_plan_bind alone that is
 * the caller's promise ("both must hold the same initial embedding").  Needs fewer than 2^31 firing edges. */
int gemhip_gf_plan_create_any_order(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int32_t d, int32_t flags,
                                    gemhip_gf_plan_t *out);
/* Unit plans: run every maximal run of two or more consecutive levels of at most max_units units (0 = off, at most 16) in ONE launch of one
 * 16-wavefront workgroup, with a workgroup barrier where the level loop has a kernel boundary.  Launches per sweep = (levels with more than
 * max_units units) + (runs of consecutive smaller levels).  Bit-identical tables either way.  Accepted without effect on a row plan. */
int gemhip_gf_plan_set_fused_levels(gemhip_gf_plan_t plan, int32_t max_units);
/* The unit schedule of a list, on the host alone (no HIP call): per edge its unit (numbered in file order of first edge), the unit's level,
 * and flags (bit 0: the neighbour is read from the working table X_new, bit 1: the unit loads its own row from X_new); edges that do not fire
 * (dst <= src) get -1 in all three.  counts = {units, levels}.  Any output may be NULL. */
int gemhip_gf_any_order_schedule(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, int32_t *unit_out, int32_t *level_out,
                                 int32_t *flags_out, int64_t *counts);
/* gf.cpp:94-113 objective on the device table: out = {f1, f2}. `m` edges as in
 * plan_create but over ALL edges (no dst>src filter), like the reference.  An edge outside [0, n), or m > 0 with a NULL src or dst, is
 * GEMHIP_E_INVALID before any device call (the first offender is named as gemhip_gf_train names it). */
int gemhip_gf_objective(int64_t n, int64_t m, const int32_t *src,
                        const int32_t *dst, const float *w, int32_t d,
                        const float *X_host, double *out);

/* ------------------------------------------------------------------ node2vec
 * Replaces: gem/embedding/node2vec.py:27-54 (node2vec.learn_embedding), i.e. the
 * subprocess call of the prebuilt SNAP binary gem/c_exe/node2vec with
 * `-i:tempGraph.graph -o:tempGraph.emb -d -l -r -k -e -p -q -v -dr -w`
 * (node2vec.py:35-46) and the text files around it (graph_util.py:137-140, 161-169).
 *
 * Graph: CSR by source (row_ptr int64[n+1], col int32[nnz], w float32[nnz] or NULL
 * for unit weights) -- what the binary builds from the "%d %d %f" edge list.
 *
 * flags (bit set): 1 = short walks are padded with token 0 and trained on, like the
 * binary's zero-initialised walk matrix (else padded with -1 and skipped);
 * 2 = negative sampling indexes the alias table the way the binary's RndUnigramInt
 * does (KTable[floor(u*n)], see oracle/n2v_oracle.c); 4 = deterministic: SGNS runs
 * on ONE wavefront in walk order (bit-reproducible, for parity tests; slow);
 * 8 = first hop of a walk is uniform over neighbours, like SimulateWalk.
 * GEMHIP_N2V_SNAP_COMPAT = 1|2|8 mirrors the reference binary. */
#define GEMHIP_N2V_PAD_ZERO 1
#define GEMHIP_N2V_UNIGRAM_QUIRK 2
#define GEMHIP_N2V_DETERMINISTIC 4
#define GEMHIP_N2V_UNIFORM_FIRST_HOP 8
#define GEMHIP_N2V_SNAP_COMPAT 11
#define GEMHIP_N2V_VOCAB_ORDER 16     /* unigram alias table laid out the way the binary lays it out: over the nodes that occur, in order of first appearance
                                         in the walk matrix (LearnVocab renames the tokens that way), instead of over all nodes in id order -- same distribution,
                                         the binary's TABLE (gemhip_n2v_build_unigram_vocab_order; single-GPU path).  GEMHIP_N2V_SNAP_COMPAT | 16 = 27 is what
                                         gem_amd.embedding.node2vec passes by default */
#define GEMHIP_N2V_SNAP_LAYOUT 27
#define GEMHIP_N2V_NO_WINDOW_CACHE 128 /* A/B switch: train with the round-1 kernel (every context row goes to memory for every pair) instead of the
                                          LDS-window kernel (gemhip_sgns_set_window_cache); same arithmetic and draws either way */
/* (bits 32 and 64 selected two round-1/2 experiments -- 16-byte row accesses, negatives shared per centre word -- that were measured slower /
 * are not the reference's sampling; round 3 removed them from the library, see DESIGN.md 3.3 and the git history of gem_amd/csrc/n2v.hip) */

typedef struct gemhip_n2v *gemhip_n2v_t;

/* One-shot drop-in for the binary: X_out [n][d] float32 = SynPos in node-id order
 * (what loadEmbedding reads back).  alpha0 = 0.025, 5 negatives as in the binary.
 * stats (optional, 4 doubles): {walk_seconds, sgns_seconds, tokens, rows_uniform}. */
int gemhip_n2v_train(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                     const float *w, int32_t d, int32_t walk_len, int32_t num_walks,
                     int32_t window, int32_t epochs, float p, float q, uint64_t seed,
                     int32_t flags, float *X_out, double *stats);

/* Staged form (graph, walks and tables resident in HBM; used by bench.py, the
 * multi-GPU driver and the parity tests). */
int gemhip_n2v_create(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                      const float *w, gemhip_n2v_t *out);
int gemhip_n2v_destroy(gemhip_n2v_t h);
/* PreprocessTransitionProbs: first-order Vose alias tables per row (no-op when every
 * row has equal weights).  2nd-order bias is applied by rejection inside the walk.
 * Rows of fewer than 2048 neighbours: GetNodeAlias's loop on one lane, fp32, bit for bit
 * oracle_alias_build_f32; longer (hub) rows: the loop's closed form on a workgroup, fp64
 * sums in a fixed order, bit for bit oracle_alias_build_hub (same alias targets as the
 * sequential loop). */
int gemhip_n2v_build_alias(gemhip_n2v_t h, void *stream);
/* InitUnigramTable in the binary's layout (flags bit GEMHIP_N2V_VOCAB_ORDER of the one-shot call): see n2v.hip.  Needs the walks and the counts
 * (gemhip_n2v_vocab) of the whole corpus on this handle.  `flags`: bit 2 (the RndUnigramInt quirk) decides what a slot maps to.  n_vocab_out: nodes
 * that occur; order_out[n_vocab]: their ids in first-appearance order; UT_out / KT_out [n_vocab]: the alias table in the binary's renamed indices
 * (all optional, caller-sized n).  gemhip_sgns_train uses this table from then on (gemhip_n2v_build_unigram switches back). */
int gemhip_n2v_build_unigram_vocab_order(gemhip_n2v_t h, int32_t flags, int64_t *n_vocab_out, int32_t *order_out, float *UT_out, int32_t *KT_out);
/* Fetch tables/sorted columns for tests.  Returns 1 (not an error) when rows are uniform
 * and no tables exist. */
int gemhip_n2v_get_alias(gemhip_n2v_t h, float *U_host, int32_t *K_host, int32_t *col_sorted_host);
/* Walks start from the m nodes that occur in the edge list (the binary never sees an isolated node):
 * gemhip_n2v_start_nodes returns m.  SimulateWalk for global walk ids [walk_begin, walk_end) of m*num_walks
 * (walk id r*m + j starts at the j-th node of round r's permutation of those m nodes): this rank's shard. */
int gemhip_n2v_start_nodes(gemhip_n2v_t h, int64_t *m);
int gemhip_n2v_walks(gemhip_n2v_t h, float p, float q, int32_t num_walks, int32_t walk_len,
                     uint64_t seed, int32_t flags, int64_t walk_begin, int64_t walk_end,
                     void *stream);
int gemhip_n2v_set_walks(gemhip_n2v_t h, const int32_t *walks_host, int64_t nwalks,
                         int32_t walk_len, int64_t walk_id_offset);
int gemhip_n2v_get_walks(gemhip_n2v_t h, int32_t *walks_host);
int gemhip_n2v_walks_ptr(gemhip_n2v_t h, void **d_walks, int64_t *nwalks, int32_t *walk_len);
/* LearnVocab: token counts of the local walks into a device int32[n] (counts_ptr exposes
 * it so a multi-GPU driver can all-reduce it), then InitUnigramTable on the host. */
int gemhip_n2v_vocab(gemhip_n2v_t h, void *stream);
int gemhip_n2v_counts_ptr(gemhip_n2v_t h, void **d_counts);
/* Use a caller-owned DEVICE int32[n] as the count buffer (e.g. a torch tensor to all-reduce). */
int gemhip_n2v_bind_counts(gemhip_n2v_t h, void *d_counts);
int gemhip_n2v_build_unigram(gemhip_n2v_t h, int32_t *counts_out, float *UT_out, int32_t *KT_out);
/* InitPosEmb / InitNegEmb.  dSynPos/dSynNeg: optional caller-owned DEVICE tables
 * [n][d] float32 (both or neither). */
int gemhip_sgns_init(gemhip_n2v_t h, int32_t d, uint64_t seed, void *dSynPos, void *dSynNeg);
/* (centre, context) pairs trained since creation / the last reset -- the unit of SURVEY 8(d)'s
 * SGNS byte count (14*4d bytes per pair). */
int gemhip_sgns_pairs(gemhip_n2v_t h, int64_t *pairs, int32_t reset);
/* Cap on concurrently training wavefronts (Hogwild width).  0 = auto: the number of wavefronts for which the expected fraction of
 * row stores that overwrite another wavefront's store, rho = W x 5 x w / n_eff (w = the load-to-store window of a negative row in pair
 * steps: ~0.4 with reload-on-update, prefetch + 1 without; n_eff = 1 / sum q_v^2 over the negative-sampling distribution: n on a
 * uniform graph, far less with hubs), stays <= 1.5 % -- n_eff/133 with reload-on-update, n_eff/1000 without -- never more than the
 * device holds (on MI355X 1792 = seven per CU when every context row is cached, 1536 otherwise), over the cold rows only once hot rows take
 * atomic adds (gemhip_sgns_set_hot_rows), at most 2 % of the rows that occur; graphs below 8192 nodes: 1/16 of the table open at most.  Derivation and the
 * measurements behind it: DESIGN.md 3.3, scripts/hogwild_emul. */
int gemhip_n2v_set_max_waves(gemhip_n2v_t h, int32_t max_waves);
/* LDS window of TrainModel's context rows (no reference counterpart: the binary keeps its tables in host RAM).
 * radius = tokens either side of the centre word whose SynPos row stays in LDS between its first and last use
 * (-1 = auto = min(window, 10); 0 = off); delta_writeback: a row leaves the window as `row_now + (working - loaded)`
 * so that concurrent wavefronts' updates survive (1), or is written back as is (0); -1 = auto (1 unless one wavefront trains). */
int gemhip_sgns_set_window_cache(gemhip_n2v_t h, int32_t radius, int32_t delta_writeback);
/* How a Hogwild launch treats the rows it shares with other wavefronts (no reference counterpart: the binary's threads race on plain
 * doubles).  prefetch_pairs: (centre, context) pairs whose five negative rows are requested ahead of their use (2 default, 1; 0 = keep).
 * reload_on_update (1 default, 0, -1 = keep): apply a negative row's update to the row as it is at store time -- a second fetch right
 * after the dot products, `row_now + g * xc` -- and the centre's positive row as an atomic add of what the centre changed, instead of
 * storing copies that are (prefetch_pairs + 1) pair steps / one centre old and overwrite whatever other wavefronts stored meanwhile. */
int gemhip_sgns_set_hogwild(gemhip_n2v_t h, int32_t prefetch_pairs, int32_t reload_on_update);
/* Hot rows: a node with at least min_count tokens in the corpus never enters a wavefront's LDS window of context rows (its row is fetched
 * per pair and updated by atomic add) -- on a power-law graph a hub would otherwise sit in hundreds of windows at once and the deltas its
 * copies leave with add up.  -1 = auto: the nodes expected to be in another wavefront's window at any time, tokens / ((W-1) x (2R+1));
 * 0 = off.  No reference counterpart. */
int gemhip_sgns_set_hot_rows(gemhip_n2v_t h, int32_t min_count);
/* The launch gemhip_sgns_train would choose for one pass over `nwalks` walks of a corpus with these token counts (counts[n], as
 * gemhip_n2v_build_unigram returns them) on a handle with default knobs -- host arithmetic only, no device needed: which kernel (0 = no LDS
 * window, 1 = window with overwrite on leave, 2 = window with delta write-back: the Hogwild path), how many concurrent wavefronts (= walks
 * trained at once; the rule rho = W x 5 x w / n_eff <= 1.5 % of DESIGN.md 3.3), the hot-row token threshold (0: none), the effective table
 * size n_eff = 1 / sum q_v^2 of the unigram^0.75 distribution and the same over the cold rows only.  Any out pointer may be NULL.  No
 * reference counterpart (the binary runs as many threads as the machine has cores). */
int gemhip_sgns_plan_launch(const int32_t *counts, int64_t n, int32_t d, int32_t window, int32_t walk_len, int64_t nwalks, int32_t flags,
                            int32_t *kernel, int32_t *waves, int32_t *hot_threshold, double *n_eff, double *n_eff_cold);
/* What the LAST gemhip_sgns_train / gemhip_sgns_train_part on this handle actually launched -- the planner's choice after every knob and
 * environment override (GEMHIP_SGNS_MAX_WAVES, ...) and for the handle's own unigram-table layout: kernel (as gemhip_sgns_plan_launch), concurrent
 * wavefronts, hot-row token threshold, and the FRESH HOT ROWS bits in force (0 when the launch had no hot rows).  bench.py reports this instead of
 * replaying the planner.  Any out pointer may be NULL. */
int gemhip_sgns_last_launch(gemhip_n2v_t h, int32_t *kernel, int32_t *waves, int32_t *hot_threshold, int32_t *fresh);
/* LOCALLY HOT ROWS.  A node whose tokens are packed into few walks -- at least `per_walk` tokens per walk that contains it (default 8; 0 = off; -1 keeps the
 * handle's setting) -- sits in the LDS window of every such walk from its first token to its last, not for 2R+1 centres: the two nodes of an isolated edge
 * make up all 80 tokens of each of their 20 walks.  Two wavefronts training two of those walks at once each apply a whole walk's worth of updates to the
 * same base and both deltas are added (measured on R-MAT scale 17: one such pair ends with 14 % more norm than its peers and outranks the true neighbour of
 * dozens of them: 2-5 % of the graph's reconstruction MAP per event).  Hogwild launches of gemhip_sgns_train therefore treat these nodes as hot rows whatever
 * their token count (never cached; per-pair reads and atomic adds).  This call builds the key the kernels compare with the hot-row threshold from the walks
 * and counts on the handle -- hotkey[v] = INT32_MAX for a locally hot node, else its token count -- and returns how many nodes are locally hot and,
 * optionally, the key (n int32, host).  Needs the WHOLE corpus on the handle (a rank's shard against all-reduced counts would flag everything: the launch
 * skips the rule there).  No reference counterpart (the binary's threads read and write rows in place). */
int gemhip_n2v_locally_hot(gemhip_n2v_t h, int32_t per_walk, int64_t *count, int32_t *hotkey_host);
/* ... from a walk corpus assembled from every rank's shard (device pointer, corpus_rows x walk_len int32, rows of -1 = padding) and the handle's all-reduced
 * counts: the partitioned N-GPU schedule's form.  gemhip_sgns_train_part launches on the handle then treat the locally hot nodes as hot rows. */
int gemhip_n2v_locally_hot_corpus(gemhip_n2v_t h, const void *d_corpus, int64_t corpus_rows, int32_t walk_len, int32_t per_walk, int64_t *count, void *stream);
/* FRESH HOT ROWS (Hogwild launches that have hot rows; gem_amd/csrc/sgns.hpp SgnsArgs::fresh).  bit 0: a hot centre word's positive row takes every
 * pair's update as a returning atomic add and continues from the returned row; bit 1: hot negative rows are re-read right before the dot products.
 * bit 2 (value 4): every negative row with at least GEMHIP_SGNS_NEG_COUNT tokens is updated by atomic add instead of reload + store.
 * Bits 0 and 1 shorten the time between reading a hub row and adding a gradient computed from it (measured: the hubs' staleness falls 4x, the MAP gap does
 * not move: profiles/r06_*.jsonl); all three are A/B knobs, off by default.  No reference counterpart (the binary's Hogwild threads
 * read and write rows in place). */
int gemhip_sgns_set_fresh(gemhip_n2v_t h, int32_t bits);
/* Building block of the SGNS kernel, exposed for its own parity test: in[64][6] per-lane partial sums -> out[64], lane l
 * receiving the wave total of value (l & 4) ? 4 + (l & 1) : (l & 3). */
int gemhip_test_wave_sum6(const float *in_host, float *out_host);
int gemhip_sgns_set_tables(gemhip_n2v_t h, const float *SynPos_host, const float *SynNeg_host);
int gemhip_sgns_get_tables(gemhip_n2v_t h, float *SynPos_host, float *SynNeg_host);
/* TrainModel over LOCAL walks [walk_lo, walk_hi) for epoch `epoch` of `epochs`.
 * tokens_total = tokens of ALL ranks per epoch (the binary's AllWords), token_offset =
 * global word count before local walk 0 -- together they drive the linear alpha decay. */
int gemhip_sgns_train(gemhip_n2v_t h, int32_t window, int32_t neg, float alpha0,
                      int32_t epochs, int32_t epoch, int64_t walk_lo, int64_t walk_hi,
                      int64_t tokens_total, int64_t token_offset, uint64_t seed,
                      int32_t flags, void *stream);

/* Partitioned ("episode") SGNS for N GPUs -- no reference counterpart (the reference is one process); this is the
 * schedule that lets SGNS shard without two GPUs ever writing the same row: node v belongs to
 * partition v % parts with local row v / parts; rank g keeps SynPos partition g, the SynNeg partitions travel around a
 * ring, and in every round a rank trains ONE bucket (contexts of its SynPos partition, centre words of the visiting
 * SynNeg partition) of the walk corpus.  build_unigram_parts: one alias table per partition over local indices
 * (the unigram^0.75 distribution restricted to the partition), from the global counts of the handle. */
int gemhip_n2v_build_unigram_parts(gemhip_n2v_t h, int32_t parts, float *UT_out, int32_t *KT_out);
/* ... in the binary's layout (GEMHIP_N2V_VOCAB_ORDER): partition p = its nodes that occur, in order of first appearance in d_corpus (device pointer: the
 * walks of all ranks in walk-id order, -1 tokens = padding, corpus_tokens int32 entries; NULL = the handle's own walks).  Optional host outputs by local
 * row (UT_out / KT_out [n]), the slot tables (slot_out [n]: partition p's at its offset, -1 beyond its slot count) and the slot counts (nslots_out [parts]). */
int gemhip_n2v_build_unigram_parts_vocab_order(gemhip_n2v_t h, int32_t parts, int32_t flags, const void *d_corpus, int64_t corpus_tokens,
                                               float *UT_out, int32_t *KT_out, int32_t *slot_out, int64_t *nslots_out);
/* One bucket of the partitioned schedule trained in WALK order (round 4; no reference counterpart beyond TrainModel itself): TrainModel
 * (ELF @0x40d6a0) over a walk corpus in device memory, restricted to the pairs whose context is a node of partition ctx_part (rows of
 * dSynPos_part, local index v / parts) and whose centre word is a node of partition word_part (rows of dSynNeg_part; negatives from the
 * unigram table restricted to word_part -- gemhip_n2v_build_unigram_parts; the handle's counts must be the GLOBAL ones).
 * Corpus: nwalks work items.  d_seg == NULL: item i is row i of d_walks, walk id walk_id_offset + i.  Otherwise the corpus is assembled
 * from nseg shards (d_seg = device int64[3 * nseg] = {first row in d_walks, walks present, global id of the first walk} per shard) and item
 * i = r * seg_len + j is walk j of shard r (skipped when j >= walks present); nwalks must equal nseg * seg_len.
 * alpha = alpha0 * max(1 - t / (alpha_tokens_total + 1), 1e-4), t = token_offset + i * walk_len + position, refreshed every 10000 tokens
 * like the binary.  Same kernel and same draws per (walk id, position) as gemhip_sgns_train; over all parts x parts buckets every pair of
 * TrainModel is trained exactly once. */
int gemhip_sgns_train_part(gemhip_n2v_t h, const void *d_walks, int64_t nwalks, int32_t walk_len, const void *d_seg, int32_t nseg,
                           int64_t seg_len, int64_t walk_id_offset, int32_t window, float alpha0, int64_t alpha_tokens_total,
                           int64_t token_offset, int32_t epoch, uint64_t seed, int32_t flags, int32_t ctx_part, int32_t word_part,
                           void *dSynPos_part, void *dSynNeg_part, int32_t d, void *stream);
/* Local walks [walk_lo, walk_hi) copied (device to device, on `stream`) into a caller-owned device buffer. */
int gemhip_n2v_copy_walks(gemhip_n2v_t h, int64_t walk_lo, int64_t walk_hi, void *d_dst, void *stream);

/* ------------------------------------------------------------ N GPUs, one process (RCCL over xGMI)
 * the one-shot drop-ins above with an `n_gpus` argument.  The reference has no multi-device path; these shard the way
 * north_star prescribes -- GF by source row, node2vec by start node -- inside ONE host process that drives n_gpus devices, with the
 * collectives on RCCL (loaded with dlopen on first use: GEMHIP_E_UNSUPPORTED when librccl.so.1 is not there; the single-GPU entry points
 * never need it).  devices: n_gpus device ordinals, NULL = 0 .. n_gpus-1.  A list that names the SAME device n_gpus times runs the ranks as
 * VIRTUAL ranks on that device (test mode: RCCL refuses two ranks on one GPU, the collectives become device-to-device copies; sharding,
 * schedule and kernels are the production ones).  gem_amd/multi_gpu.py is the one-process-per-GPU form of the same schedules.
 *
 * gemhip_gf_train_multi: gemhip_gf_train with the source rows in n_gpus contiguous blocks, an in-place all-gather of the owned row blocks
 * after EVERY sweep -- bit-identical to one GPU (needs the firing sources in ascending id order when n_gpus > 1: GEMHIP_E_UNSUPPORTED
 * otherwise).  stats (optional, 8 doubles): {sweep + exchange seconds, updates per sweep, rows per sweep, exchange bytes per rank per
 * sweep, n_gpus, virtual (0/1), 0, 0}.
 * gemhip_n2v_train_multi: gemhip_n2v_train with walks by start-node shard, an all-reduce of the token counts, one all-gather of the walk
 * shards and the partitioned-table schedule (`episodes` slices of every shard; rank g trains bucket (g, (g+s) % n_gpus) of each with
 * gemhip_sgns_train_part and passes its SynNeg partition around a ring).  stats (optional, 8 doubles): {walk + vocabulary + gather
 * seconds, training seconds, tokens, pairs trained, ring bytes per rank per round, n_gpus, virtual (0/1), bucket launches per rank}.
 * Unigram-table layout: flags with GEMHIP_N2V_VOCAB_ORDER (bit 16, the plugin default) lay every partition's alias table out over its nodes in order
 * of first appearance in the whole corpus (gemhip_n2v_build_unigram_parts_vocab_order: the binary's layout restricted to the partition; with one
 * device it IS gemhip_n2v_train's table, and the deterministic mode gives the same embedding bit for bit); without the bit, in node-id order
 * (gemhip_n2v_build_unigram_parts).  Round 4 ignored the bit here.
 * STATUS of n_gpus > 1 on DISTINCT devices: the RCCL path (grouped in-place ncclAllGather, ncclAllReduce, ncclSend/ncclRecv ring, one
 * non-blocking stream per device, all driven from one host thread) has only ever run with ONE rank (a 1-GPU test pool); with n_gpus > 1
 * it has been exercised as virtual ranks only, where the three collectives are copies on one stream.  Treat the multi-device path as
 * unvalidated until tests/test_multi_capi_gpu.py::test_real_devices_* has run on a box with >= 2 GPUs (they skip otherwise).
 * gemhip_rccl_selftest: communicator create -> all-gather / all-reduce / ring shift of `bytes` per rank on known patterns, every word
 * checked -> destroy. */
int gemhip_gf_train_multi(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int32_t d, float eta,
                          float regu, int32_t max_iter, int32_t n_gpus, const int32_t *devices, float *X_inout, double *stats);
int gemhip_n2v_train_multi(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t d,
                           int32_t walk_len, int32_t num_walks, int32_t window, int32_t epochs, float p, float q, uint64_t seed,
                           int32_t flags, int32_t n_gpus, const int32_t *devices, int32_t episodes, float *X_out, double *stats);
int gemhip_rccl_selftest(int32_t n_gpus, const int32_t *devices, int64_t bytes, double *seconds);

/* ---------------------------------------------------------------------- HOPE
 * Replaces: gem/embedding/hope.py:23-41 (HOPE.learn_embedding): S = inv(I - beta A) (beta A)
 * as dense numpy matrices (:28-31) and u, s, vt = scipy.sparse.linalg.svds(S, k=d//2) (:33).
 *
 * Graph: CSR of A with rows AND columns indexed in graph.nodes order (hope.py:28 uses
 * nx.to_numpy_matrix, whose index is insertion order).  Outputs, all caller-owned float32:
 *   U_sqrtS [n][k] = u * sqrt(s),  V_sqrtS [n][k] = vt.T * sqrt(s)   (hope.py:34-35; X = [U | V]),
 *   sigma [k] ASCENDING like svds (hope.py:33).  Column signs: largest |entry| of each u positive.
 * Solver knobs: oversample (block = k + oversample columns), krylov_steps (Krylov blocks per cycle until pairs
 * start to lock; converged leading pairs are frozen and the freed basis columns -- capacity 1.2 * (krylov_steps + 1)
 * blocks -- deepen the polynomial for the rest), max_restarts, tol (max relative change of the k singular values
 * between cycles; pairs lock at a relative residual of 0.1 * sqrt(tol)).
 * stats (optional, 12 doubles): {device_seconds, spmm_launches, spmm_columns_total, katz_terms,
 * basis_columns, restarts_done, last_sigma_change, beta*sigma_max(A) estimate, host_eig_seconds,
 * host_eig_calls, max relative Ritz residual of the previous cycle,
 * seconds inside SpMM launches (HIP events)}.
 * Symmetric A (A == A^T entry for entry, rows sorted by column, beta > 0, n >= 16384; GEMHIP_HOPE_SYM=0/1 forces it off/on):
 * S = f(A), f(x) = beta x / (1 - beta x), shares A's eigenvectors, so the same triplets -- sigma = |f(lambda)|, v = q,
 * u = sign(f(lambda)) q -- come from a Chebyshev-filtered subspace iteration on A itself (one SpMM per polynomial degree,
 * block-sized Rayleigh-Ritz, locked pairs deflated inside the filter); krylov_steps is unused there, max_restarts bounds the
 * cycles at max(40, 3 * max_restarts), and a run that does not converge is redone by the block-Krylov solver.  stats then
 * carries katz_terms = 0 and restarts_done = filter cycles.
 * Returns GEMHIP_E_NOTCONVERGED when beta*sigma_max(A) >= 0.95 (Katz series too slow). */
/* Staged form: the graph-dependent setup (A and A^T in CSR on the device, Katz series length) is done once. */
typedef struct gemhip_hope_plan *gemhip_hope_plan_t;
int gemhip_hope_plan_create(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w,
                            float beta, gemhip_hope_plan_t *out);
int gemhip_hope_plan_solve(gemhip_hope_plan_t plan, int32_t k, int32_t oversample, int32_t krylov_steps,
                           int32_t max_restarts, float tol, uint64_t seed, float *U_sqrtS, float *V_sqrtS,
                           float *sigma, double *stats);
/* gemhip_hope_plan_solve with U sqrt(S) / V sqrt(S) written to DEVICE memory (n x k floats each; sigma, stats: host): the embedding stays in HBM
 * for a caller that evaluates or post-processes it there.  No reference counterpart (hope.py returns numpy arrays). */
int gemhip_hope_plan_solve_device(gemhip_hope_plan_t P, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol,
                                  uint64_t seed, void *dU_sqrtS, void *dV_sqrtS, float *sigma, double *stats);
int gemhip_hope_plan_destroy(gemhip_hope_plan_t plan);
int gemhip_hope(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w,
                float beta, int32_t k, int32_t oversample, int32_t krylov_steps,
                int32_t max_restarts, float tol, uint64_t seed, float *U_sqrtS, float *V_sqrtS,
                float *sigma, double *stats);
/* hope.py:38-40 `print('SVD error (low rank): %f' % norm(u diag(s) vt - S))`: for the truncated SVD that matrix is S (I - V V^T), and its
 * squared Frobenius norm is estimated with `probes` (1..128; 32 is plenty) Gaussian probe columns, deflated by V, pushed through the Katz series by
 * the solver's own SpMM kernel, with the exactly known ||beta A (I - V V^T)||_F^2 as a control variate.  sigma / V_sqrtS: the k singular values and
 * the n x k block V sqrt(Sigma) a solve returned (host).  frob2_out (optional): err^2 + sum sigma^2, the estimate of ||S||_F^2. */
int gemhip_hope_plan_svd_error(gemhip_hope_plan_t plan, int32_t k, const float *sigma, const float *V_sqrtS, int32_t probes, uint64_t seed,
                               double *err_out, double *frob2_out);
int gemhip_hope_svd_error(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta, int32_t k,
                          const float *sigma, const float *V_sqrtS, int32_t probes, uint64_t seed, double *err_out, double *frob2_out);
/* ... with the U side: ||u diag(s) vt - S||_F^2 = ||S (I - V V^T)||_F^2 + ||S V - U Sigma||_F^2 for orthonormal V (the two parts are orthogonal); the second
 * term is computed exactly (the Katz series on V's k columns) and is ~0 for a converged solve, so a wrong or unconverged U shows in the number exactly as
 * it does in hope.py:38-40's.  The V-only forms above report the truncation error an exact SVD with this V would have.  Columns with sigma[j] <= 0 (k
 * above the rank of S) are skipped.  uside_out (optional): sqrt of the second term alone.  What HOPE(..., verbose=True) prints. */
int gemhip_hope_plan_svd_error_uv(gemhip_hope_plan_t plan, int32_t k, const float *sigma, const float *U_sqrtS, const float *V_sqrtS, int32_t probes,
                                  uint64_t seed, double *err_out, double *frob2_out, double *uside_out);
int gemhip_hope_svd_error_uv(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta, int32_t k,
                             const float *sigma, const float *U_sqrtS, const float *V_sqrtS, int32_t probes, uint64_t seed, double *err_out,
                             double *frob2_out, double *uside_out);

/* ------------------------------------------------ Laplacian Eigenmaps ("next")
 * Replaces gem/embedding/lap.py:21-37: eigs(nx.normalized_laplacian_matrix(graph.to_undirected()), k=d+1, which='SM').
 * Input: CSR of the SYMMETRIC weighted adjacency in graph.nodes order (w NULL = unit).  The k smallest eigenpairs of
 * L_sym = I - D^-1/2 A D^-1/2 are computed as the k largest of I + D^-1/2 A D^-1/2 with the HOPE block-Krylov solver
 * (one SpMM per operator application).  V_out [n][k]: unit eigenvectors, eigvals[k] ascending (column 0 is the
 * trivial eigenvector lap.py drops with v[:, 1:]).  stats: as gemhip_hope.  From 16384 nodes up (GEMHIP_HOPE_SYM=0/1 forces it
 * off/on) the Chebyshev-filtered eigen-path of gemhip_hope is used (stats katz_terms = -1), with the block-Krylov solver as
 * the fallback when it does not converge. */
int gemhip_lap_eigmap(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w,
                      int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol,
                      uint64_t seed, float *V_out, float *eigvals, double *stats);

/* Locally Linear Embedding.  Replaces gem/embedding/lle.py:23-35: svds(I - D^-1 A, k=d+1, which='SM').
 * Input as gemhip_lap_eigmap (symmetric adjacency; rows are l1-normalised here).  sing[k]: the k smallest singular
 * values of I - P ascending; V_out [n][k]: matching right singular vectors (column 0 ~ the constant vector lle.py drops).
 * Same size switch as gemhip_lap_eigmap: the eigen-path filters N^T N, N = I - P, towards its smallest eigenvalues
 * (stats katz_terms = -2). */
int gemhip_lle(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t k,
               int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed,
               float *V_out, float *sing, double *stats);

/* HOPE building blocks, exposed so each kernel can be parity-tested on its own (host buffers in,
 * host buffers out, blocking).  Dense blocks are row-major with leading dimension = column count.
 *   sym_eig : host fp64 symmetric eigensolver used for the projected problems (A overwritten by
 *             eigenvectors in columns, w ascending) -- pure host code, callable without a GPU;
 *   spmm    : Y[n][b] = alpha * A X (+ Wadd)        gram : G[m1][m2] = X^T Y  (fp64 out, MFMA fp32)
 *   tsgemm  : Out[n][b2] = (Src or 0) + alpha * X[n][m] C[m][b2]   (C given in fp64, MFMA fp32).
 * These three pass compact blocks, the plain epilogue and distinct buffers only; the gemhip_test_hope_* hooks below reach the
 * same host functions with the solvers' leading dimensions, column offsets, three-term epilogue and aliased blocks, and the
 * blocks that have no export here (Ritz rotation, column arg-max, device projection, the LLE operator, lincomb, randn). */
int gemhip_sym_eig(int32_t n, double *A_inout, double *w_out);
int gemhip_sym_eig_builtin(int32_t n, double *A_inout, double *w_out);
/* The m largest eigenpairs only (what the Rayleigh-Ritz step consumes): Householder reduction, QL eigenvalues, inverse
 * iteration, back-transformation of m vectors.  A destroyed; w_out: m eigenvalues DESCENDING; Z_out: m eigenvectors,
 * one after the other (n doubles each).  Host code, callable without a GPU. */
int gemhip_sym_eig_top(int32_t n, double *A_inout, int32_t m, double *w_out, double *Z_out);
/* Host threads of the built-in eigensolver's O(n^3) phases (Householder reduction from n = 192 on, back-transformation of the
 * wanted vectors).  threads >= 1 (at most 16) sets the count, <= 0 restores the default: GEMHIP_EIG_THREADS, else
 * min(4, half the cores this process may run on).  in_effect_out (may be NULL) receives the count in effect.  Results of the
 * reduction agree between thread counts to rounding (sums are taken in a different order), not bit for bit.  There is no
 * reference counterpart: hope.py:32 hands the whole SVD to ARPACK/LAPACK, which thread through their BLAS. */
int gemhip_set_host_threads(int32_t threads, int32_t *in_effect_out);
/* Optional: let the host supply a faster symmetric eigensolver for the projected problems (same contract as
 * gemhip_sym_eig: row-major symmetric A overwritten by eigenvectors in columns, w ascending, return 0).  The Python
 * layer registers numpy's LAPACK (dsyevd) here; NULL restores the built-in Householder/QL solver. */
int gemhip_set_sym_eig_callback(int (*fn)(int32_t n, double *A_inout, double *w_out));
int gemhip_hope_spmm(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w,
                     float alpha, int32_t b, const float *X_host, const float *Wadd_host, float *Y_host);
int gemhip_hope_gram(int64_t n, int32_t m1, int32_t m2, const float *X_host, const float *Y_host,
                     double *G_host);
int gemhip_hope_tsgemm(int64_t n, int32_t m, int32_t b2, const float *X_host, const double *C_host,
                       float alpha, const float *Src_host, float *Out_host);

/* -------------------------------------------------- test hooks (HOPE building blocks under the solvers' calling conventions)
 * Like gemhip_test_wave_sum6: not part of the product API.  Each hook uploads its host blocks, calls the host function the
 * solvers call (spmm, gram, gram2, tsgemm, ritz_rotate, colmax, project_out, apply_sym_op, lincomb, randn in
 * gem_amd/csrc/hope_ops.hip; the hooks themselves: hope_hooks.hip) on a state of its own, and copies the result back; blocking.  Unlike the three exports above,
 * every dense block has its own leading dimension (ld >= logical columns; an "off" argument is a column offset into the
 * block, as in `Vall + nl`), and blocks named *_inout are uploaded WHOLE before the call and downloaded WHOLE after it:
 * a caller that fills the padding columns with a sentinel sees every write outside the logical columns.
 *   spmm       : Y[:, :b] = alpha A X + wa W + wb W2.  variant 0 = production dispatch, 1 = one row per wavefront
 *                (hope_spmm_kernel), 2 / 4 / 8 = hope_spmm16_kernel with that many gathers in flight (b <= 128; widths whose
 *                instantiation list lacks that U get the nearest smaller one, as GEMHIP_HOPE_SPMM16_U does).  w_is_x: W is
 *                the very device block of X (the (I + M) X and X - P X calls); w2_is_y: W2 is the very device block of Y,
 *                holding Y_inout's contents (apply_sym_op kind 2).  launched_out (may be NULL) receives the instantiation the
 *                dispatch chose: {CPL16, U} of hope_spmm16_kernel or {CPL, 0} of hope_spmm_kernel.  Without an override the environment variables
 *                GEMHIP_HOPE_SPMM16 / GEMHIP_HOPE_SPMM16_U / GEMHIP_HOPE_COLMAX2 decide, as in the solvers (read at every hook call).
 *   gram       : G[m1][m2] = X[:, xoff:+m1]^T Y[:, yoff:+m2] (fp64); Y_host NULL = Y is X's device block; Gf_host (optional):
 *                the same values rounded to fp32 on the device (what project_out feeds its GEMM).
 *   gram2      : two such products in one call (shared scratch, one round trip).
 *   tsgemm     : Out[:, :b2] = (Src or 0) + alpha X[:, xoff:+m] C; in_place: Src is Out's device block (Out_inout's contents).
 *   ritz       : Out[:, :b2] = V[:, voff:+m] C;  res2[j] = || B[:, boff:+m] C[:, j] - theta[j] Out[:, j] ||^2  (C: m x b2, fp64).
 *   colmax     : val[j] = the entry of column j < mc with the largest magnitude, the first row on ties.  variant 0 = production
 *                choice, 1 = one pass (hope_colmax_kernel), 2 = two passes (hope_colmax1/2_kernel).
 *   project_out: W[:, :cols] -= V[:, :m] (V[:, :m]^T W[:, :cols]) without a host round trip.  woff < 0: W is a block of its own;
 *                woff >= 0: W = columns [woff, woff + cols) of V's block (ldw = ldv), and W_inout receives that whole block.
 *   sym_op     : Out[:, :cols] = alpha Op X + wa W + wb W2; kind 0: Op = A (CSR); kind 2: Op = (I - A)^T (I - A), A^T built
 *                as gemhip_lle builds it (rows are NOT normalised here).  W_host / W2_host may be NULL.
 *   lincomb    : Out[:, :b] = a X + b2 Y + c Z; out_is_x: X is Out's device block (X_host NULL, Out_inout holds X).
 *   randn      : X[:, :b] = the solvers' Gaussian starting block for `seed`. */
int gemhip_test_hope_spmm(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t variant,
                          float alpha, int32_t b, const float *X_host, int32_t ldx, float wa, const float *W_host, int32_t ldw,
                          float wb, const float *W2_host, int32_t ldw2, int32_t w_is_x, int32_t w2_is_y, float *Y_inout,
                          int32_t ldy, int32_t *launched_out);
int gemhip_test_hope_gram(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m1, const float *Y_host,
                          int32_t ldy, int32_t yoff, int32_t m2, double *G_host, float *Gf_host);
int gemhip_test_hope_gram2(int64_t n, const float *Xa_host, int32_t ldxa, int32_t xaoff, int32_t ma1, const float *Ya_host,
                           int32_t ldya, int32_t yaoff, int32_t ma2, double *Ga_host, const float *Xb_host, int32_t ldxb,
                           int32_t xboff, int32_t mb1, const float *Yb_host, int32_t ldyb, int32_t yboff, int32_t mb2,
                           double *Gb_host);
int gemhip_test_hope_tsgemm(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m, const double *C_host,
                            int32_t b2, float alpha, const float *Src_host, int32_t lds, int32_t in_place, float *Out_inout,
                            int32_t ldo);
int gemhip_test_hope_ritz(int64_t n, const float *V_host, int32_t ldv, int32_t voff, const float *B_host, int32_t ldb,
                          int32_t boff, int32_t m, const double *C_host, const double *theta_host, int32_t b2,
                          float *Out_inout, int32_t ldo, double *res2_out);
int gemhip_test_hope_colmax(int64_t n, const float *X_host, int32_t ld, int32_t mc, int32_t variant, float *val_out);
int gemhip_test_hope_project_out(int64_t n, const float *V_host, int32_t ldv, int32_t m, float *W_inout, int32_t ldw,
                                 int32_t cols, int32_t woff);
int gemhip_test_hope_sym_op(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t kind,
                            float alpha, const float *X_host, int32_t ldx, int32_t cols, float wa, const float *W_host,
                            int32_t ldw, float wb, const float *W2_host, int32_t ldw2, float *Out_inout, int32_t ldo);
int gemhip_test_hope_lincomb(int64_t n, int32_t b, float a, const float *X_host, int32_t ldx, float b2, const float *Y_host,
                             int32_t ldy, float c, const float *Z_host, int32_t ldz, int32_t out_is_x, float *Out_inout,
                             int32_t ldo);
int gemhip_test_hope_randn(int64_t n, int32_t b, int32_t ld, uint64_t seed, float *X_inout);

/* One layer up: what the solvers and the set-ups compose of those launch functions (hope_ops.hip apply_S / apply_ST, hope_solve.hip
 * cheb_filter / orth / orth_scaled, hope.hip katz_rho_estimate / lle_shift_estimate).  Same conventions: the CSR matrix is used as given
 * (with its transpose built as the entry points build it), *_inout blocks travel whole, scratch blocks are the hook's own.
 *   apply_s          : Out[:, :b] = S X (transpose 0, apply_S) or S^T X (transpose 1, apply_ST).  mode 0: S = sum_{t=1..terms+1} (beta A)^t;
 *                      mode 1: S = I + A; mode 2: S = beta I - (I - A)^T (I - A) (`terms` unused in modes 1 and 2).  T0, T1, W0: n x ldt.
 *   cheb_filter      : V[:, :cols] <- T_m((Op - c I) / e) V[:, :cols], Op of `kind` as in sym_op (0 or 2); with nl > 0 the columns Q[:, :nl] are
 *                      projected out of the two live terms of the recurrence every q degrees.  The recurrence blocks are n x ldf.
 *   orth             : scaled 0: orth(Y, b, tol, abs_floor, passes); scaled 1: orth_scaled(Y, b, passes) (tol, abs_floor unused), in place through an
 *                      n x ldt scratch.  keep_out: the columns kept, [0, keep) of Y; the columns behind them keep what they held.
 *   spectrum_estimate: which 0: the rho hope_setup derives beta x sigma_max and the Katz term count from (power iteration on A^T A, x 1.1, capped by
 *                      the absolute row / column sums); which 1: the shift c gemhip_lle uses (power iteration on (I - P)^T (I - P), x 1.05), with the
 *                      rows l1-normalised here as gemhip_lle normalises them. */
int gemhip_test_hope_apply_s(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t mode, float beta,
                             int32_t transpose, int32_t terms, int32_t b, const float *X_host, int32_t ldx, int32_t ldt, float *Out_inout,
                             int32_t ldo);
int gemhip_test_hope_cheb_filter(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t kind, int32_t m,
                                 double c, double e, float *V_inout, int32_t ldv, int32_t cols, int32_t ldf, const float *Q_host, int32_t ldq,
                                 int32_t nl, int32_t q);
int gemhip_test_hope_orth(int64_t n, float *Y_inout, int32_t ld, int32_t b, int32_t ldt, int32_t scaled, double tol, double abs_floor,
                          int32_t passes, int32_t *keep_out);
int gemhip_test_hope_spectrum_estimate(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t which,
                                       double *estimate_out);

/* -------------------------------------------------- evaluation
 * Average precision of graph reconstruction for SAMPLED nodes, with the exact semantics of
 * gem/evaluation/metrics.py:27-46 (computeMAP) over the candidate list of
 * gem/utils/evaluation_util.py:28-35 (j > i when undirected, weight > 0), where the weight is
 * score(i, j) = A_i . B_j  (A = B = X for GF / node2vec, gf.py:103-104; A = X[:, :k], B = X[:, k:] for
 * HOPE, hope.py:43-44) -- without the n x n matrix of static_graph_embedding.py:48-65.
 * A_host, B_host: [n][ld] float32 (B_host NULL = A); row_ptr/col: CSR of the TRUE graph; ap_out[nsample].
 * MAP over the sample = mean(ap_out).  Any degree: a hub's true neighbours are processed in chunks of 512
 * (one workgroup per chunk); duplicate columns in the CSR count once. */
int gemhip_eval_sampled_ap(int64_t n, int32_t da, int32_t ld, const float *A_host, const float *B_host,
                           const int64_t *row_ptr, const int32_t *col, int32_t undirected,
                           int64_t nsample, const int32_t *nodes, double *ap_out);

/* Evaluator handle: the embedding and the CSR of the TRUE graph are uploaded once and serve the three calls below, so that the
 * reference's whole return tuple (MAP, precision curve, err, err_baseline of evaluate_graph_reconstruction.py:8-46) is available
 * at sizes where the n x n matrix cannot be formed.
 * kind 0: score(i, j) = A_i . B_j, as above (B_host NULL = A).
 * kind 1: score(i, j) = exp(-(sqrt(sum_k (a_ik - a_jk)^2))^2) in fp64, B_host NULL: the scalar get_edge_weight of Laplacian Eigenmaps
 *         and LLE (lap.py:74, lle.py:53) -- differences of the fp32 inputs are exact in fp64; sqrt, then square, then exp.  Ranks
 *         and ties are decided on the exp output; where it saturates the tie classes are those of the device's fp64 exp, which may
 *         differ from the host libm's by one ulp.
 * A_host, B_host: [n][ld] float32, 1 <= da <= 512.  row_ptr/col are copied; gemhip_eval_pairs' edge lookup needs every row's
 * columns in ascending order (duplicates allowed), gemhip_eval_ap does not. */
typedef struct gemhip_eval *gemhip_eval_t;
int gemhip_eval_create(int64_t n, int32_t da, int32_t ld, const float *A_host, const float *B_host, int32_t kind,
                       const int64_t *row_ptr, const int32_t *col, gemhip_eval_t *out);
/* gemhip_eval_sampled_ap's result for `nodes`, with the handle's score kind. */
int gemhip_eval_ap(gemhip_eval_t h, int32_t undirected, int64_t nsample, const int32_t *nodes, double *ap_out);
/* For every pair p: score_out[p] = (st == ed) ? 0 : score(st, ed)   (the zero diagonal of get_reconstructed_adj,
 * static_graph_embedding.py:48-65), hit_out[p] = 1 if the CSR holds the arc st -> ed (true_digraph.has_edge; directed), else 0.
 * hit_out may be NULL.  npairs = 0 is legal.  fp64 accumulation in a fixed order, no atomics: identical bits on every run. */
int gemhip_eval_pairs(gemhip_eval_t h, int64_t npairs, const int32_t *st, const int32_t *ed, double *score_out,
                      uint8_t *hit_out);
/* Device time of the last gemhip_eval_pairs kernel of this handle, milliseconds (HIP events). */
int gemhip_eval_last_pairs_ms(gemhip_eval_t h, double *ms_out);

/* Link prediction: the handle's CSR is the TEST graph and a second CSR, the TRAIN graph, is a MASK with directed has_edge semantics.
 * The candidates of node i are the j with j != i, j > i when `undirected`, score(i, j) > 0 (evaluation_util.py:28-35) and (i -> j)
 * not in the mask, ordered by score descending and node id ascending on ties (Python's stable sorted(..., reverse=True) of metrics.py:12
 * on the ascending-j list).  The positives of i are its test neighbours that are candidates: a test arc that is also a mask arc is
 * neither a hit nor a positive.
 *
 * gemhip_eval_set_mask copies the mask after validating it on the host as gemhip_eval_create validates its CSR (GEMHIP_E_INVALID, nothing
 * reaches a kernel); rows are sorted and de-duplicated on the host, the caller need not sort.  mask_row_ptr NULL clears the mask. */
int gemhip_eval_set_mask(gemhip_eval_t h, const int64_t *mask_row_ptr, const int32_t *mask_col);
/* ap_out[s] = mean over the positives t of nodes[s] of rank_hit(t) / rank_all(t), both ranks inside the candidate list; 0 without a
 * positive.  npos_out (may be NULL): the number of positives ranked.  Without a mask, or with an empty one, the bytes of gemhip_eval_ap. */
int gemhip_eval_ap_masked(gemhip_eval_t h, int32_t undirected, int64_t nsample, const int32_t *nodes, double *ap_out,
                          int64_t *npos_out);
/* The first k candidates of every node, [nsample][k]: node id, score, and whether (i -> id) is a test arc; id -1, score 0, hit 0 where a
 * node has fewer than k candidates.  1 <= k <= 1024.  use_mask 0 ignores the handle's mask.  Exact under the tie rule, identical bytes on
 * every call, no nsample x n matrix.  Needs the test CSR's columns in ascending order (as gemhip_eval_pairs' edge lookup). */
int gemhip_eval_topk(gemhip_eval_t h, int32_t undirected, int32_t use_mask, int64_t nsample, const int32_t *nodes, int32_t k,
                     int32_t *id_out, double *score_out, uint8_t *hit_out);
/* Device time of the last gemhip_eval_ap, gemhip_eval_ap_masked or gemhip_eval_topk kernel of this handle, milliseconds (HIP events). */
int gemhip_eval_last_kernel_ms(gemhip_eval_t h, double *ms_out);
int gemhip_eval_destroy(gemhip_eval_t h);

/* ------------------------------------------- connected components, largest component
 * Replaces: gem/utils/graph_util.py:29-34 (get_lcc: the largest weakly connected component of a graph, its nodes renumbered 0..k-1), which
 * upstream's link-prediction driver applies to the train graph of a split.  (That function calls nx.weakly_connected_component_subgraphs, which current networkx no longer has.)
 *
 * The graph is the arc list of the GF entry points: m arcs (src, dst[, w]) in any order.  Direction is ignored (WEAK connectivity); self-loops
 * and duplicate arcs are legal; m = 0 is legal (every node its own component).  1 <= n < 2^31 and m < 2^31, otherwise GEMHIP_E_UNSUPPORTED
 * (n < 1: GEMHIP_E_INVALID).  Validated on the host before any device call, like gemhip_gf_objective: a NULL pointer, or an arc outside [0, n)
 * (named as gemhip_gf_train names it: "lcc: edge 1 = (1,5) outside [0,5)"), is GEMHIP_E_INVALID.
 *
 * Device: lock-free union-find, one thread per arc, then one kernel per phase (DESIGN.md "Connected components"); no thread waits for another.
 * Every result is exact and identical on every run.
 *
 * labels_out[v] = the smallest node id of v's component; *n_components_out = the number of components. */
int gemhip_cc_labels(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, int32_t *labels_out, int32_t *n_components_out);
/* The largest component; of several largest ones, the one with the smallest label (= holding the smallest node id).
 * *n_out nodes and *m_out arcs are kept.  new_of_old[n]: the new id of every node, ascending with the old id, -1 where the node is dropped;
 * old_of_new[0 .. *n_out): its inverse.  src_out / dst_out / w_out [0 .. *m_out): the arcs whose source is kept (their target then is too), in
 * their original order, both ends renumbered, weights copied bit for bit.  old_of_new needs room for n entries, src_out / dst_out / w_out for m;
 * entries past *n_out / *m_out are not written.  w and w_out are both given or both NULL; src_out / dst_out may be NULL when m = 0. */
int gemhip_lcc(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w /* or NULL */, int64_t *n_out, int64_t *m_out,
               int32_t *old_of_new, int32_t *new_of_old, int32_t *src_out, int32_t *dst_out, float *w_out /* or NULL */,
               int32_t *n_components_out);
/* Device time of the kernels of the last gemhip_cc_labels / gemhip_lcc call on this thread, milliseconds (HIP events): out[8] = {init, union,
 * flatten (labels), component sizes, winner, node compaction, arc compaction, 0}; the last two are 0 after gemhip_cc_labels. */
int gemhip_cc_last_kernel_ms(double *out);

/* ------------------------------------------- t-SNE to two dimensions (embedding plots)
 * Replaces: gem/evaluation/visualize_embedding.py:9-12, where an embedding with d > 2 goes through sklearn.manifold.TSNE(n_components=2)
 * before it is plotted.  The scheme: k nearest neighbours with k = min(n - 1, floor(3 * perplexity) + 1), sklearn's binary
 * search of the conditional affinities p_{j|i} over them, P = (p_{j|i} + p_{i|j}) / 2n held as the kNN lists and their transpose (never merged,
 * never n x n), the repulsive term summed EXACTLY over all pairs (no tree), sklearn's gradient descent with gains and momentum.
 * No floating-point atomics, every reduction in a fixed order: identical bits on every run.
 *
 * gemhip_tsne_create: X_host [n][ld] float32, 1 <= d <= ld.  5 <= perplexity <= 100 and perplexity < n, every value finite and at most 1e15 in
 * magnitude, n * k < 2^31: otherwise GEMHIP_E_INVALID (GEMHIP_E_UNSUPPORTED for the last), checked on the host before any device call.
 * Runs the kNN search, the affinities and the transpose.  The embedding Y is [n][2] float32 and must be set before the first run. */
typedef struct gemhip_tsne *gemhip_tsne_t;
int gemhip_tsne_create(int64_t n, int32_t d, int32_t ld, const float *X_host, double perplexity, gemhip_tsne_t *out);
/* Sets Y and resets the optimiser's state (update = 0, gains = 1). */
int gemhip_tsne_set_embedding(gemhip_tsne_t h, const float *Y_host);
/* n_iter steps of sklearn's _gradient_descent at fixed arguments: grad = 4 (exaggeration * attr - rep / Z); gains += 0.2 where update * grad < 0,
 * otherwise *= 0.8, at least 0.01; update = momentum * update - lr * gains * grad; Y += update.  The optimiser's state carries over from call to
 * call.  *kl_out (may be NULL): KL(P || Q) of the UNEXAGGERATED P at the Y the last step's gradient was taken at; *grad_norm_out (may be NULL):
 * the 2-norm of that step's gains * grad, the quantity sklearn's min_grad_norm rule looks at.  n_iter >= 1. */
int gemhip_tsne_run(gemhip_tsne_t h, int32_t n_iter, double exaggeration, double momentum, double lr, double *kl_out, double *grad_norm_out);
int gemhip_tsne_get_embedding(gemhip_tsne_t h, float *Y_out);
/* Device time, milliseconds (HIP events): out[4] = {kNN search, affinities, transpose, the last gemhip_tsne_run}. */
int gemhip_tsne_last_ms(gemhip_tsne_t h, double *out);
/* out[4] = {n, d, k, number of j-slices of the repulsion grid}. */
int gemhip_tsne_info(gemhip_tsne_t h, int64_t *out);
int gemhip_tsne_destroy(gemhip_tsne_t h);
/* Stages on their own (tests).
 * gemhip_tsne_knn: for every row the k nearest OTHER rows, 1 <= k <= min(n - 1, 301): id_out / dist_out [n][k], ascending by (distance, id),
 * distance = sum_c (x_ic - x_jc)^2 in fp32.  Candidates are chosen by ||a||^2 + ||b||^2 - 2 a.b of the mean-centred rows (fp32 matrix units).
 * gemhip_tsne_affinities: dist [n][k] float32 -> p_out [n][k] float32, sklearn's _binary_search_perplexity (fp64, at most 100 steps, 1e-5 on the
 * entropy), 1 <= k <= 320.
 * gemhip_tsne_set_affinities: replaces the handle's kNN lists and conditional P by the caller's, [n][k] each with the handle's k; ids are
 * checked against [0, n) and the row itself on the host.
 * gemhip_tsne_gradient: the gradient at the handle's Y, [n][2] float32, the KL of the unexaggerated P and Z = sum_{i != j} 1 / (1 + |y_i - y_j|^2). */
int gemhip_tsne_knn(int64_t n, int32_t d, int32_t ld, const float *X_host, int32_t k, int32_t *id_out, float *dist_out);
int gemhip_tsne_affinities(int64_t n, int32_t k, const float *dist, double perplexity, float *p_out);
int gemhip_tsne_set_affinities(gemhip_tsne_t h, const int32_t *id, const float *p);
int gemhip_tsne_gradient(gemhip_tsne_t h, double exaggeration, float *grad_out, double *kl_out, double *z_out);

/* ------------------------------------------- node classification (one-vs-rest L2 logistic regression, top-k ranker)
 * Replaces: GEM's fourth evaluation task, sklearn's OneVsRestClassifier(LogisticRegression()) on embedding rows with the "top-k ranker" of the
 * embedding literature.  The scheme: for every class c independently the minimiser over theta = (w, b) of
 *     F_c = C * sum_{i in T} log(1 + exp(-y_ic (x_i . w + b))) + |w|^2 / 2,   y_ic = +-1,   the intercept unpenalised
 * (sklearn LogisticRegression(penalty='l2', C, fit_intercept=True), any solver but liblinear), by damped Newton: one device pass over the
 * training rows gives loss, gradient and Hessian of a block of classes, the host solves the (d+1) x (d+1) systems by fp64 Cholesky (Levenberg
 * shift when a pivot is not positive) and runs an Armijo line search (c1 = 1e-4, halving) on device loss evaluations.  A class is converged
 * after the step whose decrement lambda^2 = -g . delta is at most dec_tol * max(1, F_c).  No floating-point atomics: identical bits on every run.
 *
 * gemhip_nc_create: X_host [n][ld] float32, uploaded once; 1 <= d <= ld, n >= 1, every X[i][c < d] finite (GEMHIP_E_INVALID, the first
 * offender named); d <= 255 and n < 2^31 (GEMHIP_E_UNSUPPORTED).  Everything is checked on the host before any device call.
 * gemhip_nc_set_labels: the multi-label indicator as a CSR of class ids per node, row_ptr [n + 1], cls [row_ptr[n]]; 1 <= K <= 65536 and
 * row_ptr[n] < 2^31 (GEMHIP_E_UNSUPPORTED beyond).  row_ptr[0] == 0, no negative row, ids in [0, K), no class twice in a row: GEMHIP_E_INVALID,
 * the first offender named by position.  Rows need not be sorted.  Forgets the handle's weights.
 * gemhip_nc_fit: train_idx [n_train] rows in [0, n), any order, a repeated row counts twice.  C > 0 and dec_tol > 0 finite, max_iter >= 1.
 * W_inout [K][d + 1] fp64, w then b: the start on input (finite), the result on output; the handle keeps it for prediction.  A class with no
 * positive among the training rows, or no negative, has no finite minimiser: w = 0, b = -inf / +inf, no iteration.  info_out (may be NULL)
 * [K][6] = {iterations, backtracks, |g|_inf and lambda^2 at the last iterate a pass evaluated, converged (1 / 0; 1 for a degenerate class),
 * degenerate (-1 no positive, +1 no negative, 0)}.  A class that does not converge in max_iter iterations is returned as it is, flagged.
 * gemhip_nc_set_weights: W [K][d + 1] for prediction without a fit; w finite, b not NaN (+-inf is a constant predictor).
 * gemhip_nc_scores: out [m][K] fp64 logits x_i . w_c + b_c of the rows idx [m].
 * gemhip_nc_predict_topk: for row t the k_t classes of largest logit, ties to the lower class id; k_t = the row's number of labels when
 * k_or_null is NULL, otherwise 0 <= k[t] <= K (GEMHIP_E_INVALID naming t).  pred_or_null [m][K] 0 / 1.  counts_out [3][K] = TP, FP, FN per
 * class over the rows (integer atomics: exact), *exact_out = rows whose predicted set equals the true set. */
typedef struct gemhip_nc *gemhip_nc_t;
int gemhip_nc_create(int64_t n, int32_t d, int32_t ld, const float *X_host, gemhip_nc_t *out);
int gemhip_nc_set_labels(gemhip_nc_t h, int32_t K, const int64_t *row_ptr, const int32_t *cls);
int gemhip_nc_fit(gemhip_nc_t h, int64_t n_train, const int32_t *train_idx, double C, double dec_tol, int32_t max_iter, double *W_inout,
                  double *info_out /* or NULL */);
int gemhip_nc_set_weights(gemhip_nc_t h, const double *W);
int gemhip_nc_scores(gemhip_nc_t h, int64_t m, const int32_t *idx, double *out);
int gemhip_nc_predict_topk(gemhip_nc_t h, int64_t m, const int32_t *idx, const int32_t *k_or_null, uint8_t *pred_or_null, int64_t *counts_out,
                           int64_t *exact_out);
/* Milliseconds: out[4] = {upload (host wall), the last fit (host wall), mean Newton pass of that fit (host wall, kernels + copy back),
 * the last predict (HIP events)}. */
int gemhip_nc_last_ms(gemhip_nc_t h, double *out);
/* out[8] = {n, d, K, Newton passes, loss evaluations and iterations of the last fit, classes per block, rows per LDS slab}. */
int gemhip_nc_info(gemhip_nc_t h, int64_t *out);
int gemhip_nc_destroy(gemhip_nc_t h);
/* Stages on their own (tests).
 * gemhip_nc_pass: one kernel pass as the solver makes it, for all K classes at W [K][d + 1] (finite): F_out [K], g_out [K][d + 1],
 * H_out [K][d + 1][d + 1] -- the objective above, its gradient and its full symmetric Hessian, regulariser included.
 * gemhip_nc_newton_step_host: host only, works without a device.  Solves (H + shift I) delta = -g by fp64 Cholesky on the upper triangle of
 * H [d1][d1]; shift = 0 unless a pivot is not positive, then 1e-10 * max(1, max |H_jj|) times 10 per retry.  *dec_out = -g . delta;
 * *shift_out (may be NULL) = the shift used.  GEMHIP_E_NOTCONVERGED if no shift helps or an input is not finite. */
int gemhip_nc_pass(gemhip_nc_t h, int64_t n_train, const int32_t *train_idx, double C, const double *W, double *F_out, double *g_out, double *H_out);
int gemhip_nc_newton_step_host(int32_t d1, const double *H, const double *g, double *delta_out, double *dec_out, double *shift_out /* or NULL */);

/* ------------------------------------------- k-means and community-recovery scores (Lloyd, k-means++, NMI / ARI / purity)
 * Replaces: sklearn.cluster.KMeans(algorithm='lloyd') on embedding rows and sklearn.metrics' normalized_mutual_info_score /
 * adjusted_rand_score against planted communities.  The scheme: the semantics are sklearn 1.7.2's on the float32 matrix,
 * restated exactly where sklearn leaves an order open.  Assign: the fp32 score |c_k|^2 - 2 x_i . c_k on the matrix units, a running minimum per
 * row, ties to the lower cluster id.  Update: integer counts, fp64 sums in a fixed order, centre = float32(sum / count).  Empty clusters:
 * the j-th empty cluster in ascending id takes the row of j-th largest fp64 squared distance to the OLD centre of its label (ties: the lower
 * row id); the row leaves its donor's sum and count; that iteration's labels stay.  Stop: labels equal to the previous iteration's (strict),
 * else sum |c_new - c_old|^2 <= tol * mean(var(X, axis=0)), else max_iter; after a non-strict stop one more assign, so that the labels belong to
 * the returned centres.  Inertia: sum_i |x_i - c_label(i)|^2, the difference form, fp64.  No floating-point atomics: identical bytes on
 * every run.
 *
 * Refused on the host before any device call, the first offender named by position -- GEMHIP_E_INVALID: n < 1, d < 1, ld < d, a non-finite
 * X[i][c < d], K < 1, K > n, a non-finite centre, max_iter < 1, tol < 0 or not finite, n_trials < 1, a u outside [0, 1), a label outside
 * [0, K), a true label outside [0, Kt), gemhip_kmeans_contingency before any labels exist; GEMHIP_E_UNSUPPORTED: n >= 2^31, d > 256, K > 16384,
 * n_trials > 16, a contingency table of more than 2^26 entries.  gemhip_kmeans_fit returns GEMHIP_E_UNSUPPORTED (nothing divided by zero) when a
 * relocation would leave the donor cluster without a row.
 *
 * gemhip_kmeans_create: X_host [n][ld] float32, uploaded once, zero-padded to a multiple of 8 columns.
 * gemhip_kmeans_seed_pp: sklearn's greedy k-means++ on host-supplied uniforms u [K][n_trials] in [0, 1).  Centre 0 is row
 * min(floor(u[0][0] n), n - 1).  Centre c > 0: candidate t is searchsorted(cumsum_fp64(D2), u[c][t] * total, side='right') clipped to n - 1, D2
 * the running minimum of the fp32 difference-form squared distances to the chosen rows, the cumulative sum in row order; the candidate of
 * smallest fp64 potential sum_i min(D2_i, |x_i - x_cand|^2) wins, ties to the lower t.  chosen_idx_out [K], centres_out [K][d].
 * gemhip_kmeans_fit: centres_inout [K][d] float32, the start on input, the result on output; labels_out [n]; info_out (may be NULL) [6] =
 * {inertia, iterations, strict (1 / 0), rows relocated, the last sum |c_new - c_old|^2, tol * mean(var(X, axis=0))}.
 * gemhip_kmeans_assign: one assign step; labels_out [n], score_out_or_null [n] the fp32 score of the chosen centre.
 * gemhip_kmeans_update: one update step of labels [n] without relocation: centres_out [K][d] (zeros for an empty cluster), counts_out [K].
 * gemhip_kmeans_contingency: table_out [K][Kt] int64 (integer atomics: exact) of the labels the last fit, assign or update left on the device
 * against labels_true [n] in [0, Kt).
 * gemhip_clustering_scores_host: host only, works without a device.  out [4] = {NMI with the arithmetic mean of the entropies (1 when both
 * partitions are a single cluster, as sklearn), ARI in sklearn's pair-count form (128-bit integers: n^2 at n = 2^31 fits), purity,
 * homogeneity}, all fp64 from table [Kp][Kt]; empty rows and columns are legal, a negative entry or an empty table is GEMHIP_E_INVALID. */
typedef struct gemhip_kmeans *gemhip_kmeans_t;
int gemhip_kmeans_create(int64_t n, int32_t d, int32_t ld, const float *X_host, gemhip_kmeans_t *out);
int gemhip_kmeans_seed_pp(gemhip_kmeans_t h, int32_t K, int32_t n_trials, const double *u, int32_t *chosen_idx_out, float *centres_out);
int gemhip_kmeans_fit(gemhip_kmeans_t h, int32_t K, float *centres_inout, double tol, int32_t max_iter, int32_t *labels_out, double *info_out /* or NULL */);
int gemhip_kmeans_assign(gemhip_kmeans_t h, int32_t K, const float *centres, int32_t *labels_out, float *score_out_or_null);
int gemhip_kmeans_update(gemhip_kmeans_t h, int32_t K, const int32_t *labels, float *centres_out, int64_t *counts_out);
int gemhip_kmeans_contingency(gemhip_kmeans_t h, int32_t Kt, const int32_t *labels_true, int64_t *table_out);
int gemhip_clustering_scores_host(const int64_t *table, int32_t Kp, int32_t Kt, double *out);
/* Milliseconds: out[6] = {upload (host wall), the last seeding (host wall), the last fit's iterations (HIP events), that over its iteration
 * count, the last gemhip_kmeans_assign's kernel (HIP events), the last gemhip_kmeans_update (HIP events, its copies included)}. */
int gemhip_kmeans_last_ms(gemhip_kmeans_t h, double *out);
/* out[12] = {n, d, d padded to 8, K of the labels on the device (0: none), rows per assign workgroup (128), centres per tile (32), the caps on
 * d (256), K (16384) and n_trials (16), members per sum slice (512), rows per counting-sort slab, iterations of the last fit}. */
int gemhip_kmeans_info(gemhip_kmeans_t h, int64_t *out);
int gemhip_kmeans_destroy(gemhip_kmeans_t h);

/* ------------------------------------------- binary ranking metrics: a device sort, ROC-AUC, average precision, the curve points
 * Replaces: sklearn.metrics roc_auc_score / average_precision_score / roc_curve / precision_recall_curve on host arrays of fp64 scores and
 * 0 / 1 labels.  The scheme: a stable LSD radix sort of order-preserving 64-bit keys, descending, -0.0 tied with +0.0,
 * +-inf ordinary keys, the int32 position as payload; eight 8-bit passes, a pass whose digit histogram has one non-empty bucket skipped.  Tie
 * groups end where two neighbouring keys differ; an integer scan of the labels gives the cumulative tp, fp at each group end.
 *     U2  = sum_g pos_g (2 (N - fp_g) + neg_g)           twice the Mann-Whitney U, an exact int64
 *     auc = U2 / (2 P N)                                  one fp64 division, correctly rounded while both integers are below 2^53
 *     ap  = (1 / P) sum_g pos_g tp_g / (tp_g + fp_g)      sklearn's step-wise average precision, fp64 terms summed in a fixed order
 * No floating-point atomics; integer atomics only in histograms; identical bytes on every run.
 *
 * Refused on the host before any device call -- GEMHIP_E_INVALID: m < 1, a NaN score (named by position), a label that is neither 0 nor 1
 * (named by position), only one class present (the message says which is missing); GEMHIP_E_UNSUPPORTED: m >= 2^31.
 *
 * gemhip_rank_argsort: perm_out [m], the stable descending permutation: what numpy.argsort(-score, kind='stable') returns.
 * gemhip_rank_binary: out [4] = {auc, ap, prevalence P / m, kernel milliseconds (HIP events around the launches; allocations and copies excluded)};
 * counts [4] = {P, N, the number T of distinct scores, U2}.
 * gemhip_rank_curve: thr_out / tp_out / fp_out [T], the threshold and the cumulative counts at each distinct score, descending; *T_out = T
 * is always written once the inputs pass; cap < T is GEMHIP_E_INVALID and nothing else is written.
 * gemhip_rank_binary_from_groups_host: host only, works without a device.  The same out and counts (out[3] = 0) from the group table tp / fp [T];
 * a table that is not cumulative (a group without a member, a decreasing count, a total of 2^31 or more) is GEMHIP_E_INVALID naming the group.
 * gemhip_rank_info: out [8] = {keys per sort workgroup W, threads per workgroup, bits per pass, passes run and passes skipped by the last
 * sort on this thread, its workgroups, T of the last group table, m}. */
int gemhip_rank_argsort(int64_t m, const double *score, int32_t *perm_out);
int gemhip_rank_binary(int64_t m, const double *score, const uint8_t *label, double *out, int64_t *counts);
int gemhip_rank_curve(int64_t m, const double *score, const uint8_t *label, int64_t cap, double *thr_out, int64_t *tp_out, int64_t *fp_out, int64_t *T_out);
int gemhip_rank_binary_from_groups_host(int64_t T, const int64_t *tp, const int64_t *fp, double *out, int64_t *counts);
int gemhip_rank_info(int64_t *out);

/* ------------------------------------------- link prediction as classification: pair features and the pair classifier
 * Replaces: the protocol of node2vec section 4.4 on the host -- a binary operator on the two embedding rows of a node pair, sklearn's
 * LogisticRegression on the pair features, ROC-AUC on held-out pairs.  Operators (op), on rows a = X[st], b = X[ed], in fp32 without FMA
 * contraction, bit-equal to the same numpy float32 expressions:
 *     0 average (a + b) * 0.5f     1 Hadamard a * b     2 L1 fabsf(a - b)     3 L2 t = a - b rounded, then t * t
 *
 * gemhip_edgeclf_create: X_host [n][ld] float32, uploaded once; 1 <= d <= ld, n >= 1, every X[i][c < d] finite and at most 1e18 in magnitude
 * (GEMHIP_E_INVALID, the first offender named: every operator's result is then finite); d <= 255 and n < 2^31 (GEMHIP_E_UNSUPPORTED).
 * Pairs: st / ed [m] node ids in [0, n) (GEMHIP_E_INVALID naming the first pair outside), 1 <= m < 2^31; st == ed and repeated pairs are legal.
 * Everything is checked on the host before any device call.
 * gemhip_edgeclf_features: F_out [m][d] float32.
 * gemhip_edgeclf_scores: score_out [m] fp64 = sum_j (double)F[p][j] * w[j] + w[d], gather, operator and reduction fused, no feature matrix
 * formed, a fixed summation order.  w [d + 1] finite (the intercept not NaN); w == NULL: the plain inner product sum_j (double)a_j (double)b_j
 * (op is then ignored).
 * gemhip_edgeclf_fit: label [m] in {0, 1}; builds the feature matrix on the device and fits the one-class problem "is an edge" with the
 * node-classification solver (gemhip_nc_fit: C, dec_tol, max_iter as there).  w_inout [d + 1], weights then intercept: the start on input
 * (finite), the minimiser on output.  info_out (may be NULL) [8] = gemhip_nc_fit's six per-class fields {iterations, backtracks, |g|_inf,
 * lambda^2, converged, degenerate}, then the Newton passes and the loss evaluations.  A fit that does not converge in max_iter iterations
 * returns its iterate, flagged; labels of one class only give the degenerate answer of gemhip_nc_fit.  Device memory at the peak:
 * 2 * m * d * 4 bytes (the feature matrix and the solver's copy; the former is freed before the first pass). */
typedef struct gemhip_edgeclf *gemhip_edgeclf_t;
int gemhip_edgeclf_create(int64_t n, int32_t d, int32_t ld, const float *X_host, gemhip_edgeclf_t *out);
int gemhip_edgeclf_features(gemhip_edgeclf_t h, int32_t op, int64_t m, const int32_t *st, const int32_t *ed, float *F_out);
int gemhip_edgeclf_scores(gemhip_edgeclf_t h, int32_t op, int64_t m, const int32_t *st, const int32_t *ed, const double *w /* or NULL */, double *score_out);
int gemhip_edgeclf_fit(gemhip_edgeclf_t h, int32_t op, int64_t m, const int32_t *st, const int32_t *ed, const uint8_t *label, double C, double dec_tol,
                       int32_t max_iter, double *w_inout, double *info_out /* or NULL */);
/* Milliseconds: out[6] = {upload (host wall), the last features kernel, the last scores kernel (HIP events), the last fit (host wall), that
 * fit's mean Newton pass (host wall), its feature kernel (HIP events)}. */
int gemhip_edgeclf_last_ms(gemhip_edgeclf_t h, double *out);
/* out[8] = {n, d, pairs a wave has in flight, pairs per workgroup, Newton passes, loss evaluations and iterations of the last fit, m of the
 * last call}. */
int gemhip_edgeclf_info(gemhip_edgeclf_t h, int64_t *out);
int gemhip_edgeclf_destroy(gemhip_edgeclf_t h);

/* ------------------------------------------- link prediction baselines: neighbourhood scores of node pairs
 * Replaces: networkx's common_neighbors, jaccard_coefficient, adamic_adar_index, resource_allocation_index and preferential_attachment, a
 * Python loop per pair -- the first rows of node2vec's table 4.  All five are defined on the SIMPLE UNDIRECTED graph of the arc list: both
 * orientations merged, self-loops dropped, repeated arcs merged, weights ignored.  G(u) the neighbour set, deg u = |G(u)|, I = G(u) & G(v):
 *     cn |I| (int32)     jaccard |I| / (deg u + deg v - |I|), 0 for an empty union     aa sum_{w in I} 1 / ln(deg w)
 *     ra sum_{w in I} 1 / deg w     pa deg u * deg v                                    (mask bits 1, 2, 4, 8, 16)
 * cn is exact; jaccard is one correctly rounded fp64 division and pa one fp64 product, bit-equal to numpy's; aa and ra are fp64 sums of the
 * entries of two tables the library makes on the host (1.0 / std::log((double)deg) and 1.0 / deg; 0 where deg < 2 and deg < 1), without
 * atomics and in an order that is a function of the two lists alone: the same bytes on every run and for both orientations of a pair.
 * Scheme: per pair the shorter list a is searched in the longer list b, element by element, by binary search (on equal lengths a is the
 * list of the smaller id).  A pair with an empty a has no work item (all five scores are zero); a of at most CHUNK elements is one item, a
 * longer one is cut into slices of CHUNK whose partial sums a second kernel adds in slice order.  Items of at most NARROW elements go to
 * groups of 16 lanes, four per wavefront; the others to one wavefront each.
 *
 * gemhip_nbr_create: src / dst [m] (m >= 0), ingested on the host into a CSR (row_ptr int64, col int32 ascending per row) and uploaded once.
 * n >= 1, every endpoint in [0, n) (GEMHIP_E_INVALID naming the first arc outside); n < 2^31 (GEMHIP_E_UNSUPPORTED).
 * gemhip_nbr_degrees: deg_out [n].  gemhip_nbr_weights: w_out [n], which = 0 the aa table, 1 the ra table, read back from the device.
 * gemhip_nbr_scores: st / ed [m], 1 <= m < 2^31 (GEMHIP_E_UNSUPPORTED above), ids in [0, n) and st != ed (GEMHIP_E_INVALID naming the first
 * offending pair; networkx raises for st == ed at a degree-1 neighbour); repeated and adjacent pairs are legal.  Outputs [m] each, NULL where
 * the score is not in mask.  Everything is checked on the host before any device call.
 * gemhip_nbr_last_ms: out [6] = {ingest (host wall), graph upload (host wall), plan of the last call (host wall), its pair and item upload
 * (host wall), its kernels (HIP events), its download (host wall)}.
 * gemhip_nbr_info: out [12] = {n, stored neighbours, largest degree, lanes per narrow group, NARROW, CHUNK, then of the last call: narrow
 * items, wide items, split pairs, partial slots, elements of the longest item, m}.  h == NULL: the constants only.
 * Host only, working without a device: gemhip_nbr_graph_host (row_ptr_out [n + 1], col_out with room for 2 m entries, deg_out [n]: the ingest
 * above), gemhip_nbr_weights_host (the two tables from given degrees) and gemhip_nbr_plan_host (counts_out [6] = {narrow items, wide items,
 * split pairs, partial slots, elements of the longest item, pairs without an item}; deg [n] with entries in [0, n), pairs checked as above). */
typedef struct gemhip_nbr *gemhip_nbr_t;
int gemhip_nbr_create(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, gemhip_nbr_t *out);
int gemhip_nbr_degrees(gemhip_nbr_t h, int32_t *deg_out);
int gemhip_nbr_weights(gemhip_nbr_t h, int32_t which, double *w_out);
int gemhip_nbr_scores(gemhip_nbr_t h, int64_t m, const int32_t *st, const int32_t *ed, int32_t mask, int32_t *cn_out, double *jaccard_out,
                      double *aa_out, double *ra_out, double *pa_out);
int gemhip_nbr_last_ms(gemhip_nbr_t h, double *out);
int gemhip_nbr_info(gemhip_nbr_t h, int64_t *out);
int gemhip_nbr_destroy(gemhip_nbr_t h);
int gemhip_nbr_graph_host(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, int64_t *row_ptr_out, int32_t *col_out, int32_t *deg_out);
int gemhip_nbr_weights_host(int64_t n, const int32_t *deg, int32_t which, double *w_out);
int gemhip_nbr_plan_host(int64_t n, const int32_t *deg, int64_t m, const int32_t *st, const int32_t *ed, int64_t *counts_out);

#ifdef __cplusplus
}
#endif
#endif /* GEM_HIP_H */
