/*
 * tfrs_hip.h -- C ABI of libtfrs_hip.so, the MI355X (gfx950) implementation of the
 * tensorflow/recommenders retrieval hot path.
 *
 * The reference's boundary for this path is a Python class API (Keras layers), not
 * an FFI; each entry point below names the reference method whose arithmetic it
 * replaces (paths relative to tensorflow_recommenders/).  The Python host classes in
 * recommenders_amd/ bind these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _h;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls only
 *     enqueue work, they never synchronise the device or allocate in launch paths:
 *     the caller supplies outputs and a workspace sized by the matching
 *     *_workspace_bytes() query (index handles own their packed corpus);
 *   - return value: 0 = OK, <0 = error (TFRS_E*); the message is available through
 *     tfrs_last_error() (thread-local);
 *   - float32 arithmetic throughout; candidate indices are int32 row numbers
 *     (the reference's default identifiers are an int32 range/counter,
 *     layers/factorized_top_k.py:380-382,544-545); identifier lookup stays on the host side;
 *   - functions are re-entrant on distinct streams/workspaces; an index handle is
 *     read-only while queries run.
 *
 * Numerics contract: a score is ONE float32 fma chain over d = 0..D-1 in increasing d
 * starting from +0 (what v_mfma_f32_32x32x2_f32 computes); top-K order is score
 * descending, ties to the lower row index (tf.math.top_k); results are therefore
 * reproducible bit for bit and comparable with == against oracle/.
 */
#ifndef TFRS_HIP_H_
#define TFRS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFRS_OK 0
#define TFRS_EINVAL (-1)   /* bad argument (shape, k, alignment, NULL) */
#define TFRS_ENOTIMPL (-2) /* valid request outside the implemented envelope */
#define TFRS_EHIP (-3)     /* a HIP runtime call failed */
#define TFRS_ENOMEM (-4)   /* workspace too small / allocation failed */
#define TFRS_ESTATE (-5)   /* handle not indexed yet */

#define TFRS_MAX_DIM 128 /* embedding dims above this are TFRS_ENOTIMPL for top-K */
#define TFRS_MAX_K 1024

int tfrs_version(void);
const char *tfrs_last_error(void);
/* Fills compute-unit count, LDS bytes per CU and the gcnArchName of device `dev`. */
int tfrs_device_info(int dev, int *cu_count_h, int *lds_bytes_h, char *arch_h,
                     int arch_len);
/* The library's configuration plane: every measurement / test switch (the TFRS_* names listed in
 * INTEGRATION.md "Runtime switches") is read through one accessor -- a value set here wins, else
 * the process environment is consulted at the time of the call.  value == NULL removes the
 * override.  tfrs_get_option returns 1 and the value in force, 0 when the option is unset.
 * Process-wide (like the environment); defaults are what bench.py and the tests run. */
int tfrs_set_option(const char *name, const char *value);
int tfrs_get_option(const char *name, char *value_h, int value_len);


/* Measurement hook (bench.py): while enabled, every launch of the fused score+filter scan
 * kernel is bracketed by HIP events on its launch stream.  tfrs_profile_read returns the
 * summed kernel time, the number of launches and their algorithmic flop (2*nq*rows*d) since
 * the last read, after waiting for the recorded events. */
int tfrs_profile_enable(int on);
int tfrs_profile_read(double *scan_ms_h, int *launches_h, double *flop_h);
/* Same sums restricted to one scan kernel (0 = exact f32 scan, 1 = fp16 filter pass over all
 * rows, 2 = fp16 threshold pass over the sampled stages); does not reset -- call before
 * tfrs_profile_read. */
int tfrs_profile_read_kind(int kind, double *scan_ms_h, int *launches_h, double *flop_h);

/* Per-box ceilings measured in the caller's process (bench.py `roofline.measured_ceiling`; no reference
 * counterpart -- measurement plumbing).  Boxes of one pool differ by several per cent in what any kernel
 * gets (the shader clock follows the power the operand data draws), so a fraction of the spec peak is only
 * comparable between runs next to the box's own ceiling.  Both calls time with HIP events on `stream` and WAIT.
 *   tfrs_calibrate_mfma_f16: saturating v_mfma_f32_32x32x16_f16 loop on uniform random fp16 operands in
 *     registers, two waves per SIMD on every CU, `iters` x 64 MFMAs per wave; returns TFLOP/s and the shader
 *     clock (MHz) the loop ran at.  `ws`: tfrs_calibrate_workspace_bytes() bytes.
 *   tfrs_calibrate_copy: float4 grid-stride copy of ws_bytes / 2 bytes from the first half of `ws` to the
 *     second (>= 64 MiB, 16-byte aligned), `iters` times; returns (bytes read + bytes written) / time in GB/s. */
size_t tfrs_calibrate_workspace_bytes(void);
int tfrs_calibrate_mfma_f16(void *ws, size_t ws_bytes, int iters, double *tflops_h, double *shader_mhz_h,
                            void *stream);
int tfrs_calibrate_copy(void *ws, size_t ws_bytes, int iters, double *gbs_h, void *stream);

/* ------------------------------------------------------------------------- *
 * Candidate index (BruteForce.index, layers/factorized_top_k.py:540-584).
 * The handle owns a device copy of the candidates in an MFMA/LDS-friendly packed
 * layout (even/odd feature planes per row, rows of 4 * padded_dim bytes with NO pad
 * slot in memory -- a dim-64 row is two whole 128-byte lines; the scan kernels
 * re-pitch rows to an odd number of 16-byte slots when they stage them in LDS, so
 * that ds_read_b128 of 16 consecutive rows is bank-conflict free).  Re-indexing
 * drops and recreates the copy, as the reference does (:163-164).
 * ------------------------------------------------------------------------- */
typedef struct tfrs_index tfrs_index_t;

int tfrs_index_create(tfrs_index_t **out_h);
int tfrs_index_destroy(tfrs_index_t *index);
/* Copies+packs candidates[n, d] (row-major f32).  May (re)allocate device memory. */
int tfrs_index_set(tfrs_index_t *index, const float *candidates, int64_t n, int d,
                   void *stream);
/* Incremental ingestion for TopK.index_from_dataset (:179-215): reserve once, then
 * append blocks in dataset order. */
int tfrs_index_reserve(tfrs_index_t *index, int64_t capacity, int d, void *stream);
int tfrs_index_append(tfrs_index_t *index, const float *block, int64_t nb, void *stream);
/* Non-finite inputs (the reference's tf.math.top_k, layers/factorized_top_k.py:605, tolerates NaN / Inf scores; this
 * library's fp16-prefiltered search does NOT: its error bound is built from row norms, and the filter kernels are
 * compiled without NaN semantics).  CONTRACT, per candidate row c and per query row q (not per element):
 *   - every element is finite;
 *   - the 2-norm is at most 2^120 (1.3e36) -- the norm bounds of the filter then stay finite for every dim up to 128 --
 *     and every product ||q|| * ||c|| is at most 2^126, so that every score is finite;
 *   - a row that is not all zero has max |x| >= 2^-120 (7.5e-37): below that the row's power-of-two scale is clamped
 *     and its fp16 image loses more than the bound accounts for.  (Zero rows are fine.)
 * Inside these limits the top-K is exact whatever the magnitudes: norms are computed as upper bounds over the whole
 * range (common.h, norm_upper_bound), never as a sum of squares that under- or overflows.  NaN / Inf are recorded,
 * never silent:
 *   bit 0 (1)  an indexed candidate row holds NaN / Inf -- set by tfrs_index_set / _append; the host layer raises
 *              ValueError from BruteForce.index / index_from_dataset and drops the index;
 *   bit 1 (2)  a query row of a tfrs_bruteforce_topk[_below] call held NaN / Inf.  Only THAT row of the result is
 *              affected (its scores are non-finite, its indices valid but unspecified); every other row of the call is
 *              the exact top-K as always.  The host layer raises ValueError at the next call (or at once under
 *              BruteForce(check_finite=True), which synchronises).
 * The word lives in pinned host memory the kernels OR into: reading it never touches the stream, and reflects
 * every launch that has completed.  reset_mask: bits to clear after the read. */
int tfrs_index_nonfinite(const tfrs_index_t *index, int reset_mask, int32_t *flags_h);
/* ORs `bits` into the handle's flag word when any element of x[0, count) or y[0, county) (either may be NULL / empty) is
 * NaN / Inf: ONE launch, no synchronisation.  For the searches that have no indexed corpus -- Streaming over blocks read
 * in place (layers/factorized_top_k.py:404-509) records its queries and its carried state through an otherwise empty
 * handle; the flag word is allocated on first use. */
int tfrs_index_note_nonfinite(tfrs_index_t *index, const float *x, int64_t count, const float *y, int64_t county,
                              int bits, void *stream);
int64_t tfrs_index_size(const tfrs_index_t *index);
int tfrs_index_dim(const tfrs_index_t *index);
/* Writes the original row-major candidates[n, d] back (checkpoint/state_dict). */
int tfrs_index_unpack(const tfrs_index_t *index, float *candidates_out, void *stream);

/* ------------------------------------------------------------------------- *
 * BruteForce.call (layers/factorized_top_k.py:586-607; scores :320-333):
 *   scores = q @ candidates^T ; values, indices = tf.math.top_k(scores, k)
 * out_scores[nq, k] f32, out_idx[nq, k] i32 (row numbers; identifiers[idx] is a
 * host-side gather, :607).  Requires k <= index size (TopKV2 raises otherwise).
 * The [nq, n] score matrix is never materialised.
 * ------------------------------------------------------------------------- */
size_t tfrs_bruteforce_topk_workspace_bytes(int64_t nq, int64_t n, int d, int k);
int tfrs_bruteforce_topk(const tfrs_index_t *index, const float *queries, int64_t nq,
                         int k, float *out_scores, int32_t *out_idx, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Measurement hook (bench.py, tests): after a tfrs_bruteforce_topk call with the same
 * (workspace, nq, n, k) has completed on `stream`, returns how many of its queries took the
 * exact-recompute ("redo") path of the fp16-prefiltered search (survivor list overflow or
 * retained set too large; 0 on well-behaved data, and always 0 on the all-f32 path).
 * Synchronises `stream`. */
/* De-duplicated index (BruteForce.call on corpora with many EXACT copies of a row; tf.math.top_k
 * breaks ties by the lower index, layers/factorized_top_k.py:605, so every copy of a top-K row is a
 * candidate and no threshold separates them).  The host indexes the distinct rows:
 *   tfrs_row_hash64: out[r] = 63-bit hash of row r's bit pattern (equal rows hash equal; the caller
 *     compares hash neighbours exactly);
 *   tfrs_topk_expand_duplicates: scores / distinct_rows[nq, k_in] = the best distinct rows of each
 *     query (descending; row < 0 = empty); distinct row u stands for the original rows
 *     dup_rows[dup_start[u] .. dup_start[u + 1]) (ascending).  Writes the exact top-k_out of the
 *     ORIGINAL corpus, order (score descending, original row ascending); empty slots carry row -1. */
int tfrs_row_hash64(const float *rows, int64_t n, int d, uint64_t *out, void *stream);
int tfrs_topk_expand_duplicates(const float *scores, const int32_t *distinct_rows, int64_t nq, int k_in,
                                const int64_t *dup_start, const int32_t *dup_rows, int k_out,
                                float *out_scores, int32_t *out_rows, void *stream);

/* Paged search for k beyond TFRS_MAX_K (tf.math.top_k has no limit, layers/factorized_top_k.py:605):
 * the best k <= TFRS_MAX_K rows among those strictly AFTER (last_scores[q * last_ld],
 * last_rows[q * last_ld]) in the result order (score descending, row ascending); NULL / NULL = the
 * first page.  Concatenated pages are exactly the sorted top-(sum of k); the caller keeps
 * sum of k <= rows.  All-f32 rounds.  Workspace: tfrs_bruteforce_topk_below_workspace_bytes. */
size_t tfrs_bruteforce_topk_below_workspace_bytes(int64_t nq, int64_t n, int d, int k);
int tfrs_bruteforce_topk_below(const tfrs_index_t *index, const float *queries, int64_t nq, int k,
                               const float *last_scores, const int32_t *last_rows, int64_t last_ld,
                               float *out_scores, int32_t *out_idx, void *workspace,
                               size_t workspace_bytes, void *stream);
int tfrs_bruteforce_topk_redo_count(const void *workspace, int64_t nq, int64_t n, int k,
                                    int32_t *redo_count_h, void *stream);
/* Same contract; reasons_h[4] = queries flagged because {0: a survivor segment or the list
 * overflowed, 1: the statistically chosen bound of a shuffled index did not hold,
 * 2: NOT redone -- queries whose retained set (rows within 2 eps of the K-th prefilter score: near-
 * duplicate clusters) exceeded K + band and was re-scored in full inside the list kernel};
 * reasons_h[3] = length of the longest survivor list of the call
 * when one exceeded 768 entries, else 0 (the list kernel holds 1024 entries per query). */
int tfrs_bruteforce_topk_redo_reasons(const void *workspace, int64_t nq, int64_t n, int k,
                                      int32_t *reasons_h, void *stream);

/* Test hook (host code only, no GPU needed): the threshold-pass plan the fp16-prefiltered search
 * would use for a corpus of n rows and top-k -- plan_h[5] = {sampling stride, sampled stages,
 * stages per bin, rank of the bin maximum the bound is taken from, 1 when that rank is a
 * statistical one (rank < k: the list kernel verifies the bound), else 0}.  shuffled != 0 asks
 * for the plan of a shuffled index (>= 65536 rows), 0 for the guaranteed plan.  sampled
 * stages == 0: the corpus is too small for the prefilter (all-f32 rounds are used). */
int tfrs_debug_topk_plan(int64_t n, int k, int shuffled, int64_t *plan_h);

/* Test hook: raw scores of the fp16 PREFILTER (never returned by the product path) for rows
 * [row_begin, row_end) of the index, row_begin a multiple of 128: out[nq, ld] with
 * ld = (row_end - row_begin) rounded up to 128; scratch: 2 * nq floats.  tests/ check
 * |s_16 - s_f32| against the bound ||q|| ||c|| * 0.0011 that the filter relies on. */
int tfrs_debug_fp16_scores(const tfrs_index_t *index, const float *queries, int64_t nq,
                           int64_t row_begin, int64_t row_end, float *out, float *scratch,
                           void *stream);
/* After the call, scratch[0, nq) holds qk[q] (the query's norm bound times kappa) and scratch[nq, 2 nq) its
 * power-of-two scale: the query-side inputs of the filter's bound.
 *
 * Test hook: the candidate-side inputs of the bound, for stages [stage_begin, stage_end) of the index (a stage is 128
 * image rows; stage_end <= ceil(rows / 128)).  Plain device-to-device copies on `stream`:
 *   image_out     the stages' fp16 image rows in image order, 2 * padded_dim16 + 16 bytes each (padded_dim16 = 16, 32,
 *                 64 or 128: x / scale in natural feature order, zero columns up to padded_dim16, one zero 16-byte slot);
 *   meta_out      4 floats per stage: {norm, scale, 1 / scale, 0};
 *   norm_max_out  one float, the largest norm of any stage of the index.
 * An index of fewer than 65536 rows is not shuffled: image row = candidate row. */
int tfrs_debug_fp16_image(const tfrs_index_t *index, int64_t stage_begin, int64_t stage_end, void *image_out,
                          void *meta_out, float *norm_max_out, void *stream);

/* ------------------------------------------------------------------------- *
 * Streaming.call (layers/factorized_top_k.py:404-509): one candidate block.
 * Replaces top_scores (:424-438) + the reduce step top_k (:440-472) for the block
 * cand_block[nb, d], whose rows carry the global row numbers base_row..base_row+nb-1
 * (enumerate_rows :474-480).  The running state is state_scores/state_idx[nq, k]
 * with state_len valid, sorted entries per row; it is updated in place and the new
 * length min(k, state_len + nb) is returned through *new_len_h
 * (handle_incomplete_batches=True semantics, :431-434,:465-468).
 * ------------------------------------------------------------------------- */
size_t tfrs_streaming_topk_workspace_bytes(int64_t nq, int64_t nb, int d, int k);
int tfrs_streaming_topk_update(const float *queries, int64_t nq, int d,
                               const float *cand_block, int64_t nb, int64_t base_row,
                               int k, float *state_scores, int32_t *state_idx,
                               int32_t state_len, int32_t *new_len_h, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 * Streaming.call over a GROUP of consecutive candidate blocks read in place
 * (layers/factorized_top_k.py:404-509; the layer keeps only a reference to its dataset and
 * re-reads it on every call, :384-390,:496-507).  blocks_h[nblocks] are DEVICE pointers to
 * row-major float32 [block_rows_h[b], d] blocks (the arrays themselves live on the host), whose
 * rows carry the global row numbers base_row, base_row + 1, ... in block order (:474-480);
 * seen_rows = candidates already folded into the state by earlier calls.  One call replaces
 * nblocks calls of tfrs_streaming_topk_update with identical results: no packed copy of the
 * blocks is built -- query batches up to 256 take ONE pass over the f32 blocks per
 * range: an fp16 filter fed by the blocks themselves, each wave converting its 32 rows of a stage in
 * registers, with exact re-scoring of the survivors from the blocks; up to 32 queries below d = 128 an
 * HBM-bound exact f32-MFMA scan; large batches one fp16 prefilter image of the group with exact
 * re-scoring from the blocks (csrc/topk_raw.hip).  Requirements: d in {8, 16, 32, 64, 128}, 16-byte aligned
 * block pointers, nblocks <= 192 (TFRS_EINVAL otherwise: use the per-block entry point); the blocks
 * must stay valid until the work enqueued on `stream` has run.  Workspace from
 * tfrs_streaming_topk_blocks_workspace_bytes(nq, total rows of the group, d, k).
 * ------------------------------------------------------------------------- */
size_t tfrs_streaming_topk_blocks_workspace_bytes(int64_t nq, int64_t total_rows, int d, int k);
int tfrs_streaming_topk_update_blocks(const float *queries, int64_t nq, int d,
                                      const float *const *blocks_h, const int64_t *block_rows_h,
                                      int nblocks, int64_t base_row, int64_t seen_rows, int k,
                                      float *state_scores, int32_t *state_idx, int32_t state_len,
                                      int32_t *new_len_h, void *workspace, size_t workspace_bytes,
                                      void *stream);

/* ------------------------------------------------------------------------- *
 * Embedding dims above TFRS_MAX_DIM (the fused scan kernels keep a row in registers): the same
 * result through materialised score blocks.
 *   tfrs_compute_scores: scores[nq, nc] = q @ c^T (TopK._compute_score,
 *     layers/factorized_top_k.py:320-333; also Retrieval.call scores tasks/retrieval.py:172-180),
 *     the candidate matrix read in place as the transposed operand; f16 != 0 selects the
 *     split-fp16 MFMA GEMM (workspace from tfrs_gemm_f16_workspace_bytes(nq, nc, d)).
 *   tfrs_topk_update_from_scores: folds a score block (columns = rows base_row.. of the corpus)
 *     into the running top-K state exactly like tfrs_streaming_topk_update (:440-472).
 * Scores of this path are GEMM sums (f32 accuracy, not the bit-defined fma chain).
 * ------------------------------------------------------------------------- */
int tfrs_compute_scores(const float *queries, const float *candidates, int64_t nq, int nc, int d,
                        float *out, int f16, void *workspace, size_t workspace_bytes,
                        void *stream);
int tfrs_topk_update_from_scores(const float *scores, int64_t nq, int64_t nb, int64_t ld,
                                 int64_t base_row, int k, float *state_scores,
                                 int32_t *state_idx, int32_t state_len, int32_t *new_len_h,
                                 void *stream);

/* ------------------------------------------------------------------------- *
 * Merge of partial top-K lists (the multi-GPU exchange step and the general form of
 * the Streaming reduce, :459-472): parts are scores[nparts, nq, k_in] /
 * idx[nparts, nq, k_in] (each sorted or not), result out[nq, k_out] under
 * (score desc, idx asc).  k_out <= nparts * k_in.
 *
 * Conventions shared by every list this selection layer reads or writes (tfrs_topk_merge*,
 * tfrs_topk_update_from_scores, tfrs_topk_expand_duplicates; pinned by
 * tests/test_select_layout_gpu.py): an entry whose idx is < 0 does not exist, whatever its score;
 * -0.0 ties with +0.0 and comes back as +0.0; all k slots of a result are written, the ones
 * past the last entry as (0.0f, -1).  A carried-in state holds its entries in its first
 * state_len slots, sorted, without holes between them (trailing idx -1 slots are fine); slots
 * at or past state_len are not read.
 * ------------------------------------------------------------------------- */
size_t tfrs_topk_merge_workspace_bytes(int64_t nq, int nparts, int k_in, int k_out);
int tfrs_topk_merge(const float *scores_parts, const int32_t *idx_parts, int nparts,
                    int64_t nq, int k_in, int k_out, float *out_scores,
                    int32_t *out_idx, void *workspace, size_t workspace_bytes,
                    void *stream);

/* Same with parts that are part_stride elements apart (>= nq * k_in): lets the multi-GPU
 * exchange gather ONE buffer [world, 2, nq, k] (scores and rows of a rank back to back)
 * with a single all-gather and merge it in place. */
int tfrs_topk_merge_strided(const float *scores_parts, const int32_t *idx_parts, int nparts,
                            int64_t part_stride, int64_t nq, int k_in, int k_out,
                            float *out_scores, int32_t *out_idx, void *stream);

/* ------------------------------------------------------------------------- *
 * _exclude (layers/factorized_top_k.py:83-115) on int32 identifiers:
 *   isin = any(ids[:, :, None] == exclude[:, None, :]); adjusted = scores - 1e5*isin;
 *   top_k(adjusted, min(k, kin)); gather ORIGINAL scores and ids.
 * scores/ids[nq, kin], exclude[nq, ne] -> out_scores/out_ids[nq, kout=min(k,kin)].
 * ------------------------------------------------------------------------- */
int tfrs_topk_exclude(const float *scores, const int32_t *ids, int64_t nq, int kin,
                      const int32_t *exclude, int ne, int k, float *out_scores,
                      int32_t *out_ids, void *stream);

/* ------------------------------------------------------------------------- *
 * FactorizedTopK.update_state, score-based branch
 * (metrics/factorized_top_k.py:133-134,181-192):
 *   pos = sum_d q*c (same fma chain as the scores);
 *   hit[b, j] = in_top_k(target 0, concat([pos, topk]), ks[j])
 *             = (#{topk[b, :] > pos[b]} < ks[j]) && isfinite(pos[b]).
 * out_hits[nks, nq] f32 (0/1).  ks_h is a HOST array.
 * ------------------------------------------------------------------------- */
int tfrs_rank_of_positive(const float *queries, const float *true_candidates,
                          int64_t nq, int d, const float *topk_scores, int kmax,
                          const int32_t *ks_h, int nks, float *out_hits, void *stream);
/* id-based branch (:141-180): hit = any(ids[b, :ks[j]] == true_id[b]). */
int tfrs_id_match_topk(const int32_t *retrieved_ids, const int32_t *true_ids,
                       int64_t nq, int kmax, const int32_t *ks_h, int nks,
                       float *out_hits, void *stream);

/* The same score-based branch WITHOUT the top-K (metrics/factorized_top_k.py:133-137,181-192):
 * the retrieved list holds the max(ks) best scores of the corpus and in_top_k counts strictly
 * greater predictions, so for every k <= max(ks)
 *     hit_k[b] = (#{candidates j : score(q_b, cand_j) > pos_b} < k) && isfinite(pos_b),
 * i.e. the metric needs ONE count per query, not a sorted list.
 *   tfrs_rank_count_accumulate: counts[b] += #{j < nc : score(q_b, row_j) > pos_b} for one block of
 *     candidates, row_j = candidates[cand_ids[j]] (cand_ids int32 / int64; NULL: row_j =
 *     candidates[j]; ids outside [0, vocab) score as zero rows, like tfrs_embedding_gather_fwd) --
 *     with an id indirection the reference's `movies.batch(128).map(item_model)` candidate sweep of
 *     an Embedding tower (README.md:69-80) is one launch: gather, scores, rank.  f32 MFMA, the
 *     d-ordered fma chain of every scoring kernel (the positive ties with its own copy).  d <= 128.
 *     `counts` (uint32 [nq]) must be zero before the first block of a sweep (first_block = 1 also
 *     flags non-finite positives in bit 31); tfrs_topk_hits_update re-arms it.
 *   tfrs_topk_hits_update: state[i] += sum_b w_b hit_ks[i][b], state[nks + i] += sum_b w_b
 *     (tf.keras.metrics.Mean per k, :85-89,191-192; sample_weight NULL = ones),
 *     results[i] = state[i] / state[nks + i] (0 when empty), optional per-example hits[nks, nq];
 *     zeroes `counts`.  One workgroup, fixed reduction order.  ks_h is a HOST array (<= 16). */
int tfrs_rank_count_accumulate(const float *queries, const float *true_candidates, int64_t nq, int d,
                               const float *candidates, const void *cand_ids, int ids_i64, int64_t nc,
                               int64_t vocab, uint32_t *counts, int first_block, void *stream);
int tfrs_topk_hits_update(uint32_t *counts, int64_t nq, const int32_t *ks_h, int nks,
                          const float *sample_weight, float *state, float *results, float *hits,
                          void *stream);
/* The split geometry of tfrs_rank_count_accumulate at (nq, nc, d), from the function the launch
 * calls (host only, no device work): out = [n_qtiles (128-query tiles), tiles_per_split (32-row
 * candidate tiles per workgroup), nsplits, max_tiles (the LDS bound on tiles_per_split)].
 * TFRS_EINVAL for nq < 1, nc < 1, d outside [1, 128] or a NULL out. */
int tfrs_rank_count_plan(int64_t nq, int64_t nc, int d, int64_t *out);

/* ------------------------------------------------------------------------- *
 * Embedding lookup (tf.keras.layers.Embedding as called at README.md:62-66,77-78;
 * TPUEmbedding CPU branch layers/embedding/tpu_embedding_layer.py:913-919).
 * ids are int32 or int64 (ids_are_i64).  Out-of-range ids set *err_flag (device
 * int32, may be NULL) and produce a zero row.
 * ------------------------------------------------------------------------- */
int tfrs_embedding_gather_fwd(const float *table, int64_t vocab, int d, const void *ids,
                              int ids_are_i64, int64_t n, float *out, int32_t *err_flag,
                              void *stream);
/* combiner: 0 = sum, 1 = mean, 2 = sqrtn.  CSR segments row_splits[nrows + 1] (i32/i64
 * like ids); weights may be NULL.  out[nrows, d]. */
int tfrs_embedding_segment_reduce_fwd(const float *table, int64_t vocab, int d,
                                      const void *ids, const void *row_splits,
                                      int ids_are_i64, const float *weights,
                                      int64_t nrows, int combiner, float *out,
                                      int32_t *err_flag, void *stream);
/* Backward of the combiner lookup: grad_rows[p, :] = (grad_out[b, :] / den_b) * w_p for every
 * entry p of segment b (den_b = 1 | sum w | sqrt(sum w^2) as in the forward), i.e. the values
 * of the IndexedSlices gradient whose indices are the looked-up ids; feed (ids, grad_rows) to
 * tfrs_embedding_scatter_add_* (TPUEmbedding CPU branch, tpu_embedding_layer.py:913-919 under
 * tape.gradient, models/base.py:77).  grad_rows[nnz, d], nnz = row_splits[nrows]. */
int tfrs_embedding_segment_reduce_bwd(const float *grad_out, int d, const void *row_splits,
                                      int splits_are_i64, const float *weights, int64_t nrows,
                                      int combiner, float *grad_rows, void *stream);
/* Backward of gather: deterministic, atomics-free scatter-add.  `perm`/`sorted_ids`
 * are caller-provided sort results (ids sorted ascending, perm = source positions).
 * Produces the dense grad_table[vocab, d] rows for the touched ids only (other rows
 * untouched) -- or, when adagrad != 0, applies the fused row-wise Adagrad update
 * (models/base.py:77-78 with Adagrad, README.md:84):
 *   g = sum of duplicate grads; acc += g*g; row -= lr * g / sqrt(acc + eps)      (adagrad == 1:
 *   tf.keras.optimizers.Adagrad of TF >= 2.11 / tf-keras), or ... / (sqrt(acc) + eps)   (adagrad == 2: the optimizer_v2
 *   kernel ResourceApplyAdagradV2 of TF <= 2.10, also torch.optim.Adagrad's form).
 * Negative ids (the padding slots of a max_sequence_length feature) contribute nothing. */
int tfrs_embedding_scatter_add_bwd(const float *grad_out, const int64_t *sorted_ids,
                                   const int64_t *perm, int64_t n, int d,
                                   float *grad_table_or_table, float *accum, float lr,
                                   float eps, int adagrad, void *stream);
/* The same from UNSORTED ids (int32 / int64): the library sorts (id, position) pairs itself
 * (stable LSD radix sort, 8 bits per pass over the bits of vocab) and then runs the segmented
 * scatter-add / fused Adagrad.  ids outside [0, vocab) are ignored -- they can never write
 * outside the table.  workspace from tfrs_embedding_scatter_add_workspace_bytes(n). */
size_t tfrs_embedding_scatter_add_workspace_bytes(int64_t n);
/* The plan of that sort for a vocabulary (host only, no device call): *passes LSD passes of *digit_bits (8, 9 or 10)
 * bits each -- the smallest pass count that covers the bits of vocab plus the one bit that sets the invalid key apart,
 * at the narrowest digit that reaches it.  The sort launches exactly this plan. */
int tfrs_embedding_sort_plan(int64_t vocab, int *passes, int *digit_bits);
int tfrs_embedding_scatter_add_unsorted(const float *grad_out, const void *ids, int ids_are_i64,
                                        int64_t n, int d, int64_t vocab,
                                        float *grad_table_or_table, float *accum, float lr,
                                        float eps, int adagrad, void *workspace,
                                        size_t workspace_bytes, void *stream);

/* Same result without the sort, for small vocabularies: one wave per table row scans the id
 * list and sums matching gradient rows in occurrence order (O(vocab * n / 64) wave steps;
 * d <= 256).  In dense mode (adagrad == 0) EVERY row of grad_table[vocab, d] is written
 * (zeros for untouched rows). */
int tfrs_embedding_scatter_add_rowscan(const float *grad_out, const void *ids, int ids_are_i64,
                                       int64_t n, int d, int64_t vocab,
                                       float *grad_table_or_table, float *accum, float lr,
                                       float eps, int adagrad, void *stream);
/* The same for up to 8 small tables in ONE launch (the user and item tables of a two-tower step):
 * the *_h arguments are HOST arrays of `ntables` entries holding the per-table arguments of
 * tfrs_embedding_scatter_add_rowscan. */
int tfrs_embedding_scatter_add_rowscan_multi(int ntables, const float *const *grad_out_h,
                                             const void *const *ids_h, const int *ids_are_i64_h,
                                             const int64_t *n_h, const int *d_h,
                                             const int64_t *vocab_h, float *const *tables_h,
                                             float *const *accum_h, float lr, float eps,
                                             int adagrad, void *stream);
/* Dense Adagrad of up to 32 parameters in ONE launch (models/base.py:77-78 with tf.keras.optimizers.Adagrad on the dense
 * variables -- Cross kernels, MLP kernels and biases): acc += g * g; p -= lr * g / denom, denom = sqrt(acc + eps) (mode 1)
 * or sqrt(acc) + eps (mode 2), the same arithmetic as the fused sparse update above.  Host arrays of device pointers. */
int tfrs_adagrad_dense_multi(int ntensors, float *const *params_h, float *const *accum_h, const float *const *grads_h,
                             const int64_t *n_h, float lr, float eps, int mode, void *stream);
/* ClippyAdagrad (experimental/optimizers/clippy_adagrad.py:188-254 with shrink_by_references, :21-70) on up to 32 dense
 * tensors per call, f32:
 *   [mode 2: acc += g * g first]   pre = 1 / sqrt(acc + eps);   delta = lr * g * pre;
 *   maxd = |w| * var_rel + pre * acc_rel + abs_thr;   factor = min(1, min_i (delta_i == 0 ? 1 : maxd_i / |delta_i|));
 *   w -= delta * factor;   [mode 0: acc += g * g after;  mode 1 (clip_accumulator_update): acc += (g * factor)^2 after]
 * Host arrays of device pointers as in tfrs_adagrad_dense_multi; factors[ntensors] is a DEVICE array that receives each
 * tensor's factor (re-armed to 1 by the call itself; it never visits the host: no synchronisation, capturable).  A factor
 * pass (reads only, atomicMin on the float's bits) and an apply pass over the same elements. */
int tfrs_clippy_dense_multi(int ntensors, float *const *params_h, float *const *accum_h, const float *const *grads_h,
                            const int64_t *n_h, float *factors, float lr, float eps, float var_rel, float acc_rel,
                            float abs_thr, int mode, void *stream);
/* The same on the looked-up rows of table[vocab, d] from UNSORTED ids (int32 / int64) and grad_out[n, d]: duplicates
 * are summed first, strictly in occurrence order; ids outside [0, vocab) are ignored; the factor (*factor, device) is
 * the min over the touched rows only; untouched rows of table and accum are not written.  rowscan != 0: the sort-free
 * row scan (d <= 256, small vocab * n), else radix sort + segments with workspace from
 * tfrs_clippy_sparse_workspace_bytes(n, rowscan).  n == 0: factor 1, nothing written. */
size_t tfrs_clippy_sparse_workspace_bytes(int64_t n, int rowscan);
int tfrs_clippy_sparse(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d, int64_t vocab,
                       float *table, float *accum, float *factor, float lr, float eps, float var_rel, float acc_rel,
                       float abs_thr, int mode, int rowscan, void *workspace, size_t workspace_bytes, void *stream);
/* optimizers.SGD / Adam / Ftrl (tf.keras.optimizers.SGD, Adam and Ftrl; on tables: row-sparse, Adam lazily, as
 * tf.tpu.experimental.embedding.Adam(lazy_adam=True) and ResourceSparseApplyFtrlV2), f32 in the written order, no
 * contraction.  rule 0 = SGD, 1 = Adam, 2 = Ftrl; hyper_h is a HOST array of 8 floats:
 *   SGD   {lr}:                          w -= lr * g
 *   Adam  {1 - beta_1, 1 - beta_2, epsilon}, slots m, v; alpha is the DEVICE float that tfrs_adam_tick wrote:
 *         m += (g - m) * (1 - beta_1);  v += (g * g - v) * (1 - beta_2);  w -= m * alpha / (sqrt(v) + epsilon)
 *   Ftrl  {lr, l1, 2 * (l2 + beta / (2 lr)), 2 * l2_shrinkage, learning_rate_power}, slots n (accumulator), lin (linear);
 *         learning_rate_power is -0.5 (n^p = sqrt(n)) or 0 (n^p = 1):
 *         g' = g + 2 shrink w;  n' = n + g * g;  lin += g' - (n'^p - n^p) / lr * w;  q = n'^p / lr + 2 l2r;
 *         w = (clip(lin, -l1, l1) - lin) / q;  n = n'
 * _sparse: the looked-up rows of table[vocab, d] (and of slot0 / slot1 of the same shape; NULL for SGD) from UNSORTED
 * ids (int32 / int64) and grad_out[n, d]: duplicates are summed first, in occurrence order from +0 (on the sorted route a run
 * longer than a piece of max(32, pow2 >= d) positions is cut at fixed positions into occurrence-order pieces that are
 * then added in order, as the sparse Adagrad update does) -- the bits
 * of tfrs_embedding_scatter_add_unsorted's sums; ids outside [0, vocab) are ignored; a touched row whose sum is zero is
 * still updated; untouched rows are not written.  rowscan != 0: the sort-free row scan (d <= 256), else radix sort +
 * segments with workspace from tfrs_table_update_workspace_bytes(n, rowscan).  n == 0: nothing is written.
 * _dense_multi: up to 32 tensors in one launch, host arrays of device pointers as in tfrs_adagrad_dense_multi (the slot
 * arrays may be NULL for SGD).
 * tfrs_adam_tick: one thread; *step += advance (0 or 1; step is a device int64, Keras's iterations + 1 after the add),
 * *alpha = (float)(lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)) computed in float64 from the integer t.  On the device, so
 * that a captured step replays with a live counter.  Every argument check comes before any device call. */
size_t tfrs_table_update_workspace_bytes(int64_t n, int rowscan);
int tfrs_table_update_sparse(int rule, const float *hyper_h, const float *alpha, const float *grad_out, const void *ids,
                             int ids_are_i64, int64_t n, int d, int64_t vocab, float *table, float *slot0, float *slot1,
                             int rowscan, void *workspace, size_t workspace_bytes, void *stream);
int tfrs_table_update_dense_multi(int rule, const float *hyper_h, const float *alpha, int ntensors,
                                  float *const *params_h, float *const *slot0_h, float *const *slot1_h,
                                  const float *const *grads_h, const int64_t *n_h, void *stream);
int tfrs_adam_tick(int64_t *step, float *alpha, double learning_rate, double beta_1, double beta_2, int advance,
                   void *stream);
/* optimizers.RowWiseAdagrad: Adagrad with ONE accumulator scalar per row of a [vocab, d] table (accum: float32 [vocab]),
 * f32 in the written order, no contraction.  With G the row's summed gradient:
 *   s = (sum_j G_j * G_j) / d;  acc' = acc + s;  den = sqrt(acc' + eps)  (mode 1)  or  sqrt(acc') + eps  (mode 2);
 *   scale = lr / den  (one division per row);  w_j' = w_j - scale * G_j
 * The order of the d additions is fixed (csrc/table_rules.h), so a call is bit-reproducible.
 * _sparse: the looked-up rows, from UNSORTED ids (int32 / int64) and grad_out[n, d]; duplicates are summed first, in the
 * order of tfrs_table_update_sparse (the same bits); ids outside [0, vocab) are ignored; untouched rows are not written.
 * rowscan != 0: the sort-free row scan (d <= 256), else radix sort + one lane group per run, with workspace from
 * tfrs_table_update_workspace_bytes(n, rowscan).  n == 0: nothing is written.
 * _dense: every row of param[rows, d] from grad[rows, d]; a row whose gradient is all zero keeps its bits.
 * lr_dev: NULL (lr is taken by value), or the device float of tfrs_lr_tick, read once at kernel entry.
 * Every argument check comes before any device call. */
int tfrs_rowwise_adagrad_sparse(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d, int64_t vocab,
                                float *table, float *accum, float lr, const float *lr_dev, float eps, int mode,
                                int rowscan, void *workspace, size_t workspace_bytes, void *stream);
int tfrs_rowwise_adagrad_dense(float *param, float *accum, const float *grad, int64_t rows, int d, float lr,
                               const float *lr_dev, float eps, int mode, void *stream);
/* Learning-rate schedules on the device (recommenders_amd/schedules.py): the learning rate of a step is a DEVICE float
 * that a one-thread kernel at the head of the step writes from a DEVICE counter, so a captured step replays the whole
 * schedule.  A schedule is a kind, a HOST array of 8 doubles and (kinds 0, 5, 6) a DEVICE f32 table of table_len entries;
 * with s the counter as a double:
 *   0 external      lr = table[0]: a device float the caller owns, re-read every step
 *   1 exponential   {initial, decay_steps, decay_rate, staircase}: p = s / decay_steps, floored when staircase;
 *                   lr = initial * decay_rate^p
 *   2 inverse time  the same four: lr = initial / (1 + decay_rate * p)
 *   3 polynomial    {initial, decay_steps, end, power, cycle}: x = min(s, decay_steps), ds = decay_steps, or with cycle
 *                   x = s, ds = decay_steps * (s == 0 ? 1 : ceil(s / decay_steps)); lr = (initial - end) * (1 - x / ds)^power + end
 *   4 cosine        {initial, decay_steps, alpha, has_warmup, warmup_target, warmup_steps}: with a warm-up and
 *                   s < warmup_steps, lr = initial + (warmup_target - initial) * s / warmup_steps; else (the warm-up
 *                   replacing initial by warmup_target and s by s - warmup_steps) x = min(s, decay_steps),
 *                   lr = initial * ((1 - alpha) * 0.5 * (1 + cos(pi * x / decay_steps)) + alpha)
 *   5 piecewise     params = table_len - 1 boundaries (1..7), table = values: table[i] for the smallest i with
 *                   s <= boundary[i], else the last value
 *   6 tabulated     table[min(counter, table_len - 1)]
 * evaluated in float64 and rounded once to f32 (the table kinds copy an f32).
 * tfrs_lr_tick: t = *iterations; lr_out[0] = schedule(t); with ftrl != 0 also
 * lr_out[1] = (float)(2 * (l2 + beta / (2 * (double)lr_out[0]))), the third hyper-parameter of the Ftrl rule;
 * *iterations = t + advance (0 or 1: the groups of one optimizer are all evaluated at the same t, the last one advances).
 * tfrs_adam_tick_scheduled: tfrs_adam_tick whose learning rate is schedule(t - 1) for t = *step + advance -- Keras's
 * iterations before the increment -- rounded to f32 into *lr_out; alpha is computed from that f32.
 * The *_dlr entries are the update entries above with one more argument, lr_dev: NULL (then they ARE the entries
 * above, which forward to them), or the device float of tfrs_lr_tick, which the kernels read once at entry in place of
 * lr; the constant-lr kernels and the device-lr kernels are separate instantiations (the constant-lr ones are
 * instruction for instruction what they were without the argument).  For tfrs_table_update_sparse / _dense_multi a
 * non-NULL alpha with rule 0 (SGD) is that device float, with rule 2 (Ftrl) the two floats lr_out[0..1]; hyper_h[0] (and
 * Ftrl's hyper_h[2]) are then not read -- the rule resolves it once at kernel entry, in the same instantiations.
 * Every argument check comes before any device call. */
int tfrs_lr_tick(int64_t *iterations, float *lr_out, int kind, const double *params_h, const float *table,
                 int64_t table_len, int ftrl, double l2, double beta, int advance, void *stream);
int tfrs_adam_tick_scheduled(int64_t *step, float *alpha, float *lr_out, int kind, const double *params_h,
                             const float *table, int64_t table_len, double beta_1, double beta_2, int advance,
                             void *stream);
int tfrs_embedding_scatter_add_unsorted_dlr(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d,
                                            int64_t vocab, float *grad_table_or_table, float *accum, float lr,
                                            const float *lr_dev, float eps, int adagrad, void *workspace,
                                            size_t workspace_bytes, void *stream);
int tfrs_embedding_scatter_add_rowscan_dlr(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d,
                                           int64_t vocab, float *grad_table_or_table, float *accum, float lr,
                                           const float *lr_dev, float eps, int adagrad, void *stream);
int tfrs_embedding_scatter_add_rowscan_multi_dlr(int ntables, const float *const *grad_out_h, const void *const *ids_h,
                                                 const int *ids_are_i64_h, const int64_t *n_h, const int *d_h,
                                                 const int64_t *vocab_h, float *const *tables_h, float *const *accum_h,
                                                 float lr, const float *lr_dev, float eps, int adagrad, void *stream);
int tfrs_adagrad_dense_multi_dlr(int ntensors, float *const *params_h, float *const *accum_h, const float *const *grads_h,
                                 const int64_t *n_h, float lr, const float *lr_dev, float eps, int mode, void *stream);
int tfrs_clippy_dense_multi_dlr(int ntensors, float *const *params_h, float *const *accum_h, const float *const *grads_h,
                                const int64_t *n_h, float *factors, float lr, const float *lr_dev, float eps,
                                float var_rel, float acc_rel, float abs_thr, int mode, void *stream);
int tfrs_clippy_sparse_dlr(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d, int64_t vocab,
                           float *table, float *accum, float *factor, float lr, const float *lr_dev, float eps,
                           float var_rel, float acc_rel, float abs_thr, int mode, int rowscan, void *workspace,
                           size_t workspace_bytes, void *stream);
/* Up to 16 device buffers copied in ONE launch: a batch's input tensors into the static buffers of a captured
 * train / test step (the `Model.fit` loop of models/base.py:64-85 replays HIP graphs; README.md:84-98).  Host arrays of
 * device pointers and byte counts; buffers must not overlap. */
int tfrs_copy_multi(int nbuffers, void *const *dst_h, const void *const *src_h, const int64_t *bytes_h, void *stream);

/* ------------------------------------------------------------------------- *
 * tf.keras.layers.Hashing(num_bins, salt=[s0, s1]) as UnifiedEmbedding applies it per
 * feature chunk (layers/feature_multiplexing/unified_embedding.py:116-119,155-159,198-205):
 * bucket = SipHash-2-4_{(s0, s1)}(bytes) mod num_bins (unsigned), where bytes is the decimal
 * string of an integer id (tf.as_string) or the string itself.  out[n] int64.
 *   _ids:   ids[n] int32/int64 on the device.
 *   _bytes: n strings packed back to back in `bytes`, string i = bytes[offsets[i]:offsets[i+1]].
 * ------------------------------------------------------------------------- */
int tfrs_hash_bucket_strong_ids(const void *ids, int ids_are_i64, int64_t n, int64_t num_bins,
                                uint64_t salt0, uint64_t salt1, int64_t *out, void *stream);
int tfrs_hash_bucket_strong_bytes(const unsigned char *bytes, const int64_t *offsets, int64_t n,
                                  int64_t num_bins, uint64_t salt0, uint64_t salt1,
                                  int64_t *out, void *stream);

/* Fused UnifiedEmbedding.call for one feature (unified_embedding.py:198-215): for value v and
 * chunk c, bucket = SipHash-2-4_{(salt0[c], salt1[c])}(value) mod num_bins and
 *   out[v, c*d:(c+1)*d] = tables[c][bucket, :]
 * i.e. Hashing -> lookup -> concat of the feature's n_chunks components in one pass.  Values are
 * ids[n_values] (int32/int64) or, when `bytes` != NULL, strings packed as in
 * tfrs_hash_bucket_strong_bytes.  `tables`, `salt0`, `salt1` are HOST arrays of n_chunks
 * entries (device table pointers, each [num_bins, d]); d must be 4 * 2^k <= 256, otherwise
 * TFRS_ENOTIMPL.  out[n_values, n_chunks * d]; buckets[n_values, n_chunks] (optional, may be
 * NULL) keeps the bucket of every lookup for the backward (the IndexedSlices indices). */
int tfrs_unified_embedding_fwd(const void *ids, int ids_are_i64, const unsigned char *bytes,
                               const int64_t *offsets, int64_t n_values, int n_chunks,
                               const float *const *tables, const uint64_t *salt0,
                               const uint64_t *salt1, int64_t num_bins, int d, float *out,
                               int64_t *buckets, void *stream);

/* The same for EVERY dense integer feature of a UnifiedEmbedding layer in one launch
 * (unified_embedding.py:186-215 loops over the features).  A unit u is one (feature, chunk):
 *   outs[u][v, chunk_index[u]*d : (chunk_index[u]+1)*d] = tables[u][bucket(ids[u][v], salt0[u], salt1[u]), :]
 * where outs[u] is the [n_values, feature_chunks[u] * d] output of the unit's feature (the units of one
 * feature share it).  All host arrays have n_units entries; every ids[u] holds n_values ids of the same
 * integer width.  buckets[n_values, n_units] (optional) keeps the buckets for the backward. */
int tfrs_unified_embedding_fwd_multi(int n_units, const void *const *ids, int ids_are_i64,
                                     int64_t n_values, const float *const *tables,
                                     const uint64_t *salt0, const uint64_t *salt1, int64_t num_bins,
                                     int d, float *const *outs, const int32_t *feature_chunks,
                                     const int32_t *chunk_index, int64_t *buckets, void *stream);

/* ------------------------------------------------------------------------- *
 * tf.keras.layers.IntegerLookup / StringLookup (the vocabulary layers in front of every Embedding of
 * the reference's tutorials): token -> index through a device-resident hash table.
 *
 * table: `capacity` slots of 16 bytes {int64 key, int64 value}, 16-byte aligned; open addressing, linear
 * probing, capacity a power of two >= 2 * n (anything else: TFRS_EINVAL).  A free slot holds
 * TFRS_VOCAB_EMPTY_KEY, which is never stored: a token of that value is skipped by the build and
 * answered by the lookup from `empty_value`.  No probe loop runs more than `capacity` steps.
 *
 * tfrs_vocab_build: clears the table and *flags (one launch), then inserts keys[i] -> i (one launch,
 *   64-bit compare-and-swap on the key word).  *flags (device) afterwards: TFRS_VOCAB_DUPLICATE_KEY when
 *   two keys are equal, TFRS_VOCAB_TABLE_FULL when a key found no slot.
 * tfrs_vocab_lookup: ids[n] int32/int64 -> out[n] int64:
 *     0                                      when has_mask and id == mask_key
 *     base + value                           when the id is a key (or is TFRS_VOCAB_EMPTY_KEY and
 *                                            empty_value >= 0; then value = empty_value)
 *     oov_base + floormod(id, num_oov)       otherwise (oov_unsigned: the unsigned remainder);
 *     -1                                     ... when num_oov == 0
 *   *unknown_count (device, optional) += the number of ids of the last two kinds.  No synchronisation,
 *   no allocation: capturable.
 * tfrs_fingerprint_bytes: out[i] = SipHash-2-4 (all 64 bits, key bytes 00 01 .. 0f) of string i, packed as in
 *   tfrs_hash_bucket_strong_bytes: the integer keys of StringLookup.
 * ------------------------------------------------------------------------- */
#define TFRS_VOCAB_EMPTY_KEY INT64_MIN
#define TFRS_VOCAB_DUPLICATE_KEY 1u
#define TFRS_VOCAB_TABLE_FULL 2u
int tfrs_vocab_build(const int64_t *keys, int64_t n, void *table, int64_t capacity, uint32_t *flags,
                     void *stream);
int tfrs_vocab_lookup(const void *ids, int ids_are_i64, int64_t n, const void *table, int64_t capacity,
                      int64_t n_tokens, int64_t base, int has_mask, int64_t mask_key, int64_t empty_value,
                      int64_t oov_base, int64_t num_oov, int oov_unsigned, int64_t *unknown_count,
                      int64_t *out, void *stream);
int tfrs_fingerprint_bytes(const unsigned char *bytes, const int64_t *offsets, int64_t n, int64_t *out,
                           void *stream);

/* ------------------------------------------------------------------------- *
 * tf.keras.layers.TextVectorization (the title tower of the reference's retrieval tutorials): packed strings
 * -> token indices in one launch.  Strings are packed as in tfrs_hash_bucket_strong_bytes:
 * bytes[n_bytes] and offsets[n + 1].  Byte rules, ASCII only:
 *   standardize  bit TFRS_TEXT_LOWER: A-Z -> a-z; bit TFRS_TEXT_STRIP_PUNCTUATION: the 32 bytes
 *                !"#$%&'()*+,-./:;<=>?@[\]^_`{|}~ are deleted.  Bytes 0x80-0xFF pass unchanged.
 *   split        TFRS_TEXT_SPLIT_WHITESPACE: tokens are maximal runs of bytes other than space \t \n \v \f \r
 *                (a run whose bytes were all deleted is no token); TFRS_TEXT_SPLIT_NONE: the standardised
 *                string is one token, none when it is empty.
 * A token is known by the SipHash-2-4 fingerprint of its standardised bytes (the key of tfrs_fingerprint_bytes)
 * and looked up in a table of tfrs_vocab_build with the probe of tfrs_vocab_lookup (its empty_value rule
 * included).  Every lane clamps its offsets into [0, n_bytes] and to lo <= hi, and no byte outside [0, n_bytes)
 * is ever read: malformed offsets give wrong indices, never a read out of bounds.  No synchronisation, no
 * allocation: capturable.  Bad arguments (NULL pointers, negative counts, a capacity that is no power of two
 * >= 2 * n_tokens, seq_len < 1 on the dense route) return TFRS_EINVAL before any launch.
 *
 * tfrs_text_count_tokens: counts[i] = tokens of string i.
 * tfrs_text_vectorize: token t of string i -> 2 + value, or 1 when unknown (0 is the padding index).
 *   row_splits == NULL: dense out[n, seq_len], the first seq_len tokens of a row, zero-filled past the last;
 *   otherwise ragged out[row_splits[i] + t] for t < row_splits[i + 1] - row_splits[i] (row_splits: the
 *   exclusive scan of tfrs_text_count_tokens with the same standardize / split).
 * tfrs_text_token_spans: the ragged emit of adapt: per token its fingerprint and the span [start, end) of its
 *   RAW bytes in the blob (whitespace split: the maximal run of bytes that are no whitespace; no split: the
 *   whole string).
 * The kernel streams a workgroup's strings through an LDS window of TFRS_TEXT_WINDOW_BYTES or reads them
 * directly (TFRS_TEXT_VARIANT = window / direct), on at most TFRS_TEXT_MAX_BLOCKS workgroups
 * of 256 strings, grid-stride beyond.
 * ------------------------------------------------------------------------- */
#define TFRS_TEXT_LOWER 1
#define TFRS_TEXT_STRIP_PUNCTUATION 2
#define TFRS_TEXT_SPLIT_NONE 0
#define TFRS_TEXT_SPLIT_WHITESPACE 1
#define TFRS_TEXT_WINDOW_BYTES 16384
#define TFRS_TEXT_MAX_BLOCKS 2048
int tfrs_text_count_tokens(const unsigned char *bytes, int64_t n_bytes, const int64_t *offsets, int64_t n,
                           int standardize, int split, int64_t *counts, void *stream);
int tfrs_text_vectorize(const unsigned char *bytes, int64_t n_bytes, const int64_t *offsets, int64_t n,
                        int standardize, int split, const void *table, int64_t capacity, int64_t n_tokens,
                        int64_t empty_value, const int64_t *row_splits, int64_t seq_len, int64_t *out,
                        void *stream);
int tfrs_text_token_spans(const unsigned char *bytes, int64_t n_bytes, const int64_t *offsets, int64_t n,
                          int standardize, int split, const int64_t *row_splits, int64_t *fingerprints,
                          int64_t *starts, int64_t *ends, void *stream);

/* ------------------------------------------------------------------------- *
 * Retrieval.call loss (tasks/retrieval.py:172-210, layers/loss.py:114-158):
 * in-batch sampled softmax without materialising the [nq, nc] logits.
 *   S = q c^T [/ temperature] [- log clip(p_c, 1e-6, 1)]
 *       [+ MIN_FLOAT where cand_ids[c] == cand_ids[b], c != b] [MIN_FLOAT where !mask]
 *   loss = sum_b w_b * (logsumexp_c S_bc - S_bb)
 * out_loss: device float; out_lse[nq], out_pos[nq] saved for backward.  Optional
 * inputs may be NULL (sample_weight, log_q_correction = log clip(p), cand_ids, mask).
 * Requires nc >= nq (labels = eye(nq, nc)) and d <= 128.  Forward and backward share one
 * workspace size query.
 * ------------------------------------------------------------------------- */
size_t tfrs_inbatch_softmax_workspace_bytes(int64_t nq, int64_t nc, int d);
int tfrs_inbatch_softmax_ce_fwd(const float *q, const float *c, int64_t nq, int64_t nc,
                                int d, const float *sample_weight, float inv_temperature,
                                const float *log_q_correction, const int64_t *cand_ids,
                                const uint8_t *score_mask, float *out_loss,
                                float *out_lse, float *out_pos, void *workspace,
                                size_t workspace_bytes, void *stream);
/* dq[nq, d], dc[nc, d] for upstream scalar gradient `gloss` (device float, NULL = 1).
 * reuse_forward_workspace != 0 promises that `workspace` is the buffer the forward call was
 * given for the same q, c, sample_weight and has not been written since: the backward then
 * reuses the operand images the forward left there instead of rebuilding them. */
int tfrs_inbatch_softmax_ce_bwd(const float *q, const float *c, int64_t nq, int64_t nc,
                                int d, const float *sample_weight, float inv_temperature,
                                const float *log_q_correction, const int64_t *cand_ids,
                                const uint8_t *score_mask, const float *lse,
                                const float *gloss, float *dq, float *dc, void *workspace,
                                size_t workspace_bytes, int reuse_forward_workspace,
                                void *stream);

/* ------------------------------------------------------------------------- *
 * The same loss for MULTI-HEAD (max-sim) queries q[nq, heads, d] (tasks/retrieval.py:172-176), without the
 * [nq * heads, nc] head scores or the [nq, nc] logits:
 *   M_bc  = max_h (q_bh . c_c)              the max is taken on the raw dot products, as the reference does
 *   S_bc  = M_bc [/ temperature] [- log clip(p_c)] [+ MIN_FLOAT accidental hits] [MIN_FLOAT where !mask]
 *   loss  = sum_b w_b (logsumexp_c S_bc - S_bb)
 *   G_bc  = gloss * w_b * (exp(S_bc - lse_b) - [b == c]) / temperature      (0 where masked)
 *   h*(b,c) = the LOWEST head index attaining the max (the first-index rule of an argmax; TensorFlow's reduce_max
 *             splits the gradient evenly among tied heads -- a deviation at exact ties only)
 *   dq_bh = sum_c [h == h*(b,c)] G_bc c_c ,   dc_c = sum_b G_bc q_{b,h*(b,c)}
 * 1 <= heads <= 32, 1 <= d <= TFRS_MAX_DIM, nc >= nq; anything else is TFRS_EINVAL before the device is touched,
 * as are NULL pointers and a workspace below tfrs_inbatch_softmax_mh_workspace_bytes (shared by both calls).
 * score_mask is [nq, nc]; out_lse[nq], out_pos[nq] are kept for the backward; dq is [nq, heads, d], dc [nc, d].
 * f32 MFMA arithmetic throughout; deterministic (no float atomics).
 * ------------------------------------------------------------------------- */
size_t tfrs_inbatch_softmax_mh_workspace_bytes(int64_t nq, int heads, int64_t nc, int d);
int tfrs_inbatch_softmax_mh_ce_fwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc, int d,
                                   const float *sample_weight, float inv_temperature,
                                   const float *log_q_correction, const int64_t *cand_ids,
                                   const uint8_t *score_mask, float *out_loss, float *out_lse, float *out_pos,
                                   void *workspace, size_t workspace_bytes, void *stream);
int tfrs_inbatch_softmax_mh_ce_bwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc, int d,
                                   const float *sample_weight, float inv_temperature,
                                   const float *log_q_correction, const int64_t *cand_ids,
                                   const uint8_t *score_mask, const float *lse, const float *gloss, float *dq,
                                   float *dc, void *workspace, size_t workspace_bytes, void *stream);
/* The split geometry of the in-batch softmax kernels under the options in force (TFRS_SOFTMAX_WAVES, _WGS, _WGS_BWD,
 * _NW: all read per call).  Host only, no device call; the launches use exactly these plans.  A side's streamed rows
 * are cut into nsplit splits of split_len rows (a multiple of 32; the last split may be shorter).
 *   _plan_f32 (f32-MFMA kernels, 1 <= heads <= 32): out[4] = {nsplit, split_len} of the forward / dq (streams the nc
 *             candidates), then of dc (streams the nq * Hp flat head slots, Hp = heads rounded up to a power of two)
 *   _plan_f16 (split-fp16 kernels): out[6] = {nsplit, split_len} of the forward, of dq (both stream candidates) and
 *             of dc (streams queries)
 * nq >= 1, nc >= nq, out != NULL, else TFRS_EINVAL. */
int tfrs_inbatch_softmax_plan_f32(int64_t nq, int heads, int64_t nc, int64_t *out);
int tfrs_inbatch_softmax_plan_f16(int64_t nq, int64_t nc, int64_t *out);

/* ------------------------------------------------------------------------- *
 * Hard-negative mining (layers/loss.py:61-111), the cross-entropy on the mined logits (tasks/retrieval.py:205-210)
 * and the batch metrics' rank count (:228-232) over ADJUSTED in-batch logits of 2-D queries, without the [nq, nc]
 * matrix.  These entry points take the TEMPERATURE itself (1 for none), not its reciprocal:
 *   S_bc = (q_b . c_c) / temperature - log_q_correction_c [+ MIN_FLOAT where cand_ids[c] == cand_ids[b], c != b]
 *          [= MIN_FLOAT where !score_mask_bc]     IEEE f32 division, as the reference's scores / temperature;
 *                                                  -0 counts as +0; non-finite embeddings are outside the contract
 *   keep(b, c) = (c == b) || S_bc > tau_b || (S_bc == tau_b && c <= cut_b)
 *   tfrs_inbatch_mined_select: with n = min(num_hard_negatives, nc - 1), tau[b] = the n-th largest negative logit of
 *     row b and cut[b] = the column of the last tied negative that is taken (INT64_MAX: all ties) -- the kept set is
 *     the positive and the n largest negatives, equal values going to the lower column (tf.math.top_k).  n = 0:
 *     tau = +inf, cut = -1.  Exact (a radix select on the device), a fixed launch sequence: capturable.
 *   tfrs_inbatch_mined_ce_fwd: loss = sum_b w_b (logsumexp_{c : keep(b, c)} S_bc - S_bb); out_lse[nq], out_pos[nq].
 *   tfrs_inbatch_mined_ce_bwd: G_bc = gloss * w_b * (exp(S_bc - lse_b) - [b == c]) / temperature where keep(b, c)
 *     and not masked, 0 elsewhere; dq = G c, dc = G^T q.  Deterministic, no float atomics.
 *   tfrs_inbatch_mined_rank_count: counts[b] = #{c != b : keep(b, c) and S_bc > S_bb}, bit 31 set for a non-finite
 *     S_bb: the uint32 counts[nq] convention of tfrs_rank_count_accumulate, consumed by tfrs_topk_hits_update.
 *   tau / cut of the last three: both NULL keeps every column (adjustments without mining).
 * Optional inputs (sample_weight, log_q_correction = log clip(p, 1e-6, 1), cand_ids, score_mask) may be NULL.
 * TFRS_EINVAL before any device call: a shape below 1, nc < nq, d > TFRS_MAX_DIM, a NULL operand / output /
 * workspace, a temperature that is zero or not finite, num_hard_negatives < 0, tau without cut, a workspace below
 * tfrs_inbatch_mined_workspace_bytes (one size for the four calls, each of which overwrites it).
 *   tfrs_inbatch_mined_plan (host only): out[4] = {nsplit, split_len} of the kernels that stream candidates
 *     (selection, forward, count, dq), then of dc (streams queries), under TFRS_SOFTMAX_WAVES.
 * ------------------------------------------------------------------------- */
size_t tfrs_inbatch_mined_workspace_bytes(int64_t nq, int64_t nc, int d);
int tfrs_inbatch_mined_plan(int64_t nq, int64_t nc, int64_t *out);
int tfrs_inbatch_mined_select(const float *q, const float *c, int64_t nq, int64_t nc, int d, float temperature,
                              const float *log_q_correction, const int64_t *cand_ids, const uint8_t *score_mask,
                              int64_t num_hard_negatives, float *tau, int64_t *cut, void *workspace,
                              size_t workspace_bytes, void *stream);
int tfrs_inbatch_mined_ce_fwd(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                              const float *sample_weight, float temperature, const float *log_q_correction,
                              const int64_t *cand_ids, const uint8_t *score_mask, const float *tau,
                              const int64_t *cut, float *out_loss, float *out_lse, float *out_pos, void *workspace,
                              size_t workspace_bytes, void *stream);
int tfrs_inbatch_mined_ce_bwd(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                              const float *sample_weight, float temperature, const float *log_q_correction,
                              const int64_t *cand_ids, const uint8_t *score_mask, const float *tau,
                              const int64_t *cut, const float *lse, const float *gloss, float *dq, float *dc,
                              void *workspace, size_t workspace_bytes, void *stream);
int tfrs_inbatch_mined_rank_count(const float *q, const float *c, int64_t nq, int64_t nc, int d, float temperature,
                                  const float *log_q_correction, const int64_t *cand_ids, const uint8_t *score_mask,
                                  const float *tau, const int64_t *cut, uint32_t *counts, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* Multi-head exact top-K (BruteForce on queries [nq, heads, d]): scores / rows [nq, heads, k_in] are the top-k_in
 * lists of the nq * heads flat (query, head) rows (descending; row < 0 = empty).  Writes, per query, the top-k_out
 * of max_h score under (score descending, row ascending): a row that appears in several lists counts once, with
 * its highest score.  With k_out <= k_in that is the exact top-k_out of the max over heads (the union of the lists
 * contains it).  heads <= 32, k_in <= TFRS_MAX_K, heads * k_in <= 8192 (one workgroup's LDS); empty output
 * slots carry row -1 and score -inf. */
int tfrs_topk_merge_heads(const float *scores, const int32_t *rows, int64_t nq, int heads, int k_in, int k_out,
                          float *out_scores, int32_t *out_rows, void *stream);

/* ------------------------------------------------------------------------- *
 * Keras CategoricalCrossentropy(from_logits=True, reduction=SUM) on an EXPLICIT logits matrix
 * (tasks/retrieval.py:86-87, :210) -- only for the Retrieval paths that must build [nq, nc] (multi-head queries
 * :172-176, dims above TFRS_MAX_DIM, batch metrics / hard negatives after a logit adjustment :205-208); the default
 * loss is the fused tfrs_inbatch_softmax_ce_*.  labels[nq, nc] as the reference builds them (:185, loss.py:108-109).
 *   fwd: row_loss[i] = w_i * (lse_i * sum_j y_ij - sum_j y_ij s_ij); lse[nq], ysum[nq] are kept for the backward
 *   bwd: dlogits[i, j] = grad_scale[0] * w_i * (softmax(S_i)_j * ysum_i - y_ij)   (grad_scale: device scalar)
 * ------------------------------------------------------------------------- */
int tfrs_logits_ce_fwd(const float *logits, const float *labels, int64_t nq, int64_t nc,
                       const float *sample_weight, float *row_loss, float *lse, float *ysum, void *stream);
int tfrs_logits_ce_bwd(const float *logits, const float *labels, int64_t nq, int64_t nc,
                       const float *sample_weight, const float *lse, const float *ysum,
                       const float *grad_scale, float *dlogits, void *stream);

/* ------------------------------------------------------------------------- *
 * Listwise ranking losses and NDCG on labels[nlists, len] / scores[nlists, len] (row-major f32), the losses and the
 * metric that the listwise-ranking tutorial hands to tasks.Ranking (losses.py, metrics/listwise.py; formulas and
 * summation orders: DESIGN 4.24 and the header of csrc/listwise.hip).  Position i of a list is valid iff
 * labels[i] >= 0 (-1 pads); invalid positions are selected out, never multiplied by zero, and receive gradient +0.
 * 1 <= len <= TFRS_LISTWISE_MAX_LEN and nlists * len < 2^31, else TFRS_EINVAL before any device call; nlists == 0
 * returns TFRS_OK without a launch.  One launch each, on `stream`, no workspace, no atomics: bit-reproducible.
 *   fwd:  loss[l] = the list's loss of `kind`
 *   bwd:  dscores[l, i] = scale[l] * d loss[l] / d scores[l, i], recomputed from labels and scores alone
 *   ndcg: ndcg[l] = DCG / IDCG over the first min(n, topn) ranks (topn == 0: no cut) and counted[l] = 1 where
 *         IDCG > 0; else both 0
 * ------------------------------------------------------------------------- */
#define TFRS_LISTWISE_MAX_LEN 1024
#define TFRS_LISTWISE_SOFTMAX 0
#define TFRS_LISTWISE_PAIRWISE_LOGISTIC 1
#define TFRS_LISTWISE_PAIRWISE_HINGE 2
#define TFRS_LISTWISE_LIST_MLE 3
int tfrs_listwise_loss_fwd(int kind, const float *labels, const float *scores, int64_t nlists, int len, float *loss,
                           void *stream);
int tfrs_listwise_loss_bwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                           const float *scale, float *dscores, void *stream);
int tfrs_listwise_ndcg(const float *labels, const float *scores, int64_t nlists, int len, int topn, float *ndcg,
                       float *counted, void *stream);
/* The list metrics of one step out of ONE launch (metrics/listwise.py; formulas: DESIGN 4.26): the list is loaded once
 * and sorted by score once for every requested metric.  kinds[m] / topns[m], m < nmetrics <= TFRS_LISTWISE_METRIC_MAX,
 * are HOST arrays, read before the launch (they travel as a kernel argument: no copy, the call can be captured);
 * topns[m] == 0 means no cut.  values[m * nlists + l] is metric m's value of list l and weights[m * nlists + l] its
 * non-negative weight (value +0 where the weight is 0); a metric's result over lists is sum w v / sum w.  With
 * rel = [label >= 1], R the relevant items of the list, c_r those at score ranks <= r and k = min(n, topn):
 *   NDCG       DCG / IDCG as tfrs_listwise_ndcg (bit for bit), weight [IDCG > 0]
 *   DCG        sum_{r<k} (2^y - 1) / log2(r + 2), weight [some label > 0]
 *   MRR        1 / (first relevant rank below k, 1-based), 0 if none        weight [R > 0] for these five
 *   HITS       1 if a relevant item ranks below k, else 0
 *   PRECISION  c_{k-1} / min(topn, len)   (len, the padded width, when topn == 0)
 *   RECALL     c_{k-1} / R
 *   MAP        (sum over the relevant ranks r < k of c_r / (r + 1)) / R
 *   ARP        sum_V y (r + 1) / sum_V y, weight sum_V y                     (no topn)
 *   OPA        C / P, P = pairs with y_i > y_j, C = those with s_i > s_j (a tie is wrong), weight P   (no topn)
 * TFRS_EINVAL before any device call: nmetrics outside 1 .. TFRS_LISTWISE_METRIC_MAX, an unknown kind, topn < 0, a
 * non-zero topn for ARP or OPA, a NULL pointer, a shape outside the envelope above. */
#define TFRS_LISTWISE_METRIC_MAX 16
#define TFRS_LISTWISE_METRIC_NDCG 0
#define TFRS_LISTWISE_METRIC_DCG 1
#define TFRS_LISTWISE_METRIC_MRR 2
#define TFRS_LISTWISE_METRIC_HITS 3
#define TFRS_LISTWISE_METRIC_PRECISION 4
#define TFRS_LISTWISE_METRIC_RECALL 5
#define TFRS_LISTWISE_METRIC_MAP 6
#define TFRS_LISTWISE_METRIC_ARP 7
#define TFRS_LISTWISE_METRIC_OPA 8
int tfrs_listwise_metrics(const float *labels, const float *scores, int64_t nlists, int len, int nmetrics,
                          const int *kinds, const int *topns, float *values, float *weights, void *stream);
/* The two pairwise kinds with LambdaRank / LambdaLoss pair weights (losses.DCGLambdaWeight / NDCGLambdaWeight; formulas:
 * DESIGN 4.25): every pair term is multiplied by
 *   w_ij = |G_i - G_j| * ((1 - smooth_fraction) * |D(r_i) - D(r_j)| + smooth_fraction * |D0(d) - D0(d + 1)|),
 * r = the rank by score (descending, ties by position ascending), d = |r_i - r_j|, D0(r) = 1 / log2(r + 1), D = D0 cut to
 * 0 beyond rank topn (topn == 0: no cut; w_ij = 0 when both ranks lie beyond it), G = 2^label - 1, divided by the
 * list's IDCG@topn when `normalized` (every weight 0 where that is not positive).  The weights are constants of the
 * backward.  Same envelope, same validity rule, one launch each on `stream`, no workspace, no atomics.  TFRS_EINVAL
 * before any device call for a kind other than the two pairwise ones, topn < 0 or a smooth_fraction outside [0, 1]
 * (NaN included). */
int tfrs_listwise_lambda_fwd(int kind, const float *labels, const float *scores, int64_t nlists, int len, int topn,
                             int normalized, float smooth_fraction, float *loss, void *stream);
int tfrs_listwise_lambda_bwd(int kind, const float *labels, const float *scores, int64_t nlists, int len, int topn,
                             int normalized, float smooth_fraction, const float *scale, float *dscores, void *stream);
/* The pair-sum losses (losses.ApproxNDCGLoss / ApproxMRRLoss / UniqueSoftmaxLoss): every item first needs a
 * sum over the other items of its list, and the gradient is a second pair sum over those.  One list, V the valid
 * positions, n = |V|, alpha = float32(1 / temperature), sigma(x) = 1 / (1 + e^-x), sigma'(x) = sigma(x) sigma(-x),
 * G_i = 2^{y_i} - 1, and the soft rank r_i = 1 + sum_{j in V, j != i} sigma(alpha (s_j - s_i)):
 *   APPROX_NDCG     l = -(1 / IDCG) sum_V G_i / log2(1 + r_i), IDCG the ideal DCG of tfrs_listwise_ndcg without a cut;
 *                   c_i = G_i / (IDCG ln2 (1 + r_i) log2(1 + r_i)^2)
 *   APPROX_MRR      l = -(1 / Y) sum_V y_i / r_i, Y = sum_V y_i;  c_i = y_i / (Y r_i^2)
 *                   both: dl/ds_k = alpha sum_{j in V, j != k} (c_j - c_k) sigma'(alpha (s_k - s_j)); l = 0 and every
 *                   gradient +0 where IDCG <= 0 (Y <= 0)
 *   UNIQUE_SOFTMAX  t = alpha s, lse_i = log(e^{t_i} + sum_{j in V: y_j < y_i} e^{t_j}), l = sum_V G_i (lse_i - t_i);
 *                   dl/ds_k = alpha [G_k (e^{t_k - lse_k} - 1) + sum_{j in V: y_j > y_k} G_j e^{t_k - lse_j}]; finite
 *                   for any finite scores (every lse is shifted by its own maximum)
 * fwd: loss[l]; bwd: dscores[l, i] = scale[l] * dl/ds_i, recomputed from labels and scores alone.  Same envelope, same
 * validity rule, one launch each on `stream`, no workspace, no atomics.  TFRS_EINVAL before any device call for an
 * unknown kind, or a temperature that is not finite and positive or whose float32 reciprocal is not finite. */
#define TFRS_LISTWISE_APPROX_NDCG 0
#define TFRS_LISTWISE_APPROX_MRR 1
#define TFRS_LISTWISE_UNIQUE_SOFTMAX 2
int tfrs_listwise_pairsum_fwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                              float temperature, float *loss, void *stream);
int tfrs_listwise_pairsum_bwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                              float temperature, const float *scale, float *dscores, void *stream);

/* ------------------------------------------------------------------------- *
 * Cross.call (layers/feature_interaction/dcn.py:151-186), full rank, linear
 * preactivation:  y = x0 * (x @ kernel + bias + diag_scale * x) + x
 * kernel[d, d] is Keras Dense layout [in, out]; bias may be NULL.
 * ------------------------------------------------------------------------- */
int tfrs_cross_fwd(const float *x0, const float *x, const float *kernel,
                   const float *bias, float diag_scale, int64_t batch, int d, float *y,
                   void *stream);
/* Gradients of the same layer (its backward under tfrs.Model.train_step, models/base.py:77):
 * with z = x @ kernel + bias + diag_scale * x and dz = dy * x0
 *   dx0 = dy * z ;  dx = dz @ kernel^T + dy + diag_scale * dz ;
 *   dkernel = x^T @ dz ;  dbias[d] = column sums of dz (NULL to skip).
 * Three fused GEMM launches: z and dz never exist in HBM and nothing is transposed.
 * tfrs_cross_bwd = f32 MFMA; tfrs_cross_bwd_f16 = split-fp16 MFMA (large products), same
 * results to f32 accuracy.  workspace from tfrs_cross_bwd_workspace_bytes(batch, d, f16). */
size_t tfrs_cross_bwd_workspace_bytes(int64_t batch, int d, int f16);
int tfrs_cross_bwd(const float *x0, const float *x, const float *kernel, const float *bias,
                   float diag_scale, const float *dy, int64_t batch, int d, float *dx0,
                   float *dx, float *dkernel, float *dbias, void *workspace,
                   size_t workspace_bytes, void *stream);
int tfrs_cross_bwd_f16(const float *x0, const float *x, const float *kernel, const float *bias,
                       float diag_scale, const float *dy, int64_t batch, int d, float *dx0,
                       float *dx, float *dkernel, float *dbias, void *workspace,
                       size_t workspace_bytes, void *stream);
/* Training pair that trades 4 * batch * d bytes for one of the three products: the forward also
 * stores u = x @ kernel + bias + diag_scale * x (u_out[batch, d]; workspace as tfrs_cross_fwd_f16),
 * the backward forms dx0 = dy * u elementwise and runs the other two fused GEMMs
 * (workspace from tfrs_cross_bwd_workspace_bytes(batch, d, 1)). */
int tfrs_cross_fwd_f16_train(const float *x0, const float *x, const float *kernel,
                             const float *bias, float diag_scale, int64_t batch, int d, float *y,
                             float *u_out, void *workspace, size_t workspace_bytes, void *stream);
int tfrs_cross_bwd_f16_saved(const float *x0, const float *x, const float *u, const float *kernel,
                             float diag_scale, const float *dy, int64_t batch, int d, float *dx0,
                             float *dx, float *dkernel, float *dbias, void *workspace,
                             size_t workspace_bytes, void *stream);
/* tfrs_cross_bwd_f16_saved inside a STACK of Cross layers on one x0 (layers/feature_interaction/dcn.py:47-56,
 * "x1 = Cross()(x0, x0); x2 = Cross()(x0, x1)"): dx0 = dy * u + dx0_add, where dx0_add (NULL or [batch, d]) may be dx0
 * itself -- x0's gradient accumulates in place from layer to layer instead of through batch x d additions of the host
 * framework's autograd; add_dx != 0 (the stack's first layer, whose x is x0) folds that layer's dx in as well:
 * dx0 = dy * u + dx0_add + dx. */
int tfrs_cross_bwd_f16_saved_acc(const float *x0, const float *x, const float *u, const float *kernel,
                                 float diag_scale, const float *dy, int64_t batch, int d, const float *dx0_add,
                                 int add_dx, float *dx0, float *dx, float *dkernel, float *dbias, void *workspace,
                                 size_t workspace_bytes, void *stream);
/* Low-rank form (dcn.py:131-148, multi_layer_dcn.py:147-153): a[batch, ka] = x @ U is
 * computed first (tfrs_dense_fwd); this call does  y = x0 * (a @ kernel[ka, d] + bias +
 * diag_scale * x) + x  with the same fused epilogue. */
int tfrs_cross_fwd_ex(const float *x0, const float *x, const float *a, int ka,
                      const float *kernel, const float *bias, float diag_scale,
                      int64_t batch, int d, float *y, void *stream);
/* z = x @ kernel (+bias) only (used for low-rank U/V and activations): out[batch, dout]. */
int tfrs_dense_fwd(const float *x, const float *kernel, const float *bias, int64_t batch,
                   int din, int dout, float *out, void *stream);
/* Gradients of the same Dense (layers/blocks.py:46-61 MLP layers, low-rank Cross projections
 * dcn.py:176-180): dx[batch, din] = dy @ kernel^T, dkernel[din, dout] = x^T @ dy,
 * dbias[dout] = column sums of dy; NULL outputs are skipped.  The transposed operands are read
 * in place.  f16 != 0 selects the split-fp16 MFMA path (large products). */
size_t tfrs_dense_bwd_workspace_bytes(int64_t batch, int din, int dout, int f16);
int tfrs_dense_bwd(const float *x, const float *kernel, const float *dy, int64_t batch, int din,
                   int dout, float *dx, float *dkernel, float *dbias, int f16, void *workspace,
                   size_t workspace_bytes, void *stream);

/* Activations fused into the product's epilogue ("tfrs_cross_fwd(x0, x, w_or_(u,v), b, diag, act,
 * y)"; Keras Dense(activation=...) of layers/blocks.py:46-52 and Cross(preactivation=...) of dcn.py:173-181).
 * Codes: */
#define TFRS_ACT_NONE 0
#define TFRS_ACT_RELU 1
#define TFRS_ACT_SIGMOID 2
#define TFRS_ACT_TANH 3
#define TFRS_ACT_SILU 4   /* swish */
#define TFRS_ACT_GELU 5   /* exact (erf) form, Keras gelu(approximate=False) */
/*   tfrs_dense_fwd_act: out = act(x @ kernel + bias); pre_out (optional, [batch, dout]) receives the
 *     pre-activation.  f16 != 0: split-fp16 MFMA, workspace from tfrs_gemm_f16_workspace_bytes(batch, dout, din).
 *   tfrs_cross_fwd_act: y = x0 * (act(a @ kernel + bias) + diag_scale * x) + x with a[batch, ka] = x (full rank,
 *     ka == d) or x @ U (low rank); pre_out (optional) receives p = a @ kernel + bias.
 *   tfrs_act_pointwise_bwd: the element-wise part of their backward in ONE pass over `count` elements:
 *       dp  = dy * x0 * act'(pre)       (x0 == NULL: dy * act'(pre))            [optional output]
 *       dx0 = dy * (act(pre) + diag_scale * x)                                  [optional output]
 *       dxd = dy * (1 + diag_scale * x0)   (the direct terms of dx)             [optional output]
 *     ref_is_output != 0: `pre` holds y = act(p) (relu / sigmoid / tanh only).
 *   tfrs_dense_bwd_add: tfrs_dense_bwd with dx = dy @ kernel^T + addend[batch, din] (addend may be NULL): with
 *     dy = dp and addend = dxd this is the input gradient of a full-rank Cross layer with a preactivation. */
int tfrs_dense_fwd_act(const float *x, const float *kernel, const float *bias, int64_t batch, int din,
                       int dout, int act, float *out, float *pre_out, int f16, void *workspace,
                       size_t workspace_bytes, void *stream);
int tfrs_cross_fwd_act(const float *x0, const float *x, const float *a, int ka, const float *kernel,
                       const float *bias, float diag_scale, int act, int64_t batch, int d, float *y,
                       float *pre_out, int f16, void *workspace, size_t workspace_bytes, void *stream);
int tfrs_act_pointwise_bwd(int act, int ref_is_output, const float *pre, const float *dy, const float *x0,
                           const float *x, float diag_scale, int64_t count, float *dp, float *dx0,
                           float *dxd, void *stream);
int tfrs_dense_bwd_add(const float *x, const float *kernel, const float *dy, const float *addend,
                       int64_t batch, int din, int dout, float *dx, float *dkernel, float *dbias, int f16,
                       void *workspace, size_t workspace_bytes, void *stream);

/* The same two products on the fp16 matrix cores with split operands (x = hi + lo per
 * power-of-two-scaled row / column; hi*hi + hi*lo + lo*hi with f32 accumulation): f32-grade
 * results at ~3x the rate for large shapes.  The caller provides the workspace that holds the
 * operand images (tfrs_gemm_f16_workspace_bytes(batch, dout, din)). */
size_t tfrs_gemm_f16_workspace_bytes(int64_t m, int n, int k);
int tfrs_dense_fwd_f16(const float *x, const float *kernel, const float *bias, int64_t batch,
                       int din, int dout, float *out, void *workspace, size_t workspace_bytes,
                       void *stream);
int tfrs_cross_fwd_f16(const float *x0, const float *x, const float *kernel, const float *bias,
                       float diag_scale, int64_t batch, int d, float *y, void *workspace,
                       size_t workspace_bytes, void *stream);

/* What the GEMM launchers would choose for the product C[m, n] = A[m, k] @ B[k, n], answered by the functions
 * the launchers themselves call.  Host only, no device work (the layout tests ask it which kernel, which operand
 * preparation and which K slices a shape reaches).  f16: 0 = the f32 MFMA kernel, 1 = the split-fp16 GEMM (which
 * reads TFRS_GEMM16_TILE / TFRS_GEMM16_SPLITK like its launcher).
 *   flags   TFRS_GEMM_PLAN_AT / _BT: the array holds the transpose of A ([k, m]) / of B ([n, k]);
 *           _AMUL / _BMUL: the operand has a fused element-wise multiplier; _EPI: a Cross-type epilogue;
 *           _BIAS: a bias; _ACT: an activation or a pre-activation output.
 *   align   the low four address bits of a | b << 4 | a's multiplier << 8 | b's multiplier << 12.
 *   out     int64[20].  f16 = 1:
 *           [0] 1 = 256 x 256 kernel, 0 = 128 x 128   [1] kp  [2] mp  [3] np  [4] K block of the images (16 or kp)
 *           [5] 256-row slabs of the column pass  [6] slices asked for  [7] K steps of 16 per slice (0: no split)
 *           [8] non-empty slices  [9] K steps of the last slice
 *           [10..14] operand A, [15..19] operand B: kind (0 row-per-wave kernel, 1 column-maximum + column pass,
 *           2 single-pass K-step-major rows, 3 two-pass K-step-major rows), register steps, 8-byte-load form,
 *           waves per four rows (kind 2 only), 16-byte loads (kinds 0, 1, 3).
 *           f16 = 0 (the A^T B product is the one that splits; A^T B^T does not exist: TFRS_EINVAL):
 *           [0] slices asked for  [1] K rows per slice (0: no split)  [2] non-empty slices  [3] K rows of the last
 *           slice  [4] / [5] 16-byte loads of A / B  [6] 128 x 128 output tiles.
 * m, n, k < 1 or an unknown flag: TFRS_EINVAL. */
#define TFRS_GEMM_PLAN_AT 1
#define TFRS_GEMM_PLAN_BT 2
#define TFRS_GEMM_PLAN_AMUL 4
#define TFRS_GEMM_PLAN_BMUL 8
#define TFRS_GEMM_PLAN_EPI 16
#define TFRS_GEMM_PLAN_BIAS 32
#define TFRS_GEMM_PLAN_ACT 64
int tfrs_gemm_plan(int f16, int64_t m, int n, int64_t k, int flags, int align, int64_t *out);

/* ------------------------------------------------------------------------- *
 * Row-sharded embedding lookup, owner bucketing (the multi-device
 * embedding of the reference is TPUEmbedding, layers/embedding/tpu_embedding_layer.py:699-720):
 * rank r owns table rows [r * rows_per_rank, (r + 1) * rows_per_rank).  For n lookups:
 *   counts[o]    (int64, DEVICE) = lookups served by owner o  (the all-to-all split sizes)
 *   send_ids[p]  (int64) shard-local row of the lookup in send slot p, owner by owner, STABLE
 *                within an owner (-1: id outside [0, input_dim) -> zero row, routed to owner 0)
 *   perm[i] = send slot of lookup i;  order[p] = lookup in send slot p   (int32)
 * so the rows that come back are gathered to their final positions through `perm`
 * (tfrs_embedding_gather_fwd with ids = perm) and the gradient rows are laid out for the way
 * back through `order`.  No sort, no host synchronisation, three short launches.
 * ------------------------------------------------------------------------- */
size_t tfrs_shard_route_workspace_bytes(int64_t n, int world);
int tfrs_shard_route_ids(const void *ids, int ids_are_i64, int64_t n, int64_t input_dim,
                         int64_t rows_per_rank, int world, int64_t *send_ids, int32_t *perm,
                         int32_t *order, int64_t *counts, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------------- *
 * DotInteraction.call (layers/feature_interaction/dot_interaction.py:53-104):
 * x[batch, f, d] -> lower-triangle pairwise dots, row-major; self_interaction adds the
 * diagonal; skip_gather emits the full f*f matrix with the upper part zeroed.
 * ------------------------------------------------------------------------- */
int tfrs_dot_interaction_fwd(const float *x, int64_t batch, int f, int d,
                             int self_interaction, int skip_gather, float *out,
                             void *stream);
int tfrs_dot_interaction_bwd(const float *x, const float *dout, int64_t batch, int f,
                             int d, int self_interaction, int skip_gather, float *dx,
                             void *stream);
/* Row-strided variants (packed-triangle output only): sample b's pairs live at out + b * out_stride
 * (dout + b * dout_stride), i.e. inside a wider [batch, out_stride] matrix -- lets the ranking model
 * write / read the block next to the bottom-stack output it is concatenated with
 * (experimental/models/ranking.py:225-232) without concat / slice copies.  The pair covers exactly
 * batch >= 512, d = 16 or 32, f <= 122 with at least one pair, under the default switches (TFRS_DOT_STAGE=0,
 * TFRS_DOT_FWD=staged / f32 and TFRS_DOT_BWD=dense / gather select kernels without a row stride); every other
 * call returns TFRS_ENOTIMPL and writes nothing (fall back to the contiguous calls), also when out_stride
 * equals the pair count.  The forward refuses wherever the backward would, so that a forward can never
 * succeed without its backward; tfrs_dot_interaction_strided_supported answers beforehand. */
int tfrs_dot_interaction_fwd_strided(const float *x, int64_t batch, int f, int d,
                                     int self_interaction, float *out, int64_t out_stride,
                                     void *stream);
int tfrs_dot_interaction_bwd_strided(const float *x, const float *dout, int64_t dout_stride,
                                     int64_t batch, int f, int d, int self_interaction, float *dx,
                                     void *stream);
/* 1 when BOTH strided entry points cover (batch, f, d): callers ask before they take the fused
 * concat path, so a forward can never succeed where its backward would return TFRS_ENOTIMPL. */
int tfrs_dot_interaction_strided_supported(int64_t batch, int f, int d, int self_interaction);

/* What the DotInteraction entry points would launch at a shape, answered by the decision function the
 * launchers themselves switch on (DESIGN.md section 2 has the table).  Host only, no device work; reads
 * TFRS_DOT_STAGE, TFRS_DOT_FWD, TFRS_DOT_BWD (and TFRS_DOT_FWD_GRID) as the launchers do.  strided = 1: the
 * tfrs_dot_interaction_*_strided pair (no skip_gather: TFRS_EINVAL).
 *   out   int64[32]: the forward route in [0..15], the backward route in [16..31], each
 *         [0] kernel (TFRS_DOT_KERNEL_*)   [1] DP  [2] NB  [3] STAGE  [4] BLOCKS  [5] NFB  [6] MAXE
 *         [7] NSTEP  [8] NEY  [9] NSET  (template arguments; 0 where the kernel has no such argument)
 *         [10] workgroups  [11] threads per workgroup  [12] dynamic LDS bytes
 *         [13] the dynamic LDS limit the launcher requests for the kernel (0: it requests none)
 *         [14] half width of the backward's S tile (dense, producer / consumer)
 *         [15] h16 backward: L words per buffer; fallback backward: samples per workgroup (4, 2 or 1).
 * Forward TFRS_DOT_KERNEL_REFUSED (TFRS_ENOTIMPL from the entry point) is exactly
 *   (f > 128 or d > 128 or ceil(f / 32) * DP / 2 > 128) and f * (d + 1) > 4096,   DP = d rounded up to 8, 16, 32, 64, 128;
 * the backward refuses only f * d > 16384 outside f, d <= 128.  TFRS_DOT_KERNEL_NONE: no pairs (f = 1 without
 * self interaction) -- the forward launches nothing (out may be NULL), the backward writes dx = 0 (dout may be NULL).
 * tfrs_dot_interaction_plan_many: n rows of (batch, f, d, self_interaction, skip_gather, strided) -> n rows of
 * int64[32], under one reading of the switches.  A shape below 1: TFRS_EINVAL. */
#define TFRS_DOT_KERNEL_REFUSED 0
#define TFRS_DOT_KERNEL_NONE 1
#define TFRS_DOT_KERNEL_GATHER 2        /* dot_interaction_fwd_kernel / dot_interaction_bwd_kernel (fallback) */
#define TFRS_DOT_KERNEL_MFMA_STAGED 3   /* dot_interaction_mfma_kernel<DP, NB, true> */
#define TFRS_DOT_KERNEL_MFMA_DIRECT 4   /* dot_interaction_mfma_kernel<DP, NB, false> */
#define TFRS_DOT_KERNEL_F16X3 5         /* dot_interaction_f16x3_kernel<DP, NB> */
#define TFRS_DOT_KERNEL_F16X3_DIRECT 6  /* dot_interaction_f16x3_direct_kernel<DP, NB, BLOCKS> */
#define TFRS_DOT_KERNEL_FWD_PC 7        /* dot_interaction_fwd_pc_kernel<NB, NSET> */
#define TFRS_DOT_KERNEL_BWD_MFMA 8      /* dot_interaction_bwd_mfma_kernel<DP, NB> */
#define TFRS_DOT_KERNEL_BWD_DENSE 9     /* dot_interaction_bwd_dense_kernel<NFB, MAXE> */
#define TFRS_DOT_KERNEL_BWD_PC 10       /* dot_interaction_bwd_pc_kernel<MAXE> */
#define TFRS_DOT_KERNEL_BWD_H16 11      /* dot_interaction_bwd_h16_kernel<NSTEP, NEY, NSET> */
int tfrs_dot_interaction_plan(int64_t batch, int f, int d, int self_interaction, int skip_gather, int strided,
                              int64_t *out);
int tfrs_dot_interaction_plan_many(int64_t n, const int64_t *shapes, int64_t *out);

/* ------------------------------------------------------------------------- *
 * ScaNN search (layers/factorized_top_k.py:613-796; csrc/scann.hip): partitioned, product-quantized approximate
 * top-K for ONE chunk of nq queries.  The caller has run the leaf pass (exact top-l_eff of q . mu over the leaf
 * centres: probes[nq, l_eff] leaf numbers, leaf_scores[nq, l_eff] their f32 fma-chain scores) and holds the index:
 *   leaf_offsets[num_leaves + 1] (int64): leaf l is positions leaf_offsets[l] .. leaf_offsets[l + 1] of the
 *     leaf-major order, perm[position] (int32) is the original row; max_leaf_rows = largest leaf (host value);
 *   codes[(n + 128) * code_bytes]: 4-bit code of block b (dims b * dims_per_block ..) in the low (b even) / high
 *     (b odd) nibble of byte b / 2 of the position's code row; the last 128 rows are padding (read, never used);
 *     code_bytes is a multiple of 4, at most 64;
 *   lut: fp16 [dp][16], dp = d rounded up to 16: codebook value of dimension i under code c, times 2^lut_exp
 *     (zero for i >= d);
 *   rows[n, d] (f32, leaf-major) or NULL: with rows the top-r candidates are re-scored exactly.
 * p_max >= every query's probed rows P_b = sum of its l_eff leaf sizes; the workspace holds an [nq, p_max] score
 * buffer.  Results out_scores / out_rows [nq, k], (score desc, original row asc): with rows, the scores are the
 * d-ordered f32 fma chain (== BruteForce, oracle/topk.py scores) of the best k of the top min(r, p_max)
 * approximate candidates; without, the approximate scores s~ of the top k.
 *
 * Approximate score of row x of leaf l (decoded residual r^ = the codebook values of its codes):
 *   s~ = (sum_i fp16(q_i 2^eq) fp16(r^_i 2^lut_exp), f32 MFMA accumulation) * 2^-(eq + lut_exp) + (q . mu_l)_f32,
 * where 2^eq puts max|q| into [2^13, 2^14) and 2^lut_exp does the same for the largest codebook value |C|max
 * (the caller's choice), so no finite input overflows fp16 and what flushes is below 2^-38 of the maximum.  Against
 * the float64 value s = sum_i q_i (mu_i + r^_i) of the same decoded vector:
 *   |s~ - s| <= 2^-9 * sum_i |q_i| (|mu_i| + |r^_i|) + 2^-32 * d * max|q| * |C|max
 * (2^-10 + 2^-22 for the two fp16 roundings, (d + 10) 2^-24 for the f32 sums, d 2^-37 max|q| |C|max for flushes).
 * Rows are distinct within a query; columns past P_b never appear ahead of probed rows.
 * tfrs_scann_search_workspace_bytes is 0 when any argument is below 1 (a call with nq = 0 needs no workspace).
 * ------------------------------------------------------------------------- */
size_t tfrs_scann_search_workspace_bytes(int64_t nq, int num_leaves, int l_eff, int d, int64_t p_max, int r);
int tfrs_scann_search(const float *queries, int64_t nq, int d, const int32_t *probes, const float *leaf_scores,
                      int l_eff, const int64_t *leaf_offsets, int num_leaves, int64_t max_leaf_rows,
                      const uint8_t *codes, int code_bytes, const void *lut, int dims_per_block, int lut_exp,
                      const int32_t *perm, const float *rows, int64_t p_max, int r, int k, float *out_scores,
                      int32_t *out_rows, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 * The recurrence of a Keras GRU (reset_after=True, tanh / sigmoid, gates z, r, h) over all `steps` time steps in
 * ONE launch, and its backward walk in one more (layers/recurrent.py).  The input projection
 * xproj[batch, steps, 3 units] = x @ kernel + bias[0] and every weight gradient are GEMMs of tfrs_dense_*.
 *   q = h_{t-1} @ recurrent_kernel[units, 3 units] + recurrent_bias[3 units] (NULL: none)
 *   z = sigmoid(a_z + q_z), r = sigmoid(a_r + q_r), hh = tanh(a_h + r q_h), h_t = z h_{t-1} + (1 - z) hh
 * mask[batch, steps] (bytes, NULL: all set): where 0, h_t = h_{t-1}.  h0[batch, units] (NULL: zeros).
 * go_backwards != 0 walks time indices steps-1 .. 0.  out_seq[batch, steps, units] (optional) is in PROCESSING
 * order; out_last[batch, units].  The training forward also fills save_z / save_r / save_hh / save_qh / save_hprev
 * [batch, steps, units], indexed by TIME index (all five or none).
 *   bwd: dseq (processing order) and dlast are the gradients of out_seq / out_last (each optional);
 *     da[batch, steps, 3 units] = (da_z, da_r, da_h), the gradient of xproj;
 *     dg[batch, steps, 3 units] = (da_z, da_r, dq_h): d recurrent_kernel = save_hprev^T @ dg, d recurrent_bias its
 *     column sums; both by time index, zeros at masked steps; dh0[batch, units].
 * units <= TFRS_GRU_MAX_UNITS (TFRS_ENOTIMPL above).  batch == 0 or steps == 0 returns without a launch.  No
 * workspace, no atomics: results are identical from run to run.
 * ------------------------------------------------------------------------- */
#define TFRS_GRU_MAX_UNITS 64
int tfrs_gru_fwd(const float *xproj, const float *recurrent_kernel, const float *recurrent_bias,
                 const uint8_t *mask, const float *h0, int64_t batch, int steps, int units, int go_backwards,
                 float *out_seq, float *out_last, float *save_z, float *save_r, float *save_hh, float *save_qh,
                 float *save_hprev, void *stream);
int tfrs_gru_bwd(const float *recurrent_kernel, const uint8_t *mask, const float *save_z, const float *save_r,
                 const float *save_hh, const float *save_qh, const float *save_hprev, const float *dseq,
                 const float *dlast, int64_t batch, int steps, int units, int go_backwards, float *da, float *dg,
                 float *dh0, void *stream);

/* ------------------------------------------------------------------------- *
 * Numeric preprocessing (layers/numeric.py; csrc/numeric.hip): the kernels behind Discretization and
 * Normalization.  Plain pointers, every launch on `stream`, no atomics, no host synchronisation, no allocation.  The
 * input x is f32, f64, int32 or int64 (TFRS_NUMERIC_*).  Bad arguments (a NULL pointer, a negative count, an unknown
 * dtype code or mode, a workspace smaller than stated, an input not aligned to its element size) return TFRS_EINVAL
 * with nothing launched; n == 0 / n_rows == 0 returns TFRS_OK with nothing launched.
 *
 * tfrs_bucketize: out[i] = the number of boundaries <= x[i] (std::upper_bound, np.searchsorted(side="right")), as
 *   TensorFlow's Bucketize kernel computes it: the nb boundaries are f32; f32 input is compared in f32; int32 and
 *   int64 input is converted to f32 with round-to-nearest-even and compared in f32; f64 input is compared in f64
 *   against the widened boundaries.  NaN goes to bucket nb; nb == 0 gives zeros; repeated boundaries are legal.  The
 *   entry does NOT check that the boundaries are sorted (non-decreasing, no NaN): unsorted boundaries give some index
 *   in [0, nb], never a fault.  Up to TFRS_BUCKETIZE_LDS_BOUNDARIES boundaries each workgroup stages them in LDS;
 *   beyond, the same branch-free search probes global memory.
 *
 * tfrs_normalize: x[n_rows, f] row-major, mean[f], scale[f]; x is converted to f32 first.  f == 1 is one scalar
 *   statistic over any shape (axis=None).  mode
 *     TFRS_NORMALIZE_FORWARD          out = (x - mean) / scale   an IEEE subtraction, then an IEEE division
 *     TFRS_NORMALIZE_INVERT           out = fma(x, scale, mean)
 *     TFRS_NORMALIZE_BACKWARD         out = x / scale            x is the gradient of the forward's output
 *     TFRS_NORMALIZE_BACKWARD | TFRS_NORMALIZE_INVERT   out = x * scale   ... of the inverted layer's output
 *
 * Moments.  state[f][3] (f64, on the device): per feature the count, the mean and M2, the sum of squared deviations
 *   from that mean, of everything seen since tfrs_moments_reset (which writes zeros).  tfrs_moments_update folds the
 *   batch x[n_rows, f] in: the values are converted to f32 (the statistics are those of the f32 values) and
 *   accumulated in f64 in two launches -- workgroups of TFRS_MOMENTS_SLICE_ELEMENTS / f rows (more once
 *   TFRS_MOMENTS_MAX_GROUPS workgroups no longer cover the batch) each write one partial per feature into the
 *   workspace, one workgroup merges them into the state with Chan's pairwise update in an order the shape fixes, so
 *   the state is bit-identical from run to run.  workspace: tfrs_moments_workspace_bytes(n_rows, f) bytes, 8-byte
 *   aligned; the size never decreases in either argument, so one workspace sized for the largest batch serves all.
 *   tfrs_moments_finalize writes f32 mean[f], variance[f] = M2 / count (population) and
 *   scale[f] = max(sqrt(variance), TFRS_NORMALIZE_EPSILON); a feature with count 0 gets mean 0, variance 1, scale 1
 *   (Keras' reset values).  Constant data gives variance exactly 0.
 * ------------------------------------------------------------------------- */
#define TFRS_NUMERIC_F32 0
#define TFRS_NUMERIC_F64 1
#define TFRS_NUMERIC_I32 2
#define TFRS_NUMERIC_I64 3
#define TFRS_BUCKETIZE_LDS_BOUNDARIES 4095   /* padded to 4096 f32 = 16 KB of LDS */
#define TFRS_NORMALIZE_FORWARD 0
#define TFRS_NORMALIZE_INVERT 1
#define TFRS_NORMALIZE_BACKWARD 2
#define TFRS_NORMALIZE_EPSILON 1e-7f         /* Keras backend.epsilon() */
#define TFRS_MOMENTS_SLICE_ELEMENTS 4096
#define TFRS_MOMENTS_MAX_GROUPS 1024
int tfrs_bucketize(const void *x, int dtype, int64_t n, const float *boundaries, int64_t nb, int64_t *out,
                   void *stream);
int tfrs_normalize(const void *x, int dtype, int64_t n_rows, int64_t f, const float *mean, const float *scale,
                   int mode, float *out, void *stream);
size_t tfrs_moments_workspace_bytes(int64_t n_rows, int64_t f);
int tfrs_moments_update(const void *x, int dtype, int64_t n_rows, int64_t f, double *state, void *workspace,
                        size_t workspace_bytes, void *stream);
int tfrs_moments_finalize(const double *state, int64_t f, float *mean, float *variance, float *scale, void *stream);
int tfrs_moments_reset(double *state, int64_t f, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TFRS_HIP_H_ */
