/*
 * include/rtrec_amd_ext.h -- the EXTENSION surface of librtrec_amd.so: entry points without a counterpart in the reference.
 *
 * include/rtrec_amd.h stands in for the method set of the reference's SLIMElastic and stays exactly that.  Calls the
 * reference has no form of at all live here, under the same discipline: the comment is the contract, every pointer named
 * d_* is a device pointer, nothing allocates, frees or synchronises, `stream` is a hipStream_t passed as void*, the return
 * value is 0 or a negative rtrec_status, and the library keeps no state and reads no environment variable.  The symbols are
 * compiled into the same librtrec_amd.so; rtrec_amd/_native.py lists them in EXT_EXPORTS, rtrec_amd/ops.py in EXT_OPS.
 */
#ifndef RTREC_AMD_EXT_H
#define RTREC_AMD_EXT_H

#include "rtrec_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * DIVERSIFIED LISTS  (greedy maximal-marginal-relevance re-rank; W is the item-item similarity.)
 * Every list served so far is ranked by score alone, so a SLIM top-10 tends to be ten neighbours of the two or three items
 * the user rated.  This call re-ranks a list by trading the score against the similarity to what already stands above.
 * Row r brings list_k positions (1..1024): item ids d_ids[r * ids_stride + p] and float32 base scores
 * d_scores[r * scores_stride + p] (both strides >= list_k), valid up to d_counts[r] (clamped to [0, list_k]).  W is given in
 * CSC form d_wc_* (d_wc_ptr[n_items + 1], rows ascending and distinct per column, float32 values; wc_nnz = length of
 * d_wc_row / d_wc_val) -- the operand of rtrec_slim_similar_topk, rtrec_slim_explain_topk and rtrec_slim_score_pairs.
 * Offsets are clamped to [0, wc_nnz], so a malformed matrix gives wrong answers, never an out-of-range read.
 *   competing   a position competes when p < counts[r], 0 <= id < n_items, its score is finite, and no earlier-chosen
 *               position holds the same item id (a diversified list never shows an item twice; duplicates only occur in
 *               lists a caller brings)
 *   similarity  for a != b: sim(a, b) = fmaxf(|W[a,b]|, |W[b,a]|), where W[j,i] is the value stored at row j of column i, or 0
 *               if none is stored; a NaN weight is ignored (fmaxf's rule).  Symmetric, non-negative, exact; a negative weight
 *               counts by its magnitude
 *   selection   pen[p] = +0.0f for every position, oml = fl(1.0f - lambda).  For t = 0 .. keep-1: every competing, unchosen
 *               position has the value v[p] = fl(fl(lambda * score[p]) - fl(oml * pen[p])): three separately rounded
 *               operations, never fused.  p beats q if v[p] > v[q], or v[p] == v[q] and p < q (lists arrive best first, so the
 *               EARLIER position wins; -0.0 == +0.0 is a tie).  A position whose v is NaN is skipped in that step; if no
 *               position has a v that is a number, the list ends.  The winner c is recorded, and every other competing
 *               position gets pen[p] = fmaxf(pen[p], sim(id[p], id[c]))
 * Out: d_out_order[n_rows][keep] holds list POSITIONS (not item ids: the caller gathers, as with rtrec_slim_score_pairs),
 * d_out_value[n_rows][keep] v at the moment of choice, d_out_penalty[n_rows][keep] pen at the moment of choice (how similar the
 * entry is to what stands above it), d_out_count[r] the number chosen; behind it -1 / -inf / -inf.  Every slot is written.
 * Consequences: with lambda == 1, v == score exactly, so a list sorted by score descending comes back as positions
 * 0 .. count-1; step 0 always has pen == 0.
 * list_k in 1..1024, keep in 1..list_k and waves_per_row in {0, 1, 4} (1 or 4 waves of 64 threads per row, 0 = chosen by the
 * library): RTREC_ERR_UNSUPPORTED otherwise.  lambda outside [0, 1] or NaN, NULL arrays, negative sizes and a stride below
 * list_k: RTREC_ERR_INVALID_ARG.  n_rows == 0: RTREC_OK before any pointer check.  No global state, no environment variable, no
 * allocation.  The results never depend on waves_per_row, on the grid size or on scheduling.
 * csrc/diversify.hip, diversify_lists_kernel: one row per workgroup; ids, lambda * score and penalties in LDS; per step an
 * arg-max under the strict order above, then two binary searches per position (the winner's column is staged in LDS up to
 * 128 entries and searched in global memory beyond that, so a column of any length works).
 * ------------------------------------------------------------------------------------- */
int rtrec_slim_diversify_lists(int32_t n_rows, int32_t n_items, const int32_t *d_wc_ptr, const int32_t *d_wc_row,
                               const float *d_wc_val, int64_t wc_nnz, const int32_t *d_ids, int64_t ids_stride,
                               const float *d_scores, int64_t scores_stride, int32_t list_k, const int32_t *d_counts,
                               int32_t keep, float lambda, int32_t waves_per_row, int32_t *d_out_order, float *d_out_value,
                               float *d_out_penalty, int32_t *d_out_count, void *stream);

/* ---------------------------------------------------------------------------------------
 * LIST QUALITY  (per list: intra-list similarity, linked pairs, a weight sum; over all lists: the catalogue exposure.)
 * The stage above ships a knob; this call measures what a value of it buys, on the lists where the scoring kernels and
 * rtrec_slim_diversify_lists leave them.  Row r brings list_k positions (1..1024): item ids d_ids[r * ids_stride + p]
 * (ids_stride >= list_k), valid up to d_counts[r] (clamped to [0, list_k]).  W is given in CSC form d_wc_* exactly as for
 * rtrec_slim_diversify_lists (d_wc_ptr[n_items + 1], rows ascending and distinct per column, float32 values; wc_nnz = length
 * of d_wc_row / d_wc_val).  Offsets are clamped to [0, wc_nnz], so a malformed matrix gives wrong answers, never an
 * out-of-range read.  d_item_weight[n_items] (float32) and d_exposure[n_items] (int32) may each be NULL.
 *   counted     position p is counted when p < counts[r], 0 <= id < n_items, and no earlier counted position of the row holds
 *               the same id: an item shown twice is judged once, at its first place.  m = the number of counted positions
 *   similarity  rtrec_slim_diversify_lists's: for a != b, sim(a, b) = fmaxf(|W[a,b]|, |W[b,a]|), 0 where nothing is stored; a
 *               NaN weight is ignored, so sim is never NaN and never negative; a stored inf gives inf
 *   sim_sum     a two-level float32 sum, never fused.  For each counted p in ascending order, s_p = the sum from +0.0f of
 *               sim(id_p, id_q) over the counted q < p in ascending q, one rounded add each; sim_sum = the sum from +0.0f of the
 *               s_p in ascending p, one rounded add each.  (Each s_p is a chain of at most p adds and the chains are independent
 *               of each other; one chain over all pairs would be about 500,000 dependent adds for a list of 1,024.)
 *   linked      the number of counted pairs q < p with sim > 0 (int32); a pair whose only stored weights are explicit zeros is
 *               not linked
 *   weight_sum  the sum from +0.0f of d_item_weight[id_p] over the counted p in ascending order, one rounded add each; +0.0f
 *               when d_item_weight is NULL.  The kernel knows nothing about what the weight means
 *   exposure    every counted position adds 1 to d_exposure[id] with an integer atomic when d_exposure is not NULL.  The array
 *               is never zeroed here, so a caller accumulates over several calls; integer adds commute, so the result does not
 *               depend on scheduling
 * Out, every slot written for every row (rows with m = 0 included): d_out_n[r] = m (int32), d_out_sim_sum[r] (float32),
 * d_out_linked[r] (int32), d_out_weight_sum[r] (float32).
 * list_k in 1..1024 and waves_per_row in {0, 1, 4} (1 or 4 waves of 64 threads per row, 0 = chosen by the library):
 * RTREC_ERR_UNSUPPORTED otherwise.  NULL required arrays, negative sizes and ids_stride < list_k: RTREC_ERR_INVALID_ARG.
 * n_rows == 0: RTREC_OK before any pointer check.  No global state, no environment variable, no allocation, no
 * synchronisation.  The results never depend on waves_per_row, on the grid size or on scheduling.
 * csrc/list_quality.hip, list_quality_kernel: one row per workgroup; ids and the spans of their columns in LDS; every position
 * looks for its id at a lower position, then its owner walks the counted positions below it with two binary searches each,
 * and one thread adds the per-position figures in order.
 * ------------------------------------------------------------------------------------- */
int rtrec_slim_list_quality(int32_t n_rows, int32_t n_items, const int32_t *d_wc_ptr, const int32_t *d_wc_row,
                            const float *d_wc_val, int64_t wc_nnz, const int32_t *d_ids, int64_t ids_stride, int32_t list_k,
                            const int32_t *d_counts, const float *d_item_weight, int32_t *d_exposure, int32_t waves_per_row,
                            int32_t *d_out_n, float *d_out_sim_sum, int32_t *d_out_linked, float *d_out_weight_sum,
                            void *stream);

/* ---------------------------------------------------------------------------------------
 * CATALOGUE RANKS  (at which position of the whole catalogue does a held-out item stand: counts, no sort.)
 * Row r brings a dense score vector d_scores[r * scores_stride + c], c in [0, n_items), scores_stride >= n_items (what lies
 * beyond n_items is never read): float32, or float64 when scores_f64 != 0 -- the rows rtrec_slim_score_rows writes, the bits
 * the top-k kernels rank by.  The interaction rows used for filtering are a CSR without values: d_row_ids[r] (NULL: row r)
 * names the row of d_xb_ptr[n_x_rows + 1] / d_xb_col[xb_nnz], columns ascending inside a row as everywhere on this surface.
 * The targets are a CSR over the rows: d_tg_ptr[n_rows + 1] (int64, non-decreasing; every offset is clamped to [0, n_tg])
 * into d_tg_items[n_tg] (int32).  The targets of a row may come in any order and may repeat.
 *   own          only when filter_interacted != 0: the columns stored in X's row, whatever their value, each once (an equal
 *                neighbour is the same column); a row id outside [0, n_x_rows) gives the empty set; offsets are clamped to
 *                [0, xb_nnz]; columns outside [0, n_items) are ignored
 *   competes(c)  s[c] is not NaN, c is not in own, and mode == RTREC_TOPK_DENSE or s[c] != 0 (-0.0 counts as zero): the
 *                competition rule of the top-k kernels for the same mode and filter_interacted
 *   target t with item i, i in [0, n_items) and competes(i):
 *                above[t] = the number of c != i with competes(c) and s[c] > s[i]
 *                tied[t]  = the number of c != i with competes(c) and s[c] == s[i]   (+0.0 == -0.0; +-inf compare as numbers)
 *                otherwise above[t] = -1 and tied[t] = 0: the item can never be listed.  The other targets of the row compete
 *                like any column; a caller subtracts them where a metric wants that
 *   score[t]     (double) s[i] when i is in range -- also for an item that does not compete -- else -inf
 *   competing[r] the number of c with competes(c)
 * CONSEQUENCE: with finite scores, tied == 0 and 0 <= above < K, the list of K entries the top-k kernels produce for the same
 * row, mode and filter_interacted holds item i at position `above`; with ties it holds i somewhere in positions
 * above .. above + tied (as far as the list reaches).
 * Out, every slot written: d_out_above[n_tg], d_out_tied[n_tg] (int32), d_out_score[n_tg] (float64), d_out_competing[n_rows]
 * (int32); a slot in front of d_tg_ptr[0] or behind d_tg_ptr[n_rows] gets -1 / 0 / -inf.  A d_tg_ptr that is not
 * non-decreasing gives wrong answers, never an out-of-range access.
 * mode other than RTREC_TOPK_SPARSE / RTREC_TOPK_DENSE: RTREC_ERR_UNSUPPORTED.  NULL required arrays (d_xb_* are required
 * only with filter_interacted, the per-target arrays only with n_tg > 0), negative sizes and scores_stride < n_items:
 * RTREC_ERR_INVALID_ARG.  n_rows == 0: RTREC_OK before any pointer check.  No global state, no environment variable, no
 * allocation, no synchronisation.  The results never depend on the grid size, on the number of targets taken per sweep or on
 * scheduling: they are integer counts and copies.
 * csrc/catalogue_ranks.hip, catalogue_ranks_kernel: one row per workgroup of four waves (grid-stride beyond 2,048 workgroups);
 * the row is swept once per group of up to 8 targets with 16-byte loads and integer counters in registers; own is taken back
 * by walking the stored row; no atomics.
 * ------------------------------------------------------------------------------------- */
int rtrec_slim_catalogue_ranks(int32_t n_rows, int32_t n_items, const void *d_scores, int64_t scores_stride, int32_t scores_f64,
                               const int32_t *d_row_ids, const int32_t *d_xb_ptr, const int32_t *d_xb_col, int32_t n_x_rows,
                               int64_t xb_nnz, int32_t filter_interacted, int32_t mode, const int64_t *d_tg_ptr,
                               const int32_t *d_tg_items, int64_t n_tg, int32_t *d_out_above, int32_t *d_out_tied,
                               double *d_out_score, int32_t *d_out_competing, void *stream);

/* ---------------------------------------------------------------------------------------
 * BLENDED LISTS  (the union of two per-row lists by item id: each min-max normalised, the second weighted per item, re-ranked.)
 * The reference's hybrid model merges SLIM's list with a second scorer's in Python, one user at a time over dicts
 * (HybridSlimFM._ensemble_by_scores); this call takes both lists where they lie.  List A is the other scorer's, list B SLIM's;
 * both arrive best first.  Row r brings ka positions of A (1..1024): item ids d_a_ids[r * a_ids_stride + p] and float32 scores
 * d_a_scores[r * a_scores_stride + p] (both strides >= ka), valid up to d_a_counts[r] (clamped to [0, ka]); and kb positions of
 * B in the same form.  With weight_mode == RTREC_BLEND_CONTACTS the row of the interaction matrix behind list r is
 * d_row_ids[r] (NULL: row r) of the CSR without values d_xb_ptr[n_x_rows + 1] / d_xb_col[xb_nnz], and the optional count CSR
 * d_cn_ptr[n_x_rows + 1] / d_cn_col[cn_nnz] / d_cn_val[cn_nnz] (all int32; d_cn_ptr may be NULL) stores how often a user
 * touched an item; columns ascend inside a row in both.  Offsets are clamped to [0, xb_nnz] / [0, cn_nnz], so a malformed CSR
 * gives wrong answers, never an out-of-range read.  With RTREC_BLEND_CONSTANT none of d_row_ids, d_xb_*, d_cn_* is read.
 *   length      a list is cut at its first position that lies behind its count, whose id is outside [0, n_items), or whose
 *               score is not finite or is <= -FLT_MAX (the reference's cut for what its top-k filtered out).  na and nb are
 *               what remains; an empty list contributes nothing
 *   norm        per non-empty list over its effective positions: mn / mx = the least / largest score,
 *               den = fl(fl(mx - mn) + 1e-8f), norm[p] = fl(fl(s[p] - mn) / den); the division is correctly rounded IEEE, float32
 *               denormals are kept.  A list whose scores are all equal normalises to zeros; mx - mn may overflow (norm is then 0
 *               or NaN by IEEE rules)
 *   weight      of a B position with item i.  RTREC_BLEND_CONSTANT: w = weight_b.  RTREC_BLEND_CONTACTS: n = the count stored for
 *               (row, i) in the count CSR (the first of equal columns); if the pair is not stored there -- or d_cn_ptr is NULL --
 *               n = 1 if X's row stores i, else 0; w = (float)((2.0 * (double)n) / ((double)n + k)), float64 left to right,
 *               rounded once to float32; n <= 0 gives +0.0f.  A row id outside [0, n_x_rows) is an empty row: every w is 0
 *   union       the entries stand in this order: first the distinct ids of A in order of first appearance -- an id repeated
 *               inside A stands at its first position and carries the normalised score of its LAST one (the reference's
 *               dict(zip(ids, scores))) -- then the ids only B holds, in order of first appearance in B, each starting from +0.0f.
 *               Then for q = 0 .. nb-1 ascending: term = fl(w * normB[q]) and the value of the entry of B's id at q becomes
 *               fl(value + term): separately rounded, never fused; an id repeated inside B adds once per occurrence
 *   mnz         mnz != 0: the value of an entry that stands in both lists is doubled once at the end (CombMNZ on the normalised
 *               scores; mnz == 0 is the reference's hybrid, the plain sum)
 *   order       an entry beats another if its value is larger, or the values are == (-0.0 == +0.0) and it stands earlier in the
 *               union: a stable descending sort.  An entry whose value is NaN is never listed
 * Out, every slot written: d_out_ids[n_rows][keep] item ids, d_out_value[n_rows][keep] their values (float32; the sign of a zero
 * is not part of the contract), d_out_source[n_rows][keep] (int32: 1 = only A holds the item, 2 = only B, 3 = both),
 * d_out_count[r] the number listed = min(keep, the entries whose value is a number); behind it -1 / -inf / 0.
 * ka and kb in 1..1024, keep in 1..ka+kb, waves_per_row in {0, 1, 4} (1 or 4 waves of 64 threads per row, 0 = chosen by the
 * library, by the rule of rtrec_slim_score_pairs on the longer list) and weight_mode one of the two above: RTREC_ERR_UNSUPPORTED
 * otherwise.  NULL required arrays (d_xb_* only with RTREC_BLEND_CONTACTS; d_cn_col / d_cn_val only with a d_cn_ptr and
 * cn_nnz > 0), negative sizes, a stride below its list length, and a weight_b or k that is negative or NaN:
 * RTREC_ERR_INVALID_ARG.  n_rows == 0: RTREC_OK before any pointer check.  No global state, no environment variable, no
 * allocation, no synchronisation.  The results never depend on waves_per_row, on the grid size or on scheduling.
 * csrc/blend.hip, blend_lists_kernel: one row per workgroup; both lists, their normalised values and the union (up to 2,048
 * entries) in LDS; lengths and extremes by a reduction; every position looks for its id at the other positions, the owner of an
 * entry adds its B terms in ascending q (two binary searches per entry of B for the contacts); ranks by counting; no atomics.
 * ------------------------------------------------------------------------------------- */
#define RTREC_BLEND_CONSTANT 0
#define RTREC_BLEND_CONTACTS 1
int rtrec_slim_blend_lists(int32_t n_rows, int32_t n_items, const int32_t *d_a_ids, int64_t a_ids_stride, const float *d_a_scores,
                           int64_t a_scores_stride, const int32_t *d_a_counts, int32_t ka, const int32_t *d_b_ids,
                           int64_t b_ids_stride, const float *d_b_scores, int64_t b_scores_stride, const int32_t *d_b_counts,
                           int32_t kb, int32_t keep, float weight_b, int32_t weight_mode, double k, int32_t mnz,
                           const int32_t *d_row_ids, const int32_t *d_xb_ptr, const int32_t *d_xb_col, int32_t n_x_rows,
                           int64_t xb_nnz, const int32_t *d_cn_ptr, const int32_t *d_cn_col, const int32_t *d_cn_val,
                           int64_t cn_nnz, int32_t waves_per_row, int32_t *d_out_ids, float *d_out_value, int32_t *d_out_source,
                           int32_t *d_out_count, void *stream);

/* ---------------------------------------------------------------------------------------
 * FACTOR TOP-K  (dense user vectors against dense item vectors: the best top_k items per job, scored and selected in one pass.)
 * The reference's hybrid model takes its second list from implicit.topk(items=item_vector, query=user_vector, k,
 * filter_query_items) (rtrec/models/hybrid.py): a float32 GEMM and a top-k per row with the interacted items filtered.  This
 * call does that for vectors the caller brings, or for the ones rtrec_factor_gram / rtrec_factor_als_solve below have trained.
 *   vectors     job r names row x = d_row_ids[r] of X (d_row_ids == NULL: x = r).  Its vector is row d_p_index[x] of
 *               d_p[n_p_rows][p_stride] (d_p_index == NULL: row x); d_p_index holds n_x_rows entries.  A job has no vector when x
 *               lies outside [0, n_x_rows), when its index is -1, or when its index lies outside [0, n_p_rows): it returns an
 *               empty list.  Item vectors are stored component-major: component c of item i is d_qt[c * qt_stride + i],
 *               qt_stride >= n_items (32 neighbouring items are one contiguous read per component)
 *   score       s = +0.0f, then for c = 0 .. dim-1 ascending s = fmaf(p[c], q[c], s): one correctly rounded fused multiply-add
 *               per component, float32 denormals kept, nothing else added.  Biases are components the caller stacks
 *               ([b_u, 1, e...] . [1, b_i, e...], as the reference does).  The sign of a zero score is not part of the contract
 *   competing   item i competes when 0 <= i < n_items; d_item_mask == NULL or d_item_mask[i] != 0; filter_interacted == 0 or i is
 *               not stored in row x of the CSR without values d_xb_ptr[n_x_rows + 1] / d_xb_col[xb_nnz] (columns ascend inside a
 *               row; offsets are clamped to [0, xb_nnz], so a malformed CSR gives wrong answers, never an out-of-range read);
 *               and its score is not NaN.  +-inf compete as numbers
 *   order       the larger score first; among == scores (-0.0 == +0.0) the lower item id.  Strict, so a list is unique
 * Out, every slot written: d_out_ids[n_rows][top_k] / d_out_scores[n_rows][top_k], behind the list -1 / -inf;
 * d_out_count[r] = min(top_k, competing items).
 * item_splits cuts the catalogue into that many chunks of whole 32-item tiles (never more chunks than tiles), each scanned by
 * its own workgroups, and a second kernel merges the chunks' lists under the same order: it is what lets a request of one job
 * use more than one CU.  Chunked calls keep their partial lists in d_workspace:
 * RTREC_FACTOR_TOPK_WORKSPACE_BYTES(n_rows, top_k, item_splits) bytes for item_splits > 1, none for 1.  With item_splits == 0
 * the library chooses (from n_rows: chunks until about four workgroups per CU exist) and lowers its choice to what the
 * workspace it was handed holds; without a workspace it is 1.  (The size is a macro, not an entry point: every symbol of this
 * header launches and stands behind exactly one op.)
 * dim in 1..256, top_k in 1..128, item_splits in 0..64: RTREC_ERR_UNSUPPORTED otherwise.  NULL required arrays (d_xb_* only with
 * filter_interacted; d_workspace only with item_splits > 1), negative sizes and strides below their widths:
 * RTREC_ERR_INVALID_ARG.  A workspace too small for an explicit item_splits: RTREC_ERR_WORKSPACE.  n_rows == 0: RTREC_OK before
 * any pointer check.  No global state, no environment variable, no allocation, no synchronisation.  The results never depend on
 * item_splits, on the grid or on scheduling.
 * csrc/factor_topk.hip, factor_topk_kernel: 32 jobs x one chunk per one-wave workgroup; a 32 x 32 tile of scores is one chain of
 * v_mfma_f32_32x32x2_f32 over ascending components (items the A operand, read straight from d_qt; the jobs' vectors the B
 * operand, in registers), which is that fmaf chain bit for bit; scores that cannot beat a job's threshold are dropped in
 * registers, survivors are checked against the mask and the row of X and appended to the job's buffer in LDS, a full buffer is
 * ranked by counting and cut to top_k; factor_merge_kernel merges the chunks.  No atomics.
 * ------------------------------------------------------------------------------------- */
#define RTREC_FACTOR_TOPK_WORKSPACE_BYTES(n_rows, top_k, item_splits) \
    ((size_t)(n_rows) * (size_t)(item_splits) * ((size_t)(top_k) * 8u + 4u))
int rtrec_factor_topk(int32_t n_rows, const int32_t *d_row_ids, const int32_t *d_p_index, int32_t n_x_rows, const float *d_p,
                      int64_t p_stride, int32_t n_p_rows, const float *d_qt, int64_t qt_stride, int32_t n_items, int32_t dim,
                      const uint8_t *d_item_mask, const int32_t *d_xb_ptr, const int32_t *d_xb_col, int64_t xb_nnz,
                      int32_t filter_interacted, int32_t top_k, int32_t item_splits, int32_t *d_out_ids, float *d_out_scores,
                      int32_t *d_out_count, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * FEATURE REPRESENTATIONS  (sparse feature rows times a dense per-feature table: the vectors rtrec_factor_topk scores.)
 * The reference's hybrid model never reads an entity's vector from a table: it builds a sparse feature row per user or item --
 * the identity column plus the columns of its tags -- and multiplies it into LightFM's per-feature embedding and bias tables
 * (get_user_representations(features) = features * user_biases, features * user_embeddings; scipy's csr_matvec / csr_matvecs).
 * This call is that product, written where rtrec_factor_topk reads: training per-feature tables is not part of this library
 * (rtrec_factor_als_solve learns one vector per user and item, no tag tables).
 *   rows        a CSR of feature rows d_f_ptr[n_f_rows + 1] / d_f_col[nnz] / d_f_val[nnz] (int32 / int32 / float32);
 *               d_f_val == NULL: every value is 1.  Offsets are clamped to [0, nnz], so a malformed CSR gives wrong answers,
 *               never an out-of-range read.  Job r takes row d_job_rows[r] (d_job_rows == NULL: row r); a value outside
 *               [0, n_f_rows) means the job has no row.  Rows may repeat among the jobs
 *   table       d_e[n_features][e_stride] float32 of dim_e components (e_stride >= dim_e), d_bias[n_features] float32
 *   sum         per component c: s = +0.0f, then for the stored entries of the row IN STORAGE ORDER
 *               s = fl(s + fl(v * e[col][c])): two correctly rounded operations per entry, never contracted to a fused
 *               multiply-add, float32 denormals kept -- scipy's loop, so equal to `csr @ table` bit for bit.  b is the same
 *               chain over d_bias.  An entry whose column lies outside [0, n_features) is skipped (the reference ignores the
 *               features it has not learned); equal columns are not merged, each stored entry adds once
 *   has         1 when the job's row stores at least one entry that is not skipped, whatever its value; else 0
 *   layout      RTREC_FEATURE_PLAIN: width = dim_e, slots e[0 .. dim_e).  RTREC_FEATURE_USER: width = dim_e + 2, slots
 *               [b, 1.0f, e...].  RTREC_FEATURE_ITEM: width = dim_e + 2, slots [1.0f, b, e...] -- the reference's stacking,
 *               whose dot product is b_u + b_i + e_u . e_i (utils/factors.stack_bias).  A job with has == 0 gets +0.0f in
 *               EVERY slot, the constant included, so that a missing vector scores 0 against everything
 * Out, every slot of every job written: slot c of job r is d_out[r * row_stride + c * comp_stride].  Either comp_stride == 1
 * and row_stride >= width (row-major: the user matrix d_p of rtrec_factor_topk) or row_stride == 1 and comp_stride >= n_jobs
 * (component-major: its item matrix d_qt); what lies between the slots is not touched.  d_has[n_jobs] (uint8) may be NULL.
 * layout outside the three above, dim_e < 1 or width > 256 (the limit of rtrec_factor_topk): RTREC_ERR_UNSUPPORTED.  Negative
 * sizes, e_stride < dim_e, output strides of neither form, NULL required arrays (d_f_ptr with n_f_rows > 0, d_f_col with
 * nnz > 0, d_e -- and d_bias with a stacking layout -- with n_features > 0, d_out): RTREC_ERR_INVALID_ARG.  n_jobs == 0:
 * RTREC_OK before any pointer check.  No global state, no environment variable, no allocation, no synchronisation.  The results
 * never depend on the grid or on scheduling: a slot is one sequential chain computed by one thread.
 * csrc/feature_repr.hip, feature_repr_kernel: one thread per output slot (job = t / width, slot = t % width), so a wave carries
 * 64 / width short rows; the lanes of a job share the reads of its offsets, columns and values and read neighbouring components
 * of a table row; plain loads and stores, no LDS, no atomics.
 * ------------------------------------------------------------------------------------- */
#define RTREC_FEATURE_PLAIN 0
#define RTREC_FEATURE_USER 1
#define RTREC_FEATURE_ITEM 2
int rtrec_feature_repr(int32_t n_jobs, const int32_t *d_job_rows, int32_t n_f_rows, const int32_t *d_f_ptr, const int32_t *d_f_col,
                       const float *d_f_val, int64_t nnz, const float *d_e, int64_t e_stride, int32_t n_features, int32_t dim_e,
                       const float *d_bias, int32_t layout, float *d_out, int64_t row_stride, int64_t comp_stride, uint8_t *d_has,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * FACTOR NORMS  (one Euclidean norm per vector of a dense float32 matrix: the divisors of rtrec_factor_similar_topk.)
 * Component c of vector r is d_v[r * row_stride + c * comp_stride]; the strides follow rtrec_feature_repr: either
 * comp_stride == 1 and row_stride >= dim (row-major) or row_stride == 1 and comp_stride >= n (component-major, the item matrix
 * d_qt of rtrec_factor_topk).
 *   norm        n2 = +0.0f, then for c = 0 .. dim-1 ascending n2 = fmaf(v[c], v[c], n2): one correctly rounded fused
 *               multiply-add per component, float32 denormals kept; d_out[r] = sqrt(n2), correctly rounded to float32 (a
 *               denormal n2 included).  n2 is rtrec_factor_topk's score of the vector with itself, bit for bit.  NOT numpy's
 *               norm: numpy rounds every square on its own and adds them in its pairwise order (DESIGN, divergences)
 * dim in 1..256: RTREC_ERR_UNSUPPORTED otherwise.  Negative n, strides of neither form, NULL arrays: RTREC_ERR_INVALID_ARG.
 * n == 0: RTREC_OK before any pointer check.  No global state, no environment variable, no allocation, no synchronisation.
 * The results never depend on the grid or on scheduling: a norm is one sequential chain computed by one thread.
 * csrc/factor_norms.hip, factor_norms_kernel: one thread per vector (component-major: neighbouring threads read neighbouring
 * items); the root is taken in float64 and rounded once more, which cannot double-round wrongly (53 >= 2 * 24 + 2).
 * ------------------------------------------------------------------------------------- */
int rtrec_factor_norms(int32_t n, const float *d_v, int64_t row_stride, int64_t comp_stride, int32_t dim, float *d_out,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * FACTOR SIMILAR TOP-K  (cosine top-k of item vectors against the whole catalogue, the query itself excluded.)
 * The reference's hybrid model takes the factor side of similar_items from implicit.topk(items=target, query=q, k,
 * item_norms=||target_i||, filter_items=[query]) (rtrec/models/hybrid.py, _similar_items): a float32 GEMM, each score divided
 * by the item's norm, the query set to -FLT_MAX, a top-k; the division by ||q|| follows later.
 *   targets     component c of item i is d_qt[c * qt_stride + i], qt_stride >= n_items, dim in 1..256.  A caller selects
 *               components by offsetting the pointer: for the matrix rtrec_feature_repr writes with RTREC_FEATURE_ITEM
 *               ([1, b, e...]) the reference's [b, e...] is d_qt + qt_stride with dim - 1.  d_norms[n_items] are the divisors
 *               (rtrec_factor_norms of the same components)
 *   queries     job r names item q = d_queries[r].  With d_p == NULL its vector is column q of d_qt and its norm d_norms[q];
 *               a q outside [0, n_items) is a job without a vector and returns an empty list.  With d_p != NULL its vector is
 *               row r of d_p[n_rows][p_stride] (p_stride >= dim) and its norm d_p_norms[r]; q only names what is excluded and
 *               may be -1 (or d_queries NULL): then nothing is excluded
 *   score       dot = +0.0f, then dot = fmaf(vq[c], v_i[c], dot) for c = 0 .. dim-1 ascending (rtrec_factor_topk's chain);
 *               s1 = fl(dot / d_norms[i]): ONE correctly rounded float32 division, denormals kept
 *   competing   0 <= i < n_items, i != q, d_item_mask == NULL or d_item_mask[i] != 0, and s1 is not NaN.  So a zero vector
 *               (0 / 0) never competes; +-inf compete as numbers
 *   order       the larger s1 first; among == (-0.0 == +0.0) the lower item id.  Strict, so a list is unique
 *   written     s1 as it is when write_cosine == 0.  With write_cosine != 0 the written score is fl(s1 / norm_q), one more
 *               correctly rounded division made where the final list is written (never on the partial list of a chunk), and a
 *               job whose query norm is not > 0 (NaN included) returns an empty list.  The list's order is s1's either way
 *   out_div     d_out_div != NULL: d_out_div[r] = the job's query norm (+0.0f for a job without a vector) -- the divisor
 *               rtrec_similar_blend applies after its cut, as the reference does
 * Out, every slot written: d_out_ids[n_rows][top_k] / d_out_scores[n_rows][top_k], behind the list -1 / -inf;
 * d_out_count[r] = min(top_k, competing items).
 * item_splits, d_workspace and workspace_bytes are rtrec_factor_topk's, RTREC_FACTOR_TOPK_WORKSPACE_BYTES included.
 * dim in 1..256, top_k in 1..128, item_splits in 0..64: RTREC_ERR_UNSUPPORTED otherwise.  NULL required arrays (d_queries
 * without d_p; d_p_norms with d_p; d_qt and d_norms with n_items > 0; d_workspace with item_splits > 1), negative sizes and
 * strides below their widths: RTREC_ERR_INVALID_ARG.  A workspace too small for an explicit item_splits: RTREC_ERR_WORKSPACE.
 * n_rows == 0: RTREC_OK before any pointer check.  No global state, no environment variable, no allocation, no
 * synchronisation.  The results never depend on item_splits, on the grid or on scheduling.
 * csrc/factor_similar.hip, factor_similar_kernel: factor_topk_kernel's scan (32 queries x one chunk per one-wave workgroup, the
 * v_mfma_f32_32x32x2_f32 chain, threshold in registers, candidate buffer in LDS, ranks by counting) with another epilogue: a lane
 * loads the 16 norms its accumulators map to, divides, then tests threshold, query and mask; factor_similar_merge_kernel merges
 * the chunks and makes the cosine division.  No atomics.
 * ------------------------------------------------------------------------------------- */
int rtrec_factor_similar_topk(int32_t n_rows, const int32_t *d_queries, const float *d_p, int64_t p_stride, const float *d_p_norms,
                              const float *d_qt, int64_t qt_stride, int32_t n_items, int32_t dim, const float *d_norms,
                              const uint8_t *d_item_mask, int32_t top_k, int32_t item_splits, int32_t write_cosine,
                              int32_t *d_out_ids, float *d_out_scores, int32_t *d_out_count, float *d_out_div, void *d_workspace,
                              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * SIMILAR BLEND  (the hybrid's similar_items after its two top-k calls: cut, exclude, divide, min-max, a FLOAT64 sum per id.)
 * The reference's HybridSlimFM._similar_items cuts the factor list at -FLT_MAX, divides it by ||q||, drops the query, runs
 * minmax_normalize on both lists, adds them per id into a defaultdict(float) (comb_sum: every += is a float64 addition) and
 * returns sorted(..., reverse=True)[:top_k].  List A is the factor list, list B SLIM's; both arrive best first, in the form of
 * rtrec_slim_blend_lists: ka / kb positions (1..1024) of ids and float32 scores per row, strides >= ka / kb, counts clamped to
 * [0, ka] / [0, kb].
 *   length      a list is cut at its first position that lies behind its count, whose id is outside [0, n_items), or whose
 *               RAW score is not finite or is <= -FLT_MAX: rtrec_slim_blend_lists' rule, applied before any division
 *   exclude     what remains loses every entry whose id == d_exclude[r] (both lists); d_exclude == NULL or -1 excludes nothing
 *   divide      with d_a_div != NULL, A's scores become fl(s / d_a_div[r]), correctly rounded; a divisor that is not > 0 (NaN
 *               included) makes A empty for that row
 *   norm        per non-empty list, over what is left: rtrec_slim_blend_lists' float32 fl(fl(s - mn) / fl(fl(mx - mn) + 1e-8f)).
 *               An EMPTY list contributes nothing -- the reference raises ValueError (min of an empty sequence) there
 *   union       the entries stand in order of first appearance: A's distinct ids, then the ids only B holds.  The value is a
 *               float64: 0.0, then + (double)normA[p] for EVERY occurrence of the id in A in ascending p, then
 *               + (double)normB[q] for every occurrence in B in ascending q; each addition is rounded to float64.  (This is not
 *               rtrec_slim_blend_lists, which adds in float32 and lets a repeat inside A keep its last score.)
 *   order       the larger value first; == values (-0.0 == +0.0) keep the union's order.  A NaN value is never listed
 * Out, every slot written: d_out_ids[n_rows][keep], d_out_value[n_rows][keep] (FLOAT64), d_out_source[n_rows][keep] (1 = only A
 * holds the item, 2 = only B, 3 = both), d_out_count[r] = min(keep, the entries whose value is a number); behind it -1 / -inf / 0.
 * ka and kb in 1..1024, keep in 1..ka+kb, waves_per_row in {0, 1, 4}: RTREC_ERR_UNSUPPORTED otherwise.  NULL required arrays
 * (all but d_a_div and d_exclude), negative sizes and a stride below its list length: RTREC_ERR_INVALID_ARG.  n_rows == 0:
 * RTREC_OK before any pointer check.  No global state, no environment variable, no allocation, no synchronisation.  The results
 * never depend on waves_per_row, on the grid size or on scheduling.
 * csrc/similar_blend.hip, similar_blend_kernel: one row per workgroup on list_stage.hip.h's frame; both lists, their normalised
 * values and the union's doubles in LDS (32 bytes per position of the longer list); an excluded position is a hole, not squeezed
 * out; the owner of an entry adds its occurrences in order; ranks by counting over the doubles; no atomics.
 * ------------------------------------------------------------------------------------- */
int rtrec_similar_blend(int32_t n_rows, int32_t n_items, const int32_t *d_a_ids, int64_t a_ids_stride, const float *d_a_scores,
                        int64_t a_scores_stride, const int32_t *d_a_counts, int32_t ka, const float *d_a_div,
                        const int32_t *d_b_ids, int64_t b_ids_stride, const float *d_b_scores, int64_t b_scores_stride,
                        const int32_t *d_b_counts, int32_t kb, const int32_t *d_exclude, int32_t keep, int32_t waves_per_row,
                        int32_t *d_out_ids, double *d_out_value, int32_t *d_out_source, int32_t *d_out_count, void *stream);

/* ---------------------------------------------------------------------------------------
 * FACTOR GRAM  (V^T V + reg I of one side's vectors: the constant part of every row's system in an ALS half-step.)
 * The reference's hybrid model owns its second model (HybridSlimFM.fit / bulk_fit call LightFMWrapper.fit_partial); LightFM's
 * WARP / hogwild SGD is not reproducible and serialises badly on a GPU.  This library trains the vectors rtrec_factor_topk
 * scores by implicit-feedback alternating least squares instead (Hu, Koren, Volinsky 2008): deterministic, dense, and pinned
 * operation by operation.  A HALF-STEP solves one side against the other side held fixed: this call, then
 * rtrec_factor_als_solve.  The fixed side is d_v[n_v][v_stride] row-major float32, v_stride >= dim (what lies between dim and
 * v_stride is never read).
 *   chunk       the rows of V are cut into chunks of 1024 -- a constant of this contract: chunk c is rows
 *               [1024 c, min(n_v, 1024 c + 1024))
 *   partial     part_c[a][b] = +0.0f, then part_c[a][b] = fmaf(v_r[a], v_r[b], part_c[a][b]) for the rows r of chunk c ascending:
 *               one correctly rounded fused multiply-add per row, float32 denormals kept
 *   sum         G[a][b] = +0.0f, then G[a][b] = fl(G[a][b] + part_c[a][b]) for c ascending, one rounded add each; finally
 *               G[a][a] = fl(G[a][a] + reg)
 * Out: d_gram[dim][dim] float32, every element written.  It is symmetric bit for bit (a product commutes).  n_v == 0 gives
 * reg * I.  The partials live in d_workspace: RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim) bytes (a macro, not an entry point,
 * as RTREC_FACTOR_TOPK_WORKSPACE_BYTES; none for n_v == 0).
 * dim in 1..64: RTREC_ERR_UNSUPPORTED otherwise.  Negative n_v, v_stride < dim, a reg that is negative or NaN, NULL d_gram, NULL
 * d_v or d_workspace with n_v > 0: RTREC_ERR_INVALID_ARG.  A workspace too small: RTREC_ERR_WORKSPACE.  No global state, no
 * environment variable, no allocation, no synchronisation.  The results never depend on the grid or on scheduling.
 * csrc/factor_gram.hip: factor_gram_partial_kernel, one one-wave workgroup per chunk, a 32 x 32 tile is one chain of
 * v_mfma_f32_32x32x2_f32 over ascending rows (that fmaf chain bit for bit), the three lower tiles for dim > 32;
 * factor_gram_sum_kernel adds the partials, one thread per element.  No atomics.
 * ------------------------------------------------------------------------------------- */
#define RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim) \
    ((((size_t)(n_v) + 1023u) / 1024u) * (size_t)(dim) * (size_t)(dim) * 4u)
int rtrec_factor_gram(int32_t n_v, const float *d_v, int64_t v_stride, int32_t dim, float reg, float *d_gram, void *d_workspace,
                      size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * FACTOR ALS SOLVE  (per row of R: build G + sum w y y^T and sum (1 + w) y, factor by Cholesky, solve -- every operation pinned.)
 * The second call of a half-step.  R is a CSR d_r_ptr[n_rows + 1] / d_r_idx[nnz] / d_r_val[nnz] (int32 / int32 / float32): X's
 * CSR for the user half-step, X's CSC read as a CSR of X^T for the item half-step.  The fixed side is d_v[n_v][v_stride] as for
 * rtrec_factor_gram, d_gram[dim][dim] what that call wrote for it.  Job r names row x = d_job_rows[r] (d_job_rows == NULL:
 * x = r).  Offsets are clamped to [0, nnz], so a malformed CSR gives wrong answers, never an out-of-range read.
 *   usable      a stored entry (i, val) of row x is usable when 0 <= i < n_v and w = fl(alpha * val) satisfies w > 0: NaN and
 *               non-positive values are skipped, and the row of V a skipped entry names is never read
 *   build       only the lower triangle a >= b is defined.  A[a][b] = G[a][b], then over the usable entries IN STORAGE ORDER
 *               A[a][b] = fmaf(fl(w * y_i[a]), y_i[b], A[a][b]) (y_i = row i of V);  rhs[a] = +0.0f, then
 *               rhs[a] = fmaf(fl(1.0f + w), y_i[a], rhs[a])
 *   Cholesky    left-looking, every element one chain.  For j = 0 .. dim-1: d = A[j][j], then d = fmaf(-L[j][k], L[j][k], d) for
 *               k = 0 .. j-1; if !(d > 0) or d is not finite the job BREAKS DOWN; L[j][j] = sqrt(d), correctly rounded; for
 *               i > j: s = A[i][j], then s = fmaf(-L[i][k], L[j][k], s) for k ascending, L[i][j] = fl(s / L[j][j]): one correctly
 *               rounded division
 *   forward     for j ascending: s = rhs[j], then s = fmaf(-L[j][k], z[k], s) for k = 0 .. j-1; z[j] = fl(s / L[j][j])
 *   backward    for j = dim-1 .. 0: s = z[j], then s = fmaf(-L[k][j], x[k], s) for k = dim-1 down to j+1; x[j] = fl(s / L[j][j])
 * Float32 denormals are kept; nothing is contracted or reordered beyond what is written here.
 * Out: the vector is written in place at d_out[x * out_stride + c], c in [0, dim); what lies between dim and out_stride is not
 * touched.  d_status[r] (uint8): 0 = solved; 1 = x lies outside [0, n_rows) (nothing else is written), or the row has no usable
 * entry (the vector is all +0.0f); 2 = breakdown, or a component that is not finite (the vector is all +0.0f).  Jobs must name
 * distinct rows, otherwise the result is unspecified.  The sign of a zero is not part of the contract.
 * dim in 1..64: RTREC_ERR_UNSUPPORTED otherwise.  Negative sizes, strides below dim, an alpha that is not > 0 (NaN included):
 * RTREC_ERR_INVALID_ARG, as are NULL required arrays (d_gram, d_out, d_status; d_r_ptr with n_rows > 0; d_r_idx and d_r_val with
 * nnz > 0; d_v with n_v > 0).  n_jobs == 0: RTREC_OK before any pointer check.  No global state, no environment variable, no
 * allocation, no synchronisation.  The results never depend on the grid or on scheduling: a job is one sequential chain
 * computed by one wave.
 * csrc/factor_als.hip, factor_als_solve_kernel: one wave per job; the build is one chain of v_mfma_f32_32x32x2_f32 per 32 x 32
 * tile with the accumulator initialised from G (A operand fl(w * y[a]), B operand y[b], k over the entries, two per
 * instruction; one tile for dim <= 32, the three lower ones for dim <= 64), which is that fmaf chain bit for bit; zero
 * operands stand where the chain has no term; rhs is a VALU chain; the accumulators go to LDS as A and Cholesky and both
 * substitutions run with lane = row.  No atomics.
 * ------------------------------------------------------------------------------------- */
int rtrec_factor_als_solve(int32_t n_jobs, const int32_t *d_job_rows, int32_t n_rows, const int32_t *d_r_ptr, const int32_t *d_r_idx,
                           const float *d_r_val, int64_t nnz, const float *d_v, int64_t v_stride, int32_t n_v, int32_t dim,
                           const float *d_gram, float alpha, float *d_out, int64_t out_stride, uint8_t *d_status, void *stream);

/* ---------------------------------------------------------------------------------------
 * FACTOR GRAM WIDE  (rtrec_factor_gram for vectors of up to 256 components.)
 * The definition is rtrec_factor_gram's word for word -- chunks of 1024 rows, per element one fmaf chain over the chunk's
 * ascending rows, the chunks added in ascending order with one rounded add each, reg added to the diagonal last -- for
 * dim in 1..256.  RTREC_FACTOR_GRAM_WORKSPACE_BYTES and every argument rule are rtrec_factor_gram's.  For dim <= 64 the output
 * equals rtrec_factor_gram's bit for bit; it is symmetric bit for bit for every dim.
 * dim in 1..256: RTREC_ERR_UNSUPPORTED otherwise.  Negative n_v, v_stride < dim, a reg that is negative or NaN, NULL d_gram, NULL
 * d_v or d_workspace with n_v > 0: RTREC_ERR_INVALID_ARG.  A workspace too small: RTREC_ERR_WORKSPACE.  No global state, no
 * environment variable, no allocation, no synchronisation.  The results never depend on the grid or on scheduling.
 * csrc/factor_gram.hip: factor_gram_wide_partial_kernel, one one-wave workgroup per (chunk, lower 32 x 32 tile), each one chain of
 * v_mfma_f32_32x32x2_f32 over ascending rows; a tile below the diagonal is written twice, once transposed;
 * factor_gram_sum_kernel adds the partials.  No atomics.
 * ------------------------------------------------------------------------------------- */
int rtrec_factor_gram_wide(int32_t n_v, const float *d_v, int64_t v_stride, int32_t dim, float reg, float *d_gram,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * FACTOR ALS CG  (per row of R: a few conjugate-gradient steps on the system of rtrec_factor_als_solve, never forming its matrix.)
 * The other second call of a half-step, for dim up to 256.  R, the jobs, V, the clamped offsets and the USABLE entries are
 * rtrec_factor_als_solve's (0 <= i < n_v and w = fl(alpha * val) > 0; a skipped entry's row of V is never read), and so is the
 * system of row x: A = G + sum_i w_i y_i y_i^T, b = sum_i (1 + w_i) y_i over the usable entries IN STORAGE ORDER.  d_gram must be
 * symmetric bit for bit (both Gram calls guarantee it); for another matrix the result is unspecified, nothing is read out of
 * range.  Every operation is pinned:
 *   chain(u, v) s = +0.0f, then s = fmaf(u[c], v[c], s) for c = 0 .. dim-1 (rtrec_factor_topk's score)
 *   tree(u, v)  q[c] = fl(u[c] * v[c]) for c < dim and +0.0f for dim <= c < D, D the least power of two >= dim; for
 *               h = D/2, D/4, .., 1: q[c] = fl(q[c] + q[c + h]) for c < h; the result is q[0] (the xor-butterfly of a
 *               cross-lane reduction: c pairs with c + h, not with a neighbour)
 *   mat(v)[a]   s = +0.0f, then s = fmaf(G[a][b], v[b], s) for b ascending
 *   start       x = the vector stored at d_out[x_row * out_stride + c]; with warm_start == 0, or when any stored component
 *               is not finite, x = +0.0f throughout
 *   residual    r[a] = -mat(x)[a]; then over the usable entries in storage order t = chain(y_i, x),
 *               coef = fl(fl(1.0f + w) - fl(w * t)), r[a] = fmaf(coef, y_i[a], r[a]).  (From x = 0, r is
 *               rtrec_factor_als_solve's rhs.)
 *   first       p = r, rs = tree(r, r); if rs < 1e-20f the job is done: x stays as it is, status 0
 *   step        cg_steps times: Ap = mat(p), then over the usable entries in storage order t = chain(y_i, p),
 *               Ap[a] = fmaf(fl(w * t), y_i[a], Ap[a]); den = tree(p, Ap); if !(den > 0) or den is not finite the job BREAKS
 *               DOWN; al = fl(rs / den), one correctly rounded division; x[a] = fmaf(al, p[a], x[a]);
 *               r[a] = fmaf(-al, Ap[a], r[a]); rn = tree(r, r); if rn < 1e-20f stop; be = fl(rn / rs);
 *               p[a] = fmaf(be, p[a], r[a]); rs = rn
 * Float32 denormals are kept; nothing is contracted or reordered beyond what is written here.
 * Out: the vector in place at d_out[x_row * out_stride + c], c in [0, dim), as rtrec_factor_als_solve writes it.  d_status[r]
 * (uint8): 0 = finished; 1 = x_row lies outside [0, n_rows) (nothing of d_out is written), or the row has no usable entry (the
 * vector is all +0.0f); 2 = breakdown, or a component of x that is not finite (the vector is all +0.0f).  d_out_rs[r] (may be
 * NULL): the last tree(r, r) computed for the job, +0.0f for status 1.  Jobs must name distinct rows.  The sign of a zero is
 * not part of the contract.
 * dim in 1..256 and cg_steps in 1..64: RTREC_ERR_UNSUPPORTED otherwise.  RTREC_ERR_INVALID_ARG as rtrec_factor_als_solve:
 * negative sizes, strides below dim, an alpha that is not > 0, NULL required arrays.  n_jobs == 0: RTREC_OK before any pointer
 * check.  warm_start: 0 or not 0.  No global state, no environment variable, no allocation, no synchronisation.  The results
 * never depend on the grid or on scheduling.
 * csrc/factor_als_cg.hip, factor_als_cg_kernel: one workgroup of 1 / 2 / 4 waves per job, lane = component for x, r, p and Ap; the
 * entries are taken 64 at a time, their rows of V staged in LDS; t with lane = entry, the updates with lane = component; mat
 * reads row b of G (= column b, by the symmetry) coalesced.  No atomics.
 * ------------------------------------------------------------------------------------- */
int rtrec_factor_als_cg(int32_t n_jobs, const int32_t *d_job_rows, int32_t n_rows, const int32_t *d_r_ptr, const int32_t *d_r_idx,
                        const float *d_r_val, int64_t nnz, const float *d_v, int64_t v_stride, int32_t n_v, int32_t dim,
                        const float *d_gram, float alpha, int32_t cg_steps, int32_t warm_start, float *d_out, int64_t out_stride,
                        uint8_t *d_status, float *d_out_rs, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RTREC_AMD_EXT_H */
