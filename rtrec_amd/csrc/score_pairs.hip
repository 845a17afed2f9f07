// rtrec_amd/csrc/score_pairs.hip -- rerank per-user candidate lists: score(u, i) for every (user row, list item) pair, and the
// order of each row's list.
//
// The reference ranks ONE list shared by all users (recommend_batch with candidate_item_ids; csrc/score_cands.hip); a
// two-stage recommender brings a list of its own per user.  The contract is the comment of rtrec_slim_score_pairs in
// include/rtrec_amd.h; in short:
//   score(u, i)  the float32 sum of fl32(x_uj * w_ji) over the j stored in both row u of X (CSR, ascending j) and column i of W
//                (CSC, ascending j): one rounded multiply per term (-ffp-contract=off: never fused), one rounded add per term, in
//                ascending j from +0.0f -- the explanations' invariant, scipy's csr_matmat order for one output entry
//   support      the number of common j; -1 for an empty list position (at or beyond counts[r], or an id outside [0, n_items))
//   ranking      position p beats q if score[p] > score[q], or the scores are == and p > q (the LATER position first: DESIGN D1,
//                the rule of CANDIDATES mode); NaN scores and, with filter_interacted, items stored in the row do not compete
//
// Mapping (the frame is list_stage.hip.h's).  Threads take list positions, strided by the workgroup's thread count.  A
// thread walks its item's column of W in entry order and looks each j up in the user's row by binary search -- the row is
// staged in LDS up to kPairsRow1 / kPairsRow4 entries and searched in global memory beyond that -- and adds the hits into its
// accumulator, so the order of the sum is the column's and a column of any length works.  The same search answers "is item i
// stored in the row" for the filter.  The scores go to LDS (NaN for what does not compete) and the ranking is by counting: a
// competing position's rank is the number of positions that beat it, found with wave-uniform (broadcast) reads of the LDS
// score array; the order is strict, so ranks are unique -- no sort, no race, nothing that depends on scheduling.
// LDS: 4 KiB of scores + 8 bytes per staged row entry = 5 KiB (one wave, 128 entries) / 20 KiB (four waves, 2,048 entries):
// 32 waves per CU fit the CU's 160 KiB in either form, so LDS never limits the occupancy.
// Malformed input cannot read out of range: CSR / CSC offsets are clamped to the arrays' lengths, counts to [0, list_k], a row
// id outside [0, n_x_rows) is an empty row and an item id outside [0, n_items) an empty position.
#include "list_stage.hip.h"
#include "../../include/rtrec_amd.h"

namespace rtrec {
namespace {

constexpr int kPairsMaxList = 1024;     // list_k limit: the LDS score array
constexpr int kPairsRow1 = 128;         // row entries staged in LDS, one wave per row
constexpr int kPairsRow4 = 2048;        // ... four waves per row

template <int WAVES, int ROW>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_num_sgpr(80))) void score_pairs_kernel(
        int n_rows, const int32_t *__restrict__ row_ids, const int32_t *__restrict__ xb_ptr, const int32_t *__restrict__ xb_col,
        const float *__restrict__ xb_val, int n_x_rows, long long xb_nnz, int n_items, const int32_t *__restrict__ wc_ptr,
        const int32_t *__restrict__ wc_row, const float *__restrict__ wc_val, long long wc_nnz, const int32_t *__restrict__ ids,
        long long ids_stride, int list_k, const int32_t *__restrict__ counts, int top_k, int filter_interacted,
        float *__restrict__ out_scores, int32_t *__restrict__ out_support, int32_t *__restrict__ out_order,
        int32_t *__restrict__ out_count) {
    constexpr int NT = WAVES * 64;
    __shared__ __attribute__((aligned(16))) float sc[kPairsMaxList];
    __shared__ int32_t lcol[ROW];
    __shared__ float lval[ROW];
    const int tid = static_cast<int>(threadIdx.x);
    const float nan = __builtin_nanf("");
    const int k4 = (list_k + 3) & ~3;                                     // the ranking reads the scores four at a time
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        long long b;
        const int len = csr_row(xb_ptr, row_behind(row_ids, r), n_x_rows, xb_nnz, b);
        const int32_t *rcol = xb_col + b;
        const float *rval = xb_val + b;
        const bool staged = len <= ROW;
        if (staged) for (int q = tid; q < len; q += NT) { lcol[q] = rcol[q]; lval[q] = rval[q]; }
        const int cnt = clamp_count(counts[r], list_k);
        __syncthreads();                                                  // the staged row is visible to every wave
        // x = the row's value at item j, if the row stores j
        auto lookup = [&](int j, float &x) -> bool {
            return staged ? find_sorted(lcol, lval, len, j, x) : find_sorted(rcol, rval, len, j, x);
        };
        // ---- scores and supports: thread t takes positions t, t + NT, ... (the trip count is the same for every thread)
        int competing = 0;
        for (int base = 0; base < k4; base += NT) {
            const int p = base + tid;
            bool competes = false;
            float acc = 0.0f;
            if (p < list_k) {
                const int item = p < cnt ? ids[r * ids_stride + p] : -1;
                int support = -1;
                if (item >= 0 && item < n_items) {
                    support = 0;
                    if (len > 0) {
                        long long s = wc_ptr[item], e = wc_ptr[item + 1];
                        clamp_span(s, e, wc_nnz);
                        for (long long q = s; q < e; ++q) {
                            float x;
                            if (lookup(wc_row[q], x)) { acc = __fadd_rn(acc, __fmul_rn(x, wc_val[q])); ++support; }
                        }
                    }
                    competes = acc == acc;                                // a NaN score is written, never listed
                    float x;
                    if (competes && filter_interacted && lookup(item, x)) competes = false;
                }
                out_scores[r * list_k + p] = acc;
                out_support[r * list_k + p] = support;
            }
            if (p < k4) sc[p] = competes ? acc : nan;
            competing += __popcll(__ballot(competes));
        }
        if (top_k > 0) {
            __syncthreads();                                              // all scores are in LDS; the staged row is not needed any more
            int n_out = block_sum<WAVES>(competing, lcol, tid);           // the waves' numbers of competitors meet in the row's slots
            n_out = n_out < top_k ? n_out : top_k;
            // ---- rank by counting
            for (int p = tid; p < list_k; p += NT) {
                const float v = sc[p];
                if (v != v) continue;
                const int rank = rank_by_count<true>(sc, k4, p, v);       // among == scores the LATER position first
                if (rank < top_k) out_order[r * top_k + rank] = p;
            }
            for (int t = n_out + tid; t < top_k; t += NT) out_order[r * top_k + t] = -1;
            if (tid == 0) out_count[r] = n_out;
        } else if (out_count && tid == 0) {
            out_count[r] = 0;
        }
        __syncthreads();                                                  // the row is done: LDS may be overwritten
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_slim_score_pairs(int32_t n_rows, const int32_t *d_row_ids, const int32_t *d_xb_ptr, const int32_t *d_xb_col,
                                      const float *d_xb_val, int32_t n_x_rows, int64_t xb_nnz, int32_t n_items,
                                      const int32_t *d_wc_ptr, const int32_t *d_wc_row, const float *d_wc_val, int64_t wc_nnz,
                                      const int32_t *d_ids, int64_t ids_stride, int32_t list_k, const int32_t *d_counts,
                                      int32_t top_k, int32_t filter_interacted, int32_t waves_per_row, float *d_out_scores,
                                      int32_t *d_out_support, int32_t *d_out_order, int32_t *d_out_count, void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_x_rows < 0 || xb_nnz < 0 || n_items < 0 || wc_nnz < 0) return RTREC_ERR_INVALID_ARG;
    if (list_k < 1 || list_k > kPairsMaxList || top_k < 0 || top_k > list_k) return RTREC_ERR_UNSUPPORTED;
    if (!list_waves_valid(waves_per_row)) return RTREC_ERR_UNSUPPORTED;
    if (ids_stride < list_k) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_ids || !d_counts || !d_out_scores || !d_out_support || (top_k > 0 && (!d_out_order || !d_out_count))) return RTREC_ERR_INVALID_ARG;
    if (!csr_present(n_x_rows, d_xb_ptr, xb_nnz, d_xb_col, d_xb_val)) return RTREC_ERR_INVALID_ARG;
    if (!csc_present(n_items, d_wc_ptr, wc_nnz, d_wc_row, d_wc_val)) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    const int waves = list_waves(waves_per_row, n_rows, list_k), grid = list_grid(n_rows);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (waves == 4)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(score_pairs_kernel<4, kPairsRow4>), dim3(grid), dim3(256), 0, st, n_rows, d_row_ids, d_xb_ptr,
                           d_xb_col, d_xb_val, n_x_rows, static_cast<long long>(xb_nnz), n_items, d_wc_ptr, d_wc_row, d_wc_val,
                           static_cast<long long>(wc_nnz), d_ids, static_cast<long long>(ids_stride), list_k, d_counts, top_k,
                           filter_interacted, d_out_scores, d_out_support, d_out_order, d_out_count);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(score_pairs_kernel<1, kPairsRow1>), dim3(grid), dim3(64), 0, st, n_rows, d_row_ids, d_xb_ptr,
                           d_xb_col, d_xb_val, n_x_rows, static_cast<long long>(xb_nnz), n_items, d_wc_ptr, d_wc_row, d_wc_val,
                           static_cast<long long>(wc_nnz), d_ids, static_cast<long long>(ids_stride), list_k, d_counts, top_k,
                           filter_interacted, d_out_scores, d_out_support, d_out_order, d_out_count);
    return launch_status();
}
