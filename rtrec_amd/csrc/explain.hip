// rtrec_amd/csrc/explain.hip -- why an item was recommended: the largest terms of score(u, i) = sum_j X[u, j] * W[j, i].
//
// The reference has no such call; the contract is the comment of rtrec_slim_explain_topk in include/rtrec_amd.h.  For a
// (user row, item) pair the contributing items are the j stored in both row u of X (CSR, ascending j) and column i of W
// (CSC, ascending j); c(j) = fl32(x_uj * w_ji) is ONE rounded float32 multiply (-ffp-contract=off: never fused), so adding the
// c(j) in ascending j from 0.0f reproduces the score the scoring kernels report (scipy's csr_matmat order).
//
// One wave per user row, looping over the row's list positions.  Feature selection caps a column of W at K stored weights
// (K = 50 in every benchmark configuration), so a pair is an intersection of <= K column entries with the sorted row:
//   lanes take the column's entries (strided by 64 when the column is longer), each binary-searches its j in the row --
//   through the wave's registers (ds_bpermute) when the row has at most 64 entries, in memory otherwise -- and forms the
//   product on a hit; __ballot + popcount of the hits give the support; top_m rounds of wave_best pick the reasons, each
//   round excluding what the previous winner beats (similar_topk_kernel's scheme: nothing is stored besides the last winner).
//   A column of at most 64 entries is probed once and kept in registers; a longer one is probed again every round.
// A NaN product counts in the support and is never a candidate (rerank's rule): cand_better is a strict total order only
// over numbers, so no NaN may reach it.  +-inf are numbers; +0.0f and -0.0f compare equal and go by item id, each written
// with its own sign bit.  The rounds end when no candidate is left, so a pair's slots from the number of its non-NaN
// contributions on stay padding.
// Malformed input cannot read out of range: CSR / CSC offsets are clamped to the arrays' lengths, a row id outside
// [0, n_x_rows) is an empty row and an item id outside [0, n_items) has no column.
#include "list_stage.hip.h"
#include "../../include/rtrec_amd.h"

namespace rtrec {

struct ExplainRow {
    const int32_t *col;     // the row's entries in memory: [0, len)
    const float *val;
    int len;
    bool in_regs;           // len <= 64: lane l holds entry l (INT32_MAX beyond len) in reg_col / reg_val
    int reg_col;
    float reg_val;
};

// The candidate of column entry (j, w): id = j on a hit whose product is a number, -1 otherwise; `hit` says whether j is
// stored in the row at all (the support counts hits).  aux = ~j: among equal contributions the LOWER item id wins
// (cand_better prefers the larger aux).  Called by all 64 lanes together (the register search shuffles).
__device__ __forceinline__ Cand<float> explain_probe(const ExplainRow &row, bool valid, int j, float w, bool &hit) {
    Cand<float> x; x.id = -1; x.score = -__builtin_huge_valf(); x.aux = 0u;
    hit = false;
    float xv = 0.0f;
    if (row.in_regs) {
        int pos = 0;                                                      // number of row entries < j (<= 63 when j is present)
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
            const int v = __shfl(row.reg_col, pos + step - 1, 64);
            if (v < j) pos += step;
        }
        const int c = __shfl(row.reg_col, pos, 64);
        xv = __shfl(row.reg_val, pos, 64);
        hit = valid && c == j;
    } else if (valid) {
        int lo = 0, hi = row.len;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            const int m = row.col[mid];
            if (m == j) { hit = true; xv = row.val[mid]; break; }
            if (m < j) lo = mid + 1; else hi = mid;
        }
    }
    if (hit) {
        const float c = __fmul_rn(xv, w);
        if (c == c) { x.id = j; x.score = c; x.aux = 0xffffffffu - static_cast<uint32_t>(j); }
    }
    return x;
}

__global__ __launch_bounds__(64) void explain_topk_kernel(
        int n_rows, const int32_t *__restrict__ row_ids, const int32_t *__restrict__ xb_ptr, const int32_t *__restrict__ xb_col,
        const float *__restrict__ xb_val, int n_x_rows, long long xb_nnz, int n_items, const int32_t *__restrict__ wc_ptr,
        const int32_t *__restrict__ wc_row, const float *__restrict__ wc_val, long long wc_nnz, const int32_t *__restrict__ ids,
        long long ids_stride, int list_k, const int32_t *__restrict__ counts, int top_m, int32_t *__restrict__ out_items,
        float *__restrict__ out_contrib, int32_t *__restrict__ out_support) {
    const int lane = lane_id();
    const float ninf = -__builtin_huge_valf();
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        ExplainRow row;
        long long b;
        row.len = csr_row(xb_ptr, row_behind(row_ids, r), n_x_rows, xb_nnz, b);
        row.col = xb_col + b; row.val = xb_val + b;
        row.in_regs = row.len <= 64;
        row.reg_col = 0x7fffffff; row.reg_val = 0.0f;
        if (row.in_regs && lane < row.len) { row.reg_col = row.col[lane]; row.reg_val = row.val[lane]; }
        const int cnt = clamp_count(counts[r], list_k);
        for (int p = 0; p < list_k; ++p) {
            const int item = p < cnt ? ids[r * ids_stride + p] : -1;
            long long s = 0, e = 0;
            if (item >= 0 && item < n_items && row.len > 0) {
                s = wc_ptr[item]; e = wc_ptr[item + 1];
                clamp_span(s, e, wc_nnz);
            }
            const bool one = e - s <= 64;                                 // the whole column in one probe: keep it in registers
            Cand<float> mine; mine.id = -1; mine.score = ninf; mine.aux = 0u;
            int support = 0;
            if (one && e > s) {
                const bool valid = s + lane < e;
                bool hit;
                mine = explain_probe(row, valid, valid ? wc_row[s + lane] : -1, valid ? wc_val[s + lane] : 0.0f, hit);
                support = __popcll(__ballot(hit));
            }
            Cand<float> last; last.id = -1; last.score = ninf; last.aux = 0u;
            int my_id = -1;
            float my_c = ninf;
            for (int m = 0; m < top_m && e > s && (m < support || (m == 0 && !one)); ++m) {
                Cand<float> b; b.id = -1; b.score = ninf; b.aux = 0u;
                if (one) {
                    if (!(last.id >= 0 && !cand_better(last, mine))) b = mine;
                } else {
                    for (long long base = s; base < e; base += 64) {
                        const bool valid = base + lane < e;
                        bool hit;
                        const Cand<float> x = explain_probe(row, valid, valid ? wc_row[base + lane] : -1, valid ? wc_val[base + lane] : 0.0f, hit);
                        if (m == 0) support += __popcll(__ballot(hit));
                        if (last.id >= 0 && !cand_better(last, x)) continue;
                        if (cand_better(x, b)) b = x;
                    }
                }
                const Cand<float> w = wave_best(b);
                if (w.id < 0) break;
                last = w;
                if (lane == m) { my_id = w.id; my_c = w.score; }
            }
            const long long slot = r * list_k + p;
            if (lane < top_m) { out_items[slot * top_m + lane] = my_id; out_contrib[slot * top_m + lane] = my_c; }
            if (lane == 0) out_support[slot] = support;
        }
    }
}

}  // namespace rtrec

using namespace rtrec;

extern "C" int rtrec_slim_explain_topk(int32_t n_rows, const int32_t *d_row_ids, const int32_t *d_xb_ptr, const int32_t *d_xb_col,
                                       const float *d_xb_val, int32_t n_x_rows, int64_t xb_nnz, int32_t n_items,
                                       const int32_t *d_wc_ptr, const int32_t *d_wc_row, const float *d_wc_val, int64_t wc_nnz,
                                       const int32_t *d_ids, int64_t ids_stride, int32_t list_k, const int32_t *d_counts,
                                       int32_t top_m, int32_t *d_out_items, float *d_out_contrib, int32_t *d_out_support,
                                       void *stream) {
    if (n_rows < 0 || n_x_rows < 0 || xb_nnz < 0 || n_items < 0 || wc_nnz < 0) return RTREC_ERR_INVALID_ARG;
    if (list_k < 1 || list_k > 64 || top_m < 1 || top_m > 32) return RTREC_ERR_UNSUPPORTED;
    if (ids_stride < list_k) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_ids || !d_counts || !d_out_items || !d_out_contrib || !d_out_support) return RTREC_ERR_INVALID_ARG;
    if (!csr_present(n_x_rows, d_xb_ptr, xb_nnz, d_xb_col, d_xb_val)) return RTREC_ERR_INVALID_ARG;
    if (!csc_present(n_items, d_wc_ptr, wc_nnz, d_wc_row, d_wc_val)) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    hipLaunchKernelGGL(explain_topk_kernel, dim3(list_grid(n_rows)), dim3(64), 0, static_cast<hipStream_t>(stream), n_rows, d_row_ids,
                       d_xb_ptr, d_xb_col, d_xb_val, n_x_rows, static_cast<long long>(xb_nnz), n_items, d_wc_ptr, d_wc_row, d_wc_val,
                       static_cast<long long>(wc_nnz), d_ids, static_cast<long long>(ids_stride), list_k, d_counts, top_m, d_out_items,
                       d_out_contrib, d_out_support);
    return rtrec::launch_status();
}
