// rtrec_amd/csrc/diversify.hip -- diversified lists: greedy MMR re-rank of per-row lists, with W as the item-item similarity.
//
// A list ranked by score alone tends to be the neighbours of the two or three items the user rated.  This stage trades the score
// against the similarity to what is already chosen.  The contract is the comment of rtrec_slim_diversify_lists in
// include/rtrec_amd_ext.h; in short:
//   competing   a position below counts[r] whose id lies in [0, n_items), whose score is finite and whose item no chosen position
//               holds
//   sim(a, b)   max(|W[a, b]|, |W[b, a]|) over the stored weights (0 where none is stored); a NaN weight is ignored
//   step t      v[p] = fl(fl(lambda * score[p]) - fl((1 - lambda) * pen[p])), three rounded operations (-ffp-contract=off: never
//               fused); the winner is the largest v, the EARLIER position among == values (lists arrive best first); a NaN v is
//               skipped; afterwards pen[p] = max(pen[p], sim(id[p], id[winner])) for every other competing position
//
// Mapping (the frame is list_stage.hip.h's).  Thread t owns the positions t, t + NT, ...: their
// ids (-1 once a position does not compete any more), lambda * score and penalties live in LDS and are written by their owner
// only.  A step is an arg-max (each thread over its positions, __shfl_xor across the wave, one LDS slot per wave across the
// workgroup) under a strict order, so the winner is unique and nothing depends on scheduling or on the wave count; then the
// winner's column of W is staged in LDS (up to kDivStage entries; a longer column is searched in global memory, so a column of
// any length works) and every thread updates its positions with two binary searches: id[p] in the winner's column, the winner
// in column id[p].  The kernel is bound by the latency of those dependent loads, like explain_topk_kernel: the LDS
// arrays are sized by the list (64 / 256 / 1024 positions), so that lists of up to 256 keep 32 one-wave workgroups per CU
// (3 KiB + 1 KiB of staged column each) and occupancy hides the latency.
// Malformed input cannot read out of range: CSC offsets are clamped to [0, wc_nnz], counts to [0, list_k], and an id outside
// [0, n_items) never competes.
#include "list_stage.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {
namespace {

constexpr int kDivMaxList = 1024;       // list_k limit: the LDS arrays of the widest instantiation
constexpr int kDivStage = 128;          // entries of the winner's column staged in LDS per step

// a beats b: the larger value, among == values the earlier position (p < 0: no candidate)
__device__ __forceinline__ bool div_beats(float va, int pa, float vb, int pb) {
    if (pa < 0) return false;
    if (pb < 0) return true;
    return va > vb || (va == vb && pa < pb);
}

template <int WAVES, int CAP>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_num_sgpr(80))) void diversify_lists_kernel(
        int n_rows, int n_items, const int32_t *__restrict__ wc_ptr, const int32_t *__restrict__ wc_row,
        const float *__restrict__ wc_val, long long wc_nnz, const int32_t *__restrict__ ids, long long ids_stride,
        const float *__restrict__ scores, long long scores_stride, int list_k, const int32_t *__restrict__ counts, int keep,
        float lambda, int32_t *__restrict__ out_order, float *__restrict__ out_value, float *__restrict__ out_penalty,
        int32_t *__restrict__ out_count) {
    constexpr int NT = WAVES * 64;
    __shared__ int32_t lid[CAP];        // the position's item, -1: it does not compete (any more)
    __shared__ float lsc[CAP];          // fl(lambda * score)
    __shared__ float lpen[CAP];
    __shared__ int32_t crow[kDivStage];
    __shared__ float cval[kDivStage];
    __shared__ float slot_v[WAVES];     // the waves' winners of a step (read before the step's second barrier, written after it)
    __shared__ int slot_p[WAVES];
    const int tid = static_cast<int>(threadIdx.x);
    const float oml = __fsub_rn(1.0f, lambda);
    const float inf = __builtin_huge_valf();
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int cnt = clamp_count(counts[r], list_k);
        for (int p = tid; p < list_k; p += NT) {
            int id = -1;
            float s = 0.0f;
            if (p < cnt) { id = ids[r * ids_stride + p]; s = scores[r * scores_stride + p]; }
            const bool ok = id >= 0 && id < n_items && __builtin_fabsf(s) < inf;       // (false for a NaN score too)
            lid[p] = ok ? id : -1;
            lsc[p] = __fmul_rn(lambda, s);
            lpen[p] = 0.0f;
        }
        __syncthreads();
        int n_out = 0;
        for (int t = 0; t < keep; ++t) {
            // ---- arg-max over the competing positions; a thread walks its positions upwards, so > keeps the earlier one
            float best = 0.0f;
            int bpos = -1;
            for (int p = tid; p < list_k; p += NT) {
                if (lid[p] < 0) continue;
                const float v = __fsub_rn(lsc[p], __fmul_rn(oml, lpen[p]));
                if (v != v) continue;
                if (bpos < 0 || v > best) { best = v; bpos = p; }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const float ov = __shfl_xor(best, m, 64);
                const int op = __shfl_xor(bpos, m, 64);
                if (div_beats(ov, op, best, bpos)) { best = ov; bpos = op; }
            }
            if constexpr (WAVES > 1) {
                if ((tid & 63) == 0) { slot_v[tid >> 6] = best; slot_p[tid >> 6] = bpos; }
                __syncthreads();        // the waves' winners are in their slots; the last step's penalties are written
                best = slot_v[0]; bpos = slot_p[0];
#pragma unroll
                for (int w = 1; w < WAVES; ++w)
                    if (div_beats(slot_v[w], slot_p[w], best, bpos)) { best = slot_v[w]; bpos = slot_p[w]; }
            }
            if (bpos < 0) break;        // (the same in every thread) nothing competes with a value that is a number
            const int c = bpos;
            const int idc = lid[c];
            const float penc = lpen[c];
            if (tid == 0) {
                out_order[r * keep + t] = c;
                out_value[r * keep + t] = best;
                out_penalty[r * keep + t] = penc;
            }
            n_out = t + 1;
            if (n_out == keep) break;   // (the same in every thread) no step follows: nobody would read the raised penalties
            // ---- the winner's column of W, staged while it fits
            long long cs = wc_ptr[idc], ce = wc_ptr[idc + 1];
            clamp_span(cs, ce, wc_nnz);
            const int clen = span_len(cs, ce);
            const bool staged = clen <= kDivStage;
            if (staged) for (int q = tid; q < clen; q += NT) { crow[q] = wc_row[cs + q]; cval[q] = wc_val[cs + q]; }
            __syncthreads();            // the column is staged; every thread has read the slots, the winner's id and its penalty
            // ---- the winner and its duplicates leave, the others' penalties rise
            for (int p = tid; p < list_k; p += NT) {
                const int idp = lid[p];
                if (idp < 0) continue;
                if (idp == idc) { lid[p] = -1; continue; }
                float pen = lpen[p], w;
                if (staged ? find_sorted(crow, cval, clen, idp, w) : find_sorted(wc_row + cs, wc_val + cs, clen, idp, w))
                    raise_abs(pen, w);                                    // W[id[p], winner]
                long long s = wc_ptr[idp], e = wc_ptr[idp + 1];
                clamp_span(s, e, wc_nnz);
                const int len = span_len(s, e);
                if (find_sorted(wc_row + s, wc_val + s, len, idc, w)) raise_abs(pen, w);    // W[winner, id[p]]
                lpen[p] = pen;
            }
        }
        for (int t = n_out + tid; t < keep; t += NT) {
            out_order[r * keep + t] = -1;
            out_value[r * keep + t] = -inf;
            out_penalty[r * keep + t] = -inf;
        }
        if (tid == 0) out_count[r] = n_out;
        __syncthreads();                // the row is done: LDS may be overwritten
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_slim_diversify_lists(int32_t n_rows, int32_t n_items, const int32_t *d_wc_ptr, const int32_t *d_wc_row,
                                          const float *d_wc_val, int64_t wc_nnz, const int32_t *d_ids, int64_t ids_stride,
                                          const float *d_scores, int64_t scores_stride, int32_t list_k, const int32_t *d_counts,
                                          int32_t keep, float lambda, int32_t waves_per_row, int32_t *d_out_order,
                                          float *d_out_value, float *d_out_penalty, int32_t *d_out_count, void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_items < 0 || wc_nnz < 0) return RTREC_ERR_INVALID_ARG;
    if (list_k < 1 || list_k > kDivMaxList || keep < 1 || keep > list_k) return RTREC_ERR_UNSUPPORTED;
    if (!list_waves_valid(waves_per_row)) return RTREC_ERR_UNSUPPORTED;
    if (ids_stride < list_k || scores_stride < list_k) return RTREC_ERR_INVALID_ARG;
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return RTREC_ERR_INVALID_ARG;            // (a NaN lambda fails both compares)
    if (n_rows == 0) return RTREC_OK;
    if (!d_ids || !d_scores || !d_counts || !d_out_order || !d_out_value || !d_out_penalty || !d_out_count) return RTREC_ERR_INVALID_ARG;
    if (!csc_present(n_items, d_wc_ptr, wc_nnz, d_wc_row, d_wc_val)) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long nnz = static_cast<long long>(wc_nnz), is = static_cast<long long>(ids_stride), ss = static_cast<long long>(scores_stride);
    list_dispatch(list_waves(waves_per_row, n_rows, list_k), list_k, [&](auto W, auto CAP) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(diversify_lists_kernel<W(), CAP()>), dim3(list_grid(n_rows)), dim3(W() * 64), 0, st, n_rows,
                           n_items, d_wc_ptr, d_wc_row, d_wc_val, nnz, d_ids, is, d_scores, ss, list_k, d_counts, keep, lambda,
                           d_out_order, d_out_value, d_out_penalty, d_out_count);
    });
    return launch_status();
}
