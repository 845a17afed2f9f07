// rtrec_amd/csrc/blend.hip -- blended lists: the union of two per-row lists by item id, each min-max normalised, the second one
// weighted per item, ranked by the summed value.
//
// The reference's hybrid model merges SLIM's list with a second scorer's in Python, one user at a time over dicts
// (HybridSlimFM._ensemble_by_scores); here both lists are taken where they lie in HBM.  The contract is the comment of
// rtrec_slim_blend_lists in include/rtrec_amd_ext.h; in short, with A the other scorer's list and B SLIM's:
//   length      a list ends at its count, or at its first position whose id lies outside [0, n_items) or whose score is not
//               finite or is <= -FLT_MAX
//   norm[p]     fl(fl(s[p] - mn) / fl(fl(mx - mn) + 1e-8f)), the division correctly rounded (__fdiv_rn), denormals kept
//   weight      of item i of B: weight_b, or (float)((2.0 * n) / (n + k)) in float64 with n = the count stored for (row, i), else
//               1 if X's row stores i, else 0
//   union       A's distinct ids by first appearance, each with the normalised score of its LAST appearance; then the ids only
//               B holds by first appearance, from +0.0f; every B position q adds fl(w * normB[q]) in ascending q, one rounded
//               multiply and one rounded add each (-ffp-contract=off: never fused); with mnz the entries of both lists double
//   order       the larger value first, among == values the earlier entry of the union; a NaN value is never listed
//
// Mapping (the frame is list_stage.hip.h's).  Ids and scores of both lists go to LDS; the two
// effective lengths and then the four extremes are found by a reduction (__shfl_xor inside a wave, one LDS slot per wave across
// the workgroup: min and max of floats do not depend on the order they are taken in).  After that the positions of both lists
// are numbered through, e = p for A and na + q for B, and thread t owns e = t, t + NT, ...: the owner looks for its id at the
// other positions (all reads, as in list_quality_kernel: whether a position is an entry is a function of the ids alone), and
// the owner of an entry adds its B terms in ascending q -- so a value is one thread's chain, whatever the wave count.  The
// contact lookup is a binary search in the count row, then in X's row (row_lookup.hip.h), once per entry B touches.  The values
// go to LDS (NaN: not an entry) and the ranking is by counting as in score_pairs_kernel: an entry's rank is the number of
// entries that beat it, read four at a time at wave-uniform addresses; the order is strict, so ranks are unique -- no sort, no
// atomics, nothing that depends on scheduling.
// On two lists of 10 twenty lanes of a wave work and each scans twenty ids: the kernel is bound by the latency of its few
// dependent loads (ids and scores, then the two binary searches per entry), like explain_topk_kernel; the LDS
// arrays are sized by the longer list (64 / 256 / 1024 positions, 24 bytes each), so short lists keep 32 one-wave workgroups
// per CU and occupancy hides the latency.  No other mapping has been measured.
// Malformed input cannot read out of range: CSR offsets are clamped to the arrays' lengths, counts to [0, ka] / [0, kb], a row id
// outside [0, n_x_rows) is an empty row, and an id outside [0, n_items) ends its list.
#include "list_stage.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {
namespace {

constexpr int kBlendMaxList = 1024;     // ka / kb limit: the LDS arrays of the widest instantiation
constexpr float kBlendFltMax = 3.402823466e+38f;

// the smallest / largest of v over the workgroup, the same in every thread; `slot` holds one entry per wave and is free again
// after the call's second barrier
template <int WAVES, bool MAX, typename T>
__device__ __forceinline__ T blend_reduce(T v, T *slot, int tid) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const T o = shfl_xor_t(v, m);
        if (MAX ? o > v : o < v) v = o;
    }
    if constexpr (WAVES > 1) {
        __syncthreads();                // the slots' last readers are done
        if ((tid & 63) == 0) slot[tid >> 6] = v;
        __syncthreads();
        v = slot[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) { const T o = slot[w]; if (MAX ? o > v : o < v) v = o; }
    }
    return v;
}

template <int WAVES, int CAP>
__global__ __launch_bounds__(WAVES * 64) void blend_lists_kernel(
        int n_rows, int n_items, const int32_t *__restrict__ a_ids, long long a_ids_stride, const float *__restrict__ a_scores,
        long long a_scores_stride, const int32_t *__restrict__ a_counts, int ka, const int32_t *__restrict__ b_ids,
        long long b_ids_stride, const float *__restrict__ b_scores, long long b_scores_stride, const int32_t *__restrict__ b_counts,
        int kb, int keep, float weight_b, int contacts, double k, int mnz, const int32_t *__restrict__ row_ids,
        const int32_t *__restrict__ xb_ptr, const int32_t *__restrict__ xb_col, int n_x_rows, long long xb_nnz,
        const int32_t *__restrict__ cn_ptr, const int32_t *__restrict__ cn_col, const int32_t *__restrict__ cn_val, long long cn_nnz,
        int32_t *__restrict__ out_ids, float *__restrict__ out_value, int32_t *__restrict__ out_source,
        int32_t *__restrict__ out_count) {
    constexpr int NT = WAVES * 64;
    __shared__ int32_t lida[CAP];       // A: the position's item, -1: an invalid position
    __shared__ int32_t lidb[CAP];
    __shared__ float lna[CAP];          // A: the score, then its normalised value
    __shared__ float lnb[CAP];
    __shared__ __attribute__((aligned(16))) float lval[2 * CAP];    // the union's values by e (NaN: not an entry, or a NaN value)
    __shared__ int islot[WAVES];
    __shared__ float fslot[WAVES];
    const int tid = static_cast<int>(threadIdx.x);
    const float inf = __builtin_huge_valf(), nan = __builtin_nanf("");
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int ca = clamp_count(a_counts[r], ka), cb = clamp_count(b_counts[r], kb);
        // ---- both lists to LDS; a list ends in front of its first invalid position
        int na = ca, nb = cb;
        for (int p = tid; p < ca; p += NT) {
            const int id = a_ids[r * a_ids_stride + p];
            const float s = a_scores[r * a_scores_stride + p];
            const bool ok = id >= 0 && id < n_items && __builtin_fabsf(s) < inf && s > -kBlendFltMax;     // (false for a NaN score)
            lida[p] = ok ? id : -1;
            lna[p] = s;
            if (!ok && p < na) na = p;
        }
        for (int q = tid; q < cb; q += NT) {
            const int id = b_ids[r * b_ids_stride + q];
            const float s = b_scores[r * b_scores_stride + q];
            const bool ok = id >= 0 && id < n_items && __builtin_fabsf(s) < inf && s > -kBlendFltMax;
            lidb[q] = ok ? id : -1;
            lnb[q] = s;
            if (!ok && q < nb) nb = q;
        }
        na = blend_reduce<WAVES, false>(na, islot, tid);
        nb = blend_reduce<WAVES, false>(nb, islot, tid);
        __syncthreads();                // ids and scores are in LDS
        // ---- the extremes over the effective positions (an empty list leaves +inf / -inf behind: nobody reads them)
        float mna = inf, mxa = -inf, mnb = inf, mxb = -inf;
        for (int p = tid; p < na; p += NT) { const float s = lna[p]; mna = s < mna ? s : mna; mxa = s > mxa ? s : mxa; }
        for (int q = tid; q < nb; q += NT) { const float s = lnb[q]; mnb = s < mnb ? s : mnb; mxb = s > mxb ? s : mxb; }
        mna = blend_reduce<WAVES, false>(mna, fslot, tid);
        mxa = blend_reduce<WAVES, true>(mxa, fslot, tid);
        mnb = blend_reduce<WAVES, false>(mnb, fslot, tid);
        mxb = blend_reduce<WAVES, true>(mxb, fslot, tid);
        const float dena = __fadd_rn(__fsub_rn(mxa, mna), 1e-8f), denb = __fadd_rn(__fsub_rn(mxb, mnb), 1e-8f);
        for (int p = tid; p < na; p += NT) lna[p] = __fdiv_rn(__fsub_rn(lna[p], mna), dena);     // (each position by its loader)
        for (int q = tid; q < nb; q += NT) lnb[q] = __fdiv_rn(__fsub_rn(lnb[q], mnb), denb);
        // ---- the row of X and of the count CSR behind this list (contacts only)
        const int32_t *xcol = xb_col, *ccol = cn_col, *cval = cn_val;
        int xlen = 0, clen = 0;
        if (contacts) {
            const long long u = row_behind(row_ids, r);
            long long s;
            xlen = csr_row(xb_ptr, u, n_x_rows, xb_nnz, s);
            xcol = xb_col + s;
            if (cn_ptr) {
                clen = csr_row(cn_ptr, u, n_x_rows, cn_nnz, s);
                ccol = cn_col + s; cval = cn_val + s;
            }
        }
        // the weight of item `id` of B
        auto weight_of = [&](int id) -> float {
            if (!contacts) return weight_b;
            int n = 0, pos;
            if (find_sorted(ccol, clen, id, pos)) n = cval[pos];
            else if (find_sorted(xcol, xlen, id, pos)) n = 1;
            if (n <= 0) return 0.0f;
            const double dn = static_cast<double>(n);
            return static_cast<float>(__ddiv_rn(__dmul_rn(2.0, dn), __dadd_rn(dn, k)));
        };
        const int ne = na + nb, ne4 = (ne + 3) & ~3;
        __syncthreads();                // the normalised values are in LDS
        // ---- the union: e = p for A, na + q for B; the owner of an entry adds its B terms in ascending q
        int listed = 0;
        for (int base = 0; base < ne4; base += NT) {            // (the trip count is the same for every thread: the ballot below)
            const int e = base + tid;
            float v = nan;
            if (e < na) {
                const int id = lida[e];
                bool first = true;
                for (int p = 0; p < e; ++p) if (lida[p] == id) { first = false; break; }
                if (first) {
                    int last = e;
                    for (int p = e + 1; p < na; ++p) if (lida[p] == id) last = p;
                    v = lna[last];
                    bool both = false;
                    float w = 0.0f;
                    for (int q = 0; q < nb; ++q) {
                        if (lidb[q] != id) continue;
                        if (!both) { w = weight_of(id); both = true; }
                        v = __fadd_rn(v, __fmul_rn(w, lnb[q]));
                    }
                    if (both && mnz) v = __fmul_rn(v, 2.0f);
                }
            } else if (e < ne) {
                const int q0 = e - na, id = lidb[q0];
                bool first = true;
                for (int p = 0; p < na; ++p) if (lida[p] == id) { first = false; break; }
                if (first) for (int q = 0; q < q0; ++q) if (lidb[q] == id) { first = false; break; }
                if (first) {
                    const float w = weight_of(id);
                    v = 0.0f;
                    for (int q = q0; q < nb; ++q) if (lidb[q] == id) v = __fadd_rn(v, __fmul_rn(w, lnb[q]));
                }
            }
            if (e < ne4) lval[e] = v;
            listed += __popcll(__ballot(v == v));
        }
        __syncthreads();                // all values are in LDS; the slots' last readers are done
        listed = block_sum<WAVES>(listed, islot, tid);
        const int n_out = listed < keep ? listed : keep;
        // ---- rank by counting
        for (int e = tid; e < ne; e += NT) {
            const float v = lval[e];
            if (v != v) continue;
            const int rank = rank_by_count<false>(lval, ne4, e, v);       // among == values the earlier entry first
            if (rank < keep) {
                const int id = e < na ? lida[e] : lidb[e - na];
                int src = 2;
                if (e < na) {
                    src = 1;
                    for (int q = 0; q < nb; ++q) if (lidb[q] == id) { src = 3; break; }
                }
                out_ids[r * keep + rank] = id;
                out_value[r * keep + rank] = v;
                out_source[r * keep + rank] = src;
            }
        }
        for (int t = n_out + tid; t < keep; t += NT) {
            out_ids[r * keep + t] = -1;
            out_value[r * keep + t] = -inf;
            out_source[r * keep + t] = 0;
        }
        if (tid == 0) out_count[r] = n_out;
        __syncthreads();                // the row is done: LDS may be overwritten
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_slim_blend_lists(int32_t n_rows, int32_t n_items, const int32_t *d_a_ids, int64_t a_ids_stride,
                                      const float *d_a_scores, int64_t a_scores_stride, const int32_t *d_a_counts, int32_t ka,
                                      const int32_t *d_b_ids, int64_t b_ids_stride, const float *d_b_scores, int64_t b_scores_stride,
                                      const int32_t *d_b_counts, int32_t kb, int32_t keep, float weight_b, int32_t weight_mode,
                                      double k, int32_t mnz, const int32_t *d_row_ids, const int32_t *d_xb_ptr,
                                      const int32_t *d_xb_col, int32_t n_x_rows, int64_t xb_nnz, const int32_t *d_cn_ptr,
                                      const int32_t *d_cn_col, const int32_t *d_cn_val, int64_t cn_nnz, int32_t waves_per_row,
                                      int32_t *d_out_ids, float *d_out_value, int32_t *d_out_source, int32_t *d_out_count,
                                      void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_items < 0 || n_x_rows < 0 || xb_nnz < 0 || cn_nnz < 0) return RTREC_ERR_INVALID_ARG;
    if (ka < 1 || ka > kBlendMaxList || kb < 1 || kb > kBlendMaxList || keep < 1 || keep > ka + kb) return RTREC_ERR_UNSUPPORTED;
    if (!list_waves_valid(waves_per_row)) return RTREC_ERR_UNSUPPORTED;
    if (weight_mode != RTREC_BLEND_CONSTANT && weight_mode != RTREC_BLEND_CONTACTS) return RTREC_ERR_UNSUPPORTED;
    if (a_ids_stride < ka || a_scores_stride < ka || b_ids_stride < kb || b_scores_stride < kb) return RTREC_ERR_INVALID_ARG;
    if (!(weight_b >= 0.0f) || !(k >= 0.0)) return RTREC_ERR_INVALID_ARG;                  // (a NaN fails the compare)
    if (n_rows == 0) return RTREC_OK;
    if (!d_a_ids || !d_a_scores || !d_a_counts || !d_b_ids || !d_b_scores || !d_b_counts) return RTREC_ERR_INVALID_ARG;
    if (!d_out_ids || !d_out_value || !d_out_source || !d_out_count) return RTREC_ERR_INVALID_ARG;
    const int contacts = weight_mode == RTREC_BLEND_CONTACTS;
    if (contacts) {
        if (!csr_present(n_x_rows, d_xb_ptr, xb_nnz, d_xb_col, d_xb_col)) return RTREC_ERR_INVALID_ARG;      // (X comes without values)
        if (d_cn_ptr && !csr_present(0, d_cn_ptr, cn_nnz, d_cn_col, d_cn_val)) return RTREC_ERR_INVALID_ARG;
    }
    (void)hipGetLastError();
    const int longer = ka > kb ? ka : kb;
    hipStream_t st = static_cast<hipStream_t>(stream);
    list_dispatch(list_waves(waves_per_row, n_rows, longer), longer, [&](auto W, auto CAP) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_lists_kernel<W(), CAP()>), dim3(list_grid(n_rows)), dim3(W() * 64), 0, st, n_rows, n_items,
                           d_a_ids, static_cast<long long>(a_ids_stride), d_a_scores, static_cast<long long>(a_scores_stride), d_a_counts,
                           ka, d_b_ids, static_cast<long long>(b_ids_stride), d_b_scores, static_cast<long long>(b_scores_stride),
                           d_b_counts, kb, keep, weight_b, contacts, k, mnz != 0 ? 1 : 0, d_row_ids, d_xb_ptr, d_xb_col, n_x_rows,
                           static_cast<long long>(xb_nnz), d_cn_ptr, d_cn_col, d_cn_val, static_cast<long long>(cn_nnz), d_out_ids,
                           d_out_value, d_out_source, d_out_count);
    });
    return launch_status();
}
