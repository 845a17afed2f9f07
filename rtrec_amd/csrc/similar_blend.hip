// rtrec_amd/csrc/similar_blend.hip -- the blend behind the hybrid's similar_items: two per-row lists, cut, the query taken out,
// the first divided by the query's norm, each min-max normalised in float32, summed per item id in FLOAT64, ranked.
//
// The reference's hybrid model does this in Python per query (HybridSlimFM._similar_items, steps after implicit.topk: the cut at
// -FLT_MAX, / ||q||, the id mask, minmax_normalize, comb_sum into a defaultdict(float), sorted(reverse=True)[:top_k]).  The
// contract is the comment of rtrec_similar_blend in include/rtrec_amd_ext.h; in short, with A the factor list and B SLIM's:
//   length      a list ends at its count, or at its first position whose id lies outside [0, n_items) or whose RAW score is not
//               finite or is <= -FLT_MAX (blend_lists' rule, applied before any division, as the reference cuts)
//   exclude     what remains loses every entry whose id == exclude[r]
//   divide      A's scores become fl(s / a_div[r]) (__fdiv_rn); a divisor that is not > 0 empties A
//   norm[p]     fl(fl(s[p] - mn) / fl(fl(mx - mn) + 1e-8f)) per non-empty list: blend_lists' float32 form; an EMPTY list
//               contributes nothing (the reference raises ValueError from min([]) there)
//   union       A's distinct ids by first appearance, then the ids only B holds; the value is a float64: 0.0, then
//               + (double)normA[p] for EVERY occurrence in A in ascending p, then + (double)normB[q] for every occurrence in B in
//               ascending q, each addition rounded to float64
//   order       the larger value first, equal values keep the union's order (Python's stable sort); a NaN is never listed
// THIS IS NOT rtrec_slim_blend_lists: that one adds in float32, weights B per item and lets an id repeated inside A keep the
// score of its LAST occurrence (dict(zip(ids, scores))); here a repeat adds once per occurrence, as comb_sum's += does, and the
// sum is a double -- on the golden cases float32 addition changes values on most rows and the order on some.
//
// Mapping (the frame is list_stage.hip.h's: one row per workgroup of 1 or 4 waves, grid-stride over the rows).  Ids and scores of
// both lists go to LDS; an excluded position becomes a HOLE (id -2) instead of being squeezed out: a hole is skipped by the
// extremes, never matches an id and is never an entry, and since ranks only compare positions the order is the one a compacted
// list would give.  Lengths, live counts and the four extremes are reductions (min / max / integer sums: independent of the
// order they are taken in).  Positions are numbered through, e = p for A and na + q for B, thread t owns e = t, t + NT, ...; the
// owner of an entry walks both lists once and adds in the contract's order, so a value is one thread's chain whatever the wave
// count.  The double values go to LDS and every entry counts the entries that beat it (two doubles per 16-byte read at
// wave-uniform addresses: rank_by_count reads floats, so the loop stands here).  No atomics, nothing depends on scheduling.
// LDS: 32 bytes per position of the longer list (two ids, two floats, two doubles): 2 / 8 / 32 KiB for 64 / 256 / 1024.
// Like blend_lists_kernel it is bound by the latency of its few dependent loads on short lists; no other mapping was measured.
// Measured (profiles/similar_c3s.json, tools/similar_bench.py; MI355X, 26,744 rows, medians of 10): two lists of 10 in 0.06 ms
// behind a cosine top-k of 2.15 ms and W's column top-k (2.7 ms for the three calls), two lists of 100 in 0.4 ms (about 30 ms for
// the three calls); the vectorised host model needs about 13 ms for 200 of the rows at 10.
// Malformed input cannot read out of range: counts are clamped to [0, ka] / [0, kb] and ids are only compared, never indexed.
#include "list_stage.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {
namespace {

constexpr int kSimBlendMaxList = 1024;     // ka / kb limit: the LDS arrays of the widest instantiation
constexpr float kSimBlendFltMax = 3.402823466e+38f;
constexpr int kSimBlendHole = -2;          // an excluded position (a position behind the cut is never looked at)

// the smallest / largest of v over the workgroup, the same in every thread (blend.hip's blend_reduce)
template <int WAVES, bool MAX, typename T>
__device__ __forceinline__ T simblend_reduce(T v, T *slot, int tid) {
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
__global__ __launch_bounds__(WAVES * 64) void similar_blend_kernel(
        int n_rows, int n_items, const int32_t *__restrict__ a_ids, long long a_ids_stride, const float *__restrict__ a_scores,
        long long a_scores_stride, const int32_t *__restrict__ a_counts, int ka, const float *__restrict__ a_div,
        const int32_t *__restrict__ b_ids, long long b_ids_stride, const float *__restrict__ b_scores, long long b_scores_stride,
        const int32_t *__restrict__ b_counts, int kb, const int32_t *__restrict__ exclude, int keep,
        int32_t *__restrict__ out_ids, double *__restrict__ out_value, int32_t *__restrict__ out_source,
        int32_t *__restrict__ out_count) {
    constexpr int NT = WAVES * 64;
    __shared__ int32_t lida[CAP];       // A: the position's item, -1: an invalid position, -2: a hole
    __shared__ int32_t lidb[CAP];
    __shared__ float lna[CAP];          // A: the score, then its normalised value
    __shared__ float lnb[CAP];
    __shared__ __attribute__((aligned(16))) double lval[2 * CAP];   // the union's values by e (NaN: not an entry, or a NaN value)
    __shared__ int islot[WAVES];
    __shared__ float fslot[WAVES];
    const int tid = static_cast<int>(threadIdx.x);
    const float inf = __builtin_huge_valf();
    const double dnan = __builtin_nan(""), dninf = -__builtin_huge_val();
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int ca = clamp_count(a_counts[r], ka), cb = clamp_count(b_counts[r], kb);
        const int ex = exclude ? exclude[r] : -1;
        const float div = a_div ? a_div[r] : 1.0f;
        // ---- both lists to LDS; a list ends in front of its first invalid position (judged on the raw score)
        int na = ca, nb = cb;
        for (int p = tid; p < ca; p += NT) {
            const int id = a_ids[r * a_ids_stride + p];
            const float s = a_scores[r * a_scores_stride + p];
            const bool ok = id >= 0 && id < n_items && __builtin_fabsf(s) < inf && s > -kSimBlendFltMax;   // (false for a NaN score)
            lida[p] = ok ? (id == ex ? kSimBlendHole : id) : -1;
            lna[p] = a_div ? __fdiv_rn(s, div) : s;
            if (!ok && p < na) na = p;
        }
        for (int q = tid; q < cb; q += NT) {
            const int id = b_ids[r * b_ids_stride + q];
            const float s = b_scores[r * b_scores_stride + q];
            const bool ok = id >= 0 && id < n_items && __builtin_fabsf(s) < inf && s > -kSimBlendFltMax;
            lidb[q] = ok ? (id == ex ? kSimBlendHole : id) : -1;
            lnb[q] = s;
            if (!ok && q < nb) nb = q;
        }
        na = simblend_reduce<WAVES, false>(na, islot, tid);
        nb = simblend_reduce<WAVES, false>(nb, islot, tid);
        if (a_div && !(div > 0.0f)) na = 0;         // (a NaN divisor fails the compare)
        __syncthreads();                // ids and scores are in LDS
        // ---- the extremes over the live positions (a list without one leaves +inf / -inf behind: nobody reads them)
        float mna = inf, mxa = -inf, mnb = inf, mxb = -inf;
        for (int p = tid; p < na; p += NT) {
            if (lida[p] == kSimBlendHole) continue;
            const float s = lna[p]; mna = s < mna ? s : mna; mxa = s > mxa ? s : mxa;
        }
        for (int q = tid; q < nb; q += NT) {
            if (lidb[q] == kSimBlendHole) continue;
            const float s = lnb[q]; mnb = s < mnb ? s : mnb; mxb = s > mxb ? s : mxb;
        }
        mna = simblend_reduce<WAVES, false>(mna, fslot, tid);
        mxa = simblend_reduce<WAVES, true>(mxa, fslot, tid);
        mnb = simblend_reduce<WAVES, false>(mnb, fslot, tid);
        mxb = simblend_reduce<WAVES, true>(mxb, fslot, tid);
        const float dena = __fadd_rn(__fsub_rn(mxa, mna), 1e-8f), denb = __fadd_rn(__fsub_rn(mxb, mnb), 1e-8f);
        for (int p = tid; p < na; p += NT) lna[p] = __fdiv_rn(__fsub_rn(lna[p], mna), dena);     // (each position by its loader)
        for (int q = tid; q < nb; q += NT) lnb[q] = __fdiv_rn(__fsub_rn(lnb[q], mnb), denb);
        const int ne = na + nb, ne2 = (ne + 1) & ~1;
        __syncthreads();                // the normalised values are in LDS
        // ---- the union: e = p for A, na + q for B; the owner of an entry adds every occurrence, A's first, in ascending order
        int listed = 0;
        for (int base = 0; base < ne2; base += NT) {            // (the trip count is the same for every thread: the ballot below)
            const int e = base + tid;
            double v = dnan;
            if (e < na) {
                const int id = lida[e];
                bool first = id != kSimBlendHole;
                for (int p = 0; first && p < e; ++p) if (lida[p] == id) first = false;
                if (first) {
                    v = 0.0;
                    for (int p = e; p < na; ++p) if (lida[p] == id) v = __dadd_rn(v, static_cast<double>(lna[p]));
                    for (int q = 0; q < nb; ++q) if (lidb[q] == id) v = __dadd_rn(v, static_cast<double>(lnb[q]));
                }
            } else if (e < ne) {
                const int q0 = e - na, id = lidb[q0];
                bool first = id != kSimBlendHole;
                for (int p = 0; first && p < na; ++p) if (lida[p] == id) first = false;
                for (int q = 0; first && q < q0; ++q) if (lidb[q] == id) first = false;
                if (first) {
                    v = 0.0;
                    for (int q = q0; q < nb; ++q) if (lidb[q] == id) v = __dadd_rn(v, static_cast<double>(lnb[q]));
                }
            }
            if (e < ne2) lval[e] = v;
            listed += __popcll(__ballot(v == v));
        }
        __syncthreads();                // all values are in LDS; the slots' last readers are done
        listed = block_sum<WAVES>(listed, islot, tid);
        const int n_out = listed < keep ? listed : keep;
        // ---- rank by counting over the doubles: o beats v when it is larger, or == and earlier in the union
        for (int e = tid; e < ne; e += NT) {
            const double v = lval[e];
            if (v != v) continue;
            int rank = 0;
            for (int q = 0; q < ne2; q += 2) {
                const double2 o = *reinterpret_cast<const double2 *>(&lval[q]);
                rank += (o.x > v || (o.x == v && q < e)) ? 1 : 0;
                rank += (o.y > v || (o.y == v && q + 1 < e)) ? 1 : 0;
            }
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
            out_value[r * keep + t] = dninf;
            out_source[r * keep + t] = 0;
        }
        if (tid == 0) out_count[r] = n_out;
        __syncthreads();                // the row is done: LDS may be overwritten
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_similar_blend(int32_t n_rows, int32_t n_items, const int32_t *d_a_ids, int64_t a_ids_stride,
                                   const float *d_a_scores, int64_t a_scores_stride, const int32_t *d_a_counts, int32_t ka,
                                   const float *d_a_div, const int32_t *d_b_ids, int64_t b_ids_stride, const float *d_b_scores,
                                   int64_t b_scores_stride, const int32_t *d_b_counts, int32_t kb, const int32_t *d_exclude,
                                   int32_t keep, int32_t waves_per_row, int32_t *d_out_ids, double *d_out_value,
                                   int32_t *d_out_source, int32_t *d_out_count, void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_items < 0) return RTREC_ERR_INVALID_ARG;
    if (ka < 1 || ka > kSimBlendMaxList || kb < 1 || kb > kSimBlendMaxList || keep < 1 || keep > ka + kb) return RTREC_ERR_UNSUPPORTED;
    if (!list_waves_valid(waves_per_row)) return RTREC_ERR_UNSUPPORTED;
    if (a_ids_stride < ka || a_scores_stride < ka || b_ids_stride < kb || b_scores_stride < kb) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_a_ids || !d_a_scores || !d_a_counts || !d_b_ids || !d_b_scores || !d_b_counts) return RTREC_ERR_INVALID_ARG;
    if (!d_out_ids || !d_out_value || !d_out_source || !d_out_count) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    const int longer = ka > kb ? ka : kb;
    hipStream_t st = static_cast<hipStream_t>(stream);
    list_dispatch(list_waves(waves_per_row, n_rows, longer), longer, [&](auto W, auto CAP) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(similar_blend_kernel<W(), CAP()>), dim3(list_grid(n_rows)), dim3(W() * 64), 0, st, n_rows,
                           n_items, d_a_ids, static_cast<long long>(a_ids_stride), d_a_scores, static_cast<long long>(a_scores_stride),
                           d_a_counts, ka, d_a_div, d_b_ids, static_cast<long long>(b_ids_stride), d_b_scores,
                           static_cast<long long>(b_scores_stride), d_b_counts, kb, d_exclude, keep, d_out_ids, d_out_value,
                           d_out_source, d_out_count);
    });
    return launch_status();
}
