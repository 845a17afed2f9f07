// rtrec_amd/csrc/factor_similar.hip -- cosine top-k of item vectors against the whole catalogue, the query itself excluded.
//
// The reference's hybrid model answers "more like this" from its factor side with implicit.topk(items=target, query=q, k,
// item_norms=||target_i||, filter_items=[query]) (rtrec/models/hybrid.py, _similar_items): a float32 GEMM, every score divided by
// the item's norm, the query set to -FLT_MAX, a top-k, and later one division by ||q||.  This is that call for vectors that
// are resident; the contract is the comment of rtrec_factor_similar_topk in include/rtrec_amd_ext.h.  In short:
//   dot         +0.0f, then fmaf(q[c], v_i[c], dot) for c = 0 .. dim-1 ascending: rtrec_factor_topk's chain
//   s1          fl(dot / norms[i]): one correctly rounded division (__fdiv_rn), denormals kept -- what the list is ranked by
//   competing   0 <= i < n_items, i != q, the mask admits i, s1 is not NaN (so a zero vector never competes; +-inf do)
//   order       the larger s1 first, among == the lower id: strict
//   out         s1, or fl(s1 / norm_q) with write_cosine -- divided once, where the final list is written (the merge kernel
//               of a chunked call, the scan kernel otherwise), never on partial lists
//
// What is built.  The scan of factor_topk_kernel (factor_topk.hip), in a kernel of its own (factor_scan.hip.h says why; the
// limits, the strict order, the host plan and the dispatch are that header's): one wave per workgroup, 32 queries x one chunk of 32-item tiles, a tile is
// one chain of v_mfma_f32_32x32x2_f32 with the items as the A operand read straight from d_qt and the queries' vectors as B in
// ceil(dim / 2) VGPRs (classes of 8 / 32 / 128 for dim <= 16 / 64 / 256), a threshold in registers, a candidate buffer in LDS
// (CAP = 64 / 128 / 224 entries for top_k <= 16 / 64 / 128, rows CAP + 1 apart: 32 queries appending at one position hit 32
// banks), compaction ranks by counting.  Without brought vectors the B operand is gathered from d_qt's columns once per
// workgroup (dim strided loads per lane, before the first tile).  Only the epilogue differs: a lane loads the 16 item norms its
// accumulator registers map to (items tile + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): four runs of four neighbours), divides,
// compares s1 against the threshold, tests i != q and the mask, and appends.
// LDS per workgroup: 16.3 / 32.3 / 56.3 KiB for the three k-classes, factor_topk_kernel's budget.
// Measured (profiles/similar_c3s.json, tools/similar_bench.py; MI355X, all 26,744 items of c3s as queries x 26,744 items, seeded
// normal vectors, write_cosine, medians of 10; rounded so that repeated runs agree): top_k 10: 2.15 ms at dim 12 and 3.35 ms at
// dim 64 (8 / 27 TFLOP/s), against 8.9 / 9.2 ms for torch.matmul + the division by the norms + the diagonal + topk, interleaved in
// the same process; top_k 100: about 28 / 31 ms against 9.2 / 9.6 ms -- the fused kernel LOSES there as factor_topk_kernel does (a
// buffer cut to 100 is full again after some 93 survivors and one wave ranks one query), which is the scan's known weakness and
// not addressed here.  One query: about 0.5 ms with 64 chunks against about 3 ms with one at top_k 10 (dim 12), about 5 against 3 ms
// at top_k 100.  The lists equalled the host model on a 200-query sample, score bits included.
// Built: the plain form, every score is divided.  Not built: a conservative pre-test in front of the division (dot against
// threshold * norm with a margin); the division's share of the kernel is not measured, so there is nothing to justify it.
// Not tried: several waves per workgroup sharing the queries, staging d_qt or the norms through LDS, prefetching the next
// tile's A operand.  No variant was measured against this one.
// Malformed input cannot read out of range: a query outside [0, n_items) is a job without a vector (or, with brought vectors,
// excludes nothing), item ids are generated, never read, and norms / mask are read only for ids < n_items.
#include "factor_scan.hip.h"

namespace rtrec {
namespace {

// the norm of job r's query vector; +0.0f for a job without a vector
__device__ __forceinline__ float similar_query_norm(long long r, const int32_t *queries, const float *p_norms, const float *norms,
                                                    int n_items) {
    if (p_norms) return p_norms[r];
    const int q = queries[r];
    return (q >= 0 && q < n_items) ? norms[q] : 0.0f;
}

template <int DP, int CAP>
__global__ __launch_bounds__(64) void factor_similar_kernel(
        int n_rows, const int32_t *__restrict__ queries, const float *__restrict__ p, long long p_stride,
        const float *__restrict__ p_norms, const float *__restrict__ qt, long long qt_stride, int n_items, int dim,
        const float *__restrict__ norms, const uint8_t *__restrict__ item_mask, int top_k, int splits, int tiles_per_chunk,
        int write_cosine, int32_t *__restrict__ out_ids, float *__restrict__ out_scores, int32_t *__restrict__ out_count,
        float *__restrict__ out_div) {
    constexpr int LD = CAP + 1;                     // a query's row of the buffer
    constexpr int EPL = (CAP + 63) / 64;            // entries per lane in a compaction
    constexpr int G = DP < 16 ? DP : 16;            // k-steps whose A operands are in flight together
    __shared__ float lsc[32 * LD];
    __shared__ int32_t lid[32 * LD];
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const int np = (dim + 1) >> 1;
    const float ninf = -__builtin_huge_valf();
    // ---- this lane's query: the item it names, its vector and its norm
    const long long r = static_cast<long long>(blockIdx.x) * 32 + j;
    bool has = false;
    int q = -1;
    float qn = 0.0f;
    if (r < n_rows) {
        if (queries) q = queries[r];
        if (p) { has = true; qn = p_norms[r]; }
        else if (q >= 0 && q < n_items) { has = true; qn = norms[q]; }
    }
    float b[DP];
#pragma unroll
    for (int kk = 0; kk < DP; ++kk) {
        const int c = 2 * kk + h;                   // (a guard, not a break: the loop must unroll for b[] to stay in registers)
        b[kk] = 0.0f;
        if (kk < np && has && c < dim) b[kk] = p ? p[r * p_stride + c] : qt[c * qt_stride + q];
    }
    int count = 0;                                  // entries in this query's buffer (the same in both of its lanes)
    float ts = ninf;                                // the threshold: (-inf, INT_MAX) lets every number through
    int ti = 0x7fffffff;

    // the whole wave ranks query u's buffer and keeps its best top_k in slots 0 .. in order
    auto compact = [&](int u) {
        const int n = readlane_i(count, u);
        float es[EPL];
        int ei[EPL], rk[EPL];
#pragma unroll
        for (int t = 0; t < EPL; ++t) {
            const int e = lane + 64 * t;
            es[t] = e < n ? lsc[u * LD + e] : 0.0f;
            ei[t] = e < n ? lid[u * LD + e] : 0;
            rk[t] = 0;
        }
        for (int f = 0; f < n; ++f) {               // (wave-uniform addresses: LDS broadcasts)
            const float os = lsc[u * LD + f];
            const int oi = lid[u * LD + f];
#pragma unroll
            for (int t = 0; t < EPL; ++t) rk[t] += factor_beats(os, oi, es[t], ei[t]) ? 1 : 0;
        }
        __syncthreads();                            // every read of the old order is done
#pragma unroll
        for (int t = 0; t < EPL; ++t) {
            if (lane + 64 * t < n && rk[t] < top_k) { lsc[u * LD + rk[t]] = es[t]; lid[u * LD + rk[t]] = ei[t]; }
        }
        __syncthreads();
        const int nn = n < top_k ? n : top_k;
        if (j == u) {
            count = nn;
            if (nn == top_k) { ts = lsc[u * LD + top_k - 1]; ti = lid[u * LD + top_k - 1]; }
        }
    };

    // ---- the chunk's tiles
    const int n_tiles = (n_items + 31) >> 5;
    const long long t0 = static_cast<long long>(blockIdx.y) * tiles_per_chunk;
    long long t1 = t0 + tiles_per_chunk;
    if (t1 > n_tiles) t1 = n_tiles;
    for (long long t = t0; t < t1; ++t) {
        const int item0 = static_cast<int>(t) * 32;
        unsigned long long need = __ballot(count > CAP - 32);
        while (need) {
            const int u = readfirst_i(__ffsll(static_cast<long long>(need)) - 1) & 31;
            need &= ~((1ull << u) | (1ull << (u + 32)));
            compact(u);
        }
        // the A operand: component 2 kk + h of item item0 + j
        const int ia = item0 + j;
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < DP; kb += G) {        // G k-steps at a time: their loads are issued together, then the chain goes on
            if (kb < np) {
                float a[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int c = 2 * (kb + g) + h;
                    a[g] = (c < dim && ia < n_items) ? qt[c * qt_stride + ia] : 0.0f;
                }
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (kb + g < np) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g], b[kb + g], acc, 0, 0, 0);
            }
        }
        // ---- the epilogue: divide by the item's norm, then the threshold, the query itself and the mask
        unsigned int m = 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int it = item0 + (g & 3) + 8 * (g >> 2) + 4 * h;
            float s = 0.0f;
            bool ok = false;
            if (has && it < n_items) {
                s = __fdiv_rn(acc[g], norms[it]);
                ok = s == s && it != q && factor_beats(s, it, ts, ti) && (!item_mask || item_mask[it] != 0);
            }
            acc[g] = s;
            if (ok) m |= 1u << g;
        }
        if (__ballot(m != 0u) == 0ull) continue;
        const int mine = __popc(m), other = __shfl_xor(mine, 32, 64);
        int at = count + (h ? other : 0);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            if (m & (1u << g)) {
                lsc[j * LD + at] = acc[g];
                lid[j * LD + at] = item0 + (g & 3) + 8 * (g >> 2) + 4 * h;
                ++at;
            }
        }
        count += mine + other;
        __syncthreads();                            // the appended entries are in LDS
    }
    // ---- rank what is left, then write: straight to the outputs, or this chunk's partial list
    {
        unsigned long long need = __ballot(count > 0);
        while (need) {
            const int u = readfirst_i(__ffsll(static_cast<long long>(need)) - 1) & 31;
            need &= ~((1ull << u) | (1ull << (u + 32)));
            compact(u);
        }
    }
    const bool final_list = splits == 1;
    for (int u = 0; u < 32; ++u) {
        const long long ru = static_cast<long long>(blockIdx.x) * 32 + u;
        if (ru >= n_rows) break;
        int n = readlane_i(count, u);
        const float nq = readlane_f(qn, u);
        const bool cosine = final_list && write_cosine;
        if (cosine && !(nq > 0.0f)) n = 0;          // (a NaN norm fails the compare)
        const long long base = (ru * splits + blockIdx.y) * top_k;
        for (int t = lane; t < top_k; t += 64) {
            float s = ninf;
            if (t < n) { s = lsc[u * LD + t]; if (cosine) s = __fdiv_rn(s, nq); }
            out_ids[base + t] = t < n ? lid[u * LD + t] : -1;
            out_scores[base + t] = s;
        }
        if (lane == 0) {
            out_count[ru * splits + blockIdx.y] = n;
            if (out_div && blockIdx.y == 0) out_div[ru] = nq;
        }
    }
}

// one wave per job: `splits` ranked lists of up to top_k entries over disjoint item ids -> the best top_k of their union
// (factor_topk.hip's merge, plus the one division of a cosine list)
__global__ __launch_bounds__(64) void factor_similar_merge_kernel(
        int n_rows, int top_k, int splits, const int32_t *__restrict__ p_ids, const float *__restrict__ p_scores,
        const int32_t *__restrict__ p_count, int write_cosine, const int32_t *__restrict__ queries,
        const float *__restrict__ q_norms, const float *__restrict__ norms, int n_items, int32_t *__restrict__ out_ids,
        float *__restrict__ out_scores, int32_t *__restrict__ out_count) {
    const int lane = lane_id();
    const float ninf = -__builtin_huge_valf();
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int32_t *cnt = p_count + r * splits;
        const int32_t *ids = p_ids + r * splits * top_k;
        const float *sc = p_scores + r * splits * top_k;
        float nq = 1.0f;
        bool live = true;
        if (write_cosine) {
            nq = similar_query_norm(r, queries, q_norms, norms, n_items);
            live = nq > 0.0f;
        }
        int total = 0;
        if (live) for (int sp = 0; sp < splits; ++sp) total += cnt[sp];
        for (int e = lane; live && e < splits * top_k; e += 64) {
            const int sp = e / top_k, t = e - sp * top_k;
            if (t >= cnt[sp]) continue;
            const float s = sc[e];
            const int id = ids[e];
            int rank = t;
            for (int o = 0; o < splits && rank < top_k; ++o) {
                if (o == sp) continue;
                int lo = 0, hi = cnt[o];            // the first position of list o that does not beat (s, id)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (factor_beats(sc[o * top_k + mid], ids[o * top_k + mid], s, id)) lo = mid + 1; else hi = mid;
                }
                rank += lo;
            }
            if (rank < top_k) {
                out_ids[r * top_k + rank] = id;
                out_scores[r * top_k + rank] = write_cosine ? __fdiv_rn(s, nq) : s;
            }
        }
        const int n_out = total < top_k ? total : top_k;
        for (int t = n_out + lane; t < top_k; t += 64) { out_ids[r * top_k + t] = -1; out_scores[r * top_k + t] = ninf; }
        if (lane == 0) out_count[r] = n_out;
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_factor_similar_topk(int32_t n_rows, const int32_t *d_queries, const float *d_p, int64_t p_stride,
                                         const float *d_p_norms, const float *d_qt, int64_t qt_stride, int32_t n_items, int32_t dim,
                                         const float *d_norms, const uint8_t *d_item_mask, int32_t top_k, int32_t item_splits,
                                         int32_t write_cosine, int32_t *d_out_ids, float *d_out_scores, int32_t *d_out_count,
                                         float *d_out_div, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_items < 0) return RTREC_ERR_INVALID_ARG;
    if (!factor_limits_ok(dim, top_k, item_splits)) return RTREC_ERR_UNSUPPORTED;
    if (qt_stride < n_items || (d_p && p_stride < dim)) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_out_ids || !d_out_scores || !d_out_count) return RTREC_ERR_INVALID_ARG;
    if (d_p ? !d_p_norms : !d_queries) return RTREC_ERR_INVALID_ARG;
    if (n_items > 0 && (!d_qt || !d_norms)) return RTREC_ERR_INVALID_ARG;
    const FactorPlan pl = factor_plan(n_rows, n_items, top_k, item_splits, d_out_ids, d_out_scores, d_out_count, d_workspace,
                                      workspace_bytes);
    if (pl.status != RTREC_OK) return pl.status;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cosine = write_cosine != 0 ? 1 : 0;
    factor_dispatch(dim, top_k, [&](auto DP, auto CAP) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(factor_similar_kernel<DP(), CAP()>), pl.grid, dim3(64), 0, st, n_rows, d_queries, d_p,
                           static_cast<long long>(p_stride), d_p_norms, d_qt, static_cast<long long>(qt_stride), n_items, dim, d_norms,
                           d_item_mask, top_k, pl.splits, pl.tiles_per_chunk, cosine, pl.ids, pl.scores, pl.count, d_out_div);
    });
    if (pl.splits > 1)
        hipLaunchKernelGGL(factor_similar_merge_kernel, dim3(pl.merge_grid), dim3(64), 0, st, n_rows, top_k, pl.splits, pl.ids, pl.scores,
                           pl.count, cosine, d_queries, d_p ? d_p_norms : static_cast<const float *>(nullptr), d_norms, n_items, d_out_ids,
                           d_out_scores, d_out_count);
    return launch_status();
}
