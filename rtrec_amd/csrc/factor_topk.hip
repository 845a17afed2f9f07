// rtrec_amd/csrc/factor_topk.hip -- factor scorer: dense user vectors against dense item vectors, top-k per user, fused.
//
// The reference's hybrid model gets its second list from implicit.topk(items=item_vector, query=user_vector, k, filter_query_items)
// (rtrec/models/hybrid.py): a float32 GEMM followed by a per-row top-k with the interacted items filtered.  This is that call for
// vectors the caller brings; the contract is the comment of rtrec_factor_topk in include/rtrec_amd_ext.h.  In short:
//   score       s = +0.0f, then s = fmaf(p[c], q[c], s) for c = 0 .. dim-1 ascending: one rounding per component, denormals kept
//   competing   0 <= i < n_items, the mask admits i, X's row does not store i (with filter_interacted), the score is not NaN
//   order       the larger score first, among == scores the lower item id: strict, so a list is unique
//
// What is built.  One wave per workgroup; a workgroup owns 32 jobs (users) and one chunk of the catalogue (blockIdx.y of
// `splits` chunks of whole 32-item tiles).  A tile is one chain of v_mfma_f32_32x32x2_f32: the items are the A operand
// (lane l reads component 2 kk + (l >> 5) of item tile + (l & 31): 128 contiguous bytes of d_qt per half wave, no transpose),
// the users the B operand, held in ceil(dim / 2) VGPRs for the life of the workgroup (classes of 8 / 32 / 128 registers for
// dim <= 16 / 64 / 256; the k-loop leaves at the true ceil(dim / 2), an odd dim is padded with one zero component on both sides:
// fmaf(0, 0, s) == s apart from the sign of a zero).  The accumulator starts at +0 and is carried through the k-steps in
// ascending order; by the ISA's description the instruction is the k-ordered float32 fmaf chain, and tests/test_gpu_factor.py
// (rounding order) compares it bit for bit with that chain on data that any other order, an unfused multiply or a wider
// accumulator would change.  A lane then holds 16 scores of user (l & 31): items tile + (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
// Selection is fused, no score block is written: every user has a candidate buffer in LDS (CAP = 64 / 128 / 224 entries for
// top_k <= 16 / 64 / 128; score and id, 8 bytes; rows are CAP + 1 apart so that 32 users appending at one position hit 32
// banks) and a threshold in registers.  A score that does not beat the threshold under the strict order is dropped in
// registers; a survivor is looked up in the mask and in the user's row of X (row_lookup.hip.h) and appended: the two lanes of
// a user take consecutive slots (one __shfl_xor of their survivor counts), so there are no atomics.  A buffer that could not
// take another tile (count > CAP - 32) is compacted by the whole wave: ranks by counting under the strict order, the best
// top_k written to slots 0 .. in order, the threshold becomes slot top_k - 1.  The kept set is always a superset of the top-k
// of the chunk and the final pass is the same ranking, so nothing depends on the order in which tiles or lanes arrive.
// With splits > 1 the ranked partial lists go to the workspace and factor_merge_kernel (one wave per job) ranks every entry
// by its own position plus a binary search in each other sorted list; the chunks' ids are disjoint, so ranks are unique.
//
// LDS per workgroup: 16.3 / 32.3 / 56.3 KiB for the three k-classes (9 / 4 / 2 workgroups of one wave per CU by LDS).
// Malformed input cannot read out of range: X's offsets are clamped to [0, xb_nnz], a row id outside [0, n_x_rows) or a vector
// index outside [0, n_p_rows) is a job without a vector, and item ids are generated, never read.
// Measured (profiles/factor_c3s.json, tools/factor_bench.py; MI355X, 138,493 jobs x 26,744 items, filter on, medians of 10):
// top_k 10: 9.1 ms at dim 12 and 17.8 ms at dim 64 (9.7 / 26.7 TFLOP/s), against 41.9 / 43.8 ms for torch.matmul + topk in 1 GiB
// passes; top_k 100: 116.6 / 139.8 ms against 42.8 / 44.7 ms -- the fused kernel LOSES there: a buffer cut to 100 is full again
// after some 93 survivors, a compaction is one wave ranking one job, and the threshold rises only then.  One job: 0.53 ms with 64
// chunks against 1.43 ms with one at top_k 10, but 5.4 against 2.1 ms at top_k 100 (the item_splits == 0 rule does not look at
// top_k).  The rounding-order test passes with the MFMA, so the __fmaf_rn fallback was not built.
// Not tried: several waves per workgroup sharing the users, staging d_qt through LDS, prefetching the next tile's A operand,
// raising the threshold without a compaction.  No variant was measured against this one.
#include "factor_scan.hip.h"

namespace rtrec {
namespace {

template <int DP, int CAP>
__global__ __launch_bounds__(64) void factor_topk_kernel(
        int n_rows, const int32_t *__restrict__ row_ids, const int32_t *__restrict__ p_index, int n_x_rows,
        const float *__restrict__ p, long long p_stride, int n_p_rows, const float *__restrict__ qt, long long qt_stride,
        int n_items, int dim, const uint8_t *__restrict__ item_mask, const int32_t *__restrict__ xb_ptr,
        const int32_t *__restrict__ xb_col, long long xb_nnz, int filter, int top_k, int splits, int tiles_per_chunk,
        int32_t *__restrict__ out_ids, float *__restrict__ out_scores, int32_t *__restrict__ out_count) {
    constexpr int LD = CAP + 1;                     // a user's row of the buffer
    constexpr int EPL = (CAP + 63) / 64;            // entries per lane in a compaction
    constexpr int G = DP < 16 ? DP : 16;            // k-steps whose A operands are in flight together
    __shared__ float lsc[32 * LD];
    __shared__ int32_t lid[32 * LD];
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const int np = (dim + 1) >> 1;
    const float ninf = -__builtin_huge_valf();
    // ---- this lane's user: its row of X and its vector
    const long long r = static_cast<long long>(blockIdx.x) * 32 + j;
    bool has = false;
    long long x = -1, pi = -1;
    if (r < n_rows) {
        x = row_ids ? static_cast<long long>(row_ids[r]) : r;
        if (x >= 0 && x < n_x_rows) {
            pi = p_index ? static_cast<long long>(p_index[x]) : x;
            has = pi >= 0 && pi < n_p_rows;
        }
    }
    float b[DP];
#pragma unroll
    for (int kk = 0; kk < DP; ++kk) {
        const int c = 2 * kk + h;                   // (a guard, not a break: the loop must unroll for b[] to stay in registers)
        b[kk] = 0.0f;
        if (kk < np) b[kk] = (has && c < dim) ? p[pi * p_stride + c] : 0.0f;
    }
    const int32_t *xcol = xb_col;
    int xlen = 0;
    if (filter && has) {
        long long s = xb_ptr[x], e = xb_ptr[x + 1];
        clamp_span(s, e, xb_nnz);
        xcol = xb_col + s;
        xlen = static_cast<int>(e - s < 0x7fffffffll ? e - s : 0x7fffffffll);
    }
    int count = 0;                                  // entries in this user's buffer (the same in both of its lanes)
    float ts = ninf;                                // the threshold: (-inf, INT_MAX) lets every number through
    int ti = 0x7fffffff;

    // the whole wave ranks user u's buffer and keeps its best top_k in slots 0 .. in order
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
        // ---- survivors: beat the threshold, then the mask and the row of X
        unsigned int m = 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int it = item0 + (g & 3) + 8 * (g >> 2) + 4 * h;
            const float s = acc[g];
            if (has && it < n_items && s == s && factor_beats(s, it, ts, ti)) {
                bool ok = !item_mask || item_mask[it] != 0;
                int pos;
                if (ok && filter && find_sorted(xcol, xlen, it, pos)) ok = false;
                if (ok) m |= 1u << g;
            }
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
    for (int u = 0; u < 32; ++u) {
        const long long ru = static_cast<long long>(blockIdx.x) * 32 + u;
        if (ru >= n_rows) break;
        const int n = readlane_i(count, u);
        const long long base = (ru * splits + blockIdx.y) * top_k;
        for (int t = lane; t < top_k; t += 64) {
            out_ids[base + t] = t < n ? lid[u * LD + t] : -1;
            out_scores[base + t] = t < n ? lsc[u * LD + t] : ninf;
        }
        if (lane == 0) out_count[ru * splits + blockIdx.y] = n;
    }
}

// one wave per job: `splits` ranked lists of up to top_k entries over disjoint item ids -> the best top_k of their union
__global__ __launch_bounds__(64) void factor_merge_kernel(int n_rows, int top_k, int splits, const int32_t *__restrict__ p_ids,
                                                          const float *__restrict__ p_scores, const int32_t *__restrict__ p_count,
                                                          int32_t *__restrict__ out_ids, float *__restrict__ out_scores,
                                                          int32_t *__restrict__ out_count) {
    const int lane = lane_id();
    const float ninf = -__builtin_huge_valf();
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int32_t *cnt = p_count + r * splits;
        const int32_t *ids = p_ids + r * splits * top_k;
        const float *sc = p_scores + r * splits * top_k;
        int total = 0;
        for (int sp = 0; sp < splits; ++sp) total += cnt[sp];
        for (int e = lane; e < splits * top_k; e += 64) {
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
            if (rank < top_k) { out_ids[r * top_k + rank] = id; out_scores[r * top_k + rank] = s; }
        }
        const int n_out = total < top_k ? total : top_k;
        for (int t = n_out + lane; t < top_k; t += 64) { out_ids[r * top_k + t] = -1; out_scores[r * top_k + t] = ninf; }
        if (lane == 0) out_count[r] = n_out;
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_factor_topk(int32_t n_rows, const int32_t *d_row_ids, const int32_t *d_p_index, int32_t n_x_rows,
                                 const float *d_p, int64_t p_stride, int32_t n_p_rows, const float *d_qt, int64_t qt_stride,
                                 int32_t n_items, int32_t dim, const uint8_t *d_item_mask, const int32_t *d_xb_ptr,
                                 const int32_t *d_xb_col, int64_t xb_nnz, int32_t filter_interacted, int32_t top_k,
                                 int32_t item_splits, int32_t *d_out_ids, float *d_out_scores, int32_t *d_out_count,
                                 void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_x_rows < 0 || n_p_rows < 0 || n_items < 0 || xb_nnz < 0) return RTREC_ERR_INVALID_ARG;
    if (!factor_limits_ok(dim, top_k, item_splits)) return RTREC_ERR_UNSUPPORTED;
    if (p_stride < dim || qt_stride < n_items) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_out_ids || !d_out_scores || !d_out_count) return RTREC_ERR_INVALID_ARG;
    if ((n_p_rows > 0 && !d_p) || (n_items > 0 && !d_qt)) return RTREC_ERR_INVALID_ARG;
    const int filter = filter_interacted != 0 ? 1 : 0;
    if (filter && ((n_x_rows > 0 && !d_xb_ptr) || (xb_nnz > 0 && !d_xb_col))) return RTREC_ERR_INVALID_ARG;
    const FactorPlan pl = factor_plan(n_rows, n_items, top_k, item_splits, d_out_ids, d_out_scores, d_out_count, d_workspace,
                                      workspace_bytes);
    if (pl.status != RTREC_OK) return pl.status;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    factor_dispatch(dim, top_k, [&](auto DP, auto CAP) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(factor_topk_kernel<DP(), CAP()>), pl.grid, dim3(64), 0, st, n_rows, d_row_ids, d_p_index, n_x_rows,
                           d_p, static_cast<long long>(p_stride), n_p_rows, d_qt, static_cast<long long>(qt_stride), n_items, dim,
                           d_item_mask, d_xb_ptr, d_xb_col, static_cast<long long>(xb_nnz), filter, top_k, pl.splits, pl.tiles_per_chunk,
                           pl.ids, pl.scores, pl.count);
    });
    if (pl.splits > 1)
        hipLaunchKernelGGL(factor_merge_kernel, dim3(pl.merge_grid), dim3(64), 0, st, n_rows, top_k, pl.splits, pl.ids, pl.scores, pl.count,
                           d_out_ids, d_out_scores, d_out_count);
    return launch_status();
}
