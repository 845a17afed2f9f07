// rtrec_amd/csrc/factor_scan.hip.h -- what rtrec_factor_topk (factor_topk.hip) and rtrec_factor_similar_topk (factor_similar.hip)
// share at no cost: the limits, the strict order, the host plan of a call and the choice of the kernel instantiation.
//
// The scan kernel and the merge kernel stay in each file, the same text apart from the job's lookup, the epilogue and the rule
// at the write.  They were folded into one template over a job type here and taken out again: the similar kernel gained 0.4 -
// 3.8 %, but rtrec_factor_topk measured 1.5 - 1.8 % slower over all users of c3s in three of four shapes and 2.5 - 3.1 % slower
// for one job in 64 chunks, in eight of eight runs ("The factor scan"; profiles/factor_scan_ab.json).  With the
// kernels in their files the disassembled device code of both is what it was before this header, addresses included.
#pragma once
#include <type_traits>
#include "row_lookup.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kFactorMaxDim = 256;
constexpr int kFactorMaxK = 128;
constexpr int kFactorMaxSplits = 64;
constexpr int kFactorMergeGrid = 65536;
constexpr int kFactorAutoBlocks = 1024;      // item_splits == 0: chunks are added until this many workgroups exist (4 per CU)

// a beats b under the strict order
__device__ __forceinline__ bool factor_beats(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// ---- host side
inline bool factor_limits_ok(int dim, int top_k, int item_splits) {
    return dim >= 1 && dim <= kFactorMaxDim && top_k >= 1 && top_k <= kFactorMaxK && item_splits >= 0 && item_splits <= kFactorMaxSplits;
}

// how a call of n_rows > 0 jobs runs: the chunks, where the scan writes (the outputs, or the partial lists carved out of the
// workspace as ids, scores, counts), its grid and the merge's; `status` is RTREC_OK or the workspace error of an explicit item_splits
struct FactorPlan {
    int status, splits, tiles_per_chunk, merge_grid;
    int32_t *ids;
    float *scores;
    int32_t *count;
    dim3 grid;
};

inline FactorPlan factor_plan(int n_rows, int n_items, int top_k, int item_splits, int32_t *d_out_ids, float *d_out_scores,
                              int32_t *d_out_count, void *d_workspace, size_t workspace_bytes) {
    FactorPlan pl = {RTREC_OK, item_splits, 0, n_rows < kFactorMergeGrid ? n_rows : kFactorMergeGrid, d_out_ids, d_out_scores,
                     d_out_count, dim3(1)};
    const int n_tiles = (n_items + 31) / 32;
    const long long blocks = (static_cast<long long>(n_rows) + 31) / 32;
    const size_t per_split = RTREC_FACTOR_TOPK_WORKSPACE_BYTES(n_rows, top_k, 1);
    if (item_splits == 0) {
        // the library's choice: chunks until kFactorAutoBlocks workgroups exist, as far as the workspace reaches.  The figure is
        // four one-wave workgroups per CU; it is not measured, and the answer never depends on it.
        const long long want = (kFactorAutoBlocks + blocks - 1) / blocks;
        pl.splits = static_cast<int>(want < kFactorMaxSplits ? want : kFactorMaxSplits);
        const size_t fits = d_workspace ? workspace_bytes / per_split : 0;
        if (static_cast<size_t>(pl.splits) > fits) pl.splits = static_cast<int>(fits);
        if (pl.splits < 2) pl.splits = 1;
    } else if (item_splits > 1) {
        if (!d_workspace) { pl.status = RTREC_ERR_INVALID_ARG; return pl; }
        if (workspace_bytes < per_split * static_cast<size_t>(item_splits)) { pl.status = RTREC_ERR_WORKSPACE; return pl; }
    }
    if (pl.splits > n_tiles) pl.splits = n_tiles > 0 ? n_tiles : 1;      // (no empty chunks)
    pl.tiles_per_chunk = n_tiles > 0 ? (n_tiles + pl.splits - 1) / pl.splits : 0;
    if (pl.splits > 1) {
        const size_t cells = static_cast<size_t>(n_rows) * static_cast<size_t>(pl.splits) * static_cast<size_t>(top_k);
        pl.ids = static_cast<int32_t *>(d_workspace);
        pl.scores = reinterpret_cast<float *>(pl.ids + cells);
        pl.count = reinterpret_cast<int32_t *>(pl.scores + cells);
    }
    pl.grid = dim3(static_cast<unsigned int>(blocks), static_cast<unsigned int>(pl.splits));
    return pl;
}

// launch(DP, CAP) with the instantiation for `dim` components (DP = 8 / 32 / 128 B registers for dim <= 16 / 64 / 256) and
// `top_k` (CAP = 64 / 128 / 224 buffer entries for top_k <= 16 / 64 / 128), both as std::integral_constant (list_dispatch's form)
template <typename F>
inline void factor_dispatch(int dim, int top_k, F &&launch) {
    auto by_k = [&](auto DP) {
        if (top_k <= 16) launch(DP, std::integral_constant<int, 64>{});
        else if (top_k <= 64) launch(DP, std::integral_constant<int, 128>{});
        else launch(DP, std::integral_constant<int, 224>{});
    };
    if (dim <= 16) by_k(std::integral_constant<int, 8>{});
    else if (dim <= 64) by_k(std::integral_constant<int, 32>{});
    else by_k(std::integral_constant<int, 128>{});
}

}  // namespace rtrec
