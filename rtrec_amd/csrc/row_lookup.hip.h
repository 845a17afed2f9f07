// rtrec_amd/csrc/row_lookup.hip.h -- "is item j stored in this sorted row, and with which value": the search of the request
// kernels (score_pairs, score_refine, score_first_touch) and the span rule of those that guard against malformed offsets
// (explain, audience, score_pairs).  The frame around these for the kernels that take one list per row -- the clamped row of X,
// the counts, the wave count and the dispatch -- is list_stage.hip.h, which includes this header.
//
// The functions are inlined into their callers, so the address space follows the argument: handed an LDS array they read LDS
// (ds_read), handed a global pointer they load from global memory.  A caller with a staged and an unstaged form of a row calls
// them once in each branch; choosing the POINTER with a condition instead would make every read a flat one.
//
// Searches that stay where they are: explain_probe's in-memory search leaves at the first equal entry (on a row that stores an
// item twice it may pick another duplicate than a lower bound) and its register search goes through __shfl; audience.hip's
// lower_bound_row and rank_metrics.hip's in_sorted work on 64-bit positions and keys; score_cands.hip keeps its own copy of this
// very search because the kernel measured slower with the shared one (the comment at its lookup lambda).
#pragma once
#include "common.hip.h"

namespace rtrec {

// [lo, hi) clamped into [0, nnz], never reversed
__device__ __forceinline__ void clamp_span(long long &lo, long long &hi, long long nnz) {
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
}

// first position in [0, n] with col[pos] >= j (n: there is none); col ascending
__device__ __forceinline__ int lower_bound_sorted(const int *col, int n, int j) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (col[mid] < j) lo = mid + 1; else hi = mid; }
    return lo;
}

// col[0 .. n) stores j: pos = where (the first of equal entries).  pos is the lower bound on a miss too.
__device__ __forceinline__ bool find_sorted(const int *col, int n, int j, int &pos) {
    pos = lower_bound_sorted(col, n, j);
    return pos < n && col[pos] == j;
}

// ... and x = its value; x is left alone on a miss
__device__ __forceinline__ bool find_sorted(const int *col, const float *val, int n, int j, float &x) {
    int pos;
    const bool hit = find_sorted(col, n, j, pos);
    if (hit) x = val[pos];
    return hit;
}

}  // namespace rtrec
