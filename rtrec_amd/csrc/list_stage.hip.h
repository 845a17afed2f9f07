// rtrec_amd/csrc/list_stage.hip.h -- the frame of the list stage: kernels that take one list of item ids per row, give a row to
// one workgroup of 1 or 4 waves (grid-stride over the rows) and write the row's answer back.  score_pairs, diversify,
// list_quality and blend stand on all of it; explain stays one wave per row and takes the clamps, the row of X, the null tests
// and the grid.
//
// Device side: the clamps that keep malformed input in range, and the two places where the waves of a workgroup meet (the sum
// of their partial counts, the rank by counting over an LDS array).  Host side: which wave count serves a call, how many
// workgroups, which (WAVES, CAP) instantiation, and the null tests of the sparse arguments.  What a kernel computes -- and every
// rounding and tie rule -- stays in its own file.
//
// Pieces that stay where they are: blend.hip's blend_reduce (min / max over the workgroup) and diversify.hip's arg-max have one
// user each; the kernels look their columns of W up by ids they have already range-checked, so they clamp those spans
// themselves (clamp_span, span_len) without csr_row's range test.
#pragma once
#include <type_traits>
#include "row_lookup.hip.h"

namespace rtrec {

// a row's count clamped into [0, k]
__device__ __forceinline__ int clamp_count(int cnt, int k) { return cnt < 0 ? 0 : (cnt > k ? k : cnt); }

// hi - lo of a clamped span as an int, saturating
__device__ __forceinline__ int span_len(long long lo, long long hi) {
    return static_cast<int>(hi - lo < 0x7fffffffll ? hi - lo : 0x7fffffffll);
}

// the row of X behind list row r: row_ids names it, absent = row r
__device__ __forceinline__ long long row_behind(const int32_t *row_ids, long long r) {
    return row_ids ? static_cast<long long>(row_ids[r]) : r;
}

// row i of a CSR (or column i of a CSC) with offsets `ptr`: its length, `start` = where it begins, clamped into [0, nnz]; the
// empty row at 0 when i lies outside [0, n_rows).  (The offsets are int32 and the clamp keeps them non-negative, so the length
// fits an int as it is.)
__device__ __forceinline__ int csr_row(const int32_t *ptr, long long i, long long n_rows, long long nnz, long long &start) {
    long long lo = 0, hi = 0;
    if (i >= 0 && i < n_rows) { lo = ptr[i]; hi = ptr[i + 1]; clamp_span(lo, hi, nnz); }
    start = lo;
    return static_cast<int>(hi - lo);
}

// m <- max(m, |w|) with fmaxf's rule for a NaN w (it is ignored); m itself is never NaN
__device__ __forceinline__ void raise_abs(float &m, float w) {
    const float a = __builtin_fabsf(w);
    if (a > m) m = a;
}

// the sum of v over the workgroup's waves, v being the same in every lane of a wave; `slots` holds one entry per wave, nobody
// may still read it when the call begins, and it is free again after the caller's next barrier.  One wave: v itself.
template <int WAVES>
__device__ __forceinline__ int block_sum(int v, int *slots, int tid) {
    if constexpr (WAVES > 1) {
        if ((tid & 63) == 0) slots[tid >> 6] = v;
        __syncthreads();
        v = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) v += slots[w];
    }
    return v;
}

// rank by counting: how many of vals[0 .. n4) beat the value v at position `self`.  o beats v when it is larger, or == and
// at a LATER position (LATER_FIRST) / an EARLIER one; a NaN beats nothing (it fails both compares).  vals is a 16-byte-aligned
// LDS array and n4 a multiple of 4: the values are read four at a time at wave-uniform addresses (LDS broadcasts).  The order
// is strict, so the ranks of the values that are numbers are unique.
template <bool LATER_FIRST>
__device__ __forceinline__ int rank_by_count(const float *vals, int n4, int self, float v) {
    int rank = 0;
    for (int q = 0; q < n4; q += 4) {
        const float4 o = *reinterpret_cast<const float4 *>(&vals[q]);
        rank += (o.x > v || (o.x == v && (LATER_FIRST ? q > self : q < self))) ? 1 : 0;
        rank += (o.y > v || (o.y == v && (LATER_FIRST ? q + 1 > self : q + 1 < self))) ? 1 : 0;
        rank += (o.z > v || (o.z == v && (LATER_FIRST ? q + 2 > self : q + 2 < self))) ? 1 : 0;
        rank += (o.w > v || (o.w == v && (LATER_FIRST ? q + 3 > self : q + 3 < self))) ? 1 : 0;
    }
    return rank;
}

// ---- host side
constexpr int kListMaxGrid = 65536;     // workgroups per launch; rows beyond it are reached by the grid stride

inline bool list_waves_valid(int w) { return w == 0 || w == 1 || w == 4; }

// The waves of a row's workgroup; waves_per_row == 0 leaves the choice to this rule.  It was measured on score_pairs
// (profiles/rerank_c3s.json): all users x 100 candidates run 2.41 ms with one wave per row and 2.81 ms with four, one row x 500
// candidates 0.31 ms and 0.09 ms.  Four waves only pay while a row's block has a CU to itself (256 CUs) and the longest list has
// work for more than one wave.  diversify, list_quality and blend BORROW the rule: tools/diverse_bench.py, quality_bench.py and
// blend_bench.py time both ends of it for their kernel (DESIGN 3.5 reports what they found), the crossover is not measured.
// The answer never depends on the choice.
inline int list_waves(int waves_per_row, int n_rows, int longest) {
    return waves_per_row != 0 ? waves_per_row : (n_rows <= 256 && longest > 64) ? 4 : 1;
}

inline int list_grid(int n_rows) { return n_rows < kListMaxGrid ? n_rows : kListMaxGrid; }

// the arrays of a CSC matrix of n columns / a CSR matrix of n rows are there where something would be read from them
inline bool csc_present(long long n, const void *ptr, long long nnz, const void *row, const void *val) {
    return !((n > 0 && !ptr) || (nnz > 0 && (!row || !val)));
}
inline bool csr_present(long long n, const void *ptr, long long nnz, const void *col, const void *val) {
    return csc_present(n, ptr, nnz, col, val);
}

// launch(WAVES, CAP) with the instantiation for `waves` (1 or 4) waves and LDS arrays of CAP >= longest positions: 1 x 64,
// 1 x 256, 1 x 1024, 4 x 256 or 4 x 1024, both as std::integral_constant (launch is a generic lambda; W() and CAP() are constants)
template <typename F>
inline void list_dispatch(int waves, int longest, F &&launch) {
    using W1 = std::integral_constant<int, 1>;
    using W4 = std::integral_constant<int, 4>;
    using C64 = std::integral_constant<int, 64>;
    using C256 = std::integral_constant<int, 256>;
    using C1024 = std::integral_constant<int, 1024>;
    if (waves == 4) {
        if (longest <= 256) launch(W4{}, C256{}); else launch(W4{}, C1024{});
    } else {
        if (longest <= 64) launch(W1{}, C64{}); else if (longest <= 256) launch(W1{}, C256{}); else launch(W1{}, C1024{});
    }
}

}  // namespace rtrec
