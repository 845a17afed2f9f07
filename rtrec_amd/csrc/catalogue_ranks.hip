// rtrec_amd/csrc/catalogue_ranks.hip -- full-catalogue ranks of held-out items: for every target (row, item) the number of
// competing columns of the row's dense score vector that score higher, the number that score the same, the score itself, and per
// row the number of competing columns.  A position needs no sort, only counts; integer counts are exact and independent of
// scheduling.
//
// The contract is the comment of rtrec_slim_catalogue_ranks in include/rtrec_amd_ext.h; in short, for row r with scores s[c]:
//   own          the distinct in-range columns stored in X's row (filter_interacted only)
//   competes(c)  s[c] is not NaN, c is not in own, and the mode is DENSE or s[c] != 0
//   above / tied the competing columns c != i with s[c] > s[i] / s[c] == s[i], for a target i that competes; -1 / 0 otherwise
//
// Mapping.  One row per workgroup of four waves, grid-stride over the rows beyond kRanksMaxGrid.  The row's targets are taken
// 4 or 8 at a time: their scores are read first and kept in registers, then the row is swept ONCE per group with 16-byte loads
// (a scalar head up to the first aligned address and a scalar tail), every thread counting `>` and `==` against each target of
// the group in integer registers.  A column that does not compete without looking at own (NaN; zero in SPARSE mode) is turned
// into a NaN as it is loaded, and a target that does not compete is compared as a NaN: every compare with a NaN is false, so
// neither needs a branch in the loop.  own is not tested per column: the sweep counts every column, then the stored row is walked
// and what its columns contributed is taken back (integers, so exact); the same walk marks a target that is stored in the row.
// The target's own `==` hit is taken back at the end.  Counters are reduced by wave shuffles and one LDS hop over the four
// waves.  Plain vector loads and stores; no atomics.
//
// The kernel is a streaming read of n_rows * n_items scores: 256 threads with two 16-byte loads in flight each are 8 KiB per
// workgroup, and the registers (120 VGPRs for float32, 88 for float64) let four to five workgroups share a CU, which is the
// ~32 KiB per CU in flight that a streaming read of HBM needs; kRanksMaxGrid = 8 * 256 CUs covers that with room.  A group of
// 16 targets would need 160 VGPRs and leave three workgroups per CU, hence 8.  With 8 targets the loop does 32 integer
// operations per score, so by the instruction count (an estimate: the 8-target form has not been timed) it is bound by them
// rather than by memory; with the three or so held-out items per user of an evaluation it takes the 4-target form.  The occupancy statements are the compiler's, not counters;
// tools/ranks_bench.py times the kernel beside a device-to-device copy of the same block (profiles/ranks_c3s.json).
// Malformed input cannot read or write out of range: offsets into X are clamped to [0, xb_nnz], offsets into the targets to
// [0, n_tg], a row id outside [0, n_x_rows) has no own, a column or target outside [0, n_items) is never read.
#include "row_lookup.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {
namespace {

constexpr int kRanksThreads = 256;      // four waves per row
constexpr int kRanksWaves = kRanksThreads / 64;
constexpr int kRanksMaxGroup = 8;       // targets per sweep, at most
constexpr int kRanksMaxGrid = 2048;     // workgroups per launch; rows beyond it are reached by the grid stride

template <typename ACC> struct RanksVec;
template <> struct RanksVec<float> { using type = float4; static constexpr int N = 4; };
template <> struct RanksVec<double> { using type = double2; static constexpr int N = 2; };

template <typename ACC>
__device__ __forceinline__ ACC ranks_nan() { return static_cast<ACC>(__builtin_nanf("")); }

// the column as the sweep compares it: a NaN where it cannot compete whatever own holds
template <typename ACC>
__device__ __forceinline__ ACC ranks_fix(ACC v, bool dense) { return (!dense && v == ACC(0)) ? ranks_nan<ACC>() : v; }

template <typename ACC, int T>
__device__ __forceinline__ void ranks_count(ACC v, const ACC (&st)[T], int (&above)[T], int (&tied)[T], int &competing) {
    competing += v == v ? 1 : 0;
#pragma unroll
    for (int k = 0; k < T; ++k) {
        above[k] += v > st[k] ? 1 : 0;
        tied[k] += v == st[k] ? 1 : 0;
    }
}

struct RanksLds {
    double st[kRanksMaxGroup];                              // the group's target scores as compared (NaN: it does not compete)
    int32_t item[kRanksMaxGroup];                           // ... and items, -1: no such column
    int32_t owned[kRanksMaxGroup];                          // the target is stored in X's row
    int32_t red[kRanksWaves][2 * kRanksMaxGroup + 1];       // per wave: above[T], tied[T], competing
};

// One group of nt <= T targets [t0, t0 + nt) of the row `s` (n_items scores), own = xb_col[a0 .. a1).
template <typename ACC, int T>
__device__ __forceinline__ void ranks_group(RanksLds &L, const ACC *__restrict__ s, int n_items, bool dense,
                                            const int32_t *__restrict__ xb_col, long long a0, long long a1,
                                            const int32_t *__restrict__ tg_items, long long t0, int nt,
                                            int32_t *__restrict__ out_above, int32_t *__restrict__ out_tied,
                                            double *__restrict__ out_score, int32_t *out_competing) {
    using Vec = typename RanksVec<ACC>::type;
    constexpr int VN = RanksVec<ACC>::N;
    const int tid = static_cast<int>(threadIdx.x);
    if (tid < T) {
        int item = -1;
        ACC v = ranks_nan<ACC>();
        if (tid < nt) {
            const int i = tg_items[t0 + tid];
            double sc = -__builtin_inf();
            if (i >= 0 && i < n_items) {
                item = i;
                const ACC raw = s[i];
                sc = static_cast<double>(raw);
                v = ranks_fix(raw, dense);
            }
            out_score[t0 + tid] = sc;
        }
        L.st[tid] = static_cast<double>(v);         // (float -> double is exact, and a NaN stays a NaN)
        L.item[tid] = item;
        L.owned[tid] = 0;
    }
    __syncthreads();
    ACC st[T];
    int above[T], tied[T], competing = 0;
#pragma unroll
    for (int k = 0; k < T; ++k) { st[k] = static_cast<ACC>(L.st[k]); above[k] = 0; tied[k] = 0; }

    // ---- the sweep: scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
    const unsigned long long addr = reinterpret_cast<unsigned long long>(s);
    int head = static_cast<int>(((16ull - (addr & 15ull)) & 15ull) / sizeof(ACC));
    head = head < n_items ? head : n_items;
    const int n_vec = (n_items - head) / VN;
    const int tail0 = head + n_vec * VN;
    if (tid < head) ranks_count<ACC, T>(ranks_fix(s[tid], dense), st, above, tied, competing);
    const Vec *__restrict__ sv = reinterpret_cast<const Vec *>(s + head);
#pragma unroll 2
    for (int i = tid; i < n_vec; i += kRanksThreads) {
        const Vec q = sv[i];
        ranks_count<ACC, T>(ranks_fix(q.x, dense), st, above, tied, competing);
        ranks_count<ACC, T>(ranks_fix(q.y, dense), st, above, tied, competing);
        if constexpr (VN == 4) {
            ranks_count<ACC, T>(ranks_fix(q.z, dense), st, above, tied, competing);
            ranks_count<ACC, T>(ranks_fix(q.w, dense), st, above, tied, competing);
        }
    }
    if (tail0 + tid < n_items) ranks_count<ACC, T>(ranks_fix(s[tail0 + tid], dense), st, above, tied, competing);

    // ---- own: take back what the stored columns contributed (an equal neighbour of an ascending row is one column), and
    // mark the targets the row stores
    for (long long p = a0 + tid; p < a1; p += kRanksThreads) {
        const int c = xb_col[p];
        if (c < 0 || c >= n_items) continue;
        if (p > a0 && xb_col[p - 1] == c) continue;
        const ACC v = ranks_fix(s[c], dense);
        competing -= v == v ? 1 : 0;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            above[k] -= v > st[k] ? 1 : 0;
            tied[k] -= v == st[k] ? 1 : 0;
            if (L.item[k] == c) L.owned[k] = 1;     // (several threads may store the same 1)
        }
    }

    // ---- reduce: wave shuffles, then one LDS hop over the waves
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        competing += shfl_xor_t(competing, m);
#pragma unroll
        for (int k = 0; k < T; ++k) { above[k] += shfl_xor_t(above[k], m); tied[k] += shfl_xor_t(tied[k], m); }
    }
    if (lane_id() == 0) {
        const int w = tid >> 6;
#pragma unroll
        for (int k = 0; k < T; ++k) { L.red[w][k] = above[k]; L.red[w][T + k] = tied[k]; }
        L.red[w][2 * T] = competing;
    }
    __syncthreads();                    // the waves' sums and the owned marks are in LDS
    if (tid < nt) {
        int a = 0, e = 0;
#pragma unroll
        for (int w = 0; w < kRanksWaves; ++w) { a += L.red[w][tid]; e += L.red[w][T + tid]; }
        const double v = L.st[tid];
        const bool competes = v == v && L.owned[tid] == 0;
        out_above[t0 + tid] = competes ? a : -1;
        out_tied[t0 + tid] = competes ? e - 1 : 0;      // (the target's own == hit)
    }
    if (out_competing && tid == 0) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < kRanksWaves; ++w) c += L.red[w][2 * T];
        *out_competing = c;
    }
    __syncthreads();                    // the group is done: LDS may be overwritten
}

template <typename ACC>
__global__ __launch_bounds__(kRanksThreads) void catalogue_ranks_kernel(
        int n_rows, int n_items, const ACC *__restrict__ scores, long long scores_stride, const int32_t *__restrict__ row_ids,
        const int32_t *__restrict__ xb_ptr, const int32_t *__restrict__ xb_col, int n_x_rows, long long xb_nnz, int filter,
        int dense, const long long *__restrict__ tg_ptr, const int32_t *__restrict__ tg_items, long long n_tg,
        int32_t *__restrict__ out_above, int32_t *__restrict__ out_tied, double *__restrict__ out_score,
        int32_t *__restrict__ out_competing) {
    __shared__ RanksLds L;
    const int tid = static_cast<int>(threadIdx.x);
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        long long tb = tg_ptr[r], te = tg_ptr[r + 1];
        clamp_span(tb, te, n_tg);
        // slots no row's span covers (in front of the first row's, behind the last row's) are still written
        const long long f1 = r == 0 ? tb : 0;
        for (long long t = tid; t < f1; t += kRanksThreads) { out_above[t] = -1; out_tied[t] = 0; out_score[t] = -__builtin_inf(); }
        if (r == n_rows - 1)
            for (long long t = te + tid; t < n_tg; t += kRanksThreads) { out_above[t] = -1; out_tied[t] = 0; out_score[t] = -__builtin_inf(); }
        long long a0 = 0, a1 = 0;
        if (filter) {
            const int xrow = row_ids ? row_ids[r] : static_cast<int>(r);
            if (xrow >= 0 && xrow < n_x_rows) { a0 = xb_ptr[xrow]; a1 = xb_ptr[xrow + 1]; clamp_span(a0, a1, xb_nnz); }
        }
        const ACC *s = scores + r * scores_stride;
        long long t0 = tb;
        bool first = true;
        do {                            // (a row without targets still sweeps once: its competing count)
            const long long left = te - t0;
            const int nt = static_cast<int>(left < kRanksMaxGroup ? left : kRanksMaxGroup);
            int32_t *oc = first ? out_competing + r : nullptr;
            if (nt <= 4)
                ranks_group<ACC, 4>(L, s, n_items, dense != 0, xb_col, a0, a1, tg_items, t0, nt, out_above, out_tied, out_score, oc);
            else
                ranks_group<ACC, kRanksMaxGroup>(L, s, n_items, dense != 0, xb_col, a0, a1, tg_items, t0, nt, out_above, out_tied,
                                                 out_score, oc);
            t0 += nt;
            first = false;
        } while (t0 < te);
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_slim_catalogue_ranks(int32_t n_rows, int32_t n_items, const void *d_scores, int64_t scores_stride,
                                          int32_t scores_f64, const int32_t *d_row_ids, const int32_t *d_xb_ptr,
                                          const int32_t *d_xb_col, int32_t n_x_rows, int64_t xb_nnz, int32_t filter_interacted,
                                          int32_t mode, const int64_t *d_tg_ptr, const int32_t *d_tg_items, int64_t n_tg,
                                          int32_t *d_out_above, int32_t *d_out_tied, double *d_out_score,
                                          int32_t *d_out_competing, void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_items < 0 || n_x_rows < 0 || xb_nnz < 0 || n_tg < 0) return RTREC_ERR_INVALID_ARG;
    if (mode != RTREC_TOPK_SPARSE && mode != RTREC_TOPK_DENSE) return RTREC_ERR_UNSUPPORTED;
    if (scores_stride < n_items) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_tg_ptr || !d_out_competing || (n_items > 0 && !d_scores)) return RTREC_ERR_INVALID_ARG;
    if (n_tg > 0 && (!d_tg_items || !d_out_above || !d_out_tied || !d_out_score)) return RTREC_ERR_INVALID_ARG;
    if (filter_interacted && ((n_x_rows > 0 && !d_xb_ptr) || (xb_nnz > 0 && !d_xb_col))) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    const int grid = n_rows < kRanksMaxGrid ? n_rows : kRanksMaxGrid;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long stride = static_cast<long long>(scores_stride), nnz = static_cast<long long>(xb_nnz);
    const long long *tg_ptr = reinterpret_cast<const long long *>(d_tg_ptr);
    if (scores_f64)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(catalogue_ranks_kernel<double>), dim3(grid), dim3(kRanksThreads), 0, st, n_rows, n_items,
                           static_cast<const double *>(d_scores), stride, d_row_ids, d_xb_ptr, d_xb_col, n_x_rows, nnz,
                           filter_interacted ? 1 : 0, mode == RTREC_TOPK_DENSE ? 1 : 0, tg_ptr, d_tg_items,
                           static_cast<long long>(n_tg), d_out_above, d_out_tied, d_out_score, d_out_competing);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(catalogue_ranks_kernel<float>), dim3(grid), dim3(kRanksThreads), 0, st, n_rows, n_items,
                           static_cast<const float *>(d_scores), stride, d_row_ids, d_xb_ptr, d_xb_col, n_x_rows, nnz,
                           filter_interacted ? 1 : 0, mode == RTREC_TOPK_DENSE ? 1 : 0, tg_ptr, d_tg_items,
                           static_cast<long long>(n_tg), d_out_above, d_out_tied, d_out_score, d_out_competing);
    return launch_status();
}
