// rtrec_amd/csrc/factor_als.hip -- one side of an implicit-feedback ALS half-step: per row of R the normal equations are built on
// the matrix cores and solved by a Cholesky factorisation, every operation pinned.
//
// Hu, Koren and Volinsky's alternating least squares: with the other side V fixed, row x solves
//   (V^T V + reg I + sum_i w_xi y_i y_i^T) p_x = sum_i (1 + w_xi) y_i,   w_xi = alpha * r_xi over the row's stored entries.
// The contract is the comment of rtrec_factor_als_solve in include/rtrec_amd_ext.h.  In short:
//   usable      entry (i, val) with 0 <= i < n_v and w = fl(alpha * val) > 0 (NaN and non-positive skipped); offsets clamped
//   build       lower triangle: A[a][b] = G[a][b], then fmaf(fl(w * y_i[a]), y_i[b], A[a][b]) over the usable entries in storage
//               order; rhs[a] = +0, then fmaf(fl(1 + w), y_i[a], rhs[a])
//   Cholesky    left-looking, every element one fmaf chain over ascending k, a correctly rounded root and division
//   solve       forward over ascending k, backward over descending k, one division per component
//   status      0 solved; 1 row outside R (nothing written) or no usable entry (zeros); 2 breakdown or a non-finite component
//
// What is built.  One wave per job.  The row's entries are read 64 at a time (lane = entry: column, w, usable or not) and handed
// out by readlane, two per k-step: lanes 0..31 take the even entry, 32..63 the odd one.  A lane loads component j (and 32 + j) of
// its entry's row of V -- 128 contiguous bytes per half wave -- kAlsGroup steps ahead of the chain.  The build is one chain of
// v_mfma_f32_32x32x2_f32 per 32 x 32 tile with the accumulator initialised from G: the A operand is fl(w * y[a]), the B operand
// y[b], which is the fmaf chain of the definition bit for bit.  dim <= 32 is one tile, dim <= 64 the three lower ones.  Zero
// operands (both) stand wherever the chain has no term: components at or beyond dim, a skipped entry, the odd last entry; a
// skipped entry's row of V is never loaded.  rhs is a VALU chain: lane l holds rhs[l]; per step the two half waves swap the
// component the other needs (one __shfl_xor), so that both apply the even entry, then the odd one.
// The accumulators go to LDS as A (rows 33 / 65 floats apart: 4.1 / 16.3 KiB); Cholesky and both substitutions run with
// lane = row: the lane reads its own row and a broadcast one, the diagonal stays in a register, the pivot and every solved
// component travel by readlane.  The root is taken in float64 and rounded once more (factor_norms.hip says why); the division
// is __fdiv_rn.  Float32 denormals are kept (hipcc's default mode; the MFMA's C/D never flush).
// No atomics, no state; a job's result does not depend on the grid.  Jobs are taken in the order given: the engine names the
// longest rows first, as the scoring kernels do with d_row_order.
// Malformed input cannot read out of range: offsets are clamped to [0, nnz], columns outside [0, n_v) are skipped before any read
// of V, a job row outside [0, n_rows) reads and writes nothing but its status.
// Not built: a row split over several waves (it would change the definition).  dim above 64 is served by the conjugate-gradient
// call beside this one (csrc/factor_als_cg.hip, rtrec_factor_als_cg), which never forms the row's matrix; this kernel stays at 64.
// Measured: profiles/als_<workload>.json (tools/als_bench.py) where committed; DESIGN quotes it beside the computed bound.
#include "factor_als.hip.h"

namespace rtrec {
namespace {

constexpr int kAlsMaxGrid = 1 << 18;      // workgroups per launch; jobs beyond it are reached by the grid stride

template <int NT>
__global__ __launch_bounds__(64) void factor_als_solve_kernel(
        int n_jobs, const int32_t *__restrict__ job_rows, int n_rows, const int32_t *__restrict__ r_ptr,
        const int32_t *__restrict__ r_idx, const float *__restrict__ r_val, long long nnz, const float *__restrict__ v,
        long long v_stride, int n_v, int dim, const float *__restrict__ gram, float alpha, float *__restrict__ out,
        long long out_stride, uint8_t *__restrict__ status) {
    constexpr int G = kAlsGroup;
    constexpr int D = NT > 1 ? 64 : 32;
    constexpr int LD = D + 1;
    constexpr int T10 = NT > 1 ? 1 : 0, T11 = NT > 1 ? 2 : 0;      // tiles (1, 0) and (1, 1); tile (0, 0) is acc[0]
    __shared__ float A[D * LD];
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const bool in0 = j < dim, in1 = NT > 1 && 32 + j < dim;
    const bool mine = lane < dim;                       // this lane owns row `lane` of A and component `lane` of the vectors
    const int ri = mine ? lane : 0;                     // (an address that is always inside A)
    for (long long job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int x = job_rows ? job_rows[job] : static_cast<int>(job);
        if (x < 0 || x >= n_rows) {
            if (lane == 0) status[job] = 1;
            continue;
        }
        long long e0 = r_ptr[x], e1 = r_ptr[x + 1];
        e0 = e0 < 0 ? 0 : (e0 > nnz ? nnz : e0);
        e1 = e1 < 0 ? 0 : (e1 > nnz ? nnz : e1);
        // ---- build: A = G + (w o Y)^T Y on the matrix cores, rhs on the VALU
        als_f32x16 acc[NT];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int a = als_acc_row(g, h);
            acc[0][g] = (a < dim && in0) ? gram[a * dim + j] : 0.0f;
            if (NT > 1) {
                acc[T10][g] = (32 + a < dim && in0) ? gram[(32 + a) * dim + j] : 0.0f;
                acc[T11][g] = (32 + a < dim && in1) ? gram[(32 + a) * dim + 32 + j] : 0.0f;
            }
        }
        float rhs = 0.0f;
        bool any = false;
        for (long long base = e0; base < e1; base += 64) {
            const long long e = base + lane;
            int col = -1;
            float w = 0.0f;
            if (e < e1) {
                const int c = r_idx[e];
                const float wv = __fmul_rn(alpha, r_val[e]);
                if (c >= 0 && c < n_v && wv > 0.0f) { col = c; w = wv; }
            }
            if (__ballot(col >= 0) == 0ull) continue;   // (a block of skipped entries has no term at all)
            any = true;
            const long long left = e1 - base;
            const int steps = left >= 64 ? 32 : static_cast<int>((left + 1) >> 1);
#pragma unroll
            for (int sb = 0; sb < 32; sb += G) {
                if (sb >= steps) break;
                float y0[G], y1[G], ww[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int s = sb + g;               // (compile-time: the entries 2 s and 2 s + 1 of the block)
                    const int c = h ? readlane_i(col, 2 * s + 1) : readlane_i(col, 2 * s);
                    ww[g] = h ? readlane_f(w, 2 * s + 1) : readlane_f(w, 2 * s);
                    const float *src = v + static_cast<long long>(c) * v_stride;
                    y0[g] = (c >= 0 && in0) ? src[j] : 0.0f;
                    y1[g] = (c >= 0 && in1) ? src[32 + j] : 0.0f;
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (sb + g < steps) {
                        const float a0 = __fmul_rn(ww[g], y0[g]);
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, y0[g], acc[0], 0, 0, 0);
                        if (NT > 1) {
                            const float a1 = __fmul_rn(ww[g], y1[g]);
                            acc[T10] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, y0[g], acc[T10], 0, 0, 0);
                            acc[T11] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, y1[g], acc[T11], 0, 0, 0);
                        }
                        // rhs[lane]: the even entry's term, then the odd one's.  The lower half wave holds the even entry and
                        // components 0..31, the upper one the odd entry and components 32..63: each sends what the other lacks.
                        // A skipped entry has y == 0 and w == 0: fmaf(1, 0, rhs) leaves rhs as it is
                        const float got = __shfl_xor(h ? y0[g] : y1[g], 32, 64);
                        const float cw = __fadd_rn(1.0f, ww[g]);
                        const float co = __shfl_xor(cw, 32, 64);
                        rhs = __fmaf_rn(h ? co : cw, h ? got : y0[g], rhs);
                        rhs = __fmaf_rn(h ? cw : co, h ? y1[g] : got, rhs);
                    }
                }
            }
        }
        float *dst = out + static_cast<long long>(x) * out_stride;
        if (!any) {                                     // no usable entry: zeros, whatever G holds
            if (mine) dst[lane] = 0.0f;
            if (lane == 0) status[job] = 1;
            continue;
        }
        __syncthreads();                                // (the last job's reads of A are done)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int a = als_acc_row(g, h);
            A[a * LD + j] = acc[0][g];
            if (NT > 1) {
                A[(32 + a) * LD + j] = acc[T10][g];
                A[(32 + a) * LD + 32 + j] = acc[T11][g];
            }
        }
        __syncthreads();
        // ---- Cholesky, left-looking, L over A's lower triangle: lane = row
        bool broken = false;
        float diag = 1.0f;
        for (int c = 0; c < dim; ++c) {
            float s = A[ri * LD + c];
            for (int k = 0; k < c; ++k) s = __fmaf_rn(-A[ri * LD + k], A[c * LD + k], s);
            const float d = readlane_f(s, c);           // (row c's chain is the diagonal's)
            if (!(d > 0.0f) || d == __builtin_huge_valf()) { broken = true; break; }
            const float root = static_cast<float>(__dsqrt_rn(static_cast<double>(d)));
            const float l = lane == c ? root : __fdiv_rn(s, root);
            if (lane == c) diag = root;
            if (mine && lane >= c) A[ri * LD + c] = l;  // (column c was read by its own lane alone)
            __syncthreads();
        }
        float s = rhs;
        if (!broken) {
            // ---- forward: z[c] = (rhs[c] - sum_{k < c} L[c][k] z[k]) / L[c][c], k ascending
            for (int k = 0; k < dim; ++k) {
                const float zk = readlane_f(__fdiv_rn(s, diag), k);
                if (lane == k) s = zk;
                else if (mine && lane > k) s = __fmaf_rn(-A[ri * LD + k], zk, s);
            }
            // ---- backward: x[c] = (z[c] - sum_{k > c} L[k][c] x[k]) / L[c][c], k descending
            for (int k = dim - 1; k >= 0; --k) {
                const float xk = readlane_f(__fdiv_rn(s, diag), k);
                if (lane == k) s = xk;
                else if (lane < k) s = __fmaf_rn(-A[k * LD + lane], xk, s);
            }
        }
        const bool finite = s - s == 0.0f;              // (inf - inf and NaN - NaN are NaN)
        const bool bad = broken || __ballot(mine && !finite) != 0ull;
        if (mine) dst[lane] = bad ? 0.0f : s;
        if (lane == 0) status[job] = bad ? 2 : 0;
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_factor_als_solve(int32_t n_jobs, const int32_t *d_job_rows, int32_t n_rows, const int32_t *d_r_ptr,
                                      const int32_t *d_r_idx, const float *d_r_val, int64_t nnz, const float *d_v, int64_t v_stride,
                                      int32_t n_v, int32_t dim, const float *d_gram, float alpha, float *d_out, int64_t out_stride,
                                      uint8_t *d_status, void *stream) {
    using namespace rtrec;
    if (dim < 1 || dim > kAlsMaxDim) return RTREC_ERR_UNSUPPORTED;
    if (n_jobs < 0 || n_rows < 0 || n_v < 0 || nnz < 0 || v_stride < dim || out_stride < dim || !(alpha > 0.0f))
        return RTREC_ERR_INVALID_ARG;
    if (n_jobs == 0) return RTREC_OK;
    if (!d_gram || !d_out || !d_status) return RTREC_ERR_INVALID_ARG;
    if ((n_rows > 0 && !d_r_ptr) || (nnz > 0 && (!d_r_idx || !d_r_val)) || (n_v > 0 && !d_v)) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned int>(n_jobs < kAlsMaxGrid ? n_jobs : kAlsMaxGrid));
    if (dim <= 32)
        hipLaunchKernelGGL(factor_als_solve_kernel<1>, grid, dim3(64), 0, st, n_jobs, d_job_rows, n_rows, d_r_ptr, d_r_idx, d_r_val,
                           static_cast<long long>(nnz), d_v, static_cast<long long>(v_stride), n_v, dim, d_gram, alpha, d_out,
                           static_cast<long long>(out_stride), d_status);
    else
        hipLaunchKernelGGL(factor_als_solve_kernel<3>, grid, dim3(64), 0, st, n_jobs, d_job_rows, n_rows, d_r_ptr, d_r_idx, d_r_val,
                           static_cast<long long>(nnz), d_v, static_cast<long long>(v_stride), n_v, dim, d_gram, alpha, d_out,
                           static_cast<long long>(out_stride), d_status);
    return launch_status();
}
