// rtrec_amd/csrc/factor_gram.hip -- the regularised Gram matrix of one side's factor vectors: the constant part of every row's
// normal equations in an implicit-feedback ALS half-step (Hu, Koren, Volinsky: A_x = V^T V + reg I + sum_i w_xi y_i y_i^T).
//
// The contract is the comment of rtrec_factor_gram in include/rtrec_amd_ext.h.  In short:
//   chunk c     rows [1024 c, min(n_v, 1024 c + 1024)) of V
//   part_c      +0, then part_c[a][b] = fmaf(v_r[a], v_r[b], part_c[a][b]) over ascending r of the chunk
//   G           +0, then G[a][b] = fl(G[a][b] + part_c[a][b]) over ascending c; finally G[a][a] = fl(G[a][a] + reg)
// fmaf(v[a], v[b], p) == fmaf(v[b], v[a], p), so G is symmetric bit for bit.
//
// What is built.  factor_gram_partial_kernel: one one-wave workgroup per chunk; a 32 x 32 tile of part_c is one chain of
// v_mfma_f32_32x32x2_f32 over ascending rows, two per instruction (lanes 0..31 bring the even row, 32..63 the odd one), which is
// that fmaf chain bit for bit (tests/test_gpu_factor.py, tests/test_gpu_als.py).  dim <= 32 is one tile; dim <= 64 computes the
// three lower tiles and writes tile (1, 0) twice, once transposed.  A lane reads component j (and 32 + j) of its row: 128 bytes
// per half wave; kAlsGroup steps of loads are issued ahead of their chain.  Zero operands stand wherever the chain has no term:
// components at or beyond dim and the row behind an odd chunk; nothing loaded is ever fed there.
// factor_gram_sum_kernel: one thread per element adds the partials in ascending chunk order and the diagonal's reg.
// No atomics; the result does not depend on the grid.  Both launches happen in the one export, as rtrec_factor_topk launches
// its merge.  Not measured on its own here; tools/als_bench.py times the call.
// rtrec_factor_gram_wide (dim up to 256, the same definition and the same bits up to 64): factor_gram_wide_partial_kernel, one
// one-wave workgroup per (chunk, lower 32 x 32 tile), then the same factor_gram_sum_kernel.
#include "factor_als.hip.h"

namespace rtrec {
namespace {

template <int NT>
__global__ __launch_bounds__(64) void factor_gram_partial_kernel(int n_v, const float *__restrict__ v, long long v_stride, int dim,
                                                                 float *__restrict__ part) {
    constexpr int G = kAlsGroup;
    constexpr int T10 = NT > 1 ? 1 : 0, T11 = NT > 1 ? 2 : 0;      // tiles (1, 0) and (1, 1); tile (0, 0) is acc[0]
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const long long r0 = static_cast<long long>(blockIdx.x) * kAlsGramChunk;
    long long r1 = r0 + kAlsGramChunk;
    if (r1 > n_v) r1 = n_v;
    const bool in0 = j < dim, in1 = NT > 1 && 32 + j < dim;
    als_f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[t][g] = 0.0f;
    for (long long rb = r0; rb < r1; rb += 2 * G) {
        float y0[G], y1[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long r = rb + 2 * g + h;
            const bool ok = r < r1;
            y0[g] = (ok && in0) ? v[r * v_stride + j] : 0.0f;
            y1[g] = (ok && in1) ? v[r * v_stride + 32 + j] : 0.0f;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (rb + 2 * g < r1) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0[g], y0[g], acc[0], 0, 0, 0);
                if (NT > 1) {
                    acc[T10] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1[g], y0[g], acc[T10], 0, 0, 0);
                    acc[T11] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1[g], y1[g], acc[T11], 0, 0, 0);
                }
            }
        }
    }
    float *dst = part + static_cast<long long>(blockIdx.x) * dim * dim;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int a = als_acc_row(g, h);
        if (a < dim && in0) dst[a * dim + j] = acc[0][g];
        if (NT > 1 && 32 + a < dim) {
            if (in0) {
                dst[(32 + a) * dim + j] = acc[T10][g];
                dst[j * dim + 32 + a] = acc[T10][g];
            }
            if (in1) dst[(32 + a) * dim + 32 + j] = acc[T11][g];
        }
    }
}

__global__ __launch_bounds__(256) void factor_gram_sum_kernel(int n_chunks, int dim, const float *__restrict__ part, float reg,
                                                              float *__restrict__ gram) {
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= dim * dim) return;
    float g = 0.0f;
    for (long long c = 0; c < n_chunks; ++c) g = __fadd_rn(g, part[c * dim * dim + e]);
    if (e / dim == e % dim) g = __fadd_rn(g, reg);
    gram[e] = g;
}

// rtrec_factor_gram_wide: one one-wave workgroup per (chunk, lower tile).  blockIdx.y counts the tiles (ti, tj), tj <= ti, row by
// row; the chain of tile (ti, tj) is the one factor_gram_partial_kernel runs for (1, 0): the A operand brings components
// 32 ti + j, the B operand 32 tj + j.  A diagonal tile is written once, whole (both triangles come out of the same products);
// a tile below the diagonal twice, once transposed.
__global__ __launch_bounds__(64) void factor_gram_wide_partial_kernel(int n_v, const float *__restrict__ v, long long v_stride,
                                                                      int dim, float *__restrict__ part) {
    constexpr int G = kAlsGroup;
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    int ti = 0, tj = static_cast<int>(blockIdx.y);
    while (tj > ti) tj -= ++ti;
    const long long r0 = static_cast<long long>(blockIdx.x) * kAlsGramChunk;
    long long r1 = r0 + kAlsGramChunk;
    if (r1 > n_v) r1 = n_v;
    const int ca = 32 * ti + j, cb = 32 * tj + j;
    const bool ina = ca < dim, inb = cb < dim;
    als_f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    for (long long rb = r0; rb < r1; rb += 2 * G) {
        float ya[G], yb[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long r = rb + 2 * g + h;
            const bool ok = r < r1;
            ya[g] = (ok && ina) ? v[r * v_stride + ca] : 0.0f;
            yb[g] = (ok && inb) ? v[r * v_stride + cb] : 0.0f;
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (rb + 2 * g < r1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ya[g], yb[g], acc, 0, 0, 0);
    }
    float *dst = part + static_cast<long long>(blockIdx.x) * dim * dim;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int a = 32 * ti + als_acc_row(g, h);
        if (a < dim && inb) {
            dst[a * dim + cb] = acc[g];
            if (ti != tj) dst[cb * dim + a] = acc[g];
        }
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_factor_gram_wide(int32_t n_v, const float *d_v, int64_t v_stride, int32_t dim, float reg, float *d_gram,
                                      void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace rtrec;
    if (dim < 1 || dim > kAlsWideMaxDim) return RTREC_ERR_UNSUPPORTED;
    if (n_v < 0 || v_stride < dim || !(reg >= 0.0f)) return RTREC_ERR_INVALID_ARG;
    if (!d_gram || (n_v > 0 && (!d_v || !d_workspace))) return RTREC_ERR_INVALID_ARG;
    if (workspace_bytes < RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim)) return RTREC_ERR_WORKSPACE;
    const int n_chunks = static_cast<int>((static_cast<long long>(n_v) + kAlsGramChunk - 1) / kAlsGramChunk);
    const int nt = (dim + 31) / 32;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(d_workspace);
    if (n_chunks > 0)
        hipLaunchKernelGGL(factor_gram_wide_partial_kernel, dim3(n_chunks, nt * (nt + 1) / 2), dim3(64), 0, st, n_v, d_v,
                           static_cast<long long>(v_stride), dim, part);
    hipLaunchKernelGGL(factor_gram_sum_kernel, dim3((dim * dim + 255) / 256), dim3(256), 0, st, n_chunks, dim, part, reg, d_gram);
    return launch_status();
}

extern "C" int rtrec_factor_gram(int32_t n_v, const float *d_v, int64_t v_stride, int32_t dim, float reg, float *d_gram,
                                 void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace rtrec;
    if (dim < 1 || dim > kAlsMaxDim) return RTREC_ERR_UNSUPPORTED;
    if (n_v < 0 || v_stride < dim || !(reg >= 0.0f)) return RTREC_ERR_INVALID_ARG;
    if (!d_gram || (n_v > 0 && (!d_v || !d_workspace))) return RTREC_ERR_INVALID_ARG;
    if (workspace_bytes < RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim)) return RTREC_ERR_WORKSPACE;
    const int n_chunks = static_cast<int>((static_cast<long long>(n_v) + kAlsGramChunk - 1) / kAlsGramChunk);
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(d_workspace);
    if (n_chunks > 0) {
        if (dim <= 32)
            hipLaunchKernelGGL(factor_gram_partial_kernel<1>, dim3(n_chunks), dim3(64), 0, st, n_v, d_v, static_cast<long long>(v_stride),
                               dim, part);
        else
            hipLaunchKernelGGL(factor_gram_partial_kernel<3>, dim3(n_chunks), dim3(64), 0, st, n_v, d_v, static_cast<long long>(v_stride),
                               dim, part);
    }
    hipLaunchKernelGGL(factor_gram_sum_kernel, dim3((dim * dim + 255) / 256), dim3(256), 0, st, n_chunks, dim, part, reg, d_gram);
    return launch_status();
}
