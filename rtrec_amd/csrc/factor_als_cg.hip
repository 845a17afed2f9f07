// rtrec_amd/csrc/factor_als_cg.hip -- one side of an implicit-feedback ALS half-step by conjugate gradient: per row of R a few CG
// steps on the system rtrec_factor_als_solve factors, without ever forming its matrix, every operation pinned.  dim up to 256.
//
// The contract is the comment of rtrec_factor_als_cg in include/rtrec_amd_ext.h.  In short, with A = G + sum_i w_i y_i y_i^T and
// b = sum_i (1 + w_i) y_i over the row's usable entries in storage order (usable as in factor_als.hip):
//   chain(u, v) the fmaf chain over ascending components          tree(u, v)  rounded products, then the xor-butterfly of rounded adds
//   mat(v)      G v, one fmaf chain per component over ascending b
//   residual    r = -mat(x), then per entry t = chain(y, x), r = fmaf(fl(fl(1 + w) - fl(w t)), y, r)
//   step        Ap = mat(p), then per entry t = chain(y, p), Ap = fmaf(fl(w t), y, Ap); den = tree(p, Ap); al = fl(rs / den);
//               x = fmaf(al, p, x); r = fmaf(-al, Ap, r); rn = tree(r, r); be = fl(rn / rs); p = fmaf(be, p, r)
//   status      0 finished; 1 row outside R (only the status and d_out_rs written) or no usable entry (zeros); 2 den not a
//               positive finite number, or a component of x that is not finite (zeros)
// Why two kinds of dot product: t is needed once per ENTRY, and a lane that owns an entry runs its chain alone, with no cross-lane
// traffic; den and rn are needed once per STEP over a vector that lives one component per lane, where a butterfly costs 6
// shuffles and a chain would cost dim dependent readlanes.
//
// What is built.  One workgroup of W = 1 / 2 / 4 waves per job (dim <= 64 / 128 / 256); thread c holds component c of x, r, p
// and Ap in registers (zero at and beyond dim).  The vector a pass multiplies by (x, then p) lies in LDS.  mat: thread a walks b
// ascending and reads G[b][a] -- row b, coalesced -- which is G[a][b] by the symmetry the contract demands; at dim 256 that is
// 256 KB per pass from L2, G does not fit LDS.  The entries of the row are taken 64 at a time: threads 0..63 read column and value,
// decide usable or not and pack the usable ones to the front (ballot and prefix count: storage order is kept); all threads stage
// their rows of V in LDS, 64 W + 1 floats apart (an odd pitch: lane = entry reads without a bank conflict); phase one, the first
// wave with lane = entry, runs each entry's chain against the vector and leaves the coefficient in LDS; phase two, lane =
// component, applies the block's entries in order, without a branch.  A skipped entry's row of V is never read; a block without
// a usable entry costs its index reads only.  tree: the cross-wave levels (h = 128, 64) are
// added by every wave from a copy in LDS, the six levels inside a wave by __shfl_xor; components at and beyond dim bring +0.0f,
// and the levels above D add it, which changes nothing but the sign of a zero.  Every wave gets the same bits, so every
// decision (stop, breakdown) is uniform.  Divisions are __fdiv_rn; float32 denormals are kept (hipcc's default mode).
// No atomics, no state; a job's result does not depend on the grid.  Jobs are taken in the order given (the engine names the
// longest rows first); jobs beyond the grid cap are reached by the grid stride.
// Malformed input cannot read out of range: offsets are clamped to [0, nnz], columns outside [0, n_v) are skipped before any read
// of V, a job row outside [0, n_rows) touches nothing of R, V or d_out.
// Not built: a long row split over several workgroups, several jobs per workgroup sharing the reads of G, phase one on more than
// one wave.  Measured: profiles/als_cg_<workload>.json (tools/als_bench.py --solver cg) where committed.
#include "factor_als.hip.h"

namespace rtrec {
namespace {

constexpr int kCgMaxGrid = 1 << 14;       // workgroups per launch; jobs beyond it are reached by the grid stride
constexpr int kCgBlock = 64;              // entries staged at a time
constexpr int kCgMaxSteps = 64;

template <int W>
__global__ __launch_bounds__(64 * W) void factor_als_cg_kernel(
        int n_jobs, const int32_t *__restrict__ job_rows, int n_rows, const int32_t *__restrict__ r_ptr,
        const int32_t *__restrict__ r_idx, const float *__restrict__ r_val, long long nnz, const float *__restrict__ v,
        long long v_stride, int n_v, int dim, const float *__restrict__ gram, float alpha, int cg_steps, int warm, float *out,
        long long out_stride, uint8_t *__restrict__ status, float *__restrict__ out_rs) {
    constexpr int T = 64 * W, LD = T + 1;
    __shared__ float Y[kCgBlock * LD];                  // the block's rows of V
    __shared__ float vec[T];                            // the vector of the pass: x, then p
    __shared__ float red[2][T];                         // tree's cross-wave copy, two in turn (one barrier per tree)
    __shared__ int col_s[kCgBlock];                     // the block's usable entries, packed in storage order: columns,
    __shared__ int nu_s;                                // how many,
    __shared__ float w_s[kCgBlock], coef_s[kCgBlock];   // w and the coefficient phase one leaves for phase two
    const int tid = static_cast<int>(threadIdx.x);
    const bool mine = tid < dim;                        // this thread owns component `tid`
    int flip = 0;

    auto tree = [&](float a, float b) -> float {
        float q = mine ? __fmul_rn(a, b) : 0.0f;
        if (W > 1) {
            float *buf = red[flip];
            flip ^= 1;
            buf[tid] = q;
            __syncthreads();
            const int l = tid & 63;
            if (W == 2) q = __fadd_rn(buf[l], buf[l + 64]);
            else q = __fadd_rn(__fadd_rn(buf[l], buf[l + 2 * 64]), __fadd_rn(buf[l + 64], buf[l + 3 * 64]));
        }
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) q = __fadd_rn(q, __shfl_xor(q, h, 64));
        return q;
    };
    auto mat = [&]() -> float {                         // (vec is in place and the barrier behind it passed)
        float s = 0.0f;
        if (mine) {
#pragma unroll 8
            for (int b = 0; b < dim; ++b) s = __fmaf_rn(gram[b * dim + tid], vec[b], s);
        }
        return s;
    };
    // one pass over the row's entries against vec: acc[a] = fmaf(coef, y[a], acc[a]) per usable entry in storage order, coef
    // from t = chain(y, vec): the residual's fl(fl(1 + w) - fl(w t)) or the step's fl(w t).  Returns whether an entry was usable
    auto sweep = [&](long long e0, long long e1, bool residual, float &acc) -> bool {
        bool any = false;
        for (long long base = e0; base < e1; base += kCgBlock) {
            const int nb = e1 - base >= kCgBlock ? kCgBlock : static_cast<int>(e1 - base);
            int col = -1;
            float wv = 0.0f;
            if (tid < nb) {
                const int c = r_idx[base + tid];
                const float w = __fmul_rn(alpha, r_val[base + tid]);
                if (c >= 0 && c < n_v && w > 0.0f) {
                    col = c;
                    wv = w;
                }
            }
            if (tid < kCgBlock) {                       // the first wave packs the usable entries to the front, order kept
                const unsigned long long usable = __ballot(col >= 0);
                if (col >= 0) {
                    const int slot = lane_prefix(usable);
                    col_s[slot] = col;
                    w_s[slot] = wv;
                }
                if (tid == 0) nu_s = __popcll(usable);
            }
            __syncthreads();
            const int nu = nu_s;
            if (nu == 0) {                              // (a block of skipped entries has no term at all)
                __syncthreads();                        // (nu_s is rewritten by the next block)
                continue;
            }
            any = true;
            for (int i = tid; i < nu * dim; i += T) {
                const int e = i / dim, c = i - e * dim;
                Y[e * LD + c] = v[static_cast<long long>(col_s[e]) * v_stride + c];
            }
            __syncthreads();
            if (tid < nu) {                             // phase one, lane = entry (the first wave)
                const float *y = Y + tid * LD;
                float t = 0.0f;
#pragma unroll 8
                for (int c = 0; c < dim; ++c) t = __fmaf_rn(y[c], vec[c], t);
                const float wt = __fmul_rn(w_s[tid], t);
                coef_s[tid] = residual ? __fsub_rn(__fadd_rn(1.0f, w_s[tid]), wt) : wt;
            }
            __syncthreads();
            if (mine) {                                 // phase two, lane = component
#pragma unroll 8
                for (int e = 0; e < nu; ++e) acc = __fmaf_rn(coef_s[e], Y[e * LD + tid], acc);
            }
            __syncthreads();                            // (Y, col_s, w_s, coef_s and nu_s are rewritten by the next block)
        }
        return any;
    };

    for (long long job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int x = job_rows ? job_rows[job] : static_cast<int>(job);
        if (x < 0 || x >= n_rows) {
            if (tid == 0) {
                status[job] = 1;
                if (out_rs) out_rs[job] = 0.0f;
            }
            continue;
        }
        long long e0 = r_ptr[x], e1 = r_ptr[x + 1];
        e0 = e0 < 0 ? 0 : (e0 > nnz ? nnz : e0);
        e1 = e1 < 0 ? 0 : (e1 > nnz ? nnz : e1);
        float *dst = out + static_cast<long long>(x) * out_stride;
        // ---- start: the stored vector, or zeros
        float xv = (warm && mine) ? dst[tid] : 0.0f;
        if (warm && __syncthreads_or(xv - xv != 0.0f)) xv = 0.0f;       // (inf - inf and NaN - NaN are NaN)
        __syncthreads();                                // (the last job's reads of vec are done)
        vec[tid] = xv;
        __syncthreads();
        // ---- residual
        float r = -mat();
        const bool any = sweep(e0, e1, true, r);
        if (!any) {                                     // no usable entry: zeros, whatever G holds
            if (mine) dst[tid] = 0.0f;
            if (tid == 0) {
                status[job] = 1;
                if (out_rs) out_rs[job] = 0.0f;
            }
            continue;
        }
        float p = r, rs = tree(r, r), last = rs;
        bool broken = false;
        if (!(rs < 1e-20f)) {
            for (int it = 0; it < cg_steps; ++it) {
                __syncthreads();                        // (the last pass's reads of vec are done)
                vec[tid] = p;
                __syncthreads();
                float ap = mat();
                sweep(e0, e1, false, ap);
                const float den = tree(p, ap);
                if (!(den > 0.0f) || den == __builtin_huge_valf()) {
                    broken = true;
                    break;
                }
                const float al = __fdiv_rn(rs, den);
                xv = __fmaf_rn(al, p, xv);
                r = __fmaf_rn(-al, ap, r);
                const float rn = tree(r, r);
                last = rn;
                if (rn < 1e-20f) break;
                const float be = __fdiv_rn(rn, rs);
                p = __fmaf_rn(be, p, r);
                rs = rn;
            }
        }
        const bool bad = __syncthreads_or(xv - xv != 0.0f) || broken;
        if (mine) dst[tid] = bad ? 0.0f : xv;
        if (tid == 0) {
            status[job] = bad ? 2 : 0;
            if (out_rs) out_rs[job] = last;
        }
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_factor_als_cg(int32_t n_jobs, const int32_t *d_job_rows, int32_t n_rows, const int32_t *d_r_ptr,
                                   const int32_t *d_r_idx, const float *d_r_val, int64_t nnz, const float *d_v, int64_t v_stride,
                                   int32_t n_v, int32_t dim, const float *d_gram, float alpha, int32_t cg_steps, int32_t warm_start,
                                   float *d_out, int64_t out_stride, uint8_t *d_status, float *d_out_rs, void *stream) {
    using namespace rtrec;
    if (dim < 1 || dim > kAlsWideMaxDim || cg_steps < 1 || cg_steps > kCgMaxSteps) return RTREC_ERR_UNSUPPORTED;
    if (n_jobs < 0 || n_rows < 0 || n_v < 0 || nnz < 0 || v_stride < dim || out_stride < dim || !(alpha > 0.0f))
        return RTREC_ERR_INVALID_ARG;
    if (n_jobs == 0) return RTREC_OK;
    if (!d_gram || !d_out || !d_status) return RTREC_ERR_INVALID_ARG;
    if ((n_rows > 0 && !d_r_ptr) || (nnz > 0 && (!d_r_idx || !d_r_val)) || (n_v > 0 && !d_v)) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned int>(n_jobs < kCgMaxGrid ? n_jobs : kCgMaxGrid));
#define RTREC_CG_LAUNCH(W)                                                                                                       \
    hipLaunchKernelGGL(factor_als_cg_kernel<W>, grid, dim3(64 * W), 0, st, n_jobs, d_job_rows, n_rows, d_r_ptr, d_r_idx, d_r_val, \
                       static_cast<long long>(nnz), d_v, static_cast<long long>(v_stride), n_v, dim, d_gram, alpha, cg_steps,   \
                       warm_start != 0 ? 1 : 0, d_out, static_cast<long long>(out_stride), d_status, d_out_rs)
    if (dim <= 64) RTREC_CG_LAUNCH(1);
    else if (dim <= 128) RTREC_CG_LAUNCH(2);
    else RTREC_CG_LAUNCH(4);
#undef RTREC_CG_LAUNCH
    return launch_status();
}
