// rtrec_amd/csrc/factor_norms.hip -- one Euclidean norm per vector of a dense float32 matrix: the divisors of the cosine top-k.
//
// The reference's hybrid model takes item_norms = ||target_i|| with numpy before it calls implicit.topk(item_norms=...)
// (rtrec/models/hybrid.py, _similar_items).  The contract is the comment of rtrec_factor_norms in include/rtrec_amd_ext.h:
//   n2 = +0.0f, then n2 = fmaf(v[c], v[c], n2) for c = 0 .. dim-1 ascending; norm = sqrt(n2) correctly rounded, denormals kept
// which is rtrec_factor_topk's score of a vector with itself, bit for bit.  numpy rounds every square on its own and adds them in
// its pairwise order, so the two differ in the last bits on some vectors (DESIGN, divergences; tests/test_similar_host.py counts
// them).  The root is taken in float64 and rounded once more: a 53-bit root rounded to 24 bits cannot double-round wrongly, and
// it does not depend on how the compiler expands a float32 sqrtf for denormal inputs (sqrtf itself was not tried).
// Mapping: one thread per vector.  Component-major (row_stride == 1) neighbouring threads read neighbouring items, 256 bytes per
// wave and component; row-major a thread walks its own row.  Plain loads, no LDS, no atomics; nothing depends on scheduling.
// Not measured on its own: it runs once per set_factors, on 26,744 x 64 floats (6.8 MB read).
#include "common.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {
namespace {

constexpr int kNormThreads = 256;
constexpr int kNormMaxGrid = 65536;      // workgroups per launch; vectors beyond it are reached by the grid stride
constexpr int kNormMaxDim = 256;         // the factor scorer's dim limit

__global__ __launch_bounds__(kNormThreads) void factor_norms_kernel(int n, const float *__restrict__ v, long long row_stride,
                                                                    long long comp_stride, int dim, float *__restrict__ out) {
    const long long step = static_cast<long long>(gridDim.x) * kNormThreads;
    for (long long r = static_cast<long long>(blockIdx.x) * kNormThreads + threadIdx.x; r < n; r += step) {
        const float *src = v + r * row_stride;
        float n2 = 0.0f;
        for (int c = 0; c < dim; ++c) {
            const float x = src[c * comp_stride];
            n2 = __fmaf_rn(x, x, n2);
        }
        out[r] = static_cast<float>(__dsqrt_rn(static_cast<double>(n2)));
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_factor_norms(int32_t n, const float *d_v, int64_t row_stride, int64_t comp_stride, int32_t dim, float *d_out,
                                  void *stream) {
    using namespace rtrec;
    if (n < 0) return RTREC_ERR_INVALID_ARG;
    if (dim < 1 || dim > kNormMaxDim) return RTREC_ERR_UNSUPPORTED;
    if (!((comp_stride == 1 && row_stride >= dim) || (row_stride == 1 && comp_stride >= n))) return RTREC_ERR_INVALID_ARG;
    if (n == 0) return RTREC_OK;
    if (!d_v || !d_out) return RTREC_ERR_INVALID_ARG;
    const long long blocks = (static_cast<long long>(n) + kNormThreads - 1) / kNormThreads;
    (void)hipGetLastError();
    hipLaunchKernelGGL(factor_norms_kernel, dim3(static_cast<unsigned int>(blocks < kNormMaxGrid ? blocks : kNormMaxGrid)),
                       dim3(kNormThreads), 0, static_cast<hipStream_t>(stream), n, d_v, static_cast<long long>(row_stride),
                       static_cast<long long>(comp_stride), dim, d_out);
    return launch_status();
}
