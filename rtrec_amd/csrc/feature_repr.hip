// rtrec_amd/csrc/feature_repr.hip -- representations of a factor model with feature (tag) rows: sparse feature row x dense table.
//
// The reference's hybrid model never reads a user's or an item's vector from a table: it builds a sparse feature row per entity
// (the identity column plus the columns of its tags) and multiplies it into LightFM's per-feature embedding and bias tables
// (get_user_representations(features) = features * user_biases, features * user_embeddings: scipy's csr_matvec / csr_matvecs).
// This is that product, written straight into the two matrices factor_topk_kernel reads (the row-major user matrix and the
// component-major item matrix); the contract is the comment of rtrec_feature_repr in include/rtrec_amd_ext.h.  In short:
//   sum         s = +0.0f, then over the stored entries of the row in storage order s = fl(s + fl(v * e[col][c])): two roundings
//               per entry, never contracted to an fma (the library is compiled with -ffp-contract=off and the two steps are
//               __fmul_rn / __fadd_rn), float32 denormals kept; the bias is the same chain over d_bias
//   skipped     an entry whose column lies outside [0, n_features)
//   has         the row stores at least one entry that is not skipped; without one every slot is +0, the constant 1 included
//
// Mapping (the plain one; the only one built).  One thread per output slot: thread t of the launch owns slot t % width of job
// t / width, width = dim_e (+ 2 with a stacked bias), so a wave carries 64 / width rows when the rows are narrow (5 rows of a
// dim-12 model) instead of idling 52 lanes on one.  The lanes of one job read the same offsets, columns and values (one
// broadcast request each) and neighbouring components of one table row (one contiguous request), and walk the row's entries in
// a plain loop, so a row of hundreds of entries is merely slow.  A lane's chain is sequential by definition; memory latency is
// hidden by the other waves (256 threads per workgroup, up to 65,536 workgroups, a grid stride beyond that).  With the
// row-major output neighbouring lanes store neighbouring floats.  With the component-major output the lanes of one job store
// n_jobs floats apart and only the 64 / width jobs of a wave are neighbours.
// Measured (profiles/feature_c3s.json, tools/feature_bench.py; MI355X, 138,493 users and 26,744 items, identity + 3 tags per row,
// biases, medians of 10 spans of 20 calls): 11.4 us users + 4.7 us items for 12 slots, 56.7 + 18.1 us for 64 slots (3.0 / 3.1 TB/s
// of the bytes the shapes need for the users, 1.4 / 1.9 TB/s for the items), against 118.8 / 546.2 us for torch.sparse.mm plus
// the stacking and the transpose, and 3.6 / 16.0 ms for scipy + stack_bias + set_factors on the host.  At the users' rate the
// item launch would save 2.5 / 7 us per rebuild of all vectors, so the variant that stages a tile of 64 items in LDS and stores
// along the items was NOT built.  28 VGPRs, no scratch (the compiler's figures); no counters were collected.
// Plain vector loads and stores, no LDS, no atomics: a slot is written by exactly one thread, so nothing depends on the grid.
// Malformed input cannot read or write out of range: offsets are clamped to [0, nnz], a job row outside [0, n_f_rows) has no
// row, a column outside [0, n_features) is never used as an index, and the output strides are checked on the host.
#include "common.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {
namespace {

constexpr int kFeatureThreads = 256;
constexpr int kFeatureMaxGrid = 65536;      // workgroups per launch; slots beyond it are reached by the grid stride
constexpr int kFeatureMaxWidth = 256;       // the factor scorer's dim limit

struct FeatureArgs {
    int n_jobs;
    const int32_t *job_rows;
    int n_f_rows;
    const int32_t *f_ptr, *f_col;
    const float *f_val;
    long long nnz;
    const float *e;
    long long e_stride;
    int n_features, dim_e;
    const float *bias;
    int layout, width;
    float *out;
    long long row_stride, comp_stride;
    uint8_t *has;
};

__device__ __forceinline__ long long feature_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// one output slot of one job
__device__ __forceinline__ void feature_slot(const FeatureArgs &a, int r, int slot) {
    // what the slot holds: a component of the table (src = the component's column of e), the bias chain, or the constant
    const int bias_slot = a.layout == RTREC_FEATURE_USER ? 0 : (a.layout == RTREC_FEATURE_ITEM ? 1 : -1);
    const int one_slot = a.layout == RTREC_FEATURE_USER ? 1 : (a.layout == RTREC_FEATURE_ITEM ? 0 : -1);
    const bool is_one = slot == one_slot;
    const float *src = a.e + (slot - (a.layout == RTREC_FEATURE_PLAIN ? 0 : 2));
    long long src_stride = a.e_stride;
    if (slot == bias_slot) { src = a.bias; src_stride = 1; }
    const int x = a.job_rows ? a.job_rows[r] : r;
    long long lo = 0, hi = 0;
    if (x >= 0 && x < a.n_f_rows) {
        lo = feature_clamp(a.f_ptr[x], a.nnz);
        hi = feature_clamp(a.f_ptr[x + 1], a.nnz);
    }
    float s = 0.0f;
    int found = 0;
    for (long long k = lo; k < hi; ++k) {
        const int col = a.f_col[k];
        if (col < 0 || col >= a.n_features) continue;          // (a feature the table has not learned)
        found = 1;
        if (!is_one) {
            const float v = a.f_val ? a.f_val[k] : 1.0f;
            s = __fadd_rn(s, __fmul_rn(v, src[static_cast<long long>(col) * src_stride]));
        }
    }
    if (is_one) s = found ? 1.0f : 0.0f;
    a.out[static_cast<long long>(r) * a.row_stride + static_cast<long long>(slot) * a.comp_stride] = s;
    if (slot == 0 && a.has) a.has[r] = static_cast<uint8_t>(found);
}

__global__ __launch_bounds__(kFeatureThreads) void feature_repr_kernel(FeatureArgs a) {
    const long long total = static_cast<long long>(a.n_jobs) * a.width;
    const long long step = static_cast<long long>(gridDim.x) * kFeatureThreads;
    const long long first = static_cast<long long>(blockIdx.x) * kFeatureThreads + threadIdx.x;
    if (total <= 0x7fffffffll) {                                // (32-bit division: the usual case)
        const unsigned int w = static_cast<unsigned int>(a.width);
        for (long long t = first; t < total; t += step) {
            const unsigned int r = static_cast<unsigned int>(t) / w;
            feature_slot(a, static_cast<int>(r), static_cast<int>(static_cast<unsigned int>(t) - r * w));
        }
    } else {
        for (long long t = first; t < total; t += step) {
            const long long r = t / a.width;
            feature_slot(a, static_cast<int>(r), static_cast<int>(t - r * a.width));
        }
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_feature_repr(int32_t n_jobs, const int32_t *d_job_rows, int32_t n_f_rows, const int32_t *d_f_ptr,
                                  const int32_t *d_f_col, const float *d_f_val, int64_t nnz, const float *d_e, int64_t e_stride,
                                  int32_t n_features, int32_t dim_e, const float *d_bias, int32_t layout, float *d_out,
                                  int64_t row_stride, int64_t comp_stride, uint8_t *d_has, void *stream) {
    using namespace rtrec;
    if (n_jobs < 0 || n_f_rows < 0 || nnz < 0 || n_features < 0) return RTREC_ERR_INVALID_ARG;
    if (layout != RTREC_FEATURE_PLAIN && layout != RTREC_FEATURE_USER && layout != RTREC_FEATURE_ITEM) return RTREC_ERR_UNSUPPORTED;
    const int extra = layout == RTREC_FEATURE_PLAIN ? 0 : 2;
    if (dim_e < 1 || dim_e > kFeatureMaxWidth - extra) return RTREC_ERR_UNSUPPORTED;
    const int width = dim_e + extra;
    if (e_stride < dim_e) return RTREC_ERR_INVALID_ARG;
    // the two orientations: row-major (rows at least `width` apart) or component-major (components at least n_jobs apart);
    // anything else would let two slots share an address
    if (!((comp_stride == 1 && row_stride >= width) || (row_stride == 1 && comp_stride >= n_jobs))) return RTREC_ERR_INVALID_ARG;
    if (n_jobs == 0) return RTREC_OK;
    if (!d_out) return RTREC_ERR_INVALID_ARG;
    if ((n_f_rows > 0 && !d_f_ptr) || (nnz > 0 && !d_f_col) || (n_features > 0 && !d_e)) return RTREC_ERR_INVALID_ARG;
    if (extra && n_features > 0 && !d_bias) return RTREC_ERR_INVALID_ARG;
    FeatureArgs a;
    a.n_jobs = n_jobs; a.job_rows = d_job_rows; a.n_f_rows = n_f_rows; a.f_ptr = d_f_ptr; a.f_col = d_f_col; a.f_val = d_f_val;
    a.nnz = static_cast<long long>(nnz); a.e = d_e; a.e_stride = static_cast<long long>(e_stride); a.n_features = n_features;
    a.dim_e = dim_e; a.bias = d_bias; a.layout = layout; a.width = width; a.out = d_out;
    a.row_stride = static_cast<long long>(row_stride); a.comp_stride = static_cast<long long>(comp_stride); a.has = d_has;
    const long long total = static_cast<long long>(n_jobs) * width;
    const long long blocks = (total + kFeatureThreads - 1) / kFeatureThreads;
    (void)hipGetLastError();
    hipLaunchKernelGGL(feature_repr_kernel, dim3(static_cast<unsigned int>(blocks < kFeatureMaxGrid ? blocks : kFeatureMaxGrid)),
                       dim3(kFeatureThreads), 0, static_cast<hipStream_t>(stream), a);
    return launch_status();
}
