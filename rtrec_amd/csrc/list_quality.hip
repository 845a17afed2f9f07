// rtrec_amd/csrc/list_quality.hip -- list quality: per list the intra-list similarity sum, its linked pairs, a weight sum, and the
// catalogue exposure of all lists together, with W as the item-item similarity.
//
// The measuring stage behind diversify.hip: what a value of `diversity` buys is read off the lists where they lie, in HBM.  The
// contract is the comment of rtrec_slim_list_quality in include/rtrec_amd_ext.h; in short:
//   counted     a position below counts[r] whose id lies in [0, n_items) and which no earlier counted position repeats
//   sim(a, b)   max(|W[a, b]|, |W[b, a]|) over the stored weights (0 where none is stored); a NaN weight is ignored
//   s_p         the float32 sum from +0 of sim(id_p, id_q) over the counted q < p, ascending, one rounded add each (__fadd_rn)
//   sim_sum     the float32 sum from +0 of the s_p, ascending p; weight_sum the same over item_weight[id_p]
//
// Mapping (the frame is list_stage.hip.h's).  Thread t owns the positions t, t + NT, ...  The
// ids go to LDS, every position looks for its id at a lower position (the de-duplication is a function of the ids alone, so
// the counted set is the same in every mapping), then the owner of p caches the span of column id_p in LDS, walks the counted
// q < p with two binary searches each -- id_q in its own column, id_p in column id_q -- and leaves s_p, its linked pairs and its
// weight in LDS; one thread adds them up in position order.  This is the plain position-owner form: at a top-10 list ten lanes
// of the wave work and the last walks nine pairs, so the kernel is bound by the latency of those dependent loads like
// diversify_lists_kernel; the LDS arrays are sized by the list (64 / 256 / 1024 positions, 24 bytes each) so that
// short lists keep 32 one-wave workgroups per CU and occupancy hides the latency.  No other mapping has been measured.
// Malformed input cannot read out of range: CSC offsets are clamped to [0, wc_nnz], counts to [0, list_k], and an id outside
// [0, n_items) is never counted.
#include "list_stage.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {
namespace {

constexpr int kQualMaxList = 1024;      // list_k limit: the LDS arrays of the widest instantiation

template <int WAVES, int CAP>
__global__ __launch_bounds__(WAVES * 64) void list_quality_kernel(
        int n_rows, int n_items, const int32_t *__restrict__ wc_ptr, const int32_t *__restrict__ wc_row,
        const float *__restrict__ wc_val, long long wc_nnz, const int32_t *__restrict__ ids, long long ids_stride, int list_k,
        const int32_t *__restrict__ counts, const float *__restrict__ item_weight, int32_t *__restrict__ exposure,
        int32_t *__restrict__ out_n, float *__restrict__ out_sim_sum, int32_t *__restrict__ out_linked,
        float *__restrict__ out_weight_sum) {
    constexpr int NT = WAVES * 64;
    __shared__ int32_t lid[CAP];        // the position's item, -1: it is not counted
    __shared__ int32_t lcs[CAP];        // column id_p of W: its clamped start ...
    __shared__ int32_t llen[CAP];       // ... and length
    __shared__ float ls[CAP];           // s_p
    __shared__ int32_t llink[CAP];      // the linked pairs (q, p), q < p
    __shared__ float lw[CAP];           // item_weight[id_p]
    const int tid = static_cast<int>(threadIdx.x);
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int cnt = clamp_count(counts[r], list_k);
        for (int p = tid; p < list_k; p += NT) {
            int id = -1;
            if (p < cnt) id = ids[r * ids_stride + p];
            lid[p] = id >= 0 && id < n_items ? id : -1;
        }
        __syncthreads();
        // ---- an item shown twice is judged once, at its first place: a position whose id stands at a lower one leaves.  All
        // positions read the ids as they were loaded, so the answer does not depend on who asks first.
        bool dup[(CAP + NT - 1) / NT];
#pragma unroll
        for (int i = 0; i < (CAP + NT - 1) / NT; ++i) {
            const int p = tid + i * NT;
            dup[i] = false;
            if (p < list_k) {
                const int id = lid[p];
                if (id >= 0)
                    for (int q = 0; q < p; ++q)
                        if (lid[q] == id) { dup[i] = true; break; }
            }
        }
        __syncthreads();                // every position has read the loaded ids
#pragma unroll
        for (int i = 0; i < (CAP + NT - 1) / NT; ++i) {
            const int p = tid + i * NT;
            if (p >= list_k) continue;
            if (dup[i]) lid[p] = -1;
            const int id = lid[p];
            long long s = 0, e = 0;
            if (id >= 0) { s = wc_ptr[id]; e = wc_ptr[id + 1]; clamp_span(s, e, wc_nnz); }
            lcs[p] = static_cast<int32_t>(s);       // (wc_ptr holds int32 offsets, and the clamp keeps them non-negative)
            llen[p] = static_cast<int32_t>(e - s);
        }
        __syncthreads();                // the counted set and its column spans are in LDS
        // ---- the owner of p walks the counted q < p upwards
        for (int p = tid; p < list_k; p += NT) {
            const int idp = lid[p];
            float sp = 0.0f, wp = 0.0f;
            int linked = 0;
            if (idp >= 0) {
                const int32_t *prow = wc_row + lcs[p];
                const float *pval = wc_val + lcs[p];
                const int plen = llen[p];
                for (int q = 0; q < p; ++q) {
                    const int idq = lid[q];
                    if (idq < 0) continue;
                    float sim = 0.0f, w;
                    if (find_sorted(prow, pval, plen, idq, w)) raise_abs(sim, w);                          // W[id_q, id_p]
                    if (find_sorted(wc_row + lcs[q], wc_val + lcs[q], llen[q], idp, w)) raise_abs(sim, w);  // W[id_p, id_q]
                    sp = __fadd_rn(sp, sim);
                    linked += sim > 0.0f ? 1 : 0;
                }
                if (item_weight) wp = item_weight[idp];
                if (exposure) atomicAdd(exposure + idp, 1);
            }
            ls[p] = sp;
            llink[p] = linked;
            lw[p] = wp;
        }
        __syncthreads();                // every position's figures are in LDS
        if (tid == 0) {
            float sim_sum = 0.0f, weight_sum = 0.0f;
            int m = 0, linked = 0;
            for (int p = 0; p < list_k; ++p) {
                if (lid[p] < 0) continue;
                ++m;
                sim_sum = __fadd_rn(sim_sum, ls[p]);
                weight_sum = __fadd_rn(weight_sum, lw[p]);
                linked += llink[p];
            }
            out_n[r] = m;
            out_sim_sum[r] = sim_sum;
            out_linked[r] = linked;
            out_weight_sum[r] = weight_sum;         // (+0.0f without item_weight: every lw is +0.0f then)
        }
        __syncthreads();                // the row is done: LDS may be overwritten
    }
}

}  // namespace
}  // namespace rtrec

extern "C" int rtrec_slim_list_quality(int32_t n_rows, int32_t n_items, const int32_t *d_wc_ptr, const int32_t *d_wc_row,
                                       const float *d_wc_val, int64_t wc_nnz, const int32_t *d_ids, int64_t ids_stride,
                                       int32_t list_k, const int32_t *d_counts, const float *d_item_weight, int32_t *d_exposure,
                                       int32_t waves_per_row, int32_t *d_out_n, float *d_out_sim_sum, int32_t *d_out_linked,
                                       float *d_out_weight_sum, void *stream) {
    using namespace rtrec;
    if (n_rows < 0 || n_items < 0 || wc_nnz < 0) return RTREC_ERR_INVALID_ARG;
    if (list_k < 1 || list_k > kQualMaxList) return RTREC_ERR_UNSUPPORTED;
    if (!list_waves_valid(waves_per_row)) return RTREC_ERR_UNSUPPORTED;
    if (ids_stride < list_k) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_ids || !d_counts || !d_out_n || !d_out_sim_sum || !d_out_linked || !d_out_weight_sum) return RTREC_ERR_INVALID_ARG;
    if (!csc_present(n_items, d_wc_ptr, wc_nnz, d_wc_row, d_wc_val)) return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long nnz = static_cast<long long>(wc_nnz), is = static_cast<long long>(ids_stride);
    list_dispatch(list_waves(waves_per_row, n_rows, list_k), list_k, [&](auto W, auto CAP) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(list_quality_kernel<W(), CAP()>), dim3(list_grid(n_rows)), dim3(W() * 64), 0, st, n_rows,
                           n_items, d_wc_ptr, d_wc_row, d_wc_val, nnz, d_ids, is, list_k, d_counts, d_item_weight, d_exposure, d_out_n,
                           d_out_sim_sum, d_out_linked, d_out_weight_sum);
    });
    return launch_status();
}
