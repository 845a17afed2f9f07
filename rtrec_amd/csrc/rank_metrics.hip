// rtrec_amd/csrc/rank_metrics.hip -- the nine ranking figures of Recommender.evaluate, per user, from top-k lists that are
// already on the device (rtrec/utils/metrics.py:5-313 as restated by rtrec_amd/utils/metrics.py::_query_metrics).
//
// Two steps per tile of 64 users, one wave per tile:
//   membership   lane = (user, list position): a binary search of the recommended item in the user's sorted ground truth,
//                __ballot -> one relevance word per user.  A list of `size` entries takes P = size rounded up to a power
//                of two lanes, so a pass of the wave covers 64 / P users and P passes cover the tile.
//   figures      lane = user: the order-sensitive float64 part walks the set bits of the word in ascending position.
// No libm on the device: 1 / log2(i + 2) and its prefix sums come in as tables made with the host's math.log2, so every
// figure is a fixed sequence of float64 additions and correctly rounded divisions (-ffp-contract=off, no fast-math): the
// same IEEE operations CPython performs.
#include "common.hip.h"
#include "../../include/rtrec_amd.h"

namespace rtrec {

__device__ __forceinline__ bool in_sorted(const int32_t *__restrict__ v, long long lo, long long hi, int32_t x) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        const int32_t m = v[mid];
        if (m == x) return true;
        if (m < x) lo = mid + 1; else hi = mid;
    }
    return false;
}

__global__ __launch_bounds__(64) void rank_metrics_kernel(
        int n_rows, int size, int log2_p, const int32_t *__restrict__ ids, int stride, const int32_t *__restrict__ counts,
        const long long *__restrict__ truth_ptr, const int32_t *__restrict__ truth_items, long long n_truth,
        const int32_t *__restrict__ truth_len, const double *__restrict__ discount, const double *__restrict__ ideal,
        unsigned long long *__restrict__ out_rel, int32_t *__restrict__ out_tp, double *__restrict__ out_metrics) {
    const int lane = lane_id();
    const int P = 1 << log2_p, users_per_pass = 64 >> log2_p;
    const unsigned long long word = P == 64 ? ~0ull : (1ull << P) - 1ull;
    const int sub = lane >> log2_p, pos = lane & (P - 1);
    for (long long base = 64ll * blockIdx.x; base < n_rows; base += 64ll * gridDim.x) {
        // ---- membership: pass j serves users base + j * users_per_pass ...; lane `sub * P + pos` looks at one list entry
        unsigned long long rel = 0;
        for (int j = 0; j < P; ++j) {
            const long long u = base + j * users_per_pass + sub;
            bool hit = false;
            if (u < n_rows && pos < size) {
                const int c = counts[u];
                if (pos < c) {
                    long long b = truth_ptr[u], e = truth_ptr[u + 1];
                    b = b < 0 ? 0 : (b > n_truth ? n_truth : b);          // a malformed CSR must not read out of bounds
                    e = e < b ? b : (e > n_truth ? n_truth : e);
                    hit = in_sorted(truth_items, b, e, ids[u * stride + pos]);
                }
            }
            const unsigned long long hits = __ballot(hit);
            const int mine = lane - j * users_per_pass;                   // this lane's user was served by this pass?
            if (mine >= 0 && mine < users_per_pass) rel = (hits >> (mine << log2_p)) & word;
        }
        // ---- figures: lane = user
        const long long u = base + lane;
        if (u < n_rows) {
            const int c = counts[u];
            const int k = c < size ? (c < 0 ? 0 : c) : size;
            const int n = truth_len[u];
            const int tp = __popcll(rel);
            const int denom = n < size ? n : size;                            // min(len(ground_truth), size)
            double dcg = 0.0, ap_sum = 0.0;
            long long ordered_pairs = 0;                                      // (hit, later miss) pairs
            int running = 0, first = -1;
            for (unsigned long long m = rel; m; m &= m - 1) {
                const int i = __ffsll(static_cast<long long>(m)) - 1;
                if (first < 0) first = i;
                ++running;
                dcg = dcg + discount[i];
                ap_sum = ap_sum + static_cast<double>(running) / static_cast<double>(i + 1);
                ordered_pairs += (k - 1 - i) - (tp - running);
            }
            const double both_empty = c == 0 ? 1.0 : 0.0;
            double prec, rec, ap, auc;
            if (n == 0) {
                prec = rec = ap = auc = both_empty;
            } else {
                prec = k ? static_cast<double>(tp) / static_cast<double>(k) : 0.0;
                rec = static_cast<double>(tp) / static_cast<double>(n);
                ap = denom ? ap_sum / static_cast<double>(denom) : 0.0;
                if (c == 0 || tp == 0) auc = 0.0;
                else if (tp == k) auc = 1.0;
                else auc = static_cast<double>(ordered_pairs) / static_cast<double>(tp * (k - tp));
            }
            double f1;
            if (n == 0 && c == 0) f1 = 1.0;
            else f1 = (prec + rec) > 0.0 ? (2.0 * prec * rec) / (prec + rec) : 0.0;
            const double idcg = denom > 0 ? ideal[denom] : 0.0;
            double *o = out_metrics + u * 8;
            o[0] = prec;
            o[1] = rec;
            o[2] = f1;
            o[3] = idcg > 0.0 ? dcg / idcg : 0.0;
            o[4] = tp ? 1.0 : 0.0;
            o[5] = first < 0 ? 0.0 : 1.0 / static_cast<double>(first + 1);
            o[6] = ap;
            o[7] = auc;
            out_rel[u] = rel;
            out_tp[u] = tp;
        }
    }
}

}  // namespace rtrec

using namespace rtrec;

extern "C" int rtrec_rank_metrics(int32_t n_rows, int32_t size, const int32_t *d_ids, int32_t stride, const int32_t *d_counts,
                                  const int64_t *d_truth_ptr, const int32_t *d_truth_items, int64_t n_truth,
                                  const int32_t *d_truth_len, const double *d_discount, const double *d_ideal,
                                  uint64_t *d_rel, int32_t *d_tp, double *d_metrics, void *stream) {
    if (n_rows < 0 || n_truth < 0) return RTREC_ERR_INVALID_ARG;
    if (size < 1 || size > 64) return RTREC_ERR_UNSUPPORTED;
    if (stride < size) return RTREC_ERR_INVALID_ARG;
    if (n_rows == 0) return RTREC_OK;
    if (!d_ids || !d_counts || !d_truth_ptr || !d_truth_len || !d_discount || !d_ideal || !d_rel || !d_tp || !d_metrics ||
        (n_truth > 0 && !d_truth_items))
        return RTREC_ERR_INVALID_ARG;
    (void)hipGetLastError();
    int log2_p = 0;
    while ((1 << log2_p) < size) ++log2_p;
    const int tiles = (n_rows - 1) / 64 + 1;
    const int grid = tiles < 16384 ? tiles : 16384;
    hipLaunchKernelGGL(rank_metrics_kernel, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream), n_rows, size, log2_p, d_ids,
                       stride, d_counts, reinterpret_cast<const long long *>(d_truth_ptr), d_truth_items,
                       static_cast<long long>(n_truth), d_truth_len, d_discount, d_ideal,
                       reinterpret_cast<unsigned long long *>(d_rel), d_tp, d_metrics);
    return rtrec::launch_status();
}
