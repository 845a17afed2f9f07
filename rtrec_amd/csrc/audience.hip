// rtrec_amd/csrc/audience.hip -- the audience of an item: the top_n users by score(u, i) = sum_j X[u, j] * W[j, i].
//
// The reference has no such call; the contract is the comment of rtrec_slim_audience_topk in include/rtrec_amd.h.  It is the
// scoring product read the other way round: column i of W holds at most K weights (feature selection), so the only users with a
// score for i are those stored in the CSC columns of X of those <= K items j, and the score of every one of them is built by
// walking those columns in ascending j -- fl32(x_uj * w_ji) added in float32 from 0.0f, the order scipy's csr_matmat (and the
// scoring kernels) use for the pair.
//
// audience_tile_kernel: one workgroup of 8 waves per (user tile of 8,192 rows, query item).
//   * The tile's accumulators live in LDS (32 KiB).  The bit pattern 0xffffffff means "no support yet": it is a NaN payload no
//     float32 addition produces from other inputs, so support >= 1 is "the slot holds anything else" and no bitmap is needed.
//   * Wave w owns rows [w * 1024, (w + 1) * 1024) of the tile.  For up to 56 entries of W's column at a time (K = 50 fits one
//     round) the 512 threads binary-search, in crow, the 9 wave boundaries of every X column; then each wave walks its own
//     segment of every column in ascending j.  Inside one column a user occurs once (a conflict-free scatter); across columns a
//     wave's LDS operations execute in issue order and the accesses are volatile, so the compiler keeps the read-modify-writes
//     in column order: no float atomics, no barrier between columns.  The first 64 entries of the next column are loaded while
//     the current column is applied.
//   * The users stored in column i of X are cleared (filter_interacted), then those outside the bitmap.  What is left is
//     eligible and counted.  A NaN accumulator (rerank's rule: counted, never listed) is cleared after it was counted, so the
//     selection sees numbers only and is told how many; +-inf are numbers.
//   * Selection: a radix select (8 bits a pass) on the UNIQUE key  [order-preserving score bits | 8191 - local row], so the
//     top_n-th key is an exact threshold: everything at or above it is taken -- the lower row first among equal scores -- and
//     the <= 1024 winners are sorted by a bitonic network in LDS.  -0.0f is keyed as +0.0f (an accumulation that starts from
//     +0.0f never yields -0.0f, so the score decoded from the key is the accumulator's bit pattern).
//   * The tile's sorted list goes to the workspace as 64-bit records [score key | ~user row], with its length and the tile's
//     number of eligible users.
// audience_merge_kernel: one workgroup per query item runs the same select + sort over the tiles' records (their keys are
// unique across tiles too) and writes users / scores / count / eligible, every slot of them.
// rtrec_slim_merge_topk is not reused: it orders by (score, aux, id) with the larger aux first and is built for the row-major
// record layout of the scoring exchange; the record above carries the whole order in one integer compare.
//
// Malformed input cannot read out of range: CSC offsets are clamped to the arrays' lengths, an item id outside [0, n_items) has
// no column, a row outside the wave's range (an unsorted column) is skipped.
#include "row_lookup.hip.h"
#include "../../include/rtrec_amd.h"

namespace rtrec {

constexpr int kAudTile = 8192;                     // users per workgroup: 32 KiB of accumulators
constexpr int kAudThreads = 512;
constexpr int kAudWaves = kAudThreads / 64;
constexpr int kAudSub = kAudTile / kAudWaves;      // users per wave
constexpr int kAudCols = 56;                       // W-column entries per round: 9 boundaries x 56 columns <= 512 threads
constexpr int kAudMaxTop = 1024;
constexpr uint32_t kNoSupport = 0xffffffffu;
constexpr size_t kAudWorkspaceCap = size_t(256) << 20;

// Larger float <=> larger key; -0.0f and +0.0f share a key; kNoSupport maps to 0, below every other key.
__device__ __forceinline__ uint32_t score_key(uint32_t b) {
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t key_score(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

struct SelectShared {
    unsigned hist[256];
    unsigned long long prefix;
    int need;
    int cnt;
};

// The min(top_n, n_valid) largest of the keys key(0 .. n) -- 0 = no candidate, n_valid = how many are not 0, all others
// distinct and below 2^kBits -- sorted descending into win[0 .. return value).  Called by all kAudThreads threads after a
// barrier; top_n <= kAudMaxTop.
template <int kBits, class KeyFn>
__device__ int select_sorted(KeyFn key, int n, int n_valid, int top_n, unsigned long long *win, SelectShared &sh) {
    const int tid = static_cast<int>(threadIdx.x);
    unsigned long long thr = 1ull;
    if (n_valid > top_n) {                                                // find the top_n-th key, 8 bits a pass
        if (tid == 0) { sh.prefix = 0ull; sh.need = top_n; }
        for (int shift = kBits - 8; shift >= 0; shift -= 8) {
            if (tid < 256) sh.hist[tid] = 0u;
            __syncthreads();
            const unsigned long long prefix = sh.prefix;
            const bool first = shift == kBits - 8;
            for (int i = tid; i < n; i += kAudThreads) {
                const unsigned long long k = key(i);
                if (k != 0ull && (first || (k >> (shift + 8)) == prefix)) atomicAdd(&sh.hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {                                               // the digit at which the suffix count reaches `need`
                const unsigned c0 = sh.hist[4 * tid], c1 = sh.hist[4 * tid + 1], c2 = sh.hist[4 * tid + 2], c3 = sh.hist[4 * tid + 3];
                const unsigned s = c0 + c1 + c2 + c3;
                unsigned S = s;                                           // bins of lanes >= tid
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned o = __shfl_down(S, d, 64);
                    if (tid + d < 64) S += o;
                }
                const unsigned need = static_cast<unsigned>(sh.need);
                const unsigned long long m = __ballot(S >= need);
                const int l = 63 - __clzll(static_cast<long long>(m));
                if (tid == l) {
                    unsigned above = S - s;
                    int d = 0;
                    if (above + c3 >= need) d = 3;
                    else if (above + c3 + c2 >= need) { above += c3; d = 2; }
                    else if (above + c3 + c2 + c1 >= need) { above += c3 + c2; d = 1; }
                    else above += c3 + c2 + c1;
                    sh.need = static_cast<int>(need - above);
                    sh.prefix = (prefix << 8) | static_cast<unsigned long long>(4 * l + d);
                }
            }
            __syncthreads();
        }
        thr = sh.prefix;
    }
    if (tid == 0) sh.cnt = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kAudThreads) {
        const unsigned long long k = key(i);
        if (k >= thr) {
            const int p = atomicAdd(&sh.cnt, 1);
            if (p < kAudMaxTop) win[p] = k;
        }
    }
    __syncthreads();
    const int cnt = sh.cnt < top_n ? sh.cnt : top_n;
    int P = 1;
    while (P < cnt) P <<= 1;
    for (int i = cnt + tid; i < P; i += kAudThreads) win[i] = 0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {                                    // bitonic network, descending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kAudThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = win[i], b = win[x];
                    if (((i & k) == 0) ? a < b : a > b) { win[i] = b; win[x] = a; }
                }
            }
            __syncthreads();
        }
    }
    return cnt;
}

// first p in [lo, hi) with row[p] >= R
__device__ __forceinline__ long long lower_bound_row(const int32_t *__restrict__ row, long long lo, long long hi, long long R) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (static_cast<long long>(row[mid]) < R) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kAudThreads) void audience_tile_kernel(
        int n_q, const int32_t *__restrict__ items, int n_users, int n_items, int n_tiles, const int32_t *__restrict__ xc_ptr,
        const int32_t *__restrict__ xc_row, const float *__restrict__ xc_val, long long xc_nnz, const int32_t *__restrict__ wc_ptr,
        const int32_t *__restrict__ wc_row, const float *__restrict__ wc_val, long long wc_nnz, int top_n, int filter_interacted,
        const int32_t *__restrict__ user_mask, unsigned long long *__restrict__ ws_keys, int32_t *__restrict__ ws_cnt) {
    __shared__ uint32_t acc[kAudTile];
    __shared__ unsigned long long win[kAudMaxTop];
    __shared__ int bounds[kAudWaves + 1][kAudCols];
    __shared__ float wv[kAudCols];
    __shared__ SelectShared sh;
    __shared__ int misc[4];                                               // the filter's segment, eligible users, those with a number
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int q = static_cast<int>(blockIdx.x % static_cast<unsigned>(n_q));      // tile-major: the workgroups in flight share
    const int tile = static_cast<int>(blockIdx.x / static_cast<unsigned>(n_q));   // one slice of X's popular columns in L2
    const long long tile_lo = static_cast<long long>(tile) * kAudTile;
    const long long slot = static_cast<long long>(q) * n_tiles + tile;
    const int item = items[q];
    long long ws = 0, we = 0;
    if (item >= 0 && item < n_items) { ws = wc_ptr[item]; we = wc_ptr[item + 1]; clamp_span(ws, we, wc_nnz); }
    if (we == ws) {                                                       // no column: nobody has support
        if (tid == 0) { ws_cnt[2 * slot] = 0; ws_cnt[2 * slot + 1] = 0; }
        return;
    }
    for (int i = tid; i < kAudTile; i += kAudThreads) acc[i] = kNoSupport;
    if (tid == 0) { misc[2] = 0; misc[3] = 0; }
    __syncthreads();

    volatile uint32_t *vacc = acc + wave * kAudSub;                       // this wave's rows; volatile: column order is kept
    const long long sub_lo = tile_lo + static_cast<long long>(wave) * kAudSub;
    auto apply = [&](int r, float v, float w) {
        const long long d = static_cast<long long>(r) - sub_lo;
        if (d >= 0 && d < kAudSub && r < n_users) {
            const uint32_t a = vacc[d];
            const float f = a == kNoSupport ? 0.0f : __uint_as_float(a);
            vacc[d] = __float_as_uint(__fadd_rn(f, __fmul_rn(v, w)));     // one rounded multiply, one rounded add: never fused
        }
    };
    for (long long base = ws; base < we; base += kAudCols) {
        const int nc = we - base < kAudCols ? static_cast<int>(we - base) : kAudCols;
        for (int t = tid; t < nc * (kAudWaves + 1); t += kAudThreads) {
            const int c = t % nc, b = t / nc;
            const int j = wc_row[base + c];
            long long lo = 0, hi = 0;
            if (j >= 0 && j < n_items) { lo = xc_ptr[j]; hi = xc_ptr[j + 1]; clamp_span(lo, hi, xc_nnz); }
            bounds[b][c] = static_cast<int>(lower_bound_row(xc_row, lo, hi, tile_lo + static_cast<long long>(b) * kAudSub));
            if (b == 0) wv[c] = wc_val[base + c];
        }
        __syncthreads();
        int nr = -1;                                                      // the first 64 entries of the next column, loaded early
        float nv = 0.0f;
        if (bounds[wave][0] + lane < bounds[wave + 1][0]) { nr = xc_row[bounds[wave][0] + lane]; nv = xc_val[bounds[wave][0] + lane]; }
        for (int c = 0; c < nc; ++c) {
            const int s = bounds[wave][c], e = bounds[wave + 1][c];
            const float w = wv[c];
            const int r = nr;
            const float v = nv;
            nr = -1;
            if (c + 1 < nc) {
                const int p = bounds[wave][c + 1] + lane;
                if (p < bounds[wave + 1][c + 1]) { nr = xc_row[p]; nv = xc_val[p]; }
            }
            apply(r, v, w);
            for (int p = s + 64 + lane; p < e; p += 64) apply(xc_row[p], xc_val[p], w);
        }
        __syncthreads();
    }

    if (filter_interacted) {                                              // the users stored in column `item` of X
        if (tid < 2) {
            long long lo = xc_ptr[item], hi = xc_ptr[item + 1];
            clamp_span(lo, hi, xc_nnz);
            misc[tid] = static_cast<int>(lower_bound_row(xc_row, lo, hi, tile_lo + static_cast<long long>(tid) * kAudTile));
        }
        __syncthreads();
        for (int p = misc[0] + tid; p < misc[1]; p += kAudThreads) {
            const long long d = static_cast<long long>(xc_row[p]) - tile_lo;
            if (d >= 0 && d < kAudTile) acc[d] = kNoSupport;
        }
        __syncthreads();
    }
    int mine = 0, numbers = 0;                                            // eligible users; those of them whose score is no NaN
    for (int i = tid; i < kAudTile; i += kAudThreads) {
        const uint32_t a = acc[i];
        if (a == kNoSupport) continue;
        const long long u = tile_lo + i;                                  // < n_users: only such rows were accumulated
        if (user_mask && !((static_cast<uint32_t>(user_mask[u >> 5]) >> (u & 31)) & 1u)) { acc[i] = kNoSupport; continue; }
        ++mine;
        if ((a & 0x7fffffffu) > 0x7f800000u) acc[i] = kNoSupport; else ++numbers;     // a NaN score: counted, never a key
    }
    for (int d = 32; d >= 1; d >>= 1) { mine += __shfl_xor(mine, d, 64); numbers += __shfl_xor(numbers, d, 64); }
    if (lane == 0 && mine) { atomicAdd(&misc[2], mine); atomicAdd(&misc[3], numbers); }
    __syncthreads();
    const int eligible = misc[2];

    auto key = [&](int i) -> unsigned long long {                         // bit 45: a candidate; 32 score bits; 13 row bits
        const uint32_t a = acc[i];
        if (a == kNoSupport) return 0ull;
        return (1ull << 45) | (static_cast<unsigned long long>(score_key(a)) << 13) | static_cast<unsigned long long>(kAudTile - 1 - i);
    };
    const int cnt = select_sorted<48>(key, kAudTile, misc[3], top_n, win, sh);
    for (int k = tid; k < cnt; k += kAudThreads) {
        const unsigned long long kk = win[k];
        const uint32_t u = static_cast<uint32_t>(tile_lo) + static_cast<uint32_t>(kAudTile - 1 - static_cast<int>(kk & (kAudTile - 1)));
        ws_keys[slot * top_n + k] = (((kk >> 13) & 0xffffffffull) << 32) | static_cast<unsigned long long>(~u);
    }
    if (tid == 0) { ws_cnt[2 * slot] = cnt; ws_cnt[2 * slot + 1] = eligible; }
}

__global__ __launch_bounds__(kAudThreads) void audience_merge_kernel(
        int n_tiles, int top_n, const unsigned long long *__restrict__ ws_keys, const int32_t *__restrict__ ws_cnt,
        int32_t *__restrict__ out_users, float *__restrict__ out_scores, int32_t *__restrict__ out_count, int32_t *__restrict__ out_eligible) {
    __shared__ unsigned long long win[kAudMaxTop];
    __shared__ SelectShared sh;
    __shared__ int total[2];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const long long q = blockIdx.x;
    const int32_t *cnt_q = ws_cnt + 2 * q * n_tiles;
    const unsigned long long *keys_q = ws_keys + q * n_tiles * top_n;
    if (tid < 2) total[tid] = 0;
    __syncthreads();
    int listed = 0, eligible = 0;
    for (int t = tid; t < n_tiles; t += kAudThreads) { listed += cnt_q[2 * t]; eligible += cnt_q[2 * t + 1]; }
    for (int d = 32; d >= 1; d >>= 1) { listed += __shfl_xor(listed, d, 64); eligible += __shfl_xor(eligible, d, 64); }
    if (lane == 0) { atomicAdd(&total[0], listed); atomicAdd(&total[1], eligible); }
    __syncthreads();
    auto key = [&](int i) -> unsigned long long {
        const int t = i / top_n, k = i - t * top_n;
        return k < cnt_q[2 * t] ? keys_q[i] : 0ull;
    };
    const int cnt = select_sorted<64>(key, n_tiles * top_n, total[0], top_n, win, sh);
    for (int k = tid; k < top_n; k += kAudThreads) {
        const unsigned long long kk = k < cnt ? win[k] : 0ull;
        out_users[q * top_n + k] = k < cnt ? static_cast<int32_t>(~static_cast<uint32_t>(kk)) : -1;
        out_scores[q * top_n + k] = k < cnt ? __uint_as_float(key_score(static_cast<uint32_t>(kk >> 32))) : -__builtin_huge_valf();
    }
    if (tid == 0) { out_count[q] = cnt; out_eligible[q] = total[1]; }
}

inline long long audience_tiles(int32_t n_users) {
    const long long t = (static_cast<long long>(n_users) + kAudTile - 1) / kAudTile;
    return t < 1 ? 1 : t;
}
inline size_t audience_query_bytes(int32_t n_users, int32_t top_n) {     // the records and the two counters of every tile
    return static_cast<size_t>(audience_tiles(n_users)) * (static_cast<size_t>(top_n) * 8 + 8);
}

}  // namespace rtrec

using namespace rtrec;

extern "C" size_t rtrec_slim_audience_workspace_bytes(int32_t n_users, int32_t n_q, int32_t top_n) {
    if (n_users < 0 || n_q < 1 || top_n < 1 || top_n > kAudMaxTop) return 0;
    const size_t one = audience_query_bytes(n_users, top_n), all = one * static_cast<size_t>(n_q);
    const size_t cap = one > kAudWorkspaceCap ? one : kAudWorkspaceCap;
    return all < cap ? all : cap;
}

extern "C" int rtrec_slim_audience_topk(int32_t n_q, const int32_t *d_items, int32_t n_users, int32_t n_items,
                                        const int32_t *d_xc_ptr, const int32_t *d_xc_row, const float *d_xc_val, int64_t xc_nnz,
                                        const int32_t *d_wc_ptr, const int32_t *d_wc_row, const float *d_wc_val, int64_t wc_nnz,
                                        int32_t top_n, int32_t filter_interacted, const int32_t *d_user_mask,
                                        int32_t *d_out_users, float *d_out_scores, int32_t *d_out_count, int32_t *d_out_eligible,
                                        void *d_workspace, size_t workspace_bytes, void *stream) {
    if (n_q < 0 || n_users < 0 || n_items < 0 || xc_nnz < 0 || wc_nnz < 0) return RTREC_ERR_INVALID_ARG;
    if (top_n < 1 || top_n > kAudMaxTop) return RTREC_ERR_UNSUPPORTED;
    if (xc_nnz > INT32_MAX || wc_nnz > INT32_MAX) return RTREC_ERR_UNSUPPORTED;
    if (n_q == 0) return RTREC_OK;
    if (!d_items || !d_out_users || !d_out_scores || !d_out_count || !d_out_eligible) return RTREC_ERR_INVALID_ARG;
    if ((n_items > 0 && (!d_xc_ptr || !d_wc_ptr)) || (xc_nnz > 0 && (!d_xc_row || !d_xc_val)) || (wc_nnz > 0 && (!d_wc_row || !d_wc_val)))
        return RTREC_ERR_INVALID_ARG;
    const long long n_tiles = audience_tiles(n_users);
    const size_t one = audience_query_bytes(n_users, top_n);
    if (!d_workspace || workspace_bytes < one) return RTREC_ERR_WORKSPACE;
    long long per_pass = static_cast<long long>(workspace_bytes / one);   // query items per pass over the workspace
    const long long max_groups = static_cast<long long>(UINT32_MAX / kAudThreads);      // a launch holds fewer than 2^32 threads
    if (per_pass > max_groups / n_tiles) per_pass = max_groups / n_tiles;
    if (per_pass < 1) return RTREC_ERR_UNSUPPORTED;
    if (per_pass > n_q) per_pass = n_q;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (long long q0 = 0; q0 < n_q; q0 += per_pass) {
        const int n = static_cast<int>(n_q - q0 < per_pass ? n_q - q0 : per_pass);
        unsigned long long *keys = static_cast<unsigned long long *>(d_workspace);
        int32_t *cnt = reinterpret_cast<int32_t *>(keys + static_cast<size_t>(n) * n_tiles * top_n);
        hipLaunchKernelGGL(audience_tile_kernel, dim3(static_cast<unsigned>(n * n_tiles)), dim3(kAudThreads), 0, st, n, d_items + q0,
                           n_users, n_items, static_cast<int>(n_tiles), d_xc_ptr, d_xc_row, d_xc_val, static_cast<long long>(xc_nnz),
                           d_wc_ptr, d_wc_row, d_wc_val, static_cast<long long>(wc_nnz), top_n, filter_interacted, d_user_mask, keys, cnt);
        hipLaunchKernelGGL(audience_merge_kernel, dim3(static_cast<unsigned>(n)), dim3(kAudThreads), 0, st, static_cast<int>(n_tiles),
                           top_n, keys, cnt, d_out_users + q0 * top_n, d_out_scores + q0 * top_n, d_out_count + q0, d_out_eligible + q0);
    }
    return rtrec::launch_status();
}
