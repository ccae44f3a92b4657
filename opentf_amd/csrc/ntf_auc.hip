// Micro-averaged ROC AUC of the reference's eval stage on the device (reference src/evl/metric.py:36-41: sklearn's
// roc_auc_score(Y.toarray(), Y_.toarray(), average='micro')) as an exact integer statistic: the Mann-Whitney U with mid-ranks over all
// n * M (score, label) pairs, U2 = sum over positives of (2 #negatives scored lower + #negatives scored equal), AUC = U2 / (2 P N).
//
// The positives are few (nnz of the truth rows), the scores are many (n * M).  The host gathers the positives' scores, maps them to
// monotone u32 keys and reduces them to G sorted distinct keys v[0, G).  They cut the key axis into 2 G + 1 buckets: bucket 2 g holds the
// keys strictly between v[g - 1] and v[g], bucket 2 g + 1 the keys equal to v[g].  The device streams every score once and counts it
// into its bucket (k_auc_count: the only pass over the n * M scores); the host finishes in integers from the 2 G + 1 counts.  Integer
// adds commute, so the result does not depend on how the counting is scheduled.
//
// The same pass gives the micro ROC curve that `aucroc+` keeps (include/opentf_amd_roc.h): the even buckets are the gaps between the positives' keys and hold
// negatives only, so the curve runs horizontally over each and all of its corners lie at the v[g] and at the far end of every non-empty gap.  The counts are their
// coordinates; the threshold at a gap's end is the gap's smallest key, one atomic min beside the count (k_roc_count; integer mins commute as the adds do).
#include "../../include/opentf_amd.h"
#include "../../include/opentf_amd_roc.h"
#include "ntf_kernels.h"
#include "ntf_host.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace ntf {

constexpr int AUC_THREADS = 256;
constexpr int AUC_MAX_BLOCKS = 2048;      // 256 CUs x 8; the rest of a chunk is walked grid-stride
constexpr int AUC_PIVOTS = 2048;          // sampled keys held in LDS: the top 11 levels of the search never leave the CU
constexpr int AUC_LDS_BUCKETS = 4096;     // up to this many buckets a workgroup counts in LDS and adds to the global counters once

// f32 bits -> u32 key whose unsigned order is the order of the values as real numbers: -0.0 becomes +0.0, negatives have all bits flipped,
// non-negatives get the top bit.  Built from the bits alone: denormals stay distinct (an f32 add could flush them).  NaN: *nan is raised.
__host__ __device__ __forceinline__ uint32_t auc_key(uint32_t u, uint32_t& nan) {
    nan |= (uint32_t)((u & 0x7fffffffu) > 0x7f800000u);
    u = (u << 1) ? u : 0u;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

// A thread's two pending (bucket, count) pairs.  `run` is the bucket of the elements just seen; `hot` is a bucket that repeated before and is
// kept for the thread's whole walk, so that a value most of the matrix holds (the exact zeros of a saturated or top-K-like prediction) costs
// one add per thread, not one per run.  A run that ends with a count of 1 (distinct real values) never displaces `hot`.
struct AucPending { uint32_t hot_b, hot_n, run_b, run_n; };

template <bool LDS_HIST>
__device__ __forceinline__ void auc_flush(uint32_t b, uint32_t c, uint32_t* hist, unsigned long long* cnt) {
    if (!c) return;
    if (LDS_HIST) atomicAdd(&hist[b], c); else atomicAdd(&cnt[b], (unsigned long long)c);
}

template <bool LDS_HIST>
__device__ __forceinline__ void auc_add(AucPending& p, uint32_t b, uint32_t* hist, unsigned long long* cnt) {
    if (b == p.hot_b) { ++p.hot_n; return; }
    if (b == p.run_b) { ++p.run_n; return; }
    if (p.run_n > 1) {                   // the run repeated: it becomes the kept bucket, the old one is added
        auc_flush<LDS_HIST>(p.hot_b, p.hot_n, hist, cnt);
        p.hot_b = p.run_b; p.hot_n = p.run_n;
    } else {
        auc_flush<LDS_HIST>(p.run_b, p.run_n, hist, cnt);
    }
    p.run_b = b; p.run_n = 1;
}

// bucket of key k: g = #{ v[j] < k } by a branchless lower bound - first over the pivots in LDS (piv[i] = v[(i + 1) * stride - 1], S of them,
// step0 = the largest power of two <= S or 0), then `stride / 2 .. 1` over v itself (global, L2-resident; none when stride == 1)
__device__ __forceinline__ uint32_t auc_bucket(uint32_t k, const uint32_t* piv, uint32_t S, uint32_t step0, const uint32_t* __restrict__ v, uint32_t G,
                                               uint32_t stride) {
    uint32_t c = 0;
    for (uint32_t s = step0; s; s >>= 1) { const uint32_t t = c + s; c = (t <= S && piv[min(t, S) - 1] < k) ? t : c; }
    uint32_t g = c * stride;
    for (uint32_t s = stride >> 1; s; s >>= 1) { const uint32_t t = g + s; g = (t <= G && v[min(t, G) - 1] < k) ? t : g; }
    const uint32_t at = min(g, G - 1), vg = stride == 1 ? piv[at] : v[at];   // (stride == 1: the pivots are v itself)
    const uint32_t eq = (g < G && vg == k) ? 1u : 0u;
    return 2u * g + eq;
}

// x [L] f32 bits, 16-byte aligned.  cnt [2 G + 1] u64 bucket counters, *nan_flag: set when a NaN was seen.
// (k_roc_count below is this kernel with a minimum beside each gap's count - a sibling, so that this one compiles as it always did: staging, the load loop, the
// tail and the LDS fold are the same lines there, and a change to them here is made there too.)
template <bool LDS_HIST>
__global__ __launch_bounds__(AUC_THREADS) void k_auc_count(const uint32_t* __restrict__ x, int64_t L, const uint32_t* __restrict__ v, uint32_t G,
                                                           const uint32_t* __restrict__ pivots, uint32_t S, uint32_t step0, uint32_t stride,
                                                           unsigned long long* __restrict__ cnt, uint32_t* __restrict__ nan_flag) {
    __shared__ uint32_t piv[AUC_PIVOTS];
    __shared__ uint32_t hist[LDS_HIST ? AUC_LDS_BUCKETS : 1];
    const uint32_t nb = 2u * G + 1u;
    for (uint32_t i = threadIdx.x; i < S; i += AUC_THREADS) piv[i] = pivots[i];
    if (LDS_HIST) for (uint32_t i = threadIdx.x; i < nb; i += AUC_THREADS) hist[i] = 0u;
    __syncthreads();

    AucPending p = {0xffffffffu, 0u, 0xffffffffu, 0u};
    uint32_t nan = 0u;
    const int64_t nvec = L >> 2, nthreads = (int64_t)gridDim.x * AUC_THREADS;
    const uint4* __restrict__ x4 = reinterpret_cast<const uint4*>(x);
    // two 16-byte loads in flight per thread and round
    for (int64_t i = (int64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < nvec; i += 2 * nthreads) {
        const int64_t j = i + nthreads;
        const uint4 a = x4[i];
        const bool two = j < nvec;
        const uint4 b = two ? x4[j] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q < 4 || two) auc_add<LDS_HIST>(p, auc_bucket(auc_key(e[q], nan), piv, S, step0, v, G, stride), hist, cnt);
        }
    }
    // the 0..3 scores behind the last whole vector
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)(L & 3))
        auc_add<LDS_HIST>(p, auc_bucket(auc_key(x[(nvec << 2) + threadIdx.x], nan), piv, S, step0, v, G, stride), hist, cnt);
    auc_flush<LDS_HIST>(p.hot_b, p.hot_n, hist, cnt);
    auc_flush<LDS_HIST>(p.run_b, p.run_n, hist, cnt);
    if (nan) atomicOr(nan_flag, 1u);
    if (LDS_HIST) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb; i += AUC_THREADS) if (hist[i]) atomicAdd(&cnt[i], (unsigned long long)hist[i]);
    }
}

// ---- the curve's arm of the count pass (include/opentf_amd_roc.h): beside the count of every even bucket 2 g (gap g: negatives only) the smallest key seen in it,
// which is the threshold at the far end of the curve's horizontal run over that gap.  gmin [G + 1] u32 starts at 0xffffffff (no score has that key: it would be a
// NaN's).  Odd buckets hold one key, v[g], and need no minimum.  Same stream, same loads and the same pending pairs as k_auc_count, each pair with its running
// minimum: a matrix of exact zeros still costs one add and one min per thread.
struct RocPending { uint32_t hot_b, hot_n, hot_m, run_b, run_n, run_m; };

template <bool LDS_HIST>
__device__ __forceinline__ void roc_flush(uint32_t b, uint32_t c, uint32_t m, uint32_t* hist, uint32_t* lmin, unsigned long long* cnt, uint32_t* gmin) {
    if (!c) return;
    if (LDS_HIST) atomicAdd(&hist[b], c); else atomicAdd(&cnt[b], (unsigned long long)c);
    if (!(b & 1u)) { if (LDS_HIST) atomicMin(&lmin[b >> 1], m); else atomicMin(&gmin[b >> 1], m); }
}

template <bool LDS_HIST>
__device__ __forceinline__ void roc_add(RocPending& p, uint32_t b, uint32_t k, uint32_t* hist, uint32_t* lmin, unsigned long long* cnt, uint32_t* gmin) {
    if (b == p.hot_b) { ++p.hot_n; p.hot_m = min(p.hot_m, k); return; }
    if (b == p.run_b) { ++p.run_n; p.run_m = min(p.run_m, k); return; }
    if (p.run_n > 1) {                   // as auc_add: the run repeated and becomes the kept bucket
        roc_flush<LDS_HIST>(p.hot_b, p.hot_n, p.hot_m, hist, lmin, cnt, gmin);
        p.hot_b = p.run_b; p.hot_n = p.run_n; p.hot_m = p.run_m;
    } else {
        roc_flush<LDS_HIST>(p.run_b, p.run_n, p.run_m, hist, lmin, cnt, gmin);
    }
    p.run_b = b; p.run_n = 1; p.run_m = k;
}

// k_auc_count plus gmin [G + 1]: keep the staging, the load loop, the tail and the LDS fold line for line what they are there (a fix to one is a fix to both).
//  LDS arm: 2 G + 1 <= AUC_LDS_BUCKETS, so the G + 1 minima fit AUC_LDS_BUCKETS / 2 words (8 KiB beside hist's 16 and piv's 8).
template <bool LDS_HIST>
__global__ __launch_bounds__(AUC_THREADS) void k_roc_count(const uint32_t* __restrict__ x, int64_t L, const uint32_t* __restrict__ v, uint32_t G,
                                                           const uint32_t* __restrict__ pivots, uint32_t S, uint32_t step0, uint32_t stride,
                                                           unsigned long long* __restrict__ cnt, uint32_t* __restrict__ gmin, uint32_t* __restrict__ nan_flag) {
    __shared__ uint32_t piv[AUC_PIVOTS];
    __shared__ uint32_t hist[LDS_HIST ? AUC_LDS_BUCKETS : 1];
    __shared__ uint32_t lmin[LDS_HIST ? AUC_LDS_BUCKETS / 2 : 1];
    const uint32_t nb = 2u * G + 1u;
    for (uint32_t i = threadIdx.x; i < S; i += AUC_THREADS) piv[i] = pivots[i];
    if (LDS_HIST) {
        for (uint32_t i = threadIdx.x; i < nb; i += AUC_THREADS) hist[i] = 0u;
        for (uint32_t i = threadIdx.x; i <= G; i += AUC_THREADS) lmin[i] = 0xffffffffu;
    }
    __syncthreads();

    RocPending p = {0xffffffffu, 0u, 0xffffffffu, 0xffffffffu, 0u, 0xffffffffu};
    uint32_t nan = 0u;
    const int64_t nvec = L >> 2, nthreads = (int64_t)gridDim.x * AUC_THREADS;
    const uint4* __restrict__ x4 = reinterpret_cast<const uint4*>(x);
    // two 16-byte loads in flight per thread and round
    for (int64_t i = (int64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < nvec; i += 2 * nthreads) {
        const int64_t j = i + nthreads;
        const uint4 a = x4[i];
        const bool two = j < nvec;
        const uint4 b = two ? x4[j] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q < 4 || two) {
                const uint32_t k = auc_key(e[q], nan);
                roc_add<LDS_HIST>(p, auc_bucket(k, piv, S, step0, v, G, stride), k, hist, lmin, cnt, gmin);
            }
        }
    }
    // the 0..3 scores behind the last whole vector
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)(L & 3)) {
        const uint32_t k = auc_key(x[(nvec << 2) + threadIdx.x], nan);
        roc_add<LDS_HIST>(p, auc_bucket(k, piv, S, step0, v, G, stride), k, hist, lmin, cnt, gmin);
    }
    roc_flush<LDS_HIST>(p.hot_b, p.hot_n, p.hot_m, hist, lmin, cnt, gmin);
    roc_flush<LDS_HIST>(p.run_b, p.run_n, p.run_m, hist, lmin, cnt, gmin);
    if (nan) atomicOr(nan_flag, 1u);
    if (LDS_HIST) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb; i += AUC_THREADS) if (hist[i]) atomicAdd(&cnt[i], (unsigned long long)hist[i]);
        for (uint32_t i = threadIdx.x; i <= G; i += AUC_THREADS) if (lmin[i] != 0xffffffffu) atomicMin(&gmin[i], lmin[i]);
    }
}


// The positives' keys of a batch of rows, one wave per row: the lanes walk the row's truth columns (CSR row rows[i], global expert ids), key j of row i goes to
// keys[slot[i] + j] (slot: the host's prefix sum over the truth rows' lengths).  Plain vector loads and stores; a NaN raises *nan_flag as auc_key does.
// Dense form: the score of column c is P[i, c] of the row-major [B, M] probabilities.
__global__ __launch_bounds__(64) void k_score_pos_keys_dense(const uint32_t* __restrict__ P, int M, const int64_t* __restrict__ rows, const int64_t* __restrict__ t_indptr,
                                                             const int32_t* __restrict__ t_indices, const int64_t* __restrict__ slot, uint32_t* __restrict__ keys,
                                                             uint32_t* __restrict__ nan_flag) {
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t trow = rows[i], tb = t_indptr[trow];
    const int R = (int)(t_indptr[trow + 1] - tb);
    uint32_t nan = 0u;
    for (int j = lane; j < R; j += 64) keys[slot[i] + j] = auc_key(P[i * M + t_indices[tb + j]], nan);
    if (nan) atomicOr(nan_flag, 1u);
}

// Top-K form: the score of column c is the stored value whose id is c, 0.0 when c is not among the row's K stored ids.  Per 64 truth columns (one per lane) the wave
// scans the stored ids in 64-wide windows (one id per lane): truth column t of the chunk is broadcast, a ballot finds the lane holding it.
__global__ __launch_bounds__(64) void k_score_pos_keys_topk(const uint32_t* __restrict__ vals, const int32_t* __restrict__ idx, int K, const int64_t* __restrict__ rows,
                                                            const int64_t* __restrict__ t_indptr, const int32_t* __restrict__ t_indices,
                                                            const int64_t* __restrict__ slot, uint32_t* __restrict__ keys, uint32_t* __restrict__ nan_flag) {
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t trow = rows[i], tb = t_indptr[trow];
    const int R = (int)(t_indptr[trow + 1] - tb);
    uint32_t nan = 0u;
    for (int jb = 0; jb < R; jb += 64) {
        const int nt = min(64, R - jb);                                  // truth columns of this chunk (wave-uniform)
        const int c_mine = lane < nt ? t_indices[tb + jb + lane] : -1;
        int found = -1;                                                  // position of this lane's truth column among the stored ids
        for (int base = 0; base < K; base += 64) {
            const int id = base + lane < K ? idx[i * K + base + lane] : -2;
            for (int t = 0; t < nt; ++t) {
                const int c = __shfl(c_mine, t, 64);
                const unsigned long long hit = __ballot(id == c);
                if (hit && lane == t) found = base + (int)__ffsll((long long)hit) - 1;
            }
        }
        if (lane < nt) keys[slot[i] + jb + lane] = auc_key(found >= 0 ? vals[i * K + found] : 0u, nan);
    }
    if (nan) atomicOr(nan_flag, 1u);
}

void launch_score_pos_keys_dense(hipStream_t st, const float* P, int B, int M, const int64_t* rows, const int64_t* t_indptr, const int32_t* t_indices,
                                 const int64_t* slot, uint32_t* keys, uint32_t* nan_flag) {
    hipLaunchKernelGGL(k_score_pos_keys_dense, dim3((unsigned)B), dim3(64), 0, st, (const uint32_t*)P, M, rows, t_indptr, t_indices, slot, keys, nan_flag);
}
void launch_score_pos_keys_topk(hipStream_t st, const float* vals, const int32_t* idx, int64_t n, int K, const int64_t* rows, const int64_t* t_indptr,
                                const int32_t* t_indices, const int64_t* slot, uint32_t* keys, uint32_t* nan_flag) {
    hipLaunchKernelGGL(k_score_pos_keys_topk, dim3((unsigned)n), dim3(64), 0, st, (const uint32_t*)vals, idx, K, rows, t_indptr, t_indices, slot, keys, nan_flag);
}

// ---- the key table, the count launch and the integer finish, shared by the two host-fed entries below (auc_run) and ntf_score_rows (device-resident scores)
struct AucState {
    std::vector<uint32_t> v;            // sorted distinct keys of the positives
    std::vector<uint64_t> pos_eq;       // positives per distinct key
    uint64_t P = 0, N = 0;
    unsigned __int128 total = 0;
    uint32_t S = 0, step0 = 0, stride = 1;
    bool lds_hist = false;
    bool minima = false;                // the curve's arm: k_roc_count, with dmin beside dcnt
    DevBuf dv, dpiv, dflag, dcnt;       // u32 keys, u32 pivots, one u32 flag, 2 G + 1 u64 counters
    DevBuf dmin;                        // minima only: G + 1 u32 gap minima, 0xffffffff = none yet
};

void auc_free(AucState* s) { delete s; }

int auc_check(uint64_t P, int64_t n, int64_t M, uint64_t* N_out) {
    const unsigned __int128 total = (unsigned __int128)n * M;
    if (P == 0 || (unsigned __int128)P >= total) return NTF_EINVAL;                       // one class only
    const unsigned __int128 N128 = total - P;
    if (N128 >> 64 || ((unsigned __int128)2 * P * N128) >> 64) return NTF_EINVAL;
    if (N_out) *N_out = (uint64_t)N128;
    return NTF_OK;
}

int auc_open(hipStream_t st, const uint32_t* pos_keys, size_t n_pos, int64_t n, int64_t M, AucState** out, bool minima) {
    uint64_t N = 0;
    if (int r = auc_check(n_pos, n, M, &N)) return r;
    AucState* s = new AucState;
    s->P = n_pos; s->N = N; s->total = (unsigned __int128)n * M;
    std::vector<uint32_t>& v = s->v;
    v.assign(pos_keys, pos_keys + n_pos);
    std::sort(v.begin(), v.end());
    size_t G = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        if (G && v[G - 1] == v[i]) { ++s->pos_eq[G - 1]; continue; }
        v[G++] = v[i]; s->pos_eq.push_back(1);
    }
    v.resize(G);
    while (G / s->stride > (size_t)AUC_PIVOTS) s->stride <<= 1;
    s->S = (uint32_t)(G / s->stride);
    std::vector<uint32_t> piv(s->S);
    for (uint32_t i = 0; i < s->S; ++i) piv[i] = v[(size_t)(i + 1) * s->stride - 1];
    if (s->S) for (s->step0 = 1; s->step0 * 2 <= s->S; s->step0 <<= 1) {}
    const size_t nb = 2 * G + 1;
    s->lds_hist = nb <= (size_t)AUC_LDS_BUCKETS;
    if (!s->dv.put(v.data(), G * 4) || !s->dpiv.put(piv.data(), (size_t)s->S * 4) || !s->dcnt.alloc(nb * 8) || !s->dflag.alloc(16)) { auc_free(s); return NTF_ENOMEM; }
    if (hipMemsetAsync(s->dcnt.p, 0, nb * 8, st) != hipSuccess || hipMemsetAsync(s->dflag.p, 0, 4, st) != hipSuccess) { auc_free(s); return NTF_EHIP; }
    if (minima) {
        s->minima = true;
        if (!s->dmin.alloc((G + 1) * 4)) { auc_free(s); return NTF_ENOMEM; }
        if (hipMemsetAsync(s->dmin.p, 0xff, (G + 1) * 4, st) != hipSuccess) { auc_free(s); return NTF_EHIP; }
    }
    *out = s;
    return NTF_OK;
}

// queues one k_auc_count pass (k_roc_count when the state was opened with minima) over x [L] (device, 16-byte aligned) on `st`
int auc_count(AucState* s, hipStream_t st, const float* x, int64_t L) {
    if (L <= 0) return NTF_OK;
    // (a workgroup's LDS counters are 32-bit: it sees at most L / blocks + 1024 scores of a chunk, far below 2^32 for any chunk that fits in HBM)
    const int64_t want = ((L >> 2) + 2 * AUC_THREADS - 1) / (2 * AUC_THREADS);
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(want, 1), AUC_MAX_BLOCKS);
    const uint32_t G = (uint32_t)s->v.size();
    if (s->minima && s->lds_hist)
        hipLaunchKernelGGL(k_roc_count<true>, dim3(blocks), dim3(AUC_THREADS), 0, st, (const uint32_t*)x, L, s->dv.as<const uint32_t>(), G, s->dpiv.as<const uint32_t>(),
                           s->S, s->step0, s->stride, s->dcnt.as<unsigned long long>(), s->dmin.as<uint32_t>(), s->dflag.as<uint32_t>());
    else if (s->minima)
        hipLaunchKernelGGL(k_roc_count<false>, dim3(blocks), dim3(AUC_THREADS), 0, st, (const uint32_t*)x, L, s->dv.as<const uint32_t>(), G, s->dpiv.as<const uint32_t>(),
                           s->S, s->step0, s->stride, s->dcnt.as<unsigned long long>(), s->dmin.as<uint32_t>(), s->dflag.as<uint32_t>());
    else if (s->lds_hist)
        hipLaunchKernelGGL(k_auc_count<true>, dim3(blocks), dim3(AUC_THREADS), 0, st, (const uint32_t*)x, L, s->dv.as<const uint32_t>(), G,
                           s->dpiv.as<const uint32_t>(), s->S, s->step0, s->stride, s->dcnt.as<unsigned long long>(), s->dflag.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_auc_count<false>, dim3(blocks), dim3(AUC_THREADS), 0, st, (const uint32_t*)x, L, s->dv.as<const uint32_t>(), G,
                           s->dpiv.as<const uint32_t>(), s->S, s->step0, s->stride, s->dcnt.as<unsigned long long>(), s->dflag.as<uint32_t>());
    return hipGetLastError() == hipSuccess ? NTF_OK : NTF_EHIP;
}

namespace {
// waits for `st`, downloads the counters (and the gap minima when gmin is given) and folds the implicit zeros in: into the count of v[g] when a positive scores
// exactly 0, else into the count and the minimum of the gap the zero key falls in
int auc_counts(AucState* s, hipStream_t st, uint64_t implicit_zeros, std::vector<uint64_t>& cnt, std::vector<uint32_t>* gmin) {
    const std::vector<uint32_t>& v = s->v;
    const size_t G = v.size(), nb = 2 * G + 1;
    cnt.resize(nb);
    uint32_t flag = 0;
    if (hipStreamSynchronize(st) != hipSuccess) return NTF_EHIP;
    if (hipMemcpy(cnt.data(), s->dcnt.p, nb * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&flag, s->dflag.p, 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (gmin) {
        gmin->resize(G + 1);
        if (!s->minima || hipMemcpy(gmin->data(), s->dmin.p, (G + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    }
    if (flag) return NTF_EINVAL;                                                           // a NaN score
    if (implicit_zeros) {
        uint32_t nan = 0;
        const uint32_t kz = auc_key(0u, nan);
        const size_t g = std::lower_bound(v.begin(), v.end(), kz) - v.begin();
        const bool eq = g < G && v[g] == kz;
        cnt[2 * g + (eq ? 1 : 0)] += implicit_zeros;
        if (gmin && !eq) (*gmin)[g] = std::min((*gmin)[g], kz);
    }
    return NTF_OK;
}

// the integer finish from the folded counters
int auc_reduce(const AucState* s, const std::vector<uint64_t>& cnt, uint64_t out_counts[3], double* out_auc) {
    const std::vector<uint32_t>& v = s->v;
    const size_t G = v.size();
    // cnt[2 g] = all scores strictly between v[g - 1] and v[g], cnt[2 g + 1] = all scores equal to v[g], the positives among them included
    unsigned __int128 u2 = 0, below = 0, seen = 0;
    for (size_t g = 0; g < G; ++g) {
        if (cnt[2 * g + 1] < s->pos_eq[g]) return NTF_EHIP;                                // (cannot happen: every positive is one of the scores)
        const uint64_t neg_eq = cnt[2 * g + 1] - s->pos_eq[g];
        below += cnt[2 * g];
        u2 += (unsigned __int128)s->pos_eq[g] * (2 * below + neg_eq);
        below += neg_eq;
        seen += (unsigned __int128)cnt[2 * g] + cnt[2 * g + 1];
    }
    seen += cnt[2 * G];
    if (seen != s->total || u2 >> 64) return NTF_EHIP;                                     // (every score was counted exactly once)
    out_counts[0] = s->P; out_counts[1] = s->N; out_counts[2] = (uint64_t)u2;
    *out_auc = (double)(uint64_t)u2 / (2.0 * (double)s->P * (double)s->N);
    return NTF_OK;
}

// inverse of auc_key; the key of either zero comes back as +0.0f
float roc_value(uint32_t k) {
    const uint32_t u = (k >> 31) ? (k & 0x7fffffffu) : ~k;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
}  // namespace

// waits for the passes queued on `st`, then finishes in integers.  NTF_EINVAL: a NaN score.  NTF_EHIP: a positive that is not among the counted scores, or
// scores counted that are not exactly n * M - for scores the caller produced twice (ntf_score_rows, dense), a second production that was not bit-identical.
int auc_finish(AucState* s, hipStream_t st, uint64_t implicit_zeros, uint64_t out_counts[3], double* out_auc) {
    std::vector<uint64_t> cnt;
    if (int r = auc_counts(s, st, implicit_zeros, cnt, nullptr)) return r;
    return auc_reduce(s, cnt, out_counts, out_auc);
}

// auc_finish of a state opened with minima, plus the curve of include/opentf_amd_roc.h: fps / tps / thr [cap] receive *n_points <= 2 G + 2 points.  Nothing is
// written unless everything checks.  NTF_EHIP beyond auc_finish's: a non-empty gap whose minimum is not strictly inside it, an empty gap with a minimum, or a curve
// whose doubled trapezoid is not U2.  NTF_EINVAL: cap < 2 G + 2.
int roc_finish(AucState* s, hipStream_t st, uint64_t implicit_zeros, int64_t cap, uint64_t* fps, uint64_t* tps, float* thr, int64_t* n_points,
               uint64_t out_counts[3], double* out_auc) {
    const std::vector<uint32_t>& v = s->v;
    const size_t G = v.size();
    if (cap < 0 || (uint64_t)cap < 2 * (uint64_t)G + 2) return NTF_EINVAL;
    std::vector<uint64_t> cnt;
    std::vector<uint32_t> m;
    if (int r = auc_counts(s, st, implicit_zeros, cnt, &m)) return r;
    uint64_t counts[3];
    double auc = 0.0;
    if (int r = auc_reduce(s, cnt, counts, &auc)) return r;
    for (size_t g = 0; g <= G; ++g) {
        if (!cnt[2 * g]) { if (m[g] != 0xffffffffu) return NTF_EHIP; continue; }
        if (m[g] == 0xffffffffu || (g > 0 && m[g] <= v[g - 1]) || (g < G && m[g] >= v[g])) return NTF_EHIP;
    }
    std::vector<uint64_t> f{0}, t{0};
    std::vector<float> th{roc_value(0xff800000u)};                                         // +inf
    uint64_t fp = 0, tp = 0;
    for (size_t g = G + 1; g-- > 0;) {
        if (cnt[2 * g]) { fp += cnt[2 * g]; f.push_back(fp); t.push_back(tp); th.push_back(roc_value(m[g])); }
        if (g >= 1) {
            fp += cnt[2 * g - 1] - s->pos_eq[g - 1]; tp += s->pos_eq[g - 1];
            f.push_back(fp); t.push_back(tp); th.push_back(roc_value(v[g - 1]));
        }
    }
    unsigned __int128 trap = 0;
    for (size_t a = 0; a + 1 < f.size(); ++a) trap += (unsigned __int128)(f[a + 1] - f[a]) * (t[a + 1] + t[a]);
    if (fp != s->N || tp != s->P || trap != (unsigned __int128)counts[2]) return NTF_EHIP;
    std::copy(f.begin(), f.end(), fps); std::copy(t.begin(), t.end(), tps); std::copy(th.begin(), th.end(), thr);
    *n_points = (int64_t)f.size();
    std::memcpy(out_counts, counts, sizeof counts);
    *out_auc = auc;
    return NTF_OK;
}

}  // namespace ntf

using namespace ntf;

namespace {
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// the truth side of both entries: validates it and lists the positives as (instance, column)
struct Truth {
    std::vector<int64_t> inst;
    std::vector<int32_t> col;
};
bool read_truth(int64_t n, int64_t M, const int64_t* t_indptr, const int32_t* t_indices, int64_t n_truth_rows, const int64_t* rows, Truth& t) {
    if (!t_indptr || n_truth_rows < 1 || (!rows && n > n_truth_rows)) return false;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = rows ? rows[i] : i;
        if (r < 0 || r >= n_truth_rows) return false;
        const int64_t b = t_indptr[r], e = t_indptr[r + 1];
        if (b < 0 || e < b || (e > b && !t_indices)) return false;
        for (int64_t j = b; j < e; ++j) {
            const int32_t c = t_indices[j];
            if (c < 0 || c >= M || (j > b && c <= t_indices[j - 1])) return false;
            t.inst.push_back(i); t.col.push_back(c);
        }
    }
    return true;
}

// the curve a ntf_roc_micro_* call asked for (null for the AUC entries)
struct RocOut {
    int64_t cap;
    uint64_t *fps, *tps;
    float* thr;
    int64_t* n_points;
    bool null_output() const { return !fps || !tps || !thr || !n_points; }
};

// Everything behind the positives' scores: the key table, the stream over `n_chunks` uploads, the integer finish (auc_open / auc_count / auc_close below).
// next_chunk(k, dev, &count) uploads chunk k into `dev` and reports its number of scores.  implicit_zeros: scores of 0.0 that are not in any chunk.
template <class Upload>
int auc_run(int device, const std::vector<uint32_t>& pos_keys, int64_t n, int64_t M, uint64_t implicit_zeros, size_t stage_bytes, int64_t n_chunks,
            Upload next_chunk, const RocOut* roc, uint64_t out_counts[3], double* out_auc) {
    if (int r0 = auc_check(pos_keys.size(), n, M, nullptr)) return r0;
    if (roc && (roc->cap < 0 || (uint64_t)roc->cap < 2 * (uint64_t)pos_keys.size() + 2)) return NTF_EINVAL;      // (2 P + 2 covers the 2 G + 2 points)
    if (hipSetDevice(device) != hipSuccess) return NTF_EHIP;
    AucState* s = nullptr;
    int r = auc_open(nullptr, pos_keys.data(), pos_keys.size(), n, M, &s, roc != nullptr);
    if (r) return r;
    struct Guard { AucState* s; ~Guard() { auc_free(s); } } guard{s};
    DevBuf dx;
    if (!dx.alloc((stage_bytes + 15) & ~(size_t)15)) return NTF_ENOMEM;
    double upload_ms = 0.0, kernel_ms = 0.0;                                               // NTF_AUC_TIMING=1: reported on stderr (profiles/auc_time.py)
    int64_t streamed = 0;
    for (int64_t k = 0; k < n_chunks; ++k) {
        int64_t L = 0;
        auto t0 = std::chrono::steady_clock::now();
        if (!next_chunk(k, dx.p, &L)) return NTF_EHIP;
        upload_ms += ms_since(t0);
        if (L <= 0) continue;
        streamed += L;
        t0 = std::chrono::steady_clock::now();
        if ((r = auc_count(s, nullptr, (const float*)dx.p, L))) return r;
        if (hipStreamSynchronize(nullptr) != hipSuccess) return NTF_EHIP;                  // the next upload reuses the staging buffer
        kernel_ms += ms_since(t0);
    }
    if (const char* t = std::getenv("NTF_AUC_TIMING"); t && t[0] == '1')
        std::fprintf(stderr, "%s: %lld scores in %lld chunk(s), G = %zu (%s counters): upload %.3f ms, kernel %.3f ms (launch + wait; %.1f GB/s of scores)\n",
                     roc ? "ntf_roc" : "ntf_auc", (long long)streamed, (long long)n_chunks, s->v.size(), s->lds_hist ? "LDS" : "global", upload_ms, kernel_ms, kernel_ms > 0 ? streamed * 4e-6 / kernel_ms : 0.0);
    if (roc) return roc_finish(s, nullptr, implicit_zeros, roc->cap, roc->fps, roc->tps, roc->thr, roc->n_points, out_counts, out_auc);
    return auc_finish(s, nullptr, implicit_zeros, out_counts, out_auc);
}

// the dense entries: the AUC alone (roc null) or with the curve
int micro_dense(int device, const float* scores, int64_t n, int64_t M, int64_t ld, const int64_t* truth_indptr, const int32_t* truth_indices, int64_t n_truth_rows,
                const int64_t* rows, int64_t chunk_bytes, const RocOut* roc, uint64_t out_counts[3], double* out_auc) {
    if (!scores || n < 1 || M < 1 || ld < M || chunk_bytes < 0 || !out_counts || !out_auc || (roc && roc->null_output())) return NTF_EINVAL;
    if (chunk_bytes == 0) chunk_bytes = NTF_AUC_CHUNK_BYTES;
    const int64_t rows_per_chunk = std::min<int64_t>(chunk_bytes / 4 / M, n);
    if (rows_per_chunk < 1) return NTF_EINVAL;
    Truth t;
    if (!read_truth(n, M, truth_indptr, truth_indices, n_truth_rows, rows, t)) return NTF_EINVAL;
    std::vector<uint32_t> keys(t.col.size());
    uint32_t nan = 0;
    for (size_t j = 0; j < keys.size(); ++j) {
        uint32_t u;
        std::memcpy(&u, scores + t.inst[j] * ld + t.col[j], 4);
        keys[j] = auc_key(u, nan);
    }
    if (nan) return NTF_EINVAL;
    const int64_t n_chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
    auto upload = [&](int64_t k, void* dev, int64_t* L) {
        const int64_t r0 = k * rows_per_chunk, nr = std::min(rows_per_chunk, n - r0);
        *L = nr * M;
        if (ld == M) return hipMemcpy(dev, scores + r0 * ld, (size_t)nr * M * 4, hipMemcpyHostToDevice) == hipSuccess;
        // rows land back to back on the device: the padding behind a row is never read, and every chunk starts 16-byte aligned
        return hipMemcpy2D(dev, (size_t)M * 4, scores + r0 * ld, (size_t)ld * 4, (size_t)M * 4, (size_t)nr, hipMemcpyHostToDevice) == hipSuccess;
    };
    return auc_run(device, keys, n, M, 0, (size_t)rows_per_chunk * M * 4, n_chunks, upload, roc, out_counts, out_auc);
}

// the CSR entries, likewise
int micro_csr(int device, const int64_t* s_indptr, const int32_t* s_indices, const float* s_values, int64_t n, int64_t M, const int64_t* truth_indptr,
              const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows, int64_t chunk_bytes, const RocOut* roc, uint64_t out_counts[3], double* out_auc) {
    if (!s_indptr || n < 1 || M < 1 || chunk_bytes < 0 || !out_counts || !out_auc || (roc && roc->null_output())) return NTF_EINVAL;
    if (chunk_bytes == 0) chunk_bytes = NTF_AUC_CHUNK_BYTES;
    if (chunk_bytes < 4) return NTF_EINVAL;
    const int64_t e0 = s_indptr[0], e1 = s_indptr[n], nnz = e1 - e0;
    if (e0 < 0 || nnz < 0 || (nnz > 0 && (!s_indices || !s_values))) return NTF_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t b = s_indptr[i], e = s_indptr[i + 1];
        if (e < b || e > e1) return NTF_EINVAL;
        for (int64_t j = b; j < e; ++j)
            if (s_indices[j] < 0 || s_indices[j] >= M || (j > b && s_indices[j] <= s_indices[j - 1])) return NTF_EINVAL;
    }
    Truth t;
    if (!read_truth(n, M, truth_indptr, truth_indices, n_truth_rows, rows, t)) return NTF_EINVAL;
    std::vector<uint32_t> keys(t.col.size());
    uint32_t nan = 0;
    for (size_t j = 0; j < keys.size(); ++j) {
        const int32_t* b = s_indices + s_indptr[t.inst[j]];
        const int32_t* e = s_indices + s_indptr[t.inst[j] + 1];
        const int32_t* f = std::lower_bound(b, e, t.col[j]);
        uint32_t u = 0;                                                                   // not stored: 0.0
        if (f != e && *f == t.col[j]) std::memcpy(&u, s_values + (f - s_indices), 4);
        keys[j] = auc_key(u, nan);
    }
    if (nan) return NTF_EINVAL;
    const int64_t per_chunk = std::max<int64_t>(std::min<int64_t>(chunk_bytes / 4, nnz), 1);
    const int64_t n_chunks = (nnz + per_chunk - 1) / per_chunk;
    auto upload = [&](int64_t k, void* dev, int64_t* L) {
        const int64_t b = k * per_chunk;
        *L = std::min(per_chunk, nnz - b);
        return hipMemcpy(dev, s_values + e0 + b, (size_t)*L * 4, hipMemcpyHostToDevice) == hipSuccess;
    };
    const unsigned __int128 total = (unsigned __int128)n * M;
    if ((total - (unsigned __int128)nnz) >> 64) return NTF_EINVAL;
    return auc_run(device, keys, n, M, (uint64_t)(total - (unsigned __int128)nnz), (size_t)per_chunk * 4, n_chunks, upload, roc, out_counts, out_auc);
}
}  // namespace

extern "C" int ntf_auc_micro_dense(int device, const float* scores, int64_t n, int64_t M, int64_t ld, const int64_t* truth_indptr,
                                   const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows, int64_t chunk_bytes, uint64_t out_counts[3],
                                   double* out_auc) {
    return micro_dense(device, scores, n, M, ld, truth_indptr, truth_indices, n_truth_rows, rows, chunk_bytes, nullptr, out_counts, out_auc);
}

extern "C" int ntf_auc_micro_csr(int device, const int64_t* s_indptr, const int32_t* s_indices, const float* s_values, int64_t n, int64_t M,
                                 const int64_t* truth_indptr, const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows, int64_t chunk_bytes,
                                 uint64_t out_counts[3], double* out_auc) {
    return micro_csr(device, s_indptr, s_indices, s_values, n, M, truth_indptr, truth_indices, n_truth_rows, rows, chunk_bytes, nullptr, out_counts, out_auc);
}

// ---- the curve beside the AUC (include/opentf_amd_roc.h)
extern "C" int ntf_roc_micro_dense(int device, const float* scores, int64_t n, int64_t M, int64_t ld, const int64_t* truth_indptr,
                                   const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows, int64_t chunk_bytes, int64_t cap_points,
                                   uint64_t* fps, uint64_t* tps, float* thresholds, int64_t* n_points, uint64_t out_counts[3], double* out_auc) {
    const RocOut roc{cap_points, fps, tps, thresholds, n_points};
    return micro_dense(device, scores, n, M, ld, truth_indptr, truth_indices, n_truth_rows, rows, chunk_bytes, &roc, out_counts, out_auc);
}

extern "C" int ntf_roc_micro_csr(int device, const int64_t* s_indptr, const int32_t* s_indices, const float* s_values, int64_t n, int64_t M,
                                 const int64_t* truth_indptr, const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows, int64_t chunk_bytes,
                                 int64_t cap_points, uint64_t* fps, uint64_t* tps, float* thresholds, int64_t* n_points, uint64_t out_counts[3], double* out_auc) {
    const RocOut roc{cap_points, fps, tps, thresholds, n_points};
    return micro_csr(device, s_indptr, s_indices, s_values, n, M, truth_indptr, truth_indices, n_truth_rows, rows, chunk_bytes, &roc, out_counts, out_auc);
}
