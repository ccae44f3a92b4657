// The row-wise top-K selection, once: k_topk_rows (ntf_kernels.hip, the probabilities of ntf_forward_topk / ntf_score_rows), k_knn_select (ntf_knn.hip, the sims
// of a (query, range)) and k_link_select (ntf_link.hip, the logits of one) are this function plus what each does with the sorted candidates; the last two merge them
// into a running list, merge_running below.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ntf {

constexpr int SEL_MAX = 2048;        // the largest K a row selection takes
constexpr int SEL_SAMPLE = 4096;     // values of the sorted sample; also the slots of the key array (SEL_MAX <= SEL_SAMPLE)

// one workgroup's LDS: the sample sort, then the candidates; the radix histogram; the selection's scalars; the tie scan's wave counts (a 1024-thread workgroup)
struct SelShared {
    unsigned long long keys[SEL_SAMPLE];
    unsigned hist[2048];
    unsigned wcnt[16];               // (16-byte aligned: a thread reads all of them, four to a load)
    unsigned prefix, remaining, count;
};

// f32 -> unsigned key in value order, and back
struct ProbKey {      // probabilities: non-negative, so the bit order is the value order
    static __device__ __forceinline__ unsigned key(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float value(unsigned k) { return __uint_as_float(k); }
};
struct SignedKey {    // negative values: all bits flipped; others: the sign bit set; every real value's key is >= 1
    static __device__ __forceinline__ unsigned key(float v) { const unsigned u = __float_as_uint(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
    static __device__ __forceinline__ float value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
};

// descending bitonic sort of n2 (power of two) 64-bit keys in LDS by the whole workgroup
__device__ __forceinline__ void bitonic_desc(unsigned long long* keys, int n2, int tid, int nthreads) {
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < n2 / 2; t += nthreads) {
                const int lo = (t / stride) * stride * 2 + (t % stride), hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a < b) == desc) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
}

// The K largest of row[0 .. M) by the composite (key << 32) | (0x7fffffff - id), id = id0 + column - value descending, id ascending among equal values - by the
// whole workgroup (K <= SEL_MAX; EXCL: column `ex` is left out).  Leaves them sorted in sh.keys[0 .. K) and returns n2, K rounded up to a power of two; the slots
// past the last candidate, up to n2, hold 0 (fewer than K eligible values: an empty slot).
// Values of one row cluster in a few exponent bins, so an MSB-first radix histogram serialises on LDS atomics (measured: 19 ms per 1000 rows of 233 629).  Instead:
// (1) a strided sample of SEL_SAMPLE values is sorted in LDS and its r-th largest taken as a threshold, r chosen so that ~4.5 K values of the row are expected above
// it; (2) one pass collects the values above the threshold (a few hundred appends); (3) if at least K and at most SEL_MAX were collected, the top K of the row are
// among them - every value >= the K-th largest is above the threshold - and a bitonic sort finishes.  Otherwise (ties, short rows, an unlucky sample) an exact
// 3-pass radix selection runs.  The result is the same deterministic ranking either way.
template <class Key, bool EXCL>
__device__ __forceinline__ int select_topk_row(SelShared& sh, const float* __restrict__ row, int M, int K, int64_t id0, int64_t ex) {
    unsigned long long* keys = sh.keys;
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6;
    int n2 = 1; while (n2 < K) n2 <<= 1;
    bool done = false;
    if (M >= 8 * SEL_SAMPLE && K * 8 <= SEL_MAX) {
        const int stride = M / SEL_SAMPLE;
        for (int k = tid; k < SEL_SAMPLE; k += NT) keys[k] = (unsigned long long)Key::key(row[(int64_t)k * stride]);
        __syncthreads();
        bitonic_desc(keys, SEL_SAMPLE, tid, NT);
        // expected number of row values above the r-th largest sample value: r * M / SEL_SAMPLE; aim at 4.5 K (>= K with overwhelming probability)
        int r = (int)((4.5 * K * SEL_SAMPLE) / M) + 1;
        if (r < 8) r = 8;
        const unsigned thr = (unsigned)keys[r < SEL_SAMPLE ? r : SEL_SAMPLE - 1];
        __syncthreads();
        if (tid == 0) sh.count = 0;
        __syncthreads();
        for (int c = tid; c < M; c += NT) {
            const unsigned u = Key::key(row[c]);
            if (u > thr && (!EXCL || c != ex)) { const unsigned p = atomicAdd(&sh.count, 1u); if (p < SEL_MAX) keys[p] = ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - (id0 + c)); }
        }
        __syncthreads();
        const unsigned cnt = sh.count;
        if (cnt >= (unsigned)K && cnt <= SEL_MAX) {
            int m2 = n2; while (m2 < (int)cnt) m2 <<= 1;
            for (int k = cnt + tid; k < m2; k += NT) keys[k] = 0ull;
            __syncthreads();
            bitonic_desc(keys, m2, tid, NT);
            done = true;
        }
        __syncthreads();
    }
    if (!done) {
        unsigned prefix = 0, prefix_mask = 0, remaining = K;
        // bits [31:21], [20:10], [9:0]
        const int shifts[3] = {21, 10, 0};
        const int widths[3] = {11, 11, 10};
        for (int pass = 0; pass < 3; ++pass) {
            const int sft = shifts[pass], nb = 1 << widths[pass];
            for (int b = tid; b < nb; b += NT) sh.hist[b] = 0;
            __syncthreads();
            for (int c = tid; c < M; c += NT) {
                const unsigned u = Key::key(row[c]);
                if ((u & prefix_mask) == prefix && (!EXCL || c != ex)) atomicAdd(&sh.hist[(u >> sft) & (nb - 1)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned rem = remaining; int b = nb - 1;
                for (; b > 0; --b) { if (sh.hist[b] >= rem) break; rem -= sh.hist[b]; }
                sh.prefix = prefix | ((unsigned)b << sft); sh.remaining = rem;
            }
            __syncthreads();
            prefix = sh.prefix; remaining = sh.remaining;
            prefix_mask |= (unsigned)(nb - 1) << sft;
            __syncthreads();
        }
        // prefix = the key of the K-th largest eligible value (0 when fewer than K are eligible); `remaining` = how many copies of it belong to the top K
        if (tid == 0) sh.count = 0;
        for (int k = tid; k < SEL_MAX; k += NT) keys[k] = 0ull;
        __syncthreads();
        const unsigned thr = prefix;
        for (int c = tid; c < M; c += NT) {       // fewer than K values are above the threshold
            const unsigned u = Key::key(row[c]);
            if (u > thr && (!EXCL || c != ex)) { const unsigned p = atomicAdd(&sh.count, 1u); keys[p] = ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - (id0 + c)); }
        }
        __syncthreads();
        // ties at the threshold: the `remaining` smallest ids, found by an ordered scan (ballot inside a wave, wave counts through LDS)
        unsigned base = sh.count, need = remaining;
        for (int b0 = 0; b0 < M && need > 0; b0 += NT) {
            const int c = b0 + tid;
            const bool hit = c < M && (!EXCL || c != ex) && Key::key(row[c]) == thr;
            const unsigned long long m = __ballot(hit);
            if (lane == 0) sh.wcnt[wave] = (unsigned)__popcll(m);
            __syncthreads();
            unsigned before = 0, total = 0;
            for (int w = 0; w < NT / 64; ++w) { const unsigned n = sh.wcnt[w]; if (w < wave) before += n; total += n; }
            const unsigned pos = before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (hit && pos < need) keys[base + pos] = ((unsigned long long)thr << 32) | (unsigned)(0x7fffffff - (id0 + c));
            const unsigned took = total < need ? total : need;
            base += took; need -= took;
            __syncthreads();
        }
        bitonic_desc(keys, n2, tid, NT);
    }
    return n2;
}

// A row walked range by range (k_knn_select, k_link_select): the sorted candidates select_topk_row left in sh.keys[0 .. K) (n2: its return value) are merged with
// the row's running list `mine` [K] (first: there is none yet) by the same composite - a total order, so the merge is exact and the order of the ranges free - and
// the list is written back.  2 n2 <= 4096 composites, sorted again; a composite of 0 is an empty slot.
__device__ __forceinline__ void merge_running(SelShared& sh, int n2, int K, unsigned long long* __restrict__ mine, int first) {
    unsigned long long* keys = sh.keys;
    const int tid = threadIdx.x, NT = blockDim.x;
    if (!first) {
        __syncthreads();
        for (int k = tid; k < n2; k += NT) keys[n2 + k] = k < K ? mine[k] : 0ull;
        for (int k = K + tid; k < n2; k += NT) keys[k] = 0ull;
        __syncthreads();
        bitonic_desc(keys, 2 * n2, tid, NT);
    }
    for (int k = tid; k < K; k += NT) mine[k] = keys[k];
}

}  // namespace ntf
