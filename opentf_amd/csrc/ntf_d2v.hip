// doc2vec team-vector producer on the MI355X: the table [n_teams, d] that D2v.get_dense_vecs hands to the Fnn / Bnn input.
// Replaces gensim.models.Doc2Vec as the reference calls it, src/mdl/emb/d2v.py:69-84 (gensim==4.3.3, requirements.txt:44, not installed here: its published
// algorithm - word2vec.py prepare_vocab / make_cum_table, doc2vec_inner.pyx fast_document_dm_neg / fast_document_dbow_neg - is restated in
// oracle/d2v_oracle.py, which also says what is pinned against the gensim objects the reference's authors committed):
//   PV-DM   (dm = 1, cbow_mean = 1)  per kept position i of a document: l1 = mean(doc vector, word vectors of the shrunk window); the word and `negative`
//           table draws: f = l1 . syn1neg[t], skipped when |f| >= 6, g = (label - sigmoid_table(f)) * alpha, work += g syn1neg[t], syn1neg[t] += g l1;
//           doc vector and window word vectors += work
//   PV-DBOW (dm = 0, dbow_words = 1) per kept position i: the same unit with every window word vector as the input (input += work), then with the doc vector
// gensim trains Hogwild on all cores (the reference's log of dblp mt10.ts2: 224 workers, 276 s per epoch of 19.07 M words, 100 epochs = 7.7 h).  Here: one
// wave per document, the doc vector in registers for the whole document (d / 64 values per lane), word / syn1neg rows as one coalesced 512-B row read and
// one coalesced f32 atomic row add each, every random draw a Philox word counted by (document, position, unit, slot) - so the result does not depend on how
// the documents are spread over waves except through the order of the atomic adds, and a one-wave launch (`serial`) reproduces the oracle's sequential pass.
#include "../../include/opentf_amd.h"
#include "ntf_device.h"
#include "ntf_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

using namespace ntf;

struct ntf_d2v {
    int device = 0; hipStream_t st = nullptr;
    int64_t n_docs = 0, n_vocab = 0, n_words = 0; int d = 0, dp = 0;   // dp: the device row stride, d rounded up to a multiple of 64 (a wave holds dp / 64 values per lane; the columns past d are zero and stay zero)
    int64_t* doc_ptr = nullptr; int32_t* words = nullptr;
    uint32_t *sample_int = nullptr, *cum_table = nullptr;
    float *dv = nullptr, *wv = nullptr, *syn1neg = nullptr;
    int64_t* order = nullptr; double* progress = nullptr;
    double* d_loss = nullptr;     // [sum of -log terms, number of terms]
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint64_t seed = 0;
    // ntf_d2v_infer: the queries of the last call (CSR, ids) and their vectors [n, dp] (initial on the way in, inferred on the way out); grown on demand
    int64_t *q_ptr = nullptr, *q_ids = nullptr; int32_t* q_words = nullptr; float* q_vec = nullptr;
    int64_t q_ptr_cap = 0, q_ids_cap = 0, q_words_cap = 0, q_vec_cap = 0;
    std::string err;
};
static thread_local std::string g_d2v_create_error;

extern "C" const char* ntf_d2v_last_error(const ntf_d2v* h) { return h ? h->err.c_str() : g_d2v_create_error.c_str(); }

namespace {
constexpr int D2V_RING = 1024;      // kept words of a document a wave holds at a time: a ring filled on demand, 64 raw words per step, just ahead of the window it is read through
constexpr int D2V_MAX_DOC = 10000;  // gensim's cap (doc2vec_inner.pyx MAX_DOCUMENT_LEN): the words of a document that survive the subsampling are collected up to this many
constexpr float D2V_MAX_EXP = 6.f;
enum { SLOT_KEEP = 0, SLOT_WINDOW = 1, SLOT_NEG0 = 2, SLOT_NEG1 = 3 };

struct D2vArgs {
    int64_t n_docs, n_vocab; int d, window, negative, serial;
    const int64_t* doc_ptr; const int32_t* words; const uint32_t *sample_int, *cum_table; const int64_t* order; const double* progress;
    float *dv, *wv, *syn1neg;
    double alpha_start, alpha_end;
    uint32_t k0, k1;
    double* loss;
};

__device__ __forceinline__ uint4 d2v_draw(uint32_t k0, uint32_t k1, int64_t doc, int pos, int unit, int slot) {
    return philox4x32(make_uint4((uint32_t)doc, (uint32_t)((uint64_t)doc >> 32), ((uint32_t)pos << 8) | (uint32_t)unit, (uint32_t)slot), make_uint2(k0, k1));
}
// EXP_TABLE lookup of doc2vec_inner.pyx (the table is built in float32: entry i = sigmoid((i / 1000 * 2 - 1) * 6))
__device__ __forceinline__ float d2v_sigmoid_table(float f) {
    const int i = (int)((f + D2V_MAX_EXP) * (1000.f / D2V_MAX_EXP / 2.f));
    const float e = expf(((float)i / 1000.f * 2.f - 1.f) * D2V_MAX_EXP);
    return e / (e + 1.f);
}
// one value of a table row.  The trainer: rows other waves add to, read past the CU's vector cache; FROZEN (inference): tables nobody writes, a plain cached load
template <bool FROZEN = false>
__device__ __forceinline__ float d2v_ld(const float* p) {
    if constexpr (FROZEN) return *p; else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the row of `table` that belongs to the word at kept position m (wave-uniform: the row address in scalar registers)
template <class T>
__device__ __forceinline__ T* d2v_row(T* table, int d, const int* kept, int m) { return table + (int64_t)__builtin_amdgcn_readfirstlane(kept[m & (D2V_RING - 1)]) * d; }
// row += v: one coalesced f32 atomic row add
template <int NV>
__device__ __forceinline__ void d2v_row_add(float* row, int lane, const float (&v)[NV]) {
#pragma unroll
    for (int q = 0; q < NV; ++q) unsafeAtomicAdd(row + lane + 64 * q, v[q]);
}

constexpr int D2V_TOP = 1024;       // cumulative table, first level: the last entry of each of <= 1024 equal buckets, in LDS (round 5: the bisection in memory was 13-16 dependent round trips a position;
                                    // now ~5: PV-DM 61.5 -> 55.2 ms a pass.  Fetching a unit's six syn1neg rows up front instead of one by one was tried with it: 95 ms - the registers cost two waves per SIMD)

// what both kernels begin with: the first table level into LDS (buckets of top_s entries; top[k] = the last entry of bucket k) and the items of this wave: first, first + stride, ..
// (one item after the other by wave 0 of block 0 when `serial`).  false: this wave has nothing to do.  Every thread of the block calls it
__device__ __forceinline__ bool d2v_prologue(const uint32_t* cum_table, int64_t n_vocab, int serial, uint32_t* s_top, int& top_s, int& top_n, int64_t& first, int64_t& stride) {
    top_s = (int)((n_vocab + D2V_TOP - 1) / D2V_TOP); top_n = (int)((n_vocab + top_s - 1) / top_s);
    for (int k = threadIdx.x; k < top_n; k += blockDim.x) s_top[k] = cum_table[min((int64_t)(k + 1) * top_s, n_vocab) - 1];
    __syncthreads();
    const int wv_id = threadIdx.x >> 6;
    first = serial ? 0 : (int64_t)blockIdx.x * 4 + wv_id;
    stride = serial ? 1 : (int64_t)gridDim.x * 4;
    return !(serial && (blockIdx.x != 0 || wv_id != 0));
}

// words that survive the frequent-word subsampling (sample_int >= draw), in order: compacted by ballot into a RING, 64 raw words per step, filled until `need` words are
// kept - just far enough ahead of position i for its window (need = i + window + 1) - so a document of any length needs 1 024 slots (round 3 held the whole kept list in
// LDS and silently cut documents at 1 024 kept words; gensim's cap is 10 000: embtype member / skillmember on gith, uspt).  words: the document's L raw words;
// K, base: kept words compacted so far (<= D2V_MAX_DOC), raw words scanned so far
__device__ __forceinline__ void d2v_fill_ring(int* kept, const int32_t* words, int L, const uint32_t* sample_int, uint32_t k0, uint32_t k1, int64_t doc, int need, int lane, int& K, int& base) {
    while (K < need && base < L && K < D2V_MAX_DOC) {
        const int p = base + lane;
        int wd = 0; bool keep = false;
        if (p < L) { wd = words[p]; keep = sample_int[wd] >= d2v_draw(k0, k1, doc, p, 0, SLOT_KEEP).x; }
        const unsigned long long m = __ballot(keep);
        const int at = K + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && at < D2V_MAX_DOC) kept[at & (D2V_RING - 1)] = wd;         // (slots older than i - window are dead: K - (i - window) <= 2 window + 64 < D2V_RING)
        K = min(K + (int)__popcll(m), D2V_MAX_DOC);
        base += 64;
        __builtin_amdgcn_wave_barrier();
    }
}

// PV-DM's input l1: the mean of the doc vector and the word vectors of the kept positions [lo, hi) without i
template <int NV, bool FROZEN>
__device__ __forceinline__ void d2v_dm_mean(const float* wv, int d, const int* kept, int lo, int hi, int i, const float (&dreg)[NV], int lane, float (&l1)[NV]) {
#pragma unroll
    for (int q = 0; q < NV; ++q) l1[q] = dreg[q];
    for (int m = lo; m < hi; ++m) {
        if (m == i) continue;
        const float* r = d2v_row(wv, d, kept, m);
#pragma unroll
        for (int q = 0; q < NV; ++q) l1[q] += d2v_ld<FROZEN>(r + lane + 64 * q);
    }
    const float inv = 1.f / (float)(hi - lo);               // (hi - lo - 1) window words + the doc tag
#pragma unroll
    for (int q = 0; q < NV; ++q) l1[q] *= inv;
}

// bisect_left(cum_table, r % cum_table[-1]): the bucket through the LDS level (the first bucket whose last entry is >= v holds the answer), then inside it
__device__ __forceinline__ int d2v_table_search(const uint32_t* cum_table, int64_t n_vocab, const uint32_t* __restrict__ top, int top_n, int top_s, uint32_t rk) {
    const uint32_t v = rk % cum_table[n_vocab - 1];
    int blo = 0, bhi = top_n;
    while (blo < bhi) { const int mid = (blo + bhi) >> 1; if (top[mid] < v) blo = mid + 1; else bhi = mid; }
    int64_t lo = (int64_t)blo * top_s, hi = min((int64_t)(blo + 1) * top_s, n_vocab);
    if (blo >= top_n) { lo = n_vocab; hi = n_vocab; }        // (v is below cum_table[-1]: never taken)
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (cum_table[mid] < v) lo = mid + 1; else hi = mid; }
    return (int)lo;
}

// the negative-sampling unit of both kernels (Args: D2vArgs or D2vInferArgs): input x (registers), predicted word `word`, Philox key (k0, k1); returns `work` in w[].
// The trainer's adds g x to the rows of syn1neg it touches and sums the loss terms; FROZEN (inference) has the same draws, targets, order of operations and skips,
// reads syn1neg with plain loads, never writes it and leaves lsum / lcnt alone
template <int NV, bool FROZEN = false, class Args>
__device__ __forceinline__ void d2v_unit(const Args& a, uint32_t k0, uint32_t k1, const uint32_t* __restrict__ top, int top_n, int top_s, const float (&x)[NV], int word, float alpha, int64_t doc,
                                         int pos, int unit, int lane, float (&w)[NV], float& lsum, float& lcnt) {
#pragma unroll
    for (int k = 0; k < NV; ++k) w[k] = 0.f;
    // lane k < 8 holds draw k: two Philox words of four draws each
    const uint4 r4 = d2v_draw(k0, k1, doc, pos, unit, SLOT_NEG0 + ((lane >> 2) & 1));
    const uint32_t rk = (lane & 3) == 0 ? r4.x : (lane & 3) == 1 ? r4.y : (lane & 3) == 2 ? r4.z : r4.w;
    const int tgt = d2v_table_search(a.cum_table, a.n_vocab, top, top_n, top_s, rk);
    for (int k = 0; k <= a.negative; ++k) {
        const int t = __builtin_amdgcn_readfirstlane(k == 0 ? word : __shfl(tgt, k - 1, 64));      // (wave-uniform: row addresses in scalar registers)
        if (k > 0 && t == word) continue;
        const float label = k == 0 ? 1.f : 0.f;
        auto* row = a.syn1neg + (int64_t)t * a.d;
        float rv[NV], f = 0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q) { rv[q] = d2v_ld<FROZEN>(row + lane + 64 * q); f += x[q] * rv[q]; }
        f = wave_reduce_sum(f);
        if (f <= -D2V_MAX_EXP || f >= D2V_MAX_EXP) continue;
        const float s = d2v_sigmoid_table(f);
        if constexpr (!FROZEN) { lsum -= logf(fmaxf(label != 0.f ? s : 1.f - s, 1e-30f)); lcnt += 1.f; }
        const float g = (label - s) * alpha;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            w[q] += g * rv[q];
            if constexpr (!FROZEN) unsafeAtomicAdd(row + lane + 64 * q, g * x[q]);
        }
    }
}

// DW > 0 (round 5): PV-DM with window == DW adds to a word vector ONCE per kept position instead of once per (position, window word).  A word at kept position m is a
// window word of positions m - DW .. m + DW: a wave that walks the document front to back holds the sums of its own pending additions to the rows of positions
// i - DW .. i + DW in registers (pend[2 DW + 1]: NV values a lane, shifted by one per position), reads a window row as memory + pending - exactly what the row would hold
// had the additions been made (gensim's sequential order inside a document; other waves' additions arrive through memory as before) - and makes ONE atomic row add when the
// position leaves the reach of every later window.  Per position: 1 + 6 atomic row adds instead of ~5 + 6 (the kernel runs at 0.8 of the chip's f32 atomic rate).  Two kept
// positions inside one reach that hold the SAME word would each miss the other's pending sum: the wave then flushes what it holds and finishes the document the plain way.
// (occupancy: the plain kernel fits six waves per SIMD in 78 registers when asked to - PV-DBOW 268 -> 253 ms a pass; the deferred one needs its 127: held to five or six it spills and loses 20 %)
template <int NV, int DW = 0>
__global__ __launch_bounds__(256, DW > 0 ? 1 : (NV <= 2 ? 6 : 5)) void k_d2v_epoch(D2vArgs a, int dm) {
    __shared__ int s_kept[4][D2V_RING];
    __shared__ uint32_t s_top[D2V_TOP];
    const int lane = threadIdx.x & 63;
    int* kept = s_kept[threadIdx.x >> 6];
    int top_s, top_n; int64_t first, stride;
    if (!d2v_prologue(a.cum_table, a.n_vocab, a.serial, s_top, top_s, top_n, first, stride)) return;
    float lsum = 0.f, lcnt = 0.f;
    for (int64_t rank = first; rank < a.n_docs; rank += stride) {
        const int64_t doc = a.order ? a.order[rank] : rank;
        const float alpha = (float)(a.alpha_start - (a.alpha_start - a.alpha_end) * (a.progress ? a.progress[rank] : (double)rank / (double)a.n_docs));
        const int64_t p0 = a.doc_ptr[doc];
        const int L = (int)(a.doc_ptr[doc + 1] - p0);
        int K = 0, base = 0;               // d2v_fill_ring's: kept words compacted so far, raw words scanned so far
        float dreg[NV];
        float* drow = a.dv + doc * a.d;
#pragma unroll
        for (int q = 0; q < NV; ++q) dreg[q] = drow[lane + 64 * q];
        constexpr int NPEND = DW > 0 ? 2 * DW + 1 : 1;
        float pend[NPEND][NV];             // DW > 0: index j <-> kept position i - DW + j
        bool defer = DW > 0;
#pragma unroll
        for (int j = 0; j < NPEND; ++j)
#pragma unroll
            for (int q = 0; q < NV; ++q) pend[j][q] = 0.f;
        auto flush_row = [&](int m, const float (&v)[NV]) { d2v_row_add(d2v_row(a.wv, a.d, kept, m), lane, v); };      // the word vector of kept position m += v
        int i = 0;
        for (;; ++i) {
            d2v_fill_ring(kept, a.words + p0, L, a.sample_int, a.k0, a.k1, doc, i + a.window + 1, lane, K, base);
            if (i >= K) break;
            const int b = (int)(d2v_draw(a.k0, a.k1, doc, i, 0, SLOT_WINDOW).x % (uint32_t)a.window), word = __builtin_amdgcn_readfirstlane(kept[i & (D2V_RING - 1)]);
            // (K is final here whenever it bounds the window: K < i + window + 1 only once every raw word has been scanned or the cap is reached)
            const int lo = max(0, i - a.window + b), hi = min(K, i + a.window + 1 - b);
            float work[NV];
            if (DW > 0 && dm) {
                if (defer) {
                    // the same word at two kept positions of this reach?  lane j holds the word of position i - DW + j (a different negative number where there is none)
                    const int mj = i - DW + lane;
                    const int wj = (lane < NPEND && mj >= 0 && mj < K) ? kept[mj & (D2V_RING - 1)] : -1 - lane;
                    bool dup = false;
#pragma unroll
                    for (int o = 1; o < NPEND; ++o) dup |= (__shfl(wj, (lane + o) & 63, 64) == wj) && lane + o < NPEND;
                    if (__ballot(dup) != 0ull) {
#pragma unroll
                        for (int j = 0; j < NPEND; ++j) {
                            const int m = i - DW + j;
                            if (m >= 0 && m < K) flush_row(m, pend[j]);
#pragma unroll
                            for (int q = 0; q < NV; ++q) pend[j][q] = 0.f;
                        }
                        defer = false;
                    }
                }
                float l1[NV];
#pragma unroll
                for (int q = 0; q < NV; ++q) l1[q] = dreg[q];
#pragma unroll
                for (int j = 0; j < NPEND; ++j) {
                    const int m = i - DW + j;
                    if (j == DW || m < lo || m >= hi) continue;
                    const float* r = d2v_row(a.wv, a.d, kept, m);
#pragma unroll
                    for (int q = 0; q < NV; ++q) l1[q] += d2v_ld(r + lane + 64 * q) + pend[j][q];
                }
                const float inv = 1.f / (float)(hi - lo);               // d2v_dm_mean's, over memory + pending (pend[j] stays in registers only under a compile-time j)
#pragma unroll
                for (int q = 0; q < NV; ++q) l1[q] *= inv;
                d2v_unit<NV>(a, a.k0, a.k1, s_top, top_n, top_s, l1, word, alpha, doc, i, 0, lane, work, lsum, lcnt);
#pragma unroll
                for (int q = 0; q < NV; ++q) dreg[q] += work[q];
#pragma unroll
                for (int j = 0; j < NPEND; ++j) {
                    const int m = i - DW + j;
                    if (j == DW || m < lo || m >= hi) continue;
                    if (defer) {
#pragma unroll
                        for (int q = 0; q < NV; ++q) pend[j][q] += work[q];
                    } else flush_row(m, work);
                }
                // position i - DW is in no later window: its row takes the sum; every slot moves one down
                if (defer && i - DW >= 0) flush_row(i - DW, pend[0]);
#pragma unroll
                for (int j = 0; j + 1 < NPEND; ++j)
#pragma unroll
                    for (int q = 0; q < NV; ++q) pend[j][q] = pend[j + 1][q];
#pragma unroll
                for (int q = 0; q < NV; ++q) pend[NPEND - 1][q] = 0.f;
            } else if (dm) {
                float l1[NV];
                d2v_dm_mean<NV, false>(a.wv, a.d, kept, lo, hi, i, dreg, lane, l1);
                d2v_unit<NV>(a, a.k0, a.k1, s_top, top_n, top_s, l1, word, alpha, doc, i, 0, lane, work, lsum, lcnt);
#pragma unroll
                for (int q = 0; q < NV; ++q) dreg[q] += work[q];
                for (int m = lo; m < hi; ++m)
                    if (m != i) flush_row(m, work);
            } else {
                int u = 0;
                for (int m = lo; m < hi; ++m) {
                    if (m == i) continue;
                    float* r = d2v_row(a.wv, a.d, kept, m);
                    float x[NV];
#pragma unroll
                    for (int q = 0; q < NV; ++q) x[q] = d2v_ld(r + lane + 64 * q);
                    d2v_unit<NV>(a, a.k0, a.k1, s_top, top_n, top_s, x, word, alpha, doc, i, 1 + u, lane, work, lsum, lcnt);
                    d2v_row_add(r, lane, work);
                    ++u;
                }
                d2v_unit<NV>(a, a.k0, a.k1, s_top, top_n, top_s, dreg, word, alpha, doc, i, 0, lane, work, lsum, lcnt);
#pragma unroll
                for (int q = 0; q < NV; ++q) dreg[q] += work[q];
            }
        }
        if (DW > 0 && dm && defer) {      // the document has ended at i = K: index j still stands for position i - DW + j; those below K hold sums
#pragma unroll
            for (int j = 0; j < DW; ++j) {
                const int m = i - DW + j;
                if (m >= 0 && m < K) flush_row(m, pend[j]);
            }
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) drow[lane + 64 * q] = dreg[q];
        __builtin_amdgcn_wave_barrier();
    }
    if (a.loss && lane == 0 && lcnt > 0.f) { atomicAdd(a.loss, (double)lsum); atomicAdd(a.loss + 1, (double)lcnt); }
}

// splitmix64 of (seed, epoch) -> the Philox key of a pass (the trainer's host side; ntf_d2v_infer's epoch loop runs inside its kernel)
__host__ __device__ inline void d2v_key(uint64_t seed, uint64_t epoch, uint32_t& k0, uint32_t& k1) {
    uint64_t x = seed ^ (epoch * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    k0 = (uint32_t)x; k1 = (uint32_t)(x >> 32);
}

// ---- infer_vector (src/mdl/emb/d2v.py:96-98): the vector of a document that was not in the corpus, trained against FROZEN tables.  gensim's infer_vector is train() on one
// document with learn_words = learn_hidden = False and train_words = False: the doc vector is the only thing that moves, so every query is independent of every other - no
// atomics, no store to a table, plain cached loads (d2v_ld<true>: the agent scope is for rows other waves add to), and the result is a pure function of (words, id, initial vector,
// tables, seed) whatever wave runs it.  One wave per query, the vector in registers from the initial row to the final store across ALL epochs of the call.
struct D2vInferArgs {
    int64_t n, n_vocab; int d, window, negative, serial, dm, epochs;
    const int64_t* q_ptr; const int32_t* q_words; const int64_t* ids; const uint32_t *sample_int, *cum_table;
    const float *wv, *syn1neg; float* vec;      // vec [n, d]: the initial vector in, the inferred one out (a row is read and written by its own wave only)
    double alpha, delta;                         // alpha of the first epoch; (alpha - min_alpha) / max(epochs - 1, 1)
    uint64_t seed;
};

// The kernel shares the trainer's prologue, ring fill, PV-DM mean and unit (d2v_unit<NV, true>, d2v_dm_mean<NV, true>: the FROZEN forms); what is its own is the loop:
// the epochs inside the kernel, around the positions.
// (the trainer's plain-kernel bounds; a query is a chain of dependent row reads, so what hides the latency is waves per SIMD.  The compiler's report for NV = 1 / 2 / 3 / 4:
//  63 / 67 / 71 / 72 VGPRs, no spill, no scratch, 20 KiB of LDS a workgroup - 8 / 7 / 7 / 7 waves a SIMD by registers, 8 workgroups a CU by LDS)
template <int NV>
__global__ __launch_bounds__(256, NV <= 2 ? 6 : 5) void k_d2v_infer(D2vInferArgs a) {
    __shared__ int s_kept[4][D2V_RING];
    __shared__ uint32_t s_top[D2V_TOP];
    const int lane = threadIdx.x & 63;
    int* kept = s_kept[threadIdx.x >> 6];
    int top_s, top_n; int64_t first, stride;
    if (!d2v_prologue(a.cum_table, a.n_vocab, a.serial, s_top, top_s, top_n, first, stride)) return;
    float no_loss = 0.f;                       // (the FROZEN unit leaves its loss arguments alone)
    for (int64_t qi = first; qi < a.n; qi += stride) {
        const int64_t doc = a.ids ? a.ids[qi] : qi;          // what the draws are counted by: a query's vector does not depend on its place in the batch
        const int64_t p0 = a.q_ptr[qi];
        const int L = (int)min(a.q_ptr[qi + 1] - p0, (int64_t)0x7fffffff);
        float dreg[NV];
        float* drow = a.vec + qi * a.d;
#pragma unroll
        for (int q = 0; q < NV; ++q) dreg[q] = drow[lane + 64 * q];
        double alpha_d = a.alpha;
        for (int e = 0; e < a.epochs; ++e) {
            uint32_t k0, k1;
            d2v_key(a.seed, (uint64_t)e, k0, k1);
            const float alpha = (float)alpha_d;
            int K = 0, base = 0;               // d2v_fill_ring's: kept words compacted so far, raw words scanned so far
            for (int i = 0;; ++i) {
                d2v_fill_ring(kept, a.q_words + p0, L, a.sample_int, k0, k1, doc, i + a.window + 1, lane, K, base);
                if (i >= K) break;
                const int b = (int)(d2v_draw(k0, k1, doc, i, 0, SLOT_WINDOW).x % (uint32_t)a.window), word = __builtin_amdgcn_readfirstlane(kept[i & (D2V_RING - 1)]);
                float work[NV];
                if (a.dm) {
                    const int lo = max(0, i - a.window + b), hi = min(K, i + a.window + 1 - b);
                    float l1[NV];
                    d2v_dm_mean<NV, true>(a.wv, a.d, kept, lo, hi, i, dreg, lane, l1);
                    d2v_unit<NV, true>(a, k0, k1, s_top, top_n, top_s, l1, word, alpha, doc, i, 0, lane, work, no_loss, no_loss);
                } else      // PV-DBOW: infer_vector leaves train_words = False - the window-word units do not run (and their draws are not taken)
                    d2v_unit<NV, true>(a, k0, k1, s_top, top_n, top_s, dreg, word, alpha, doc, i, 0, lane, work, no_loss, no_loss);
#pragma unroll
                for (int q = 0; q < NV; ++q) dreg[q] += work[q];
            }
            alpha_d -= a.delta;                // gensim's Python loop: one subtraction in double per epoch
            __builtin_amdgcn_wave_barrier();   // the next epoch refills the ring from slot 0
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) drow[lane + 64 * q] = dreg[q];
    }
}

// ---- the host side's checks and launch shape, once.  A check returns the text of what is wrong under the caller's prefix, or an empty string
std::string d2v_param_error(const std::string& prefix, const char* window_note, int dm, int window, int negative) {
    if (window < 1 || window > 255 || (!dm && 2 * window > 254)) return prefix + ": window outside 1..255 (dm = 0: 1..127" + window_note;
    if (negative < 0 || negative > 8) return prefix + ": negative outside 0..8";
    if (dm != 0 && dm != 1) return prefix + ": dm is 0 or 1";
    return "";
}
// documents in CSR form: ptr (called `name` in the text) [n + 1] from 0 and monotone, words inside the vocabulary
std::string d2v_csr_error(const std::string& prefix, const char* name, const int64_t* ptr, int64_t n, const int32_t* words, int64_t n_vocab) {
    if (ptr[0] != 0) return prefix + ": " + name + "[0] != 0";
    for (int64_t i = 0; i < n; ++i) if (ptr[i + 1] < ptr[i]) return prefix + ": " + name + " not monotone";
    for (int64_t p = 0; p < ptr[n]; ++p) if (words[p] < 0 || words[p] >= n_vocab) return prefix + ": word index out of the vocabulary";
    return "";
}
// n one-wave items.  Parallel: enough waves to fill the chip several times over, each striding through the items; serial: one wave
struct D2vDims { dim3 grid, block; };
D2vDims d2v_dims(int64_t n, bool serial) { return {dim3(serial ? 1u : (unsigned)std::min<int64_t>((n + 3) / 4, 256 * 16)), dim3(serial ? 64 : 256)}; }
// ntf_d2v_get / ntf_d2v_set: the table `what` names and its rows, on the handle's device with its stream drained
int d2v_table(ntf_d2v* h, const void* host, int what, float** table, int64_t* rows) {
    if (!h || !host || what < 0 || what > 2) return NTF_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->st));
    *table = what == 0 ? h->dv : what == 1 ? h->wv : h->syn1neg;
    *rows = what == 0 ? h->n_docs : h->n_vocab;
    return NTF_OK;
}

}  // namespace

extern "C" void ntf_d2v_destroy(ntf_d2v* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    for (void* p : {(void*)h->doc_ptr, (void*)h->words, (void*)h->sample_int, (void*)h->cum_table, (void*)h->dv, (void*)h->wv, (void*)h->syn1neg, (void*)h->order, (void*)h->progress, (void*)h->d_loss,
                    (void*)h->q_ptr, (void*)h->q_ids, (void*)h->q_words, (void*)h->q_vec})
        if (p) hipFree(p);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

extern "C" int ntf_d2v_create(int device, int64_t n_docs, int64_t n_vocab, int32_t d, const int64_t* doc_ptr, const int32_t* words, const uint32_t* sample_int,
                              const uint32_t* cum_table, const float* init_wv, const float* init_dv, uint64_t seed, ntf_d2v** out) {
    if (!out) { g_d2v_create_error = "out is NULL"; return NTF_EINVAL; }
    *out = nullptr;
    if (n_docs < 1 || n_vocab < 1 || d < 1 || d > 256 || !doc_ptr || !words || !sample_int || !cum_table || !init_wv || !init_dv) {
        g_d2v_create_error = "d2v: need n_docs >= 1, n_vocab >= 1, 1 <= d <= 256, the documents, the vocabulary tables and the initial vectors"; return NTF_EINVAL; }
    const std::string bad = d2v_csr_error("d2v", "doc_ptr", doc_ptr, n_docs, words, n_vocab);
    if (!bad.empty()) { g_d2v_create_error = bad; return NTF_EINVAL; }
    const int64_t nw = doc_ptr[n_docs];
    for (int64_t v = 1; v < n_vocab; ++v) if (cum_table[v] < cum_table[v - 1]) { g_d2v_create_error = "d2v: cum_table not monotone"; return NTF_EINVAL; }
    if (cum_table[n_vocab - 1] == 0) { g_d2v_create_error = "d2v: empty cum_table"; return NTF_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_d2v_create_error = "no such HIP device (there is no CPU fallback)"; return NTF_EHIP; }
    hipSetDevice(device);
    ntf_d2v* h = new ntf_d2v();
    h->device = device; h->n_docs = n_docs; h->n_vocab = n_vocab; h->n_words = nw; h->d = d; h->dp = (d + 63) / 64 * 64; h->seed = seed;
    const int64_t dp = h->dp;
    int rc = NTF_OK;
    auto A = [&](int r) { if (rc == NTF_OK) rc = r; };
    if (hipStreamCreate(&h->st) != hipSuccess) { g_d2v_create_error = "hipStreamCreate failed"; delete h; return NTF_EHIP; }
    A(dev_alloc(h, &h->doc_ptr, n_docs + 1)); A(dev_alloc(h, &h->words, std::max<int64_t>(nw, 1))); A(dev_alloc(h, &h->sample_int, n_vocab)); A(dev_alloc(h, &h->cum_table, n_vocab));
    A(dev_alloc(h, &h->dv, n_docs * dp)); A(dev_alloc(h, &h->wv, n_vocab * dp)); A(dev_alloc(h, &h->syn1neg, n_vocab * dp)); A(dev_alloc(h, &h->order, n_docs)); A(dev_alloc(h, &h->progress, n_docs)); A(dev_alloc(h, &h->d_loss, 2));
    if (rc != NTF_OK) { g_d2v_create_error = h->err; ntf_d2v_destroy(h); return rc; }
    bool ok = true;
    auto H = [&](hipError_t s) { ok = ok && s == hipSuccess; };
    H(hipMemcpy(h->doc_ptr, doc_ptr, (n_docs + 1) * 8, hipMemcpyHostToDevice));
    if (nw) H(hipMemcpy(h->words, words, nw * 4, hipMemcpyHostToDevice));
    H(hipMemcpy(h->sample_int, sample_int, n_vocab * 4, hipMemcpyHostToDevice));
    H(hipMemcpy(h->cum_table, cum_table, n_vocab * 4, hipMemcpyHostToDevice));
    // any vector size (the reference's CI trains d9 tables, data.embedding.d is free): rows of d floats at a stride of dp, the pad columns zero.  A zero column of
    // every table stays zero through every update (each update is a multiple of another table's same column), and adds nothing to a dot product
    H(upload_padded(h->dv, dp, init_dv, d, n_docs));
    H(upload_padded(h->wv, dp, init_wv, d, n_vocab));
    H(hipMemsetAsync(h->syn1neg, 0, (size_t)n_vocab * dp * 4, h->st));
    H(hipStreamSynchronize(h->st));
    if (!ok) { g_d2v_create_error = "device initialisation failed"; ntf_d2v_destroy(h); return NTF_EHIP; }
    *out = h;
    return NTF_OK;
}

extern "C" int ntf_d2v_train_epoch(ntf_d2v* h, int32_t dm, int32_t window, int32_t negative, double alpha_start, double alpha_end, uint64_t epoch, int32_t serial,
                                   const int64_t* order, const double* progress, double* mean_loss, double* device_ms) {
    if (!h) { g_d2v_create_error = "d2v train: the handle is NULL"; return NTF_EINVAL; }
    const std::string bad = d2v_param_error("d2v train", ": the unit index 1 + u of a window word is 8 bits of the Philox counter)", dm, window, negative);
    if (!bad.empty()) FAIL(h, NTF_EINVAL, bad);
    HIPCHK(h, hipSetDevice(h->device));
    if (order) {
        std::vector<char> seen((size_t)h->n_docs, 0);
        for (int64_t i = 0; i < h->n_docs; ++i) { if (order[i] < 0 || order[i] >= h->n_docs || seen[(size_t)order[i]]) FAIL(h, NTF_EINVAL, "d2v: order is not a permutation of the documents"); seen[(size_t)order[i]] = 1; }
        HIPCHK(h, hipMemcpyAsync(h->order, order, h->n_docs * 8, hipMemcpyHostToDevice, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
    }
    if (progress) {
        for (int64_t i = 0; i < h->n_docs; ++i) if (!(progress[i] >= 0.0 && progress[i] <= 1.0)) FAIL(h, NTF_EINVAL, "d2v: progress outside [0, 1]");
        HIPCHK(h, hipMemcpyAsync(h->progress, progress, h->n_docs * 8, hipMemcpyHostToDevice, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
    }
    HIPCHK(h, hipMemsetAsync(h->d_loss, 0, 16, h->st));
    D2vArgs a;
    a.n_docs = h->n_docs; a.n_vocab = h->n_vocab; a.d = h->dp; a.window = window; a.negative = negative; a.serial = serial ? 1 : 0;
    a.doc_ptr = h->doc_ptr; a.words = h->words; a.sample_int = h->sample_int; a.cum_table = h->cum_table; a.order = order ? h->order : nullptr; a.progress = progress ? h->progress : nullptr;
    a.dv = h->dv; a.wv = h->wv; a.syn1neg = h->syn1neg; a.alpha_start = alpha_start; a.alpha_end = alpha_end; a.loss = mean_loss ? h->d_loss : nullptr;
    d2v_key(h->seed, epoch, a.k0, a.k1);
    const D2vDims dims = d2v_dims(h->n_docs, serial != 0);
    // PV-DM at the reference's window (src/mdl/emb/__config__.yaml: w = 5): word-vector additions deferred to one per kept position (k_d2v_epoch<.., 5>); NTF_D2V_DEFER=0 (read per call): the plain kernel
    const char* defer_env = getenv("NTF_D2V_DEFER");
    const bool defer_ok = !(defer_env && atoi(defer_env) == 0);
    const int rc = timed_launch(h, device_ms, "d2v", [&] {
        if (dm && window == 5 && defer_ok && h->dp >= 128) {     // (d = 64: the rows are 256 B and the plain kernel's shorter chain wins - 45.7 against 49.4 ms; d = 128 / 192 / 256: 55 / 78 / 98 against 66 / 102 / 133)
            with_nv<2>(h->dp / 64, [&](auto nv) { hipLaunchKernelGGL((k_d2v_epoch<decltype(nv)::value, 5>), dims.grid, dims.block, 0, h->st, a, dm); });   // <1, 5> is never launched, so never built
        } else
            with_nv(h->dp / 64, [&](auto nv) { hipLaunchKernelGGL(k_d2v_epoch<decltype(nv)::value>, dims.grid, dims.block, 0, h->st, a, dm); });
    });
    if (rc != NTF_OK) return rc;
    if (mean_loss) {
        double l[2] = {0, 0};
        HIPCHK(h, hipMemcpy(l, h->d_loss, 16, hipMemcpyDeviceToHost));
        *mean_loss = l[1] > 0 ? l[0] / l[1] : 0.0;
    }
    return NTF_OK;
}

extern "C" int ntf_d2v_infer(ntf_d2v* h, int64_t n, const int64_t* q_ptr, const int32_t* q_words, const int64_t* ids, int32_t dm, int32_t window, int32_t negative, int32_t epochs,
                             double alpha, double min_alpha, uint64_t seed, int32_t serial, const float* init, float* out, double* device_ms) {
    if (!h) { g_d2v_create_error = "d2v infer: the handle is NULL"; return NTF_EINVAL; }
    if (!q_ptr || !q_words || !init || !out) FAIL(h, NTF_EINVAL, "d2v infer: q_ptr, q_words, init and out are required");
    if (n < 1) FAIL(h, NTF_EINVAL, "d2v infer: n < 1");
    std::string bad = d2v_param_error("d2v infer", "), as ntf_d2v_train_epoch", dm, window, negative);
    if (!bad.empty()) FAIL(h, NTF_EINVAL, bad);
    if (epochs < 1) FAIL(h, NTF_EINVAL, "d2v infer: epochs < 1");
    if (!std::isfinite(alpha) || !std::isfinite(min_alpha)) FAIL(h, NTF_EINVAL, "d2v infer: alpha / min_alpha not finite");
    bad = d2v_csr_error("d2v infer", "q_ptr", q_ptr, n, q_words, h->n_vocab);
    if (!bad.empty()) FAIL(h, NTF_EINVAL, bad);
    const int64_t nw = q_ptr[n];
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->st));
    const int64_t dp = h->dp; const int d = h->d;
    {
        int rc = NTF_OK;
        auto A = [&](int r) { if (rc == NTF_OK) rc = r; };
        A(dev_grow(h, &h->q_ptr, &h->q_ptr_cap, n + 1)); A(dev_grow(h, &h->q_ids, &h->q_ids_cap, n)); A(dev_grow(h, &h->q_vec, &h->q_vec_cap, n * dp));
        A(dev_grow(h, &h->q_words, &h->q_words_cap, std::max<int64_t>(nw, 1)));
        if (rc != NTF_OK) return rc;
    }
    HIPCHK(h, hipMemcpy(h->q_ptr, q_ptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
    if (nw) HIPCHK(h, hipMemcpy(h->q_words, q_words, (size_t)nw * 4, hipMemcpyHostToDevice));
    if (ids) HIPCHK(h, hipMemcpy(h->q_ids, ids, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(h, upload_padded(h->q_vec, dp, init, d, n));       // the pad columns zero, as the tables'
    D2vInferArgs a;
    a.n = n; a.n_vocab = h->n_vocab; a.d = h->dp; a.window = window; a.negative = negative; a.serial = serial ? 1 : 0; a.dm = dm; a.epochs = epochs;
    a.q_ptr = h->q_ptr; a.q_words = h->q_words; a.ids = ids ? h->q_ids : nullptr; a.sample_int = h->sample_int; a.cum_table = h->cum_table;
    a.wv = h->wv; a.syn1neg = h->syn1neg; a.vec = h->q_vec;
    a.alpha = alpha; a.delta = (alpha - min_alpha) / (double)std::max(epochs - 1, 1); a.seed = seed;
    const D2vDims dims = d2v_dims(n, serial != 0);
    const int rc = timed_launch(h, device_ms, "d2v infer", [&] { with_nv(h->dp / 64, [&](auto nv) { hipLaunchKernelGGL(k_d2v_infer<decltype(nv)::value>, dims.grid, dims.block, 0, h->st, a); }); });
    if (rc != NTF_OK) return rc;
    HIPCHK(h, hipMemcpy2D(out, (size_t)d * 4, h->q_vec, (size_t)dp * 4, (size_t)d * 4, (size_t)n, hipMemcpyDeviceToHost));
    return NTF_OK;
}

extern "C" int ntf_d2v_get(ntf_d2v* h, int what, float* host) {   // what: 0 = doc vectors [n_docs, d], 1 = word vectors [n_vocab, d], 2 = syn1neg [n_vocab, d]
    float* src; int64_t rows;
    if (const int rc = d2v_table(h, host, what, &src, &rows); rc != NTF_OK) return rc;
    HIPCHK(h, hipMemcpy2D(host, (size_t)h->d * 4, src, (size_t)h->dp * 4, (size_t)h->d * 4, (size_t)rows, hipMemcpyDeviceToHost));
    return NTF_OK;
}

extern "C" int ntf_d2v_set(ntf_d2v* h, int what, const float* host) {   // resume from a saved table (same `what` as ntf_d2v_get)
    float* dst; int64_t rows;
    if (const int rc = d2v_table(h, host, what, &dst, &rows); rc != NTF_OK) return rc;
    HIPCHK(h, hipMemcpy2D(dst, (size_t)h->dp * 4, host, (size_t)h->d * 4, (size_t)h->d * 4, (size_t)rows, hipMemcpyHostToDevice));
    return NTF_OK;
}
