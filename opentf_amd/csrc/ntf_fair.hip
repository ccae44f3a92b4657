// The fair stage on the device (include/opentf_amd_fair.h, opentf_amd_fairsort.h): DetGreedy / DetCons / DetRelaxed / DetConstSort re-ranking of ranked expert lists
// and the NDKL / skew / infeasible measures of a ranked list (Geyik, Ambler, Kenthapadi, KDD 2019).  One wave per row, one lane per group, four rows per workgroup;
// the per-row work is a strictly serial loop over ranks with a vote over the groups at each rank: integer / index work and a few f64 operations, latency-bound,
// nothing here is MFMA-shaped.
#include "../../include/opentf_amd_fairsort.h"
#include "ntf_device.h"
#include "ntf_host.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

// every f64 result below is pinned operation by operation (tests/fair_reference.py): no product may fuse into a sum
#pragma clang fp contract(off)

namespace ntf {

constexpr int FAIR_ROWS = 4;             // rows (waves) per workgroup
constexpr int FAIR_NONE = 0xFFFF;        // "no position": every real one is < NTF_FAIR_MAX_K = 2048
constexpr int FAIR_MAX_CUT = 8;
struct FairCuts { int n; int k[FAIR_MAX_CUT]; };

// the group labels of a row's first `len` candidates, gathered through the candidate ids into the wave's LDS row
__device__ __forceinline__ void fair_gather(uint8_t* grp, const int32_t* __restrict__ ids, int len, const uint8_t* __restrict__ group, int lane) {
    for (int j = lane; j < len; j += 64) grp[j] = group[ids[j]];
}

// the next-same-group link of every position, back to front: lane g threads the positions of its group; what it saw last (the smallest) is its head
__device__ __forceinline__ int fair_links(const uint8_t* grp, uint16_t* nxt, int K, int lane) {
    int head = FAIR_NONE;
    for (int j = K - 1; j >= 0; --j)
        if (grp[j] == lane) { nxt[j] = (uint16_t)head; head = j; }
    return head;
}

// Lane g < G owns cnt[g], head[g], p_g and its own lo / hi / key.  LDS per row: the labels (1 B a position), the next-same-group link of every position and the
// emitted positions (2 B each): 10 KB at K = 2048.  A step: two ballots (A, B), one wave-wide lexicographic min over (key, head) by shuffles, and the winner lane
// follows its link.  The results leave the LDS row coalesced once the row is done.
__global__ __launch_bounds__(64 * FAIR_ROWS) void k_fair_rerank(int alg, const int32_t* __restrict__ cand_idx, const float* __restrict__ cand_val, int64_t n, int K,
                                                                  const uint8_t* __restrict__ group, int G, const double* __restrict__ p, int p_per_row, int K_out,
                                                                  int32_t* __restrict__ out_idx, float* __restrict__ out_val, int32_t* __restrict__ out_pos) {
    __shared__ uint8_t s_grp[FAIR_ROWS][NTF_FAIR_MAX_K];
    __shared__ uint16_t s_next[FAIR_ROWS][NTF_FAIR_MAX_K];
    __shared__ uint16_t s_pos[FAIR_ROWS][NTF_FAIR_MAX_K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * FAIR_ROWS + w;
    const bool active = r < n;
    const int64_t row = active ? r : n - 1;          // a wave past the last row repeats it and stores nothing: every wave reaches every barrier
    uint8_t* grp = s_grp[w]; uint16_t* nxt = s_next[w]; uint16_t* pos = s_pos[w];
    const int32_t* ids = cand_idx + row * K;
    fair_gather(grp, ids, K, group, lane);
    __syncthreads();
    int head = fair_links(grp, nxt, K, lane);
    const double pg = lane < G ? p[(p_per_row ? row * G : 0) + lane] : 0.0;
    int cnt = 0;
    for (int k = 1; k <= K_out; ++k) {
        const double x = (double)k * pg, lo = floor(x), hi = ceil(x), c = (double)cnt;
        const bool live = lane < G && head != FAIR_NONE;
        const bool inA = live && c < lo, inB = live && !inA && c < hi;
        const unsigned long long mA = __ballot(inA), mB = __ballot(inB);
        const bool keyed = !mA && mB && alg != NTF_FAIR_DET_GREEDY;
        const bool elig = mA ? inA : mB ? inB : live;
        int h = elig ? head : 0x7fffffff;
        if (keyed) {
            double q = hi / pg;                                          // a lane of B has hi >= 1, hence p_g > 0
            if (alg == NTF_FAIR_DET_RELAXED) q = ceil(q);
            double key = elig ? q : HUGE_VAL;                          // (an eligible key may itself be +inf, for a subnormal p_g: its real head still wins the tie)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double k2 = __shfl_xor(key, o, 64); const int h2 = __shfl_xor(h, o, 64);
                if (k2 < key || (k2 == key && h2 < h)) { key = k2; h = h2; }
            }
        } else {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) h = min(h, __shfl_xor(h, o, 64));
        }
        if (live && head == h) { pos[k - 1] = (uint16_t)head; head = nxt[head]; ++cnt; }      // heads are distinct positions: one lane
    }
    __syncthreads();
    if (!active) return;
    for (int t = lane; t < K_out; t += 64) {
        const int j = pos[t];
        out_idx[row * K_out + t] = ids[j];
        if (out_pos) out_pos[row * K_out + t] = j;
        if (out_val) out_val[row * K_out + t] = cand_val[row * K + t];
    }
}

// Lanes hold c_g(k); one pass over k.  KL_k is summed over g ASCENDING (part of the definition): the lanes' terms are read one by one in lane order, the lanes of a
// group that has not appeared yet are skipped (their term is no part of the sum).  The weighted sums over k are carried by every lane alike.
__global__ __launch_bounds__(64 * FAIR_ROWS) void k_fair_metrics(const int32_t* __restrict__ idx, int64_t n, int K, const uint8_t* __restrict__ group, int G,
                                                                   const double* __restrict__ p, int p_per_row, FairCuts cut, double* __restrict__ out_ndkl,
                                                                   double* __restrict__ out_skew) {
    __shared__ uint8_t s_grp[FAIR_ROWS][NTF_FAIR_MAX_K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * FAIR_ROWS + w;
    const bool active = r < n;
    const int64_t row = active ? r : n - 1;
    int kmax = 0;
    for (int q = 0; q < cut.n; ++q) kmax = max(kmax, cut.k[q]);
    uint8_t* grp = s_grp[w];
    fair_gather(grp, idx + row * K, kmax, group, lane);
    __syncthreads();
    if (!active) return;
    const double pg = lane < G ? p[(p_per_row ? row * G : 0) + lane] : 0.0;
    int c = 0;
    double num = 0.0, den = 0.0;
    for (int k = 1; k <= kmax; ++k) {
        if (grp[k - 1] == lane) ++c;
        const double d = (double)c / (double)k;
        const double term = c > 0 ? d * log(d / pg) : 0.0;             // p_g == 0 < c: d / 0 = +inf, ln = +inf, the term and the NDKL are +inf
        unsigned long long m = __ballot(c > 0);
        double kl = 0.0;
        while (m) { const int g = __builtin_ctzll(m); m &= m - 1; kl += __shfl(term, g, 64); }
        const double wk = 1.0 / log2((double)(k + 1));
        num += wk * kl; den += wk;
        for (int q = 0; q < cut.n; ++q) {
            if (cut.k[q] != k) continue;
            if (out_ndkl && lane == 0) out_ndkl[row * cut.n + q] = num / den;
            if (out_skew && lane < G)
                out_skew[(row * cut.n + q) * G + lane] = c == 0 ? (pg > 0.0 ? -HUGE_VAL : 0.0) : (pg == 0.0 ? HUGE_VAL : log(d / pg));
        }
    }
}

// DetConstSort (include/opentf_amd_fairsort.h).  The layout of k_fair_rerank: lane g < G owns head[g], min[g] and p_g (the definition's cnt[g] decides nothing and is
// not kept).  LDS per row: the labels, the links and the list L as positions and deadlines (2 B each, a deadline is at most K_out + G + 1 <= 2113): 14 KB
// at K = 2048, 56 KB a workgroup.
// An insertion is not a swap loop.  The serial loop moves the new entry j left past every entry that may move down ("deadline >= the rank it lands on and position
// > j") and stops at the first that may not: it ends right of the NEAREST entry on its left that fails that test.  The wave looks at 64 ranks at a time, leftwards
// from the tail; one ballot finds the stop in a chunk (its highest set bit), the lanes right of it store their entry one rank to the right, and the new entry
// goes into the hole.  Every entry that shifts was tested for exactly that move, which is why this equals the serial definition.  Chunks are walked from the right
// and a chunk is read whole before any lane of it writes (the value written is the value read), so the shifted block never overwrites what is still to be read.
// Every ballot and shuffle stands outside lane-dependent control flow: the loops below run on wave-uniform values only.
__global__ __launch_bounds__(64 * FAIR_ROWS) void k_fair_constsort(const int32_t* __restrict__ cand_idx, const float* __restrict__ cand_val, int64_t n, int K,
                                                                     const uint8_t* __restrict__ group, int G, const double* __restrict__ p, int p_per_row, int K_out,
                                                                     int32_t* __restrict__ out_idx, float* __restrict__ out_val, int32_t* __restrict__ out_pos,
                                                                     int32_t* __restrict__ out_tail) {
    __shared__ uint8_t s_grp[FAIR_ROWS][NTF_FAIR_MAX_K];
    __shared__ uint16_t s_next[FAIR_ROWS][NTF_FAIR_MAX_K];
    __shared__ uint16_t s_pos[FAIR_ROWS][NTF_FAIR_MAX_K];
    __shared__ uint16_t s_dl[FAIR_ROWS][NTF_FAIR_MAX_K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * FAIR_ROWS + w;
    const bool active = r < n;
    const int64_t row = active ? r : n - 1;          // a wave past the last row repeats it and stores nothing: every wave reaches every barrier
    uint8_t* grp = s_grp[w]; uint16_t* nxt = s_next[w]; uint16_t* pos = s_pos[w]; uint16_t* dl = s_dl[w];
    const int32_t* ids = cand_idx + row * K;
    fair_gather(grp, ids, K, group, lane);
    __syncthreads();
    int head = fair_links(grp, nxt, K, lane);
    const double pg = lane < G ? p[(p_per_row ? row * G : 0) + lane] : 0.0;
    int mn = 0, len = 0;                             // len = |L|, wave-uniform
    for (int k = 1; k <= K_out + G + 1 && len < K_out; ++k) {
        const int t = (int)floor((double)k * pg);
        bool due = lane < G && head != FAIR_NONE && t > mn;
        mn = t;
        unsigned long long mC = __ballot(due);
        while (mC && len < K_out) {
            int j = due ? head : 0x7fffffff;                                       // the group of C with the smallest head
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) j = min(j, __shfl_xor(j, o, 64));
            // the stop: the nearest index i < len (rank i + 1) whose entry may not move to rank i + 2; the lanes right of it shift as they go
            int hole = 0;
            for (int hi = len; hi > 0; hi -= 64) {
                const int i = hi - 64 + lane;
                const int pj = i >= 0 ? pos[i] : 0, d = i >= 0 ? dl[i] : 0;        // (i < 0: no entry there, the ballot leaves it out)
                const unsigned long long stop = __ballot(i >= 0 && (d < i + 2 || pj < j));
                const int s = stop ? hi - 1 - __builtin_clzll(stop) : hi - 65;     // the stop's index, or none in this chunk
                if (i > s && i >= 0) { pos[i + 1] = (uint16_t)pj; dl[i + 1] = (uint16_t)d; }
                if (stop) { hole = s + 1; break; }
            }
            if (lane == 0) { pos[hole] = (uint16_t)j; dl[hole] = (uint16_t)k; }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                 // the list is shared by the wave's lanes: the next scan reads these stores
            ++len;
            if (due && head == j) { due = false; head = nxt[head]; }               // heads are distinct positions: one lane
            mC = __ballot(due);
        }
    }
    int tail = 0;
    for (; len < K_out; ++len, ++tail) {                                           // the best untaken candidate, no swap
        int j = lane < G && head != FAIR_NONE ? head : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) j = min(j, __shfl_xor(j, o, 64));
        if (head == j) { pos[len] = (uint16_t)j; head = nxt[head]; }
    }
    __syncthreads();
    if (!active) return;
    if (out_tail && lane == 0) out_tail[row] = tail;
    for (int t = lane; t < K_out; t += 64) {
        const int j = pos[t];
        out_idx[row * K_out + t] = ids[j];
        if (out_pos) out_pos[row * K_out + t] = j;
        if (out_val) out_val[row * K_out + t] = cand_val[row * K + t];
    }
}

// InfeasibleIndex / InfeasibleCount: lanes hold c_g(k) as in k_fair_metrics; one pass over k, one ballot per k on "c_g(k) < floor(k p_g)", a popcount for the count
__global__ __launch_bounds__(64 * FAIR_ROWS) void k_fair_infeasible(const int32_t* __restrict__ idx, int64_t n, int K, const uint8_t* __restrict__ group, int G,
                                                                      const double* __restrict__ p, int p_per_row, FairCuts cut, int32_t* __restrict__ out_index,
                                                                      int32_t* __restrict__ out_count) {
    __shared__ uint8_t s_grp[FAIR_ROWS][NTF_FAIR_MAX_K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * FAIR_ROWS + w;
    const bool active = r < n;
    const int64_t row = active ? r : n - 1;
    int kmax = 0;
    for (int q = 0; q < cut.n; ++q) kmax = max(kmax, cut.k[q]);
    uint8_t* grp = s_grp[w];
    fair_gather(grp, idx + row * K, kmax, group, lane);
    __syncthreads();
    if (!active) return;
    const double pg = lane < G ? p[(p_per_row ? row * G : 0) + lane] : 0.0;
    int c = 0, index = 0, count = 0;
    for (int k = 1; k <= kmax; ++k) {
        if (grp[k - 1] == lane) ++c;
        const unsigned long long viol = __ballot(lane < G && c < (int)floor((double)k * pg));
        index += viol != 0; count += __popcll(viol);
        for (int q = 0; q < cut.n; ++q) {
            if (cut.k[q] != k || lane != 0) continue;
            if (out_index) out_index[row * cut.n + q] = index;
            if (out_count) out_count[row * cut.n + q] = count;
        }
    }
}

}  // namespace ntf

using namespace ntf;

namespace {

// what every entry takes: the ranked ids, the labels and the target
bool fair_args_ok(const int32_t* idx, int64_t n, int32_t K, const uint8_t* group, int64_t n_experts, int32_t G, const double* p, int64_t n_p) {
    if (!idx || !group || !p || n < 1 || K < 1 || K > NTF_FAIR_MAX_K || G < 1 || G > NTF_FAIR_MAX_GROUPS || n_experts < 1 || (n_p != 1 && n_p != n)) return false;
    if ((n + FAIR_ROWS - 1) / FAIR_ROWS > 0x7fffffff) return false;
    for (int64_t i = 0; i < n_experts; ++i) if (group[i] >= G) return false;
    for (int64_t i = 0; i < n * K; ++i) if (idx[i] < 0 || idx[i] >= n_experts) return false;
    for (int64_t i = 0; i < n_p; ++i) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) { const double v = p[i * G + g]; if (!std::isfinite(v) || v < 0.0 || v > 1.0) return false; s += v; }
        if (!(std::fabs(s - 1.0) <= 1e-6)) return false;
    }
    return true;
}

// the cutoffs of a measure: at most FAIR_MAX_CUT, each in [1, K]
bool fair_cuts_ok(const int32_t* cutoffs, int32_t n_cut, int32_t K, FairCuts* cut) {
    if (!cutoffs || n_cut < 1 || n_cut > FAIR_MAX_CUT) return false;
    cut->n = n_cut;
    for (int q = 0; q < FAIR_MAX_CUT; ++q) cut->k[q] = 0;
    for (int q = 0; q < n_cut; ++q) { if (cutoffs[q] < 1 || cutoffs[q] > K) return false; cut->k[q] = cutoffs[q]; }
    return true;
}

// NTF_FAIR_TIMES=1 (read per call): one line on stderr with the call's upload / kernel / download split (profiles/fair_time.py)
struct PhaseClock {
    bool on; std::chrono::steady_clock::time_point t; double ms[3] = {0, 0, 0};
    PhaseClock() { const char* e = getenv("NTF_FAIR_TIMES"); on = e && e[0] == '1'; t = std::chrono::steady_clock::now(); }
    void lap(int i) {
        if (!on) return;
        if (i <= 1) hipDeviceSynchronize();      // (the uploads and the kernel have finished before their lap is read)
        const auto now = std::chrono::steady_clock::now();
        ms[i] = std::chrono::duration<double, std::milli>(now - t).count(); t = now;
    }
    void report(const char* name) { if (on) fprintf(stderr, "%s: upload %.3f ms kernel %.3f ms download %.3f ms\n", name, ms[0], ms[1], ms[2]); }
};

}  // namespace

extern "C" int ntf_fair_rerank(int device, int32_t algorithm, const int32_t* cand_idx, const float* cand_val, int64_t n, int32_t K, const uint8_t* group,
                               int64_t n_experts, int32_t G, const double* p, int64_t n_p, int32_t K_out, int32_t* out_idx, float* out_val, int32_t* out_pos) {
    if (algorithm != NTF_FAIR_DET_GREEDY && algorithm != NTF_FAIR_DET_CONS && algorithm != NTF_FAIR_DET_RELAXED) return NTF_EINVAL;
    if (!out_idx || (out_val && !cand_val) || K_out < 1 || K_out > K) return NTF_EINVAL;
    if (!fair_args_ok(cand_idx, n, K, group, n_experts, G, p, n_p)) return NTF_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return NTF_EHIP;
    PhaseClock clk;
    const size_t in = (size_t)n * K, out = (size_t)n * K_out;
    DevBuf di, dv, dg, dp, oi, ov, op;
    if (!di.put(cand_idx, in * 4) || (out_val && !dv.put(cand_val, in * 4)) || !dg.put(group, (size_t)n_experts) || !dp.put(p, (size_t)n_p * G * 8) ||
        !oi.alloc(out * 4) || (out_val && !ov.alloc(out * 4)) || (out_pos && !op.alloc(out * 4))) return NTF_ENOMEM;
    clk.lap(0);
    hipLaunchKernelGGL(k_fair_rerank, dim3((unsigned)((n + FAIR_ROWS - 1) / FAIR_ROWS)), dim3(64 * FAIR_ROWS), 0, 0, (int)algorithm, di.as<const int32_t>(),
                       out_val ? dv.as<const float>() : nullptr, n, (int)K, dg.as<const uint8_t>(), (int)G, dp.as<const double>(), n_p == 1 ? 0 : 1, (int)K_out,
                       oi.as<int32_t>(), out_val ? ov.as<float>() : nullptr, out_pos ? op.as<int32_t>() : nullptr);
    if (hipGetLastError() != hipSuccess) return NTF_EHIP;
    clk.lap(1);
    if (hipMemcpy(out_idx, oi.p, out * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (out_val && hipMemcpy(out_val, ov.p, out * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (out_pos && hipMemcpy(out_pos, op.p, out * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    clk.lap(2); clk.report("ntf_fair_rerank");
    return NTF_OK;
}

extern "C" int ntf_fair_metrics(int device, const int32_t* idx, int64_t n, int32_t K, const uint8_t* group, int64_t n_experts, int32_t G, const double* p, int64_t n_p,
                                const int32_t* cutoffs, int32_t n_cut, double* out_ndkl, double* out_skew) {
    FairCuts cut;
    if (!fair_cuts_ok(cutoffs, n_cut, K, &cut) || (!out_ndkl && !out_skew)) return NTF_EINVAL;
    if (!fair_args_ok(idx, n, K, group, n_experts, G, p, n_p)) return NTF_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return NTF_EHIP;
    PhaseClock clk;
    const size_t nd = (size_t)n * n_cut * 8, ns = nd * G;
    DevBuf di, dg, dp, on, os;
    if (!di.put(idx, (size_t)n * K * 4) || !dg.put(group, (size_t)n_experts) || !dp.put(p, (size_t)n_p * G * 8) || (out_ndkl && !on.alloc(nd)) ||
        (out_skew && !os.alloc(ns))) return NTF_ENOMEM;
    clk.lap(0);
    hipLaunchKernelGGL(k_fair_metrics, dim3((unsigned)((n + FAIR_ROWS - 1) / FAIR_ROWS)), dim3(64 * FAIR_ROWS), 0, 0, di.as<const int32_t>(), n, (int)K,
                       dg.as<const uint8_t>(), (int)G, dp.as<const double>(), n_p == 1 ? 0 : 1, cut, out_ndkl ? on.as<double>() : nullptr,
                       out_skew ? os.as<double>() : nullptr);
    if (hipGetLastError() != hipSuccess) return NTF_EHIP;
    clk.lap(1);
    if (out_ndkl && hipMemcpy(out_ndkl, on.p, nd, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (out_skew && hipMemcpy(out_skew, os.p, ns, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    clk.lap(2); clk.report("ntf_fair_metrics");
    return NTF_OK;
}

extern "C" int ntf_fair_constsort(int device, const int32_t* cand_idx, const float* cand_val, int64_t n, int32_t K, const uint8_t* group, int64_t n_experts, int32_t G,
                                  const double* p, int64_t n_p, int32_t K_out, int32_t* out_idx, float* out_val, int32_t* out_pos, int32_t* out_tail) {
    if (!out_idx || (out_val && !cand_val) || K_out < 1 || K_out > K) return NTF_EINVAL;
    if (!fair_args_ok(cand_idx, n, K, group, n_experts, G, p, n_p)) return NTF_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return NTF_EHIP;
    PhaseClock clk;
    const size_t in = (size_t)n * K, out = (size_t)n * K_out;
    DevBuf di, dv, dg, dp, oi, ov, op, ot;
    if (!di.put(cand_idx, in * 4) || (out_val && !dv.put(cand_val, in * 4)) || !dg.put(group, (size_t)n_experts) || !dp.put(p, (size_t)n_p * G * 8) ||
        !oi.alloc(out * 4) || (out_val && !ov.alloc(out * 4)) || (out_pos && !op.alloc(out * 4)) || (out_tail && !ot.alloc((size_t)n * 4))) return NTF_ENOMEM;
    clk.lap(0);
    hipLaunchKernelGGL(k_fair_constsort, dim3((unsigned)((n + FAIR_ROWS - 1) / FAIR_ROWS)), dim3(64 * FAIR_ROWS), 0, 0, di.as<const int32_t>(),
                       out_val ? dv.as<const float>() : nullptr, n, (int)K, dg.as<const uint8_t>(), (int)G, dp.as<const double>(), n_p == 1 ? 0 : 1, (int)K_out,
                       oi.as<int32_t>(), out_val ? ov.as<float>() : nullptr, out_pos ? op.as<int32_t>() : nullptr, out_tail ? ot.as<int32_t>() : nullptr);
    if (hipGetLastError() != hipSuccess) return NTF_EHIP;
    clk.lap(1);
    if (hipMemcpy(out_idx, oi.p, out * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (out_val && hipMemcpy(out_val, ov.p, out * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (out_pos && hipMemcpy(out_pos, op.p, out * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (out_tail && hipMemcpy(out_tail, ot.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    clk.lap(2); clk.report("ntf_fair_constsort");
    return NTF_OK;
}

extern "C" int ntf_fair_infeasible(int device, const int32_t* idx, int64_t n, int32_t K, const uint8_t* group, int64_t n_experts, int32_t G, const double* p, int64_t n_p,
                                   const int32_t* cutoffs, int32_t n_cut, int32_t* out_index, int32_t* out_count) {
    FairCuts cut;
    if (!fair_cuts_ok(cutoffs, n_cut, K, &cut) || (!out_index && !out_count)) return NTF_EINVAL;
    if (!fair_args_ok(idx, n, K, group, n_experts, G, p, n_p)) return NTF_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return NTF_EHIP;
    PhaseClock clk;
    const size_t nb = (size_t)n * n_cut * 4;
    DevBuf di, dg, dp, oi, oc;
    if (!di.put(idx, (size_t)n * K * 4) || !dg.put(group, (size_t)n_experts) || !dp.put(p, (size_t)n_p * G * 8) || (out_index && !oi.alloc(nb)) ||
        (out_count && !oc.alloc(nb))) return NTF_ENOMEM;
    clk.lap(0);
    hipLaunchKernelGGL(k_fair_infeasible, dim3((unsigned)((n + FAIR_ROWS - 1) / FAIR_ROWS)), dim3(64 * FAIR_ROWS), 0, 0, di.as<const int32_t>(), n, (int)K,
                       dg.as<const uint8_t>(), (int)G, dp.as<const double>(), n_p == 1 ? 0 : 1, cut, out_index ? oi.as<int32_t>() : nullptr,
                       out_count ? oc.as<int32_t>() : nullptr);
    if (hipGetLastError() != hipSuccess) return NTF_EHIP;
    clk.lap(1);
    if (out_index && hipMemcpy(out_index, oi.p, nb, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    if (out_count && hipMemcpy(out_count, oc.p, nb, hipMemcpyDeviceToHost) != hipSuccess) return NTF_EHIP;
    clk.lap(2); clk.report("ntf_fair_infeasible");
    return NTF_OK;
}
