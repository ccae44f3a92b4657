// The [query group] x [row range] product over a resident padded table, once: k_sims is the tile loop of the cosine search (ntf_knn.hip, epilogue SimCosine:
// the dot scaled by the two reciprocal norms) and of the link decode (ntf_link.hip, epilogue SimLogit: the dot itself), with the workspace plan both walk by.
//   exact-f32 MFMA (v_mfma_f32_32x32x2_f32): the query chunk resident in LDS, the table streamed with 16-byte loads through a wave-private LDS stage that gives
//   the MFMA operand its [row][k] -> lane transpose.  The dot of (row, query) is one k-ordered fmaf chain from 0: its bits do not depend on the tile or the range.
#pragma once
#include "ntf_device.h"
#include "ntf_fused_common.h"
#include "ntf_host.h"

#include <algorithm>

namespace ntf {

constexpr int SIM_KC = 32;               // k-chunk: floats of a row staged at a time (one 128-B line a row); rows are padded to a multiple of it
constexpr int SIM_SLD = SIM_KC + 1;      // odd LDS row stride: the fragment reads (32 lanes = 32 rows, same k) hit 32 different banks
constexpr int SIM_WAVES = 8;             // waves a workgroup, 32 table rows each
constexpr int SIM_RB = SIM_WAVES * 32;   // table rows a workgroup takes at a time (the row unit of the workspace plan)
constexpr int SIM_QUNIT = 32;            // the query unit of the workspace plan
constexpr int SIM_MAX_GROUP = 1024;      // queries a group holds at most
constexpr int64_t SIM_MAX_RANGE = 262144;   // rows a range holds at most: a selection workgroup walks one (query, range) row of sims

struct SimArgs {
    const float *T, *rinv_t, *Q, *rinv_q;   // Q / rinv_q: the group's first query; the reciprocal norms are read by an epilogue with NORMS only
    float* S;                               // [group, ld] sims of the range
    int64_t r0, ld; int rr, nq, dp;         // the range [r0, r0 + rr), queries in the group, row stride
};

// what a finished dot becomes.  rq, rt: the reciprocal norms of the query and of the table row (NORMS), else 1
struct SimCosine {
    static constexpr bool NORMS = true;
    static __device__ __forceinline__ float apply(float dot, float rq, float rt) {
        float sim = (dot * rq) * rt;
        if (rq == 0.f || rt == 0.f || sim == 0.f) sim = 0.f;           // a norm below FLT_MIN scores 0 with everything; -0 is returned as +0
        return sim;
    }
};
struct SimLogit {
    static constexpr bool NORMS = false;
    static __device__ __forceinline__ float apply(float dot, float, float) { return dot == 0.f ? 0.f : dot; }      // -0 is returned as +0
};

// NQT 32-query tiles resident a workgroup (blockIdx.y picks the chunk of the group); blockIdx.x strides over the range's 256-row blocks.
// MFMA operands: A = queries (lane: query lane & 31, k = 2 s + (lane >> 5)), B = table rows (lane: row lane & 31, same k) - so the accumulator's lane axis is the
// table row and a store of one accumulator register is two 128-B runs of a query's sims row.  Step s of the chain takes k = 2 s then 2 s + 1: k-ordered from 0.
template <int NQT, class Epi>
__global__ __launch_bounds__(SIM_WAVES * 64) void k_sims(SimArgs a) {
    extern __shared__ float smem[];
    const int qld = a.dp + 1;
    float* Qs = smem;                                         // [NQT * 32][dp + 1]
    float* rqs = Qs + NQT * 32 * qld;                         // [NQT * 32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* stage = rqs + NQT * 32 + wave * (32 * SIM_SLD);    // [32][33], private to the wave
    const int q0 = blockIdx.y * (NQT * 32);
    for (int e = tid; e < NQT * 32 * a.dp; e += blockDim.x) {
        const int q = e / a.dp, k = e - q * a.dp;
        Qs[q * qld + k] = (q0 + q < a.nq) ? a.Q[(int64_t)(q0 + q) * a.dp + k] : 0.f;
    }
    if constexpr (Epi::NORMS)
        for (int q = tid; q < NQT * 32; q += blockDim.x) rqs[q] = (q0 + q < a.nq) ? a.rinv_q[q0 + q] : 0.f;
    __syncthreads();
    const int nkc = a.dp / SIM_KC, nrb = (a.rr + SIM_RB - 1) / SIM_RB;
    const int lrow = lane >> 3, lk = (lane & 7) * 4;          // staging: 8 lanes a row of the chunk, 8 rows an instruction
    const float* aq = Qs + (lane & 31) * qld + (lane >> 5);
    const float* bs = stage + (lane & 31) * SIM_SLD + (lane >> 5);
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const int w0 = rb * SIM_RB + wave * 32;               // the wave's first row inside the range
        if (w0 >= a.rr) continue;                             // (no workgroup barrier below)
        const float* Tw = a.T + (a.r0 + w0) * a.dp;
        float4 pre[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = j * 8 + lrow;
            pre[j] = (w0 + r < a.rr) ? *reinterpret_cast<const float4*>(Tw + (int64_t)r * a.dp + lk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        f32x16 acc[NQT];
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        for (int kc = 0; kc < nkc; ++kc) {
            __builtin_amdgcn_wave_barrier();                  // the previous chunk's fragment reads are issued before the stage is overwritten
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float* s = stage + (j * 8 + lrow) * SIM_SLD + lk;
                s[0] = pre[j].x; s[1] = pre[j].y; s[2] = pre[j].z; s[3] = pre[j].w;
            }
            __builtin_amdgcn_wave_barrier();
            if (kc + 1 < nkc) {                               // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = j * 8 + lrow;
                    pre[j] = (w0 + r < a.rr) ? *reinterpret_cast<const float4*>(Tw + (int64_t)r * a.dp + (kc + 1) * SIM_KC + lk) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            const float* ak = aq + kc * SIM_KC;
#pragma unroll 4
            for (int s = 0; s < SIM_KC / 2; ++s) {
                const float b = bs[2 * s];
#pragma unroll
                for (int t = 0; t < NQT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[t * 32 * qld + 2 * s], b, acc[t], 0, 0, 0);
            }
        }
        const int row = w0 + (lane & 31);
        if (row < a.rr) {
            float rt = 1.f;
            if constexpr (Epi::NORMS) rt = a.rinv_t[a.r0 + row];
            // register r of tile t is query 32 t + 8 (r >> 2) + 4 (lane >> 5) + (r & 3); group x range <= 2^28 floats, so the offsets are 32-bit
            int ldi = (int)a.ld;
            asm volatile("" : "+v"(ldi));       // kept in a vector register: 64 scalar multiples of it, one per store, do not fit the scalar file
            int ql = 4 * (lane >> 5), off = (q0 + ql) * ldi + row;
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float rq = 1.f;
                    if constexpr (Epi::NORMS) rq = rqs[ql];   // (a query past the group's last has rq = 0: its row of the workspace exists, the workspace holds whole chunks)
                    a.S[off] = Epi::apply(acc[t][r], rq, rt);
                    const int step = (r & 3) == 3 ? 5 : 1;
                    ql += step; off += step * ldi;
                }
        }
    }
}

inline size_t sims_lds(int nqt, int dp) { return ((size_t)nqt * 32 * (dp + 1) + (size_t)nqt * 32 + (size_t)SIM_WAVES * 32 * SIM_SLD) * sizeof(float); }

// The plan of a call (include/opentf_amd.h, ntf_knn_query): n queries in groups of G = 32 g, N rows in ranges of R = 256 r, a workspace of Gw x R floats within
// the budget wsb (>= the 32 KiB unit, checked by the caller).
struct SimsPlan {
    int64_t G, Gw, R; int nqt_max;
    SimsPlan(int64_t wsb, int64_t n, int64_t N, int64_t dp) {
        const int64_t g = std::min<int64_t>(std::max<int64_t>(wsb / ((int64_t)8 << 20), 1), std::min<int64_t>(SIM_MAX_GROUP / SIM_QUNIT, (n + SIM_QUNIT - 1) / SIM_QUNIT));
        G = g * SIM_QUNIT;
        // query tiles resident a workgroup of the sims kernel: 4 (dp <= 128: a 4-tile image of wider rows does not fit LDS beside the stages), 2 or 1, as many as a full group
        // fills.  The workspace holds whole chunks of 32 nqt rows (gw = g rounded up to a multiple of nqt), so every query slot a workgroup stores to has its row there
        nqt_max = (std::min(G, n) > 64 && dp <= 128) ? 4 : (std::min(G, n) > 32) ? 2 : 1;
        Gw = (g + nqt_max - 1) / nqt_max * nqt_max * SIM_QUNIT;
        R = std::min<int64_t>(std::min<int64_t>(wsb / (Gw * SIM_RB * 4), SIM_MAX_RANGE / SIM_RB), (N + SIM_RB - 1) / SIM_RB) * SIM_RB;
    }
};

// the sims of the ng queries at Q (and rinv_q) against the rows [r0, r0 + rr) of T into ws [Gw, ld]
template <class Epi>
void launch_sims(hipStream_t st, int n_cu, int nqt_max, const float* T, const float* rinv_t, const float* Q, const float* rinv_q, float* ws,
                 int64_t r0, int64_t ld, int rr, int ng, int dp) {
    const int nqt = std::min(nqt_max, ng > 64 ? 4 : ng > 32 ? 2 : 1);      // a shorter last group takes a shorter chunk (1, 2 and 4 divide nqt_max)
    const size_t lds = sims_lds(nqt, dp);
    const int per_cu = std::max<int>(1, (int)((160u << 10) / lds));
    SimArgs a;
    a.T = T; a.rinv_t = rinv_t; a.Q = Q; a.rinv_q = rinv_q; a.S = ws; a.r0 = r0; a.ld = ld; a.rr = rr; a.nq = ng; a.dp = dp;
    const dim3 grid((unsigned)std::min<int64_t>((rr + SIM_RB - 1) / SIM_RB, (int64_t)n_cu * per_cu), (unsigned)((ng + nqt * 32 - 1) / (nqt * 32)));
    with_value<1, 2, 4>(nqt, [&](auto q) { launch_lds(k_sims<decltype(q)::value, Epi>, grid, dim3(SIM_WAVES * 64), lds, st, a); });
}

}  // namespace ntf
