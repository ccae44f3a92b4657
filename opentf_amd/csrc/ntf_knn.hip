// Batched cosine nearest-neighbour search over a resident [n_rows, d] f32 table on the MI355X (include/opentf_amd.h ntf_knn_*): what
// KeyedVectors.most_similar (opentf_amd/mdl/emb/d2v.py, the second half of the reference's infer_d2v, src/mdl/emb/d2v.py:96-98) does one query at a time on the host.
//   k_knn_norms   reciprocal row norms (once per table at create, once per call for the queries)
//   k_sims        (ntf_sims.h, shared with the link decode; the cosine epilogue) sims of a query group against a row range into the workspace, exact-f32 MFMA
//   k_knn_select  per (query, range): the topn largest of the range by (sim desc, id asc), merged into the query's running list by the same 64-bit composite
//   k_knn_finish  running lists -> ids and sims
// [n, n_rows] is never formed: the workspace holds [query group, row range] and is sized by the caller's budget alone.
#include "../../include/opentf_amd.h"
#include "ntf_device.h"
#include "ntf_fused_common.h"
#include "ntf_host.h"
#include "ntf_select.h"
#include "ntf_sims.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

using namespace ntf;

struct ntf_knn {
    int device = 0, n_cu = 0; hipStream_t st = nullptr;
    int64_t n_rows = 0; int d = 0, dp = 0;        // dp: the device row stride, d rounded up to the 32-float k-chunk; the columns past d are zero
    float *table = nullptr, *rinv = nullptr;      // [n_rows, dp], [n_rows]
    int* flag = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the last call's queries [n, dp], their reciprocal norms, exclusions, results [n, topn] and running lists [group, topn]; the sims workspace; grown on demand
    float *q = nullptr, *q_rinv = nullptr, *o_sims = nullptr, *ws = nullptr; int32_t *q_excl = nullptr, *o_idx = nullptr; unsigned long long* run = nullptr;
    int64_t q_cap = 0, qr_cap = 0, qe_cap = 0, oi_cap = 0, os_cap = 0, run_cap = 0, ws_cap = 0;
    std::string err;
};
static thread_local std::string g_knn_create_error;

extern "C" const char* ntf_knn_last_error(const ntf_knn* h) { return h ? h->err.c_str() : g_knn_create_error.c_str(); }

namespace {
// ---- reciprocal norms: n2 = one k-ordered fmaf chain from 0, rinv = 1 / sqrt(n2) (IEEE sqrt, IEEE divide), 0 when n2 < FLT_MIN.  flag |= 1: a non-finite value, |= 2: n2 overflows.
// One thread a row keeps the chain sequential; the rows come through LDS in 32-float chunks so that the global reads are whole 128-B lines (8 lanes a row, 16 bytes each)
// and the chain's reads - 256 rows at the same k, odd stride - hit different banks.  The pad columns are zeros: fmaf(0, 0, n2) = n2.
__global__ __launch_bounds__(256) void k_knn_norms(const float* __restrict__ T, int64_t n, int d, int dp, float* __restrict__ rinv, int* __restrict__ flag) {
    __shared__ float tile[256 * SIM_SLD];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + tid;
    float n2 = 0.f; bool bad = false;
    for (int k0 = 0; k0 < dp; k0 += SIM_KC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = j * 32 + (tid >> 3), k = (tid & 7) * 4;
            const float4 v = (i0 + r < n) ? *reinterpret_cast<const float4*>(T + (i0 + r) * dp + k0 + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            float* s = tile + r * SIM_SLD + k;
            s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
        }
        __syncthreads();
        for (int k = 0; k < SIM_KC; ++k) { const float v = tile[tid * SIM_SLD + k]; bad |= !(fabsf(v) <= FLT_MAX); n2 = fmaf(v, v, n2); }
    }
    if (i >= n) return;
    if (bad) atomicOr(flag, 1);
    else if (!(n2 <= FLT_MAX)) atomicOr(flag, 2);
    rinv[i] = n2 < FLT_MIN ? 0.f : 1.f / sqrtf(n2);
}

// One workgroup per query of the group: the K largest of its sims row S[q, 0 .. M) by the composite (key << 32) | (0x7fffffff - id), id = r0 + column, the
// excluded id left out (the selection of ntf_select.h on signed values), then merged with the query's running list (first = 0) by the same composite: a total
// order, so the merge is exact and the order of the ranges free.  A composite of 0 is an empty slot.
__global__ __launch_bounds__(1024) void k_knn_select(const float* __restrict__ S, int64_t ld, int M, int64_t r0, int K, const int32_t* __restrict__ excl,
                                                     unsigned long long* __restrict__ run, int first) {
    __shared__ SelShared sh;
    const int64_t i = blockIdx.x;
    const int64_t ex = excl ? (int64_t)excl[i] - r0 : -1;     // the excluded column of this range, if it lies in it
    const int n2 = select_topk_row<SignedKey, true>(sh, S + i * ld, M, K, r0, ex);
    merge_running(sh, n2, K, run + i * K, first);
}

__global__ void k_knn_finish(const unsigned long long* __restrict__ run, int64_t n, int32_t* __restrict__ idx, float* __restrict__ sims) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const unsigned long long c = run[e];
    idx[e] = c ? 0x7fffffff - (int32_t)(c & 0xffffffffu) : -1;
    sims[e] = c ? SignedKey::value((unsigned)(c >> 32)) : -INFINITY;
}

}  // namespace

extern "C" void ntf_knn_destroy(ntf_knn* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    for (void* p : {(void*)h->table, (void*)h->rinv, (void*)h->flag, (void*)h->q, (void*)h->q_rinv, (void*)h->q_excl, (void*)h->o_idx, (void*)h->o_sims, (void*)h->run, (void*)h->ws})
        if (p) hipFree(p);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

extern "C" int ntf_knn_create(int device, const float* table, int64_t n_rows, int32_t d, ntf_knn** out) {
    if (!out) { g_knn_create_error = "knn: out is NULL"; return NTF_EINVAL; }
    *out = nullptr;
    if (!table || n_rows < 1 || n_rows > 0x7fffffffll || d < 1 || d > 256) { g_knn_create_error = "knn: need a table, 1 <= n_rows <= 2^31 - 1 and 1 <= d <= 256"; return NTF_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_knn_create_error = "no HIP device: the search has no CPU fallback"; return NTF_EHIP; }
    if (device < 0 || device >= ndev) { g_knn_create_error = "no such HIP device (there is no CPU fallback)"; return NTF_EHIP; }
    hipSetDevice(device);
    ntf_knn* h = new ntf_knn();
    h->device = device; h->n_rows = n_rows; h->d = d; h->dp = (d + SIM_KC - 1) / SIM_KC * SIM_KC;
    const int64_t dp = h->dp;
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->n_cu < 1) h->n_cu = 256;
    if (hipStreamCreate(&h->st) != hipSuccess) { g_knn_create_error = "hipStreamCreate failed"; delete h; return NTF_EHIP; }
    int rc = NTF_OK;
    auto A = [&](int r) { if (rc == NTF_OK) rc = r; };
    A(dev_alloc(h, &h->table, n_rows * dp)); A(dev_alloc(h, &h->rinv, n_rows)); A(dev_alloc(h, &h->flag, 1));
    if (rc != NTF_OK) { g_knn_create_error = h->err; ntf_knn_destroy(h); return rc; }
    bool ok = true;
    auto H = [&](hipError_t s) { ok = ok && s == hipSuccess; };
    H(upload_padded(h->table, dp, table, d, n_rows));
    H(hipMemsetAsync(h->flag, 0, 4, h->st));
    hipLaunchKernelGGL(k_knn_norms, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, h->st, h->table, n_rows, (int)d, (int)dp, h->rinv, h->flag);
    H(hipGetLastError());
    int flag = 0;
    H(hipMemcpyAsync(&flag, h->flag, 4, hipMemcpyDeviceToHost, h->st));
    H(hipStreamSynchronize(h->st));
    if (!ok) { g_knn_create_error = "knn: device initialisation failed"; ntf_knn_destroy(h); return NTF_EHIP; }
    if (flag) {
        g_knn_create_error = (flag & 1) ? "knn: a table value is not finite" : "knn: the f32 squared norm of a table row overflows";
        ntf_knn_destroy(h); return NTF_EINVAL;
    }
    *out = h;
    return NTF_OK;
}

extern "C" int ntf_knn_query(ntf_knn* h, const float* queries, int64_t n, int32_t topn, const int64_t* exclude, int64_t workspace_bytes,
                             int32_t* out_idx, float* out_sims, double* device_ms) {
    if (!h) { g_knn_create_error = "knn query: the handle is NULL"; return NTF_EINVAL; }
    if (!queries || !out_idx || !out_sims) FAIL(h, NTF_EINVAL, "knn query: queries, out_idx and out_sims are required");
    if (n < 1) FAIL(h, NTF_EINVAL, "knn query: n < 1");
    if (topn < 1 || topn > SEL_MAX) FAIL(h, NTF_EINVAL, "knn query: topn outside 1..2048");
    if (workspace_bytes < 0) FAIL(h, NTF_EINVAL, "knn query: workspace_bytes < 0");
    const int64_t wsb = workspace_bytes ? workspace_bytes : NTF_KNN_WORKSPACE_BYTES;
    const int64_t unit = (int64_t)SIM_QUNIT * SIM_RB * 4;
    if (wsb < unit) FAIL(h, NTF_EINVAL, "knn query: workspace_bytes below one unit of work (32 queries x 256 rows of f32 sims = 32 KiB)");
    const int d = h->d; const int64_t dp = h->dp, N = h->n_rows;
    for (int64_t e = 0; e < n * d; ++e) if (!std::isfinite(queries[e])) FAIL(h, NTF_EINVAL, "knn query: a query value is not finite");
    std::vector<int32_t> excl;
    if (exclude) {
        excl.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) { if (exclude[i] < -1 || exclude[i] >= N) FAIL(h, NTF_EINVAL, "knn query: an exclude value outside [-1, n_rows)"); excl[(size_t)i] = (int32_t)exclude[i]; }
    }
    // the plan (header): a group of 32 g queries, a range of 256 r rows, group x range x 4 bytes <= the budget
    const SimsPlan plan(wsb, n, N, dp);
    const int64_t G = plan.G, Gw = plan.Gw, R = plan.R;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->st));
    {
        int rc = NTF_OK;
        auto A = [&](int r) { if (rc == NTF_OK) rc = r; };
        A(dev_grow(h, &h->q, &h->q_cap, n * dp)); A(dev_grow(h, &h->q_rinv, &h->qr_cap, n)); A(dev_grow(h, &h->q_excl, &h->qe_cap, n));
        A(dev_grow(h, &h->o_idx, &h->oi_cap, n * topn)); A(dev_grow(h, &h->o_sims, &h->os_cap, n * topn)); A(dev_grow(h, &h->run, &h->run_cap, G * topn)); if (h->ws_cap != Gw * R) { if (h->ws) hipFree(h->ws); h->ws = nullptr; h->ws_cap = 0; A(dev_grow(h, &h->ws, &h->ws_cap, Gw * R)); }      // never above this call's budget
        if (rc != NTF_OK) return rc;
    }
    HIPCHK(h, upload_padded(h->q, dp, queries, d, n));
    if (exclude) HIPCHK(h, hipMemcpy(h->q_excl, excl.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemsetAsync(h->flag, 0, 4, h->st));
    hipLaunchKernelGGL(k_knn_norms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->q, n, d, (int)dp, h->q_rinv, h->flag);
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, h->flag, 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (flag) FAIL(h, NTF_EINVAL, "knn query: the f32 squared norm of a query overflows");
    const int rc = timed_launch(h, device_ms, "knn", [&] {
        for (int64_t g0 = 0; g0 < n; g0 += G) {
            const int ng = (int)std::min<int64_t>(G, n - g0);
            for (int64_t r0 = 0; r0 < N; r0 += R) {
                const int rr = (int)std::min<int64_t>(R, N - r0);
                launch_sims<SimCosine>(h->st, h->n_cu, plan.nqt_max, h->table, h->rinv, h->q + g0 * dp, h->q_rinv + g0, h->ws, r0, R, rr, ng, (int)dp);
                hipLaunchKernelGGL(k_knn_select, dim3((unsigned)ng), dim3(1024), 0, h->st, h->ws, R, rr, r0, (int)topn, exclude ? h->q_excl + g0 : nullptr, h->run, r0 == 0 ? 1 : 0);
            }
            const int64_t ne = (int64_t)ng * topn;
            hipLaunchKernelGGL(k_knn_finish, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, h->st, h->run, ne, h->o_idx + g0 * topn, h->o_sims + g0 * topn);
        }
    });
    if (rc != NTF_OK) return rc;
    HIPCHK(h, hipMemcpy(out_idx, h->o_idx, (size_t)n * topn * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(out_sims, h->o_sims, (size_t)n * topn * 4, hipMemcpyDeviceToHost));
    return NTF_OK;
}
