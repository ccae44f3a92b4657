// Link decode over a resident [n_rows, d] f32 node-embedding table on the MI355X (include/opentf_amd_link.h ntf_link_*): the logit <E[query], E[candidate]> and
// its sigmoid for every row of a candidate block, ranked - the `test` of the reference's random-walk Gnn (src/mdl/emb/gnn.py:512-545) for a batch of teams.
//   k_link_finite   a non-finite table value raises the flag (once, at create)
//   k_link_gather   query form `rows`: table rows -> the [n, dp] query buffer (form `pooled`: k_gather_pool through launch_gather_meanpool, the same buffer)
//   k_sims          (ntf_sims.h, shared with the cosine search; the logit epilogue) logits of a query group against a candidate range into the workspace
//   k_link_select   per (query, range): the K largest of the range by (logit desc, id asc), merged into the query's running list by the same 64-bit composite
//   k_link_finish   running lists -> ids, logits and link_sigmoid of them
//   k_link_prob     dense entry: link_sigmoid over the workspace rows in place, between the copy of the logits and the copy of the probabilities
// [n, C] is never formed on the device: the workspace holds [query group, candidate range] and is sized by the caller's budget alone.
#include "../../include/opentf_amd_link.h"
#include "ntf_device.h"
#include "ntf_host.h"
#include "ntf_kernels.h"
#include "ntf_select.h"
#include "ntf_sims.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

using namespace ntf;

struct ntf_link {
    int device = 0, n_cu = 0; hipStream_t st = nullptr;
    int64_t n_rows = 0, cand_lo = 0, C = 0; int d = 0, dp = 0;      // dp: the device row stride, d rounded up to the 32-float k-chunk; the columns past d are zero
    float* table = nullptr;                                         // [n_rows, dp]
    int* flag = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the last call's query rows / CSR, queries [n, dp], results [n, K] and running lists [group, K]; the logit workspace; grown on demand
    int64_t *q_rows = nullptr, *q_ptr = nullptr; int32_t *q_items = nullptr, *o_idx = nullptr; float *q = nullptr, *o_logit = nullptr, *o_prob = nullptr, *ws = nullptr;
    unsigned long long* run = nullptr;
    int64_t qrow_cap = 0, qptr_cap = 0, qit_cap = 0, q_cap = 0, oi_cap = 0, ol_cap = 0, op_cap = 0, run_cap = 0, ws_cap = 0;
    std::string err;
};
static thread_local std::string g_link_create_error;

extern "C" const char* ntf_link_last_error(const ntf_link* h) { return h ? h->err.c_str() : g_link_create_error.c_str(); }

namespace {
// the ONE probability of a logit (header): every output path calls it
__device__ __forceinline__ float link_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(256) void k_link_finite(const float4* __restrict__ T, int64_t n4, int* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const float4 v = T[e];
    if (!(fabsf(v.x) <= FLT_MAX) || !(fabsf(v.y) <= FLT_MAX) || !(fabsf(v.z) <= FLT_MAX) || !(fabsf(v.w) <= FLT_MAX)) atomicOr(flag, 1);
}

// Q[i, :] = T[rows[i], :], dp4 = dp / 4 16-byte pieces a row (the pad columns come along: zeros)
__global__ __launch_bounds__(256) void k_link_gather(const float4* __restrict__ T, const int64_t* __restrict__ rows, int64_t n, int dp4, float4* __restrict__ Q) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * dp4) return;
    const int64_t i = e / dp4; const int c = (int)(e - i * dp4);
    Q[e] = T[rows[i] * dp4 + c];
}

// One workgroup per query of the group: the K largest of its logit row S[q, 0 .. M) by the composite (key << 32) | (0x7fffffff - id), id = r0 + column: the
// candidate id, local to the block (the selection of ntf_select.h on signed values), then merged with the query's running list (first = 0).
__global__ __launch_bounds__(1024) void k_link_select(const float* __restrict__ S, int64_t ld, int M, int64_t r0, int K, unsigned long long* __restrict__ run, int first) {
    __shared__ SelShared sh;
    const int64_t i = blockIdx.x;
    const int n2 = select_topk_row<SignedKey, false>(sh, S + i * ld, M, K, r0, -1);
    merge_running(sh, n2, K, run + i * K, first);
}

__global__ void k_link_finish(const unsigned long long* __restrict__ run, int64_t n, int32_t* __restrict__ idx, float* __restrict__ logit, float* __restrict__ prob) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const unsigned long long c = run[e];
    const float x = c ? SignedKey::value((unsigned)(c >> 32)) : -INFINITY;
    idx[e] = c ? 0x7fffffff - (int32_t)(c & 0xffffffffu) : -1;
    if (logit) logit[e] = x;
    if (prob) prob[e] = c ? link_sigmoid(x) : 0.f;
}

// S[i, 0 .. rr) <- link_sigmoid, blockIdx.y = the query of the group
__global__ __launch_bounds__(256) void k_link_prob(float* __restrict__ S, int64_t ld, int rr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= rr) return;
    float* p = S + (int64_t)blockIdx.y * ld + c;
    *p = link_sigmoid(*p);
}

// what both entries check and plan: the arguments they share, then the plan of the call
struct LinkCall { int64_t wsb = 0, nnz = 0; std::vector<int32_t> items; };

int link_check(ntf_link* h, const char* who, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const int64_t* q_items, int64_t workspace_bytes, LinkCall* c) {
    const std::string w = who;
    const bool rows = q_rows != nullptr, pooled = q_ptr != nullptr || q_items != nullptr;
    if (rows == pooled) FAIL(h, NTF_EINVAL, w + ": exactly one query form is required, q_rows or q_ptr + q_items");
    if (pooled && (!q_ptr || !q_items)) FAIL(h, NTF_EINVAL, w + ": the pooled form needs both q_ptr and q_items");
    if (n < 1) FAIL(h, NTF_EINVAL, w + ": n < 1");
    if (workspace_bytes < 0) FAIL(h, NTF_EINVAL, w + ": workspace_bytes < 0");
    c->wsb = workspace_bytes ? workspace_bytes : NTF_KNN_WORKSPACE_BYTES;
    if (c->wsb < (int64_t)SIM_QUNIT * SIM_RB * 4) FAIL(h, NTF_EINVAL, w + ": workspace_bytes below one unit of work (32 queries x 256 rows of f32 logits = 32 KiB)");
    const int64_t N = h->n_rows;
    if (rows) {
        for (int64_t i = 0; i < n; ++i) if (q_rows[i] < 0 || q_rows[i] >= N) FAIL(h, NTF_EINVAL, w + ": a query row outside [0, n_rows)");
        return NTF_OK;
    }
    if (q_ptr[0] != 0) FAIL(h, NTF_EINVAL, w + ": q_ptr[0] != 0");
    for (int64_t i = 0; i < n; ++i) {
        if (q_ptr[i + 1] < q_ptr[i]) FAIL(h, NTF_EINVAL, w + ": q_ptr is not monotone");
        if (q_ptr[i + 1] == q_ptr[i]) FAIL(h, NTF_EINVAL, w + ": an empty pooled row (its mean is 0 / 0)");
    }
    c->nnz = q_ptr[n];
    c->items.resize((size_t)c->nnz);
    for (int64_t e = 0; e < c->nnz; ++e) {
        if (q_items[e] < 0 || q_items[e] >= N) FAIL(h, NTF_EINVAL, w + ": a pooled item outside [0, n_rows)");
        c->items[(size_t)e] = (int32_t)q_items[e];
    }
    return NTF_OK;
}

// the query buffer h->q [n, dp] of either form, queued on the stream
int link_queries(ntf_link* h, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const LinkCall& c) {
    const int64_t dp = h->dp;
    int rc = dev_grow(h, &h->q, &h->q_cap, n * dp);
    if (rc != NTF_OK) return rc;
    if (q_rows) {
        if ((rc = dev_grow(h, &h->q_rows, &h->qrow_cap, n)) != NTF_OK) return rc;
        HIPCHK(h, hipMemcpy(h->q_rows, q_rows, (size_t)n * 8, hipMemcpyHostToDevice));
        const int64_t ne = n * (dp / 4);
        hipLaunchKernelGGL(k_link_gather, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, h->st, reinterpret_cast<const float4*>(h->table), h->q_rows, n, (int)(dp / 4),
                           reinterpret_cast<float4*>(h->q));
    } else {
        if ((rc = dev_grow(h, &h->q_ptr, &h->qptr_cap, n + 1)) != NTF_OK) return rc;
        if ((rc = dev_grow(h, &h->q_items, &h->qit_cap, c.nnz)) != NTF_OK) return rc;
        HIPCHK(h, hipMemcpy(h->q_ptr, q_ptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->q_items, c.items.data(), (size_t)c.nnz * 4, hipMemcpyHostToDevice));
        // the padded table is a table of width dp: the pad columns pool to 0 / count = +0, the others are k_gather_pool's own bits
        launch_gather_meanpool(h->st, h->q_ptr, h->q_items, h->table, nullptr, n, (int)dp, 1, h->q);
    }
    return NTF_OK;
}

int link_workspace(ntf_link* h, const SimsPlan& plan) {
    if (h->ws_cap == plan.Gw * plan.R) return NTF_OK;
    if (h->ws) hipFree(h->ws);
    h->ws = nullptr; h->ws_cap = 0;      // never above this call's budget
    return dev_grow(h, &h->ws, &h->ws_cap, plan.Gw * plan.R);
}

int link_launch_error(ntf_link* h) {
    const hipError_t s = hipGetLastError();
    if (s != hipSuccess) FAIL(h, NTF_EHIP, std::string("link kernel launch: ") + hipGetErrorString(s));
    return NTF_OK;
}

int link_clock_start(ntf_link* h, double* device_ms) {
    if (!device_ms) return NTF_OK;
    if (!h->ev0) { HIPCHK(h, hipEventCreate(&h->ev0)); HIPCHK(h, hipEventCreate(&h->ev1)); }
    HIPCHK(h, hipEventRecord(h->ev0, h->st));
    return NTF_OK;
}
int link_clock_stop(ntf_link* h, double* device_ms) {
    if (device_ms) HIPCHK(h, hipEventRecord(h->ev1, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (device_ms) { float ms = 0.f; HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1)); *device_ms = ms; }
    return NTF_OK;
}
}  // namespace

extern "C" void ntf_link_destroy(ntf_link* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    for (void* p : {(void*)h->table, (void*)h->flag, (void*)h->q_rows, (void*)h->q_ptr, (void*)h->q_items, (void*)h->q, (void*)h->o_idx, (void*)h->o_logit, (void*)h->o_prob,
                    (void*)h->run, (void*)h->ws})
        if (p) hipFree(p);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

extern "C" int ntf_link_create(int device, const float* table, int64_t n_rows, int32_t d, int64_t cand_lo, int64_t cand_hi, ntf_link** out) {
    if (!out) { g_link_create_error = "link: out is NULL"; return NTF_EINVAL; }
    *out = nullptr;
    if (!table || n_rows < 1 || n_rows > 0x7fffffffll || d < 1 || d > 256) { g_link_create_error = "link: need a table, 1 <= n_rows <= 2^31 - 1 and 1 <= d <= 256"; return NTF_EINVAL; }
    if (cand_lo < 0 || cand_hi > n_rows || cand_hi - cand_lo < 1) { g_link_create_error = "link: the candidate block needs 0 <= cand_lo < cand_hi <= n_rows"; return NTF_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_link_create_error = "no HIP device: the link decode has no CPU fallback"; return NTF_EHIP; }
    if (device < 0 || device >= ndev) { g_link_create_error = "no such HIP device (there is no CPU fallback)"; return NTF_EHIP; }
    hipSetDevice(device);
    ntf_link* h = new ntf_link();
    h->device = device; h->n_rows = n_rows; h->d = d; h->dp = (d + SIM_KC - 1) / SIM_KC * SIM_KC; h->cand_lo = cand_lo; h->C = cand_hi - cand_lo;
    const int64_t dp = h->dp;
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->n_cu < 1) h->n_cu = 256;
    if (hipStreamCreate(&h->st) != hipSuccess) { g_link_create_error = "hipStreamCreate failed"; delete h; return NTF_EHIP; }
    int rc = dev_alloc(h, &h->table, n_rows * dp);
    if (rc == NTF_OK) rc = dev_alloc(h, &h->flag, 1);
    if (rc != NTF_OK) { g_link_create_error = h->err; ntf_link_destroy(h); return rc; }
    bool ok = true;
    auto H = [&](hipError_t s) { ok = ok && s == hipSuccess; };
    H(upload_padded(h->table, dp, table, d, n_rows));
    H(hipMemsetAsync(h->flag, 0, 4, h->st));
    const int64_t n4 = n_rows * dp / 4;
    hipLaunchKernelGGL(k_link_finite, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, h->st, reinterpret_cast<const float4*>(h->table), n4, h->flag);
    H(hipGetLastError());
    int flag = 0;
    H(hipMemcpyAsync(&flag, h->flag, 4, hipMemcpyDeviceToHost, h->st));
    H(hipStreamSynchronize(h->st));
    if (!ok) { g_link_create_error = "link: device initialisation failed"; ntf_link_destroy(h); return NTF_EHIP; }
    if (flag) { g_link_create_error = "link: a table value is not finite"; ntf_link_destroy(h); return NTF_EINVAL; }
    *out = h;
    return NTF_OK;
}

extern "C" int ntf_link_topk(ntf_link* h, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const int64_t* q_items, int32_t K, int64_t workspace_bytes,
                             int32_t* out_idx, float* out_logit, float* out_prob, double* device_ms) {
    if (!h) { g_link_create_error = "link topk: the handle is NULL"; return NTF_EINVAL; }
    if (!out_idx) FAIL(h, NTF_EINVAL, "link topk: out_idx is required");
    if (K < 1 || K > SEL_MAX) FAIL(h, NTF_EINVAL, "link topk: K outside 1..2048");
    LinkCall c;
    int rc = link_check(h, "link topk", n, q_rows, q_ptr, q_items, workspace_bytes, &c);
    if (rc != NTF_OK) return rc;
    const int64_t dp = h->dp, C = h->C;
    const SimsPlan plan(c.wsb, n, C, dp);
    const int64_t G = plan.G, R = plan.R;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->st));
    {
        auto A = [&](int r) { if (rc == NTF_OK) rc = r; };
        A(dev_grow(h, &h->o_idx, &h->oi_cap, n * K)); A(dev_grow(h, &h->run, &h->run_cap, G * K)); A(link_workspace(h, plan));
        if (out_logit) A(dev_grow(h, &h->o_logit, &h->ol_cap, n * K));
        if (out_prob) A(dev_grow(h, &h->o_prob, &h->op_cap, n * K));
        if (rc != NTF_OK) return rc;
    }
    if ((rc = link_clock_start(h, device_ms)) != NTF_OK) return rc;
    if ((rc = link_queries(h, n, q_rows, q_ptr, c)) != NTF_OK) return rc;
    const float* cand = h->table + h->cand_lo * dp;
    for (int64_t g0 = 0; g0 < n; g0 += G) {
        const int ng = (int)std::min<int64_t>(G, n - g0);
        for (int64_t r0 = 0; r0 < C; r0 += R) {
            const int rr = (int)std::min<int64_t>(R, C - r0);
            launch_sims<SimLogit>(h->st, h->n_cu, plan.nqt_max, cand, nullptr, h->q + g0 * dp, nullptr, h->ws, r0, R, rr, ng, (int)dp);
            hipLaunchKernelGGL(k_link_select, dim3((unsigned)ng), dim3(1024), 0, h->st, h->ws, R, rr, r0, (int)K, h->run, r0 == 0 ? 1 : 0);
        }
        const int64_t ne = (int64_t)ng * K;
        hipLaunchKernelGGL(k_link_finish, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, h->st, h->run, ne, h->o_idx + g0 * K,
                           out_logit ? h->o_logit + g0 * K : nullptr, out_prob ? h->o_prob + g0 * K : nullptr);
        if ((rc = link_launch_error(h)) != NTF_OK) return rc;
    }
    if ((rc = link_clock_stop(h, device_ms)) != NTF_OK) return rc;
    HIPCHK(h, hipMemcpy(out_idx, h->o_idx, (size_t)n * K * 4, hipMemcpyDeviceToHost));
    if (out_logit) HIPCHK(h, hipMemcpy(out_logit, h->o_logit, (size_t)n * K * 4, hipMemcpyDeviceToHost));
    if (out_prob) HIPCHK(h, hipMemcpy(out_prob, h->o_prob, (size_t)n * K * 4, hipMemcpyDeviceToHost));
    return NTF_OK;
}

extern "C" int ntf_link_dense(ntf_link* h, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const int64_t* q_items, int64_t workspace_bytes,
                              float* out_logit, float* out_prob, double* device_ms) {
    if (!h) { g_link_create_error = "link dense: the handle is NULL"; return NTF_EINVAL; }
    if (!out_logit && !out_prob) FAIL(h, NTF_EINVAL, "link dense: out_logit or out_prob is required");
    LinkCall c;
    int rc = link_check(h, "link dense", n, q_rows, q_ptr, q_items, workspace_bytes, &c);
    if (rc != NTF_OK) return rc;
    const int64_t dp = h->dp, C = h->C;
    const SimsPlan plan(c.wsb, n, C, dp);
    const int64_t G = plan.G, R = plan.R;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if ((rc = link_workspace(h, plan)) != NTF_OK) return rc;
    if ((rc = link_clock_start(h, device_ms)) != NTF_OK) return rc;
    if ((rc = link_queries(h, n, q_rows, q_ptr, c)) != NTF_OK) return rc;
    const float* cand = h->table + h->cand_lo * dp;
    for (int64_t g0 = 0; g0 < n; g0 += G) {
        const int ng = (int)std::min<int64_t>(G, n - g0);
        for (int64_t r0 = 0; r0 < C; r0 += R) {
            const int rr = (int)std::min<int64_t>(R, C - r0);
            launch_sims<SimLogit>(h->st, h->n_cu, plan.nqt_max, cand, nullptr, h->q + g0 * dp, nullptr, h->ws, r0, R, rr, ng, (int)dp);
            if ((rc = link_launch_error(h)) != NTF_OK) return rc;
            // the group's rows of the range, out of the workspace (row stride R) into [n, C]: the logits, then the same rows as probabilities
            if (out_logit) HIPCHK(h, hipMemcpy2DAsync(out_logit + g0 * C + r0, (size_t)C * 4, h->ws, (size_t)R * 4, (size_t)rr * 4, (size_t)ng, hipMemcpyDeviceToHost, h->st));
            if (out_prob) {
                hipLaunchKernelGGL(k_link_prob, dim3((unsigned)((rr + 255) / 256), (unsigned)ng), dim3(256), 0, h->st, h->ws, R, rr);
                if ((rc = link_launch_error(h)) != NTF_OK) return rc;
                HIPCHK(h, hipMemcpy2DAsync(out_prob + g0 * C + r0, (size_t)C * 4, h->ws, (size_t)R * 4, (size_t)rr * 4, (size_t)ng, hipMemcpyDeviceToHost, h->st));
            }
        }
    }
    return link_clock_stop(h, device_ms);
}
