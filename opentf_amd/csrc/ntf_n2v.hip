// node2vec skill-embedding producer on the MI355X: the table E [S, d] that the team2vec gather (k_gather_pool) consumes.
// Replaces the node2vec branch of the reference, src/mdl/emb/gnn.py:153-168 (torch_geometric.nn.Node2Vec, pinned 2.6.1 in requirements.txt:51,
// not installed here: its published algorithm is restated in oracle/n2v_oracle.py) and its training loop _train_rw, gnn.py:401-453:
//   loader  : per batch of start nodes, `walks_per_node` random walks (uniform at p = q = 1, else biased: ntf_n2v_set_walk_bias) of `walk_length` nodes, cut into windows of
//             `context_size`; negatives = the same start nodes followed by uniformly random nodes
//   loss    : -mean log(sigmoid(<e_start, e_rest>) + 1e-15) over positive pairs  - mean log(1 - sigmoid(.) + 1e-15) over negative pairs
//   update  : torch.optim.Adam on the dense embedding matrix (every row moves every step through its moments); opt-in (ntf_n2v_set_optimizer) torch.optim.SparseAdam
//             over the rows the batch names: k_n2v_touch -> k_n2v_compact -> k_n2v_adam_rows
//             opt-in too (ntf_n2v_set_lazy) LAZY dense Adam: dense Adam's table bit for bit, only the rows a batch names written - k_n2v_touch -> k_n2v_compact<false> ->
//             k_n2v_catchup_rows before the pairs, k_n2v_catchup_rows<NV, true> after them, k_n2v_catchup_all where a reader wants the whole table
// One training step (ntf_n2v_train_batch) for the three of them, every stage written once: the checks; the WINDOWS (make_windows: walks, negatives, both window
// launches - or upload_windows for injected rows); ACCUMULATE: not dense - mark the rows the windows name; lazy - list them, marks kept, and bring them to adam_t;
// then the positive pairs, then the negative pairs; APPLY (apply != 0): lazy flushes a full ring, adam_t goes up, the mode's own launch runs; the loss is read.
// So sparse marks before the pairs, not after them, and launches them behind the negative windows as lazy does.  Nothing sees other inputs for it: one stream;
// walks, negatives and windows touch none of W, G, the loss cell and the bitmap; k_n2v_touch reads the window rows and writes only the bitmap, which the pairs
// do not read; positive pairs still precede negative ones.  A native DENSE batch keeps each sign's pairs right behind its window launch (make_windows' pairs_now).
// One wave per window row: the start row lives in registers (d / 64 values per lane), every rest row costs one coalesced row read, a wave
// reduction and one coalesced f32 atomic row add (the forms that run at full rate on gfx950: 256 contiguous bytes per wave-instruction).
// metapath2vec (torch_geometric.nn.MetaPath2Vec, the `m2v` method of the same plugin) is node2vec after the walks: ntf_m2v_create makes an ntf_n2v handle that carries a
// metapath over per-hop CSRs.  Its own kernels are k_m2v_walks / k_m2v_negs (typed walks and negatives; the draws are n2v_draw's, as k_n2v_walks' / k_n2v_negs'); every
// other kernel serves both handle kinds: k_n2v_windows, k_n2v_adam, the three of sparse Adam, those of lazy dense Adam, k_n2v_edge_bce, and the one pair kernel k_n2v_pairs<NV, DUMMY> - its
// plain form is node2vec's, its DUMMY form (a metapath handle's default) sums the dummy row's terms per workgroup.
#include "../../include/opentf_amd.h"
#include "ntf_device.h"
#include "ntf_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

using namespace ntf;

// metapath of an m2v handle, handed to k_m2v_walks / k_m2v_negs by value: hop i leads from a node of type src to one of type dst over its own CSR (LOCAL ids);
// src_start / dst_start / dst_count are the table's first row and row count of those types, total = the dummy row
struct m2v_path {
    int n_hops = 0; int64_t total = 0;
    const int64_t* rowptr[NTF_M2V_MAX_HOPS] = {}; const int32_t* col[NTF_M2V_MAX_HOPS] = {};
    int64_t src_start[NTF_M2V_MAX_HOPS] = {}, dst_start[NTF_M2V_MAX_HOPS] = {}, dst_count[NTF_M2V_MAX_HOPS] = {};
};

// the row list of a sparse or a lazy handle.  bits: one bit per row (ceil(n / 32) words), set by k_n2v_touch; k_n2v_compact lists the marked rows in list [cap]
// and counts them in count, and clears the marks unless told to keep them.  Absent (all null) on a handle that was never anything but dense
struct n2v_rowlist { uint32_t* bits = nullptr; int64_t* list = nullptr; int64_t cap = 0; unsigned long long* count = nullptr; };
// what lazy dense Adam adds to it.  window > 0 = on: dense Adam that writes only the rows a batch names.  applied [n]: the Adam steps applied to each row
// (<= adam_t); ring [window]: slot s % window holds (lr / bc1, sqrt(bc2)) of step s, for the steps base + 1 .. adam_t - every row is at base or later;
// flushes: full flushes (k_n2v_catchup_all) so far
struct n2v_lazy { int window = 0; uint32_t* applied = nullptr; float2* ring = nullptr; int64_t base = 0, flushes = 0; };
struct ntf_n2v {
    int device = 0; hipStream_t st = nullptr;
    int64_t n = 0; int d = 0, d_user = 0; int64_t nnz = 0;      // d: the device row stride (a multiple of 64); d_user: the embedding size the host sees
    int64_t* rowptr = nullptr; int32_t* col = nullptr;
    float *W = nullptr, *G = nullptr, *M1 = nullptr, *V2 = nullptr;
    int64_t* d_batch = nullptr; int64_t batch_cap = 0;
    int64_t* d_rows = nullptr; int64_t rows_cap = 0;     // window rows [n_rows, ctx]
    const int64_t *win_p = nullptr, *win_n = nullptr; int64_t n_win_p = 0, n_win_n = 0; int win_ctx = 0;   // the last batch's window rows inside d_rows (ntf_n2v_last_windows)
    double* d_loss = nullptr;
    int64_t adam_t = 0; uint64_t seed = 0, step = 0;
    // ntf_n2v_set_optimizer: opt 0 = dense Adam, 1 = sparse Adam; ntf_n2v_set_lazy: lz.window > 0 (opt stays 0) - read through mode().  pend_entries: the window entries whose gradient is in G
    int opt = 0; n2v_rowlist rl; n2v_lazy lz; int64_t pend_entries = 0;
    bool m2v = false, cycle = false; m2v_path mp; int64_t start_count = 0;   // ntf_m2v_create: the metapath; rowptr / col above stay NULL, n = total + 1
    bool dummy_pairs = false;                                                // pairs through k_n2v_pairs<NV, true>: a metapath handle's default (NTF_M2V_PAIRS=0, read by ntf_m2v_create, turns it off)
    std::vector<void*> hop_bufs;                                           // the per-hop CSRs the metapath points into
    // ntf_n2v_set_walk_bias: biased = some (p, q) other than (1, 1) is in force and the walks go through k_n2v_walks_biased with these thresholds;
    // rows_ascending: -1 = not looked at yet, 0 / 1 = what k_n2v_rows_ascending found (asked once, the first time a bias is set)
    bool biased = false; unsigned long long bias_thr[3] = {0, 0, 0}; int rows_ascending = -1;
    std::string err;
};
enum n2v_mode { N2V_DENSE, N2V_SPARSE, N2V_LAZY };
static n2v_mode mode(const ntf_n2v* h) { return h->lz.window > 0 ? N2V_LAZY : h->opt == 1 ? N2V_SPARSE : N2V_DENSE; }
static thread_local std::string g_n2v_create_error;

extern "C" const char* ntf_n2v_last_error(const ntf_n2v* h) { return h ? h->err.c_str() : g_n2v_create_error.c_str(); }

// the draw of position s >= 1 of row r, for walks (base 0) and negatives (base N2V_NEG_BASE) of either handle kind: word (s - 1) & 3 of
// Philox4x32-10(counter (r lo, r hi, base + ((s - 1) >> 2), step), key (k0, k1)).  `rnd` holds the block and is refilled every fourth position; s must go up by one from 1.
constexpr uint32_t N2V_NEG_BASE = 0x4E454700u;
__device__ __forceinline__ uint32_t n2v_draw(uint4& rnd, uint32_t base, int64_t r, int s, uint32_t k0, uint32_t k1, uint32_t step) {
    if (((s - 1) & 3) == 0) rnd = philox4x32(make_uint4((uint32_t)r, (uint32_t)(r >> 32), base + (uint32_t)((s - 1) >> 2), step), make_uint2(k0, k1));
    return ((s - 1) & 3) == 0 ? rnd.x : ((s - 1) & 3) == 1 ? rnd.y : ((s - 1) & 3) == 2 ? rnd.z : rnd.w;
}

// uniform random walk, the walk of a handle whose bias is (1, 1) (torch_cluster / pyg-lib semantics: a node without neighbours keeps the walk where it is).
// Row r starts at batch[r % B] (`batch.repeat(walks_per_node)`); one thread per walk, one Philox call per 4 steps.
__global__ void k_n2v_walks(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ batch, int64_t B,
                            int64_t n_walks, int wl, uint32_t k0, uint32_t k1, uint32_t step, int64_t* __restrict__ rw) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_walks) return;
    int64_t cur = batch[r % B];
    rw[r * wl] = cur;
    uint4 rnd = make_uint4(0, 0, 0, 0);
    for (int s = 1; s < wl; ++s) {
        const uint32_t u = n2v_draw(rnd, 0, r, s, k0, k1, step);
        const int64_t a = rowptr[cur], deg = rowptr[cur + 1] - a;
        if (deg > 0) cur = col[a + (int64_t)(((uint64_t)u * (uint64_t)deg) >> 32)];
        rw[r * wl + s] = cur;
    }
}
// ---- biased (p, q) second-order walks: torch_cluster's random_walk(rowptr, col, start, walk_length, p, q) as include/opentf_amd.h pins it (ntf_n2v_set_walk_bias).
// thr[k] = floor(prob_k * 2^32) of the classes 0: x == t (1 / p), 1: t is in the CSR row of x (1), 2: otherwise (1 / q), each over max(1 / p, 1, 1 / q)
struct n2v_bias { unsigned long long thr[3]; };
// class of candidate x for a walk that came from t: lower bound of t in the ascending row of x (repeats allowed), at most 31 probes of a row below 2^31 entries
__device__ __forceinline__ int n2v_bias_class(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t x, int64_t t) {
    if (x == t) return 0;
    int64_t lo = rowptr[x]; const int64_t end = rowptr[x + 1]; int64_t hi = end;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if ((int64_t)col[mid] < t) lo = mid + 1; else hi = mid; }
    return lo < end && (int64_t)col[lo] == t ? 1 : 2;
}
// the class's threshold by selects: the three stay in scalar registers (an index into the by-value array would send it to scratch)
__device__ __forceinline__ unsigned long long n2v_bias_thr(const n2v_bias& b, int k) { return k == 0 ? b.thr[0] : k == 1 ? b.thr[1] : b.thr[2]; }
// word i of a walk's stream: word i & 3 of Philox4x32-10(counter (r lo, r hi, NTF_N2V_BIAS_BASE + (i >> 2), step), key); only steps that draw advance i
__device__ __forceinline__ uint32_t n2v_bias_word(uint4& rnd, uint32_t& i, int64_t r, uint32_t k0, uint32_t k1, uint32_t step) {
    if ((i & 3) == 0) rnd = philox4x32(make_uint4((uint32_t)r, (uint32_t)(r >> 32), NTF_N2V_BIAS_BASE + (i >> 2), step), make_uint2(k0, k1));
    const uint32_t w = (i & 3) == 0 ? rnd.x : (i & 3) == 1 ? rnd.y : (i & 3) == 2 ? rnd.z : rnd.w;
    ++i;
    return w;
}
__device__ __forceinline__ unsigned long long wave_bcast_u64(unsigned long long v, int src) {
    return ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64);
}
__device__ __forceinline__ unsigned long long wave_shfl_up_u64(unsigned long long v, int o) {
    return ((unsigned long long)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, o, 64);
}
// One thread per walk, like k_n2v_walks.  A step of a walk on a node of degree >= 2, past position 1, is drawn in two stages.  Stage 1, per lane: up to
// NTF_N2V_BIAS_TRIES rejection attempts (a candidate load and a binary search each).  Stage 2, for the lanes still undecided, one lane at a time with the WHOLE wave:
// the exact inverse-CDF scan of the row over the same integer weights - 64 entries a stride, a 64-bit wave prefix sum carried across the strides, first the total,
// then the crossing of target = (U * total) >> 64 - so a hub row of 1e5 entries costs 2 * ceil(deg / 64) strides, not one lane's 1e5 probes.  Stage 2 crosses lanes:
// it sits outside every lane-dependent branch and loop, and a lane with r >= n_walks does not return - it stays as an idle participant (live = false).
// Integer arithmetic throughout: the walk does not depend on how the scan is split over the lanes, and the host replay (tests/n2v_bias_reference.py) pins it.
__global__ __launch_bounds__(256) void k_n2v_walks_biased(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ batch,
                                                          int64_t B, int64_t n_walks, int wl, uint32_t k0, uint32_t k1, uint32_t step, const n2v_bias bias,
                                                          int64_t* __restrict__ rw) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = r < n_walks;
    int64_t cur = live ? batch[r % B] : 0, prev = cur;
    if (live) rw[r * wl] = cur;
    uint4 rnd = make_uint4(0, 0, 0, 0);
    uint32_t nw = 0;                                        // words consumed so far
    for (int s = 1; s < wl; ++s) {                          // wave-uniform trip count
        int64_t a = 0, deg = 0, next = cur;
        unsigned long long U = 0;
        bool undecided = false;
        if (live) {
            a = rowptr[cur]; deg = rowptr[cur + 1] - a;
            if (deg == 1) next = col[a];
            else if (deg >= 2 && s == 1) next = col[a + (int64_t)(((uint64_t)n2v_bias_word(rnd, nw, r, k0, k1, step) * (uint64_t)deg) >> 32)];
            else if (deg >= 2) {
                undecided = true;
                for (int k = 0; k < NTF_N2V_BIAS_TRIES && undecided; ++k) {
                    const uint32_t uc = n2v_bias_word(rnd, nw, r, k0, k1, step), ua = n2v_bias_word(rnd, nw, r, k0, k1, step);
                    const int64_t c = col[a + (int64_t)(((uint64_t)uc * (uint64_t)deg) >> 32)];
                    if ((unsigned long long)ua < n2v_bias_thr(bias, n2v_bias_class(rowptr, col, c, prev))) { next = c; undecided = false; }
                }
                if (undecided) {
                    const uint32_t uhi = n2v_bias_word(rnd, nw, r, k0, k1, step), ulo = n2v_bias_word(rnd, nw, r, k0, k1, step);
                    U = ((unsigned long long)uhi << 32) | ulo;
                }
            }
        }
        // stage 2: every lane of the wave is here
        for (unsigned long long pend = __ballot(undecided); pend; pend &= pend - 1) {
            const int o = __ffsll(pend) - 1;
            const int64_t oa = (int64_t)wave_bcast_u64((unsigned long long)a, o), odeg = (int64_t)wave_bcast_u64((unsigned long long)deg, o);
            const int64_t ot = (int64_t)wave_bcast_u64((unsigned long long)prev, o);
            const unsigned long long oU = wave_bcast_u64(U, o);
            unsigned long long total = 0;                   // < 2^63: below 2^31 entries of at most 2^32 each
            for (int64_t j = lane; j < odeg; j += 64) total += n2v_bias_thr(bias, n2v_bias_class(rowptr, col, col[oa + j], ot));
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) total += wave_bcast_u64(total, lane ^ m);
            const unsigned long long target = __umul64hi(oU, total);      // < total: a crossing exists
            unsigned long long carry = 0;
            int64_t at = odeg - 1;
            for (int64_t base = 0; base < odeg; base += 64) {             // wave-uniform trip count and exit
                const int64_t j = base + lane;
                unsigned long long incl = j < odeg ? n2v_bias_thr(bias, n2v_bias_class(rowptr, col, col[oa + j], ot)) : 0ull;
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) { const unsigned long long up = wave_shfl_up_u64(incl, m); if (lane >= m) incl += up; }
                incl += carry;
                const unsigned long long hit = __ballot(j < odeg && incl > target);
                if (hit) { at = base + (__ffsll(hit) - 1); break; }
                carry = wave_bcast_u64(incl, 63);
            }
            const int64_t x = col[oa + at];
            if (lane == o) next = x;
        }
        prev = cur; cur = next;
        if (live) rw[r * wl + s] = cur;
    }
}
// the ascending order the binary search of n2v_bias_class needs: one thread per CSR entry p >= 1, out of order when col[p] < col[p - 1] inside one row (p is
// no row's first entry: lower bound of p in rowptr).  Run once per handle, the first time a bias is set.
__global__ void k_n2v_rows_ascending(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n, int64_t nnz, int* __restrict__ bad) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (p >= nnz || col[p] >= col[p - 1]) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (rowptr[mid] < p) lo = mid + 1; else hi = mid; }
    if (rowptr[lo] != p) *bad = 1;
}
// negative rows: start node followed by uniformly random nodes (`torch.randint(num_nodes, ...)`), start = batch[r % B]
__global__ void k_n2v_negs(const int64_t* __restrict__ batch, int64_t B, int64_t n_rows, int wl, int64_t num_nodes, uint32_t k0, uint32_t k1, uint32_t step,
                           int64_t* __restrict__ rw) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    rw[r * wl] = batch[r % B];
    uint4 rnd = make_uint4(0, 0, 0, 0);
    for (int s = 1; s < wl; ++s) {
        const uint32_t u = n2v_draw(rnd, N2V_NEG_BASE, r, s, k0, k1, step);
        rw[r * wl + s] = (int64_t)(((uint64_t)u * (uint64_t)num_nodes) >> 32);
    }
}
// metapath2vec walks (MetaPath2Vec.pos_sample): step s goes over hop (s - 1) % n_hops; `cur` is the LOCAL id inside the type the walk stands on, -1 = the dummy.
// A node without neighbours in that hop leads to the dummy and the dummy stays; both still take their draw slot, so the Philox layout is k_n2v_walks'.
__global__ void k_m2v_walks(const m2v_path mp, const int64_t* __restrict__ batch, int64_t B, int64_t n_walks, int wl, uint32_t k0, uint32_t k1, uint32_t step,
                            int64_t* __restrict__ rw) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_walks) return;
    int64_t cur = batch[r % B];
    rw[r * wl] = mp.src_start[0] + cur;
    uint4 rnd = make_uint4(0, 0, 0, 0);
    for (int s = 1; s < wl; ++s) {
        const uint32_t u = n2v_draw(rnd, 0, r, s, k0, k1, step);
        const int hp = (s - 1) % mp.n_hops;
        if (cur >= 0) {
            const int64_t a = mp.rowptr[hp][cur], deg = mp.rowptr[hp][cur + 1] - a;
            cur = deg > 0 ? (int64_t)mp.col[hp][a + (int64_t)(((uint64_t)u * (uint64_t)deg) >> 32)] : -1;
        }
        rw[r * wl + s] = cur >= 0 ? mp.dst_start[hp] + cur : mp.total;
    }
}
// metapath2vec negatives (MetaPath2Vec.neg_sample): the start node, then at position s a uniformly random node of the type hop (s - 1) % n_hops leads to; never the dummy
__global__ void k_m2v_negs(const m2v_path mp, const int64_t* __restrict__ batch, int64_t B, int64_t n_rows, int wl, uint32_t k0, uint32_t k1, uint32_t step,
                           int64_t* __restrict__ rw) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    rw[r * wl] = mp.src_start[0] + batch[r % B];
    uint4 rnd = make_uint4(0, 0, 0, 0);
    for (int s = 1; s < wl; ++s) {
        const uint32_t u = n2v_draw(rnd, N2V_NEG_BASE, r, s, k0, k1, step);
        const int hp = (s - 1) % mp.n_hops;
        rw[r * wl + s] = mp.dst_start[hp] + (int64_t)(((uint64_t)u * (uint64_t)mp.dst_count[hp]) >> 32);
    }
}
// windows of `ctx` consecutive nodes: out row j * n_walks + r = rw[r, j : j + ctx]   (torch.cat of the slices along dim 0)
__global__ void k_n2v_windows(const int64_t* __restrict__ rw, int64_t n_walks, int wl, int ctx, int64_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nw = wl + 1 - ctx;
    if (t >= n_walks * nw * ctx) return;
    const int c = (int)(t % ctx); const int64_t row = t / ctx, j = row / n_walks, r = row % n_walks;
    out[t] = rw[r * wl + j + c];
}

// loss and gradient of one set of window rows; positive != 0: positive pairs, 0: negative pairs.  NV = d / 64 values per lane.  One wave per window row: every
// term is one atomic row add on G (the rest row's per pair, the start row's once per window row).
// DUMMY (a metapath handle's default): the same terms, but those that land on the `dummy` row (a rest row or a start row that is the dummy - every walk that met a
// dead end names it from there on) do not go to G one atomic row add each: a wave keeps their sum in gd, the workgroup's four waves meet in LDS, and G[dummy]
// takes one row add per workgroup that had such a term.  gd, any, the LDS array and the barrier exist only in that form; !DUMMY ignores `dummy`.
template <int NV, bool DUMMY>
__global__ __launch_bounds__(256) void k_n2v_pairs(const float* __restrict__ W, const int64_t* __restrict__ rows, int64_t n_rows, int ctx, int d,
                                                   float inv_pairs, int positive, int64_t dummy, float* __restrict__ G, double* __restrict__ loss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wave;
    float lsum = 0.f, gd[NV];
    int any = 0;          // wave-uniform: a window row is one wave's
#pragma unroll
    for (int k = 0; k < NV; ++k) gd[k] = 0.f;
    if (r < n_rows) {
        const int64_t s = rows[r * ctx];
        float hs[NV], gs[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) { hs[k] = W[s * d + lane + 64 * k]; gs[k] = 0.f; }
        for (int c = 1; c < ctx; ++c) {
            const int64_t v = rows[r * ctx + c];
            float hv[NV], dot = 0.f;
#pragma unroll
            for (int k = 0; k < NV; ++k) { hv[k] = W[v * d + lane + 64 * k]; dot += hs[k] * hv[k]; }
            dot = wave_reduce_sum(dot);
            const float sg = 1.f / (1.f + expf(-dot));
            float coef;   // d loss / d dot
            if (positive) { lsum -= logf(sg + 1e-15f); coef = -sg * (1.f - sg) / (sg + 1e-15f) * inv_pairs; }
            else { lsum -= logf(1.f - sg + 1e-15f); coef = sg * (1.f - sg) / (1.f - sg + 1e-15f) * inv_pairs; }
            if (DUMMY && v == dummy) {
                any = 1;
#pragma unroll
                for (int k = 0; k < NV; ++k) { gd[k] += coef * hs[k]; gs[k] += coef * hv[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < NV; ++k) { atomicAdd(G + v * d + lane + 64 * k, coef * hs[k]); gs[k] += coef * hv[k]; }
            }
        }
        if (DUMMY && s == dummy) {
            any = 1;
#pragma unroll
            for (int k = 0; k < NV; ++k) gd[k] += gs[k];
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) atomicAdd(G + s * d + lane + 64 * k, gs[k]);
        }
    }
    if (lane == 0 && r < n_rows) atomicAdd(loss, (double)lsum * (double)inv_pairs);
    if constexpr (DUMMY) {
        __shared__ float sh[4][NV * 64];
#pragma unroll
        for (int k = 0; k < NV; ++k) sh[wave][lane + 64 * k] = gd[k];
        if (__syncthreads_or(any))          // every thread of the workgroup arrives here (no early return above)
            for (int q = threadIdx.x; q < NV * 64; q += 256) atomicAdd(G + dummy * d + q, (sh[0][q] + sh[1][q]) + (sh[2][q] + sh[3][q]));
    }
}

// dense Adam that also clears the gradient for the next batch (one pass over the four buffers)
__global__ void k_n2v_adam(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n, float lr_over_bc1,
                           float b1, float b2, float eps, float bc2_sqrt) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < (n >> 2); q += (int64_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[q], mm = reinterpret_cast<float4*>(m)[q], vv = reinterpret_cast<float4*>(v)[q];
        const float4 gg = reinterpret_cast<float4*>(g)[q];
        float* P = &pp.x; float* M = &mm.x; float* V = &vv.x; const float* Gv = &gg.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            M[k] = M[k] * b1 + (1.f - b1) * Gv[k];
            V[k] = V[k] * b2 + (1.f - b2) * Gv[k] * Gv[k];
            P[k] -= lr_over_bc1 * (M[k] / (sqrtf(V[k]) / bc2_sqrt + eps));
        }
        reinterpret_cast<float4*>(p)[q] = pp; reinterpret_cast<float4*>(m)[q] = mm; reinterpret_cast<float4*>(v)[q] = vv;
        reinterpret_cast<float4*>(g)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ---- sparse Adam (torch.optim.SparseAdam: only the rows a batch names move, their moments decay only in the steps that name them; ntf_n2v_set_optimizer(1))
// marks the row of every window entry, start or rest: one bit per row.  A hub is named hundreds of times a batch: the plain read keeps all but the first of them
// off the atomic unit (a stale read costs one more atomic OR, nothing else).  `hot` (the dummy row of a metapath handle, -1 otherwise) is named by a sizeable
// share of ALL entries: the whole grid is in flight before the first OR lands, so the read alone left hundreds of thousands of atomics on one address (0.51 ms
// of a 2.26 ms batch at dblp shapes); of the lanes of a wave that would mark it, one does.
__global__ __launch_bounds__(256) void k_n2v_touch(const int64_t* __restrict__ rows, int64_t n_entries, int64_t hot, uint32_t* __restrict__ bits) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t v = t < n_entries ? rows[t] : -1;        // no early return: the ballot is the whole wave's
    uint32_t b = 0; bool need = false;
    if (v >= 0) { b = 1u << (uint32_t)(v & 31); need = !(bits[v >> 5] & b); }
    const bool on_hot = need && v == hot;
    const unsigned long long hm = __ballot(on_hot);
    if (on_hot && (int)(threadIdx.x & 63) != __ffsll(hm) - 1) need = false;
    if (need) atomicOr(bits + (v >> 5), b);
}
// the marked rows as a list: one thread per bitmap word, a wave takes ONE slot range from the counter (inclusive scan of the popcounts, the last lane asks), every
// lane writes the ids of its word behind those of the lanes before it and clears the word.  The order of the waves' ranges is not fixed; each row is listed once.
// !CLEAR: the same list with the marks left standing (lazy dense Adam lists the rows BEFORE the pairs and keeps the marks of a gradient that stays pending)
template <bool CLEAR>
__global__ __launch_bounds__(256) void k_n2v_compact(uint32_t* __restrict__ bits, int64_t n_words, int64_t* __restrict__ list, unsigned long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t word = w < n_words ? bits[w] : 0u;            // no early return: every lane takes part in the shuffles
    if (CLEAR && word) bits[w] = 0u;
    const int c = __popc(word);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
    const int total = __shfl(incl, 63, 64);
    if (total == 0) return;                                // wave-uniform
    unsigned long long base = 0;
    if (lane == 63) base = atomicAdd(count, (unsigned long long)total);
    const uint32_t lo = __shfl((uint32_t)base, 63, 64), hi = __shfl((uint32_t)(base >> 32), 63, 64);
    int64_t at = (int64_t)(((unsigned long long)hi << 32) | lo) + (incl - c);
    while (word) { list[at++] = w * 32 + (__ffs(word) - 1); word &= word - 1; }
}
// torch.optim._functional.sparse_adam on the listed rows, one wave per row (NV = d / 64 values per lane), and the row of G cleared for the next batch.
// step = lr sqrt(1 - b2^t) / (1 - b1^t); omb1 = 1 - b1, omb2 = 1 - b2 (rounded once, on the host); eps is added to sqrt(v) itself - not k_n2v_adam's placement.
// The grid strides over the count k_n2v_compact left on the device: no host read between the two.  A pad column has g = m = v = 0 and stays 0.
template <int NV>
__global__ __launch_bounds__(256) void k_n2v_adam_rows(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                       const int64_t* __restrict__ list, const unsigned long long* __restrict__ count, int d, float step,
                                                       float omb1, float omb2, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)*count;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
        const int64_t o = list[i] * d + lane;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int64_t q = o + 64 * k;
            const float gg = g[q];
            float mm = m[q], vv = v[q];
            mm += omb1 * (gg - mm);
            vv += omb2 * (gg * gg - vv);
            p[q] -= step * (mm / (sqrtf(vv) + eps));
            m[q] = mm; v[q] = vv; g[q] = 0.f;
        }
    }
}

// ---- lazy dense Adam (ntf_n2v_set_lazy): k_n2v_adam's table, bit for bit, with only the rows a batch names written.  A row whose gradient is zero in step t
// takes k_n2v_adam's update with g = 0 (n2v_adam_elem) from nothing but its own p, m, v and the step's two constants, so a row left behind at step `applied[row]` is brought to `upto` by
// running the steps applied + 1 .. upto in order, in registers, each with its own ring entry (wave-uniform).  There is no closed form (eps, the bias corrections,
// a changing lr) and no early exit: 0.9 * min_denormal rounds back to min_denormal, a moment never reaches zero.  The one shortcut: a row whose m and v are all
// +0 bits is unchanged by such a step and is not loaded further.  One wave per row, NV = d / 64 values per lane.
// one element of k_n2v_adam's step for the lazy kernels below.  Sharing one inline function with k_n2v_adam was tried and MOVED that kernel: inside the function the
// compiler contracted m as fma(1 - b1, g, b1 m) where k_n2v_adam has fma(b1, m, (1 - b1) g) - another rounding (profiles/n2v_lazy_check.md).  So k_n2v_adam
// keeps its text, and this copy spells out, with contraction off, the operations that kernel's code performs: the products (1 - b1) g, (1 - b2) g and b2 v are
// rounded, the three sums are fused.  sqrtf and both divisions are correctly rounded in either.  tests/test_gpu_n2v_lazy.py holds the two together bit for bit.
__device__ __forceinline__ void n2v_adam_elem(float& p, float& m, float& v, float g, float lr_over_bc1, float b1, float b2, float eps, float bc2_sqrt) {
#pragma clang fp contract(off)
    const float mg = (1.f - b1) * g, vg = (1.f - b2) * g, vb = b2 * v;
    m = __builtin_fmaf(b1, m, mg);
    v = __builtin_fmaf(g, vg, vb);
    p = __builtin_fmaf(-lr_over_bc1, m / (sqrtf(v) / bc2_sqrt + eps), p);
}
// one row, by its wave: the zero-gradient steps applied[row] + 1 .. upto, each with its ring entry.
//   GRAD: after the catch-up the row takes step upto + 1 with its row of G (constants lr_over_bc1 / bc2_sqrt, the kernel's own), the row of G is cleared and
//         applied = upto + 1
//   ALL : a row without moments keeps its `applied` (k_n2v_catchup_all leaves the rows nothing ever named at 0); otherwise applied = upto
template <int NV, bool GRAD, bool ALL>
__device__ __forceinline__ void n2v_catchup(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, uint32_t* __restrict__ applied,
                                            const float2* __restrict__ ring, uint32_t window, int64_t row, int d, int lane, uint32_t upto, float lr_over_bc1,
                                            float b1, float b2, float eps, float bc2_sqrt) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)applied[row]);
    if (!GRAD && a >= upto) return;                          // current: nothing but `applied` was read
    const int64_t o = row * d + lane;
    float pp[NV], mm[NV], vv[NV];
    bool nz = false;
#pragma unroll
    for (int k = 0; k < NV; ++k) { mm[k] = m[o + 64 * k]; vv[k] = v[o + 64 * k]; nz = nz || (__float_as_uint(mm[k]) | __float_as_uint(vv[k])) != 0u; }
    const bool run = a < upto && __ballot(nz) != 0ull;        // wave-uniform
    if (GRAD || run) {
#pragma unroll
        for (int k = 0; k < NV; ++k) pp[k] = p[o + 64 * k];
    }
    if (run) {
        uint32_t slot = (a + 1u) % window;
        for (uint32_t s = a; s < upto; ++s) {
            const float2 c = ring[slot];
            slot = slot + 1u == window ? 0u : slot + 1u;
#pragma unroll
            for (int k = 0; k < NV; ++k) n2v_adam_elem(pp[k], mm[k], vv[k], 0.f, c.x, b1, b2, eps, c.y);
        }
    }
    if (GRAD) {
#pragma unroll
        for (int k = 0; k < NV; ++k) { n2v_adam_elem(pp[k], mm[k], vv[k], g[o + 64 * k], lr_over_bc1, b1, b2, eps, bc2_sqrt); g[o + 64 * k] = 0.f; }
    }
    if (GRAD || run) {
#pragma unroll
        for (int k = 0; k < NV; ++k) { p[o + 64 * k] = pp[k]; m[o + 64 * k] = mm[k]; v[o + 64 * k] = vv[k]; }
    }
    if (lane == 0 && (GRAD || run || !ALL)) applied[row] = GRAD ? upto + 1u : upto;
}
// the listed rows (k_n2v_compact; the grid strides over the count left on the device, as k_n2v_adam_rows does).  GRAD: the step of the batch
// itself; its first lane also files the step's constants in the ring (`ring_slot` = the slot of step upto + 1, which no catch-up of this launch reads: they stop at upto)
template <int NV, bool GRAD>
__global__ __launch_bounds__(256) void k_n2v_catchup_rows(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                          uint32_t* __restrict__ applied, const float2* __restrict__ ring, float2* ring_slot, uint32_t window,
                                                          const int64_t* __restrict__ list, const unsigned long long* __restrict__ count, int d, uint32_t upto,
                                                          float lr_over_bc1, float b1, float b2, float eps, float bc2_sqrt) {
    const int lane = threadIdx.x & 63;
    if (GRAD && blockIdx.x == 0 && threadIdx.x == 0) *ring_slot = make_float2(lr_over_bc1, bc2_sqrt);
    const int64_t n = (int64_t)*count;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4)
        n2v_catchup<NV, GRAD, false>(p, g, m, v, applied, ring, window, list[i], d, lane, upto, lr_over_bc1, b1, b2, eps, bc2_sqrt);
}
// every row (the full flush): a row that is current costs the read of its `applied`
template <int NV>
__global__ __launch_bounds__(256) void k_n2v_catchup_all(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, uint32_t* __restrict__ applied,
                                                         const float2* __restrict__ ring, uint32_t window, int64_t n, int d, uint32_t upto, float b1, float b2, float eps) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4)
        n2v_catchup<NV, false, true>(p, nullptr, m, v, applied, ring, window, row, d, lane, upto, 0.f, b1, b2, eps, 0.f);
}

// v_loss of _train_rw (gnn.py:420-431): mean BCE-with-logits of the held-out edges' scores against 1 = mean softplus(-score)
__global__ __launch_bounds__(256) void k_n2v_edge_bce(const float* __restrict__ W, const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t n, int d,
                                                      double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float dot = 0.f;
    for (int k = lane; k < d; k += 64) dot += W[src[r] * d + k] * W[dst[r] * d + k];
    dot = wave_reduce_sum(dot);
    if (lane == 0) atomicAdd(out, (double)(fmaxf(-dot, 0.f) + log1pf(expf(-fabsf(dot)))));
}

extern "C" void ntf_n2v_destroy(ntf_n2v* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    for (void* p : {(void*)h->rowptr, (void*)h->col, (void*)h->W, (void*)h->G, (void*)h->M1, (void*)h->V2, (void*)h->d_batch, (void*)h->d_rows, (void*)h->d_loss,
                    (void*)h->rl.bits, (void*)h->rl.list, (void*)h->rl.count, (void*)h->lz.applied, (void*)h->lz.ring})
        if (p) hipFree(p);
    for (void* p : h->hop_bufs) if (p) hipFree(p);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

// what ntf_n2v_create and ntf_m2v_create share once their arguments are checked: the device, the handle over a table [n, d] and its stream, the caller's graph
// (`graph(h, ok)` sets its fields and uploads its CSRs: it returns its first failed allocation's code and ands its copies into ok), the four tables and the loss
// cell, the padded upload, the zeroing.  A failure leaves its text in g_n2v_create_error and frees what was made (ntf_n2v_destroy).
// Any embedding size 1..256 (data.embedding.d is free in the reference): a device row is padded to a multiple of 64 floats (h->d, what the kernels see); the pad
// columns of the table are zero and stay zero - their gradient is a multiple of another row's zero pad, and Adam leaves a zero parameter with zero moments where it is
template <class Graph>
static int n2v_create_on_device(int device, int64_t n, int32_t d, const float* init_weight, uint64_t seed, ntf_n2v** out, Graph&& graph) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_n2v_create_error = "no such HIP device (there is no CPU fallback)"; return NTF_EHIP; }
    hipSetDevice(device);
    ntf_n2v* h = new ntf_n2v();
    h->device = device; h->n = n; h->d_user = d; h->d = (d + 63) / 64 * 64; h->seed = seed;
    if (hipStreamCreate(&h->st) != hipSuccess) { g_n2v_create_error = "hipStreamCreate failed"; delete h; return NTF_EHIP; }
    bool ok = true;
    auto H = [&](hipError_t s) { ok = ok && s == hipSuccess; };
    int rc = graph(h, ok);
    auto A = [&](int r) { if (rc == NTF_OK) rc = r; };
    const int64_t np = n * h->d;
    A(dev_alloc(h, &h->W, np)); A(dev_alloc(h, &h->G, np)); A(dev_alloc(h, &h->M1, np)); A(dev_alloc(h, &h->V2, np)); A(dev_alloc(h, &h->d_loss, 2));
    if (rc != NTF_OK) { g_n2v_create_error = h->err; ntf_n2v_destroy(h); return rc; }
    H(upload_padded(h->W, h->d, init_weight, d, n));
    H(hipMemsetAsync(h->G, 0, np * 4, h->st)); H(hipMemsetAsync(h->M1, 0, np * 4, h->st)); H(hipMemsetAsync(h->V2, 0, np * 4, h->st));
    H(hipStreamSynchronize(h->st));
    if (!ok) { g_n2v_create_error = "device initialisation failed"; ntf_n2v_destroy(h); return NTF_EHIP; }
    *out = h;
    return NTF_OK;
}

extern "C" int ntf_n2v_create(int device, int64_t num_nodes, int32_t d, const int64_t* rowptr, const int32_t* col, const float* init_weight, uint64_t seed, ntf_n2v** out) {
    if (!out) { g_n2v_create_error = "out is NULL"; return NTF_EINVAL; }
    *out = nullptr;
    if (num_nodes < 1 || d < 1 || d > 256 || !rowptr || !init_weight) { g_n2v_create_error = "n2v: need num_nodes >= 1, 1 <= d <= 256, a CSR graph and initial weights"; return NTF_EINVAL; }
    const int64_t nnz = rowptr[num_nodes];
    for (int64_t i = 0; i < num_nodes; ++i) if (rowptr[i + 1] < rowptr[i]) { g_n2v_create_error = "n2v: rowptr not monotone"; return NTF_EINVAL; }
    for (int64_t p = 0; p < nnz; ++p) if (col[p] < 0 || col[p] >= num_nodes) { g_n2v_create_error = "n2v: neighbour id out of range"; return NTF_EINVAL; }
    return n2v_create_on_device(device, num_nodes, d, init_weight, seed, out, [&](ntf_n2v* h, bool& ok) {
        h->nnz = nnz;
        if (int r = dev_alloc(h, &h->rowptr, num_nodes + 1)) return r;
        if (int r = dev_alloc(h, &h->col, std::max<int64_t>(nnz, 1))) return r;
        ok = ok && hipMemcpy(h->rowptr, rowptr, (num_nodes + 1) * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (nnz) ok = ok && hipMemcpy(h->col, col, nnz * 4, hipMemcpyHostToDevice) == hipSuccess;
        return (int)NTF_OK;
    });
}

// metapath2vec: an ntf_n2v handle over [total + 1, d] that carries a metapath (include/opentf_amd.h); everything is checked on the host before anything is allocated
extern "C" int ntf_m2v_create(int device, int32_t n_types, const int64_t* type_count, int32_t n_hops, const int32_t* hop_src, const int32_t* hop_dst,
                              const int64_t* const* hop_rowptr, const int32_t* const* hop_col, int32_t d, const float* init_weight, uint64_t seed, ntf_n2v** out) {
    if (!out) { g_n2v_create_error = "out is NULL"; return NTF_EINVAL; }
    *out = nullptr;
    auto bad = [&](const char* m) { g_n2v_create_error = m; return (int)NTF_EINVAL; };
    if (n_types < 1 || n_types > NTF_M2V_MAX_TYPES || n_hops < 1 || n_hops > NTF_M2V_MAX_HOPS) return bad("m2v: need 1 .. 8 node types and 1 .. 8 hops");
    if (d < 1 || d > 256 || !type_count || !hop_src || !hop_dst || !hop_rowptr || !hop_col || !init_weight) return bad("m2v: need 1 <= d <= 256, type counts, hops with their CSRs and initial weights");
    int64_t start[NTF_M2V_MAX_TYPES + 1] = {0};
    for (int t = 0; t < n_types; ++t) {
        if (type_count[t] < 1 || type_count[t] > 0x7FFFFFFF) return bad("m2v: a node type needs between 1 and 2^31 - 1 nodes");
        start[t + 1] = start[t] + type_count[t];
    }
    const int64_t total = start[n_types];
    int64_t nnz[NTF_M2V_MAX_HOPS];
    for (int i = 0; i < n_hops; ++i) {
        if (hop_src[i] < 0 || hop_src[i] >= n_types || hop_dst[i] < 0 || hop_dst[i] >= n_types) return bad("m2v: a hop names a node type outside [0, n_types)");
        if (i + 1 < n_hops && hop_dst[i] != hop_src[i + 1]) return bad("m2v: the metapath does not chain (a hop's destination type is not the next hop's source type)");
        const int64_t ns = type_count[hop_src[i]], nd = type_count[hop_dst[i]]; const int64_t* rp = hop_rowptr[i];
        if (!rp || rp[0] != 0) return bad("m2v: a hop's rowptr is missing or does not start at 0");
        for (int64_t k = 0; k < ns; ++k) if (rp[k + 1] < rp[k]) return bad("m2v: rowptr not monotone");
        nnz[i] = rp[ns];
        if (nnz[i] > 0 && !hop_col[i]) return bad("m2v: a hop with edges has no column array");
        for (int64_t p = 0; p < nnz[i]; ++p) if (hop_col[i][p] < 0 || hop_col[i][p] >= nd) return bad("m2v: neighbour id outside its destination type");
    }
    return n2v_create_on_device(device, total + 1, d, init_weight, seed, out, [&](ntf_n2v* h, bool& ok) {
        h->m2v = true; h->cycle = hop_dst[n_hops - 1] == hop_src[0]; h->start_count = type_count[hop_src[0]];
        h->mp.n_hops = n_hops; h->mp.total = total;
        h->dummy_pairs = true;                                                  // 3.32 against 4.73 ms per batch at dblp shapes (profiles/m2v_bench.md); 0 keeps the plain form
        if (const char* e = getenv("NTF_M2V_PAIRS")) h->dummy_pairs = atoi(e) != 0;
        for (int i = 0; i < n_hops; ++i) {
            const int64_t ns = type_count[hop_src[i]];
            int64_t* rp = nullptr; int32_t* cl = nullptr;
            int rc = dev_alloc(h, &rp, ns + 1); h->hop_bufs.push_back(rp);
            if (rc == NTF_OK) { rc = dev_alloc(h, &cl, std::max<int64_t>(nnz[i], 1)); h->hop_bufs.push_back(cl); }
            if (rc != NTF_OK) return rc;
            ok = ok && hipMemcpy(rp, hop_rowptr[i], (ns + 1) * 8, hipMemcpyHostToDevice) == hipSuccess;
            if (nnz[i]) ok = ok && hipMemcpy(cl, hop_col[i], nnz[i] * 4, hipMemcpyHostToDevice) == hipSuccess;
            h->mp.rowptr[i] = rp; h->mp.col[i] = cl;
            h->mp.src_start[i] = start[hop_src[i]]; h->mp.dst_start[i] = start[hop_dst[i]]; h->mp.dst_count[i] = type_count[hop_dst[i]];
        }
        return (int)NTF_OK;
    });
}

static void n2v_key(const ntf_n2v* h, uint64_t step, int tensor, uint32_t& k0, uint32_t& k1) {
    uint64_t x = h->seed ^ (step * 0x9E3779B97F4A7C15ull + (uint64_t)tensor * 0xBF58476D1CE4E5B9ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    k0 = (uint32_t)x; k1 = (uint32_t)(x >> 32);
}
static int stage_batch(ntf_n2v* h, const int64_t* batch, int64_t B) {
    const int64_t lim = h->m2v ? h->start_count : h->n;        // a metapath handle takes LOCAL ids of its start type
    for (int64_t i = 0; i < B; ++i) if (batch[i] < 0 || batch[i] >= lim) FAIL(h, NTF_EINVAL, "n2v: start node out of range");
    if (int r = dev_grow(h, &h->d_batch, &h->batch_cap, B)) return r;
    HIPCHK(h, hipMemcpyAsync(h->d_batch, batch, B * 8, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return NTF_OK;
}
static bool m2v_too_long(const ntf_n2v* h, int walk_length) { return h->m2v && !h->cycle && walk_length - 1 > h->mp.n_hops; }
static int need_rows(ntf_n2v* h, int64_t elems) {
    h->win_p = h->win_n = nullptr; h->n_win_p = h->n_win_n = 0; h->win_ctx = 0;   // every writer of d_rows comes through here
    return dev_grow(h, &h->d_rows, &h->rows_cap, elems);
}
// the walks / the negative rows of call `step` from the staged batch of B start nodes into rw [n_rows, wl]: the typed kernel on a metapath handle, the untyped one
// otherwise - uniform, or biased while a (p, q) other than (1, 1) is in force
static void launch_walks(ntf_n2v* h, int64_t B, int64_t n_rows, int wl, uint64_t step, int64_t* rw) {
    uint32_t k0, k1; n2v_key(h, step, 0, k0, k1);
    const dim3 grid((unsigned)((n_rows + 255) / 256)), block(256);
    if (h->m2v) hipLaunchKernelGGL(k_m2v_walks, grid, block, 0, h->st, h->mp, h->d_batch, B, n_rows, wl, k0, k1, (uint32_t)step, rw);
    else if (h->biased) {
        const n2v_bias bias = {{h->bias_thr[0], h->bias_thr[1], h->bias_thr[2]}};
        hipLaunchKernelGGL(k_n2v_walks_biased, grid, block, 0, h->st, h->rowptr, h->col, h->d_batch, B, n_rows, wl, k0, k1, (uint32_t)step, bias, rw);
    } else hipLaunchKernelGGL(k_n2v_walks, grid, block, 0, h->st, h->rowptr, h->col, h->d_batch, B, n_rows, wl, k0, k1, (uint32_t)step, rw);
}
static void launch_negs(ntf_n2v* h, int64_t B, int64_t n_rows, int wl, uint64_t step, int64_t* rw) {
    uint32_t k0, k1; n2v_key(h, step, 1, k0, k1);
    const dim3 grid((unsigned)((n_rows + 255) / 256)), block(256);
    if (h->m2v) hipLaunchKernelGGL(k_m2v_negs, grid, block, 0, h->st, h->mp, h->d_batch, B, n_rows, wl, k0, k1, (uint32_t)step, rw);
    else hipLaunchKernelGGL(k_n2v_negs, grid, block, 0, h->st, h->d_batch, B, n_rows, wl, h->n, k0, k1, (uint32_t)step, rw);
}

extern "C" int ntf_n2v_walks(ntf_n2v* h, const int64_t* start, int64_t n, int32_t walk_length, uint64_t step, int64_t* out_host) {
    if (!h || !start || n < 1 || walk_length < 1 || !out_host) return NTF_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    if (m2v_too_long(h, walk_length)) FAIL(h, NTF_EINVAL, "m2v: a walk longer than the metapath needs a metapath that ends on its start type");
    int r = stage_batch(h, start, n); if (r) return r;
    if ((r = need_rows(h, n * walk_length))) return r;
    launch_walks(h, n, n, walk_length, step, h->d_rows);
    HIPCHK(h, hipMemcpyAsync(out_host, h->d_rows, n * walk_length * 8, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return NTF_OK;
}

// ---- the row list, host side: what sparse and lazy Adam share.  rowlist_make: the bitmap and the counter of a handle that has none, allocated and cleared into
// `made` (left empty where the handle has them); the stream is idle on return.  Nothing of the handle changes: the caller commits `made` once all it needs is there
static int64_t rowlist_words(const ntf_n2v* h) { return (h->n + 31) / 32; }
static int rowlist_make(ntf_n2v* h, n2v_rowlist* made) {
    HIPCHK(h, hipSetDevice(h->device));
    int r = NTF_OK; hipError_t s = hipSuccess;
    if (!h->rl.bits) {
        if (!(r = dev_alloc(h, &made->bits, rowlist_words(h)))) r = dev_alloc(h, &made->count, 1);
        if (!r && (s = hipMemsetAsync(made->bits, 0, (size_t)rowlist_words(h) * 4, h->st)) == hipSuccess) s = hipMemsetAsync(made->count, 0, 8, h->st);
    }
    if (!r && s == hipSuccess) s = hipStreamSynchronize(h->st);
    if (!r && s != hipSuccess) { h->err = std::string("n2v: clearing the row marks: ") + hipGetErrorString(s); r = NTF_EHIP; }
    if (r) { hipFree(made->bits); hipFree(made->count); *made = n2v_rowlist(); }
    return r;
}
// marks the rows of n ids (k_n2v_touch; `hot`: the row a sizeable share of them names, -1 for none)
static void rowlist_mark(ntf_n2v* h, const int64_t* ids, int64_t n, int64_t hot) {
    if (n > 0) hipLaunchKernelGGL(k_n2v_touch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, ids, n, hot, h->rl.bits);
}
// the marked rows into rl.list (the caller has grown it to their bound), their number into rl.count; keep: the marks stay
static void rowlist_list(ntf_n2v* h, bool keep) {
    hipMemsetAsync(h->rl.count, 0, 8, h->st);
    hipLaunchKernelGGL((keep ? k_n2v_compact<false> : k_n2v_compact<true>), dim3((unsigned)((rowlist_words(h) + 255) / 256)), dim3(256), 0, h->st, h->rl.bits,
                       rowlist_words(h), h->rl.list, h->rl.count);
}
// the grid of a kernel that strides over the listed rows, one wave a row, for a list of at most `cap` rows
static dim3 rowlist_grid(int64_t cap) { return dim3((unsigned)std::min<int64_t>((std::max<int64_t>(cap, 1) + 3) / 4, 256 * 8)); }

extern "C" int ntf_n2v_set_optimizer(ntf_n2v* h, int32_t kind) {
    if (!h) return NTF_EINVAL;
    if (kind != 0 && kind != 1) FAIL(h, NTF_EINVAL, "n2v: optimizer kind must be 0 (dense Adam) or 1 (sparse Adam)");
    if (h->adam_t > 0 || h->pend_entries > 0) FAIL(h, NTF_ESTATE, "n2v: the optimizer is chosen before the first step and with no gradient pending");
    if (kind == 1 && h->lz.window) FAIL(h, NTF_ESTATE, "n2v: a lazy dense handle takes no sparse Adam (ntf_n2v_set_lazy(h, 0) first)");
    if (kind == 1) {
        n2v_rowlist made;
        if (int r = rowlist_make(h, &made)) return r;
        if (made.bits) h->rl = made;
    }
    h->opt = kind;
    return NTF_OK;
}

// lazy dense Adam on or off (include/opentf_amd.h).  Everything is allocated before anything of the handle changes: a refused call changes nothing
extern "C" int ntf_n2v_set_lazy(ntf_n2v* h, int32_t window) {
    if (!h) return NTF_EINVAL;
    if (window < 0) FAIL(h, NTF_EINVAL, "n2v: the lazy window is 0 (off) or a number of steps >= 1");
    if (h->opt == 1) FAIL(h, NTF_ESTATE, "n2v: lazy dense Adam is a mode of the dense optimizer; this handle runs sparse Adam");
    if (h->adam_t > 0 || h->pend_entries > 0) FAIL(h, NTF_ESTATE, "n2v: the lazy mode is chosen before the first step and with no gradient pending");
    if (window == 0 || window == h->lz.window) { h->lz.window = window; return NTF_OK; }
    HIPCHK(h, hipSetDevice(h->device));
    n2v_rowlist made; uint32_t* applied = nullptr; float2* ring = nullptr;
    int r = dev_alloc(h, &ring, window);
    if (!r && !h->lz.applied) r = dev_alloc(h, &applied, h->n);
    hipError_t s = !r && applied ? hipMemsetAsync(applied, 0, (size_t)h->n * 4, h->st) : hipSuccess;
    if (s != hipSuccess) { h->err = std::string("n2v: clearing the lazy state: ") + hipGetErrorString(s); r = NTF_EHIP; }
    if (!r) r = rowlist_make(h, &made);                       // its wait is the wait for `applied` too
    if (r) { hipFree(ring); hipFree(applied); return r; }
    if (h->lz.ring) hipFree(h->lz.ring);
    h->lz.ring = ring;
    if (applied) h->lz.applied = applied;
    if (made.bits) h->rl = made;
    h->lz.window = window; h->lz.base = 0;
    return NTF_OK;
}
extern "C" int ntf_n2v_lazy_state(ntf_n2v* h, uint32_t* applied, int64_t* steps, int64_t* flushes) {
    if (!h) return NTF_EINVAL;
    if (!h->lz.window) FAIL(h, NTF_ESTATE, "n2v: not a lazy handle (ntf_n2v_set_lazy)");
    HIPCHK(h, hipSetDevice(h->device));
    if (applied) {
        HIPCHK(h, hipMemcpyAsync(applied, h->lz.applied, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
    }
    if (steps) *steps = h->adam_t;
    if (flushes) *flushes = h->lz.flushes;
    return NTF_OK;
}

// node2vec's return / in-out parameters.  (1, 1) is the uniform walk again (k_n2v_walks, its slots, its bits); any other pair sends the walks through
// k_n2v_walks_biased.  Walks carry no state between calls, so the entry may come at any time and takes no step index.  A refused call changes nothing.
extern "C" int ntf_n2v_set_walk_bias(ntf_n2v* h, double p, double q) {
    if (!h) return NTF_EINVAL;
    if (!std::isfinite(p) || !std::isfinite(q) || p < 1e-4 || p > 1e4 || q < 1e-4 || q > 1e4) FAIL(h, NTF_EINVAL, "n2v: walk bias p and q must be finite and in [1e-4, 1e4]");
    if (h->m2v) FAIL(h, NTF_ESTATE, "m2v: a metapath handle takes no walk bias (MetaPath2Vec has no p / q)");
    if (p == 1.0 && q == 1.0) { h->biased = false; return NTF_OK; }
    if (h->rows_ascending < 0) {
        HIPCHK(h, hipSetDevice(h->device));
        int* d_bad = nullptr; int bad = 0;
        if (int r = dev_alloc(h, &d_bad, 1)) return r;
        hipError_t s = hipMemsetAsync(d_bad, 0, sizeof(int), h->st);
        if (s == hipSuccess && h->nnz > 1) {
            hipLaunchKernelGGL(k_n2v_rows_ascending, dim3((unsigned)((h->nnz - 1 + 255) / 256)), dim3(256), 0, h->st, h->rowptr, h->col, h->n, h->nnz, d_bad);
            s = hipGetLastError();
        }
        if (s == hipSuccess) s = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, h->st);
        if (s == hipSuccess) s = hipStreamSynchronize(h->st);
        hipFree(d_bad);
        if (s != hipSuccess) FAIL(h, NTF_EHIP, std::string("n2v: checking the order of the CSR rows: ") + hipGetErrorString(s));
        h->rows_ascending = bad ? 0 : 1;
    }
    if (!h->rows_ascending) FAIL(h, NTF_EINVAL, "n2v: a walk bias needs every CSR row's neighbour ids in ascending order (repeats allowed); this graph has a row that is not");
    // IEEE double, in this order of operations: a Python float computes the same bits (tests/n2v_bias_reference.py `thresholds`)
    const double ip = 1.0 / p, iq = 1.0 / q, mx = std::max(ip, std::max(1.0, iq));
    const double prob[3] = {ip / mx, 1.0 / mx, iq / mx};
    for (int k = 0; k < 3; ++k) h->bias_thr[k] = (unsigned long long)std::floor(prob[k] * 4294967296.0);      // in [1, 2^32] over the accepted range
    h->biased = true;
    return NTF_OK;
}

// Adam's constants at step t >= 1 (torch's defaults), in f64: what both launches below round their float arguments from
struct adam_consts { double b1, b2, bc1, bc2; float eps; };
static adam_consts adam_at(int64_t t) {
    const double b1 = 0.9, b2 = 0.999;
    return {b1, b2, 1.0 - std::pow(b1, (double)t), 1.0 - std::pow(b2, (double)t), 1e-8f};
}
// the dense step over the whole table; G is clear afterwards
static void launch_dense_adam(ntf_n2v* h, float lr) {
    const adam_consts c = adam_at(h->adam_t);
    const int64_t np = h->n * h->d;
    const int blocks = (int)std::min<int64_t>((np / 4 + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(k_n2v_adam, dim3(blocks), dim3(256), 0, h->st, h->W, h->G, h->M1, h->V2, np, lr / (float)c.bc1, (float)c.b1, (float)c.b2, c.eps, (float)std::sqrt(c.bc2));
}
// the sparse step: marked rows -> list (at most `cap` rows) -> sparse_adam on the listed rows; the marks and the rows of G are clear afterwards
static void launch_sparse_adam(ntf_n2v* h, float lr, int64_t cap) {
    const adam_consts c = adam_at(h->adam_t);
    const float step = (float)((double)lr * std::sqrt(c.bc2) / c.bc1);
    if (cap <= 0) return;
    rowlist_list(h, false);
    with_nv(h->d / 64, [&](auto nv) {
        hipLaunchKernelGGL(k_n2v_adam_rows<decltype(nv)::value>, rowlist_grid(cap), dim3(256), 0, h->st, h->W, h->G, h->M1, h->V2, h->rl.list, h->rl.count, h->d, step,
                           (float)(1.0 - c.b1), (float)(1.0 - c.b2), c.eps);
    });
}

// ---- lazy dense Adam, host side.  The listed rows (at most `cap`) brought to step adam_t
static void lazy_catchup_rows(ntf_n2v* h, int64_t cap) {
    const adam_consts c = adam_at(1);                         // b1, b2 and eps alone: every step's own two constants come from the ring
    with_nv(h->d / 64, [&](auto nv) {
        hipLaunchKernelGGL((k_n2v_catchup_rows<decltype(nv)::value, false>), rowlist_grid(cap), dim3(256), 0, h->st, h->W, h->G, h->M1, h->V2, h->lz.applied, h->lz.ring,
                           (float2*)nullptr, (uint32_t)h->lz.window, h->rl.list, h->rl.count, h->d, (uint32_t)h->adam_t, 0.f, (float)c.b1, (float)c.b2, c.eps, 0.f);
    });
}
// the full flush: every row to step adam_t, after which the ring is free again.  It reads no mark, so a pending gradient's marks survive it
static void lazy_flush(ntf_n2v* h) {
    if (h->adam_t == h->lz.base) return;                     // every row is there already
    const adam_consts c = adam_at(1);                         // b1, b2 and eps alone: every step's own two constants come from the ring
    const dim3 grid((unsigned)std::min<int64_t>((h->n + 3) / 4, 256 * 32)), block(256);
    with_nv(h->d / 64, [&](auto nv) {
        hipLaunchKernelGGL(k_n2v_catchup_all<decltype(nv)::value>, grid, block, 0, h->st, h->W, h->M1, h->V2, h->lz.applied, h->lz.ring, (uint32_t)h->lz.window, h->n, h->d,
                           (uint32_t)h->adam_t, (float)c.b1, (float)c.b2, c.eps);
    });
    h->lz.base = h->adam_t; h->lz.flushes += 1;
}
// the step of the batch on the listed rows (already at adam_t - 1, the step before): k_n2v_adam's two constants, rounded as launch_dense_adam rounds them, go to
// the kernel and from its first lane into the ring (the caller has made room in it).  G and the marks are clear afterwards
static void launch_lazy_adam(ntf_n2v* h, float lr, int64_t cap) {
    const adam_consts c = adam_at(h->adam_t);
    with_nv(h->d / 64, [&](auto nv) {
        hipLaunchKernelGGL((k_n2v_catchup_rows<decltype(nv)::value, true>), rowlist_grid(cap), dim3(256), 0, h->st, h->W, h->G, h->M1, h->V2, h->lz.applied, h->lz.ring,
                           h->lz.ring + h->adam_t % h->lz.window, (uint32_t)h->lz.window, h->rl.list, h->rl.count, h->d, (uint32_t)(h->adam_t - 1),
                           lr / (float)c.bc1, (float)c.b1, (float)c.b2, c.eps, (float)std::sqrt(c.bc2));
    });
    hipMemsetAsync(h->rl.bits, 0, (size_t)rowlist_words(h) * 4, h->st);
}

static void launch_pairs(ntf_n2v* h, const int64_t* rows, int64_t n_rows, int ctx, int positive) {
    if (n_rows <= 0 || ctx < 2) return;
    const float inv = 1.f / (float)(n_rows * (ctx - 1));
    const dim3 grid((unsigned)((n_rows + 3) / 4)), block(256);
    const int64_t dummy = h->mp.total;          // read by the dummy form alone
    with_nv(h->d / 64, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if (h->dummy_pairs) hipLaunchKernelGGL((k_n2v_pairs<NV, true>), grid, block, 0, h->st, h->W, rows, n_rows, ctx, h->d, inv, positive, dummy, h->G, h->d_loss);
        else hipLaunchKernelGGL((k_n2v_pairs<NV, false>), grid, block, 0, h->st, h->W, rows, n_rows, ctx, h->d, inv, positive, dummy, h->G, h->d_loss);
    });
}

// the window rows of a native batch: walks, negatives and both window launches into the scratch [pos walks | neg walks | pos windows | neg windows]; *win = the positive
// windows, the negative ones right behind.  pairs_now (dense): each sign's pairs behind its window launch - behind both, n2v measured slower (profiles/n2v_step_paths_check.md)
static int make_windows(ntf_n2v* h, int64_t B, int64_t pw, int64_t ng, int wl, int ctx, uint64_t step, bool pairs_now, const int64_t** win) {
    const int nw = wl + 1 - ctx;
    if (int r = need_rows(h, (pw + ng) * wl + (pw + ng) * nw * ctx)) return r;
    int64_t *rw_p = h->d_rows, *rw_n = rw_p + pw * wl, *win_p = rw_n + ng * wl, *win_n = win_p + pw * nw * ctx;
    launch_walks(h, B, pw, wl, step, rw_p);
    hipLaunchKernelGGL(k_n2v_windows, dim3((unsigned)((pw * nw * ctx + 255) / 256)), dim3(256), 0, h->st, rw_p, pw, wl, ctx, win_p);
    if (pairs_now) launch_pairs(h, win_p, pw * nw, ctx, 1);
    if (ng) {
        launch_negs(h, B, ng, wl, step, rw_n);
        hipLaunchKernelGGL(k_n2v_windows, dim3((unsigned)((ng * nw * ctx + 255) / 256)), dim3(256), 0, h->st, rw_n, ng, wl, ctx, win_n);
        if (pairs_now) launch_pairs(h, win_n, ng * nw, ctx, 0);
    }
    *win = win_p;
    return NTF_OK;
}
// the window rows of an injected call (the parity tests give them): the two uploads into the scratch the caller has sized
static int upload_windows(ntf_n2v* h, const int64_t* pos, int64_t n_pos, const int64_t* neg, int64_t n_neg, int ctx, const int64_t** win) {
    if (n_pos) HIPCHK(h, hipMemcpyAsync(h->d_rows, pos, n_pos * ctx * 8, hipMemcpyHostToDevice, h->st));
    if (n_neg) HIPCHK(h, hipMemcpyAsync(h->d_rows + n_pos * ctx, neg, n_neg * ctx * 8, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    *win = h->d_rows;
    return NTF_OK;
}

extern "C" int ntf_n2v_train_batch(ntf_n2v* h, const int64_t* batch, int32_t B, int32_t walk_length, int32_t context, int32_t walks_per_node, int32_t num_neg,
                                   float lr, const int64_t* inj_pos, int64_t n_pos, const int64_t* inj_neg, int64_t n_neg, int32_t apply, float* loss_out) {
    if (!h || walk_length < 2 || context < 2 || context > walk_length) return NTF_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    // every argument check (and stage_batch, which checks the start nodes) comes before the step index is taken and before anything on the device is touched:
    // a refused call changes nothing, so the draws of the calls after it are the ones they would have been without it
    int r;
    const bool injected = inj_pos || inj_neg;
    if (injected) {   // parity tests: the window rows themselves are given
        if ((n_pos > 0 && !inj_pos) || (n_neg > 0 && !inj_neg) || n_pos < 0 || n_neg < 0) FAIL(h, NTF_EINVAL, "n2v: injected rows missing or a negative row count");
        for (int64_t i = 0; i < n_pos * context; ++i) if (inj_pos[i] < 0 || inj_pos[i] >= h->n) FAIL(h, NTF_EINVAL, "n2v: injected node out of range");
        for (int64_t i = 0; i < n_neg * context; ++i) if (inj_neg[i] < 0 || inj_neg[i] >= h->n) FAIL(h, NTF_EINVAL, "n2v: injected node out of range");
        if ((r = need_rows(h, (n_pos + n_neg) * context))) return r;
    } else {
        if (!batch || B < 1 || walks_per_node < 1 || num_neg < 0) FAIL(h, NTF_EINVAL, "n2v: need a batch of B >= 1 start nodes, walks_per_node >= 1 and num_neg >= 0");
        if (m2v_too_long(h, walk_length)) FAIL(h, NTF_EINVAL, "m2v: a walk longer than the metapath needs a metapath that ends on its start type");
        if ((r = stage_batch(h, batch, B))) return r;
    }
    // the window rows of this call, positive and negative, and their entries: what k_n2v_touch runs over, and with the pending ones the bound of the row list
    const int64_t pw = (int64_t)B * walks_per_node, ng = pw * num_neg;
    const int64_t n_p = injected ? n_pos : pw * (walk_length + 1 - context), n_n = injected ? n_neg : ng * (walk_length + 1 - context), entries = (n_p + n_n) * context;
    const n2v_mode m = mode(h);
    if (m == N2V_LAZY && apply && h->adam_t >= 0xFFFFFFFFll) FAIL(h, NTF_ESTATE, "n2v: the step count of a lazy handle no longer fits its per-row counter (uint32)");
    if (m != N2V_DENSE && (r = dev_grow(h, &h->rl.list, &h->rl.cap, std::min<int64_t>(h->n, h->pend_entries + entries)))) return r;
    HIPCHK(h, hipMemsetAsync(h->d_loss, 0, 8, h->st));
    const uint64_t step = h->step++;
    const int64_t* win = nullptr;                            // windows: positive rows, then negative rows, back to back from `win` on
    const bool pairs_now = !injected && m == N2V_DENSE;      // make_windows has launched the pairs already
    if ((r = injected ? upload_windows(h, inj_pos, n_pos, inj_neg, n_neg, context, &win) : make_windows(h, B, pw, ng, walk_length, context, step, pairs_now, &win))) return r;
    h->win_p = win; h->win_n = win + n_p * context; h->n_win_p = n_p; h->n_win_n = n_n; h->win_ctx = context;
    // accumulate.  The pairs read W only at the rows the windows name, so a lazy handle first lists the marked rows - with those earlier apply = 0 calls marked
    // (current already: an empty loop) - and brings them to adam_t
    h->pend_entries += entries;
    const int64_t cap = std::min<int64_t>(h->n, h->pend_entries);
    if (m != N2V_DENSE) rowlist_mark(h, win, entries, h->m2v ? h->mp.total : (int64_t)-1);
    if (m == N2V_LAZY) { rowlist_list(h, true); lazy_catchup_rows(h, cap); }
    if (!pairs_now) { launch_pairs(h, h->win_p, n_p, context, 1); launch_pairs(h, h->win_n, n_n, context, 0); }
    if (apply) {
        if (m == N2V_LAZY && h->adam_t - h->lz.base == h->lz.window) lazy_flush(h);  // the ring is full: every row to adam_t, and its slots are free
        h->adam_t += 1;
        if (m == N2V_LAZY) launch_lazy_adam(h, lr, cap); else if (m == N2V_SPARSE) launch_sparse_adam(h, lr, cap); else launch_dense_adam(h, lr);
        h->pend_entries = 0;
    }
    if (loss_out) {
        double l = 0;
        HIPCHK(h, hipMemcpyAsync(&l, h->d_loss, 8, hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
        *loss_out = (float)l;
    }
    hipError_t s = hipGetLastError();
    if (s != hipSuccess) FAIL(h, NTF_EHIP, std::string("n2v kernel launch: ") + hipGetErrorString(s));
    return NTF_OK;
}

extern "C" int ntf_n2v_get(ntf_n2v* h, int what, float* host) {   // what: 0 = embedding.weight, 1 = its gradient (as the last batch with apply = 0 left it)
    if (!h || !host || what < 0 || what > 1) return NTF_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->lz.window && what == 0) lazy_flush(h);         // the table a reader sees is dense Adam's at step adam_t
    HIPCHK(h, hipStreamSynchronize(h->st));
    HIPCHK(h, hipMemcpy2D(host, (size_t)h->d_user * 4, what ? h->G : h->W, (size_t)h->d * 4, (size_t)h->d_user * 4, (size_t)h->n, hipMemcpyDeviceToHost));
    if (what) {   // reading the gradient consumes it, and with it the marks of the rows it named
        HIPCHK(h, hipMemsetAsync(h->G, 0, (size_t)h->n * h->d * 4, h->st));
        if (h->rl.bits) HIPCHK(h, hipMemsetAsync(h->rl.bits, 0, (size_t)rowlist_words(h) * 4, h->st));
        h->pend_entries = 0;
    }
    return NTF_OK;
}

extern "C" int ntf_n2v_moments(ntf_n2v* h, float* exp_avg, float* exp_avg_sq) {   // Adam's two moments [num_nodes, d], either may be NULL; reads only
    if (!h) return NTF_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->lz.window) lazy_flush(h);
    HIPCHK(h, hipStreamSynchronize(h->st));
    const size_t row = (size_t)h->d_user * 4;
    if (exp_avg) HIPCHK(h, hipMemcpy2D(exp_avg, row, h->M1, (size_t)h->d * 4, row, (size_t)h->n, hipMemcpyDeviceToHost));
    if (exp_avg_sq) HIPCHK(h, hipMemcpy2D(exp_avg_sq, row, h->V2, (size_t)h->d * 4, row, (size_t)h->n, hipMemcpyDeviceToHost));
    return NTF_OK;
}

extern "C" int ntf_n2v_last_windows(ntf_n2v* h, int64_t* n_pos, int64_t* n_neg, int32_t* context, int64_t* pos_rows, int64_t* neg_rows) {
    if (!h || !n_pos || !n_neg || !context) return NTF_EINVAL;
    if (!h->win_ctx) FAIL(h, NTF_ESTATE, "n2v: no batch since the scratch was last reused (ntf_n2v_walks and ntf_n2v_edge_bce write over the window rows)");
    *n_pos = h->n_win_p; *n_neg = h->n_win_n; *context = h->win_ctx;
    HIPCHK(h, hipSetDevice(h->device));
    if (pos_rows && h->n_win_p) HIPCHK(h, hipMemcpyAsync(pos_rows, h->win_p, h->n_win_p * h->win_ctx * 8, hipMemcpyDeviceToHost, h->st));
    if (neg_rows && h->n_win_n) HIPCHK(h, hipMemcpyAsync(neg_rows, h->win_n, h->n_win_n * h->win_ctx * 8, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return NTF_OK;
}

extern "C" int ntf_n2v_edge_bce(ntf_n2v* h, const int64_t* src, const int64_t* dst, int64_t n, float* mean_bce) {
    if (!h || !src || !dst || n < 1 || !mean_bce) return NTF_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    for (int64_t i = 0; i < n; ++i) if (src[i] < 0 || src[i] >= h->n || dst[i] < 0 || dst[i] >= h->n) FAIL(h, NTF_EINVAL, "n2v: edge endpoint out of range");
    int r = need_rows(h, 2 * n); if (r) return r;
    const int64_t cap = std::min<int64_t>(h->n, 2 * n);
    const bool lazy_rows = h->lz.window > 0 && h->pend_entries == 0;       // no gradient pending: the bitmap is free for the endpoints
    if (lazy_rows && (r = dev_grow(h, &h->rl.list, &h->rl.cap, cap))) return r;
    HIPCHK(h, hipMemcpyAsync(h->d_rows, src, n * 8, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(h->d_rows + n, dst, n * 8, hipMemcpyHostToDevice, h->st));
    if (lazy_rows) {                                        // only the rows read are brought to adam_t
        rowlist_mark(h, h->d_rows, 2 * n, -1);
        rowlist_list(h, false);
        lazy_catchup_rows(h, cap);
    } else if (h->lz.window) lazy_flush(h);                 // a gradient is pending and its marks must survive: the full flush reads none
    HIPCHK(h, hipMemsetAsync(h->d_loss + 1, 0, 8, h->st));
    hipLaunchKernelGGL(k_n2v_edge_bce, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, h->st, h->W, h->d_rows, h->d_rows + n, n, h->d, h->d_loss + 1);
    double l = 0;
    HIPCHK(h, hipMemcpyAsync(&l, h->d_loss + 1, 8, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    *mean_bce = (float)(l / (double)n);
    return NTF_OK;
}
