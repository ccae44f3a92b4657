/* Link decode over a resident node-embedding table on the device: for a batch of query nodes, the logit and the probability of an edge to every row of a
 * candidate block, ranked - the `test` of a random-walk Gnn (node2vec / metapath2vec) used as a recommender: every member scored for a team.  The decode is PyG's
 * dot-product link decode, sigmoid(<E[query], E[candidate]>), the logit of ntf_n2v_edge_bce.  A header of its own beside opentf_amd.h (whose status codes
 * and workspace default it uses): the entries live in the same libopentf_amd.so and do not change NTF_ABI_VERSION.
 *
 * Table.  f32 [n_rows, d] on the host, 1 <= d <= 256, 1 <= n_rows <= 2^31 - 1, every value finite.  ntf_link_create uploads it once; on the device the rows are
 *   padded to a multiple of 32 floats with exact zeros, as ntf_knn does.
 * Candidates.  The contiguous block [cand_lo, cand_hi) of table rows, C = cand_hi - cand_lo >= 1.  Candidate id j is table row cand_lo + j.
 * Queries.  Exactly one of two forms a call:
 *   rows    q_rows [n]: query i is table row q_rows[i], anywhere in the table (inside the candidate block or not), gathered on the device;
 *   pooled  a CSR, q_ptr [n + 1] and q_items (table rows): query i is the mean pool of the rows q_items[q_ptr[i] .. q_ptr[i + 1]), bit for bit what
 *           ntf_gather_meanpool returns for the same CSR over the same table (a CSR-ordered f32 sum, then one division by the count; it is that kernel).
 *           An empty row is refused (0 / 0).
 * Logit.  x(i, j) = one k-ordered fmaf chain from +0 over k = 0 .. d-1: acc = fmaf(t_j[k], q_i[k], acc) (what v_mfma_f32_32x32x2_f32 computes; pad columns add
 *   exact zeros).  -0.0f is returned as +0.0f and ties with it.  The bits of x(i, j) depend on the two vectors alone - not on the tile, range, group, batch split
 *   or workspace budget.  (Finite rows can still overflow the chain: such a logit is returned as computed.)
 * Probability.  p = link_sigmoid(x) = 1.f / (1.f + expf(-x)) in f32, ONE device function behind every output: the p of the same x has the same bits everywhere.
 *   Accuracy, for |x| <= 30 (no operand or result subnormal), u = 2^-24: expf is within 1 ulp (HIP's documented bound), a relative error <= 2 u, which the
 *   addition 1 + e passes on scaled by e / (1 + e) < 1; the addition and the division (IEEE, correctly rounded as compiled: no fast-math flag) add u each:
 *   |p - p*| <= (4 u + 2^-40) p*  against p* = 1 / (1 + exp(-x)) of the returned f32 x in exact arithmetic (2^-40 covers the second-order terms, < 6 u^2).
 * Ranking.  By the logit, not by p (p saturates to 1.0f from x of about 17): largest x first, equal x (as real numbers) by ascending candidate id.  link_sigmoid
 *   is non-decreasing, so this is a valid top-K of the probabilities.
 * ntf_link_topk: out_idx [n, K] int32 candidate ids (required), out_logit / out_prob [n, K] (either may be NULL), 1 <= K <= 2048.  With K > C the trailing
 *   slots hold id -1, logit -inf, probability 0.
 * ntf_link_dense: out_logit and / or out_prob [n, C] row-major on the host (at least one), produced group by group through the same workspace: [n, C] never
 *   exists on the device.
 * Workspace.  Planned as ntf_knn_query plans it (opentf_amd.h: the 32-query x 256-row unit of 32 KiB, the g / r formulas with C for n_rows), workspace_bytes = 0
 *   meaning NTF_KNN_WORKSPACE_BYTES; the device holds no larger workspace.  Per range the logits of the group go to the workspace; top-K: each query's K largest of
 *   the range are selected and merged into its running list by the 64-bit composite (order-preserving key of x << 32 | 0x7fffffff - j) - a total order; dense: the
 *   workspace rows are copied out, link_sigmoid applied in place between the two copies.
 * Purity.  No table is written.  The result of query i is a pure function of (table, candidate block, query vector, K): bit-identical under any budget, any split
 *   or permutation of the queries, and either query form when a pooled vector has a row's bits.
 * device_ms (nullable): stream time of the call from the query gather to the last kernel (dense: the copies to the host between them included).
 * NTF_EINVAL with every output untouched (message: ntf_link_last_error; of a failed create: ntf_link_last_error(NULL)) for: a NULL required pointer; both or
 *   neither query forms (q_rows against q_ptr + q_items; one of q_ptr / q_items alone); n < 1; K outside [1, 2048]; d outside [1, 256]; cand_lo < 0,
 *   cand_hi > n_rows or C < 1; a query row or pooled item outside [0, n_rows); q_ptr[0] != 0, a non-monotone q_ptr or an empty pooled row; a non-finite table
 *   value (create); workspace_bytes negative or below the 32 KiB unit.  No HIP device: NTF_EHIP from create (there is no CPU fallback). */
#ifndef OPENTF_AMD_LINK_H
#define OPENTF_AMD_LINK_H
#include "opentf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntf_link ntf_link;
int  ntf_link_create(int device, const float* table /* [n_rows, d] host */, int64_t n_rows, int32_t d,
                     int64_t cand_lo, int64_t cand_hi, ntf_link** out);
void ntf_link_destroy(ntf_link* h);
const char* ntf_link_last_error(const ntf_link* h);           /* NULL: of a failed create */
int  ntf_link_topk (ntf_link* h, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const int64_t* q_items,
                    int32_t K, int64_t workspace_bytes, int32_t* out_idx, float* out_logit, float* out_prob, double* device_ms);
int  ntf_link_dense(ntf_link* h, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const int64_t* q_items,
                    int64_t workspace_bytes, float* out_logit, float* out_prob, double* device_ms);

#ifdef __cplusplus
}
#endif
#endif /* OPENTF_AMD_LINK_H */
