/* Fairness-aware re-ranking of ranked expert lists on the device, and the fairness measures of a ranked list: the `fair` stage of the reference's
 * cmd=[train,test,eval,fair] pipeline.  The algorithms are DetGreedy, DetCons and DetRelaxed with the NDKL and skew measures of Geyik, Ambler and
 * Kenthapadi, "Fairness-aware ranking in search and recommendation systems", KDD 2019.  A header of its own beside opentf_amd.h (whose status codes it
 * uses): the two entries are handle-less, live in the same libopentf_amd.so and do not change NTF_ABI_VERSION.
 *
 * ntf_fair_rerank, row by row (rows are independent).  Candidate j of row i is cand_idx[i, j], its group g_j = group[cand_idx[i, j]].  The input is ranked
 * best first, so the best remaining candidate of group g is the untaken j with the smallest position among those with g_j == g: head[g].  A group with none
 * left is exhausted.  Scores are never compared: the algorithm is integer logic on positions plus the f64 products below.  cnt[g] starts at 0.
 * For k = 1 .. K_out:
 *   x_g = (double)k * p_g (one IEEE multiplication), lo_g = floor(x_g), hi_g = ceil(x_g);
 *   A = {g not exhausted: cnt[g] < lo_g},  B = {g not exhausted: lo_g <= cnt[g] < hi_g};
 *   A non-empty:      g* = argmin over A of head[g]                                               (all three algorithms)
 *   else B non-empty: DetGreedy   g* = argmin over B of head[g]
 *                     DetCons     g* = argmin over B of hi_g / p_g (one IEEE division), ties to the smaller head[g]
 *                     DetRelaxed  g* = argmin over B of ceil(hi_g / p_g), ties to the smaller head[g]
 *   else:             g* = argmin over the non-exhausted groups of head[g]: the best remaining candidate (reachable through exhaustion only)
 *   j* = head[g*]:  out_pos[i, k-1] = j*;  out_idx[i, k-1] = cand_idx[i, j*];  out_val[i, k-1] = cand_val[i, k-1] (the k-th largest score goes to the k-th
 *   re-ranked expert: the values stay non-increasing along a row);  cnt[g*] += 1;  head[g*] advances.
 * Heads are distinct positions, so every argmin is unique: the result is one deterministic permutation prefix of the row, a pure function of the row, its
 * target and the algorithm (bit-identical under any split of the rows over calls).
 *
 * ntf_fair_metrics, of a ranked list (the original or the re-ranked one).  c_g(k) = the number of group-g entries among the first k, d = c_g(k) / k; all in f64:
 *   KL_k          = sum over g ascending with c_g(k) > 0 of d * ln(d / p_g)
 *   w_k           = 1 / log2(k + 1)
 *   ndkl[i, c]    = (sum over k = 1 .. c ascending of w_k * KL_k) / (sum over k = 1 .. c ascending of w_k)
 *   skew[i, c, g] = ln((c_g(c) / c) / p_g);  -inf when c_g(c) == 0 < p_g, +inf when p_g == 0 < c_g(c), 0.0 when both are 0.
 * A KL_k with p_g == 0 < c_g(k) is +inf and so is the NDKL: reported, not refused.
 *
 * p [n_p, G]: the target distribution, one row for all rows (n_p == 1) or one per row (n_p == n).
 * NTF_EINVAL with every output untouched for: a null required pointer; n < 1; K outside [1, NTF_FAIR_MAX_K]; K_out outside [1, K]; G outside
 * [1, NTF_FAIR_MAX_GROUPS]; n_p neither 1 nor n; an unknown algorithm; a candidate id outside [0, n_experts); a group label >= G; a p entry that is not finite
 * or lies outside [0, 1]; a p row whose sum differs from 1 by more than 1e-6 (an input sanity bound, not a tolerance of the result); n_cut outside [1, 8];
 * a cutoff outside [1, K]; both metric outputs null.  Repeated ids inside a row are not checked: they are separate candidates.
 * No HIP device: NTF_EHIP (there is no CPU fallback). */
#ifndef OPENTF_AMD_FAIR_H
#define OPENTF_AMD_FAIR_H
#include "opentf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define NTF_FAIR_MAX_GROUPS 64
#define NTF_FAIR_MAX_K      2048      /* = the deepest list the device ranks per row (SEL_MAX) */
enum { NTF_FAIR_DET_GREEDY = 0, NTF_FAIR_DET_CONS = 1, NTF_FAIR_DET_RELAXED = 2 };

int ntf_fair_rerank(int device, int32_t algorithm,
                    const int32_t* cand_idx /* [n, K] host, ranked best first */, const float* cand_val /* [n, K] or NULL */,
                    int64_t n, int32_t K,
                    const uint8_t* group /* [n_experts] host, values < G */, int64_t n_experts, int32_t G,
                    const double* p /* [n_p, G] host */, int64_t n_p /* 1: one target for all rows; n: one per row */,
                    int32_t K_out /* 1 .. K */,
                    int32_t* out_idx /* [n, K_out] */, float* out_val /* [n, K_out] or NULL */, int32_t* out_pos /* [n, K_out] or NULL */);

int ntf_fair_metrics(int device, const int32_t* idx /* [n, K] host */, int64_t n, int32_t K,
                     const uint8_t* group, int64_t n_experts, int32_t G, const double* p, int64_t n_p,
                     const int32_t* cutoffs, int32_t n_cut /* <= 8, each in [1, K] */,
                     double* out_ndkl /* [n, n_cut] or NULL */, double* out_skew /* [n, n_cut, G] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OPENTF_AMD_FAIR_H */
