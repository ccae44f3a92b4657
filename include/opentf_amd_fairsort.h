/* DetConstSort re-ranking (Algorithm 3 of Geyik, Ambler and Kenthapadi, "Fairness-aware ranking in search and recommendation systems", KDD 2019) and the
 * paper's feasibility measures, InfeasibleIndex and InfeasibleCount, on the device: the fourth re-ranker of the fair stage and the measure that states the
 * guarantee it gives.  A header of its own beside opentf_amd_fair.h, whose limits (NTF_FAIR_MAX_K, NTF_FAIR_MAX_GROUPS), argument conventions and status codes
 * it uses: the two entries are handle-less, live in the same libopentf_amd.so and do not change NTF_ABI_VERSION.  ntf_fair_rerank keeps refusing every
 * algorithm code but its three.
 *
 * ntf_fair_constsort, row by row (rows are independent).  Candidates, groups, head[g] and "exhausted" are as in opentf_amd_fair.h.  "Better" means the smaller
 * input position (the input is ranked best first): scores are never compared, so cand_val may be NULL and tied scores cannot make the result ambiguous; the
 * paper's score[a] < score[b] is pos[a] > pos[b].  Everything is integer logic on positions plus one IEEE f64 product.
 * State: the list L (1-based ranks, empty at first), one deadline per entry of L, cnt[g] = 0, min[g] = 0.
 * For k = 1, 2, .., K_out + G + 1, stopping as soon as |L| == K_out (also in the middle of a step):
 *   t_g = floor((double)k * p_g) (one IEEE multiplication);
 *   C = {g not exhausted: t_g > min[g]};  then min[g] = t_g for every g, exhausted or not;
 *   for the groups of C in ascending order of head[g] (the paper: "by the score of their next candidate, descending"):
 *     j = head[g] is appended at rank r = |L| + 1 with deadline k;
 *     while r > 1 and the entry at rank r - 1 has deadline >= r and position > j: the two entries swap, deadlines included, and r = r - 1;
 *     cnt[g] += 1;  head[g] advances.
 * Tail (reachable only through an exhausted group or a p_g too small to fall due within the loop): while |L| < K_out the untaken candidate with the smallest
 * position is appended, with no swap; out_tail[i] is the number of ranks filled this way.
 * out_pos[i, r-1] = the position at rank r;  out_idx[i, r-1] = cand_idx[i, that position];  out_val[i, r-1] = cand_val[i, r-1] (the convention of
 * ntf_fair_rerank: the r-th largest score goes to the r-th re-ranked expert).  Heads are distinct positions, so the order within C is unique and the result is
 * one deterministic permutation prefix of the row (bit-identical under any split of the rows over calls).
 * An entry moves down only past the guard "deadline >= r", r being the rank it would move to, so no entry ever sits below its deadline: in a row where no
 * group runs out of candidates while one is due (every group g holding at least floor((K_out + G + 1) * p_g) candidates is enough), the first k ranks hold at
 * least floor(k * p_g) entries of every group g for every k, i.e. ntf_fair_infeasible of the result is 0 at every cutoff, and out_tail is 0.  A group that
 * runs out cannot be given what it is owed by any re-ranker; out_tail == 0 alone does not exclude that (p = [0.5, 0.5], groups [0,0,0,1], K_out = 4: the
 * loop's last steps fill the list, out_tail is 0, and group 1 is one short at rank 4).
 *
 * Two departures from the paper's printed pseudocode.
 *   1. The swap guard.  The paper prints maxIndices[start - 1] >= start with 0-based slots, which lets an entry due by rank D end at rank D + 1 and so breaks
 *      the feasibility the paper proves (p = [0.5, 0.5], groups by position [0,0,0,1,1,1]: the printed guard gives positions [0,1,3,..] and misses group 1 at
 *      k = 2; the guard above gives [0,3,1,4,2,5]).  The guard above is the one under which "no entry sits below its deadline" is an invariant.
 *   2. The loop end.  The paper's `while lastEmpty <= kmax` overshoots K_out; exactly K_out ranks come out here.
 *
 * ntf_fair_infeasible, of a ranked list (the original or a re-ranked one).  c_g(k) = the number of group-g entries among the first k, as in ntf_fair_metrics;
 * viol_g(k) = c_g(k) < floor((double)k * p_g):
 *   out_index[i, c] = #{k in 1 .. cutoff_c : viol_g(k) for some g}            (InfeasibleIndex)
 *   out_count[i, c] = sum over k = 1 .. cutoff_c of #{g : viol_g(k)}          (InfeasibleCount)
 *
 * Status codes and refusals are those of opentf_amd_fair.h.  NTF_EINVAL with every output untouched for each refusal that header lists for the shared
 * arguments (ids, n, K, group, n_experts, G, p, n_p, K_out, cutoffs, n_cut) and for: out_idx null; out_val given without cand_val; out_index and out_count
 * both null.  No HIP device: NTF_EHIP (there is no CPU fallback). */
#ifndef OPENTF_AMD_FAIRSORT_H
#define OPENTF_AMD_FAIRSORT_H
#include "opentf_amd_fair.h"
#ifdef __cplusplus
extern "C" {
#endif

int ntf_fair_constsort(int device,
                       const int32_t* cand_idx /* [n, K] host, ranked best first */, const float* cand_val /* [n, K] or NULL */,
                       int64_t n, int32_t K,
                       const uint8_t* group /* [n_experts] host, values < G */, int64_t n_experts, int32_t G,
                       const double* p /* [n_p, G] host */, int64_t n_p /* 1: one target for all rows; n: one per row */,
                       int32_t K_out /* 1 .. K */,
                       int32_t* out_idx /* [n, K_out] */, float* out_val /* [n, K_out] or NULL */, int32_t* out_pos /* [n, K_out] or NULL */,
                       int32_t* out_tail /* [n] or NULL: ranks filled by the tail rule */);

int ntf_fair_infeasible(int device, const int32_t* idx /* [n, K] host */, int64_t n, int32_t K,
                        const uint8_t* group, int64_t n_experts, int32_t G, const double* p, int64_t n_p,
                        const int32_t* cutoffs, int32_t n_cut /* <= 8, each in [1, K] */,
                        int32_t* out_index /* [n, n_cut] or NULL */, int32_t* out_count /* [n, n_cut] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OPENTF_AMD_FAIRSORT_H */
