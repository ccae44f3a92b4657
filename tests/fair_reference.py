"""The fair stage's contract (include/opentf_amd_fair.h) restated as plain sequential Python: DetGreedy, DetCons and DetRelaxed re-ranking and the NDKL / skew
measures of Geyik, Ambler and Kenthapadi, "Fairness-aware ranking in search and recommendation systems", KDD 2019.  The reference's own stage needs a submodule
that was never vendored, so the published algorithms are restated here and THIS file is the pin (as tests/n2v_bias_reference.py is for the biased walks).

A row: `groups[j]` = the group of the candidate at ranked position j (best first), `p[g]` = the target share of group g.  Scores are never compared; everything
is integer logic on positions plus Python-float (IEEE double) products and quotients, math.floor / ceil / log / log2.

TEST INFRASTRUCTURE ONLY: imports nothing from opentf_amd.
"""
import math

DET_GREEDY, DET_CONS, DET_RELAXED = 0, 1, 2
INF = float("inf")


def _div(a, b):
    """a / b as IEEE does it for a > 0: +inf for b == 0 (Python raises there)"""
    return a / b if b != 0.0 else INF


def _ceil(x):
    return x if x == INF else float(math.ceil(x))


def rerank_row(groups, p, algorithm, k_out):
    """-> the ranked positions [k_out] the algorithm emits for one row"""
    K, G = len(groups), len(p)
    assert 1 <= k_out <= K and algorithm in (DET_GREEDY, DET_CONS, DET_RELAXED)
    queue = [[] for _ in range(G)]                 # the untaken positions of every group, ascending: head[g] = queue[g][0]
    for j, g in enumerate(groups):
        queue[int(g)].append(j)
    cnt = [0] * G
    out = []
    for k in range(1, k_out + 1):
        x = [float(k) * float(p[g]) for g in range(G)]
        lo = [math.floor(v) for v in x]
        hi = [math.ceil(v) for v in x]
        live = [g for g in range(G) if queue[g]]
        A = [g for g in live if cnt[g] < lo[g]]
        B = [g for g in live if lo[g] <= cnt[g] < hi[g]]
        if A:
            g_star = min(A, key=lambda g: queue[g][0])
        elif B:
            if algorithm == DET_GREEDY:
                g_star = min(B, key=lambda g: queue[g][0])
            elif algorithm == DET_CONS:
                g_star = min(B, key=lambda g: (_div(float(hi[g]), float(p[g])), queue[g][0]))
            else:
                g_star = min(B, key=lambda g: (_ceil(_div(float(hi[g]), float(p[g]))), queue[g][0]))
        else:
            g_star = min(live, key=lambda g: queue[g][0])
        out.append(queue[g_star].pop(0))
        cnt[g_star] += 1
    return out


def rerank(cand_idx, cand_val, group, p, algorithm, k_out):
    """ntf_fair_rerank on nested lists / arrays: -> (out_idx, out_val or None, out_pos) as lists of rows; p is [1][G] or [n][G]"""
    out_idx, out_val, out_pos = [], [], []
    for i, ids in enumerate(cand_idx):
        pos = rerank_row([group[e] for e in ids], p[i if len(p) > 1 else 0], algorithm, k_out)
        out_pos.append(pos)
        out_idx.append([int(ids[j]) for j in pos])
        if cand_val is not None:
            out_val.append([cand_val[i][k] for k in range(k_out)])
    return out_idx, (out_val if cand_val is not None else None), out_pos


def metrics_row(groups, p, cutoffs):
    """-> (ndkl [n_cut], skew [n_cut][G], abs_ndkl [n_cut]) of one ranked row; abs_ndkl is the NDKL's chain over the ABSOLUTE KL terms (the scale of its
    rounding error, what a test's bound is stated in)"""
    G = len(p)
    c = [0] * G
    num = den = num_abs = 0.0
    ndkl, skew, abs_ndkl = {}, {}, {}
    for k in range(1, max(cutoffs) + 1):
        c[int(groups[k - 1])] += 1
        kl = kl_abs = 0.0
        for g in range(G):
            if c[g] > 0:
                d = c[g] / k
                t = d * math.log(d / p[g]) if p[g] != 0.0 else INF
                kl += t
                kl_abs += abs(t)
        w = 1.0 / math.log2(k + 1)
        num += w * kl
        num_abs += w * kl_abs
        den += w
        if k in cutoffs:
            ndkl[k] = num / den
            abs_ndkl[k] = num_abs / den
            row = []
            for g in range(G):
                if c[g] == 0:
                    row.append(-INF if p[g] > 0.0 else 0.0)
                elif p[g] == 0.0:
                    row.append(INF)
                else:
                    row.append(math.log((c[g] / k) / p[g]))
            skew[k] = row
    return [ndkl[k] for k in cutoffs], [skew[k] for k in cutoffs], [abs_ndkl[k] for k in cutoffs]


def metrics(idx, group, p, cutoffs):
    """ntf_fair_metrics on nested lists / arrays: -> (ndkl [n][n_cut], skew [n][n_cut][G], abs_ndkl [n][n_cut])"""
    res = [metrics_row([group[e] for e in ids], p[i if len(p) > 1 else 0], list(cutoffs)) for i, ids in enumerate(idx)]
    return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
