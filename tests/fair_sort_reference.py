"""The contract of include/opentf_amd_fairsort.h restated as plain sequential Python: DetConstSort (Algorithm 3 of Geyik, Ambler and Kenthapadi, KDD 2019, with
the two departures the header writes down) and the InfeasibleIndex / InfeasibleCount measures.  A literal transcription: the insertion is the swap loop, one swap
at a time, not the device's scan.  THIS file is the pin, as tests/fair_reference.py is for the other three re-rankers.

A row: `groups[j]` = the group of the candidate at ranked position j (best first), `p[g]` = the target share of group g.  Scores are never compared; everything is
integer logic on positions plus one Python-float (IEEE double) product and math.floor.

TEST INFRASTRUCTURE ONLY: imports nothing from opentf_amd.
"""
import math


def _guard(deadline, r):
    """may an entry with this deadline move down to rank r?  The header's guard (a test passes the paper's printed one instead, to show what it breaks)"""
    return deadline >= r


def constsort_row(groups, p, k_out, guard=_guard, stats=None):
    """-> (positions [k_out], tail count, deadlines [k_out - tail count]) of one row; stats (a dict) receives 'longest': the most swaps one insertion made"""
    K, G = len(groups), len(p)
    assert 1 <= k_out <= K
    queue = [[] for _ in range(G)]                 # the untaken positions of every group, ascending: head[g] = queue[g][0]
    for j, g in enumerate(groups):
        queue[int(g)].append(j)
    pos, dl = [], []                               # the list L: pos[r - 1], dl[r - 1] at rank r
    mn = [0] * G
    longest = 0
    for k in range(1, k_out + G + 2):
        if len(pos) == k_out:
            break
        t = [math.floor(float(k) * float(p[g])) for g in range(G)]
        C = [g for g in range(G) if queue[g] and t[g] > mn[g]]
        mn = t
        for g in sorted(C, key=lambda g: queue[g][0]):
            if len(pos) == k_out:
                break
            j = queue[g].pop(0)
            pos.append(j); dl.append(k)
            r, swaps = len(pos), 0
            while r > 1 and guard(dl[r - 2], r) and pos[r - 2] > j:
                pos[r - 2], pos[r - 1] = pos[r - 1], pos[r - 2]
                dl[r - 2], dl[r - 1] = dl[r - 1], dl[r - 2]
                r -= 1; swaps += 1
            longest = max(longest, swaps)
    deadlines = list(dl)
    tail = 0
    while len(pos) < k_out:
        g = min((g for g in range(G) if queue[g]), key=lambda g: queue[g][0])
        pos.append(queue[g].pop(0)); tail += 1
    if stats is not None:
        stats["longest"] = max(stats.get("longest", 0), longest)
    return pos, tail, deadlines


def constsort(cand_idx, group, p, k_out, stats=None):
    """ntf_fair_constsort on nested lists / arrays: -> (out_idx, out_pos, out_tail) as lists of rows; p is [1][G] or [n][G]"""
    out_idx, out_pos, out_tail = [], [], []
    for i, ids in enumerate(cand_idx):
        pos, tail, _ = constsort_row([group[e] for e in ids], p[i if len(p) > 1 else 0], k_out, stats=stats)
        out_pos.append(pos); out_tail.append(tail)
        out_idx.append([int(ids[j]) for j in pos])
    return out_idx, out_pos, out_tail


def infeasible_row(groups, p, cutoffs):
    """-> (InfeasibleIndex [n_cut], InfeasibleCount [n_cut]) of one ranked row"""
    G = len(p)
    c = [0] * G
    index = count = 0
    at = {}
    for k in range(1, max(cutoffs) + 1):
        c[int(groups[k - 1])] += 1
        viol = sum(1 for g in range(G) if c[g] < math.floor(float(k) * float(p[g])))
        index += 1 if viol else 0
        count += viol
        at[k] = (index, count)
    return [at[k][0] for k in cutoffs], [at[k][1] for k in cutoffs]


def infeasible(idx, group, p, cutoffs):
    """ntf_fair_infeasible on nested lists / arrays: -> (index [n][n_cut], count [n][n_cut])"""
    res = [infeasible_row([group[e] for e in ids], p[i if len(p) > 1 else 0], list(cutoffs)) for i, ids in enumerate(idx)]
    return [r[0] for r in res], [r[1] for r in res]
