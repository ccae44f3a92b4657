"""The fair stage of the reference's pipeline (cmd=[train,test,eval,fair]) on the MI355X: fairness-aware re-ranking of ranked expert lists (DetGreedy, DetCons,
DetRelaxed, DetConstSort) and the NDKL / skew / infeasible measures of a ranked list, after Geyik, Ambler and Kenthapadi, "Fairness-aware ranking in search and
recommendation systems", KDD 2019.  The per-row work goes through `ntf_fair_rerank` / `ntf_fair_metrics` (include/opentf_amd_fair.h) and `ntf_fair_constsort` /
`ntf_fair_infeasible` (include/opentf_amd_fairsort.h) of libopentf_amd.so; this module prepares their inputs - the protected attribute of every expert and the
target distribution - and shapes their outputs.

The reference's own stage lives in a git submodule (src/Adila) that is absent from it, so three things here are unpinned choices, each kept in ONE function:
the popularity rule (`popularity_groups`), the keys of the stage's config (`FairSpec.from_cfg`) and the names of the files it leaves (`fair_stem`); INTEGRATION.md
says so.  Timing against the sequential host loop it replaces: profiles/fair_bench.md.
"""
from __future__ import annotations

import os

import numpy as np
import scipy.sparse as sp

POPULARITY_NAMES = ("nonpopular", "popular")


def popularity_groups(member, rows=None):
    """-> (group uint8 [M], names): expert e is `popular` (label 1) when the number of teams of `rows` (None: all) that e is a member of exceeds the mean of that
    count over the experts with at least one such team, `nonpopular` (label 0) otherwise.  THE popularity rule (unpinned, see the module text)."""
    Y = sp.csr_matrix(member)
    if rows is not None:
        Y = Y[np.asarray(rows, dtype=np.int64)]
    count = np.bincount(Y.indices[Y.data != 0], minlength=Y.shape[1]).astype(np.int64)
    seen = count > 0
    mean = float(count[seen].mean()) if seen.any() else 0.0
    return (count > mean).astype(np.uint8), POPULARITY_NAMES


def load_groups(path, M):
    """-> (group uint8 [M], names) from a `.npy` of M integer labels: an attribute the matrices do not carry (gender, ..); the names are the labels' digits"""
    a = np.load(path, allow_pickle=False)
    if a.shape != (M,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{path}: expected {M} integer labels, got {a.dtype} {a.shape}")
    if a.min() < 0 or a.max() >= 64:
        raise ValueError(f"{path}: labels must lie in [0, 64), got [{a.min()}, {a.max()}]")
    return a.astype(np.uint8), tuple(str(g) for g in range(int(a.max()) + 1))


def target_distribution(notion, group, G, Y=None):
    """The shares the re-ranked lists aim at.  'dp' (demographic parity): [1, G], the groups' frequencies over all experts.  'eo' (equality of opportunity):
    [n, G], per team of Y (the truth rows, sparse) the groups' frequencies among its true members; a team without a member takes the 'dp' row."""
    group = np.asarray(group, dtype=np.int64).reshape(-1)
    dp = (np.bincount(group, minlength=G).astype(np.float64) / float(len(group))).reshape(1, G)
    if notion == "dp":
        return dp
    if notion != "eo":
        raise ValueError(f"unknown fairness notion {notion!r}: 'dp' or 'eo'")
    if Y is None:
        raise ValueError("notion 'eo' needs the truth rows Y")
    Y = sp.csr_matrix(Y)
    n = Y.shape[0]
    keep = Y.data != 0
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(Y.indptr))[keep]
    cnt = np.bincount(rows * G + group[Y.indices[keep]], minlength=n * G).reshape(n, G).astype(np.float64)
    tot = cnt.sum(axis=1, keepdims=True)
    return np.where(tot > 0, cnt / np.where(tot > 0, tot, 1.0), dp)


def rerank(ranked_idx, ranked_val, group, p, algorithm, k_max, device=0):
    """-> (idx [n, k_max] int32, val [n, k_max] f32 or None): the first k_max ranks of every row of ranked_idx [n, K] (best first) re-ranked by `algorithm`
    ('det_greedy', 'det_cons', 'det_relaxed', 'det_const_sort') towards the target p ([1, G] or [n, G]); the k-th largest score goes to the k-th re-ranked expert"""
    from .. import libntf
    if algorithm == libntf.FAIR_CONST_SORT:
        return libntf.fair_constsort(ranked_idx, ranked_val, group, p, k_out=int(k_max), device=device)
    return libntf.fair_rerank(ranked_idx, ranked_val, group, p, algorithm, k_out=int(k_max), device=device)


def fair_metrics(ranked_idx, group, p, cutoffs, device=0, names=None):
    """-> (per-instance DataFrame, mean DataFrame) with the columns ndkl_{c} and skew_{name}_{c} over the cutoffs c; names[g] (None: the labels' digits) names group g.
    An infinite value (a group with target 0 that appears, a group with a positive target that does not) is reported as it is."""
    import pandas as pd
    from .. import libntf
    cuts = [int(c) for c in cutoffs]
    ndkl, skew = libntf.fair_metrics(ranked_idx, group, p, cuts, device=device)
    G = skew.shape[2]
    names = [str(g) for g in range(G)] if names is None else list(names)[:G] + [str(g) for g in range(len(names), G)]
    cols = {f"ndkl_{c}": ndkl[:, q] for q, c in enumerate(cuts)}
    for g in range(G):
        for q, c in enumerate(cuts):
            cols[f"skew_{names[g]}_{c}"] = skew[:, q, g]
    df = pd.DataFrame(cols)
    return df, df.mean().to_frame("mean").rename_axis("metrics")


def fair_infeasible(ranked_idx, group, p, cutoffs, device=0):
    """-> (per-instance DataFrame, mean DataFrame) with the columns infeasible_index_{c} and infeasible_count_{c} over the cutoffs c: the ranks k <= c at which some
    group holds fewer than floor(k p_g) of the first k entries, and those shortfalls counted per group (InfeasibleIndex / InfeasibleCount of the paper)"""
    import pandas as pd
    from .. import libntf
    cuts = [int(c) for c in cutoffs]
    index, count = libntf.fair_infeasible(ranked_idx, group, p, cuts, device=device)
    cols = {f"infeasible_index_{c}": index[:, q] for q, c in enumerate(cuts)}
    cols.update({f"infeasible_count_{c}": count[:, q] for q, c in enumerate(cuts)})
    df = pd.DataFrame(cols)
    return df, df.mean().to_frame("mean").rename_axis("metrics")


class FairSpec:
    """what a fair config asks for, parsed once.  THE keys of the stage's config (unpinned): algorithm, notion, attribute, k_max, cutoffs, infeasible"""
    def __init__(self, algorithm="det_greedy", notion="dp", attribute="popularity", k_max=100, cutoffs=(2, 5, 10), infeasible=False):
        from .. import libntf
        algorithms = sorted(libntf.FAIR_ALGORITHMS) + [libntf.FAIR_CONST_SORT]
        if algorithm not in algorithms:
            raise ValueError(f"unknown fair algorithm {algorithm!r}: one of {algorithms}")
        if notion not in ("dp", "eo"):
            raise ValueError(f"unknown fairness notion {notion!r}: 'dp' or 'eo'")
        self.algorithm, self.notion, self.attribute, self.k_max = str(algorithm), str(notion), str(attribute), int(k_max)
        self.cutoffs = [int(c) for c in (cutoffs.split(",") if isinstance(cutoffs, str) else cutoffs)]
        if isinstance(infeasible, str):                  # a hand-written config may carry the word, and bool("false") is True
            if infeasible.strip().lower() not in ("true", "false"):
                raise ValueError(f"infeasible must be true or false, got {infeasible!r}")
            infeasible = infeasible.strip().lower() == "true"
        self.infeasible = bool(infeasible)

    @classmethod
    def from_cfg(cls, faircfg):
        from ..mdl.ntf import cfg_get
        d = cls()
        return cls(cfg_get(faircfg, "algorithm") or d.algorithm, cfg_get(faircfg, "notion") or d.notion, cfg_get(faircfg, "attribute") or d.attribute,
                   cfg_get(faircfg, "k_max") or d.k_max, cfg_get(faircfg, "cutoffs") or d.cutoffs, cfg_get(faircfg, "infeasible") or d.infeasible)

    def attribute_name(self):
        return "popularity" if self.attribute == "popularity" else os.path.splitext(os.path.basename(self.attribute))[0]

    def groups(self, member):
        return popularity_groups(member) if self.attribute == "popularity" else load_groups(self.attribute, member.shape[1])


def fair_stem(pred_path, spec):
    """THE names of the stage's files (unpinned): `<pred file>.{algorithm}.{notion}.{attribute}.k{k_max}` + `.rerank.pred` / `.faireval.csv` / `.utileval.csv`"""
    return f"{pred_path}.{spec.algorithm}.{spec.notion}.{spec.attribute_name()}.k{spec.k_max}"


def ranked_values(Y_, ranked):
    """the scores of the ranked ids [n, K] in a dense or scipy-sparse prediction matrix (an id a sparse row does not store scores 0), f32"""
    n = ranked.shape[0]
    rows = np.arange(n, dtype=np.int64)[:, None]
    if sp.issparse(Y_):
        return np.ascontiguousarray(np.asarray(sp.csr_matrix(Y_)[rows, ranked.astype(np.int64)].todense()), dtype=np.float32)
    return np.ascontiguousarray(np.asarray(Y_)[rows, ranked], dtype=np.float32)


def _before_after(before, after):
    import pandas as pd
    return pd.concat([before["mean"].rename("before"), after["mean"].rename("after")], axis=1).rename_axis("metrics")


def fair_predictions(teamsvecs, rows, Y_, spec, group, names, device=0):
    """One prediction matrix through the stage: ranked k_max deep, re-ranked, and both lists scored for fairness (NDKL, skew) and utility (the trec metrics at the
    spec's cutoffs, skill coverage where the dataset carries the expert-skill matrix).  -> (re-ranked ids [n, k_max], their values [n, k_max], faireval table,
    utileval table); the tables have one `before` and one `after` column."""
    import pandas as pd
    from . import metric
    Y = sp.csr_matrix(teamsvecs["member"])[np.asarray(rows, dtype=np.int64)]
    M = Y.shape[1]
    k_max = min(spec.k_max, M)
    cuts = [c for c in spec.cutoffs if c <= k_max]
    if not cuts:
        raise ValueError(f"no cutoff of {spec.cutoffs} lies within the {k_max} ranks the stage re-ranks")
    ranked = metric._ranked_topk(Y_, k_max)
    vals = ranked_values(Y_, ranked)
    p = target_distribution(spec.notion, group, len(names), Y)
    idx, val = rerank(ranked, vals, group, p, spec.algorithm, k_max, device=device)
    fair = _before_after(fair_metrics(ranked, group, p, cuts, device=device, names=names)[1], fair_metrics(idx, group, p, cuts, device=device, names=names)[1])
    if spec.infeasible:
        fair = pd.concat([fair, _before_after(fair_infeasible(ranked, group, p, cuts, device=device)[1], fair_infeasible(idx, group, p, cuts, device=device)[1])])
    ks = ",".join(str(c) for c in cuts)
    trec = [f"{f}_{ks}" for f in ("P", "recall", "ndcg_cut", "map_cut")]
    parts = []
    for r in (ranked, idx):
        mean = [metric.calculate_metrics(Y, None, None, False, trec, device=device, ranked=r)[1]]
        if teamsvecs.get("skillcoverage") is not None:
            X = teamsvecs["skill"] if sp.issparse(teamsvecs["skill"]) else teamsvecs["original_skill"]
            mean.append(metric.calculate_skill_coverage(sp.csr_matrix(X)[np.asarray(rows, dtype=np.int64)], None, teamsvecs["skillcoverage"], False, topks=ks,
                                                        device=device, ranked=r)[1])
        parts.append(pd.concat(mean, axis=0))
    return idx, val, fair, _before_after(parts[0], parts[1])
