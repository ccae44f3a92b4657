"""Mirror of the reference's `evl.metric` (src/evl/metric.py) with the per-instance work on the MI355X.

Same function names, arguments and returned DataFrames as the reference (`calculate_metrics` 5-35, `calculate_skill_coverage`
44-73); the reference builds python dicts for pytrec_eval row by row, here the ranked top-K lists go through
`ntf_rank_metrics` / `ntf_skill_coverage` of libopentf_amd.so.  `calculate_auc_roc` takes the host routes by default (sklearn as in the reference for dense
predictions, `micro_auc_sparse` for sparse ones); with a device ordinal - `score_predictions` passes one when NTF_AUC_DEVICE=1 - the micro-averaged AUC is
`micro_auc_device`: one streaming pass over the scores on the GPU (`ntf_auc_micro_dense` / `ntf_auc_micro_csr`), exact in integers.  The curve of `aucroc+` is
sklearn's by default; with `curve_device` - `score_predictions` passes one when NTF_ROC_DEVICE=1 - curve and AUC come from one such pass (`micro_roc_device`:
`ntf_roc_micro_dense` / `ntf_roc_micro_csr`, include/opentf_amd_roc.h): the corner list of the same curve, not sklearn's `drop_intermediate=True` point list.
`score_engine` (NTF_EVAL_ENGINE=1 in `Ntf.evaluate`) returns `score_predictions`' tables without a prediction matrix at all: the model's engine infers the rows and scores them
where they are (`Engine.score_rows`, `ntf_score_rows`).
Ties in the scores are ranked by ascending expert id (trec_eval: descending document name) — irrelevant for real-valued model
outputs, stated here because it is the one place the two can differ.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

TREC = ("P", "recall", "ndcg_cut", "map_cut", "success")
_ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."     # sklearn's message


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ranked_topk(Y_, k):
    """[n, k] expert ids by decreasing score (stable: ascending id among equal scores), from a dense array or a scipy CSR.  Sparse input (the
    top-K `.pred` files): ONE lexsort over all stored entries, no per-row Python work; only rows that store fewer than k entries (never the case
    for files test() wrote with topK >= k) are completed one by one with the lowest-id unstored experts, which all score 0."""
    n = Y_.shape[0]
    if sp.issparse(Y_):
        Y_ = sp.csr_matrix(Y_)
        cnt = np.diff(Y_.indptr)
        rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
        order = np.lexsort((Y_.indices, -Y_.data, rows))                 # by row, then score descending, then expert id
        pos = np.arange(len(order), dtype=np.int64) - np.repeat(Y_.indptr[:-1].astype(np.int64), cnt)   # rank inside the row
        keep = pos < k
        out = np.zeros((n, k), dtype=np.int32)
        out[rows[keep], pos[keep]] = Y_.indices[order][keep]
        for i in np.nonzero(cnt < k)[0]:
            cols = Y_.indices[Y_.indptr[i]:Y_.indptr[i + 1]]
            out[i, cnt[i]:] = np.setdiff1d(np.arange(Y_.shape[1], dtype=np.int64), cols)[: k - cnt[i]]
        return out
    Y_ = np.asarray(Y_)
    idx = np.argsort(-Y_, axis=1, kind="stable")[:, :k]
    return np.ascontiguousarray(idx, dtype=np.int32)


def _cutoffs(metrics, family):
    for m in metrics:
        if m.startswith(family + "_"):
            return [int(x) for x in m[len(family) + 1:].split(",")]
    return []


def calculate_metrics(Y, Y_, topK=None, per_instance=False, metrics=("P_2,5", "recall_2,5", "ndcg_cut_2,5"), device=0, ranked=None):
    """`ranked` [n, K] int32 (optional): the ranked expert ids themselves, e.g. `Engine.forward_topk`'s indices straight from the device; Y_ may
    then be None - no prediction matrix, sparse or dense, is formed or sorted on the host."""
    import pandas as pd
    from .. import libntf
    assert ranked is not None or Y.shape == Y_.shape, f"Shape mismatch between truth Y {Y.shape} vs preds Y_ {Y_.shape}!"
    Y = sp.csr_matrix(Y); Y.sort_indices()
    n, M = Y.shape
    fams = [f for f in TREC if _cutoffs(metrics, f)]
    cuts = sorted({k for f in fams for k in _cutoffs(metrics, f)})
    kmax = min(max(cuts), min(topK, M) if topK else M)
    if ranked is not None:
        top = np.ascontiguousarray(np.asarray(ranked)[:, :kmax], dtype=np.int32)
        assert top.shape == (n, kmax), f"ranked ids {np.asarray(ranked).shape} cover fewer than the {kmax} ranks the cutoffs need"
    else:
        top = _ranked_topk(Y_, kmax)
    ip, ix = np.ascontiguousarray(Y.indptr, dtype=np.int64), np.ascontiguousarray(Y.indices, dtype=np.int32)
    cu = np.ascontiguousarray(cuts, dtype=np.int32)
    out = np.zeros((n, 5 * len(cuts)), dtype=np.float32)
    rc = libntf.lib().ntf_rank_metrics(int(device), _ptr(top), n, top.shape[1], _ptr(ip), _ptr(ix), n, None, _ptr(cu), len(cuts), _ptr(out))
    if rc != 0:
        raise libntf.NtfError(f"ntf_rank_metrics failed ({rc})")
    return _metric_frames(out, cuts, metrics, per_instance)


def _metric_frames(out, cuts, metrics, per_instance):
    """(per-instance table or None, mean table) from k_rank_metrics' [n, 5 * len(cuts)] output over the sorted cutoffs `cuts`"""
    import pandas as pd
    cols, data = [], []
    for f in [f for f in TREC if _cutoffs(metrics, f)]:  # the reference's column order: family by family, each over its cutoffs
        for k in _cutoffs(metrics, f):
            cols.append(f"{f}_{k}"); data.append(out[:, TREC.index(f) * len(cuts) + cuts.index(k)].astype(np.float64))
    df = pd.DataFrame(np.stack(data, axis=1), columns=cols, index=[f"q{i}" for i in range(out.shape[0])])
    df_mean = df.mean().to_frame("mean").rename_axis("metrics")
    return (df if per_instance else None), df_mean


def micro_auc_sparse(Y, Y_):
    """Micro-averaged ROC AUC of a SPARSE score matrix against sparse 0/1 truth without densifying either: the Mann-Whitney statistic
    with mid-ranks, U = sum over positives of (#negatives scored lower + 0.5 #negatives scored equal), AUC = U / (P * N_neg).  All the
    entries a top-K prediction does not store are one tie group at score 0.  Equals sklearn's `roc_auc_score(Y.toarray(),
    Y_.toarray(), average='micro')` (what src/evl/metric.py:36-41 computes) — which needs the dense [n_test, M] pair."""
    Y = sp.csr_matrix(Y); Y_ = sp.csr_matrix(Y_)
    n, M = Y_.shape
    total = n * M
    P = int((Y.data != 0).sum())
    if P == 0 or P == total:
        raise ValueError(_ONE_CLASS)
    Yb = Y.copy(); Yb.data = (Yb.data != 0).astype(np.int8); Yb.eliminate_zeros(); Yb.sort_indices()
    S = Y_.copy(); S.sum_duplicates(); S.sort_indices()
    # label of every stored score: flat keys row * M + col looked up among the positives' keys
    key_s = (np.repeat(np.arange(n, dtype=np.int64), np.diff(S.indptr)) * M + S.indices.astype(np.int64))
    key_p = (np.repeat(np.arange(n, dtype=np.int64), np.diff(Yb.indptr)) * M + Yb.indices.astype(np.int64))
    is_pos = np.isin(key_s, key_p, assume_unique=True)
    scores = S.data.astype(np.float64)
    pos_stored = int(is_pos.sum())
    # tie groups over the stored scores plus the implicit zeros
    vals, inv = np.unique(scores, return_inverse=True)
    p_g = np.bincount(inv, weights=is_pos.astype(np.float64), minlength=len(vals))
    n_g = np.bincount(inv, minlength=len(vals)).astype(np.float64) - p_g
    imp_total = total - len(scores)
    imp_pos = P - pos_stored
    z = np.searchsorted(vals, 0.0)
    if z < len(vals) and vals[z] == 0.0:
        p_g[z] += imp_pos; n_g[z] += imp_total - imp_pos
    else:
        vals = np.insert(vals, z, 0.0); p_g = np.insert(p_g, z, imp_pos); n_g = np.insert(n_g, z, imp_total - imp_pos)
    neg_below = np.concatenate([[0.0], np.cumsum(n_g)[:-1]])
    U = float(np.sum(p_g * (neg_below + 0.5 * n_g)))
    return U / (float(P) * float(total - P))


def _auc_inputs(Y, Y_, who):
    """what the AUC and the curve entries take: (truth indptr, truth indices, n, M, scores) with scores a (indptr, indices, values) triple for a scipy sparse `Y_`
    and a contiguous f32 array for a dense one.  Raises as sklearn does for one class only, TypeError for a dense dtype other than f32 / f16."""
    assert Y.shape == Y_.shape, f"Shape mismatch between truth Y {Y.shape} vs preds Y_ {Y_.shape}!"
    if not sp.issparse(Y_):
        Y_ = np.asarray(Y_)
        if Y_.dtype not in (np.float32, np.float16):
            raise TypeError(f"{who} takes dense scores as float32 or float16, not {Y_.dtype}: a cast could merge values that are distinct")
    Yb = sp.csr_matrix(Y).copy(); Yb.data = (Yb.data != 0).astype(np.int8); Yb.eliminate_zeros(); Yb.sort_indices()
    n, M = Yb.shape
    if Yb.nnz == 0 or Yb.nnz == n * M:
        raise ValueError(_ONE_CLASS)
    ip, ix = np.ascontiguousarray(Yb.indptr, dtype=np.int64), np.ascontiguousarray(Yb.indices, dtype=np.int32)
    if sp.issparse(Y_):
        S = sp.csr_matrix(Y_).copy(); S.sum_duplicates(); S.sort_indices()
        scores = (np.ascontiguousarray(S.indptr, dtype=np.int64), np.ascontiguousarray(S.indices, dtype=np.int32), np.ascontiguousarray(S.data, dtype=np.float32))
    else:
        scores = np.ascontiguousarray(Y_, dtype=np.float32)      # f16 -> f32 is exact
    return ip, ix, n, M, scores


def micro_auc_device(Y, Y_, device=0, chunk_bytes=0, return_counts=False):
    """Micro-averaged ROC AUC on the device: what `micro_auc_sparse` / sklearn's `roc_auc_score(Y.toarray(), Y_.toarray(), average='micro')`
    (src/evl/metric.py:36-41) compute, from one streaming pass over the scores (`ntf_auc_micro_csr` for a scipy sparse `Y_`, whose unstored entries
    score 0; `ntf_auc_micro_dense` for a dense f32 or f16 array) - no dense truth matrix, no sort of the n * M pairs.  The library returns the integers
    P, N and U2 = sum over positives of (2 #negatives scored lower + #negatives scored equal); the AUC is U2 / (2 P N), one division in f64.  Dense
    input of any other dtype is refused: a cast to f32 could merge values that sklearn keeps apart.  `chunk_bytes`: device staging budget per upload
    (0: the library's default, NTF_AUC_CHUNK_BYTES).  return_counts: -> (auc, (P, N, U2)) with Python ints."""
    ip, ix, n, M, scores = _auc_inputs(Y, Y_, "micro_auc_device")
    from .. import libntf
    counts, auc = np.zeros(3, dtype=np.uint64), C.c_double()
    if isinstance(scores, tuple):
        sip, six, sv = scores
        rc = libntf.lib().ntf_auc_micro_csr(int(device), _ptr(sip), _ptr(six), _ptr(sv), n, M, _ptr(ip), _ptr(ix), n, None, int(chunk_bytes), _ptr(counts), C.byref(auc))
        name = "ntf_auc_micro_csr"
    else:
        rc = libntf.lib().ntf_auc_micro_dense(int(device), _ptr(scores), n, M, M, _ptr(ip), _ptr(ix), n, None, int(chunk_bytes), _ptr(counts), C.byref(auc))
        name = "ntf_auc_micro_dense"
    if rc != 0:
        raise libntf.NtfError(f"{name} failed ({rc})" + (": a NaN score, or an argument outside the contract" if rc == libntf.NTF_EINVAL else ""))
    return (auc.value, tuple(int(c) for c in counts)) if return_counts else auc.value


def micro_roc_device(Y, Y_, device=0, chunk_bytes=0, return_counts=False):
    """Micro-averaged ROC curve on the device, from the one streaming pass `micro_auc_device` makes (`ntf_roc_micro_csr` / `ntf_roc_micro_dense`,
    include/opentf_amd_roc.h): -> (fpr, tpr, thresholds), f64, f64 and f32, first point (0, 0, inf), last (1, 1); with return_counts also (P, N, U2) as Python ints,
    the integers `micro_auc_device` returns for the same input (AUC = U2 / (2 P N) = the polyline's own trapezoid).  fpr = fps / N and tpr = tps / P, one f64 division
    each.  The points are the corners of sklearn's `roc_curve(Y.toarray().ravel(), Y_.toarray().ravel())`: the same piecewise-linear curve, each point one of
    `roc_curve(..., drop_intermediate=False)`; not the `drop_intermediate=True` list, which keeps further points inside the horizontal runs.  Inputs as
    `micro_auc_device`: scipy sparse (unstored entries score 0) or dense f32 / f16, other dtypes refused."""
    ip, ix, n, M, scores = _auc_inputs(Y, Y_, "micro_roc_device")
    from .. import libntf
    P = len(ix)
    cap = 2 * P + 2
    fps, tps, thr = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.float32)
    npts, counts, auc = C.c_int64(), np.zeros(3, dtype=np.uint64), C.c_double()
    tail = (int(chunk_bytes), cap, _ptr(fps), _ptr(tps), _ptr(thr), C.byref(npts), _ptr(counts), C.byref(auc))
    if isinstance(scores, tuple):
        sip, six, sv = scores
        rc = libntf.lib().ntf_roc_micro_csr(int(device), _ptr(sip), _ptr(six), _ptr(sv), n, M, _ptr(ip), _ptr(ix), n, None, *tail)
        name = "ntf_roc_micro_csr"
    else:
        rc = libntf.lib().ntf_roc_micro_dense(int(device), _ptr(scores), n, M, M, _ptr(ip), _ptr(ix), n, None, *tail)
        name = "ntf_roc_micro_dense"
    if rc != 0:
        raise libntf.NtfError(f"{name} failed ({rc})" + (": a NaN score, or an argument outside the contract" if rc == libntf.NTF_EINVAL else ""))
    k = npts.value
    Pn, Nn, U2 = (int(c) for c in counts)
    curve = (fps[:k].astype(np.float64) / float(Nn), tps[:k].astype(np.float64) / float(Pn), thr[:k].copy())
    return curve + ((Pn, Nn, U2),) if return_counts else curve


def calculate_auc_roc(Y, Y_, curve=False, device=None, curve_device=None):
    """src/evl/metric.py:36-41.  Sparse predictions (the top-K `.pred` files) go through `micro_auc_sparse`; dense ones, and the curve
    itself, through sklearn as in the reference.  `device` (an ordinal; None: the host routes above): without the curve, sparse and dense
    f32 predictions go through `micro_auc_device` instead.  `curve_device` (an ordinal; None: sklearn's curve, also with `device`): with the curve,
    AUC (U2 / (2 P N)) and (fpr, tpr) of sparse and dense f32 predictions both come from the one device pass of `micro_roc_device` - the curve's corners, see there."""
    assert Y.shape == Y_.shape
    if curve and curve_device is not None and (sp.issparse(Y_) or np.asarray(Y_).dtype == np.float32):
        fpr, tpr, _, (P, N, U2) = micro_roc_device(Y, Y_, device=curve_device, return_counts=True)
        return U2 / (2.0 * float(P) * float(N)), (fpr, tpr)
    if device is not None and not curve and (sp.issparse(Y_) or np.asarray(Y_).dtype == np.float32):
        return micro_auc_device(Y, Y_, device=device), None
    if sp.issparse(Y_) and not curve:
        return micro_auc_sparse(Y, Y_), None
    from sklearn import metrics as skm
    dense = Y_.toarray() if sp.issparse(Y_) else np.asarray(Y_)
    auc = skm.roc_auc_score(Y.toarray(), dense, average="micro", multi_class="ovr")
    if curve:
        fpr, tpr, _ = skm.roc_curve(Y.toarray().ravel(), dense.ravel())
        return auc, (fpr, tpr)
    return auc, None


def calculate_skill_coverage(X, Y_, expertskillvecs, per_instance=False, topks="2,5,10", device=0, ranked=None):
    """`ranked` [n, K] int32 (optional, K >= min(max(topks), experts)): the ranked expert ids themselves, as in `calculate_metrics`; Y_ may then be None."""
    import pandas as pd
    from .. import libntf
    assert X.shape[0] == (Y_.shape[0] if ranked is None else np.asarray(ranked).shape[0])
    X = sp.csr_matrix(X); X.sort_indices()
    cov = sp.csr_matrix(expertskillvecs); cov.sort_indices()
    cuts = [int(k) for k in topks.split(",")]
    n, E = (Y_.shape if ranked is None else (X.shape[0], cov.shape[0]))
    empty = np.nonzero(np.diff(X.indptr) == 0)[0]
    if len(empty):  # 0 / 0 in the reference (ZeroDivisionError, src/evl/metric.py:69); a NaN here would silently poison the mean
        raise libntf.NtfError(f"skill coverage is undefined for instance {int(empty[0])}: it has no required skill ({len(empty)} such instance(s))")
    if ranked is not None:
        top = np.ascontiguousarray(np.asarray(ranked)[:, :min(max(cuts), E)], dtype=np.int32)
        assert top.shape == (n, min(max(cuts), E)), f"ranked ids {np.asarray(ranked).shape} cover fewer than the {min(max(cuts), E)} ranks the cutoffs need"
    else:
        top = _ranked_topk(Y_, min(max(cuts), E))
    out = np.zeros((n, len(cuts)), dtype=np.float32)
    cu = np.ascontiguousarray(cuts, dtype=np.int32)
    xs, xi = np.ascontiguousarray(X.indptr, dtype=np.int64), np.ascontiguousarray(X.indices, dtype=np.int32)
    cs, ci = np.ascontiguousarray(cov.indptr, dtype=np.int64), np.ascontiguousarray(cov.indices, dtype=np.int32)
    rc = libntf.lib().ntf_skill_coverage(int(device), _ptr(top), n, top.shape[1], _ptr(xs), _ptr(xi), n, None, _ptr(cs), _ptr(ci), E, _ptr(cu), len(cuts), _ptr(out))
    if rc != 0:
        raise libntf.NtfError(f"ntf_skill_coverage failed ({rc})")
    df = pd.DataFrame(out.astype(np.float64), columns=[f"skill_coverage_{k}" for k in cuts])
    return df, df.mean().to_frame("mean").rename_axis("metrics")


class EvalSpec:
    """what an eval config asks for (src/__config__.yaml eval section), parsed once"""
    def __init__(self, topK, per_instance, trec, other):
        self.topK, self.per_instance, self.trec = topK, bool(per_instance), list(trec or [])
        other = list(other or [])
        self.auc = next((m for m in other if "aucroc" in m), None)               # 'aucroc' or 'aucroc+' (+ = keep the curve)
        self.skc = next((m for m in other if "skill_coverage" in m), None)       # 'skill_coverage_2,5,10'

    @classmethod
    def from_cfg(cls, evalcfg):
        from ..mdl.ntf import cfg_get
        m = cfg_get(evalcfg, "metrics")
        return cls(cfg_get(evalcfg, "topK"), cfg_get(evalcfg, "per_instance"), cfg_get(m, "trec"), cfg_get(m, "other"))


def score_predictions(teamsvecs, rows, Y_, spec, device=0):
    """One prediction matrix against the truth rows `rows` of teamsvecs: (per-instance table, mean table, roc curve or None).  Row order of the mean table as the
    reference writes it: trec metrics, aucroc, skill coverage (src/mdl/ntf.py:57-84)."""
    import pandas as pd
    Y = teamsvecs["member"][rows]
    assert Y.shape == Y_.shape, f"Shape mismatch between truth Y {Y.shape} vs preds Y_ {Y_.shape}!"
    inst_parts, mean_parts, roc = [], [], None
    if spec.trec:
        df, df_mean = calculate_metrics(Y, Y_, spec.topK, spec.per_instance, spec.trec, device=device)
        inst_parts.append(df); mean_parts.append(df_mean)
    if spec.auc:
        on_device = os.environ.get("NTF_AUC_DEVICE", "0") == "1"      # read per call; off: the host routes, as before the device entry existed
        roc_on_device = os.environ.get("NTF_ROC_DEVICE", "0") == "1"  # likewise; only aucroc+ (the curve) reads it
        auc, roc = calculate_auc_roc(Y, Y_, curve=(spec.auc == "aucroc+"), device=device if on_device else None, curve_device=device if roc_on_device else None)
        mean_parts.append(pd.DataFrame({"mean": [auc]}, index=pd.Index(["aucroc"], name="metrics")))
    if spec.skc:
        X = teamsvecs["skill"] if sp.issparse(teamsvecs["skill"]) else teamsvecs["original_skill"]
        df, df_mean = calculate_skill_coverage(X[rows], Y_, teamsvecs["skillcoverage"], spec.per_instance, topks=spec.skc.replace("skill_coverage_", ""), device=device)
        inst_parts.append(df); mean_parts.append(df_mean)
    inst_parts = [d.reset_index(drop=True) for d in inst_parts if d is not None and not d.empty]
    inst = pd.concat(inst_parts, axis=1) if inst_parts else pd.DataFrame()
    mean = pd.concat(mean_parts, axis=0) if mean_parts else pd.DataFrame(columns=["mean"])
    mean.index.name = "metrics"
    return inst, mean, roc


def eval_engine_enabled():
    """NTF_EVAL_ENGINE=1 (read per call, off by default): `Ntf.evaluate` scores a model's predictions inside its engine (`score_engine`) instead of reading `.pred` files"""
    return os.environ.get("NTF_EVAL_ENGINE", "0") == "1"


def _engine_plan(spec, M):
    """How `score_engine` asks `Engine.score_rows` for what `spec` wants at M experts: (K, cutoffs of the call, K_out, reason).  K >= 1: the top-K-sparsified
    prediction test() writes with that topK, 0: the dense one.  `reason` (a string; the rest is None then) says why the spec stays with the file route."""
    if spec.auc == "aucroc+":
        return None, None, None, "aucroc+ keeps the ROC curve, which stays with sklearn"
    topK = int(spec.topK) if spec.topK else 0
    K = topK if 0 < topK < M else 0                 # test(): a topK of M or more, or none, writes the dense matrix
    if K > 2048:
        return None, None, None, f"topK = {K} is above the 2048 ranks the device ranks per row"
    cap = min(M, 2048)
    trec = sorted({k for f in TREC for k in _cutoffs(spec.trec, f)})
    skc = [int(k) for k in spec.skc.replace("skill_coverage_", "").split(",")] if spec.skc else []
    k_skc = min(max(skc), M) if skc else 0
    cuts = list(trec)
    if K == 0:
        if trec and max(trec) > cap:
            return None, None, None, f"a dense prediction is ranked {cap} deep at most, the cutoffs ask for {max(trec)}"
        if k_skc and (not cuts or k_skc > max(cuts)): cuts = sorted(set(cuts) | {k_skc})     # the ranked list of a dense call is max(cutoffs) wide
        if cuts and max(cuts) > cap:
            return None, None, None, f"a dense prediction is ranked {cap} deep at most, skill coverage asks for {k_skc}"
    elif k_skc > K:
        return None, None, None, f"skill coverage over {k_skc} ranks needs more than the {K} stored experts of a row"
    if len(cuts) > 8:
        return None, None, None, "more than 8 distinct cutoffs in one call"
    return K, cuts, k_skc, None


def score_engine(engine, teamsvecs, rows, spec, nmc, batch, device=0):
    """`score_predictions` without a prediction matrix: the engine (its parameters loaded, its seed set by the caller) infers `rows` in batches of `batch` and scores
    them where they are (`Engine.score_rows`: ranking metrics, exact integer micro AUC); the ranked ids come back only when the spec asks for skill coverage, which
    `ntf_skill_coverage` then computes from them.  Same (per-instance table, mean table, None) triple, column and row order as `score_predictions` on the `.pred`
    file test() writes with topK = spec.topK.  Raises for a spec `_engine_plan` leaves to the file route."""
    import pandas as pd
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
    member = teamsvecs["member"]
    M = member.shape[1]
    K, cuts, k_out, reason = _engine_plan(spec, M)
    if reason:
        raise ValueError(f"score_engine: {reason}")
    if spec.auc:
        P = int((sp.csr_matrix(member[rows]).data != 0).sum())
        if P == 0 or P == len(rows) * M:
            raise ValueError(_ONE_CLASS)
    res = engine.score_rows(rows, batch, nmc=nmc, K=K, cutoffs=cuts, auc=bool(spec.auc), K_out=k_out)
    inst_parts, mean_parts = [], []
    if spec.trec:
        trec = sorted({k for f in TREC for k in _cutoffs(spec.trec, f)})
        out = res.metrics
        if cuts != trec:     # a cutoff added for the width of the ranked list: its columns are dropped
            keep = [m * len(cuts) + cuts.index(k) for m in range(5) for k in trec]
            out = np.ascontiguousarray(out[:, keep])
        df, df_mean = _metric_frames(out, trec, spec.trec, spec.per_instance)
        inst_parts.append(df); mean_parts.append(df_mean)
    if spec.auc:
        mean_parts.append(pd.DataFrame({"mean": [res.auc]}, index=pd.Index(["aucroc"], name="metrics")))
    if spec.skc:
        X = teamsvecs["skill"] if sp.issparse(teamsvecs["skill"]) else teamsvecs["original_skill"]
        df, df_mean = calculate_skill_coverage(X[rows], None, teamsvecs["skillcoverage"], spec.per_instance, topks=spec.skc.replace("skill_coverage_", ""),
                                               device=device, ranked=res.idx)
        inst_parts.append(df); mean_parts.append(df_mean)
    inst_parts = [d.reset_index(drop=True) for d in inst_parts if d is not None and not d.empty]
    inst = pd.concat(inst_parts, axis=1) if inst_parts else pd.DataFrame()
    mean = pd.concat(mean_parts, axis=0) if mean_parts else pd.DataFrame(columns=["mean"])
    mean.index.name = "metrics"
    return inst, mean, None
