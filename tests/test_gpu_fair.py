"""The fair stage on a real MI355X (opentf_amd/csrc/ntf_fair.hip, include/opentf_amd_fair.h, opentf_amd/evl/fair.py, Ntf.adila) against the pin
tests/fair_reference.py.  Re-ranking is integer logic plus single IEEE operations: positions, ids and values must be EQUAL.  The measures go through log / log2,
whose last bits differ between the device library and the host's libm: see `test_metrics_match_the_reference` for the bound.  Every shape is the smallest at
which one thing can break; random inputs come from fixed numpy seeds; each (case, algorithm) reference is computed once and shared."""
import functools
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse
import torch

import fair_reference as R
from conftest import golden

pytestmark = pytest.mark.gpu

EINVAL = -1            # NTF_EINVAL, include/opentf_amd.h
ALGS = {"det_greedy": R.DET_GREEDY, "det_cons": R.DET_CONS, "det_relaxed": R.DET_RELAXED}


def _zipf_groups(rng, n_experts, G):
    w = 1.0 / np.arange(1, G + 1) ** 1.5
    g = rng.choice(G, size=n_experts, p=w / w.sum()).astype(np.uint8)
    g[:G] = np.arange(G)                      # every label exists among the experts
    return g


def _rows(rng, n, K, pool):
    """n ranked rows of K distinct ids from `pool`, with non-increasing scores"""
    idx = np.stack([rng.choice(pool, size=K, replace=False) for _ in range(n)]).astype(np.int32)
    val = -np.sort(-rng.random((n, K)).astype(np.float32), axis=1)
    return idx, val


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(idx [n, K], val [n, K], group [n_experts], p [n_p, G], k_out)"""
    rng = np.random.default_rng({"one": 1, "two": 2, "per_row": 3, "deep": 4, "prefix": 5, "zero_p": 6, "quarters": 7, "halves": 8, "thirds": 9, "absent": 10}[name])
    if name == "one":                         # K = 1, G = 1: the loop runs once, one lane votes
        group = np.zeros(20, np.uint8); idx, val = _rows(rng, 7, 1, 20); p = np.array([[1.0]]); k_out = 1
    elif name == "two":                       # one full 64-wide pass over the row, two groups
        group = (rng.random(300) < 0.3).astype(np.uint8); idx, val = _rows(rng, 33, 64, 300); p = np.array([[0.6, 0.4]]); k_out = 64
    elif name == "per_row":                   # K no multiple of 64, n no multiple of the rows of a workgroup, one target per row
        group = _zipf_groups(rng, 500, 3); idx, val = _rows(rng, 65, 100, 500)
        p = rng.dirichlet(np.ones(3), size=65); k_out = 100
    elif name == "deep":                      # the deepest list and the most groups; Zipf-like group sizes against a nearly flat target: the small groups exhaust
        group = _zipf_groups(rng, 6000, 64); idx, val = _rows(rng, 5, 2048, 6000)
        p = 0.5 + rng.random((1, 64)); p /= p.sum(); k_out = 2048
    elif name == "prefix":                    # K_out < K
        group = _zipf_groups(rng, 200, 2); idx, val = _rows(rng, 9, 50, 200); p = np.array([[0.5, 0.5]]); k_out = 17
    elif name == "zero_p":                    # a target of 0: the group is never in A or B (hi = 0) and comes last, through the fallback
        group = _zipf_groups(rng, 200, 3); idx, val = _rows(rng, 6, 40, 200); p = np.array([[0.5, 0.0, 0.5]]); k_out = 40
    elif name in ("quarters", "halves", "thirds"):      # k * p on integers and half-integers (floor == ceil at times), and never on one
        group = (rng.random(200) < 0.5).astype(np.uint8); idx, val = _rows(rng, 6, 40, 200)
        p = np.array([{"quarters": [0.25, 0.75], "halves": [0.5, 0.5], "thirds": [1 / 3, 2 / 3]}[name]]); k_out = 40
    elif name == "absent":                    # experts of group 2 exist, no row ranks one
        group = _zipf_groups(rng, 300, 3); idx, val = _rows(rng, 6, 30, np.nonzero(group != 2)[0]); p = np.array([[0.4, 0.3, 0.3]]); k_out = 30
    return dict(idx=idx, val=val, group=group, p=np.ascontiguousarray(p, dtype=np.float64), k_out=k_out)


CASES = ("one", "two", "per_row", "deep", "prefix", "zero_p", "quarters", "halves", "thirds", "absent")


@functools.lru_cache(maxsize=None)
def reference(name, alg):
    c = case(name)
    idx, val, pos = R.rerank(c["idx"].tolist(), c["val"].tolist(), c["group"].tolist(), c["p"].tolist(), ALGS[alg], c["k_out"])
    return np.array(idx, np.int32), np.array(val, np.float32), np.array(pos, np.int32)


@functools.lru_cache(maxsize=None)
def device(name, alg):
    from opentf_amd import libntf
    c = case(name)
    return libntf.fair_rerank(c["idx"], c["val"], c["group"], c["p"], alg, k_out=c["k_out"], want_pos=True)


@pytest.mark.parametrize("alg", list(ALGS))
@pytest.mark.parametrize("name", CASES)
def test_rerank_equals_the_reference(name, alg):
    c = case(name)
    ridx, rval, rpos = reference(name, alg)
    idx, val, pos = device(name, alg)
    assert pos.shape == (len(c["idx"]), c["k_out"]) and pos.dtype == np.int32 and idx.dtype == np.int32 and val.dtype == np.float32
    assert np.array_equal(pos, rpos), (name, alg, np.argwhere(pos != rpos)[:4])
    assert np.array_equal(idx, ridx) and np.array_equal(val.view(np.uint32), rval.view(np.uint32))
    for i in range(len(pos)):                 # a permutation prefix of the row
        assert len(set(pos[i].tolist())) == c["k_out"] and pos[i].min() >= 0 and pos[i].max() < c["idx"].shape[1]
    if name == "deep":                        # the case is only worth its time if groups do run out
        g = c["group"][c["idx"]]
        assert min(np.bincount(g[i], minlength=64).min() for i in range(len(g))) < 2048 // 64
    if name == "zero_p":                      # the zero-target group is in neither A nor B: it is not placed while both other groups still have candidates
        g = c["group"][idx]
        for i in range(len(g)):
            first = np.nonzero(g[i] == 1)[0]
            assert len(first) == 0 or min((g[i][first[0]:] == 0).sum(), (g[i][first[0]:] == 2).sum()) == 0


def test_rerank_without_values_and_positions():
    from opentf_amd import libntf
    c = case("two")
    idx, val = libntf.fair_rerank(c["idx"], None, c["group"], c["p"], "det_cons")
    assert val is None and np.array_equal(idx, reference("two", "det_cons")[0])


@pytest.mark.parametrize("alg", list(ALGS))
def test_rerank_is_bit_identical_under_a_split_of_the_rows(alg):
    from opentf_amd import libntf
    c = case("per_row")
    whole = device("per_row", alg)
    a = libntf.fair_rerank(c["idx"][:30], c["val"][:30], c["group"], c["p"][:30], alg, k_out=c["k_out"], want_pos=True)
    b = libntf.fair_rerank(c["idx"][30:], c["val"][30:], c["group"], c["p"][30:], alg, k_out=c["k_out"], want_pos=True)
    for w, x, y in zip(whole, a, b):
        assert np.concatenate([x, y]).tobytes() == w.tobytes()


# --------------------------------------------------------------------------------- the measures
METRIC_CASES = {"two": [1, 2, 5, 64], "per_row": [1, 3, 10, 64, 65, 100], "deep": [1, 2, 5, 10, 100, 1000, 2047, 2048], "zero_p": [1, 7, 40], "absent": [2, 30],
                "one": [1]}


@pytest.mark.parametrize("which", ["original", "reranked"])
@pytest.mark.parametrize("name", list(METRIC_CASES))
def test_metrics_match_the_reference(name, which, capsys):
    """ntf_fair_metrics against tests/fair_reference.py on the original list and on the DetGreedy re-ranked one.  +-inf and the 0.0 of an absent group with target 0
    must be EQUAL.  Finite values: device and reference perform the same IEEE operations in the same order on the same inputs, except that log and log2 come from
    two libraries.  ASSUMPTION (the device library's accuracy table is not in this tree): its f64 log and log2 are good to 1 ulp, as HIP's math API documentation
    lists them; the host's libm is taken at 1 ulp as well.  In units of 2^-53 (half an ulp at worst is one unit, an ulp two) the two NDKL chains at cutoff c over G
    groups can drift apart by
        numerator:    4 (ln, both sides) + 2 (d * ln) + 2 (G - 1) (the sum over g) + 4 (log2) + 2 (1 / log2) + 2 (w * KL) + 2 (c - 1) (the sum over k)
        denominator:  4 (log2) + 2 (1 / log2) + 2 (c - 1)
        quotient:     2
    that is L = 4 c + 2 G + 16 units, each relative to at most the chain over the ABSOLUTE terms, S = (sum_k w_k sum_g |d ln(d / p_g)|) / (sum_k w_k), which the
    reference computes beside the NDKL.  Bound: |device - reference| <= L * 2^-53 * S.  A skew is one ln of one identical quotient: 4 units of |reference|.
    The bound is measured against the reference only; where S = 0 (every term exactly 0) the values must be equal.  The largest differences seen on the MI355X
    are in profiles/fair_parity.md."""
    from opentf_amd import libntf
    c = case(name)
    cuts = METRIC_CASES[name]
    idx = c["idx"] if which == "original" else device(name, "det_greedy")[0]
    cuts = [k for k in cuts if k <= idx.shape[1]]
    G = c["p"].shape[1]
    rn, rs, ra = (np.array(a, np.float64) for a in R.metrics(idx.tolist(), c["group"].tolist(), c["p"].tolist(), cuts))
    ndkl, skew = libntf.fair_metrics(idx, c["group"], c["p"], cuts)
    assert ndkl.shape == rn.shape and skew.shape == rs.shape and ndkl.dtype == np.float64 and skew.dtype == np.float64
    worst_n = worst_s = 0.0
    for q, k in enumerate(cuts):
        bound = (4 * k + 2 * G + 16) * 2.0 ** -53 * ra[:, q]
        fin = np.isfinite(rn[:, q])
        assert np.array_equal(ndkl[~fin, q], rn[~fin, q])
        diff = np.abs(ndkl[fin, q] - rn[fin, q])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst_n = max(worst_n, float(np.max(np.where(bound[fin] > 0, diff / bound[fin], 0.0), initial=0.0)))
        assert (diff <= bound[fin]).all(), (name, which, k, float(diff.max()), float(bound[fin].min()))
    fin = np.isfinite(rs)
    assert np.array_equal(skew[~fin], rs[~fin])
    zero = fin & (rs == 0.0)
    assert (skew[zero] == 0.0).all()
    diff, bound = np.abs(skew[fin] - rs[fin]), 4 * 2.0 ** -53 * np.abs(rs[fin])
    if diff.size:
        with np.errstate(invalid="ignore", divide="ignore"):
            worst_s = float(np.max(np.where(bound > 0, diff / bound, 0.0)))
    with capsys.disabled():
        print(f"\nfair parity {name:8s} {which:9s} ndkl: worst |diff| / bound = {worst_n:.4f}   skew: worst |diff| / bound = {worst_s:.4f}", flush=True)
    assert (diff <= bound).all(), (name, which, float(diff.max()))
    if name == "zero_p" and which == "original":
        assert np.isinf(ndkl).any() and (skew == np.inf).any()
    if name == "absent":
        assert (skew[:, :, 2] == -np.inf).all()


def test_metrics_one_output_at_a_time():
    from opentf_amd import libntf
    c = case("two")
    both = libntf.fair_metrics(c["idx"], c["group"], c["p"], [5, 64])
    n_only = libntf.fair_metrics(c["idx"], c["group"], c["p"], [5, 64], skew=False)
    s_only = libntf.fair_metrics(c["idx"], c["group"], c["p"], [5, 64], ndkl=False)
    assert n_only[1] is None and s_only[0] is None and n_only[0].tobytes() == both[0].tobytes() and s_only[1].tobytes() == both[1].tobytes()


# --------------------------------------------------------------------------------- refusals
def _ptr(a):
    import ctypes
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_every_refusal_leaves_the_outputs_untouched():
    from opentf_amd import libntf
    lib = libntf.lib()
    n, K, G, E = 4, 8, 2, 16
    rng = np.random.default_rng(0)
    good = dict(alg=0, idx=np.stack([rng.permutation(E)[:K] for _ in range(n)]).astype(np.int32), val=np.zeros((n, K), np.float32), n=n, K=K,
                group=(np.arange(E) % 2).astype(np.uint8), E=E, G=G, p=np.array([[0.5, 0.5]]), n_p=1, k_out=K, cuts=np.array([1, K], np.int32), n_cut=2,
                want_idx=True, want_val=True, want_ndkl=True, want_skew=True)

    def rerank(**kw):
        a = {**good, **kw}
        oi, ov, op = np.full((n, K), -7, np.int32), np.full((n, K), -7.0, np.float32), np.full((n, K), -7, np.int32)
        rc = lib.ntf_fair_rerank(0, a["alg"], _ptr(a["idx"]), _ptr(a["val"]), a["n"], a["K"], _ptr(a["group"]), a["E"], a["G"], _ptr(a["p"]), a["n_p"], a["k_out"],
                                 _ptr(oi) if a["want_idx"] else None, _ptr(ov) if a["want_val"] else None, _ptr(op))
        return rc, bool((oi == -7).all() and (ov == -7.0).all() and (op == -7).all())

    def metrics(**kw):
        a = {**good, **kw}
        on, os_ = np.full((n, 2), -7.0), np.full((n, 2, G), -7.0)
        rc = lib.ntf_fair_metrics(0, _ptr(a["idx"]), a["n"], a["K"], _ptr(a["group"]), a["E"], a["G"], _ptr(a["p"]), a["n_p"], _ptr(a["cuts"]), a["n_cut"],
                                  _ptr(on) if a["want_ndkl"] else None, _ptr(os_) if a["want_skew"] else None)
        return rc, bool((on == -7.0).all() and (os_ == -7.0).all())

    assert rerank()[0] == 0 and metrics()[0] == 0          # the base call is accepted: each refusal below is owed to its one change
    bad_idx_hi, bad_idx_lo, bad_group = good["idx"].copy(), good["idx"].copy(), good["group"].copy()
    bad_idx_hi[2, 3] = E; bad_idx_lo[0, 0] = -1; bad_group[5] = G
    shared = [dict(idx=None), dict(group=None), dict(p=None), dict(n=0), dict(K=0), dict(K=2049), dict(G=0), dict(G=65), dict(n_p=2), dict(n_p=0),
              dict(idx=bad_idx_hi), dict(idx=bad_idx_lo), dict(group=bad_group),
              dict(p=np.array([[np.nan, 0.5]])), dict(p=np.array([[np.inf, 0.5]])), dict(p=np.array([[-0.1, 1.1]])), dict(p=np.array([[1.5, 0.0]])),
              dict(p=np.array([[0.5, 0.5 + 3e-6]])), dict(p=np.array([[0.5, 0.5 - 3e-6]]))]
    for kw in shared + [dict(alg=3), dict(alg=-1), dict(k_out=0), dict(k_out=K + 1), dict(want_idx=False), dict(val=None)]:
        assert rerank(**kw) == (EINVAL, True), kw
    for kw in shared + [dict(cuts=None), dict(n_cut=0), dict(n_cut=9), dict(cuts=np.array([0, K], np.int32)), dict(cuts=np.array([1, K + 1], np.int32)),
                        dict(want_ndkl=False, want_skew=False)]:
        assert metrics(**kw) == (EINVAL, True), kw
    # inside the sanity bound of the target's sum: accepted
    assert rerank(p=np.array([[0.5, 0.5 + 5e-7]]))[0] == 0 and metrics(p=np.array([[0.5, 0.5 - 5e-7]]))[0] == 0
    with pytest.raises(libntf.NtfError):
        libntf.fair_rerank(good["idx"], None, good["group"], good["p"], "fa*ir")
    with pytest.raises(libntf.NtfError):
        libntf.fair_metrics(good["idx"], good["group"], good["p"], [K + 1])


# --------------------------------------------------------------------------------- Ntf.adila end to end
class Cfg(dict):
    """attribute-dict standing in for an omegaconf DictConfig (missing keys read as None, like optional yaml keys)"""
    def __getattr__(self, k):
        if k.startswith("__"): raise AttributeError(k)
        return self.get(k)


def _toy(name):
    toy = golden(f"toy_{name}")
    n, S, M = [int(v) for v in toy["shape"]]
    skill = scipy.sparse.csr_matrix((np.ones(len(toy["skill_indices"]), np.uint8), toy["skill_indices"], toy["skill_indptr"]), shape=(n, S)).tolil()
    member = scipy.sparse.csr_matrix((np.ones(len(toy["member_indices"]), np.uint8), toy["member_indices"], toy["member_indptr"]), shape=(n, M)).tolil()
    splits = {"test": toy["test"], "folds": {k: {"train": toy[f"train{k}"], "valid": toy[f"valid{k}"]} for k in range(3)}}
    return {"skill": skill, "member": member, "loc": None}, splits


FAIRCFG = dict(algorithm="det_cons", notion="dp", attribute="popularity", k_max=10, cutoffs=[2, 5, 10])


def _check_files(m, tv, splits, faircfg):
    """the three files beside every prediction file; `ranked` is fair.rerank of the file's own ranking"""
    import pandas as pd
    from opentf_amd.evl import fair, metric
    from opentf_amd.mdl.ntf import _read_pred
    spec = fair.FairSpec.from_cfg(faircfg)
    group, names = fair.popularity_groups(tv["member"])
    out = {}
    for k in range(3):
        stem = f"{m.output}/f{k}.test.pred.{spec.algorithm}.{spec.notion}.popularity.k{spec.k_max}"
        assert stem == fair.fair_stem(f"{m.output}/f{k}.test.pred", spec)
        assert all(os.path.exists(stem + s) for s in (".rerank.pred", ".faireval.csv", ".utileval.csv"))
        pr = torch.load(stem + ".rerank.pred", map_location="cpu", weights_only=False)
        assert list(pr.keys()) == ["y_pred", "ranked", "uncertainty"] and pr["uncertainty"] is None
        Y_ = _read_pred(f"{m.output}/f{k}.test.pred")
        ranked = metric._ranked_topk(Y_, spec.k_max)
        p = fair.target_distribution(spec.notion, group, 2, scipy.sparse.csr_matrix(tv["member"])[splits["test"]])
        idx, val = fair.rerank(ranked, fair.ranked_values(Y_, ranked), group, p, spec.algorithm, spec.k_max)
        assert pr["ranked"].dtype == np.int32 and pr["ranked"].shape == (len(splits["test"]), spec.k_max) and np.array_equal(pr["ranked"], idx)
        ref_idx = np.array(R.rerank(ranked.tolist(), None, group.tolist(), p.tolist(), ALGS[spec.algorithm], spec.k_max)[0], np.int32)
        assert np.array_equal(idx, ref_idx)
        y = pr["y_pred"]
        assert y.is_sparse and y.is_coalesced() and tuple(y.shape) == (len(splits["test"]), tv["member"].shape[1]) and y._nnz() == idx.size
        dense = y.to_dense().numpy()
        assert np.array_equal(np.take_along_axis(dense, idx.astype(np.int64), axis=1), val)     # the k-th largest score sits on the k-th re-ranked expert
        fe, ue = pd.read_csv(stem + ".faireval.csv", index_col=0), pd.read_csv(stem + ".utileval.csv", index_col=0)
        assert list(fe.columns) == ["before", "after"] == list(ue.columns)
        assert list(fe.index) == [f"ndkl_{c}" for c in spec.cutoffs] + [f"skew_{nm}_{c}" for nm in names for c in spec.cutoffs]
        assert list(ue.index) == [f"{f}_{c}" for f in ("P", "recall", "ndcg_cut", "map_cut") for c in spec.cutoffs]
        out[k] = (fe, ranked, idx, group, p)
    return out


def test_adila_on_a_toy_models_predictions(tmp_path):
    from opentf_amd.mdl.fnn import Fnn
    tv, splits = _toy("dblp")
    m = Fnn(str(tmp_path), "cuda:0", 0, Cfg(b=8, e=1, ns=2, lr=0.01, es=2, h=[16], spe=0, l="bce", tpw=10, tnw=1, nsd="uniform"))
    m.learn(tv, splits, None)
    m.test(tv, splits, Cfg(per_epoch=False, on_train=False, topK=None))
    m.adila(tv, splits, Cfg(FAIRCFG))
    _check_files(m, tv, splits, FAIRCFG)


def test_adila_lowers_the_ndkl_of_a_skewed_prediction(tmp_path):
    """a synthetic prediction that scores every expert by popularity (the popular ones first, all of them): under demographic parity the re-ranked lists are no
    further from the target than the original ones - for the reference on the CPU first, then in the files adila() writes"""
    from opentf_amd.evl import fair
    from opentf_amd.mdl.ntf import Ntf
    tv, splits = _toy("dblp")
    count = np.asarray(scipy.sparse.csr_matrix(tv["member"]).sum(axis=0)).reshape(-1).astype(np.float32)
    rng = np.random.default_rng(11)
    m = Ntf(str(tmp_path), "cuda:0", 0, Cfg(b=1))
    for k in range(3):
        y = count[None, :] / count.max() * 0.9 + rng.random((len(splits["test"]), len(count))).astype(np.float32) * 0.01
        torch.save({"y_pred": torch.from_numpy(y.astype(np.float32)), "uncertainty": None}, f"{m.output}/f{k}.test.pred", pickle_protocol=4)
    m.adila(tv, splits, Cfg(FAIRCFG))
    for k, (fe, ranked, idx, group, p) in _check_files(m, tv, splits, FAIRCFG).items():
        before = np.array(R.metrics(ranked.tolist(), group.tolist(), p.tolist(), [10])[0]).mean()
        after = np.array(R.metrics(idx.tolist(), group.tolist(), p.tolist(), [10])[0]).mean()
        assert after <= before and before > 0.05, (before, after)            # the reference, on the CPU
        assert fe.loc["ndkl_10", "after"] <= fe.loc["ndkl_10", "before"]
        assert abs(fe.loc["ndkl_10", "before"] - before) <= 1e-12 and abs(fe.loc["ndkl_10", "after"] - after) <= 1e-12
