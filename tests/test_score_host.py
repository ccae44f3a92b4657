"""Host side of scoring inside the engine (NTF_EVAL_ENGINE=1), no GPU: `evl.metric.score_engine` assembles the frames `score_predictions` assembles - index,
columns, order, values - from an engine object's `score_rows` result; the switch is parsed per call; `_engine_plan` sends what the device entry does not do to the
file route; `_ckpt_jobs` lists the checkpoints as test() does, under the names `_pred_jobs` gives the prediction files.

The library calls of both routes (`ntf_rank_metrics`, `ntf_skill_coverage`) are served here by one numpy restatement behind a stand-in for `libntf.lib()`, and
the stand-in engine's `score_rows` is built on the same restatement: what is compared is everything the Python layer does around them."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from opentf_amd import libntf
from opentf_amd.evl import metric
from opentf_amd.mdl import ntf as ntf_mod

TREC = ["P_2,5", "recall_2,5,10", "ndcg_cut_5", "map_cut_2,5", "success_10"]


# ------------------------------------------------------------------------------------------------------------------ numpy restatements
def np_rank_metrics(top, ip, ix, rows, cuts):
    n, K = top.shape
    out = np.zeros((n, 5 * len(cuts)), np.float32)
    for i in range(n):
        truth = set(ix[ip[rows[i]]:ip[rows[i] + 1]].tolist())
        rel = np.array([c in truth for c in top[i, :min(max(cuts), K)]], dtype=np.float64)
        pos = np.arange(len(rel))
        for q, k in enumerate(cuts):
            r = rel[:k]
            hits = r.sum()
            dcg = (r / np.log2(pos[:k] + 2)).sum()
            idcg = (1 / np.log2(np.arange(min(len(truth), k)) + 2)).sum()
            ap = (r * np.cumsum(r) / (pos[:k] + 1)).sum()
            out[i, 0 * len(cuts) + q] = hits / k
            out[i, 1 * len(cuts) + q] = hits / len(truth) if truth else 0
            out[i, 2 * len(cuts) + q] = dcg / idcg if idcg else 0
            out[i, 3 * len(cuts) + q] = ap / len(truth) if truth else 0
            out[i, 4 * len(cuts) + q] = hits > 0
    return out


def np_skill_coverage(top, sip, six, rows, cip, cix, cuts):
    out = np.zeros((len(top), len(cuts)), np.float32)
    for i in range(len(top)):
        req = set(six[sip[rows[i]]:sip[rows[i] + 1]].tolist())
        for q, k in enumerate(cuts):
            held = set()
            for ex in top[i, :k]: held |= set(cix[cip[ex]:cip[ex + 1]].tolist())
            out[i, q] = len(held & req) / len(req)
    return out


def _arr(ptr, dtype, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=shape)


class FakeLib:
    """`ntf_rank_metrics` / `ntf_skill_coverage` with the library's argument lists, computed by the restatements above"""
    def ntf_rank_metrics(self, device, top, n, K, ip, ix, n_truth, rows, cu, n_cut, out):
        ip_ = _arr(ip, np.int64, (n_truth + 1,)); ix_ = _arr(ix, np.int32, (max(int(ip_[-1]), 1),))
        r = np.arange(n) if rows is None else _arr(rows, np.int64, (n,))
        _arr(out, np.float32, (n, 5 * n_cut))[:] = np_rank_metrics(_arr(top, np.int32, (n, K)), ip_, ix_, r, _arr(cu, np.int32, (n_cut,)).tolist())
        return 0

    def ntf_skill_coverage(self, device, top, n, K, sip, six, n_skill_rows, rows, cip, cix, E, cu, n_cut, out):
        sip_ = _arr(sip, np.int64, (n_skill_rows + 1,)); six_ = _arr(six, np.int32, (int(sip_[-1]),))
        cip_ = _arr(cip, np.int64, (E + 1,)); cix_ = _arr(cix, np.int32, (int(cip_[-1]),))
        r = np.arange(n) if rows is None else _arr(rows, np.int64, (n,))
        _arr(out, np.float32, (n, n_cut))[:] = np_skill_coverage(_arr(top, np.int32, (n, K)), sip_, six_, r, cip_, cix_, _arr(cu, np.int32, (n_cut,)).tolist())
        return 0


class StubEngine:
    """`Engine.score_rows` over a fixed probability matrix P [all teams, M]: what the device entry returns, restated on the host"""
    def __init__(self, P, member):
        self.P, self.member, self.calls = P, sp.csr_matrix(member), []

    def score_rows(self, rows, batch, nmc=1, K=0, cutoffs=(), auc=False, K_out=0):
        from test_gpu_auc import oracle_counts
        self.calls.append(dict(batch=batch, nmc=nmc, K=K, cutoffs=list(cutoffs), auc=auc, K_out=K_out))
        D = self.P[rows]
        n, M = D.shape
        R = K if K else (max(cutoffs) if len(cutoffs) else 0)
        ranked = np.argsort(-D, axis=1, kind="stable")[:, :R].astype(np.int32)
        S = D
        if K:
            S = np.zeros_like(D); np.put_along_axis(S, ranked.astype(np.int64), np.take_along_axis(D, ranked.astype(np.int64), 1), 1)
        Y = self.member; Y.sort_indices()
        metrics = np_rank_metrics(ranked, Y.indptr, Y.indices, rows, list(cutoffs)) if len(cutoffs) else None
        counts = aucv = None
        if auc:
            counts = oracle_counts(S, Y[rows].toarray() != 0)
            aucv = float(counts[2]) / (2.0 * float(counts[0]) * float(counts[1]))
        assert K_out <= R
        return libntf.ScoreResult(metrics, counts, aucv, np.take_along_axis(D, ranked[:, :K_out].astype(np.int64), 1) if K_out else None, ranked[:, :K_out] if K_out else None)


@pytest.fixture
def toy(monkeypatch):
    monkeypatch.setattr(libntf, "lib", lambda: FakeLib())
    monkeypatch.delenv("NTF_AUC_DEVICE", raising=False)
    rng = np.random.default_rng(7)
    N, M, S = 60, 45, 30
    lab = rng.random((N, M)) < 0.08
    lab[5] = False                                                 # a team without a member among the experts
    member = sp.csr_matrix(lab.astype(np.uint8))
    skill = sp.csr_matrix((rng.random((N, S)) < 0.2).astype(np.uint8)).tolil()
    for i in range(N): skill[i, i % S] = 1                         # every team requires a skill
    cov = sp.csr_matrix((rng.random((M, S)) < 0.15).astype(np.uint8))
    grid = (0.05 + 0.9 * (np.arange(M) + 1.0) / (M + 1.0)).astype(np.float32)
    P = np.stack([grid[rng.permutation(M)] for _ in range(N)])     # distinct scores inside a row: no ranking left to a tie rule
    tv = {"member": member.tolil(), "skill": skill, "skillcoverage": cov}
    rows = np.concatenate([[5], rng.permutation(N)[:22]])
    return tv, rows, P, M


def _pred(P, rows, K, M):
    """the matrix test() writes: dense, or the top K of every row as a sparse matrix"""
    D = P[rows]
    if not K: return D
    idx = np.argsort(-D, axis=1, kind="stable")[:, :K]
    return sp.csr_matrix((np.take_along_axis(D, idx, 1).ravel(), (np.repeat(np.arange(len(rows)), K), idx.ravel())), shape=(len(rows), M))


@pytest.mark.parametrize("per_instance", [True, False])
@pytest.mark.parametrize("other", [["aucroc", "skill_coverage_2,5"], ["skill_coverage_2,12"], ["aucroc"], []])
@pytest.mark.parametrize("topK", [None, 12, 45, 100])
def test_score_engine_assembles_the_frames_of_score_predictions(toy, topK, other, per_instance):
    tv, rows, P, M = toy
    spec = metric.EvalSpec(topK, per_instance, TREC, other)
    K = topK if topK and topK < M else 0
    eng = StubEngine(P, tv["member"])
    inst_e, mean_e, roc_e = metric.score_engine(eng, tv, rows, spec, nmc=4, batch=9)
    inst_f, mean_f, roc_f = metric.score_predictions(tv, rows, _pred(P, rows, K, M), spec)
    assert roc_e is None and roc_f is None
    assert list(inst_e.columns) == list(inst_f.columns) and list(inst_e.index) == list(inst_f.index)
    assert np.array_equal(inst_e.values, inst_f.values) and inst_e.dtypes.tolist() == inst_f.dtypes.tolist()
    assert list(mean_e.index) == list(mean_f.index) and mean_e.index.name == mean_f.index.name == "metrics" and list(mean_e.columns) == list(mean_f.columns) == ["mean"]
    rest = [m for m in mean_f.index if m != "aucroc"]
    assert np.array_equal(mean_e.loc[rest, "mean"].values, mean_f.loc[rest, "mean"].values)
    if "aucroc" in other:
        assert list(mean_f.index).index("aucroc") == 9            # behind the 9 trec columns, in front of skill coverage
        assert abs(mean_e.loc["aucroc", "mean"] - mean_f.loc["aucroc", "mean"]) <= 1e-12        # the file route's f64 sums against the integer statistic
    # one call, with the arguments of the job; the ranked ids travel only for skill coverage
    (call,) = eng.calls
    skc = [m for m in other if m.startswith("skill_coverage")]
    assert call["batch"] == 9 and call["nmc"] == 4 and call["K"] == K and call["auc"] == ("aucroc" in other)
    assert call["K_out"] == (min(int(skc[0].split(",")[-1]), M) if skc else 0)
    assert len(call["cutoffs"]) <= 8 and call["cutoffs"] == sorted(set(call["cutoffs"]))


def test_score_engine_refuses_what_the_plan_leaves_to_the_files(toy):
    tv, rows, P, M = toy
    eng = StubEngine(P, tv["member"])
    with pytest.raises(ValueError, match="curve"):
        metric.score_engine(eng, tv, rows, metric.EvalSpec(12, True, TREC, ["aucroc+"]), 1, 9)
    with pytest.raises(ValueError, match="Only one class"):
        metric.score_engine(eng, tv, np.array([5, 5]), metric.EvalSpec(12, True, TREC, ["aucroc"]), 1, 9)
    assert not eng.calls


def test_engine_plan():
    S = metric.EvalSpec
    plan = metric._engine_plan
    assert plan(S(10, True, ["P_2,5", "recall_10"], ["aucroc"]), 1000) == (10, [2, 5, 10], 0, None)
    assert plan(S(None, True, ["P_2,5"], []), 1000) == (0, [2, 5], 0, None)
    assert plan(S(1000, True, ["P_2,5"], []), 1000)[0] == 0 and plan(S(5000, True, ["P_2,5"], []), 1000)[0] == 0       # test() writes the dense matrix
    assert plan(S(2048, True, ["P_2"], []), 10**5)[0] == 2048
    assert "2048" in plan(S(2049, True, ["P_2"], []), 10**5)[3]
    assert "curve" in plan(S(10, True, ["P_2"], ["aucroc+"]), 1000)[3]
    # cutoffs above K are the kernel's business; skill coverage needs its ranks stored
    assert plan(S(10, True, ["P_2,50"], ["skill_coverage_2,10"]), 1000) == (10, [2, 50], 10, None)
    assert "stored" in plan(S(10, True, ["P_2"], ["skill_coverage_2,11"]), 1000)[3]
    # dense: the ranked list is max(cutoffs) wide, so skill coverage beyond the trec cutoffs adds one
    assert plan(S(None, True, ["P_2,5"], ["skill_coverage_2,10"]), 1000) == (0, [2, 5, 10], 10, None)
    assert plan(S(None, True, ["P_2,50"], ["skill_coverage_2,10"]), 1000) == (0, [2, 50], 10, None)
    assert plan(S(None, True, [], ["skill_coverage_2,10"]), 1000) == (0, [10], 10, None)
    assert plan(S(None, True, [], ["skill_coverage_2,10"]), 7) == (0, [7], 7, None)
    assert "ranked" in plan(S(None, True, ["P_3000"], []), 10**5)[3] and "ranked" in plan(S(None, True, ["P_2"], ["skill_coverage_3000"]), 10**5)[3]
    assert "8 distinct" in plan(S(None, True, ["P_1,2,3,4,5", "recall_6,7,8,9"], []), 1000)[3]
    assert plan(S(None, True, ["P_1,2,3,4", "recall_5,6,7,8"], []), 1000)[3] is None


@pytest.mark.parametrize("value,on", [(None, False), ("", False), ("0", False), ("1", True), ("true", False), ("2", False), (" 1", False)])
def test_switch_is_read_per_call(monkeypatch, value, on):
    if value is None: monkeypatch.delenv("NTF_EVAL_ENGINE", raising=False)
    else: monkeypatch.setenv("NTF_EVAL_ENGINE", value)
    assert metric.eval_engine_enabled() is on
    monkeypatch.setenv("NTF_EVAL_ENGINE", "1"); assert metric.eval_engine_enabled()
    monkeypatch.delenv("NTF_EVAL_ENGINE"); assert not metric.eval_engine_enabled()


def test_checkpoint_jobs_follow_the_prediction_jobs(tmp_path):
    splits = {"folds": {0: {}, 1: {}}}
    names = ["f0.pt", "f1.pt", "f0.e0.pt", "f0.e2.pt", "f0.e10.pt", "f1.e1.pt", "f10.e3.pt", "f0.e1.pt.bak", "xf0.e5.pt", "f0.test.pred", "f0.e2.pth", "logs4tboard"]
    out = str(tmp_path)
    for nm in names: open(f"{out}/{nm}", "w").close()
    got = [(j.pred_set, j.fold, j.path, j.final, c) for j, c in ntf_mod._ckpt_jobs(out, splits, False, True)]
    assert got == [("test", 0, f"{out}/f0.test.pred", True, f"{out}/f0.pt"),
                   ("test", 0, f"{out}/f0.test.e0.pred", False, f"{out}/f0.e0.pt"),
                   ("test", 0, f"{out}/f0.test.e2.pred", False, f"{out}/f0.e2.pt"),
                   ("test", 0, f"{out}/f0.test.e10.pred", False, f"{out}/f0.e10.pt"),
                   ("test", 1, f"{out}/f1.test.pred", True, f"{out}/f1.pt"),
                   ("test", 1, f"{out}/f1.test.e1.pred", False, f"{out}/f1.e1.pt")]
    # without per_epoch the directory is not even listed; on_train adds the two other sets, set by set
    got = [(j.pred_set, j.fold, j.final, c) for j, c in ntf_mod._ckpt_jobs(out + "/nowhere", splits, True, False)]
    assert got == [(s, k, True, f"{out}/nowhere/f{k}.pt") for s in ("test", "train", "valid") for k in (0, 1)]
    # the prediction files test() writes for these checkpoints are the files _pred_jobs lists, in the same order
    for j, c in list(ntf_mod._ckpt_jobs(out, splits, True, True)): open(j.path, "w").close()
    a = [(j.pred_set, j.fold, j.path, j.final) for j, _ in ntf_mod._ckpt_jobs(out, splits, True, True)]
    b = [(j.pred_set, j.fold, j.path, j.final) for j in ntf_mod._pred_jobs(out, splits, True, True)]
    assert a == b and len(a) == 3 * 6


def test_models_without_an_engine_keep_the_file_route(monkeypatch, tmp_path, caplog):
    import logging
    m = ntf_mod.Ntf(str(tmp_path), "cuda:0", 0, {})
    with caplog.at_level(logging.INFO):
        assert m._eval_engine({"member": sp.csr_matrix((3, 50))}, metric.EvalSpec(10, True, ["P_2"], [])) is None
    assert "owns no engine" in caplog.text
    made = []
    m._engine = lambda tv, b, train=False: (made.append((b, train)) or "ENGINE", None)
    m.cfg = {"b": 17}
    with caplog.at_level(logging.INFO):
        assert m._eval_engine({"member": sp.csr_matrix((3, 50))}, metric.EvalSpec(10, True, ["P_2"], ["aucroc+"])) is None
    assert "curve" in caplog.text and not made
    assert m._eval_engine({"member": sp.csr_matrix((3, 50))}, metric.EvalSpec(10, True, ["P_2"], ["aucroc"])) == "ENGINE" and made == [(17, False)]
