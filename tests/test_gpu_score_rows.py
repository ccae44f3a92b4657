"""`ntf_score_rows` (`Engine.score_rows`): a prediction set scored inside the engine - ranking metrics, the exact integer micro AUC, the ranked entries -
against the entries it replaces, run batch by batch from the same `set_seed(seed, step)`: `ntf_forward` / `ntf_forward_topk` for the probabilities and the
ranked lists, `ntf_rank_metrics` on those lists, `ntf_auc_micro_dense` / `ntf_auc_micro_csr` and the sort-based integer oracle of tests/test_gpu_auc.py
(`oracle_counts`) for the counts.  Every comparison is exact: integers EQUAL, floats bit for bit (`np.array_equal` on the f32 arrays, `==` on the f64 AUC), no
element left out.  Where sklearn is named the bar is 1e-12, as in tests/test_gpu_eval.py.

The matrix that is scored: K == 0 the dense probabilities; K >= 1 the top-K-sparsified prediction (the K stored values of a row, 0.0 everywhere else), which is
what test() writes with topK = K."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_auc import auc_csr, auc_dense, auc_of, keys_of, oracle_counts, sklearn_auc

pytestmark = pytest.mark.gpu

EINVAL, EHIP, ESTATE = -1, -2, -3
SEED, STEP = 3, 11
CUTS = (1, 2, 5, 10, 64, 65)


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    import random
    import torch
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


# ------------------------------------------------------------------------------------------------------------------ models and references
_DS = {}


def dataset(D, M, n_rows=400, mean_members=None):
    """synthetic teams (made once per shape); mean_members: a denser member matrix than dblp's 3.06 experts a team"""
    from opentf_amd.synth import make_dataset, zipf_csr
    key = (D, M, n_rows, mean_members)
    if key not in _DS:
        ds = make_dataset("dblp", d=D, seed=7, n_rows=n_rows, n_experts=M)
        if mean_members: ds["member"] = zipf_csr(n_rows, M, mean_members, 99)
        _DS[key] = ds
    return _DS[key]


def engine(ds, dims, bayesian, B, multihot=False, scale_out=None, poke=None):
    from opentf_amd.synth import init_params
    from test_gpu_ep import _mk
    e = _mk(ds, dims, bayesian, B, "uniform", multihot=multihot)
    if scale_out or poke:
        sd = init_params(dims, bayesian, 0)
        L = len(dims) - 2
        if scale_out:
            for k in (("mu_weight", "mu_bias") if bayesian else ("weight", "bias")): sd[f"layers.{L}.{k}"] = sd[f"layers.{L}.{k}"] * np.float32(scale_out)
        if poke: sd[f"layers.{L}.{'mu_weight' if bayesian else 'weight'}"][poke[0], poke[1]] = poke[2]
        e.load_state_dict(sd)
    return e


def labels_of(ds, rows, M):
    ip, ix = ds["member"]
    Y = sp.csr_matrix((np.ones(len(ix), np.int8), ix, ip), shape=(len(ip) - 1, M))[rows]
    return Y.toarray() != 0


def batches(n, B):
    return [(o, min(o + B, n)) for o in range(0, n, B)]


def ref_dense(e, rows, B, nmc):
    e.set_seed(SEED, STEP)
    return np.concatenate([e.forward(rows[a:b], nmc=nmc) for a, b in batches(len(rows), B)])


def ref_topk(e, rows, B, nmc, K):
    e.set_seed(SEED, STEP)
    parts = [e.forward_topk(rows[a:b], K, nmc=nmc) for a, b in batches(len(rows), B)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def rank_metrics(ds, rows, idx, cuts):
    """ntf_rank_metrics on ranked ids [n, K]"""
    from opentf_amd import libntf
    ip, ix = (np.ascontiguousarray(a) for a in ds["member"])
    idx = np.ascontiguousarray(idx, dtype=np.int32); cu = np.ascontiguousarray(cuts, dtype=np.int32); r = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.zeros((len(rows), 5 * len(cu)), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = libntf.lib().ntf_rank_metrics(0, p(idx), len(rows), idx.shape[1], p(ip), p(ix), len(ip) - 1, p(r), p(cu), len(cu), p(out))
    assert rc == 0
    return out


def sparsified(tv, ti, M):
    S = np.zeros((tv.shape[0], M), dtype=np.float32)
    np.put_along_axis(S, ti.astype(np.int64), tv, axis=1)
    return S


def check(e, ds, rows, B, nmc, K, cuts=CUTS, sklearn=False, after=False):
    """score_rows against the reference loop, everything exact.  -> (result, the scored matrix S [n, M], labels)"""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    n, M = len(rows), e.dims[-1]
    R = K if K else max(cuts)
    e.set_seed(SEED, STEP)
    res = e.score_rows(rows, B, nmc=nmc, K=K, cutoffs=cuts, auc=True, K_out=R)
    nxt = e.forward(rows[:min(B, n)], nmc=nmc) if after else None
    lab = labels_of(ds, rows, M)
    ip, ix = (np.ascontiguousarray(a) for a in ds["member"])
    if K == 0:
        S = ref_dense(e, rows, B, nmc)
        nxt_ref = e.forward(rows[:min(B, n)], nmc=nmc) if after else None
        tv, ti = ref_topk(e, rows, B, nmc, R)
        got_lib = auc_dense(S, ip, ix, rows=rows)
    else:
        tv, ti = ref_topk(e, rows, B, nmc, K)
        # (forward and forward_topk take the same steps: one reference for "the step counter lands where the loop leaves it")
        nxt_ref = e.forward(rows[:min(B, n)], nmc=nmc) if after else None
        S = sparsified(tv, ti, M)
        o = np.argsort(ti, axis=1, kind="stable")
        got_lib = auc_csr(np.arange(n + 1, dtype=np.int64) * K, np.take_along_axis(ti, o, 1).ravel(), np.take_along_axis(tv, o, 1).ravel(), n, M, ip, ix, rows=rows)
    want = oracle_counts(S, lab)
    print(f"K={K} n={n} B={B} nmc={nmc}: counts {res.counts} oracle {want} library {got_lib[1]} auc {res.auc!r}")
    assert res.counts == want
    assert got_lib[0] == 0 and res.counts == got_lib[1] and res.auc == got_lib[2]
    assert res.auc == auc_of(want)
    if sklearn:
        print("auc - sklearn", res.auc - sklearn_auc(S, lab))
        assert abs(res.auc - sklearn_auc(S, lab)) <= 1e-12
    assert res.vals.dtype == np.float32 and res.idx.dtype == np.int32
    assert np.array_equal(res.idx, ti) and np.array_equal(res.vals.view(np.uint32), tv.view(np.uint32))
    assert np.array_equal(res.metrics.view(np.uint32), rank_metrics(ds, rows, ti, cuts).view(np.uint32))
    if after:
        assert np.array_equal(nxt.view(np.uint32), nxt_ref.view(np.uint32)), "the step counter did not land where the reference loop leaves it"
    return res, S, lab


# ------------------------------------------------------------------------------------------------------------------ 1. dense, Fnn, h = [128]
M1, B1 = 1003, 70


@pytest.fixture(scope="module")
def fnn128():
    ds = dataset(128, M1)
    e = engine(ds, [128, 128, M1], False, B1)
    yield e, ds
    e.close()


def test_dense_fnn(fnn128):
    e, ds = fnn128
    rows = np.arange(2 * B1 + 7)
    res, S, lab = check(e, ds, rows, B1, 1, 0, sklearn=True, after=True)
    assert (M1 * 4) % 16 != 0                                   # rows end inside a 16-byte vector
    assert len(np.unique(S)) > S.size // 2                      # real-valued scores


# ------------------------------------------------------------------------------------------------------------------ 2. top-K mode
@pytest.mark.parametrize("K", [1, 10, 100, M1])
def test_topk_fnn(fnn128, K):
    e, ds = fnn128
    rows = np.arange(2 * B1 + 7)
    # cutoffs above K for the small K, below and above 64 for the large ones
    res, S, lab = check(e, ds, rows, B1, 1, K, cuts=CUTS, sklearn=(K == 10), after=True)
    if K < M1:
        assert (lab & (S == 0)).any()                           # positives outside the stored top K score 0.0


@pytest.mark.parametrize("K", [0, 10, 700])
def test_saturated_model_ties(K):
    """output layer scaled by 1e6: probabilities of exactly 0.0 and 1.0 - large tie groups in both classes; K = 700 stores zeros, K = 10 leaves positives outside"""
    ds = dataset(128, M1)
    e = engine(ds, [128, 64, M1], False, B1, scale_out=1e6)
    rows = np.arange(B1 + 9)
    res, S, lab = check(e, ds, rows, B1, 1, K)
    D = ref_dense(e, rows, B1, 1)
    e.close()
    assert ((D == 0) | (D == 1)).mean() > 0.5, ((D == 0).mean(), (D == 1).mean())
    for cls in (lab, ~lab):
        assert (D[cls] == 0).sum() > 10 and (D[cls] == 1).sum() > 10
    if K == 700:
        assert (res.vals == 0).any()                            # stored zeros
    if K == 10:
        assert (lab & (D == 1) & (S == 0)).any()                # a positive of probability 1.0 that the top K left out


# ------------------------------------------------------------------------------------------------------------------ 3. Bnn, nmc = 3
@pytest.fixture(scope="module")
def bnn128():
    ds = dataset(128, M1)
    e = engine(ds, [128, 128, M1], True, B1)
    yield e, ds
    e.close()


@pytest.mark.parametrize("K", [0, 10])
def test_bnn_mc(bnn128, K):
    e, ds = bnn128
    rows = np.arange(2 * B1 + 7)
    res, S, lab = check(e, ds, rows, B1, 3, K, sklearn=True, after=True)
    # the same call again from the same seed and step
    e.set_seed(SEED, STEP)
    again = e.score_rows(rows, B1, nmc=3, K=K, cutoffs=CUTS, auc=True, K_out=K if K else max(CUTS))
    assert again.counts == res.counts and again.auc == res.auc
    for a, b in ((again.metrics, res.metrics), (again.vals, res.vals), (again.idx, res.idx)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # one pass is another sample: the three-pass mean really was scored
    e.set_seed(SEED, STEP)
    assert e.score_rows(rows, B1, nmc=1, K=K, auc=True).counts != res.counts


# ------------------------------------------------------------------------------------------------------------------ 4. past 2048 distinct positive keys
def test_many_distinct_positive_keys():
    """G >= 2049 distinct keys among the positives: the pivots become a sample of the key table and the bucket counters leave LDS (2 G + 1 > 4096); the twin stays below"""
    M, n_rows, B = 5000, 1400, 256
    ds = dataset(128, M, n_rows=n_rows, mean_members=8.0)
    nnz = np.diff(ds["member"][0])
    rich = np.nonzero(nnz >= 5)[0]
    assert len(rich) >= 600
    e = engine(ds, [128, 64, M], False, B)
    rows = rich[:600]
    res, S, lab = check(e, ds, rows, B, 1, 0, cuts=(2, 5))
    G = len(np.unique(keys_of(S[lab])))
    print("distinct positive keys", G)
    assert G >= 2049
    few = rich[:np.searchsorted(np.cumsum(nnz[rich]), 2000)]
    res, S, lab = check(e, ds, few, B, 1, 0, cuts=(2, 5))
    G = len(np.unique(keys_of(S[lab])))
    print("distinct positive keys (twin)", G)
    assert 1000 < G < 2047
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 5. every inference family
FAMILIES = {
    "h64_exact_f32": dict(dims=[128, 64, M1]),
    "h96_pad": dict(dims=[128, 96, M1]),
    "h100_generic": dict(dims=[128, 100, M1]),
    "no_hidden": dict(dims=[128, M1]),
    "two_hidden": dict(dims=[128, 32, 128, M1]),
    "multihot": dict(dims=[90_671, 128, M1], multihot=True),
    "infer_f32_off": dict(dims=[128, 64, M1], env={"NTF_INFER_F32": "0"}),
    "infer_f32_off_128": dict(dims=[128, 128, M1], env={"NTF_INFER_F32": "0"}),
    "infer_mc": dict(dims=[128, 128, M1], env={"NTF_INFER_MC": "1"}, bayes_only=True, nmc=3),
}


@pytest.mark.parametrize("name,bayesian", [(n, b) for n in FAMILIES for b in (False, True) if b or not FAMILIES[n].get("bayes_only")])
def test_inference_families(name, bayesian, monkeypatch):
    """dense AUC (two sweeps: the replay must be bit-identical on every arm) + metrics"""
    f = FAMILIES[name]
    for k, v in f.get("env", {}).items(): monkeypatch.setenv(k, v)        # read when the engine is created
    dims = f["dims"]
    ds = dataset(128 if not f.get("multihot") else 8, M1)
    e = engine(ds, dims, bayesian, B1, multihot=bool(f.get("multihot")))
    nmc = f.get("nmc", 2 if bayesian else 1)
    rows = np.arange(B1 + 13)
    mc0 = e.mc_fused_passes()
    check(e, ds, rows, B1, nmc, 0, cuts=(1, 5, 65), after=True)
    if name == "infer_mc":
        assert e.mc_fused_passes() > mc0                         # the arm really ran
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 6. a range fallback inside the call
@pytest.mark.parametrize("bayesian", [False, True], ids=["fnn", "bnn"])
@pytest.mark.parametrize("K", [0, 10])
def test_range_fallback_inside_the_call(bayesian, K):
    ds = dataset(128, M1)
    e = engine(ds, [128, 128, M1], bayesian, B1, poke=(7, 5, 1e6))
    f0 = e.range_fallbacks()
    rows = np.arange(B1 + 13)
    e.set_seed(SEED, STEP)
    e.score_rows(rows, B1, nmc=2 if bayesian else 1, K=K, cutoffs=(5,), auc=True)
    grown = e.range_fallbacks() - f0
    print("range fallbacks inside the call", grown)
    assert grown >= 2                                           # every batch of every sweep
    check(e, ds, rows, B1, 2 if bayesian else 1, K, cuts=(1, 5, 65))
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 7. row handling
def _with_empty_row(ds, r):
    ip, ix = ds["member"]
    keep = np.ones(len(ix), bool); keep[ip[r]:ip[r + 1]] = False
    nnz = np.diff(ip).copy(); nnz[r] = 0
    out = dict(ds); out["member"] = (np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64), ix[keep].copy())
    return out


@pytest.mark.parametrize("K", [0, 10])
def test_row_handling(K):
    ds = _with_empty_row(dataset(128, M1), 3)
    assert np.diff(ds["member"][0])[3] == 0
    e = engine(ds, [128, 128, M1], False, B1)
    cases = {
        "repeated id and an empty truth row": (np.array([5, 3, 5, 9, 3, 5, 200, 0]), 3),
        "B = 1": (np.array([4, 3, 17, 5, 6]), 1),
        "n < B": (np.arange(20, 31), B1),
        "B = max_batch, a short last batch": (np.arange(B1 + 1), B1),
        "one row": (np.array([8]), B1),
    }
    for what, (rows, B) in cases.items():
        print(what)
        check(e, ds, rows, B, 1, K, cuts=(1, 5, 65), after=True)
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 8. the contract
SENT_F, SENT_I, SENT_U = np.float32(-77.0), np.int32(-77), np.uint64(77)


def raw_call(e, rows, n=None, B=B1, nmc=1, K=0, cuts=(2, 5), n_cut=None, K_out=None, want=("metrics", "auc", "vals", "idx"), null=(), cap=None):
    """ntf_score_rows itself on sentinel-filled buffers -> (status, untouched?)"""
    from opentf_amd import libntf
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    n = len(rows) if n is None else n
    cu = np.ascontiguousarray(cuts, dtype=np.int32)
    n_cut = len(cu) if n_cut is None else n_cut
    nn = max(len(rows), 1)
    if K_out is None: K_out = (K if K else (max(cuts) if len(cuts) else 0)) if ("vals" in want or "idx" in want) else 0
    w = cap or max(K_out, 1)
    metrics = np.full((nn, 5 * max(n_cut, 1)), SENT_F); counts = np.full(3, SENT_U); auc = C.c_double(-7.0)
    vals = np.full((nn, w), SENT_F); idx = np.full((nn, w), SENT_I)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = dict(rows=p(rows), cuts=p(cu) if len(cu) else None, metrics=p(metrics) if "metrics" in want else None, counts=p(counts) if "auc" in want else None,
                auc=C.byref(auc) if "auc" in want else None, vals=p(vals) if "vals" in want else None, idx=p(idx) if "idx" in want else None)
    for k in null: args[k] = None
    rc = libntf.lib().ntf_score_rows(e._h, args["rows"], n, B, nmc, K, args["cuts"], n_cut, args["metrics"], args["counts"], args["auc"], K_out, args["vals"], args["idx"])
    untouched = bool((metrics == SENT_F).all() and (counts == SENT_U).all() and auc.value == -7.0 and (vals == SENT_F).all() and (idx == SENT_I).all())
    return rc, untouched


def test_contract(fnn128):
    e, ds = fnn128
    rows = np.arange(B1 + 5)
    n_rows = len(ds["member"][0]) - 1
    assert raw_call(e, rows) == (0, False)                                          # the good call the refusals below are variations of
    assert raw_call(e, rows, K=10) == (0, False)
    refused = {
        "rows NULL": dict(null=("rows",)),
        "n = 0": dict(n=0),
        "n < 0": dict(n=-1),
        "B = 0": dict(B=0),
        "B > max_batch": dict(B=B1 + 1),
        "nmc = 0": dict(nmc=0),
        "K < 0": dict(K=-1, K_out=1),
        "K > M": dict(K=M1 + 1, K_out=1),
        "n_cut = 9": dict(cuts=(1, 2, 3, 4, 5, 6, 7, 8, 9)),
        "n_cut < 0": dict(n_cut=-1),
        "a cutoff of 0": dict(cuts=(2, 0)),
        "cutoffs NULL": dict(null=("cuts",)),
        "metrics without cutoffs": dict(cuts=(), want=("metrics", "auc")),
        "dense: the largest cutoff above M": dict(cuts=(2, M1 + 1), want=("metrics", "auc")),
        "nothing asked for": dict(want=()),
        "nothing asked for, cutoffs alone": dict(want=(), cuts=(2,)),
        "counts without auc": dict(null=("auc",)),
        "auc without counts": dict(null=("counts",)),
        "K_out above K": dict(K=10, K_out=11, cap=11),
        "dense: K_out above max(cutoffs)": dict(K_out=6, cap=6),
        "K_out without a buffer": dict(K_out=2, want=("metrics", "auc")),
        "buffers without K_out": dict(K_out=0),
    }
    for what, kw in refused.items():
        rc, untouched = raw_call(e, rows, **kw)
        assert (rc, untouched) == (EINVAL, True), (what, rc, untouched)
    for bad in (-1, n_rows, 2**40):
        r = rows.copy(); r[-1] = bad                                                # in the LAST batch: the first one must not have run
        for K in (0, 10):
            assert raw_call(e, r, K=K) == (EINVAL, True), bad
    # the step counter of a refused call stays where it was
    e.set_seed(SEED, STEP); a = e.forward(rows[:4])
    e.set_seed(SEED, STEP); raw_call(e, rows, B=0); b = e.forward(rows[:4])
    assert np.array_equal(a, b)
    # K above 2048 at an M above it
    ds5 = dataset(128, 5000, n_rows=1400, mean_members=8.0)
    e5 = engine(ds5, [128, 64, 5000], False, 8)
    assert raw_call(e5, np.arange(8), B=8, K=2049, K_out=1) == (EINVAL, True)
    assert raw_call(e5, np.arange(8), B=8, cuts=(2049,), want=("metrics",)) == (EINVAL, True)
    assert raw_call(e5, np.arange(8), B=8, K=2048, K_out=2048)[0] == 0
    e5.close()


def test_contract_one_class_nan_and_python_layer():
    from opentf_amd import libntf
    from opentf_amd.synth import init_params
    M = 40
    ds = dict(dataset(128, M, n_rows=50))
    ip, ix = ds["member"]
    nnz = np.diff(ip).copy(); nnz[0] = 0; nnz[1] = M               # row 0 has no member, row 1 has them all
    cols = [np.arange(M, dtype=np.int32) if r == 1 else ix[ip[r]:ip[r + 1]] for r in range(len(nnz)) if r != 0]
    ds["member"] = (np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64), np.concatenate(cols).astype(np.int32))
    e = engine(ds, [128, 64, M], False, 16)
    for K in (0, 5):
        assert raw_call(e, np.array([0, 0]), B=16, K=K) == (EINVAL, True)           # P == 0
        assert raw_call(e, np.array([1]), B=16, K=K) == (EINVAL, True)              # N == 0
        assert raw_call(e, np.array([0, 0]), B=16, K=K, want=("metrics", "vals", "idx"))[0] == 0      # without the AUC both are fine
        check(e, ds, np.array([0, 1, 2, 1]), 16, 1, K, cuts=(1, 5))
    # a NaN probability
    sd = init_params([128, 64, M], False, 0)
    sd["layers.1.bias"][7] = np.nan
    e.load_state_dict(sd)
    assert np.isnan(e.forward(np.arange(3))).any()
    for K in (0, M):
        assert raw_call(e, np.arange(20), B=16, K=K) == (EINVAL, True)
    with pytest.raises(libntf.NtfError, match="NaN"):
        e.score_rows(np.arange(20), 16, auc=True)
    e.close()
    # the Python layer: only what was asked for comes back
    e = engine(ds, [128, 64, M], False, 16)
    r = e.score_rows(np.arange(2, 20), 16, cutoffs=(2, 5))
    assert r.metrics.shape == (18, 10) and r.counts is None and r.auc is None and r.vals is None and r.idx is None
    r = e.score_rows(np.arange(2, 20), 16, K=7, auc=True, K_out=3)
    assert r.metrics is None and len(r.counts) == 3 and all(isinstance(c, int) for c in r.counts) and r.vals.shape == (18, 3) and r.idx.shape == (18, 3)
    v, i = e.forward_topk(np.arange(2, 18), 7)
    assert np.array_equal(r.idx[:16], i[:, :3]) and np.array_equal(r.vals[:16], v[:, :3])
    e.close()


def test_expert_shard_is_refused():
    from opentf_amd.ep import expert_shards
    from test_gpu_ep import _mk
    ds = dataset(128, 3000)
    e = _mk(ds, [128, 64, 3000], False, 32, "uniform", shard=expert_shards(3000, 2)[0], world=2)
    assert raw_call(e, np.arange(32), B=32) == (ESTATE, True)
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 9. the plugin
TREC = ["P_2,5", "recall_2,5", "ndcg_cut_2,5", "map_cut_2,5", "success_2,5"]


def _eval_files(out):
    out = glob.escape(out)                                       # the run directory carries the config: "h[32]"
    names = sorted(glob.glob(f"{out}/*.csv") + glob.glob(f"{out}/*.pkl"))
    return {os.path.basename(p): open(p, "rb").read() for p in names}


def _clear_eval_files(out):
    for p in glob.glob(f"{glob.escape(out)}/*.csv") + glob.glob(f"{glob.escape(out)}/*.pkl"): os.remove(p)


def test_plugin_evaluate_in_the_engine_writes_the_same_files(tmp_path, monkeypatch):
    """toy Fnn learn -> test -> evaluate, with NTF_EVAL_ENGINE unset and set: every csv file byte for byte.  NTF_AUC_DEVICE=1 in both runs: the file route then takes
    the integer AUC too (`ntf_auc_micro_dense` / `_csr`), the only one of its AUC routes whose f64 is defined bit for bit; sklearn's and `micro_auc_sparse`'s
    sums agree with it to 1e-12 (tests/test_gpu_auc.py), which a csv of 17 digits does not hide."""
    import scipy.sparse
    from conftest import golden
    from opentf_amd.mdl import ntf as ntf_mod
    from opentf_amd.mdl.fnn import Fnn
    from test_gpu_plugin import Cfg, _toy
    tv, splits = _toy("dblp")
    g = golden("g10_metrics")
    n_exp, n_skill = tv["member"].shape[1], tv["skill"].shape[1]
    tv["skillcoverage"] = scipy.sparse.csr_matrix((np.ones(len(g["dblp.fnn.cov_indices"]), np.uint8), g["dblp.fnn.cov_indices"], g["dblp.fnn.cov_indptr"]),
                                                 shape=(n_exp, n_skill))
    cfg = Cfg(b=6, e=3, ns=3, lr=0.01, es=5, h=[32], spe=1, l="bce", tpw=10, tnw=1, nsd="uniform")
    m = Fnn(str(tmp_path), "cuda:0", 0, cfg)
    m.learn(tv, splits, None)
    assert os.path.exists(f"{m.output}/f0.e1.pt")
    monkeypatch.setenv("NTF_AUC_DEVICE", "1")
    reads = []
    real_read = ntf_mod._read_pred
    monkeypatch.setattr(ntf_mod, "_read_pred", lambda path: (reads.append(path), real_read(path))[1])
    other = ["skill_coverage_2,5", "aucroc"]
    assert n_exp > 8
    for topK, per_epoch, on_train in ((8, True, True), (None, False, False), (n_exp, True, False)):      # sparse top-8 files; dense files
        m.test(tv, splits, Cfg(per_epoch=per_epoch, on_train=on_train, topK=topK))
        evalcfg = Cfg(topK=topK, per_instance=True, on_train=on_train, per_epoch=per_epoch, metrics=Cfg(trec=TREC, other=other))
        monkeypatch.delenv("NTF_EVAL_ENGINE", raising=False)
        _clear_eval_files(m.output); del reads[:]
        m.evaluate(tv, splits, evalcfg)
        by_file, n_read = _eval_files(m.output), len(reads)
        monkeypatch.setenv("NTF_EVAL_ENGINE", "1")
        _clear_eval_files(m.output); del reads[:]
        m.evaluate(tv, splits, evalcfg)
        by_engine = _eval_files(m.output)
        assert not reads, "the engine route read a prediction file"
        n_sets, n_ckpt = (3 if on_train else 1), (len(glob.glob(f"{glob.escape(m.output)}/f*.pt")) if per_epoch else 3)
        assert n_ckpt >= 3 + 3 * per_epoch
        assert n_read == n_sets * n_ckpt
        assert sorted(by_engine) == sorted(by_file) and len(by_file) == 2 * n_read + 2 * n_sets
        for name in by_file:
            assert by_engine[name] == by_file[name], name
        assert b"aucroc" in by_file["f0.test.pred.eval.mean.csv"] and b"skill_coverage_5" in by_file["f0.test.pred.eval.instance.csv"]
    # aucroc+ keeps the curve: the switch falls back to the file route
    evalcfg = Cfg(topK=n_exp, per_instance=False, on_train=False, per_epoch=False, metrics=Cfg(trec=TREC, other=["aucroc+"]))
    _clear_eval_files(m.output); del reads[:]
    m.evaluate(tv, splits, evalcfg)
    assert len(reads) == 3 and os.path.exists(f"{m.output}/f0.test.pred.eval.roc.pkl")
