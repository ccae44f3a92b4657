"""`ntf_roc_micro_dense` / `ntf_roc_micro_csr` (ntf_auc.hip: k_roc_count, roc_finish; include/opentf_amd_roc.h) and `micro_roc_device` on a real MI355X against the
pin, tests/roc_reference.py (a stable sort of all pairs and a walk over the distinct scores; checked against sklearn in tests/test_roc_host.py).

Everything is compared for EQUALITY: fps and tps as integers, the thresholds as f32 bits, P / N / U2 and the double against `ntf_auc_micro_*` on the same input.
There is no tolerance anywhere in this file.  Each case sits at an edge of the kernel: the LDS / global counter arms and the pivot stride, the load loop's tail
and absent second load, chunked uploads, the hot bucket, the CSR entry's host-side fold of the implicit zeros, and the key map's special values."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

import roc_reference as R
from roc_calls import EINVAL, roc_csr, roc_dense
from test_gpu_auc import auc_csr, auc_dense, truth_csr

pytestmark = pytest.mark.gpu

def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def assert_is_reference(got, lab, S, auc_entry):
    """got = (status, Curve); the reference over the dense pair (lab, S); auc_entry = what ntf_auc_micro_* returned for the same input"""
    rc, out = got
    assert rc == 0, rc
    fps, tps, thr, counts, auc = out.points()
    w_fps, w_tps, w_thr, w_counts, G = R.roc_points(lab, S)
    assert len(fps) == len(w_fps) <= 2 * G + 2
    assert np.array_equal(fps, w_fps) and np.array_equal(tps, w_tps)
    assert np.array_equal(bits(thr), bits(w_thr)), "thresholds differ in their f32 bits"
    assert counts == w_counts
    a_rc, a_counts, a_auc = auc_entry
    assert a_rc == 0 and counts == a_counts and auc == a_auc                               # bit for bit the AUC entry's own return
    assert R.doubled_trapezoid(fps, tps) == counts[2]
    return fps, tps, thr


def check_dense(S, lab, chunk=0):
    ip, ix = truth_csr(lab)
    return assert_is_reference(roc_dense(S, ip, ix, chunk=chunk), lab, S, auc_dense(S, ip, ix, chunk=chunk))


def check_csr(D, lab, chunk=0):
    """D: scipy CSR of the stored scores (explicit zeros kept as stored)"""
    n, M = D.shape
    ip, ix = truth_csr(lab)
    a = (D.indptr, D.indices, D.data, n, M, ip, ix)
    return assert_is_reference(roc_csr(*a, chunk=chunk), lab, D.toarray(), auc_csr(*a, chunk=chunk))


# ------------------------------------------------------------------------------------------------------------------ 1. the counter arms
def pooled_case(n, M, per_row, G, seed):
    """positives drawn from exactly G distinct values, negatives mostly inside the gaps, some tied with a positive's value"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((n, M), dtype=bool)
    for i in range(n):
        lab[i, rng.choice(M, per_row, replace=False)] = True
    pool = np.sort(rng.permutation(np.unique(rng.random(4 * G, dtype=np.float32)))[:G]) if G > 1 else np.array([0.5], np.float32)
    assert len(pool) == G
    S = rng.random((n, M), dtype=np.float32)
    tie = rng.random((n, M)) < 0.05
    S[tie] = pool[rng.integers(G, size=int(tie.sum()))]
    P = int(lab.sum())
    assert P >= G
    pv = np.concatenate([pool, pool[rng.integers(G, size=P - G)]])
    S[lab] = pv[rng.permutation(P)]
    return S, lab


@pytest.mark.parametrize("G", [1, 2047, 2048, 5000], ids=["G=1", "G=2047:last-LDS", "G=2048:first-global", "G=5000:stride-4"])
def test_counter_arms(G):
    S, lab = pooled_case(200, 2000, 30, G, 100 + G)
    assert len(np.unique(S[lab])) == G
    fps, tps, thr = check_dense(S, lab)
    if G > 1: assert len(fps) > G + 2                                                       # gaps were non-empty: their ends are listed too


# ------------------------------------------------------------------------------------------------------------------ 2. the load loop
@pytest.mark.parametrize("L", [3, 5, 7, 4 * 301 + 2, 4 * 511 + 1, 4 * (3 * 512 + 77) + 3],
                         ids=["tail-only", "one-vector+1", "one-vector+3", "301-vectors+2", "511-vectors+1", "4-blocks:1613-vectors+3"])
def test_load_loop(L):
    """L & 3 in {1, 2, 3}; an odd number of 16-byte vectors (a thread's second load of the round is absent); L below one workgroup's first round"""
    rng = np.random.default_rng(200 + L)
    S = rng.standard_normal((1, L)).astype(np.float32)
    lab = np.zeros((1, L), dtype=bool)
    lab[0, rng.choice(L, max(1, L // 40), replace=False)] = True
    lab[0, L - 1] = True                                                                   # a positive in the scalar tail
    if L > 3: lab[0, L - 2] = False
    S[0, : L // 3] = np.round(S[0, : L // 3], 1)                                           # ties between the classes too
    check_dense(S, lab)


# ------------------------------------------------------------------------------------------------------------------ 3. chunking
def test_chunks_are_bit_identical():
    n, M = 9, 1003
    rng = np.random.default_rng(301)
    lab = rng.random((n, M)) < 0.02
    S = rng.random((n, M), dtype=np.float32)
    # one gap whose smallest score sits in the last row while most of its count sits in the first ones
    v = np.sort(np.unique(S[lab]))
    lo, hi = v[len(v) // 2], v[len(v) // 2 + 1]
    inside = (S > lo) & (S < hi) & ~lab
    S[inside] = hi - (hi - lo) * np.float32(0.25)
    S[n - 1, np.flatnonzero(~lab[n - 1])[0]] = lo + (hi - lo) * np.float32(0.125)
    ip, ix = truth_csr(lab)
    one = check_dense(S, lab)
    rc, out = roc_dense(S, ip, ix, chunk=M * 4)                                            # one row per upload
    assert rc == 0
    for a, b in zip(one, out.points()[:3]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    check_dense(S, lab, chunk=M * 4)
    D = sp.csr_matrix(np.where(rng.random((n, M)) < 0.2, S, 0).astype(np.float32))
    a = check_csr(D, lab)
    b = check_csr(D, lab, chunk=64)
    assert all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ 4. the hot bucket
@pytest.mark.parametrize("positive_at_zero", [False, True], ids=["zero-in-a-gap", "a-positive-scores-0"])
def test_hot_bucket(positive_at_zero):
    n, M = 64, 3001
    rng = np.random.default_rng(401)
    lab = rng.random((n, M)) < 0.01
    S = np.where(rng.random((n, M)) < 0.9, 0, rng.standard_normal((n, M))).astype(np.float32)
    S[rng.random((n, M)) < 0.05] = -0.0
    S[lab & (S == 0)] = np.float32(0.75)
    at = np.argwhere(lab)
    if positive_at_zero:
        S[tuple(at[0])] = 0.0; S[tuple(at[1])] = -0.0
    else:
        S[tuple(at[0])] = np.float32(-1e-30)                                               # the positive next below zero: zero is the smallest score of its gap
        assert not ((S > np.float32(-1e-30)) & (S < 0)).any()
    assert (S == 0).mean() > 0.85 and bool((S[lab] == 0).any()) == positive_at_zero
    fps, tps, thr = check_dense(S, lab)
    z = np.flatnonzero(thr == 0)
    assert len(z) == 1 and not np.signbit(thr[z[0]])                                       # listed once, as +0.0, whichever zero the data held


# ------------------------------------------------------------------------------------------------------------------ 5. the CSR entry
def test_csr_minimum_from_the_host_fold_alone():
    """every stored value is above the smallest positive score, which is stored: gap 0 holds the implicit zeros only, its minimum never saw the device"""
    n, M = 40, 500
    rng = np.random.default_rng(501)
    lab = rng.random((n, M)) < 0.02
    stored = lab | (rng.random((n, M)) < 0.1)
    V = (np.float32(0.6) + np.float32(0.4) * rng.random((n, M), dtype=np.float32)) * stored
    V[tuple(np.argwhere(lab)[0])] = np.float32(0.5)
    D = sp.csr_matrix(V.astype(np.float32))
    assert D.nnz == stored.sum() and V[stored].min() == np.float32(0.5)
    fps, tps, thr = check_csr(D, lab)
    assert thr[-1] == 0 and int(fps[-1] - fps[-2]) == n * M - D.nnz and tps[-1] == tps[-2]


def test_csr_implicit_zeros_at_a_positives_key_and_a_stored_negative_below():
    n, M = 40, 500
    rng = np.random.default_rng(502)
    lab = rng.random((n, M)) < 0.02
    stored = (lab & (rng.random((n, M)) < 0.5)) | (~lab & (rng.random((n, M)) < 0.1))      # half the positives are not stored: they score 0
    V = (rng.random((n, M), dtype=np.float32) + np.float32(0.01)) * stored
    neg = np.argwhere(stored & ~lab)
    V[tuple(neg[0])] = np.float32(-0.3); V[tuple(neg[1])] = np.float32(-1e-40)             # gap 0 is non-empty; its minimum is the device's
    D = sp.csr_matrix(V.astype(np.float32))
    fps, tps, thr = check_csr(D, lab)
    assert thr[-1] == np.float32(-0.3) and (thr == 0).sum() == 1
    D2 = D.copy(); D2.data[np.flatnonzero(D2.data == V[tuple(neg[2])])[0]] = 0.0           # a stored zero beside the implicit ones
    assert D2.nnz == D.nnz and (D2.data == 0).sum() == 1
    check_csr(D2, lab)


def test_csr_empty_top_and_bottom_gaps():
    """the largest and the smallest score are positives': gaps G and 0 are empty and must still hold no minimum"""
    n, M = 30, 400
    rng = np.random.default_rng(503)
    lab = rng.random((n, M)) < 0.03
    stored = lab | (rng.random((n, M)) < 0.1)
    V = (rng.random((n, M), dtype=np.float32) * np.float32(0.8) + np.float32(0.1)) * stored
    pos = np.argwhere(lab)
    V[tuple(pos[0])] = np.float32(2.0)                                                     # the top score is a positive's
    stored[tuple(pos[1])] = False; V[tuple(pos[1])] = 0                                    # a positive among the implicit zeros, the lowest score there is
    D = sp.csr_matrix(V.astype(np.float32))
    fps, tps, thr = check_csr(D, lab)
    assert (fps[1], tps[1], thr[1]) == (0, 1, np.float32(2.0)) and thr[-1] == 0 and tps[-1] > tps[-2]
    # dense, the same property
    S = rng.random((n, M), dtype=np.float32)
    S[tuple(pos[0])] = 3.0; S[tuple(pos[1])] = -3.0
    fps, tps, thr = check_dense(S, lab)
    assert thr[1] == 3.0 and thr[-1] == -3.0


# ------------------------------------------------------------------------------------------------------------------ 6. keys
def test_special_keys():
    """negative scores, -0.0 beside +0.0 (one value), denormals of both signs (distinct values, never flushed), both infinities"""
    n, M = 12, 1001
    rng = np.random.default_rng(601)
    lab = rng.random((n, M)) < 0.03
    S = (50 * rng.standard_normal((n, M))).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3e-39, np.inf, -np.inf], dtype=np.float32)
    pick = rng.random((n, M)) < 0.3
    S[pick] = special[rng.integers(len(special), size=int(pick.sum()))]
    for cls in (lab, ~lab):
        for s in special:
            assert (bits(S[cls]) == bits(np.float32(s))).any()
    fps, tps, thr = check_dense(S, lab)
    assert np.isinf(thr[0]) and thr[1] == np.inf and thr[-1] == -np.inf
    for s in (1e-40, -1e-40, 1.4e-45, -1.4e-45, 3e-39):
        assert (bits(thr) == bits(np.float32(s))).sum() == 1
    assert (thr == 0).sum() == 1


# ------------------------------------------------------------------------------------------------------------------ 7. the Python layer and evaluate()
def test_micro_roc_device():
    from opentf_amd.evl import metric
    n, M = 60, 700
    rng = np.random.default_rng(701)
    lab = rng.random((n, M)) < 0.02
    Y = sp.csr_matrix(lab.astype(np.float32))
    D = np.where(rng.random((n, M)) < 0.1, rng.random((n, M)), 0).astype(np.float32)
    w_fps, w_tps, w_thr, (P, N, U2), _ = R.roc_points(lab, D)
    for pred in (D, sp.csr_matrix(D)):
        fpr, tpr, thr, counts = metric.micro_roc_device(Y, pred, return_counts=True)
        assert counts == (P, N, U2) and all(type(c) is int for c in counts)
        assert fpr.dtype == tpr.dtype == np.float64 and thr.dtype == np.float32
        assert np.array_equal(fpr, w_fps.astype(np.float64) / float(N)) and np.array_equal(tpr, w_tps.astype(np.float64) / float(P))
        assert np.array_equal(bits(thr), bits(w_thr))
        assert all(np.array_equal(a, b) for a, b in zip(metric.micro_roc_device(Y, pred, chunk_bytes=M * 4), (fpr, tpr, thr)))
        auc, curve = metric.calculate_auc_roc(Y, pred, curve=True, curve_device=0)
        assert auc == metric.micro_auc_device(Y, pred) and np.array_equal(curve[0], fpr) and np.array_equal(curve[1], tpr)
    assert all(np.array_equal(a, b) for a, b in zip(metric.micro_roc_device(Y, D.astype(np.float16)), metric.micro_roc_device(Y, D.astype(np.float16).astype(np.float32))))
    with pytest.raises(TypeError):
        metric.micro_roc_device(Y, D.astype(np.float64))


def test_evaluate_with_the_curve_on_the_device(tmp_path, monkeypatch):
    """`aucroc+` through Ntf.evaluate: under NTF_ROC_DEVICE=1 the pickled curve is micro_roc_device's and the aucroc row the value NTF_AUC_DEVICE=1 gives for
    `aucroc`; with the switch unset the pickle holds sklearn's arrays"""
    import pandas as pd
    from sklearn import metrics as skm
    from opentf_amd.evl import metric
    from opentf_amd.mdl.fnn import Fnn
    from opentf_amd.mdl.ntf import _read_pred
    from test_gpu_plugin import Cfg, _toy
    tv, splits = _toy("dblp")
    m = Fnn(str(tmp_path), "cuda:0", 0, Cfg(b=6, e=1, ns=3, lr=0.01, es=5, h=[32], spe=0, l="bce", tpw=10, tnw=1, nsd="uniform"))
    m.learn(tv, splits, None)
    m.test(tv, splits, Cfg(per_epoch=False, on_train=False, topK=8))

    def run(other, **env):
        for k in ("NTF_ROC_DEVICE", "NTF_AUC_DEVICE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m.evaluate(tv, splits, Cfg(topK=8, per_instance=False, on_train=False, per_epoch=False, metrics=Cfg(trec=["P_2,5"], other=[other])))
        path = f"{m.output}/f0.test.pred"
        mean = pd.read_csv(f"{path}.eval.mean.csv", index_col=0, float_precision="round_trip").loc["aucroc", "mean"]
        roc = None
        if other == "aucroc+":
            with open(f"{path}.eval.roc.pkl", "rb") as f: roc = pickle.load(f)
        return mean, roc

    Y = sp.csr_matrix(tv["member"])[splits["test"]]
    pred = _read_pred(f"{m.output}/f0.test.pred")
    auc_dev, _ = run("aucroc", NTF_AUC_DEVICE="1")
    auc_roc, roc = run("aucroc+", NTF_ROC_DEVICE="1")
    fpr, tpr, _ = metric.micro_roc_device(Y, pred)
    assert auc_roc == auc_dev and len(roc) == 2 and np.array_equal(roc[0], fpr) and np.array_equal(roc[1], tpr)
    for env in ({}, {"NTF_AUC_DEVICE": "1"}):
        auc_host, roc_host = run("aucroc+", **env)
        s_fpr, s_tpr, _ = skm.roc_curve(Y.toarray().ravel(), pred.toarray().ravel())
        assert np.array_equal(roc_host[0], s_fpr) and np.array_equal(roc_host[1], s_tpr)
        assert auc_host == skm.roc_auc_score(Y.toarray(), pred.toarray(), average="micro", multi_class="ovr")


# ------------------------------------------------------------------------------------------------------------------ 8. refusals leave nothing behind
def test_refusals():
    n, M = 6, 40
    rng = np.random.default_rng(801)
    lab = rng.random((n, M)) < 0.1
    S = rng.random((n, M), dtype=np.float32)
    ip, ix = truth_csr(lab)
    P = len(ix)
    D = sp.csr_matrix(S)
    csr = (D.indptr, D.indices, D.data, n, M, ip, ix)
    bad_neg = S.copy(); bad_neg[tuple(np.argwhere(~lab)[0])] = np.nan                      # found by the kernel's flag, not on the host
    for rc, out in (roc_dense(S, ip, ix, cap=2 * P + 1), roc_csr(*csr, cap=2 * P + 1), roc_dense(S, ip, ix, cap=0), roc_dense(bad_neg, ip, ix),
                    roc_dense(S, ip, ix, chunk=M * 4 - 1), roc_csr(*csr, chunk=3),
                    *[roc_dense(S, ip, ix, null=(k,)) for k in ("scores", "fps", "tps", "thr", "n", "counts", "auc")],
                    *[roc_csr(*csr, null=(k,)) for k in ("fps", "tps", "thr", "n", "counts", "auc")]):
        assert rc == EINVAL and out.untouched()
    check_dense(S, lab)
    rc, out = roc_dense(S, ip, ix, cap=2 * P + 40)                                         # a roomier buffer: the same points, nothing behind them
    assert rc == 0 and np.array_equal(out.points()[0], check_dense(S, lab)[0])
