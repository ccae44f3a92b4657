"""Host side of the device ROC curve (include/opentf_amd_roc.h, opentf_amd/evl/metric.py) and the yardstick of tests/test_gpu_roc.py, where no GPU is needed: the
pin (tests/roc_reference.py) against sklearn on seeded families, the header / export / binding surface, the refusals that return before any device call, and the
routes `score_predictions` / `calculate_auc_roc` take while NTF_ROC_DEVICE is unset."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import roc_reference as R
from conftest import ROOT
from roc_calls import EINVAL, roc_csr, roc_dense

N_H, M_H = 20, 301


def _labels(seed, density=0.03):
    return np.random.default_rng(seed).random((N_H, M_H)) < density


def _family(name, seed):
    """-> (labels, scores f32 [n, M]); the CSR families return the dense form of a matrix whose unstored entries are the zeros"""
    rng = np.random.default_rng(seed)
    lab = _labels(seed + 1000)
    n, M = lab.shape
    if name == "uniform":
        S = rng.random((n, M), dtype=np.float32)
    elif name == "six_valued":
        S = (rng.integers(0, 6, (n, M)) / 5).astype(np.float32)
    elif name == "zeros_80":
        S = np.where(rng.random((n, M)) < 0.8, 0, rng.random((n, M))).astype(np.float32)
    elif name == "negative_signed_zero_denormal":
        S = rng.standard_normal((n, M)).astype(np.float32)
        special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -3e-39], dtype=np.float32)
        pick = rng.random((n, M)) < 0.4
        S[pick] = special[rng.integers(len(special), size=int(pick.sum()))]
    elif name == "positives_tied":
        S = rng.random((n, M), dtype=np.float32)
        S[lab] = np.float32(0.5)
        S[~lab & (rng.random((n, M)) < 0.05)] = np.float32(0.5)
    elif name in ("topk_zero_in_a_gap", "topk_positive_at_zero"):
        S = np.zeros((n, M), dtype=np.float32)
        for i in range(n):
            c = rng.choice(M, 12, replace=False)
            S[i, c] = rng.random(12, dtype=np.float32) + np.float32(0.01)
        neg = np.argwhere((S != 0) & ~lab)
        S[tuple(neg[0])] = np.float32(-0.25)                                  # a stored value below zero
        if name == "topk_zero_in_a_gap":
            S[lab & (S == 0)] = np.float32(0.3)                               # every positive is stored with a non-zero score
            S[tuple(np.argwhere(lab)[0])] = np.float32(-0.5)                  # and one lies below the zeros: they fall strictly between two positive keys
        else:
            assert (S[lab] == 0).any()
    else:
        raise KeyError(name)
    return lab, S


FAMILIES = ("uniform", "six_valued", "zeros_80", "negative_signed_zero_denormal", "positives_tied", "topk_zero_in_a_gap", "topk_positive_at_zero")


# --------------------------------------------------------------------------------- the pin against sklearn
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", FAMILIES)
def test_reference_is_sklearns_curve(name, seed):
    from sklearn import metrics as skm
    lab, S = _family(name, seed)
    y, s = lab.ravel(), S.ravel().astype(np.float64)                          # f32 -> f64 is exact: sklearn sees the same real numbers
    fps, tps, thr, (P, N, U2), G = R.roc_points(lab, S)
    assert G == len(np.unique(S[lab] + np.float32(0.0))) and (name != "positives_tied" or G == 1)
    assert len(fps) <= 2 * G + 2 and (int(fps[0]), int(tps[0])) == (0, 0) and np.isposinf(thr[0]) and (int(fps[-1]), int(tps[-1])) == (N, P)
    s_fpr, s_tpr, s_thr = skm.roc_curve(y, s, drop_intermediate=False)
    s_fps, s_tps = np.rint(s_fpr * N).astype(np.int64), np.rint(s_tpr * P).astype(np.int64)
    assert np.array_equal(s_fps / N, s_fpr) and np.array_equal(s_tps / P, s_tpr)
    # every listed point is one of sklearn's, threshold included
    at = {(int(f), int(t)): (k, float(h)) for k, (f, t, h) in enumerate(zip(s_fps, s_tps, s_thr))}
    for f, t, h in zip(fps, tps, thr):
        k, sk_h = at[int(f), int(t)]
        assert float(h) == sk_h and int(f) / N == s_fpr[k] and int(t) / P == s_tpr[k]
    # every sklearn point lies on the polyline: inside a segment's box and collinear with its ends, in integers
    F, T = [int(x) for x in fps], [int(x) for x in tps]
    a = 0
    for f, t in zip(s_fps.tolist(), s_tps.tolist()):
        while not (F[a] <= f <= F[a + 1] and T[a] <= t <= T[a + 1]):
            a += 1
            assert a + 1 < len(F), "a sklearn point outside every segment"
        assert (F[a + 1] - F[a]) * (t - T[a]) == (T[a + 1] - T[a]) * (f - F[a])
    # the default list (drop_intermediate=True) is a subset of that one: on the polyline as well
    d_fpr, d_tpr, _ = skm.roc_curve(y, s)
    assert set(zip(d_fpr.tolist(), d_tpr.tolist())) <= set(zip(s_fpr.tolist(), s_tpr.tolist()))
    # its area
    assert R.doubled_trapezoid(fps, tps) == U2 == int(np.rint(2 * P * N * skm.roc_auc_score(y, s)))
    if name.startswith("topk"):                                                 # the sparse form of the same matrix is the same pair
        f2, t2, h2, c2, _ = R.roc_reference(sp.csr_matrix(lab.astype(np.float32)), sp.csr_matrix(S))
        assert np.array_equal(f2, fps) and np.array_equal(t2, tps) and np.array_equal(h2.view(np.uint32), thr.view(np.uint32)) and c2 == (P, N, U2)


def test_reference_by_hand():
    # scores 0.9+ 0.8- 0.8- 0.7+ 0.7- 0.2- -0.0- 0.0-: keys of the positives {0.7, 0.9}; gap 1 holds 0.8 x 2, gap 0 holds 0.2 and the two zeros
    lab = np.array([1, 0, 0, 1, 0, 0, 0, 0], dtype=bool)
    S = np.array([0.9, 0.8, 0.8, 0.7, 0.7, 0.2, -0.0, 0.0], dtype=np.float32)
    fps, tps, thr, counts, G = R.roc_points(lab, S)
    assert G == 2 and fps.tolist() == [0, 0, 2, 3, 6] and tps.tolist() == [0, 1, 1, 2, 2]
    assert thr.tolist() == [np.inf, np.float32(0.9), np.float32(0.8), np.float32(0.7), 0.0] and not np.signbit(thr[-1])
    assert counts == (2, 6, 2 * 6 + (2 * 3 + 1)) and R.doubled_trapezoid(fps, tps) == counts[2]


# --------------------------------------------------------------------------------- header, exports, binding
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ntf_\w+)\s*\(", src)))


def test_roc_header_exports_and_binding_agree():
    from opentf_amd import libntf
    declared = _declared("opentf_amd_roc.h")
    assert declared == ["ntf_roc_micro_csr", "ntf_roc_micro_dense"] == sorted(libntf.ROC_SYMBOLS)
    path = os.path.join(ROOT, "opentf_amd", "libopentf_amd.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(path)
    lib = libntf.lib()
    for name, (res, args) in libntf.ROC_SYMBOLS.items():
        assert hasattr(raw, name), f"{name} declared in include/opentf_amd_roc.h but not exported"
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    tail = [I64, I64, P, P, P, P, P, P]                                         # chunk_bytes, cap_points, fps, tps, thresholds, n_points, out_counts, out_auc
    assert libntf.ROC_SYMBOLS["ntf_roc_micro_dense"] == (ctypes.c_int, [ctypes.c_int, P, I64, I64, I64, P, P, I64, P] + tail)
    assert libntf.ROC_SYMBOLS["ntf_roc_micro_csr"] == (ctypes.c_int, [ctypes.c_int, P, P, P, I64, I64, P, P, I64, P] + tail)
    # the AUC pair, argument for argument, up to chunk_bytes; then the curve; then the AUC pair's own outputs
    for roc, auc in (("ntf_roc_micro_dense", "ntf_auc_micro_dense"), ("ntf_roc_micro_csr", "ntf_auc_micro_csr")):
        a = libntf.SYMBOLS[auc][1]
        assert libntf.ROC_SYMBOLS[roc][1] == a[:-2] + [I64, P, P, P, P] + a[-2:]


def test_roc_entries_stay_out_of_the_main_header():
    from opentf_amd import libntf
    main = _declared("opentf_amd.h")
    for name in libntf.ROC_SYMBOLS:
        assert name not in main and name not in libntf.SYMBOLS
    assert len(libntf.SYMBOLS) == 90 == len(main) and sorted(libntf.SYMBOLS) == main
    assert libntf.NTF_ABI_VERSION == 2 and libntf.lib().ntf_abi_version() == 2


# --------------------------------------------------------------------------------- refusals before any device call
def test_refusals_leave_every_output_untouched():
    lab, S = _family("uniform", 5)
    Y = sp.csr_matrix(lab.astype(np.int8)); Y.sort_indices()
    ip, ix = Y.indptr.astype(np.int64), Y.indices.astype(np.int32)
    P = len(ix)
    D = sp.csr_matrix(S)
    csr = (D.indptr, D.indices, D.data, N_H, M_H)
    nan_at_a_positive = S.copy(); nan_at_a_positive[tuple(np.argwhere(lab)[0])] = np.nan
    Dn = sp.csr_matrix(nan_at_a_positive)                                       # (NaN != 0: it is stored)
    empty = (np.zeros(N_H + 1, dtype=np.int64), np.zeros(1, dtype=np.int32))
    Yf = sp.csr_matrix(np.ones((N_H, M_H), dtype=np.int8)); Yf.sort_indices()
    full = (Yf.indptr.astype(np.int64), Yf.indices.astype(np.int32))
    calls = [roc_dense(S, ip, ix, cap=2 * P + 1), roc_csr(*csr, ip, ix, cap=2 * P + 1), roc_dense(S, ip, ix, cap=-1),
             roc_dense(nan_at_a_positive, ip, ix), roc_csr(Dn.indptr, Dn.indices, Dn.data, N_H, M_H, ip, ix),
             roc_dense(S, *empty), roc_csr(*csr, *empty), roc_dense(S, *full, cap=2 * N_H * M_H + 2)]
    calls += [roc_dense(S, ip, ix, null=(k,)) for k in ("fps", "tps", "thr", "n", "counts", "auc")]
    calls += [roc_csr(*csr, ip, ix, null=(k,)) for k in ("fps", "tps", "thr", "n", "counts", "auc")]
    for rc, out in calls:
        assert rc == EINVAL and out.untouched()


# --------------------------------------------------------------------------------- the routes with the switch unset
@pytest.fixture
def no_library(monkeypatch):
    from opentf_amd import libntf

    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(libntf, "lib", refuse)


def test_routes_without_the_switch(no_library, monkeypatch):
    from sklearn import metrics as skm
    from opentf_amd.evl import metric
    lab, S = _family("zeros_80", 7)
    Y = sp.csr_matrix(lab.astype(np.float32))
    want_auc = skm.roc_auc_score(Y.toarray(), S, average="micro", multi_class="ovr")
    want_fpr, want_tpr, _ = skm.roc_curve(lab.ravel(), S.ravel())
    for pred in (S, sp.csr_matrix(S)):
        for kw in ({}, {"device": 0}, {"curve_device": None}, {"device": 0, "curve_device": None}):
            auc, (fpr, tpr) = metric.calculate_auc_roc(Y, pred, curve=True, **kw)
            assert auc == want_auc and np.array_equal(fpr, want_fpr) and np.array_equal(tpr, want_tpr)
        # without the curve, curve_device changes nothing either
        assert metric.calculate_auc_roc(Y, pred, curve_device=0) == metric.calculate_auc_roc(Y, pred)
    # a dense prediction that is not f32 stays with sklearn, as it does for `device`
    auc, (fpr, tpr) = metric.calculate_auc_roc(Y, S.astype(np.float64), curve=True, curve_device=0)
    assert auc == want_auc and np.array_equal(fpr, want_fpr)
    spec = metric.EvalSpec(10, False, [], ["aucroc+"])
    rows = np.arange(N_H)
    for env in ({}, {"NTF_ROC_DEVICE": "0"}, {"NTF_AUC_DEVICE": "1"}):
        for k in ("NTF_ROC_DEVICE", "NTF_AUC_DEVICE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for pred in (S, sp.csr_matrix(S)):
            _, mean, roc = metric.score_predictions({"member": Y}, rows, pred, spec)
            assert mean.loc["aucroc", "mean"] == want_auc and np.array_equal(roc[0], want_fpr) and np.array_equal(roc[1], want_tpr)
    # and the switch does reach for the library
    monkeypatch.setenv("NTF_ROC_DEVICE", "1")
    with pytest.raises(AssertionError, match="the library was touched"):
        metric.score_predictions({"member": Y}, rows, S, spec)
    with pytest.raises(AssertionError, match="the library was touched"):
        metric.calculate_auc_roc(Y, sp.csr_matrix(S), curve=True, curve_device=0)


def test_micro_roc_device_refuses_on_the_host(no_library):
    from opentf_amd.evl import metric
    lab, S = _family("uniform", 9)
    Y = sp.csr_matrix(lab.astype(np.float32))
    for one_class in (sp.csr_matrix((N_H, M_H), dtype=np.float32), sp.csr_matrix(np.ones((N_H, M_H), dtype=np.float32))):
        for pred in (S, sp.csr_matrix(S)):
            with pytest.raises(ValueError, match="Only one class present in y_true"):
                metric.micro_roc_device(one_class, pred)
    for dtype in (np.float64, np.int32):
        with pytest.raises(TypeError, match="micro_roc_device"):
            metric.micro_roc_device(Y, S.astype(dtype))
