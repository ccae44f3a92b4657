"""The host side of the device AUC (opentf_amd/evl/metric.py) and the yardstick of tests/test_gpu_auc.py, where no GPU is needed:
`micro_auc_device` refuses what it must before it touches the library, `calculate_auc_roc` without a device takes exactly the routes it
always took, and the integer Mann-Whitney oracle the GPU tests compare with agrees with sklearn."""
import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_auc import FAMILIES, M_RAG, N_RAG, auc_of, check_family, family, labels, oracle_counts, sklearn_auc


@pytest.fixture
def no_library(monkeypatch):
    from opentf_amd import libntf

    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(libntf, "lib", refuse)


def test_micro_auc_device_refuses_on_the_host(no_library):
    from opentf_amd.evl import metric
    lab = labels(20, 300, 0.03, 1)
    Y = sp.csr_matrix(lab.astype(np.float32))
    S = family("uniform", 20, 300, 2)
    for one_class in (sp.csr_matrix((20, 300), dtype=np.float32), sp.csr_matrix(np.ones((20, 300), dtype=np.float32))):
        for pred in (S, sp.csr_matrix(S)):
            with pytest.raises(ValueError, match="Only one class present in y_true"):
                metric.micro_auc_device(one_class, pred)
    zeros_stored = Y.copy(); zeros_stored.data[:] = 0                 # explicit zeros are no positives
    with pytest.raises(ValueError, match="Only one class present in y_true"):
        metric.micro_auc_device(zeros_stored, S)
    try:
        metric.micro_auc_sparse(sp.csr_matrix((20, 300), dtype=np.float32), sp.csr_matrix(S))
    except ValueError as e:
        with pytest.raises(ValueError) as same:
            metric.micro_auc_device(sp.csr_matrix((20, 300), dtype=np.float32), sp.csr_matrix(S))
        assert str(same.value) == str(e)
    for dtype in (np.float64, np.int32, np.longdouble):
        with pytest.raises(TypeError):
            metric.micro_auc_device(Y, S.astype(dtype))


def test_default_route_is_unchanged(no_library):
    from sklearn import metrics as skm
    from opentf_amd.evl import metric
    lab = labels(20, 300, 0.03, 1)
    Y = sp.csr_matrix(lab.astype(np.float32))
    S = family("zero_heavy", 20, 300, 2)
    auc, curve = metric.calculate_auc_roc(Y, S)
    assert curve is None and auc == skm.roc_auc_score(Y.toarray(), S, average="micro", multi_class="ovr")      # dense: sklearn itself
    assert auc == metric.calculate_auc_roc(Y, S, device=None)[0]
    Ssp = sp.csr_matrix(S)
    auc_s, curve = metric.calculate_auc_roc(Y, Ssp)
    assert curve is None and auc_s == metric.micro_auc_sparse(Y, Ssp) and abs(auc_s - auc) <= 1e-12
    # the curve stays sklearn whatever `device` says
    a, (fpr, tpr) = metric.calculate_auc_roc(Y, S, curve=True, device=0)
    assert a == auc and fpr[0] == 0.0 and tpr[-1] == 1.0
    assert abs(auc_of(oracle_counts(S, lab)) - auc) <= 1e-12


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_agrees_with_sklearn(name):
    lab = labels(N_RAG, M_RAG, 0.02, 11)
    S = family(name, N_RAG, M_RAG, 12)
    check_family(name, S, lab)
    P, N, U2 = oracle_counts(S, lab)
    assert P == int(lab.sum()) and P + N == lab.size and 0 <= U2 <= 2 * P * N
    assert abs(auc_of((P, N, U2)) - sklearn_auc(S, lab)) <= 1e-12
