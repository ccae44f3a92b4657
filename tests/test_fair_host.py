"""Host side of the fair stage (include/opentf_amd_fair.h, opentf_amd/evl/fair.py): hand-worked cases of the pin (tests/fair_reference.py), the header / export /
binding surface, and the two input builders (popularity groups, target distributions) on toy matrices.  Needs no GPU."""
import ctypes
import math
import os
import re

import numpy as np
import scipy.sparse as sp

import fair_reference as R
from conftest import ROOT

ALGS = (R.DET_GREEDY, R.DET_CONS, R.DET_RELAXED)


# --------------------------------------------------------------------------------- the pin, by hand
def test_reference_alternates_two_equal_groups():
    # k=1: both in B, smaller head -> 0; k=2: group 1 is below floor(2 * 0.5) = 1 -> its head 3; and so on
    assert R.rerank_row([0, 0, 0, 1, 1, 1], [0.5, 0.5], R.DET_GREEDY, 6) == [0, 3, 1, 4, 2, 5]


def test_reference_leaves_a_proportional_row_unchanged():
    for alg in ALGS:
        assert R.rerank_row([0, 1, 0, 1, 0, 1], [0.5, 0.5], alg, 6) == [0, 1, 2, 3, 4, 5]
        assert R.rerank_row([0, 0, 1, 0, 0, 1, 0, 0, 1], [2 / 3, 1 / 3], alg, 9) == list(range(9))


def test_reference_detcons_and_detgreedy_differ():
    # k=1: both groups in B.  DetGreedy takes the smaller head (position 0, group 1); DetCons the smaller ceil(k p) / p: 1 / 0.7 < 1 / 0.3 -> group 0's head 1.
    # DetCons then: k=2 keys 2 / 0.7 < 1 / 0.3 -> 2; k=3 keys 3 / 0.7 > 1 / 0.3 -> group 1's head 0; k=4 group 1 is exhausted -> 3
    groups, p = [1, 0, 0, 0], [0.7, 0.3]
    assert R.rerank_row(groups, p, R.DET_GREEDY, 4) == [0, 1, 2, 3]
    assert R.rerank_row(groups, p, R.DET_CONS, 4) == [1, 2, 0, 3]
    assert R.rerank_row(groups, p, R.DET_RELAXED, 4) == [1, 2, 0, 3]


def test_reference_detrelaxed_ties_where_detcons_does_not():
    # k=1, all in B: keys 1 / 0.4 = 2.5, 1 / 0.35 = 2.86, 1 / 0.25 = 4.  DetCons: group 0 (position 1).  DetRelaxed: ceil gives 3, 3, 4 - a tie, the smaller head wins
    groups, p = [1, 0, 2], [0.4, 0.35, 0.25]
    assert R.rerank_row(groups, p, R.DET_CONS, 1) == [1]
    assert R.rerank_row(groups, p, R.DET_RELAXED, 1) == [0]


def test_reference_exhausted_group_takes_the_fallback():
    # group 1 has no candidate: at k=2, floor = ceil = 1 = cnt[0], so neither A nor B holds a live group - the best remaining candidate is taken
    for alg in ALGS:
        assert R.rerank_row([0, 0, 0, 0], [0.5, 0.5], alg, 4) == [0, 1, 2, 3]
    # and a group that runs out half way: its share goes to whoever is left
    assert R.rerank_row([1, 0, 0, 0, 0], [0.5, 0.5], R.DET_GREEDY, 5) == [0, 1, 2, 3, 4]


def test_reference_k_out_is_a_prefix_and_values_keep_their_ranks():
    idx, val, pos = R.rerank([[7, 8, 9, 3]], [[0.9, 0.5, 0.4, 0.1]], {7: 0, 8: 0, 9: 0, 3: 1}, [[0.5, 0.5]], R.DET_GREEDY, 2)
    assert pos == [[0, 3]] and idx == [[7, 3]] and val == [[0.9, 0.5]]


def test_reference_measures_by_hand():
    ndkl, skew, absn = R.metrics_row([0, 1], [0.5, 0.5], [1, 2])
    # k=1: d = (1, 0): KL = ln 2, w = 1;  k=2: d = (0.5, 0.5): KL = 0, w = 1 / log2(3)
    assert ndkl[0] == math.log(2.0) and ndkl[1] == math.log(2.0) / (1.0 + 1.0 / math.log2(3))
    assert skew == [[math.log(2.0), -math.inf], [0.0, 0.0]] and absn == ndkl
    ndkl, skew, _ = R.metrics_row([0, 0], [0.0, 1.0, 0.0], [2])
    assert ndkl == [math.inf] and skew == [[math.inf, -math.inf, 0.0]]


# --------------------------------------------------------------------------------- header, exports, binding
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ntf_\w+)\s*\(", src)))


def test_fair_header_exports_and_binding_agree():
    from opentf_amd import libntf
    declared = _declared("opentf_amd_fair.h")
    assert declared == ["ntf_fair_metrics", "ntf_fair_rerank"] == sorted(libntf.FAIR_SYMBOLS)
    path = os.path.join(ROOT, "opentf_amd", "libopentf_amd.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(path)
    lib = libntf.lib()
    for name, (res, args) in libntf.FAIR_SYMBOLS.items():
        assert hasattr(raw, name), f"{name} declared in include/opentf_amd_fair.h but not exported"
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    assert libntf.FAIR_SYMBOLS["ntf_fair_rerank"][1] == [ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                         ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 3
    assert libntf.FAIR_SYMBOLS["ntf_fair_metrics"][1] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                          ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]


def test_fair_entries_stay_out_of_the_main_header():
    from opentf_amd import libntf
    main = _declared("opentf_amd.h")
    for name in libntf.FAIR_SYMBOLS:
        assert name not in main and name not in libntf.SYMBOLS
    assert libntf.NTF_ABI_VERSION == 2 and libntf.lib().ntf_abi_version() == 2
    src = open(os.path.join(ROOT, "include", "opentf_amd_fair.h")).read()
    assert int(re.search(r"#define NTF_FAIR_MAX_GROUPS\s+(\d+)", src).group(1)) == libntf.NTF_FAIR_MAX_GROUPS == 64
    assert int(re.search(r"#define NTF_FAIR_MAX_K\s+(\d+)", src).group(1)) == libntf.NTF_FAIR_MAX_K == 2048
    assert (libntf.FAIR_DET_GREEDY, libntf.FAIR_DET_CONS, libntf.FAIR_DET_RELAXED) == ALGS


# --------------------------------------------------------------------------------- the input builders
def _member():
    # 5 teams x 4 experts: expert 0 sits in three teams, experts 1 and 2 in one each, expert 3 in none; team 3 has no member
    return sp.csr_matrix(np.array([[1, 1, 0, 0], [1, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint8))


def test_popularity_groups():
    from opentf_amd.evl import fair
    group, names = fair.popularity_groups(_member())
    assert names == ("nonpopular", "popular") and group.dtype == np.uint8
    assert group.tolist() == [1, 0, 0, 0]            # counts (3, 1, 1, 0): mean over the three experts with a team = 5 / 3
    assert fair.popularity_groups(_member().tolil())[0].tolist() == [1, 0, 0, 0]
    assert fair.popularity_groups(_member(), rows=[0])[0].tolist() == [0, 0, 0, 0]      # counts (1, 1, 0, 0): nobody exceeds the mean 1
    assert fair.popularity_groups(_member(), rows=[0, 1])[0].tolist() == [1, 0, 0, 0]   # counts (2, 1, 0, 0): mean 1.5
    assert fair.popularity_groups(_member(), rows=[3])[0].tolist() == [0, 0, 0, 0]      # no team member at all


def test_target_distribution():
    from opentf_amd.evl import fair
    group = np.array([1, 0, 0, 0], dtype=np.uint8)
    dp = fair.target_distribution("dp", group, 2)
    assert dp.shape == (1, 2) and dp.dtype == np.float64 and dp.tolist() == [[0.75, 0.25]]
    assert fair.target_distribution("dp", group, 3).tolist() == [[0.75, 0.25, 0.0]]
    eo = fair.target_distribution("eo", group, 2, _member())
    assert eo.shape == (5, 2)
    assert eo.tolist() == [[0.5, 0.5], [0.0, 1.0], [0.5, 0.5], [0.75, 0.25], [0.75, 0.25]]       # the teams without a member take the dp row
    assert np.abs(eo.sum(axis=1) - 1.0).max() <= 1e-12


def test_load_groups_and_spec(tmp_path):
    import pytest
    from opentf_amd.evl import fair
    np.save(tmp_path / "gender.npy", np.array([0, 2, 1, 0], dtype=np.int64))
    group, names = fair.load_groups(str(tmp_path / "gender.npy"), 4)
    assert group.dtype == np.uint8 and group.tolist() == [0, 2, 1, 0] and names == ("0", "1", "2")
    with pytest.raises(ValueError):
        fair.load_groups(str(tmp_path / "gender.npy"), 5)
    spec = fair.FairSpec.from_cfg({"algorithm": "det_cons", "notion": "eo", "attribute": str(tmp_path / "gender.npy"), "k_max": 20, "cutoffs": [5, 10]})
    assert fair.fair_stem("/run/f0.test.pred", spec) == "/run/f0.test.pred.det_cons.eo.gender.k20"
    assert fair.fair_stem("f0.test.pred", fair.FairSpec.from_cfg({})) == "f0.test.pred.det_greedy.dp.popularity.k100"
    with pytest.raises(ValueError):
        fair.FairSpec(algorithm="fa*ir")
