"""Host side of DetConstSort and the infeasible measures (include/opentf_amd_fairsort.h, opentf_amd/evl/fair.py): hand-worked rows of the pin
(tests/fair_sort_reference.py), the invariant the header's swap guard keeps and the paper's printed guard breaks, the measure on a DetGreedy output that misses
a group, and the header / export / binding surface.  Needs no GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import fair_reference as R
import fair_sort_reference as S
from conftest import ROOT

HALVES = ([0, 0, 0, 1, 1, 1], [0.5, 0.5], 6)             # the header's first hand row
# four groups owed 1/18, 6/18, 5/18, 6/18: after four ranks every group holds one entry and nobody is below its floor; at k = 5 DetGreedy takes the best of those
# below their ceiling (position 4, group 2); at k = 6 groups 1 and 3 are BOTH owed floor(6 * 6/18) = 2 and one rank is left.  No group runs out of candidates.
GREEDY_MISS = ([2, 3, 0, 1, 2, 2, 2, 1, 3, 3, 1, 3], [1 / 18, 6 / 18, 5 / 18, 6 / 18], 6)


def _rows(seed, n, K, G, skew=1.0):
    """n random rows of K labels with random targets; every group holds what the header's sufficient condition asks for at K_out = K // 2"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = rng.dirichlet(np.full(G, skew))
        groups = rng.integers(0, G, K).tolist()
        if all(groups.count(g) >= math.floor((K // 2 + G + 1) * p[g]) for g in range(G)):
            out.append((groups, p.tolist(), K // 2))
    return out


# --------------------------------------------------------------------------------- the pin, by hand
def test_reference_hand_rows():
    # k=2: both groups fall due (t = 1, 1), heads 0 and 3 in that order; k=4: heads 1 and 4; k=6: heads 2 and 5.  Position 1 (deadline 4) enters at rank 3 behind
    # position 3, whose deadline 2 < 3 holds it at rank 2: no swap anywhere
    st = {}
    assert S.constsort_row(*HALVES, stats=st) == ([0, 3, 1, 4, 2, 5], 0, [2, 2, 4, 4, 6, 6]) and st["longest"] == 0
    # k=2: t = (1, 0): position 2.  k=3: t = (2, 0): position 3.  k=4: t = (3, 1): heads 0 (group 1) and 4 (group 0), in that order: position 0 enters at rank 3,
    # passes position 3 (deadline 3 >= 3) and position 2 (deadline 2 >= 2) and heads the list; position 4 fills rank 4
    st = {}
    assert S.constsort_row([1, 1, 0, 0, 0, 0], [0.75, 0.25], 4, stats=st) == ([0, 2, 3, 4], 0, [4, 2, 3, 4]) and st["longest"] == 2


def test_reference_tail_and_prefix():
    # group 1 has no candidate: group 0 falls due at k = 2, 4, 6 and the loop ends at k = K_out + G + 1 = 7 with three ranks; the tail rule fills the fourth
    assert S.constsort_row([0, 0, 0, 0], [0.5, 0.5], 4)[:2] == ([0, 1, 2, 3], 1)
    # a zero target never falls due: its candidates come only through the tail
    assert S.constsort_row([1, 0, 1, 0], [1.0, 0.0], 4)[:2] == ([1, 3, 0, 2], 2)
    # K_out < K stops the loop in the middle of a step: at k = 2 both groups are due and one rank is asked for
    assert S.constsort_row([0, 1, 0, 1], [0.5, 0.5], 1)[:2] == ([0], 0)
    # the header's caveat: group 1 runs out, the loop's last steps (k = 6 <= K_out + G + 1) fill the list, the tail count is 0 and group 1 is one short at rank 4
    pos, tail, _ = S.constsort_row([0, 0, 0, 1], [0.5, 0.5], 4)
    assert (pos, tail) == ([0, 3, 1, 2], 0)
    assert S.infeasible_row([[0, 0, 0, 1][j] for j in pos], [0.5, 0.5], [1, 2, 3, 4]) == ([0, 0, 0, 1], [0, 0, 0, 1])


def test_infeasible_by_hand():
    # k=1: floors (0, 0); k=2: (1, 1), group 1 has none; k=3: (1, 1) still none; k=4: (2, 2): group 0 holds 3, group 1 one
    assert S.infeasible_row([0, 0, 0, 1], [0.5, 0.5], [1, 2, 3, 4]) == ([0, 1, 2, 3], [0, 1, 2, 3])
    # two groups short at one rank count twice in the count, once in the index
    assert S.infeasible_row([0, 0, 0], [1 / 3, 1 / 3, 1 / 3], [3]) == ([1], [2])


# --------------------------------------------------------------------------------- the guarantee
@pytest.mark.parametrize("G,K,skew", [(2, 40, 1.0), (3, 60, 0.5), (8, 96, 1.0), (5, 30, 0.3)])
def test_no_entry_sits_below_its_deadline_and_the_result_is_feasible(G, K, skew):
    for groups, p, k_out in _rows(100 + G, 25, K, G, skew):
        pos, tail, dl = S.constsort_row(groups, p, k_out)
        assert sorted(set(pos)) == sorted(pos) and len(pos) == k_out and len(dl) == k_out - tail
        assert all(r + 1 <= d for r, d in enumerate(dl)), (groups, p)
        assert tail == 0                                                          # (the rows were drawn so that no group can run out)
        index, count = S.infeasible_row([groups[j] for j in pos], p, list(range(1, k_out + 1)))
        assert index == [0] * k_out and count == [0] * k_out, (groups, p)


def test_the_deadline_invariant_holds_under_exhaustion_too():
    for groups, p, _ in _rows(7, 25, 40, 3):
        pos, tail, dl = S.constsort_row(groups[:14], p, 14)                       # 14 candidates: groups do run out
        assert all(r + 1 <= d for r, d in enumerate(dl)) and len(dl) == 14 - tail


def test_the_papers_printed_guard_breaks_the_first_hand_row():
    # the printed guard, `maxIndices[start - 1] >= start` with 0-based slots: the neighbour's deadline (a rank, 1-based) against the SLOT the new entry leaves, which
    # is the rank the neighbour lands on minus one - it lets an entry due by rank D end at rank D + 1
    printed = lambda deadline, r: deadline >= r - 1
    pos, _, dl = S.constsort_row(*HALVES, guard=printed)
    assert pos[:3] == [0, 1, 3] and dl[2] == 2                                    # position 3, due by rank 2, sits at rank 3
    assert S.infeasible_row([HALVES[0][j] for j in pos], HALVES[1], [2])[0] == [1]
    assert S.infeasible_row([HALVES[0][j] for j in S.constsort_row(*HALVES)[0]], HALVES[1], [2, 6])[0] == [0, 0]


def test_the_measure_sees_what_detgreedy_misses():
    groups, p, k_out = GREEDY_MISS
    assert all(groups.count(g) >= math.floor((k_out + len(p) + 1) * p[g]) for g in range(len(p)))          # nobody runs out
    greedy = R.rerank_row(groups, p, R.DET_GREEDY, k_out)
    assert greedy == [0, 1, 3, 2, 4, 7]
    assert S.infeasible_row([groups[j] for j in greedy], p, [5, 6]) == ([0, 1], [0, 1])                     # group 3 holds one of the two it is owed at k = 6
    pos, tail, _ = S.constsort_row(groups, p, k_out)
    assert tail == 0 and S.infeasible_row([groups[j] for j in pos], p, [5, 6]) == ([0, 0], [0, 0])


# --------------------------------------------------------------------------------- header, exports, binding
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ntf_\w+)\s*\(", src)))


def test_fairsort_header_exports_and_binding_agree():
    from opentf_amd import libntf
    assert _declared("opentf_amd_fairsort.h") == ["ntf_fair_constsort", "ntf_fair_infeasible"] == sorted(libntf.FAIRSORT_SYMBOLS)
    path = os.path.join(ROOT, "opentf_amd", "libopentf_amd.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(path)
    lib = libntf.lib()
    for name, (res, args) in libntf.FAIRSORT_SYMBOLS.items():
        assert hasattr(raw, name), f"{name} declared in include/opentf_amd_fairsort.h but not exported"
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    # ntf_fair_rerank's arguments without the algorithm, plus out_tail; ntf_fair_metrics' arguments (the two outputs are int32 here)
    rerank, metrics = libntf.FAIR_SYMBOLS["ntf_fair_rerank"][1], libntf.FAIR_SYMBOLS["ntf_fair_metrics"][1]
    assert libntf.FAIRSORT_SYMBOLS["ntf_fair_constsort"] == (ctypes.c_int, rerank[:1] + rerank[2:] + [ctypes.c_void_p])
    assert libntf.FAIRSORT_SYMBOLS["ntf_fair_infeasible"] == (ctypes.c_int, metrics)


def test_fairsort_entries_are_declared_nowhere_else():
    from opentf_amd import libntf
    for header in ("opentf_amd.h", "opentf_amd_fair.h", "opentf_amd_link.h", "opentf_amd_roc.h"):
        assert not set(_declared(header)) & set(libntf.FAIRSORT_SYMBOLS), header
    for table in (libntf.SYMBOLS, libntf.FAIR_SYMBOLS, libntf.LINK_SYMBOLS, libntf.ROC_SYMBOLS):
        assert not set(table) & set(libntf.FAIRSORT_SYMBOLS)
    assert sorted(libntf.FAIR_SYMBOLS) == ["ntf_fair_metrics", "ntf_fair_rerank"] and sorted(libntf.FAIR_ALGORITHMS) == ["det_cons", "det_greedy", "det_relaxed"]
    assert libntf.NTF_ABI_VERSION == 2 and libntf.lib().ntf_abi_version() == 2
    src = open(os.path.join(ROOT, "include", "opentf_amd_fairsort.h")).read()
    assert '#include "opentf_amd_fair.h"' in src and "#define" not in re.sub(r"#define OPENTF_AMD_FAIRSORT_H", "", src)      # limits and codes by reference


def test_fairspec_accepts_the_new_name_and_the_new_key():
    from opentf_amd.evl import fair
    spec = fair.FairSpec.from_cfg({"algorithm": "det_const_sort", "k_max": 20, "infeasible": True})
    assert spec.algorithm == "det_const_sort" and spec.infeasible is True
    assert fair.fair_stem("f0.test.pred", spec) == "f0.test.pred.det_const_sort.dp.popularity.k20"
    assert fair.FairSpec.from_cfg({}).infeasible is False and fair.FairSpec.from_cfg({"algorithm": "det_cons"}).infeasible is False
    assert fair.FairSpec.from_cfg({"infeasible": "false"}).infeasible is False and fair.FairSpec.from_cfg({"infeasible": " True"}).infeasible is True
    with pytest.raises(ValueError):
        fair.FairSpec(infeasible="maybe")
    with pytest.raises(ValueError):
        fair.FairSpec(algorithm="fa*ir")
    with pytest.raises(ValueError):
        fair.FairSpec.from_cfg({"algorithm": "fa*ir", "infeasible": True})
