"""DetConstSort and the infeasible measures on a real MI355X (opentf_amd/csrc/ntf_fair.hip k_fair_constsort / k_fair_infeasible, include/opentf_amd_fairsort.h,
opentf_amd/evl/fair.py, Ntf.adila) against the pin tests/fair_sort_reference.py.  Everything is integer logic plus one IEEE product: every comparison is EQUALITY.
Each shape sits where the kernel can break: the 64-rank chunks of the scan and the shift (K = 63, 64, 65, 129, insertions longer than one and two chunks), the rows
of a workgroup (n = 1, 4, 5, 9), K = 2048 with 2 and 64 groups.  Only the cases of TAIL exercise the tail rule; for every other case the reference alone shows, on
the CPU, that its tail count is 0, so that no equality below compares two tail fills.  Each case's reference is computed once and shared."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import scipy.sparse
import torch

import fair_reference as R
import fair_sort_reference as S
from test_fair_sort_host import GREEDY_MISS
from test_gpu_fair import Cfg, _toy

pytestmark = pytest.mark.gpu

EINVAL = -1            # NTF_EINVAL, include/opentf_amd.h
POOL = 2048            # experts per group: expert e belongs to group e % G


def _counts_that_last(p, K):
    """how many candidates of each group a row of K must hold for DetConstSort at K_out = K to end with nobody short: what every group is owed at the last k
    whose dues fit into K ranks, the rest going to groups that fall due at the next k"""
    G = len(p)
    owed = lambda k: [math.floor(float(k) * float(p[g])) for g in range(G)]
    k = 1
    while sum(owed(k + 1)) <= K:
        k += 1
    counts, nxt = owed(k), owed(k + 1)
    due = [g for g in range(G) if nxt[g] > counts[g]]
    for g in due[:K - sum(counts)]:
        counts[g] += 1
    assert sum(counts) == K
    return counts


def _row(rng, G, labels):
    """ids with these labels, in this order: distinct experts of group g are g + G * (a draw without replacement)"""
    labels = np.asarray(labels)
    ids = np.empty(len(labels), np.int64)
    for g in range(G):
        at = np.nonzero(labels == g)[0]
        ids[at] = g + G * rng.choice(POOL, size=len(at), replace=False)
    return ids


def _matched(rng, p, K, order):
    """labels of one row whose composition lasts to K_out = K (see _counts_that_last): shuffled, or in blocks by group ascending ('up') / descending ('down')"""
    labels = np.repeat(np.arange(len(p)), _counts_that_last(p, K))
    return rng.permutation(labels) if order == "shuffled" else labels if order == "up" else labels[::-1]


TAIL = ("exhaust", "zero_tail")
SEEDS = {"k1": 1, "k2": 2, "k63": 3, "k64": 4, "k65": 5, "k129": 6, "skew": 7, "deep2": 8, "deep64": 9, "prefix": 10, "zero_p": 11, "almost_one": 12, "exhaust": 13,
         "zero_tail": 14}
CASES = tuple(SEEDS)
LONGEST = {"k129": 64, "skew": 64, "deep2": 128, "deep64": 32}       # the most swaps one insertion makes exceeds this: the scan crosses one / two chunk edges


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(idx [n, K], val [n, K], group [n_experts], p [n_p, G], k_out)"""
    rng = np.random.default_rng(SEEDS[name])
    k_out = None
    if name == "k1":                          # one rank, one group, one row: a workgroup with three idle waves
        p = [[1.0]]; rows = [_matched(rng, p[0], 1, "up")]
    elif name == "k2":                        # n = 4: one full workgroup; both groups fall due at k = 2
        p = [[0.5, 0.5]]; rows = [_matched(rng, p[0], 2, "shuffled") for _ in range(4)]
    elif name == "k63":                       # one rank short of a chunk; n = 5: a second workgroup with one row
        p = [[0.5, 0.3, 0.2]]; rows = [_matched(rng, p[0], 63, "shuffled") for _ in range(5)]
    elif name == "k64":                       # exactly one chunk; n = 9
        p = [[0.5, 0.5]]; rows = [_matched(rng, p[0], 64, o) for o in ("shuffled", "up", "down") * 3]
    elif name == "k65":                       # one rank into the second chunk; four groups fall due at one k
        p = [[0.25] * 4]; rows = [_matched(rng, p[0], 65, o) for o in ("shuffled", "down", "shuffled", "up", "shuffled")]
    elif name == "k129":                      # two chunks and one rank, one target per row.  A group owed 1 % falls due at k = 100, when 98 majority entries with one
        # rank of slack each stand in the list: from the top of the input its candidate passes them all (no stop in either chunk); with two such groups the second
        # candidate stops behind the first (a stop in the second chunk)
        p = [[0.98, 0.01, 0.01]] * 3 + [[0.01, 0.98, 0.01]] * 3 + [[1 / 3] * 3] * 3
        rows = [_matched(rng, p[i], 129, o) for i, o in enumerate(("down", "up", "shuffled") * 3)]
    elif name == "skew":                      # [0.9, 0.1] with the minority at the bottom and at the top of the input, and a rarer minority whose entries, when they
        p = [[0.9, 0.1]] * 2 + [[0.99, 0.01]] * 2        # fall due, pass a hundred majority entries that each have one rank of slack
        rows = [_matched(rng, p[i], 300, o) for i, o in enumerate(("up", "down", "up", "down"))]
    elif name == "deep2":                     # the deepest list, two groups: the minority's entries pass two hundred ranks (three chunks of the scan)
        p = [[0.9, 0.1], [0.995, 0.005], [0.995, 0.005], [0.5, 0.5], [0.3, 0.7]]
        rows = [_matched(rng, p[i], 2048, o) for i, o in enumerate(("up", "down", "shuffled", "shuffled", "down"))]
    elif name == "deep64":                    # the deepest list and the most groups, a nearly flat target
        q = 0.5 + rng.random(64); p = [(q / q.sum()).tolist()]
        rows = [_matched(rng, p[0], 2048, o) for o in ("shuffled", "down", "up", "shuffled")]
    elif name == "prefix":                    # K_out < K, one target per row; every group holds far more than it is owed in 37 ranks
        p = rng.dirichlet(np.full(3, 4.0), size=9).tolist(); k_out = 37
        rows = [rng.permutation(np.repeat(np.arange(3), [34, 33, 33])) for _ in range(9)]
    elif name == "zero_p":                    # a target of 0 never falls due: K_out < K keeps its candidates out without the tail rule
        p = [[0.5, 0.0, 0.5]]; k_out = 40
        rows = [rng.permutation(np.repeat(np.arange(3), [30, 20, 30])) for _ in range(6)]
    elif name == "almost_one":                # a target summing to 1 - 5e-7: group 1 falls due one k late throughout
        p = [[0.5, 0.5 - 5e-7]]; rows = [_matched(rng, p[0], 64, "shuffled") for _ in range(4)]
    elif name == "exhaust":                   # TAIL: group 2 holds two candidates and is owed fifteen
        p = [[0.4, 0.3, 0.3]]; rows = [rng.permutation(np.repeat(np.arange(3), [28, 20, 2])) for _ in range(5)]
    elif name == "zero_tail":                 # TAIL: K_out = K with a target of 0: that group's candidates come last, through the tail rule
        p = [[0.5, 0.0, 0.5]]; rows = [rng.permutation(np.repeat(np.arange(3), [15, 10, 15])) for _ in range(4)]
    G = len(p[0])
    idx = np.stack([_row(rng, G, r) for r in rows]).astype(np.int32)
    val = -np.sort(-rng.random(idx.shape).astype(np.float32), axis=1)
    return dict(idx=idx, val=val, group=(np.arange(G * POOL) % G).astype(np.uint8), p=np.ascontiguousarray(p, dtype=np.float64), k_out=k_out or idx.shape[1])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (idx, pos, tail, longest insertion) of the pin"""
    c, st = case(name), {}
    idx, pos, tail = S.constsort(c["idx"].tolist(), c["group"].tolist(), c["p"].tolist(), c["k_out"], stats=st)
    return np.array(idx, np.int32), np.array(pos, np.int32), np.array(tail, np.int32), st["longest"]


@functools.lru_cache(maxsize=None)
def device(name):
    from opentf_amd import libntf
    c = case(name)
    return libntf.fair_constsort(c["idx"], c["val"], c["group"], c["p"], k_out=c["k_out"], want_pos=True, want_tail=True)


def _cuts(k):
    return sorted({c for c in (1, 2, 63, 64, 65, 129, k - 1, k) if 1 <= c <= k})[-8:]


# --------------------------------------------------------------------------------- the re-ranker
@pytest.mark.parametrize("name", CASES)
def test_constsort_equals_the_reference(name):
    c = case(name)
    ridx, rpos, rtail, longest = reference(name)
    if name in TAIL:
        assert rtail.min() > 0
    else:
        assert (rtail == 0).all(), (name, rtail)                  # the reference alone, on the CPU: the equalities below compare no tail fill
    assert longest > LONGEST.get(name, -1), (name, longest)
    idx, val, pos, tail = device(name)
    n, k_out = len(c["idx"]), c["k_out"]
    assert pos.shape == idx.shape == val.shape == (n, k_out) and tail.shape == (n,)
    assert pos.dtype == idx.dtype == tail.dtype == np.int32 and val.dtype == np.float32
    assert np.array_equal(tail, rtail)
    assert np.array_equal(pos, rpos), (name, np.argwhere(pos != rpos)[:4])
    assert np.array_equal(idx, ridx)
    assert np.array_equal(val.view(np.uint32), c["val"][:, :k_out].view(np.uint32))        # the r-th largest score goes to the r-th re-ranked expert


def test_constsort_without_values_positions_and_tail():
    from opentf_amd import libntf
    for name in ("k65", "prefix"):
        c = case(name)
        idx, val = libntf.fair_constsort(c["idx"], None, c["group"], c["p"], k_out=c["k_out"])
        assert val is None and idx.tobytes() == device(name)[0].tobytes()
        idx, val, tail = libntf.fair_constsort(c["idx"], c["val"], c["group"], c["p"], k_out=c["k_out"], want_tail=True)
        assert idx.tobytes() == device(name)[0].tobytes() and val.tobytes() == device(name)[1].tobytes() and tail.tobytes() == device(name)[3].tobytes()


@pytest.mark.parametrize("name,cut", [("prefix", 4), ("prefix", 5), ("k129", 1), ("skew", 3)])
def test_constsort_is_bit_identical_under_a_split_of_the_rows(name, cut):
    from opentf_amd import libntf
    c = case(name)
    per_row = len(c["p"]) > 1
    parts = [libntf.fair_constsort(c["idx"][s], c["val"][s], c["group"], c["p"][s] if per_row else c["p"], k_out=c["k_out"], want_pos=True, want_tail=True)
             for s in (slice(0, cut), slice(cut, None))]
    for whole, a, b in zip(device(name), *parts):
        assert np.concatenate([a, b]).tobytes() == whole.tobytes()


def test_the_three_other_algorithms_go_where_they_went():
    from opentf_amd import libntf
    from opentf_amd.evl import fair
    c = case("prefix")
    for alg, code in (("det_greedy", R.DET_GREEDY), ("det_cons", R.DET_CONS), ("det_relaxed", R.DET_RELAXED)):
        idx, val = fair.rerank(c["idx"], c["val"], c["group"], c["p"], alg, c["k_out"])
        direct = libntf.fair_rerank(c["idx"], c["val"], c["group"], c["p"], alg, k_out=c["k_out"])
        assert idx.tobytes() == direct[0].tobytes() and val.tobytes() == direct[1].tobytes()
        assert np.array_equal(idx, np.array(R.rerank(c["idx"].tolist(), None, c["group"].tolist(), c["p"].tolist(), code, c["k_out"])[0], np.int32))
    idx, val = fair.rerank(c["idx"], c["val"], c["group"], c["p"], "det_const_sort", c["k_out"])
    assert np.array_equal(idx, reference("prefix")[0]) and val.tobytes() == device("prefix")[1].tobytes()


# --------------------------------------------------------------------------------- the measure
@pytest.mark.parametrize("name", CASES)
def test_the_devices_own_output_is_feasible_where_no_tail_was_needed(name):
    """A tail count of 0 does not by itself make a list feasible (the header's caveat: a group can run out and the loop's last steps still fill the list).  It does
    here because every case outside TAIL is built by `_matched` / `_counts_that_last`, or holds far more of every group than K_out ranks owe it: no group runs out
    while one is due.  A case added without that property fails this test for that reason, not for a fault of the kernel."""
    from opentf_amd import libntf
    c = case(name)
    idx, _, _, tail = device(name)
    cuts = _cuts(c["k_out"])
    index, count = libntf.fair_infeasible(idx, c["group"], c["p"], cuts)
    assert index.shape == count.shape == (len(idx), len(cuts)) and index.dtype == count.dtype == np.int32
    assert (index[tail == 0] == 0).all() and (count[tail == 0] == 0).all()
    if name in TAIL:                          # and with a group that cannot be served the measure says so
        assert (index[:, -1] > 0).all() and (count >= index).all()


@pytest.mark.parametrize("which", ["original", "det_greedy"])
@pytest.mark.parametrize("name", ["k1", "k63", "k65", "k129", "deep2", "deep64", "prefix", "zero_p", "almost_one", "exhaust"])
def test_infeasible_equals_the_reference(name, which):
    from opentf_amd import libntf
    c = case(name)
    idx = c["idx"] if which == "original" else libntf.fair_rerank(c["idx"], None, c["group"], c["p"], "det_greedy", k_out=c["k_out"])[0]
    cuts = _cuts(idx.shape[1])
    rindex, rcount = S.infeasible(idx.tolist(), c["group"].tolist(), c["p"].tolist(), cuts)
    index, count = libntf.fair_infeasible(idx, c["group"], c["p"], cuts)
    assert np.array_equal(index, np.array(rindex, np.int32)) and np.array_equal(count, np.array(rcount, np.int32))
    if which == "original" and name in ("deep2", "deep64", "k129"):       # block-ordered rows are far from feasible: the equality is not one of zeros
        assert index.max() > 64 and (count >= index).all()
    i_only = libntf.fair_infeasible(idx, c["group"], c["p"], cuts, count=False)
    c_only = libntf.fair_infeasible(idx, c["group"], c["p"], cuts, index=False)
    assert i_only[1] is None and c_only[0] is None and i_only[0].tobytes() == index.tobytes() and c_only[1].tobytes() == count.tobytes()


def test_infeasible_sees_what_detgreedy_misses():
    from opentf_amd import libntf
    groups, p, k_out = GREEDY_MISS
    ids = np.arange(len(groups), dtype=np.int32)[None, :]
    greedy = libntf.fair_rerank(ids, None, groups, p, "det_greedy", k_out=k_out)[0]
    assert [a.tolist() for a in libntf.fair_infeasible(greedy, groups, p, [5, 6])] == [[[0, 1]], [[0, 1]]]
    idx, _, tail = libntf.fair_constsort(ids, None, groups, p, k_out=k_out, want_tail=True)
    assert tail.tolist() == [0] and [a.tolist() for a in libntf.fair_infeasible(idx, groups, p, [5, 6])] == [[[0, 0]], [[0, 0]]]


# --------------------------------------------------------------------------------- refusals
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_every_refusal_leaves_the_outputs_untouched():
    from opentf_amd import libntf
    lib = libntf.lib()
    n, K, G, E = 4, 8, 2, 16
    rng = np.random.default_rng(0)
    good = dict(idx=np.stack([rng.permutation(E)[:K] for _ in range(n)]).astype(np.int32), val=np.zeros((n, K), np.float32), n=n, K=K,
                group=(np.arange(E) % 2).astype(np.uint8), E=E, G=G, p=np.array([[0.5, 0.5]]), n_p=1, k_out=K, cuts=np.array([1, K], np.int32), n_cut=2,
                want_idx=True, want_val=True, want_index=True, want_count=True)

    def constsort(**kw):
        a = {**good, **kw}
        oi, ov, op, ot = np.full((n, K), -7, np.int32), np.full((n, K), -7.0, np.float32), np.full((n, K), -7, np.int32), np.full(n, -7, np.int32)
        rc = lib.ntf_fair_constsort(0, _ptr(a["idx"]), _ptr(a["val"]), a["n"], a["K"], _ptr(a["group"]), a["E"], a["G"], _ptr(a["p"]), a["n_p"], a["k_out"],
                                    _ptr(oi) if a["want_idx"] else None, _ptr(ov) if a["want_val"] else None, _ptr(op), _ptr(ot))
        return rc, bool((oi == -7).all() and (ov == -7.0).all() and (op == -7).all() and (ot == -7).all())

    def infeasible(**kw):
        a = {**good, **kw}
        oi, oc = np.full((n, 2), -7, np.int32), np.full((n, 2), -7, np.int32)
        rc = lib.ntf_fair_infeasible(0, _ptr(a["idx"]), a["n"], a["K"], _ptr(a["group"]), a["E"], a["G"], _ptr(a["p"]), a["n_p"], _ptr(a["cuts"]), a["n_cut"],
                                     _ptr(oi) if a["want_index"] else None, _ptr(oc) if a["want_count"] else None)
        return rc, bool((oi == -7).all() and (oc == -7).all())

    assert constsort()[0] == 0 and infeasible()[0] == 0          # the base call is accepted: each refusal below is owed to its one change
    bad_idx_hi, bad_idx_lo, bad_group = good["idx"].copy(), good["idx"].copy(), good["group"].copy()
    bad_idx_hi[2, 3] = E; bad_idx_lo[0, 0] = -1; bad_group[5] = G
    shared = [dict(idx=None), dict(group=None), dict(p=None), dict(n=0), dict(K=0), dict(K=2049), dict(G=0), dict(G=65), dict(n_p=2), dict(n_p=0),
              dict(idx=bad_idx_hi), dict(idx=bad_idx_lo), dict(group=bad_group),
              dict(p=np.array([[np.nan, 0.5]])), dict(p=np.array([[np.inf, 0.5]])), dict(p=np.array([[-0.1, 1.1]])), dict(p=np.array([[1.5, 0.0]])),
              dict(p=np.array([[0.5, 0.5 + 3e-6]])), dict(p=np.array([[0.5, 0.5 - 3e-6]]))]
    for kw in shared + [dict(k_out=0), dict(k_out=K + 1), dict(want_idx=False), dict(val=None)]:
        assert constsort(**kw) == (EINVAL, True), kw
    for kw in shared + [dict(cuts=None), dict(n_cut=0), dict(n_cut=9), dict(cuts=np.array([0, K], np.int32)), dict(cuts=np.array([1, K + 1], np.int32)),
                        dict(want_index=False, want_count=False)]:
        assert infeasible(**kw) == (EINVAL, True), kw
    assert constsort(p=np.array([[0.5, 0.5 + 5e-7]]))[0] == 0 and infeasible(p=np.array([[0.5, 0.5 - 5e-7]]))[0] == 0      # inside the sanity bound of the sum
    # the existing entry keeps refusing the code after its three
    oi = np.full((n, K), -7, np.int32)
    assert lib.ntf_fair_rerank(0, 3, _ptr(good["idx"]), None, n, K, _ptr(good["group"]), E, G, _ptr(good["p"]), 1, K, _ptr(oi), None, None) == EINVAL and (oi == -7).all()
    with pytest.raises(libntf.NtfError):
        libntf.fair_rerank(good["idx"], None, good["group"], good["p"], "det_const_sort")
    with pytest.raises(libntf.NtfError):
        libntf.fair_infeasible(good["idx"], good["group"], good["p"], [K + 1])


# --------------------------------------------------------------------------------- Ntf.adila end to end
def test_adila_with_det_const_sort_and_the_infeasible_rows(tmp_path):
    import pandas as pd
    from opentf_amd.evl import fair, metric
    from opentf_amd.mdl.fnn import Fnn
    from opentf_amd.mdl.ntf import _read_pred
    tv, splits = _toy("dblp")
    m = Fnn(str(tmp_path), "cuda:0", 0, Cfg(b=8, e=1, ns=2, lr=0.01, es=2, h=[16], spe=0, l="bce", tpw=10, tnw=1, nsd="uniform"))
    m.learn(tv, splits, None)
    m.test(tv, splits, Cfg(per_epoch=False, on_train=False, topK=None))
    # the toy has 13 experts, 5 nonpopular and 8 popular (target 5/13, 8/13): any 10 of them hold at least 2 and 5, which is what the groups are owed up to
    # k = 7 (floor(7 * 5/13) = 2, floor(7 * 8/13) = 4), so whatever the model predicts no group runs out before rank 7 and the re-ranked lists are feasible there
    cuts = (2, 5, 7)
    faircfg = dict(algorithm="det_const_sort", notion="dp", attribute="popularity", k_max=10, cutoffs=list(cuts), infeasible=True)
    m.adila(tv, splits, Cfg(faircfg))
    group, names = fair.popularity_groups(tv["member"])
    p = fair.target_distribution("dp", group, 2)
    assert np.bincount(group).tolist() == [5, 8]
    measures = [f"ndkl_{c}" for c in cuts] + [f"skew_{nm}_{c}" for nm in names for c in cuts]
    for k in range(3):
        stem = f"{m.output}/f{k}.test.pred.det_const_sort.dp.popularity.k10"
        assert all(os.path.exists(stem + s) for s in (".rerank.pred", ".faireval.csv", ".utileval.csv"))
        ranked = metric._ranked_topk(_read_pred(f"{m.output}/f{k}.test.pred"), 10)
        ref_idx, _, _ = S.constsort(ranked.tolist(), group.tolist(), p.tolist(), 10)
        pr = torch.load(stem + ".rerank.pred", map_location="cpu", weights_only=False)
        assert pr["ranked"].dtype == np.int32 and np.array_equal(pr["ranked"], np.array(ref_idx, np.int32))
        fe = pd.read_csv(stem + ".faireval.csv", index_col=0)
        assert list(fe.columns) == ["before", "after"]
        assert list(fe.index) == measures + [f"infeasible_{w}_{c}" for w in ("index", "count") for c in cuts]
        rindex, rcount = S.infeasible(ranked.tolist(), group.tolist(), p.tolist(), cuts)
        assert np.allclose(fe.loc[[f"infeasible_index_{c}" for c in cuts], "before"], np.mean(rindex, axis=0), rtol=1e-12, atol=0)
        assert np.allclose(fe.loc[[f"infeasible_count_{c}" for c in cuts], "before"], np.mean(rcount, axis=0), rtol=1e-12, atol=0)
        assert (fe.loc[[i for i in fe.index if i.startswith("infeasible_")], "after"] == 0.0).all()
    # without the key the table has the rows it always had
    m.adila(tv, splits, Cfg({**faircfg, "infeasible": None}))
    assert list(pd.read_csv(stem + ".faireval.csv", index_col=0).index) == measures
