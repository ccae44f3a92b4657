"""The eval-stage kernels (`k_rank_metrics`, `k_skill_coverage`, ntf_metrics.hip) against the float64 metric oracle beyond the toy shapes:
cutoffs above the 64-wide window, long truth / required-skill rows, the `rows` indirection, the limits of the contract, and the Python
mirror at n = 500, M = 20 000.

Ranked id lists go STRAIGHT into the ABI: the oracle (trec_eval) breaks score ties by document name, the device by id, and a list has no ties.

What is asserted
* P, recall, success, skill coverage: an integer count over an integer, divided once in f32 (no fast-math in the build) -> BIT-equal to
  `np.float32(count) / np.float32(denominator)`, the count being the oracle's.
* ndcg_cut_k and map_cut_k are f32 sums; the bound counts roundings, with u = 2^-24 the unit roundoff of f32:
    - a term of a DCG sum is fl(1 / log2f(fl(p + 2))): p + 2 is exact, log2f is taken to be within 3 ulp <= 6 u relative (its value is >= 1, no
      cancellation), the division is correctly rounded, 1 u: 7 u per term.  The 3 ulp are an ASSUMPTION: it is the limit the OpenCL C
      specification sets for single-precision log2 ("Relative error as ULPs"), to which the ROCm device library's math functions are
      written; the HIP math API reference reports 1 ulp for log2f.  Nothing rests on the difference: the terms' 7 u are small beside
      the k u of the summation, and the observed errors are a hundredth of the bound;
    - a sum of at most k non-negative terms has, in ANY order of summation (the device adds a 6-level butterfly per window and the windows in
      sequence; its ideal DCG serially), a relative error of at most (k - 1) u to first order;
    - so each of DCG and IDCG is within (k + 6) u relative; SUM_REL(k) = (k + 8) u leaves 2 u per sum for the second-order terms (below
      1e-4 u for k <= 4096) and the final division.  ndcg = fl(DCG / IDCG) <= 1, so |ndcg - oracle| <= 2 (k + 8) u = NDCG_BOUND(k);
    - a term of the AP sum is fl(seen / (p + 1)), integers below 2^24, one rounding; <= k terms; one division by R: (k + 1) u relative, and
      map_cut <= 1, so |map - oracle| <= (k + 8) u = MAP_BOUND(k) with room to spare.
  The oracle's own float64 error (k 2^-53) is nine orders of magnitude below.
* The largest bound in use (k = 1000: ndcg 1.2e-4, map 6.0e-5) stays at least 4 times under the smallest change that one dropped, doubled
  or misplaced ranked position makes in the hand-placed cases (6.7e-4, see `test_window_edges_hand_placed`), and this relation is asserted.

Largest errors observed on an MI355X are recorded in DESIGN.md (§2, metric kernels); every test prints its own with `-s`.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import metric_oracle as MO

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EINVAL = -1            # NTF_EINVAL, include/opentf_amd.h
FAMS = ("P", "recall", "ndcg_cut", "map_cut", "success")


def SUM_REL(k):
    assert 1 <= k <= 4096      # the range over which the second-order terms fit in the 2 u of slack
    return (k + 8) * U


def NDCG_BOUND(k):
    return 2.0 * SUM_REL(k)


def MAP_BOUND(k):
    return SUM_REL(k)


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _csr(rows_):
    """CSR (int64 indptr, int32 indices) from a list of id arrays, each row sorted"""
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows_])]).astype(np.int64)
    ix = np.concatenate([np.sort(np.asarray(r, dtype=np.int64)) for r in rows_] + [np.empty(0, np.int64)]).astype(np.int32)
    return ip, ix


def _row(ip, ix, i):
    return ix[ip[i]:ip[i + 1]]


def rank_metrics(top, t_ip, t_ix, cuts, rows=None, n=None):
    """-> (status, out [n, 5, n_cut]) of ntf_rank_metrics"""
    from opentf_amd import libntf
    top = np.ascontiguousarray(top, dtype=np.int32)
    n = top.shape[0] if n is None else n
    cu = np.ascontiguousarray(cuts, dtype=np.int32)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    out = np.full((n, 5, len(cu)), -7.0, dtype=np.float32)
    rc = libntf.lib().ntf_rank_metrics(0, _p(top), n, top.shape[1], _p(t_ip), _p(t_ix), len(t_ip) - 1, _p(r), _p(cu), len(cu), _p(out))
    return rc, out


def coverage(top, s_ip, s_ix, c_ip, c_ix, cuts, rows=None, n=None, n_experts=None):
    """-> (status, out [n, n_cut]) of ntf_skill_coverage"""
    from opentf_amd import libntf
    top = np.ascontiguousarray(top, dtype=np.int32)
    n = top.shape[0] if n is None else n
    cu = np.ascontiguousarray(cuts, dtype=np.int32)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    out = np.full((n, len(cu)), -7.0, dtype=np.float32)
    E = len(c_ip) - 1 if n_experts is None else n_experts
    rc = libntf.lib().ntf_skill_coverage(0, _p(top), n, top.shape[1], _p(s_ip), _p(s_ix), len(s_ip) - 1, _p(r), _p(c_ip), _p(c_ix), E, _p(cu), len(cu), _p(out))
    return rc, out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_rank_metrics(out, top, t_ip, t_ix, cuts, label):
    """every value of `out` [n, 5, n_cut] against MO.trec_metrics; -> {family: [max |err| per cutoff]} for ndcg_cut and map_cut"""
    n = out.shape[0]
    err = {"ndcg_cut": np.zeros(len(cuts)), "map_cut": np.zeros(len(cuts))}
    for i in range(n):
        truth = _row(t_ip, t_ix, i)
        d = MO.trec_metrics(top[i], set(int(c) for c in truth), cuts)
        R = len(truth)
        hit = np.isin(top[i], truth)
        for q, k in enumerate(cuts):
            count = int(hit[:k].sum())
            assert d[f"P_{k}"] == count / k and d[f"success_{k}"] == float(count > 0), (label, i, k)      # the count IS the oracle's
            want = (np.float32(count) / np.float32(k), np.float32(count) / np.float32(R) if R else np.float32(0), np.float32(count > 0))
            for f, w in zip((0, 1, 4), want):
                assert _bits(out[i, f, q]) == _bits(w), (label, FAMS[f], k, i, float(out[i, f, q]), float(w))
            for f, name, bound in ((2, "ndcg_cut", NDCG_BOUND(k)), (3, "map_cut", MAP_BOUND(k))):
                e = abs(float(out[i, f, q]) - d[f"{name}_{k}"])
                err[name][q] = max(err[name][q], e)
                assert e <= bound, (label, name, k, i, float(out[i, f, q]), d[f"{name}_{k}"], e, bound)
    for name in err:
        bound = NDCG_BOUND if name == "ndcg_cut" else MAP_BOUND
        print(f"[{label}] {name}: " + ", ".join(f"k={k} max|err| {e:.2e} (bound {bound(k):.2e})" for k, e in zip(cuts, err[name])))
    return err


def check_coverage(out, top, s_ip, s_ix, c_ip, c_ix, cuts, label):
    """every value of `out` [n, n_cut] BIT-equal to f32(count) / f32(required) with the oracle's count"""
    for i in range(out.shape[0]):
        req = _row(s_ip, s_ix, i)
        d = MO.skill_coverage_ranked(top[i], req, c_ip, c_ix, cuts)
        for q, k in enumerate(cuts):
            v = d[f"skill_coverage_{k}"]
            count = int(round(v * len(req)))
            assert count / len(req) == v
            w = np.float32(count) / np.float32(len(req))
            assert _bits(out[i, q]) == _bits(w), (label, k, i, len(req), float(out[i, q]), float(w))


def _planted_ranking(rng, M, K, truth, p_plant):
    """K distinct ids of range(M): a random list free of `truth`, then each truth id with probability p_plant written over a position drawn
    without replacement with weight 1 / (position + 1) - relevant experts turn up early, as in a trained model's ranking"""
    pool = rng.permutation(M)
    ranked = pool[~np.isin(pool, truth)][:K].copy()
    assert len(ranked) == K
    chosen = np.asarray(truth)[rng.random(len(truth)) < p_plant][:K]
    if len(chosen):
        w = 1.0 / (np.arange(K) + 1.0)
        ranked[rng.choice(K, len(chosen), replace=False, p=w / w.sum())] = chosen
    assert len(np.unique(ranked)) == K
    return ranked


# ------------------------------------------------------------------------------------------------------------------ (a) window edges
def test_window_edges_hand_placed():
    """K = 1000 and the eight cutoffs (1, 63, 64, 65, 128, 129, 500, 1000): 16 windows of 64 ranked positions, the relevant ids placed by hand
    on both sides of window edges and of cutoffs.

    Smallest change of a value when ONE hit position is dropped, counted twice or moved across a cutoff, over all the instances here: a hit at
    position p under cutoff k carries 1 / log2(p + 2) / IDCG_k of ndcg_cut_k and at least seen(p) / (p + 1) / R of map_cut_k.  The minimum
    is the all-relevant instance with R = 1500: 1 / 1500 = 6.67e-4 of map_cut; for ndcg_cut it is position 999 of the all-relevant
    instances, 1 / log2(1001) / IDCG_1000 = 0.1003 / 123.09 = 8.15e-4.  Every other instance has R <= 2, where one position is worth >= 1e-3 (R = 1 at rank
    999: map_cut_1000 = 0.001, ndcg_cut_1000 = 0.100).  Both minima are computed below from the inputs, asserted to be these figures and to be >= 4 x the widest bound."""
    K, M = 1000, 6000
    cuts = (1, 63, 64, 65, 128, 129, 500, 1000)
    rng = np.random.default_rng(11)
    tops, truths = [], []

    def add(ranked, truth):
        tops.append(ranked); truths.append(np.asarray(truth, dtype=np.int64))

    def fresh():
        return rng.permutation(M)[:K]

    for r in (0, 62, 63, 64, 127, 128, 499, 500, 999):                       # R = 1
        t = fresh(); add(t, [t[r]])
    for a, b in ((10, 70), (63, 64), (127, 128), (0, 999), (64, 128), (499, 500)):   # one before, one after a window edge / cutoff
        t = fresh(); add(t, [t[a], t[b]])
    t = fresh(); add(t, t)                                                   # every ranked id relevant, R = 1000
    t = fresh(); add(t, np.concatenate([t, np.setdiff1d(np.arange(M), t)[:500]]))      # ... and R = 1500
    t = fresh(); add(t, np.setdiff1d(np.arange(M), t)[:3])                   # no relevant id in the list
    t = fresh(); add(t, [])                                                  # R = 0
    t = fresh(); add(t, t[np.arange(0, K, 2)])                               # every second position, R = 500
    top = np.stack(tops).astype(np.int32)
    t_ip, t_ix = _csr(truths)
    assert sorted(set(np.diff(t_ip).tolist())) == [0, 1, 2, 3, 500, 1000, 1500]

    # the smallest one-position change (f64, on the inputs; see the docstring)
    smallest = {"ndcg_cut": np.inf, "map_cut": np.inf}
    disc = 1.0 / np.log2(np.arange(K) + 2.0)
    for i in range(len(tops)):
        truth = _row(t_ip, t_ix, i); R = len(truth)
        hit = np.isin(top[i], truth)
        seen = np.cumsum(hit)
        for k in cuts:
            pos = np.nonzero(hit[:k])[0]
            if len(pos):
                smallest["ndcg_cut"] = min(smallest["ndcg_cut"], float((disc[pos] / disc[:min(R, k)].sum()).min()))
                smallest["map_cut"] = min(smallest["map_cut"], float((seen[pos] / (pos + 1.0) / R).min()))
    print(f"[hand-placed] smallest one-position change: ndcg_cut {smallest['ndcg_cut']:.3e}, map_cut {smallest['map_cut']:.3e}")
    assert abs(smallest["map_cut"] - 1.0 / 1500.0) < 1e-12 and 8.1e-4 <= smallest["ndcg_cut"] <= 8.2e-4
    assert 4.0 * NDCG_BOUND(max(cuts)) <= smallest["ndcg_cut"] and 4.0 * MAP_BOUND(max(cuts)) <= smallest["map_cut"]

    rc, out = rank_metrics(top, t_ip, t_ix, cuts)
    assert rc == 0
    check_rank_metrics(out, top, t_ip, t_ix, cuts, "hand-placed")
    # spelled out for the carry across the window edge: relevant at ranks 63 and 64 (R = 2) -> map_cut_65 = (1/64 + 2/65) / 2
    i = 10
    assert np.array_equal(np.nonzero(np.isin(top[i], _row(t_ip, t_ix, i)))[0], [63, 64])
    assert abs(float(out[i, 3, cuts.index(65)]) - (1 / 64 + 2 / 65) / 2) <= MAP_BOUND(65)
    assert abs(float(out[i, 3, cuts.index(64)]) - (1 / 64) / 2) <= MAP_BOUND(64) and out[i, 3, cuts.index(63)] == 0.0
    # R = 0 and no relevant id in the list: all five families exactly 0
    assert not out[-2].any() and not out[-3].any()


# ------------------------------------------------------------------------------------------------------------------ (b) random at scale
def test_random_at_scale_trec_cutoffs():
    """n = 2000 instances, M = 20 000 experts, K = 1000 ranked ids, trec_eval's cutoffs; Zipf truth rows plus hand-made long ones (R = 65 ... 1500)"""
    from opentf_amd.synth import zipf_csr
    n, M, K = 2000, 20000, 1000
    cuts = (5, 10, 15, 20, 30, 100, 200, 500)
    rng = np.random.default_rng(21)
    z_ip, z_ix = zipf_csr(n, M, 4.0, 3)
    truths = [_row(z_ip, z_ix, i) for i in range(n)]
    for i, R in ((7, 65), (300, 129), (301, 1001), (1024, 1500), (1999, 1000)):
        truths[i] = rng.choice(M, R, replace=False)
    truths[55] = np.empty(0, np.int64)                                       # and one instance without truth
    t_ip, t_ix = _csr(truths)
    top = np.stack([_planted_ranking(rng, M, K, truths[i], 0.7) for i in range(n)]).astype(np.int32)
    early = sum(bool(np.isin(top[i, :100], truths[i]).any()) for i in range(n))
    assert early >= n // 2, early                                            # a condition on the inputs: the metrics are not mostly zero
    rc, out = rank_metrics(top, t_ip, t_ix, cuts)
    assert rc == 0
    check_rank_metrics(out, top, t_ip, t_ix, cuts, "random n=2000")
    assert (out[:, 3, -1] > 0).sum() >= n // 2 and len(np.unique(out[:, 2, -1])) > n // 4        # map_cut_500 / ndcg_cut_500 really vary


# ------------------------------------------------------------------------------------------------------------------ (c) cutoff above K
@pytest.mark.parametrize("K,cuts", [(50, (10, 50, 100)), (1, (1,)), (1, (1, 5, 64, 65)), (64, (64, 65, 1000)), (65, (1, 64, 65, 66))])
def test_cutoff_longer_than_the_ranked_list(K, cuts):
    """trec_eval divides P_k by k also when the list is shorter; IDCG_k runs to min(R, k) whatever the list holds"""
    n, M = 96, 200
    rng = np.random.default_rng(31 + K)
    truths = [rng.choice(M, int(r), replace=False) for r in rng.integers(0, 80, n)]
    truths[0] = rng.choice(M, 130, replace=False)
    t_ip, t_ix = _csr(truths)
    top = np.stack([_planted_ranking(rng, M, K, truths[i], 0.5) for i in range(n)]).astype(np.int32)
    rc, out = rank_metrics(top, t_ip, t_ix, cuts)
    assert rc == 0
    check_rank_metrics(out, top, t_ip, t_ix, cuts, f"K={K}")
    assert out[:, 0].any()


# ------------------------------------------------------------------------------------------------------------------ (e) skill coverage
def _coverage_world(rng, E, S, n, K):
    """expert skill rows from empty to 400 skills (sorted), required-skill rows of 1, 64, 65, 300, ... entries, random rankings"""
    kind = rng.random(E)
    sizes = np.where(kind < 0.3, 0, np.where(kind < 0.7, rng.integers(1, 6, E), np.where(kind < 0.9, rng.integers(10, 51, E), rng.integers(100, 401, E))))
    sizes[:4] = (0, 400, 1, 0)
    c_ip, c_ix = _csr([rng.choice(S, int(s), replace=False) for s in sizes])
    nreq = rng.integers(1, 131, n)
    nreq[:8] = (1, 64, 65, 300, 63, 128, 129, 2)
    s_ip, s_ix = _csr([rng.choice(S, int(r), replace=False) for r in nreq])
    top = np.stack([rng.permutation(E)[:K] for _ in range(n)]).astype(np.int32)
    return sizes, (c_ip, c_ix), (s_ip, s_ix), top


def test_skill_coverage_long_rows_and_cutoffs():
    E, S, n, K = 3000, 5000, 200, 100
    rng = np.random.default_rng(41)
    sizes, (c_ip, c_ix), (s_ip, s_ix), top = _coverage_world(rng, E, S, n, K)
    assert sizes.min() == 0 and sizes.max() == 400 and (sizes[top[:, :10]] == 0).any() and (sizes[top[:, :10]] >= 100).any()
    for k_list, cuts in ((K, (1, 2, 5, 10, 100)), (10, (2, 5, 10, 100)), (K, (1, 2, 3, 5, 10, 20, 50, 100))):
        t = np.ascontiguousarray(top[:, :k_list])
        rc, out = coverage(t, s_ip, s_ix, c_ip, c_ix, cuts)
        assert rc == 0
        check_coverage(out, t, s_ip, s_ix, c_ip, c_ix, cuts, f"coverage K={k_list}")
        assert 0.0 < out[:, -1].mean() < 0.95 and (np.diff(out, axis=1) >= 0).all()      # neither empty nor saturated; monotone in k
        if k_list == 10:
            assert np.array_equal(out[:, -1], out[:, -2])                                 # a cutoff above K sees the K experts there are


def test_skill_coverage_first_holder_exactly_at_the_cutoff():
    """a required skill whose first holder sits at rank k - 1 counts for cutoff k; at rank k it does not (k = 5, 64, 100; K = 100)"""
    E, S, K = 400, 200, 100
    rng = np.random.default_rng(43)
    special = 199                                               # held by expert 399 only
    cov_rows = [rng.choice(S - 1, int(c), replace=False) for c in rng.integers(0, 4, E)]
    cov_rows[399] = np.array([special, 3, 17])
    c_ip, c_ix = _csr(cov_rows)
    cuts = (1, 4, 5, 6, 64, 65, 100)
    places = (0, 3, 4, 5, 63, 64, 99)
    tops, reqs = [], []
    for r in places:
        t = rng.permutation(E - 1)[:K]; t[r] = 399             # expert 399 at rank r, nowhere else
        tops.append(t); reqs.append(np.array([special]))
    top = np.stack(tops).astype(np.int32)
    s_ip, s_ix = _csr(reqs)
    rc, out = coverage(top, s_ip, s_ix, c_ip, c_ix, cuts)
    assert rc == 0
    for i, r in enumerate(places):
        assert np.array_equal(out[i], [1.0 if r < k else 0.0 for k in cuts]), (r, out[i])
    check_coverage(out, top, s_ip, s_ix, c_ip, c_ix, cuts, "first holder")
    # the same with 100 more required skills before it (two windows of required skills; the special one, the highest id, in the second)
    reqs2 = [np.concatenate([[special], rng.choice(S - 1, 100, replace=False)]) for _ in places]
    s2_ip, s2_ix = _csr(reqs2)
    rc, out2 = coverage(top, s2_ip, s2_ix, c_ip, c_ix, cuts)
    assert rc == 0
    check_coverage(out2, top, s2_ip, s2_ix, c_ip, c_ix, cuts, "first holder among 101")


def test_mirror_skill_coverage_sorts_an_unsorted_cov():
    """`calculate_skill_coverage` with expert skill rows whose indices are deliberately out of order: the kernel's binary search needs them
    sorted, the mirror sorts them"""
    from opentf_amd.evl import metric
    E, S, n, K = 3000, 5000, 200, 100
    rng = np.random.default_rng(47)
    sizes, (c_ip, c_ix), (s_ip, s_ix), top = _coverage_world(rng, E, S, n, K)
    shuffled = c_ix.copy()
    for e in range(E):
        shuffled[c_ip[e]:c_ip[e + 1]] = rng.permutation(c_ix[c_ip[e]:c_ip[e + 1]])
    assert (shuffled != c_ix).mean() > 0.5
    cov = sp.csr_matrix((np.ones(len(shuffled), np.uint8), shuffled, c_ip), shape=(E, S))
    assert not cov.has_sorted_indices
    X = sp.csr_matrix((np.ones(len(s_ix), np.float32), s_ix, s_ip), shape=(n, S))
    Y_ = np.zeros((n, E), np.float32)
    Y_[np.arange(n)[:, None], top] = (1.0 - np.arange(K) / 128.0).astype(np.float32)[None, :]      # distinct, exact in f32, decreasing with rank
    cuts = (1, 2, 5, 10, 100)
    df, mean = metric.calculate_skill_coverage(X, Y_, cov, per_instance=True, topks="1,2,5,10,100")
    assert list(df.columns) == [f"skill_coverage_{k}" for k in cuts]
    check_coverage(df.values.astype(np.float32), top, s_ip, s_ix, c_ip, c_ix, cuts, "mirror, unsorted cov")
    np.testing.assert_allclose(mean["mean"].values, df.values.mean(0), rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------------ (d) rows
def test_rows_indirection_equals_the_host_slice():
    """both entries with `rows`: a permuted, repeating subset of a larger CSR must give what the same call gives on the CSR sliced on the host"""
    N, M, n, K = 700, 3000, 300, 130
    rng = np.random.default_rng(51)
    truths = [rng.choice(M, int(r), replace=False) for r in rng.integers(0, 40, N)]
    truths[5] = rng.choice(M, 200, replace=False)
    t_ip, t_ix = _csr(truths)
    rows = rng.integers(0, N, n); rows[:3] = (5, 699, 0); rows[10:20] = rows[20:30]; rows[40] = 5
    assert len(np.unique(rows)) < n and not np.array_equal(rows, np.sort(rows))
    top = np.stack([_planted_ranking(rng, M, K, truths[r], 0.6) for r in rows]).astype(np.int32)
    cuts = (1, 10, 64, 65, 100, 130)
    rc, got = rank_metrics(top, t_ip, t_ix, cuts, rows=rows)
    sl_ip, sl_ix = _csr([truths[r] for r in rows])
    rc2, want = rank_metrics(top, sl_ip, sl_ix, cuts)
    rc3, ident = rank_metrics(top, t_ip, t_ix, cuts)            # rows = NULL on the big CSR: instance i against row i, a different answer
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert np.array_equal(_bits(got), _bits(want)) and not np.array_equal(_bits(got), _bits(ident))
    check_rank_metrics(got[:60], top[:60], sl_ip, sl_ix, cuts, "rows")

    E, S, Kc = 500, 800, 40
    cov_ip, cov_ix = _csr([rng.choice(S, int(c), replace=False) for c in rng.integers(0, 30, E)])
    reqs = [rng.choice(S, int(r), replace=False) for r in rng.integers(1, 100, N)]
    s_ip, s_ix = _csr(reqs)
    topc = np.stack([rng.permutation(E)[:Kc] for _ in range(n)]).astype(np.int32)
    ccuts = (1, 2, 5, 10, 40)
    rc, got = coverage(topc, s_ip, s_ix, cov_ip, cov_ix, ccuts, rows=rows)
    sl = _csr([reqs[r] for r in rows])
    rc2, want = coverage(topc, sl[0], sl[1], cov_ip, cov_ix, ccuts)
    rc3, ident = coverage(topc, s_ip, s_ix, cov_ip, cov_ix, ccuts)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert np.array_equal(_bits(got), _bits(want)) and not np.array_equal(_bits(got), _bits(ident))
    check_coverage(got, topc, sl[0], sl[1], cov_ip, cov_ix, ccuts, "rows")


# ------------------------------------------------------------------------------------------------------------------ (f) the mirror at size
def _check_table(df_trec, df_cov, cols, table, cuts, label):
    """mirror DataFrames against MO.instance_table.  A quotient of two integers below 2^24 rounded to f64 and then to f32 equals the
    correctly rounded f32 quotient (double rounding is innocuous for division when the wide format has >= 2 p + 2 = 50 bits), so the
    counting families are compared bit for bit through np.float32(oracle)."""
    got = np.concatenate([df_trec.values, df_cov.values], axis=1)
    assert list(df_trec.columns) + list(df_cov.columns) == cols
    for j, c in enumerate(cols):
        fam, k = c.rsplit("_", 1); k = int(k)
        if fam in ("ndcg_cut", "map_cut"):
            bound = NDCG_BOUND(k) if fam == "ndcg_cut" else MAP_BOUND(k)
            e = float(np.abs(got[:, j] - table[:, j]).max())
            print(f"[{label}] {c}: max|err| {e:.2e} (bound {bound:.2e})")
            assert e <= bound, (label, c, e, bound)
        else:
            assert np.array_equal(_bits(got[:, j]), _bits(table[:, j].astype(np.float32))), (label, c)
        assert table[:, j].any(), (label, c)                    # no column of the comparison is trivially zero


def test_mirror_at_size_dense_and_sparse_predictions():
    """`calculate_metrics` and `calculate_skill_coverage` on a dense f32 prediction matrix with distinct scores (n = 500, M = 20 000) and on a
    sparse top-100 form of it in which some rows store fewer than 100 entries (0, 1, 5, 99), against `MO.instance_table`"""
    from opentf_amd.evl import metric
    from opentf_amd.synth import zipf_csr
    n, M, S = 500, 20000, 2000
    cuts = (2, 10, 100)
    rng = np.random.default_rng(61)
    t_ip, t_ix = zipf_csr(n, M, 4.0, 5)
    x_ip, x_ix = zipf_csr(n, S, 6.0, 6)
    c_ip, c_ix = zipf_csr(M, S, 3.0, 7)
    row_of = np.repeat(np.arange(M), np.diff(c_ip))
    keep = (rng.random(M) > 0.2)[row_of]                                     # a fifth of the experts hold no skill
    c_ix = c_ix[keep]; c_ip = np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=M))]).astype(np.int64)
    assert (np.diff(c_ip) == 0).sum() > M // 10 and np.diff(x_ip).min() >= 1
    # scores: a grid of M distinct f32 values handed out along a full ranking that has the relevant experts early
    grid = ((np.arange(M, dtype=np.float64) + 1.0) / (M + 1.0)).astype(np.float32)
    assert len(np.unique(grid)) == M
    Y_ = np.empty((n, M), np.float32)
    w = 1.0 / (np.arange(200) + 1.0)
    for i in range(n):
        order = rng.permutation(M)
        truth = _row(t_ip, t_ix, i)
        if i % 5:                                                            # four rows in five: the relevant experts somewhere in the first 200 ranks
            early = np.zeros(M, bool); early[rng.choice(200, len(truth), replace=False, p=w / w.sum())] = True
            rest = order[~np.isin(order, truth)]
            order[early] = rng.permutation(truth); order[~early] = rest
        Y_[i, order] = grid[::-1]
    assert all(len(np.unique(Y_[i])) == M for i in (0, 1, n - 1))
    Y = sp.csr_matrix((np.ones(len(t_ix), np.float32), t_ix, t_ip), shape=(n, M))
    X = sp.csr_matrix((np.ones(len(x_ix), np.float32), x_ix, x_ip), shape=(n, S))
    cov = sp.csr_matrix((np.ones(len(c_ix), np.uint8), c_ix, c_ip), shape=(M, S))
    names = [f"{f}_2,10,100" for f in FAMS]

    df, mean = metric.calculate_metrics(Y, Y_, 128, True, names)
    dfc, meanc = metric.calculate_skill_coverage(X, Y_, cov, True, topks="2,10,100")
    cols, table = MO.instance_table(Y_.astype(np.float64), t_ip, t_ix, x_ip, x_ix, c_ip, c_ix, cutoffs=cuts, topK=128)
    _check_table(df, dfc, cols, table, cuts, "mirror dense")
    np.testing.assert_allclose(mean["mean"].values, df.values.mean(0), rtol=1e-12)
    assert list(mean.index) == cols[:15]
    assert (table[:, cols.index("P_100")] > 0).mean() > 0.5

    # sparse top-100 form; rows 0..39 store fewer than 100 entries
    stored = np.full(n, 100); stored[:40] = np.tile((0, 1, 5, 99), 10)
    top100 = np.argsort(-Y_, axis=1, kind="stable")[:, :100]
    r = np.repeat(np.arange(n), stored)
    c = np.concatenate([top100[i, :stored[i]] for i in range(n)])
    Ysp = sp.csr_matrix((Y_[r, c], (r, c)), shape=(n, M))
    assert np.array_equal(np.diff(Ysp.indptr), stored)
    df, mean = metric.calculate_metrics(Y, Ysp, 100, True, names)
    dfc, meanc = metric.calculate_skill_coverage(X, Ysp, cov, True, topks="2,10,100")
    cols, table = MO.instance_table(MO.tiebreak_free_dense(Ysp), t_ip, t_ix, x_ip, x_ix, c_ip, c_ix, cutoffs=cuts, topK=100)
    _check_table(df, dfc, cols, table, cuts, "mirror sparse")


# ------------------------------------------------------------------------------------------------------------------ (g) contract
def _small_world():
    rng = np.random.default_rng(71)
    E, S, n, K = 40, 30, 6, 10
    t_ip, t_ix = _csr([rng.choice(E, 3, replace=False) for _ in range(n)])
    s_ip, s_ix = _csr([rng.choice(S, 4, replace=False) for _ in range(n)])
    c_ip, c_ix = _csr([rng.choice(S, int(c), replace=False) for c in rng.integers(0, 6, E)])
    top = np.stack([rng.permutation(E)[:K] for _ in range(n)]).astype(np.int32)
    return E, S, n, K, (t_ip, t_ix), (s_ip, s_ix), (c_ip, c_ix), top


def test_contract_violations_are_refused():
    from opentf_amd.evl import metric
    from opentf_amd.libntf import NtfError
    E, S, n, K, (t_ip, t_ix), (s_ip, s_ix), (c_ip, c_ix), top = _small_world()
    ok = (1, 2, 3, 4, 5, 6, 7, 8)
    assert rank_metrics(top, t_ip, t_ix, ok)[0] == 0 and coverage(top, s_ip, s_ix, c_ip, c_ix, ok)[0] == 0       # eight cutoffs: the limit itself
    # nine cutoffs; a cutoff of 0
    for bad in (ok + (9,), (2, 0, 5), (0,), (-1, 2)):
        assert rank_metrics(top, t_ip, t_ix, bad)[0] == EINVAL, bad
        assert coverage(top, s_ip, s_ix, c_ip, c_ix, bad)[0] == EINVAL, bad
    # a rows entry out of range
    for bad_rows in ([0, 1, 2, 3, 4, n], [0, -1, 2, 3, 4, 5]):
        assert rank_metrics(top, t_ip, t_ix, (2, 5), rows=bad_rows)[0] == EINVAL
        assert coverage(top, s_ip, s_ix, c_ip, c_ix, (2, 5), rows=bad_rows)[0] == EINVAL
    assert rank_metrics(top, t_ip, t_ix, (2, 5), rows=[5, 5, 0, 1, 5, 0])[0] == 0
    # a ranked id >= n_experts, for coverage (it indexes the experts' CSR)
    worse = top.copy(); worse[3, 7] = E
    assert coverage(worse, s_ip, s_ix, c_ip, c_ix, (2, 5))[0] == EINVAL
    worse[3, 7] = -1
    assert coverage(worse, s_ip, s_ix, c_ip, c_ix, (2, 5))[0] == EINVAL
    assert coverage(top, s_ip, s_ix, c_ip, c_ix, (2, 5), n_experts=int(top.max()))[0] == EINVAL
    # more instances than CSR rows without `rows`
    assert rank_metrics(top, t_ip[:n], t_ix, (2, 5))[0] == EINVAL
    assert coverage(top, s_ip[:n], s_ix, c_ip, c_ix, (2, 5))[0] == EINVAL
    assert rank_metrics(top, t_ip[:n], t_ix, (2, 5), rows=[0, 1, 2, 3, 4, 4])[0] == 0

    # the mirror raises - for the cutoffs.  The other three violations cannot be reached through it: both mirror functions pass
    # rows = NULL with n = the CSR's row count, and calculate_skill_coverage takes its ranked ids from _ranked_topk alone, which yields
    # columns of the prediction matrix, all below n_experts.
    Y = sp.csr_matrix((np.ones(len(t_ix)), t_ix, t_ip), shape=(n, E))
    X = sp.csr_matrix((np.ones(len(s_ix)), s_ix, s_ip), shape=(n, S))
    cov = sp.csr_matrix((np.ones(len(c_ix)), c_ix, c_ip), shape=(E, S))
    Y_ = np.zeros((n, E), np.float32); Y_[np.arange(n)[:, None], top] = (1.0 - np.arange(K) / 16.0).astype(np.float32)
    assert metric.calculate_metrics(Y, Y_, None, True, ["P_1,2,3,4,5,6,7,8"])[0].shape == (n, 8)
    for names in (["P_1,2,3,4,5,6,7,8,9"], ["P_2,5", "ndcg_cut_0,5"], ["P_1,2,3,4,5", "recall_6,7,8,9"]):
        with pytest.raises(NtfError, match="ntf_rank_metrics"):
            metric.calculate_metrics(Y, Y_, None, True, names)
        with pytest.raises(NtfError, match="ntf_rank_metrics"):
            metric.calculate_metrics(Y, None, None, True, names, ranked=top)
    for topks in ("1,2,3,4,5,6,7,8,9", "0,2"):
        with pytest.raises(NtfError, match="ntf_skill_coverage"):
            metric.calculate_skill_coverage(X, Y_, cov, True, topks=topks)


def test_an_instance_without_a_required_skill_is_refused_not_nan():
    """0 / 0: the reference raises ZeroDivisionError; the kernel used to write NaN into the table and the mean turned NaN without an error"""
    from opentf_amd.evl import metric
    from opentf_amd.libntf import NtfError
    E, S, n, K, _, (s_ip, s_ix), (c_ip, c_ix), top = _small_world()
    reqs = [_row(s_ip, s_ix, i) for i in range(n)]
    reqs[3] = np.empty(0, np.int64)
    e_ip, e_ix = _csr(reqs)
    assert coverage(top, e_ip, e_ix, c_ip, c_ix, (2, 5))[0] == EINVAL                                   # without rows
    assert coverage(top, e_ip, e_ix, c_ip, c_ix, (2, 5), rows=[0, 1, 2, 3, 4, 5])[0] == EINVAL          # with rows that select it
    assert coverage(top[:3], e_ip, e_ix, c_ip, c_ix, (2, 5))[0] == 0                                    # the first three instances: row 3 not among them
    rc, out = coverage(top, e_ip, e_ix, c_ip, c_ix, (2, 5), rows=[0, 1, 2, 4, 5, 0])                    # rows that avoid it
    assert rc == 0 and np.isfinite(out).all()
    sl = _csr([reqs[r] for r in (0, 1, 2, 4, 5, 0)])
    check_coverage(out, top, sl[0], sl[1], c_ip, c_ix, (2, 5), "rows around an empty row")
    with pytest.raises(ZeroDivisionError):
        MO.skill_coverage_ranked(top[3], reqs[3], c_ip, c_ix, (2, 5))
    X = sp.csr_matrix((np.ones(len(e_ix)), e_ix, e_ip), shape=(n, S))
    cov = sp.csr_matrix((np.ones(len(c_ix)), c_ix, c_ip), shape=(E, S))
    Y_ = np.zeros((n, E), np.float32); Y_[np.arange(n)[:, None], top] = (1.0 - np.arange(K) / 16.0).astype(np.float32)
    with pytest.raises(NtfError, match="instance 3"):
        metric.calculate_skill_coverage(X, Y_, cov, True, topks="2,5")
    df, mean = metric.calculate_skill_coverage(X[[0, 1, 2, 4, 5]], Y_[[0, 1, 2, 4, 5]], cov, True, topks="2,5")
    assert np.isfinite(df.values).all() and np.isfinite(mean.values).all()
