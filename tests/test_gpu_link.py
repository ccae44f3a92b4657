"""Link decode on the MI355X (opentf_amd/csrc/ntf_link.hip, include/opentf_amd_link.h ntf_link_*, libntf.Link, Gnn.test / evaluate / adila / recommend) against
numpy in f64 on the same f32 inputs, x* = t64 . q64, within E(i, j) = (d + 2) * 2^-24 * sum_k |t_jk| |q_ik| a logit, and against f64 1 / (1 + exp(-x)) of the
returned x within (4 * 2^-24 + 2^-40) relative a probability (both derived in tests/test_link_host.py, which also holds the reference and the generators).

Largest |x - x*| / E seen over the parity cases on the device: 0.121 (d = 9, C = 33, one query; 0.06 - 0.09 at d >= 100).  Largest |p - p*| / p* over 98 998 logits in
[-28.9, 29.5]: 2.204 * 2^-24 = 0.551 of the bound (profiles/link_parity.md has the table).
At C = 70 001 and 131 073 (tests/test_gpu_long_ranges.py: the sampled selection route, the block-stride loop of k_sims): 0.147 (d = 80), 0.067 (d = 256)."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest
import scipy.sparse
import torch

pytestmark = pytest.mark.gpu

from n2v_reference import Cfg                                                                                      # noqa: E402
from opentf_amd import libntf                                                                                      # noqa: E402
from test_link_host import (E, P_BOUND, P_RANGE, PARITY_CASES, make_pooled, make_query_rows, make_table,          # noqa: E402
                            plant_tables, rank, reference_logits, sigmoid64)

UNIT = libntf.Link.UNIT_BYTES      # the header's smallest unit of work: 32 queries x 256 rows of f32 logits
NEG_INF = np.float32(-np.inf)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def check_topk_against_dense(idx, logit, prob, dl, dp, K):
    """the exact part of the contract: the ids are the first K of the dense entry's own logits by (value desc, id asc), the values are the dense bits at those ids,
    the slots past the C candidates hold -1 / -inf / 0"""
    n, Cn = dl.shape
    assert idx.shape == logit.shape == prob.shape == (n, K) and idx.dtype == np.int32 and logit.dtype == prob.dtype == np.float32
    k = min(K, Cn)
    want = rank(dl)[:, :k]
    assert np.array_equal(idx[:, :k], want)
    assert same_bits(logit[:, :k], np.take_along_axis(dl, want, axis=1)) and same_bits(prob[:, :k], np.take_along_axis(dp, want, axis=1))
    assert (idx[:, k:] == -1).all() and (logit[:, k:] == NEG_INF).all() and same_bits(prob[:, k:], np.zeros((n, K - k), np.float32))
    assert not np.signbit(dl[dl == 0]).any()


def check_probabilities(x, p):
    """0 <= p <= 1, and p is non-decreasing in x over everything the test scored (so the ranking by x is a valid ranking by p)"""
    x, p = x.reshape(-1), p.reshape(-1)
    o = np.argsort(x, kind="stable")
    assert (p >= 0).all() and (p <= 1).all() and (np.diff(p[o]) >= 0).all()
    same = np.diff(x[o]) == 0
    assert (np.diff(p[o])[same] == 0).all()          # one function: the same x has the same p


@functools.lru_cache(maxsize=None)
def parity_case(ci):
    n_rows, d, lo, Cn, n, K = PARITY_CASES[ci]
    T = make_table(n_rows, d, seed=ci)
    rows = make_query_rows(n_rows, n, seed=ci)
    for a in (T, rows): a.setflags(write=False)
    cand = T[lo:lo + Cn]
    return T, rows, reference_logits(cand, T[rows]), E(cand, T[rows])


@pytest.mark.parametrize("ci", range(len(PARITY_CASES)), ids=["rows%d-d%d-lo%d-C%d-n%d-K%d" % c for c in PARITY_CASES])
def test_logit_parity_and_exact_ranking(ci):
    n_rows, d, lo, Cn, n, K = PARITY_CASES[ci]
    T, rows, ref, tol = parity_case(ci)
    link = libntf.Link(T, lo, lo + Cn)
    assert (link.n_rows, link.d, link.n_cand) == (n_rows, d, Cn)
    dl, dp, ms = link.dense(rows=rows, want_ms=True)
    assert dl.shape == (n, Cn) and dl.dtype == np.float32 and ms > 0
    ratio = np.abs(dl.astype(np.float64) - ref) / tol
    print(f"\nn_rows={n_rows} d={d} lo={lo} C={Cn} n={n}: max |x - x*| / E = {ratio.max():.3f}, dense {ms:.3f} ms")
    assert (ratio <= 1.0).all()
    check_probabilities(dl, dp)
    idx, logit, prob, ms = link.topk(rows=rows, K=K, want_ms=True)
    check_topk_against_dense(idx, logit, prob, dl, dp, K)
    # one output of the dense entry alone has the bits of both
    only_l, none = link.dense(rows=rows, prob=False)
    none2, only_p = link.dense(rows=rows, logit=False)
    assert none is None and none2 is None and same_bits(only_l, dl) and same_bits(only_p, dp)
    link.close(); link.close()
    with pytest.raises(libntf.NtfError, match="closed"):
        link.topk(rows=rows)
    with pytest.raises(libntf.NtfError, match="closed"):
        link.dense(rows=rows)


def test_purity_under_split_permutation_budget_and_query_form():
    """C = 700 under a 32 KiB budget is three ranges (the merge runs); the default budget takes the 97 queries as one group of 4-tile workgroups"""
    n_rows, d, lo, Cn, n, _ = PARITY_CASES[2]
    T, rows, _, _ = parity_case(2)
    link = libntf.Link(T, lo, lo + Cn)
    base = link.topk(rows=rows, K=10)
    dbase = link.dense(rows=rows)
    check_topk_against_dense(*base, *dbase, 10)

    def same(got, want, sel=slice(None)):
        return all(same_bits(g, w[sel]) for g, w in zip(got, want))
    for wsb in (UNIT, 1 << 20, 0):
        assert same(link.topk(rows=rows, K=10, workspace_bytes=wsb), base), wsb
        assert same(link.dense(rows=rows, workspace_bytes=wsb), dbase), wsb
        assert same(link.topk(rows=rows, K=Cn + 5, workspace_bytes=wsb), link.topk(rows=rows, K=Cn + 5)), wsb
    for cut in (1, n // 2):
        for sel in (slice(0, cut), slice(cut, n)):
            assert same(link.topk(rows=rows[sel], K=10), base, sel) and same(link.dense(rows=rows[sel], workspace_bytes=UNIT), dbase, sel)
    perm = np.random.default_rng(0).permutation(n)
    assert same(link.topk(rows=rows[perm], K=10, workspace_bytes=UNIT), base, perm) and same(link.dense(rows=rows[perm]), dbase, perm)
    # the pooled form with one-item rows: the mean of one row is the row
    one = (np.arange(n + 1, dtype=np.int64), rows)
    assert same(link.topk(pooled=one, K=10), base) and same(link.dense(pooled=one, workspace_bytes=UNIT), dbase)
    link.close()


@pytest.mark.parametrize("d", [9, 100, 128])
def test_pooled_queries_are_gather_meanpool_bit_for_bit(d):
    """candidates = the unit vectors e_0 .. e_{d-1}: the chain of (e_k, q) is fmaf(1, q[k], +0) and exact zeros around it, so the dense logits ARE the query vectors"""
    n_rows, n = d + 150, 67
    T = make_table(n_rows, d, seed=d, scale=3.0)
    T[:d] = np.eye(d, dtype=np.float32)
    ptr, items = make_pooled(d, n_rows, n, seed=d, most=9)
    e = libntf.Engine([d, 1, 1], input_mode=libntf.INPUT_MEANPOOL, max_batch=1, ns=0, nsd=None)
    e.set_skill_table(T); e.set_skill_csr((ptr, items.astype(np.int32)))
    want = e.gather_meanpool(n=n) + np.float32(0)          # (-0 is returned as +0)
    e.close()
    link = libntf.Link(T, 0, d)
    got, _ = link.dense(pooled=(ptr, items), prob=False)
    assert same_bits(got, want)
    ref = np.stack([T[items[ptr[i]:ptr[i + 1]]].astype(np.float64).mean(0) for i in range(n)])
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7)
    # the scipy form of the binding, and the top-K entry on pooled queries
    sp = scipy.sparse.csr_matrix((np.ones(len(items), np.uint8), items, ptr), shape=(n, n_rows))
    assert same_bits(link.dense(pooled=sp, prob=False)[0], want)
    idx, logit, prob = link.topk(pooled=(ptr, items), K=7, workspace_bytes=UNIT)
    check_topk_against_dense(idx, logit, prob, *link.dense(pooled=(ptr, items)), 7)
    # an empty row is refused (0 / 0)
    bad = ptr.copy(); bad[5:] -= bad[5] - bad[4]
    with pytest.raises(libntf.NtfError, match="empty pooled row"):
        link.dense(pooled=(bad, items))
    link.close()


def test_signed_values_every_logit_negative():
    """the queries point away from every candidate: a selection that orders raw f32 bit patterns returns the MOST negative first"""
    rng = np.random.default_rng(3)
    d, Cn = 64, 700
    u = rng.standard_normal(d) / 8
    T = np.concatenate([(u[None, :] + 0.05 * rng.standard_normal((Cn, d))), -u[None, :], -3 * u[None, :]]).astype(np.float32)
    link = libntf.Link(T, 0, Cn)
    rows = np.array([Cn, Cn + 1], dtype=np.int64)
    dl, dp = link.dense(rows=rows)
    assert (dl < -0.3).all()
    for K in (1, 10, 300):
        idx, logit, prob = link.topk(rows=rows, K=K, workspace_bytes=UNIT)
        check_topk_against_dense(idx, logit, prob, dl, dp, K)
        assert (logit < 0).all() and same_bits(logit[:, 0], dl.max(axis=1))          # the first result is the least negative
    link.close()


def test_identical_candidates_come_back_in_ascending_id():
    rng = np.random.default_rng(4)
    d, Cn = 100, 600
    T = (rng.standard_normal((Cn + 3, d)) * 0.1).astype(np.float32)
    q = T[Cn]
    for j in (517, 3, 258, 40):          # four bit-identical rows, across two ranges of a 32 KiB budget, that outscore everything
        T[7 + j] = 5 * q
    link = libntf.Link(T, 7, 7 + Cn - 7)
    for wsb in (UNIT, 0):
        idx, logit, prob = link.topk(rows=[Cn], K=6, workspace_bytes=wsb)
        assert idx[0, :4].tolist() == [3, 40, 258, 517] and len(set(_bits(logit[0, :4]).tolist())) == 1 and logit[0, 4] < logit[0, 3]
    link.close()


def test_saturated_logits_keep_the_order_of_the_logits():
    """logits beyond +-20 and +-100: p saturates to 1.0f / underflows towards 0, the lists stay ordered by x"""
    rng = np.random.default_rng(6)
    d, Cn = 128, 257
    T = (rng.standard_normal((Cn + 4, d))).astype(np.float32)
    T[Cn:] *= np.array([[0.3], [3.0], [12.0], [40.0]], np.float32) / np.sqrt(d)
    T[:Cn] *= np.float32(3.0)
    link = libntf.Link(T, 0, Cn)
    rows = np.arange(Cn, Cn + 4, dtype=np.int64)
    dl, dp = link.dense(rows=rows)
    assert np.abs(dl[1]).max() > 20 and dl[3].max() > 100 and dl[3].min() < -100 and np.isfinite(dl).all()
    check_probabilities(dl, dp)
    idx, logit, prob = link.topk(rows=rows, K=Cn)
    check_topk_against_dense(idx, logit, prob, dl, dp, Cn)
    assert (np.diff(logit, axis=1) <= 0).all() and (np.diff(prob, axis=1) <= 0).all() and (prob >= 0).all() and (prob <= 1).all()
    ones = prob[3] == 1.0
    assert ones.sum() > 10 and (np.diff(logit[3][ones]) < 0).any()          # ties in p, still ordered by x
    assert (prob[3][logit[3] < -100] == 0).all()
    link.close()


def test_probability_accuracy_within_the_derived_bound():
    """p against f64 1 / (1 + exp(-x)) of the returned f32 x for |x| <= 30, relative, within the header's bound (4 u + 2^-40, u = 2^-24)"""
    rng = np.random.default_rng(8)
    d, Cn = 100, 3000
    T = rng.standard_normal((Cn + 33, d)).astype(np.float32)
    T[Cn:] *= (np.linspace(0.05, 1.0, 33)[:, None] * 0.9).astype(np.float32)
    link = libntf.Link(T, 0, Cn)
    dl, dp = link.dense(rows=np.arange(Cn, Cn + 33))
    link.close()
    m = np.abs(dl) <= P_RANGE
    assert m.sum() > 50000 and dl[m].min() < -25 and dl[m].max() > 25
    ref = sigmoid64(dl[m])
    ratio = np.abs(dp[m].astype(np.float64) - ref) / ref / P_BOUND
    print(f"\nmax |p - p*| / p* = {ratio.max() * P_BOUND / 2.0 ** -24:.3f} u = {ratio.max():.3f} of the bound, over {int(m.sum())} logits in [{dl[m].min():.1f}, {dl[m].max():.1f}]")
    assert (ratio <= 1.0).all()
    check_probabilities(dl, dp)


def test_refusals_leave_the_outputs_untouched():
    n_rows, d, lo, Cn = 60, 9, 7, 33
    T = make_table(n_rows, d, seed=1)
    L = libntf.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    # create
    for bad in (np.nan, np.inf, -np.inf):
        Tb = T.copy(); Tb[41, 8] = bad
        with pytest.raises(libntf.NtfError, match="not finite"):
            libntf.Link(Tb, lo, lo + Cn)
    for args in ((-1, 5), (0, n_rows + 1), (5, 5), (6, 5)):
        with pytest.raises(libntf.NtfError, match="candidate block"):
            libntf.Link(T, *args)
    with pytest.raises(libntf.NtfError, match="d <= 256"):
        libntf.Link(np.ones((3, 257), np.float32), 0, 3)
    link = libntf.Link(T, lo, lo + Cn)
    rows = np.array([0, 59, 8], dtype=np.int64)
    ptr, items = np.array([0, 2, 3, 6], dtype=np.int64), np.array([1, 50, 59, 0, 3, 4], dtype=np.int64)
    good = link.topk(rows=rows, K=4) + link.dense(pooled=(ptr, items))
    K = 4
    idx = np.full((3, K), -7, np.int32); lg = np.full((3, K), -7, np.float32); pr = np.full((3, K), -7, np.float32)
    dlg = np.full((3, Cn), -7, np.float32); dpr = np.full((3, Cn), -7, np.float32)
    i64 = lambda *v: np.array(v, dtype=np.int64)

    def topk(n=3, q_rows=rows, q_ptr=None, q_items=None, K=K, wsb=0, out_idx=idx):
        return L.ntf_link_topk(link._h, n, p(q_rows), p(q_ptr), p(q_items), K, wsb, p(out_idx), p(lg), p(pr), None)

    def dense(n=3, q_rows=rows, q_ptr=None, q_items=None, wsb=0, outs=(dlg, dpr)):
        return L.ntf_link_dense(link._h, n, p(q_rows), p(q_ptr), p(q_items), wsb, p(outs[0]), p(outs[1]), None)
    refusals = [
        ("out_idx", lambda: topk(out_idx=None)), ("out_logit or out_prob", lambda: dense(outs=(None, None))),
        ("exactly one query form", lambda: topk(q_rows=None)), ("exactly one query form", lambda: dense(q_rows=None)),
        ("exactly one query form", lambda: topk(q_ptr=ptr, q_items=items)), ("exactly one query form", lambda: dense(q_ptr=ptr, q_items=items)),
        ("exactly one query form", lambda: topk(q_ptr=ptr)),
        ("both q_ptr and q_items", lambda: topk(q_rows=None, q_ptr=ptr)), ("both q_ptr and q_items", lambda: dense(q_rows=None, q_items=items)),
        ("n < 1", lambda: topk(n=0)), ("n < 1", lambda: dense(n=-2)),
        ("K outside", lambda: topk(K=0)), ("K outside", lambda: topk(K=2049)),
        ("query row outside", lambda: topk(q_rows=i64(0, -1, 8))), ("query row outside", lambda: dense(q_rows=i64(0, 1, n_rows))),
        ("pooled item outside", lambda: topk(q_rows=None, q_ptr=ptr, q_items=i64(1, 50, n_rows, 0, 3, 4))),
        ("pooled item outside", lambda: dense(q_rows=None, q_ptr=ptr, q_items=i64(1, 50, 59, 0, -1, 4))),
        (r"q_ptr\[0\] != 0", lambda: topk(q_rows=None, q_ptr=i64(1, 2, 3, 6), q_items=items)),
        ("not monotone", lambda: dense(q_rows=None, q_ptr=i64(0, 3, 2, 6), q_items=items)),
        ("empty pooled row", lambda: topk(q_rows=None, q_ptr=i64(0, 2, 2, 6), q_items=items)),
        ("workspace_bytes below", lambda: topk(wsb=UNIT - 1)), ("workspace_bytes below", lambda: dense(wsb=UNIT - 1)),
        ("workspace_bytes < 0", lambda: topk(wsb=-1)), ("workspace_bytes < 0", lambda: dense(wsb=-1)),
    ]
    import re
    for msg, call in refusals:
        assert call() == libntf.NTF_EINVAL, msg
        text = L.ntf_link_last_error(link._h).decode()
        assert re.search(msg, text), (msg, text)
        assert all((a == -7).all() for a in (idx, lg, pr, dlg, dpr)), msg
        # the handle is as good as before
        again = link.topk(rows=rows, K=4) + link.dense(pooled=(ptr, items))
        assert all(same_bits(a, b) for a, b in zip(again, good)), msg
    # a unit-sized budget is accepted
    assert topk(wsb=UNIT) == 0 and dense(wsb=UNIT) == 0
    assert all(same_bits(a, b) for a, b in zip((idx, lg, pr), good[:3]))
    with pytest.raises(libntf.NtfError, match="error -1: link topk: K outside"):
        link.topk(rows=rows, K=0)
    link.close()


# ---------------------------------------------------------------------------------------------------------------- the plugin, on a planted table
def _clustered_toy():
    """4 communities of 10 members, 4 skills and 12 teams each: a team takes 3 members and 2 skills, mostly from its own community; one fold"""
    rng = np.random.default_rng(0)
    Cc, nm, ns, nt = 4, 10, 4, 12
    M, S, N = Cc * nm, Cc * ns, Cc * nt
    member = scipy.sparse.lil_matrix((N, M), dtype=np.uint8); skill = scipy.sparse.lil_matrix((N, S), dtype=np.uint8)
    for t in range(N):
        c = t // nt
        while member[t].nnz < 3:
            cc = c if rng.random() < 0.9 else int(rng.integers(Cc))
            member[t, cc * nm + int(rng.integers(nm))] = 1
        while skill[t].nnz < 2:
            cc = c if rng.random() < 0.9 else int(rng.integers(Cc))
            skill[t, cc * ns + int(rng.integers(ns))] = 1
    teams = np.arange(N)
    splits = {"test": teams[teams % 6 == 0], "folds": {0: {"train": teams[teams % 6 > 1], "valid": teams[teams % 6 == 1]}}}
    return {"skill": skill, "member": member, "loc": None}, splits, N, S, M


def _planted_table(tv, d=64):
    """member j: 2 e_j + noise; a team: the mean of its members' rows + small noise; skills: a skill's row is the mean of the members it works with"""
    member = scipy.sparse.csr_matrix(tv["member"]).astype(np.float64); skill = scipy.sparse.csr_matrix(tv["skill"]).astype(np.float64)

    def make(off, n, name):
        rng = np.random.default_rng(len(name))
        M, S, N = member.shape[1], skill.shape[1], member.shape[0]
        W = rng.standard_normal((n, d)) * 0.3                # (the m2v dummy row stays noise: it is outside every block)
        Em = 2.0 * np.eye(M, d) + 0.05 * rng.standard_normal((M, d))
        Et = np.asarray(member @ Em) / np.asarray(member.sum(1)) + 0.01 * rng.standard_normal((N, d))
        Es = np.asarray(skill.T @ Et) / np.maximum(np.asarray(skill.sum(0)).reshape(-1, 1), 1)
        W[off["member"]:off["member"] + M], W[off["team"]:off["team"] + N], W[off["skill"]:off["skill"] + S] = Em, Et, Es
        return W.astype(np.float32)
    return make


@pytest.mark.parametrize("method", ["n2v", "m2v"])
def test_gnn_as_a_recommender_on_a_planted_table(method, tmp_path):
    from opentf_amd.mdl.ntf import Ntf, _read_pred
    tv, splits, N, S, M = _clustered_toy()
    g, files, off = plant_tables(tmp_path, method, tv, splits, d=64, tables=_planted_table(tv))
    W = files["f0.pt"]
    assert np.array_equal(g.model, W) and W.shape[0] == S + M + N + (method == "m2v")
    m_lo, t_lo = off["member"], off["team"]
    truth = scipy.sparse.csr_matrix(tv["member"])
    link = libntf.Link(W, m_lo, m_lo + M)
    sets = {"test": splits["test"], "train": splits["folds"][0]["train"], "valid": splits["folds"][0]["valid"]}
    # topK = 5: the sparse files, y_pred = what Link returns for those rows (ids and value bits)
    g.test(tv, splits, Cfg(topK=5, per_epoch=False, on_train=True))
    for s, teams in sets.items():
        pr = torch.load(f"{g.output}/f0.{s}.pred", map_location="cpu", weights_only=False)
        assert list(pr.keys()) == ["y_pred", "uncertainty"] and pr["uncertainty"] is None
        y = pr["y_pred"]
        idx, logit, prob = link.topk(rows=teams + t_lo, K=5)
        assert y.is_sparse and y.is_coalesced() and tuple(y.shape) == (len(teams), M) and y._nnz() == 5 * len(teams)
        assert same_bits(np.take_along_axis(y.to_dense().numpy(), idx.astype(np.int64), axis=1), prob)
        for i, t in enumerate(teams):          # a block offset that is off by one type would put anything but the team's members here
            true = truth[t].indices
            assert set(idx[i, :len(true)].tolist()) == set(true.tolist()), (s, t)
    # evaluate() on those files leaves what Ntf.evaluate leaves for the same file in a directory of its own (Fnn's run goes through the same method)
    evalcfg = Cfg(topK=5, per_instance=True, on_train=False, per_epoch=False, metrics=Cfg(trec=["P_2,5", "recall_2,5", "ndcg_cut_2,5", "map_cut_2,5"], other=["aucroc"]))
    before = set(os.listdir(g.output))
    g.evaluate(tv, splits, evalcfg)
    plain = Ntf(str(tmp_path / "plain"), "cuda:0", 0, Cfg(b=1))
    shutil.copy(f"{g.output}/f0.test.pred", f"{plain.output}/f0.test.pred")
    plain.evaluate(tv, splits, evalcfg)
    new = set(os.listdir(g.output)) - before
    assert new == set(os.listdir(plain.output)) - {"f0.test.pred"} and {"f0.test.pred.eval.mean.csv", "f0.test.pred.eval.instance.csv", "test.pred.eval.mean.csv"} <= new
    for f in new:
        assert open(f"{g.output}/{f}", "rb").read() == open(f"{plain.output}/{f}", "rb").read(), f
    import pandas as pd
    mean = pd.read_csv(f"{g.output}/f0.test.pred.eval.mean.csv", index_col=0)
    assert mean.loc["recall_5", "mean"] == 1.0 and mean.loc["P_2", "mean"] == 1.0          # the planted members lead every list
    # topK = None: the dense files
    g.test(tv, splits, Cfg(topK=None, per_epoch=False, on_train=True))
    for s, teams in sets.items():
        y = torch.load(f"{g.output}/f0.{s}.pred", map_location="cpu", weights_only=False)["y_pred"]
        assert not y.is_sparse and same_bits(y.numpy(), link.dense(rows=teams + t_lo, logit=False)[1])
    # adila() runs on the files
    from opentf_amd.evl import fair
    faircfg = Cfg(algorithm="det_cons", notion="dp", attribute="popularity", k_max=10, cutoffs=[2, 5, 10])
    g.adila(tv, splits, faircfg)
    stem = fair.fair_stem(f"{g.output}/f0.test.pred", fair.FairSpec.from_cfg(faircfg))
    assert all(os.path.exists(stem + e) for e in (".rerank.pred", ".faireval.csv", ".utileval.csv"))
    ranked = torch.load(stem + ".rerank.pred", map_location="cpu", weights_only=False)["ranked"]
    assert ranked.shape == (len(splits["test"]), 10) and ((ranked >= 0) & (ranked < M)).all()
    # recommend(): teams that are not in the graph, from their skills alone - the pooled form over the skill block
    sk = scipy.sparse.csr_matrix(tv["skill"])[splits["test"]]
    idx, prob = g.recommend(sk, topn=7)
    assert idx.shape == prob.shape == (len(splits["test"]), 7) and idx.dtype == np.int32 and ((idx >= 0) & (idx < M)).all() and (np.diff(prob, axis=1) <= 0).all()
    idx2, prob2 = g.recommend([sk[i].indices.tolist() for i in range(sk.shape[0])], topn=7)
    want = link.topk(pooled=(sk.indptr.astype(np.int64), sk.indices.astype(np.int64) + off["skill"]), K=7)
    assert np.array_equal(idx, idx2) and same_bits(prob, prob2) and np.array_equal(idx, want[0]) and same_bits(prob, want[2])
    with pytest.raises(ValueError, match="skill id outside"):
        g.recommend([[0, S]])
    g.close(); g.close(); link.close()
    assert _read_pred(f"{g.output}/f0.test.pred").shape == (len(splits["test"]), M)
