"""The cosine search (ntf_knn) and the link decode (ntf_link) at the sizes real tables have, where three paths of their shared device code run that the small cases of
tests/test_gpu_knn.py and tests/test_gpu_link.py never reach: the sampled-threshold route of select_topk_row on signed values (M >= 32 768, K <= 256; with an excluded
column; its two fallbacks; merged into a running list), the block-stride loop of k_sims (a range of more than 256 * n_cu * per_cu rows) and a range at SIM_MAX_RANGE.

Every case asserts (i) parity with the f64 reference through the checkers and tolerances of those two files, (ii) bit identity of ids and values with the same call
under workspace_bytes = UNIT (256-row ranges: the radix route, no block stride - the route the small cases hold to the reference), which also shows a wrong pick
inside the 2 E band that (i) tolerates, and (iii) the preconditions that make the case mean something, from tests/select_route.py: range count, route, a grid narrower
than the row-block count.  The inputs (tests/long_range_cases.py) are chosen so that the reference alone decides the route (tests/test_select_route_host.py).  The CU
count comes from the device; where it is above 256, the cases grow until a workgroup takes a second row block.

Measured on an MI355X (256 CUs; the stride loop ran in cases 1, 2 and 5: 274 row blocks on 256 workgroups, 513 on 512):
  largest |sim - s*| / E(d): 0.057 on the 70 001-row tables (clustered, d = 96; 0.043 normal; 0.051 planted), 0.075 on the 262 444-row table (d = 8), 0.084 on the
  aliasing table and 0.068 on the tie tables (d = 3) - beside 0.061 over the small cases of tests/test_gpu_knn.py: no growth with N, as the bound says;
  largest |x - x*| / E: 0.147 (d = 80, C = 70 001), 0.112 (d = 161), 0.067 (d = 256, C = 131 073) - beside 0.121 over the small cases of tests/test_gpu_link.py;
  wall time a test, references included: case 1 0.3 - 0.8 s a (table, topn), case 2 0.8 s, case 3 0.1 s each, case 4 0.35 s, case 5 3.1 s (d = 80, both query
  forms), 1.1 s (d = 161), 1.0 s (d = 256); the file 12.6 s.
Three deliberately wrong builds, each caught here: the sampled route's candidates taken whatever their number (no fallback) fails case 3 (aliasing and both tie
tables); ProbKey in k_knn_select fails cases 1 - 4; k_sims without the second trip of its row-block loop fails cases 1, 2 and 5."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import long_range_cases as LC                                                                       # noqa: E402
import select_route as SR                                                                           # noqa: E402
from opentf_amd import libntf                                                                       # noqa: E402
from test_gpu_knn import UNIT, _bits, check_lists                                                   # noqa: E402
from test_gpu_link import check_topk_against_dense, same_bits                                       # noqa: E402
from test_knn_host import E                                                                         # noqa: E402

D, DP, Q = LC.LONG_D, SR.padded(LC.LONG_D), LC.LONG_Q


@functools.lru_cache(maxsize=None)
def n_cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def tables():
    """one resident handle a table, closed when the module is done"""
    made = {}

    def get(name, T):
        if name not in made: made[name] = libntf.Knn(T)
        return made[name]
    yield get
    for k in made.values(): k.close()


def one_striding_range(n, N, dp, nqt):
    """(iii) of the long cases: the default budget takes the N rows as one range and the n queries as one group of nqt-tile workgroups, and the grid of that launch
    is narrower than its row blocks; under UNIT nothing strides"""
    plan = SR.SimsPlan(0, n, N, dp)
    assert plan.ranges() == [(0, N)] and plan.groups() == [(0, n)] and plan.launch_nqt(n) == nqt
    assert SR.strides(N, n_cu(), nqt, dp), (N, n_cu())
    unit = SR.SimsPlan(UNIT, n, N, dp)
    assert unit.R == SR.SIM_RB and not SR.strides(unit.R, n_cu(), unit.nqt, dp)
    return f"{SR.row_blocks(N)} row blocks on {SR.grid_width(N, n_cu(), nqt, dp)} workgroups"


# ------------------------------------------------------------------------------------------------------------------ 1. search, sampled route, one range
@pytest.mark.parametrize("topn", LC.LONG_TOPN)
@pytest.mark.parametrize("kind", ["clustered", "normal"])
def test_search_one_long_range(kind, topn, tables):
    N = LC.long_n(n_cu())
    T, Qv, ref, ex = LC.long_case(kind, N)
    grid = one_striding_range(Q, N, DP, 4)
    want = "sampled" if topn <= 256 else "radix"
    for e in (None, ex):
        assert set(SR.routes_of_call(ref, topn, 0, DP, e, 2 * E(D)).values()) == {want}
    k = tables(kind, T)
    idx, sims = k.query(Qv, topn=topn)
    worst = check_lists(idx, sims, ref, D, topn)
    idx2, sims2 = k.query(Qv, topn=topn, exclude=ex)
    worst = max(worst, check_lists(idx2, sims2, ref, D, topn, ex))
    print(f"\n{kind} N={N} topn={topn} ({want}; {grid}): max |sim - s*| / E(d) = {worst:.3f}")
    none = ex < 0
    assert none.sum() >= Q // 3 - 1 and same((idx2[none], sims2[none]), (idx[none], sims[none]))
    assert ex[63] in SR.sample_columns(N).tolist()          # an excluded row that the sample holds
    assert same(k.query(Qv, topn=topn, workspace_bytes=UNIT), (idx, sims))
    assert same(k.query(Qv, topn=topn, exclude=ex, workspace_bytes=UNIT), (idx2, sims2))


# ------------------------------------------------------------------------------------------------------------------ 2. search, merge of sampled ranges
def test_search_merges_sampled_and_radix_ranges(tables):
    N = LC.long_n(n_cu())
    T, Qv, ref = LC.merge_case(N)
    planted = LC.merge_planted(N)
    plan = SR.SimsPlan(LC.MERGE_WSB, Q, N, DP)
    lens = [rr for _, rr in plan.ranges()]
    assert plan.G == 32 and len(plan.groups()) == 3 and plan.R == 32768 and len(lens) >= 3 and lens[-1] < 32768 and planted[1] + 1 == planted[2] == plan.R
    k = tables("planted", T)
    rng = np.random.default_rng(7)
    ex = rng.integers(-1, N, size=Q); ex[:4] = planted
    for topn in (10, 256):
        routes = SR.routes_of_call(ref, topn, LC.MERGE_WSB, DP, None, 2 * E(D))
        assert all(r == ("sampled" if r0 + plan.R <= N else "radix") for (q, r0), r in routes.items())          # two (or more) sampled ranges and a radix tail
        idx, sims = k.query(Qv, topn=topn)
        worst = check_lists(idx, sims, ref, D, topn)
        print(f"\nplanted N={N} topn={topn}: max |sim - s*| / E(d) = {worst:.3f}")
        assert all(sorted(row[:4].tolist()) == planted for row in idx)               # the top of every list straddles the ranges
        for ws in (LC.MERGE_WSB, UNIT):
            assert same(k.query(Qv, topn=topn, workspace_bytes=ws), (idx, sims)), ws
        e1 = k.query(Qv, topn=topn, exclude=ex)
        check_lists(e1[0], e1[1], ref, D, topn, ex)
        for ws in (LC.MERGE_WSB, UNIT):
            assert same(k.query(Qv, topn=topn, exclude=ex, workspace_bytes=ws), e1), ws
    # the tables of case 1 through the same three-range plan
    for kind in ("clustered", "normal"):
        T1, Q1, _, ex1 = LC.long_case(kind, N)
        k1 = tables(kind, T1)
        assert same(k1.query(Q1, topn=256, exclude=ex1, workspace_bytes=LC.MERGE_WSB), k1.query(Q1, topn=256, exclude=ex1))


# ------------------------------------------------------------------------------------------------------------------ 3. search, the two fallbacks
def test_search_sampled_route_collects_too_many_and_too_few():
    T, Qv, ref = LC.aliasing_case()
    assert SR.SimsPlan(0, 2, LC.FALL_M, 32).ranges() == [(0, LC.FALL_M)]
    k = libntf.Knn(T)
    for K in (1, 50, 256):
        routes = [SR.route(ref[q], K, margin=2 * E(3))[0] for q in range(2)]
        assert routes[0] == "many" and routes[1] == LC.ALIAS_ROUTES.get((1, K), "sampled"), (K, routes)
        idx, sims = k.query(Qv, topn=K)
        worst = check_lists(idx, sims, ref, 3, K)
        print(f"\naliasing K={K} {routes}: max |sim - s*| / E(d) = {worst:.3f}")
        assert (sims[0] > 0).all() and (sims[1, :min(K, 8)] > 0).all()
        assert same(k.query(Qv, topn=K, workspace_bytes=UNIT), (idx, sims))
    k.close()


@pytest.mark.parametrize("zero", [False, True], ids=["negative-ties", "zero-ties"])
def test_search_kth_place_inside_a_tie_group_that_holds_the_threshold(zero):
    T, Qv, ref, pos, tie = LC.tie_case(zero)
    tied = np.zeros(LC.FALL_M, bool); tied[tie] = True
    P = LC.TIE_POSITIVE
    ex = np.asarray([-1, tie[2]], dtype=np.int64)
    k = libntf.Knn(T)
    for K, want in LC.TIE_ROUTES.items():
        assert [SR.route(ref[q], K, int(ex[q]), 2 * E(3), tied)[0] for q in range(2)] == [want, want]
        idx, sims = k.query(Qv, topn=K, exclude=ex)
        worst = check_lists(idx, sims, ref, 3, K, ex)
        print(f"\nties zero={zero} K={K} {want}: max |sim - s*| / E(d) = {worst:.3f}")
        n_pos = min(K, P)
        if K >= P: assert sorted(idx[0, :P].tolist()) == pos.tolist()
        else: assert set(idx[0].tolist()) <= set(pos.tolist())
        assert (sims[:, :n_pos] > 0.5).all() and np.array_equal(idx[1, :n_pos], idx[0, :n_pos])
        if K > P:
            # inside the group the ids ascend and are its lowest; one of them excluded: the list shifts by one
            assert idx[0, P:].tolist() == tie[:K - P].tolist()
            assert idx[1, P:].tolist() == np.delete(tie, 2)[:K - P].tolist()
            group = _bits(sims[:, P:])
            assert len(set(group.reshape(-1).tolist())) == 1 and ((group == 0).all() if zero else (sims[:, P:] < -0.41).all())
        assert same(k.query(Qv, topn=K, exclude=ex, workspace_bytes=UNIT), (idx, sims))
    k.close()


# ------------------------------------------------------------------------------------------------------------------ 4. search, a range at its cap
def test_search_a_range_at_its_cap():
    T, Qv, ref = LC.cap_case()
    N, d, topn = LC.CAP_N, LC.CAP_D, LC.CAP_TOPN
    assert SR.SimsPlan(0, LC.CAP_Q, N, SR.padded(d)).ranges() == [(0, SR.SIM_MAX_RANGE), (SR.SIM_MAX_RANGE, 300)]
    routes = SR.routes_of_call(ref, topn, 0, SR.padded(d), None, 2 * E(d))
    assert all(r == ("sampled" if r0 == 0 else "radix") for (q, r0), r in routes.items())
    k = libntf.Knn(T)
    idx, sims = k.query(Qv, topn=topn)
    worst = check_lists(idx, sims, ref, d, topn)
    print(f"\ncap N={N}: max |sim - s*| / E(d) = {worst:.3f}")
    assert all(sorted(row[:2].tolist()) == LC.CAP_PLANTED for row in idx)              # the last id of the capped range and the first of the next
    assert same(k.query(Qv, topn=topn, workspace_bytes=UNIT), (idx, sims))
    ex = np.asarray(LC.CAP_PLANTED + [-1], dtype=np.int64)
    idx2, sims2 = k.query(Qv, topn=topn, exclude=ex)
    check_lists(idx2, sims2, ref, d, topn, ex)
    assert same(k.query(Qv, topn=topn, exclude=ex, workspace_bytes=UNIT), (idx2, sims2))
    k.close()


# ------------------------------------------------------------------------------------------------------------------ 5. link decode, long candidate blocks
@pytest.mark.parametrize("si", range(len(LC.LINK_SHAPES)), ids=["d%d-n%d-lo%d-C%d-nqt%d" % s for s in LC.LINK_SHAPES])
def test_link_long_candidate_blocks(si):
    d, n, lo, _, nqt = LC.LINK_SHAPES[si]
    Cn = LC.link_c(si, n_cu())
    T, rows, ref, tol = LC.link_case(si, Cn)
    grid = one_striding_range(n, Cn, SR.padded(d), nqt)
    link = libntf.Link(T, lo, lo + Cn)
    dl, dp = link.dense(rows=rows)
    ratio = np.abs(dl.astype(np.float64) - ref) / tol
    print(f"\nd={d} n={n} C={Cn} ({grid}): max |x - x*| / E = {ratio.max():.3f}")
    assert (ratio <= 1.0).all()
    assert (dl[-1] < 0).all() and (dl[:-1].max(axis=1) > 0).all()          # the negated mean of the candidates: a row of negative logits
    assert same(link.dense(rows=rows, workspace_bytes=UNIT), (dl, dp))
    forms = [("rows", dict(rows=rows), dl, dp)]
    if si == 0:
        pooled = LC.link_pooled(si, Cn)
        forms.append(("pooled", dict(pooled=pooled)) + link.dense(pooled=pooled))
    for name, q, xl, xp in forms:
        for K in LC.LINK_K:
            # the device's own logits decide the route exactly; the reference had decided the same (tests/test_select_route_host.py)
            routes = {SR.route(xl[i], K)[0] for i in range(n)}
            assert routes == ({"sampled"} if K <= 256 else {"radix"}), (name, K, routes)
            got = link.topk(K=K, **q)
            check_topk_against_dense(*got, xl, xp, K)
            assert all(same_bits(a, b) for a, b in zip(link.topk(K=K, workspace_bytes=UNIT, **q), got)), (name, K)
    link.close()
