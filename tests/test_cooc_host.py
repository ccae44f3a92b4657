"""The host side of tests/test_gpu_cooc_paths.py (co-occurrence kernels on the scan, sort and histogram paths): every condition a case of
tests/cooc_cases.py has to meet BEFORE a device sees it - the branch of ntf_cooc.hip it is named for, taken from `profile()` and the kernels'
own constants - and oracle/cooc_oracle.py against the reference's own expression (`Team.gen_skill_coverage`, src/cmn/team.py:327-335, as
tests/golden/make_golden_cooc.py::reference_expression spells it) on every case.  No GPU."""
import copy

import numpy as np
import pytest
import scipy.sparse

import cooc_cases as CC


def _rows(name, skipped=True):
    """row lengths of the oracle's result"""
    return np.diff(CC.expected(name, skipped)[0])


def test_the_cases_are_sized_for_the_constants_the_kernels_are_built_with():
    assert CC.constants() == CC.SIZED_FOR, (f"ntf_cooc.hip is built with {CC.constants()}, tests/cooc_cases.py is sized for {CC.SIZED_FOR}: resize the cases "
                                            "(boundary works, the number of long rows of hist_rounds, the M of scan_wide) and SIZED_FOR with them")


def test_sort_edges_has_both_rows_at_every_boundary_work_and_empty_rows_between_full_ones():
    c, r, K = CC.case("sort_edges"), CC.roles("sort_edges"), CC.constants()
    p, rows = CC.profile(c), _rows("sort_edges")
    ip, ix, data = CC.expected("sort_edges")
    assert c[6] == 2051 and p["hist_rows"] == 0 and p["sort_rows"] == 2 * len(CC.SORT_WORKS)
    assert {K["SORT_MAX"] - 1, K["SORT_MAX"]} <= set(CC.SORT_WORKS) and max(CC.SORT_WORKS) == K["SORT_MAX"]
    for n in (64, 128, 1024): assert {n - 1, n, n + 1} & set(CC.SORT_WORKS) >= {n, n + 1}     # a full padded array and the first work of the next size
    assert {63, 127, 1023} <= set(CC.SORT_WORKS)
    for w in CC.SORT_WORKS:
        d, q = r["distinct"][w], r["repeated"][w]
        assert p["work"][d] == w and p["work"][q] == w
        assert rows[d] == w and (data[ip[d]:ip[d + 1]] == 1).all()                            # w run heads
        assert rows[q] == (w % 256 != 0) and (not rows[q] or data[ip[q]] == w % 256)          # one run of length w
    empty = [r["repeated"][1024], r["repeated"][2048], r["no_team"], r["all_skipped"]]
    assert p["work"][r["repeated"][1024]] == 1024 and p["work"][r["repeated"][2048]] == 2048    # work, and nothing to store
    assert p["work"][r["no_team"]] == 0 and p["work"][r["all_skipped"]] == 0
    assert CC.profile(c, skipped=False)["work"][r["all_skipped"]] > 0
    assert not np.isin(r["no_team"], c[1])
    for m in empty: assert rows[m] == 0 and rows[m - 1] > 0 and rows[m + 1] > 0, m             # compaction steps over it between two rows it copies


@pytest.mark.parametrize("S", [1027, 2051])
def test_hist_edges_has_the_rows_the_histogram_passes_can_get_wrong(S):
    name = f"hist_edges-{S}"
    c, r, K = CC.case(name), CC.roles(name), CC.constants()
    p, rows = CC.profile(c), _rows(name)
    ip, ix, data = CC.expected(name)
    row = lambda k: (ix[ip[r[k]]:ip[r[k] + 1]], data[ip[r[k]]:ip[r[k] + 1]])
    W = K["SORT_MAX"]
    assert c[6] == S and S % 4 and S > 1024                                                    # a bin group straddles S in a later pass
    assert p["work"][r["w2049"]] == W + 1 and p["work"][r["w2050"]] == W + 2 and p["work"][r["several_x"]] > 3 * W
    long_ = [v for k, v in r.items() if k != "short"]
    assert (p["work"][long_] > W).all() and p["hist_rows"] == len(long_) and p["rounds"] == 1
    assert ((p["work"][r["short"]] > 0) & (p["work"][r["short"]] <= W)).all() and p["sort_rows"] == len(r["short"])
    assert min(long_) < min(r["short"]) < max(r["short"]) < max(long_)                         # both row kernels write into the same tmp arrays, interleaved
    assert rows[r["full"]] == S and np.array_equal(row("full")[0], np.arange(S))                # the kept length equals S
    assert rows[r["multiples"]] == 0 and p["work"][r["multiples"]] > W                          # every count a multiple of 256: empty after > 2048 entries
    assert rows[r["multiples"] - 1] > 0 and rows[r["multiples"] + 1] > 0
    assert np.array_equal(row("mixed")[0], [3, 1022, 1024, S - 1]) and np.array_equal(row("mixed")[1], [255, 1, 255, 1])   # 256 and 512 dropped
    assert np.array_equal(row("only_0")[0], [0]) and np.array_equal(row("only_1023_1024")[0], [1023, 1024]) and np.array_equal(row("only_last")[0], [S - 1])
    assert np.array_equal(row("first_and_last")[0], [0, S - 1])                                 # `run` carried over passes that keep nothing
    full_skip = CC.expected(name, False)
    assert np.diff(full_skip[0])[r["multiples"]] > 0                                            # the skipped teams would have shown


def test_hist_rounds_reuses_scratch_rows_and_a_stale_bin_shows_whatever_the_assignment():
    c, r, K = CC.case("hist_rounds"), CC.roles("hist_rounds"), CC.constants()
    p, rows = CC.profile(c), _rows("hist_rounds")
    ip, ix, _ = CC.expected("hist_rounds")
    S = c[6]
    assert S == 1027 and p["hist_rows"] == len(r["long"]) == 1100 and p["rounds"] == 3 and p["hist_rows"] > 2 * K["HIST_WGS"]
    assert (p["work"][r["long"]] > K["SORT_MAX"]).all() and p["sort_rows"] >= 24 and p["total"] < 5_000_000
    sup = np.zeros((len(rows), S), np.float32)
    sup[np.repeat(np.arange(len(rows)), rows), ix] = 1
    sup = sup[r["long"]]
    assert (sup.sum(1) <= S / 4).all()
    missing = sup @ (1 - sup).T                                    # [a, b] = |support(a) \ support(b)|
    np.fill_diagonal(missing, 1)
    assert (missing >= 1).all()                                    # whichever row ran before b on its scratch row, a bin it left set is no bin of b


@pytest.mark.parametrize("M", CC.SCAN_MS)
def test_scan_wide_takes_the_strips_and_has_work_on_both_sides_of_every_edge(M):
    name = f"scan_wide-{M}"
    c, r, K = CC.case(name), CC.roles(name), CC.constants()
    p, rows = CC.profile(c), _rows(name)
    blocks = -(-M // K["SCAN_BLOCK"])
    assert c[5] == M and p["scan_blocks"] == blocks == {262144: 256, 262145: 257, 263169: 258, 600000: 586}[M]
    assert p["strips"] == {262144: 1, 262145: 2, 263169: 2, 600000: 3}[M]
    assert (M % K["SCAN_BLOCK"] != 0) == (M in (262145, 263169, 600000))                       # a partial last block
    want = [m for m in CC.SCAN_FORCED if m < M] + [M - 1]
    assert (p["work"][want] > 0).all() and (rows[want] > 0).all()
    assert 2000 <= p["sort_rows"] <= 5000 and p["sort_rows"] + p["hist_rows"] < M / 50          # most members have no work
    assert (p["work"][r["hist"]] > K["SORT_MAX"]).all() and p["hist_rows"] == len(r["hist"])
    if p["strips"] > 1:                                                                         # a long row behind the first strip's carry
        assert max(r["hist"]) >= CC.TOP_STRIP * K["SCAN_BLOCK"]
        assert (p["work"][:CC.TOP_STRIP * K["SCAN_BLOCK"]] > 0).any() and (rows[CC.TOP_STRIP * K["SCAN_BLOCK"]:] > 0).any()
    if p["strips"] > 2: assert (rows[2 * CC.TOP_STRIP * K["SCAN_BLOCK"]:] > 0).any()


def test_degenerate_cases_are_what_they_are_named_for():
    for d in ("all_skipped", "no_pairs"):
        p = CC.profile(CC.case(f"degenerate-{d}"))
        assert p["total"] == 0 and len(CC.expected(f"degenerate-{d}")[1]) == 0
    assert CC.profile(CC.case("degenerate-all_skipped"), skipped=False)["total"] > 0
    c = CC.case("degenerate-no_pairs")
    assert ((np.diff(c[0]) == 0) | (np.diff(c[2]) == 0)).all() and c[0][-1] > 0 and c[2][-1] > 0
    skip = CC.case("degenerate-skip_repeated")[7]
    assert len(np.unique(skip)) < len(skip)
    for n in (1, 255, 256, 257):
        c = CC.case(f"degenerate-n{n}")
        ip, ix, data = CC.expected(f"degenerate-n{n}")
        assert c[4:7] == (n, 1, 1) and CC.profile(c)["work"][0] == n
        assert (ip[1], data.tolist()) == ((1, [n % 256]) if n % 256 else (0, []))


# ---------------------------------------------------------------- the oracle against the reference's expression
def _lil(indptr, indices, shape):
    return scipy.sparse.csr_matrix((np.ones(len(indices), np.uint8), indices, indptr), shape=shape).tolil()


def reference_expression(member, skill, skipteams):
    """src/cmn/team.py:327-335 on uint8 lil matrices"""
    member, skill = copy.deepcopy(member), copy.deepcopy(skill)
    if skipteams is not None:
        for i in skipteams:
            member.rows[i] = []; member.data[i] = []
            skill.rows[i] = []; skill.data[i] = []
    return scipy.sparse.csr_matrix(np.dot(member.transpose(), skill))


def _same_as(ref, exp, M, S):
    ref.sort_indices()
    assert ref.dtype == np.uint8 and ref.shape == (M, S)
    assert np.array_equal(ref.indptr, exp[0]) and np.array_equal(ref.indices, exp[1]) and np.array_equal(ref.data, exp[2])


@pytest.mark.parametrize("skipped", [True, False])
@pytest.mark.parametrize("name", [n for n in CC.NAMES if n != "scan_wide-600000"])
def test_oracle_is_the_reference_expression_on_every_case(name, skipped):
    m_ip, m_ix, s_ip, s_ix, n, M, S, skip = CC.case(name)
    ref = reference_expression(_lil(m_ip, m_ix, (n, M)), _lil(s_ip, s_ix, (n, S)), skip if skipped else None)
    _same_as(ref, CC.expected(name, skipped), M, S)


@pytest.mark.parametrize("skipped", [True, False])
def test_oracle_is_the_sparse_product_at_600000_members(skipped):
    """the same product on CSR operands in uint8 (`csr.T @ csr`): the lil transpose of 600 000 columns is what takes the time, not the product.  All rows compared."""
    m_ip, m_ix, s_ip, s_ix, n, M, S, skip = CC.case("scan_wide-600000")
    keep = np.ones(n, bool)
    if skipped: keep[skip] = False
    def csr(ip, ix, width):                                                                     # the skipped rows emptied
        ix = ix[np.repeat(keep, np.diff(ip))]
        return scipy.sparse.csr_matrix((np.ones(len(ix), np.uint8), ix, np.concatenate([[0], np.cumsum(np.diff(ip) * keep)])), shape=(n, width))
    member, skill = csr(m_ip, m_ix, M), csr(s_ip, s_ix, S)
    assert member.dtype == skill.dtype == np.uint8
    _same_as(scipy.sparse.csr_matrix(member.T @ skill), CC.expected("scan_wide-600000", skipped), M, S)
