"""Which path every input of tests/test_gpu_long_ranges.py takes through select_topk_row and k_sims, decided on the host from the f64 reference alone
(tests/select_route.py; the margin is 2 E: the device's values and its threshold are each within E of the reference's).  No (query, range) of a designated case may
be "undecided": then the GPU file's preconditions hold on any device whose results are within the tolerance.  No GPU."""
import collections

import numpy as np
import pytest

import long_range_cases as LC
import select_route as SR
from test_knn_host import E
from test_link_host import E as link_E, reference_logits


def test_the_headers_still_state_the_modelled_decisions():
    for name in SR.RULES:
        assert SR.rule_stands(name), name
    assert (SR.SEL_MAX, SR.SEL_SAMPLE) == (2048, 4096) and SR.SEL_MAX <= SR.SEL_SAMPLE
    assert (SR.SIM_KC, SR.SIM_SLD, SR.SIM_WAVES, SR.SIM_RB, SR.SIM_QUNIT, SR.SIM_MAX_GROUP, SR.SIM_MAX_RANGE) == (32, 33, 8, 256, 32, 1024, 262144)
    assert SR.WORKSPACE_BYTES == 256 << 20 and SR.UNIT_BYTES == 32 * 256 * 4
    with pytest.raises(KeyError):
        SR._constants("constexpr int A = 1;", ["B"])
    assert SR._constants("constexpr int A = 8;\nconstexpr int64_t B = A * 32 + 1;", ["A", "B"]) == {"A": 8, "B": 257}


def test_the_model_of_the_decisions_on_small_examples():
    assert not SR.sampled_entered(32767, 10) and SR.sampled_entered(32768, 256) and not SR.sampled_entered(32768, 257) and not SR.sampled_entered(262144, 2048)
    assert SR.sample_columns(40000)[[0, 1, 4095]].tolist() == [0, 9, 36855] and SR.sample_columns(70001)[-1] == 4095 * 17
    assert [SR.sample_rank(M, K) for M, K in ((32768, 256), (70001, 256), (70001, 1), (262144, 10), (40000, 200))] == [145, 68, 8, 8, 93]
    row = -np.arange(40000, dtype=np.float64)                     # descending: the sample's index r is column 9 r, and 9 r values lie above it
    assert SR.threshold(row, 256) == -9.0 * 118 and SR.count_above(row, SR.threshold(row, 256)) == 9 * 118
    assert SR.count_above(row, -1062.0, ex=5) == 1061 and SR.count_above(row, -1062.0, ex=1062) == 1062
    assert SR.route(row, 256) == ("sampled", (1062, 1062)) and SR.route(row, 257)[0] == "radix" and SR.route(row[:30000], 10)[0] == "radix"
    assert SR.route(row, 256, margin=2000.0)[0] == "undecided"    # 0 .. 3062 values above: fewer than K at one end, more than 2048 at the other
    assert SR.route(np.zeros(40000), 5) == ("few", (0, 0))
    up = np.arange(40000, dtype=np.float64); up[SR.sample_columns(40000)] = -1.0
    assert SR.route(up, 5)[0] == "many"
    # a tie group that holds the threshold: its values are never above it, whatever the margin
    tied = np.zeros(40000, bool); tied[100:30000] = True
    flat = np.where(tied, -0.5, np.where(np.arange(40000) < 100, 1.0, -1.0))
    assert SR.route(flat, 50, margin=1e-3)[0] == "undecided" and SR.route(flat, 50, margin=1e-3, tied=tied) == ("sampled", (100, 100))
    assert SR.route(flat, 101, margin=1e-3, tied=tied)[0] == "few"


def test_the_sims_grid_arithmetic():
    assert SR.sims_lds(4, 96) == (128 * 97 + 128 + 8 * 32 * 33) * 4 and [SR.padded(d) for d in (8, 80, 96, 161, 256)] == [32, 96, 96, 192, 256]
    # per_cu = 1 for 4 tiles at dp = 96 and 128 and for 2 tiles from dp = 192; for 1 tile 3 at dp = 160, 2 from dp = 192, 4 at dp = 32
    assert [SR.per_cu(*a) for a in ((4, 96), (4, 128), (2, 192), (2, 256), (1, 160), (1, 256), (1, 32), (2, 160))] == [1, 1, 1, 1, 3, 2, 4, 2]
    assert SR.rows_that_stride(256, 4, 96) == 65537 and SR.rows_that_stride(256, 1, 256) == 131073
    assert SR.grid_width(70001, 256, 4, 96) == 256 and SR.row_blocks(70001) == 274 and SR.strides(70001, 256, 4, 96) and not SR.strides(65536, 256, 4, 96)
    p = SR.SimsPlan(0, 65, 70001, 96)
    assert (p.G, p.Gw, p.R, p.nqt) == (96, 128, 70144, 4) and p.ranges() == [(0, 70001)] and p.groups() == [(0, 65)] and p.launch_nqt(65) == 4
    p = SR.SimsPlan(LC.MERGE_WSB, 65, 70001, 96)
    assert (p.G, p.Gw, p.R, p.nqt) == (32, 32, 32768, 1) and p.ranges() == [(0, 32768), (32768, 32768), (65536, 4465)] and len(p.groups()) == 3
    p = SR.SimsPlan(SR.UNIT_BYTES, 65, 70001, 96)
    assert (p.G, p.R) == (32, 256) and len(p.ranges()) == 274 and not SR.strides(p.R, 256, 1, 96)
    p = SR.SimsPlan(0, 3, LC.CAP_N, 32)
    assert p.ranges() == [(0, SR.SIM_MAX_RANGE), (SR.SIM_MAX_RANGE, 300)] and (p.G, p.nqt) == (32, 1)
    assert SR.SimsPlan(0, 33, 70001, 192).nqt == 2 and SR.SimsPlan(0, 5, 131073, 256).nqt == 1 and SR.SimsPlan(0, 97, 3000, 160).nqt == 2
    # every long case strides on the MI355X's 256 CUs; on a wider device the case grows
    assert LC.long_n(256) == 70001 and LC.long_n(304) == 256 * 304 + 1
    for si, (d, n, lo, Cn, nqt) in enumerate(LC.LINK_SHAPES):
        plan = SR.SimsPlan(0, n, Cn, SR.padded(d))
        assert plan.ranges() == [(0, Cn)] and plan.launch_nqt(n) == nqt and SR.strides(Cn, 256, nqt, SR.padded(d)) and LC.link_c(si, 256) == Cn
        assert SR.strides(LC.link_c(si, 320), 320, nqt, SR.padded(d))


def _tally(routes):
    return dict(collections.Counter(routes.values()))


@pytest.mark.parametrize("kind", ["clustered", "normal"])
def test_long_tables_take_the_sampled_route(kind):
    T, Qv, ref, ex = LC.long_case(kind)
    if kind == "normal": assert 0.45 < (ref < 0).mean() < 0.55          # half of all sims are negative
    margin, dp = 2 * E(LC.LONG_D), SR.padded(LC.LONG_D)
    assert (ex[np.arange(0, 63, 3)] == -1).all() and ex[63] % (LC.LONG_N // SR.SEL_SAMPLE) == 0 and ex[63] // (LC.LONG_N // SR.SEL_SAMPLE) < SR.SEL_SAMPLE
    for K in LC.HOST_TOPN[kind] + (257,):
        for e in (None, ex):
            one = SR.routes_of_call(ref, K, 0, dp, e, margin)
            assert _tally(one) == {("sampled" if K <= 256 else "radix"): LC.LONG_Q}, (K, _tally(one))
            if kind == "clustered":
                three = SR.routes_of_call(ref, K, LC.MERGE_WSB, dp, e, margin)
                want = {"sampled": 2 * LC.LONG_Q, "radix": LC.LONG_Q} if K <= 256 else {"radix": 3 * LC.LONG_Q}
                assert _tally(three) == want and all(r == "radix" for (q, r0), r in three.items() if r0 == 65536), (K, _tally(three))


def test_the_planted_table_merges_two_sampled_ranges_and_a_radix_range():
    T, Qv, ref = LC.merge_case()
    planted = LC.merge_planted()
    assert planted == [0, 32767, 32768, 70000]
    assert (np.sort(np.argsort(-ref, axis=1)[:, :4], axis=1) == planted).all()
    gap = np.sort(ref, axis=1)
    assert ((gap[:, -4] - gap[:, -5]) > 4 * E(LC.LONG_D)).all()          # the four lead by more than the tolerance decides
    for K in (10, 256):
        three = SR.routes_of_call(ref, K, LC.MERGE_WSB, SR.padded(LC.LONG_D), None, 2 * E(LC.LONG_D))
        assert _tally(three) == {"sampled": 2 * LC.LONG_Q, "radix": LC.LONG_Q}, _tally(three)


def test_the_aliasing_table_overflows_and_starves_the_collection():
    T, Qv, ref = LC.aliasing_case()
    for (q, K), want in LC.ALIAS_ROUTES.items():
        got, counts = SR.route(ref[q], K, margin=2 * E(3))
        assert got == want, (q, K, got, counts)
        if want == "many": assert counts[0] > 30000
        else: assert counts[1] <= SR.sample_rank(LC.FALL_M, K) + 1 < K      # only sample columns lie above the sample's own value at index r: r of them


@pytest.mark.parametrize("zero", [False, True])
def test_the_tie_table_puts_the_threshold_and_the_kth_place_inside_the_group(zero):
    T, Qv, ref, pos, tie = LC.tie_case(zero)
    tied = np.zeros(LC.FALL_M, bool); tied[tie] = True
    assert len(set(T[tie].tobytes()[i:i + 12] for i in range(0, 12 * len(tie), 12))) == 1          # one row, so one chain and one f32 sim on the device
    assert (ref[0, pos] > 0.5).all() and (ref[0, ~tied][ref[0, ~tied] < 0.5] < -0.58).all()
    assert (ref[0, tie] == 0).all() if zero else (np.abs(ref[0, tie] - np.cos(2.0)) < 1e-7).all()
    for K, want in LC.TIE_ROUTES.items():
        for ex in (-1, int(tie[2]), int(pos[0])):
            got, counts = SR.route(ref[0], K, ex, margin=2 * E(3), tied=tied)
            assert got == want and counts[0] == counts[1] == LC.TIE_POSITIVE - (ex == pos[0]), (K, ex, got, counts)
        assert SR.route(ref[0], K, margin=2 * E(3))[0] == "undecided"          # without the group's bit equality the margin cannot tell


def test_the_capped_range_is_sampled_and_its_tail_is_not():
    T, Qv, ref = LC.cap_case()
    assert (np.sort(np.argsort(-ref, axis=1)[:, :2], axis=1) == LC.CAP_PLANTED).all()
    routes = SR.routes_of_call(ref, LC.CAP_TOPN, 0, SR.padded(LC.CAP_D), None, 2 * E(LC.CAP_D))
    assert routes == {**{(q, 0): "sampled" for q in range(LC.CAP_Q)}, **{(q, SR.SIM_MAX_RANGE): "radix" for q in range(LC.CAP_Q)}}, routes
    # 1024 row blocks on 4 workgroups a CU: the capped range itself does not stride on 256 CUs (cases 1 and 5 do)
    assert not SR.strides(SR.SIM_MAX_RANGE, 256, 1, 32)


@pytest.mark.parametrize("si", range(len(LC.LINK_SHAPES)))
def test_long_candidate_blocks_take_the_sampled_route(si):
    d, n, lo, Cn, nqt = LC.LINK_SHAPES[si]
    T, rows, ref, tol = LC.link_case(si)
    assert rows[-1] == len(T) - 1 and (ref[-1] + tol[-1] < 0).all()          # the negated mean: every logit of the row is negative, on the device too
    assert (ref.max(axis=1)[:-1] > 0).all()
    for K in LC.LINK_K:
        got = collections.Counter(SR.route(ref[i], K, margin=2 * tol[i].max())[0] for i in range(n))
        print(f"d={d} C={Cn} K={K}: {dict(got)}")
        assert dict(got) == {("sampled" if K <= 256 else "radix"): n}, (K, dict(got))
    if si == 0:          # the pooled form: means of up to 6 table rows
        ptr, items = LC.link_pooled(si)
        Qp = np.stack([T[items[ptr[i]:ptr[i + 1]]].astype(np.float64).mean(axis=0) for i in range(n)])
        cand = T[lo:lo + Cn]
        refp, tolp = reference_logits(cand, Qp), link_E(cand, Qp)
        for K in LC.LINK_K:
            got = {SR.route(refp[i], K, margin=4 * tolp[i].max())[0] for i in range(n)}          # (twice the margin: the device pools in f32)
            assert got == ({"sampled"} if K <= 256 else {"radix"}), (K, got)
