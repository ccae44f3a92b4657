"""ntf_infer_mc_plan (include/opentf_amd.h): the ring plan of the fused Monte-Carlo inference arm, a host function that needs no GPU.  Per expert a pass takes
4 h + 4 bytes (two fp16 planes of sigma * eps, the f32 bias operand), a range 4 h bytes once (the two planes of mu)."""
import itertools

import pytest

H = 128
PER_PASS, MU = 4 * H + 4, 4 * H
EXPERTS = [1, 255, 256, 257, 233_629, 5_020_000]
PASSES = [1, 2, 10, 50]


def _bytes(group, rng):
    return group * rng * PER_PASS + rng * MU


def _budgets(passes):
    """tiny: below one pass over one 256-expert range; one range: exactly that many bytes and one byte less / a byte less than two passes;
    a 256-expert range of every pass of a group, to the byte and one short; ample: 64 GiB"""
    from opentf_amd import libntf
    g = min(passes, libntf.NTF_MC_MAX_GROUP)
    return sorted({1, 1000, _bytes(1, 256) - 1, _bytes(1, 256), _bytes(2, 256) - 1, _bytes(g, 256) - 1, _bytes(g, 256), _bytes(g, 256) + 3 * 256 * PER_PASS,
                   _bytes(g, 512) - 1, 1 << 31, 1 << 36})


@pytest.mark.parametrize("experts,passes", list(itertools.product(EXPERTS, PASSES)))
def test_plan_grid(experts, passes):
    from opentf_amd import libntf
    gmax = min(passes, libntf.NTF_MC_MAX_GROUP)
    for budget in _budgets(passes):
        plan = libntf.infer_mc_plan(experts, H, passes, budget)
        fits_one = _bytes(1, 256) <= budget
        assert (plan is None) == (not fits_one), (experts, passes, budget, plan)      # NTF_EINVAL exactly when nothing fits
        if plan is None: continue
        group, rng = plan
        assert 1 <= group <= gmax
        assert rng > 0 and rng % 256 == 0
        assert _bytes(group, rng) <= budget                                            # the bytes formula stays within the budget
        # the ranges tile [0, experts): full ranges of rng experts and a last one that may be short, none empty, none past the layer's padded end
        n = -(-experts // rng)
        bounds = [(k * rng, min(experts, (k + 1) * rng)) for k in range(n)]
        assert bounds[0][0] == 0 and bounds[-1][1] == experts and all(lo < hi for lo, hi in bounds)
        assert all(bounds[k][1] == bounds[k + 1][0] for k in range(n - 1))
        assert rng <= -(-experts // 256) * 256
        # every pass (up to the launch's limit) in one group whenever one 256-expert range of them fits; else the most that fit
        if _bytes(gmax, 256) <= budget: assert group == gmax
        else: assert _bytes(group + 1, 256) > budget
        # and, behind that choice, the longest range
        if rng < -(-experts // 256) * 256: assert _bytes(group, rng + 256) > budget


def test_plan_rejects_non_positive_arguments():
    from opentf_amd import libntf
    ok = (3000, H, 10, 1 << 31)
    assert libntf.infer_mc_plan(*ok) is not None
    for k in range(4):
        for bad in (0, -1):
            args = list(ok); args[k] = bad
            assert libntf.infer_mc_plan(*args) is None, args
    assert libntf.lib().ntf_infer_mc_plan(3000, H, 10, 1 << 31, None, None) == libntf.NTF_EINVAL


def test_default_budget_runs_config_2_as_one_group_over_one_range():
    """2 GiB: config 2's 233 629 experts, ten passes - one launch; the unfiltered dblp matrix (5.02 M experts) stays inside the same 2 GiB"""
    from opentf_amd import libntf
    assert libntf.infer_mc_plan(233_629, H, 10, 2 << 30) == (10, -(-233_629 // 256) * 256)
    group, rng = libntf.infer_mc_plan(5_020_000, H, 10, 2 << 30)
    assert group == 10 and _bytes(group, rng) <= 2 << 30
