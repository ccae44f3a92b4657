"""The host side of test_gpu_loss_edges.py without a GPU: its label generator, the float64 oracle of every case and the caps on the kink
exclusions (which depend on the parameters, inputs, noise, labels and negatives of a case, not on its loss weights)."""
import numpy as np
import pytest
import torch

import test_gpu_loss_edges as E


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


def test_the_edge_rows_are_what_they_claim_to_be():
    """counts of rows 0 to 7, and negatives that name positives exactly where a row has fewer than ns negatives"""
    for name, (dims, B, ns, _, _) in E.CASES.items():
        pb = E._edge_problem(name, False, ns)
        M = dims[-1]
        cnt = pb["y"].sum(1).long().tolist()
        assert cnt[:8] == [0, M - 2, M, 70, 65, 9, 8, M - ns] and 1 <= min(cnt[8:]) and max(cnt[8:]) < 20, (name, cnt[:12])
        assert np.array_equal(np.diff(pb["member"][0]), cnt)
        on_pos = (pb["y"][torch.arange(B).unsqueeze(1), pb["neg"]] != 0).sum(1).tolist()
        assert on_pos[:8] == [0, ns - 2, ns, 0, 0, 0, 0, 0] and not any(on_pos[8:]), (name, on_pos[:12])
        assert all(len(set(r.tolist())) == ns for r in pb["neg"])


@pytest.mark.parametrize("name", list(E.CASES))
@pytest.mark.parametrize("bayesian", [True, False], ids=["bnn", "fnn"])
def test_every_case_builds_its_oracle_inside_the_kink_caps(name, bayesian):
    ns = E.CASES[name][2]
    for k in (ns, 0) if name in E.NO_NEGATIVES else (ns,):
        pb, orc, dz, special = E._edge_case(name, bayesian, k, 3.0, 0.5)
        assert np.isfinite(orc["loss"]) and np.isfinite(dz).all() and dz.shape == special.shape
        assert special[:8].sum() == pb["y"][:8].sum() + (k * 8 - sum((0, k - 2, k, 0, 0, 0, 0, 0)) if k else 0)
