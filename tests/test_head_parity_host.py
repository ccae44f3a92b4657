"""The host side of test_gpu_head_parity.py without a GPU: every case of tests/head_cases.py is what it claims to be, its float64 oracle is
finite and inside the kink caps, and the reference alone - the same oracle evaluated in float32 - clears the bars the device is held to
(loss 2e-5 relative, every gradient 3e-4 of its tensor's maximum outside the kink-flagged units).  A case that missed them here would have to
change; the bars are the suite's."""
import numpy as np
import pytest
import torch

import head_cases as HC
from oracle import ntf_oracle as O
from test_gpu_shapes import _check_grads, _oracle


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


def test_the_cases_are_the_cross_product_and_the_three_extras():
    got = {(c["dims"][0], c["bayesian"], c["input"], c["B"], c["dims"][2]) for c in HC.CASES.values()}
    want = {(D, bay, inp, *HC.SHAPES[D]) for D in (64, 128, 256) for bay in (True, False) for inp in ("meanpool", "dense")}
    want |= {(64, True, "meanpool", 1, 1501), (256, True, "meanpool", 32, 1504), (128, True, "meanpool", 96, 1501)}
    assert got == want and len(HC.CASES) == 15
    assert {c["dims"][2] % 4 for c in HC.CASES.values()} == {0, 1, 2, 3}
    assert all(c["dims"][1] == 128 and (c["ns"], c["tpw"], c["tnw"]) == (5, 10.0, 1.0) for c in HC.CASES.values())


@pytest.mark.parametrize("name", HC.NAMES)
def test_case_reaches_what_it_is_named_for(name):
    c, pb = HC.CASES[name], HC.problem(name)
    (D, _, M), B = c["dims"], c["B"]
    s_ip, s_ix = pb["skill"]
    N = len(s_ip) - 1
    assert N == 2 * B and pb["table"].shape == (HC.S, D) and pb["table"].dtype == np.float32
    # every length of the cycle among the teams, and among the rows of the batch (B = 1: two teams, one row - whichever of the two it is)
    lengths = HC.row_lengths(D)
    assert set(np.diff(s_ip).tolist()) == set(lengths[:N])
    if B >= 6: assert set(pb["nnz"].tolist()) == set(lengths), sorted(set(pb["nnz"].tolist()))
    else: assert set(pb["nnz"].tolist()) <= set(lengths)
    assert np.diff(s_ip).min() >= 1                                       # no empty row: the reference gives NaN there by design
    assert all(np.all(np.diff(s_ix[s_ip[i]: s_ip[i + 1]]) > 0) for i in range(N)) and 0 <= s_ix.min() and s_ix.max() < HC.S
    rows = pb["rows"]
    assert len(rows) == B == len(set(rows.tolist())) and 0 <= rows.min() and rows.max() < N
    if B > 1: assert not np.array_equal(rows, np.arange(B))
    assert np.array_equal(pb["X"].numpy(), pb["Xall"][rows]) and pb["Xall"].shape == (N, D)
    cnt = np.diff(pb["member"][0])
    assert cnt.min() >= 1 and cnt.max() <= M - c["ns"] and np.array_equal(pb["y"].sum(1).numpy(), cnt[rows])
    neg = pb["neg"]
    assert bool((pb["y"][torch.arange(B).unsqueeze(1), neg] == 0).all()) and all(len(set(r.tolist())) == c["ns"] for r in neg)


@pytest.mark.parametrize("name", HC.NAMES)
def test_the_f32_oracle_alone_clears_the_bars_and_the_kink_caps_hold(name):
    c, pb = HC.CASES[name], HC.problem(name)
    orc = _oracle(pb, c["tpw"], c["tnw"])
    assert np.isfinite(orc["loss"]) and np.isfinite(orc["logits"]).all() and all(np.isfinite(g).all() for g in orc["grads"].values())
    hidden, experts = HC.kink_counts(orc["kinks"])
    cap_h, cap_e = HC.kink_caps(c["dims"][2])
    assert hidden <= cap_h and experts <= cap_e, (name, hidden, experts)
    loss32, g32 = O.loss_and_grads(pb["sd"], pb["X"], pb["y"], pb["neg"], c["tpw"], c["tnw"], pb["noise"])
    g32 = {k: v.numpy() for k, v in g32.items()}
    print(name, "kink units", (hidden, experts), {k: f"{v:.2e}" for k, v in HC.worst_errors(loss32, g32, orc).items()})
    assert abs(loss32 - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (name, loss32, orc["loss"])
    _check_grads(g32, orc["grads"], orc["kinks"], name)
