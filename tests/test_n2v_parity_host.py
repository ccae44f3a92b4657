"""The host side of test_gpu_n2v_parity.py without a GPU: the replay of the device's draws, the float64 reference against torch autograd, the proof that
its bars admit a correct f32 implementation (torch f32 autograd of the oracle's loss), and every condition the GPU tests put on their inputs."""
import numpy as np
import pytest
import torch

import test_gpu_n2v_parity as P
from n2v_reference import global_generators_left_as_found      # the fixture: autouse
from oracle import n2v_oracle as N


def _autograd(W, pos, neg, dtype):
    w = torch.from_numpy(np.array(W)).to(dtype).requires_grad_(True)
    l = N.loss(w, torch.from_numpy(np.array(pos)), torch.from_numpy(np.array(neg))) if len(pos) and len(neg) else None
    if l is None:      # N.loss means over an empty set otherwise (nan): one side alone
        rw = torch.from_numpy(np.array(pos if len(pos) else neg))
        out = (w[rw[:, :1]] * w[rw[:, 1:]]).sum(-1).view(-1)
        l = -torch.log(torch.sigmoid(out) + N.EPS).mean() if len(pos) else -torch.log(1 - torch.sigmoid(out) + N.EPS).mean()
    l.backward()
    return float(l.detach()), w.grad.numpy()


def test_the_graph_has_the_rows_the_cases_need():
    rp, col, nn, sp = P.graph()
    assert nn == 555 and len(rp) == nn + 1 and rp[-1] == len(col) and (np.diff(rp) >= 0).all() and col.min() >= 0 and col.max() < nn
    assert col[rp[sp["loop"]]] == sp["loop"] and col[rp[sp["leaf"]]] == 0 and sp["leaf"] in col[rp[0]:rp[1]]
    for B in (12, 33, 64, 97):
        b = P.start_nodes(B, B)
        assert len(set(b.tolist())) == B and set(sp["isolated"] + [sp["loop"], sp["leaf"], sp["hub"]]) <= set(b.tolist())
    pos, neg = P.injected_case()
    assert len(pos) == 1746 and len(neg) == 3492 and len(pos) % 4 and (len(pos) + len(neg)) < 6500
    # a start node inside its own window, in both launches; a hub row that takes hundreds of adds
    assert (pos[:, 1:] == pos[:, :1]).any(1).sum() > 100 and (neg[:, 1:] == neg[:, :1]).any(1).sum() >= 10
    assert P.ref_batch(P.table(9), pos, neg)["K"].max() > 150


@pytest.mark.parametrize("t", range(len(P.NATIVE_STEPS)))
def test_the_replay_is_a_walk_on_the_graph(t):
    rp, col, nn, _ = P.graph()
    B, wl, ctx, wpn, nneg = P.NATIVE_STEPS[t]
    batch, rw, pos, neg = P.replay_step(t)
    assert rw.shape == (B * wpn, wl) and np.array_equal(rw[:, 0], np.tile(batch, wpn))
    A = np.zeros((nn, nn), dtype=bool); A[np.repeat(np.arange(nn), np.diff(rp)), col] = True
    a, b = rw[:, :-1].ravel(), rw[:, 1:].ravel()
    assert (A[a, b] | ((a == b) & (np.diff(rp)[a] == 0))).all()              # every step is an edge, or a stay on a node of degree 0
    nw = wl + 1 - ctx
    assert np.array_equal(pos, N.windows(torch.from_numpy(rw), ctx).numpy()) and pos.shape == (B * wpn * nw, ctx)
    for j in range(nw):                                                       # row j * n_walks + r = rw[r, j : j + ctx]
        assert np.array_equal(pos[j * B * wpn:(j + 1) * B * wpn], rw[:, j:j + ctx])
    nr = P.replay_negs(batch, B * wpn * nneg, wl, nn, P.NATIVE_SEED, t)
    assert nr.shape == (B * wpn * nneg, wl) and (nr >= 0).all() and (nr < nn).all()
    assert np.array_equal(nr[:, 0], np.tile(batch, wpn * nneg))              # batch[r % B]
    assert np.array_equal(neg, N.windows(torch.from_numpy(nr), ctx).numpy()) if nneg else len(neg) == 0
    if nneg: assert len(np.unique(nr[:, 1:])) > 0.5 * min(nn, nr[:, 1:].size)   # draws, not a constant
    # a walk's first five nodes come from Philox block 0 alone, whatever its length: a longer walk extends a shorter one
    assert np.array_equal(P.replay_walks(rp, col, batch, B * wpn, min(wl, 5), P.NATIVE_SEED, t), rw[:, :5])


def test_the_key_mix_is_taken_modulo_2_64():
    assert P.n2v_key(11, 0, 0) != P.n2v_key(11, 0, 1) != P.n2v_key(11, 1, 0)
    for seed, step, tensor in ((11, 2, 1), (2 ** 64 - 1, 2 ** 40, 1)):
        k0, k1 = P.n2v_key(seed, step, tensor)
        with np.errstate(over="ignore"):      # uint64 arithmetic wraps, as the device's does
            x = np.uint64(seed) ^ (np.uint64(step) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(tensor) * np.uint64(0xBF58476D1CE4E5B9))
            x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9); x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB); x ^= x >> np.uint64(31)
        assert (k0, k1) == (int(x) & 0xFFFFFFFF, int(x) >> 32)


def test_ref_pairs_is_the_oracles_loss_in_float64():
    for d in (1, 9, 129):
        W = P.table(d)
        cases = [P.injected_case(), *P.single_row_cases(), P.replay_step(2)[2:]]
        for pos, neg in cases:
            ref = P.ref_batch(W, pos, neg)
            loss, g = _autograd(W, pos, neg, torch.float64)
            assert abs(ref["loss"] - loss) <= 1e-12 * abs(loss)
            assert np.abs(ref["grad"] - g).max() <= 1e-12 * np.abs(g).max()
            assert ref["K"].sum() == 2 * (len(pos) + len(neg)) * (pos.shape[1] - 1) and (ref["bar"][ref["K"] == 0] == 0).all()


@pytest.mark.parametrize("d", P.SIZES)
def test_the_bars_admit_a_correct_f32_implementation(d):
    """torch f32 autograd of the oracle's loss - other roundings in another order than the kernel's, the same number format - inside the bars of every
    case the GPU tests run on injected windows; the dot conditions hold on all of them"""
    W = P.table(d)
    worst = 0.0
    cases = [P.injected_case(), *P.single_row_cases(), P.sampled_windows(97, 9, 4, 3, 2, 1)] + [P.replay_step(t)[2:] for t in range(3) if d in P.NATIVE_SIZES]
    if d == P.CONTRACT_D: cases += list(P.contract_case()[2:])
    for pos, neg in cases:
        ref = P.ref_batch(W, pos, neg)
        assert P.conditions_hold(ref)
        loss, g = _autograd(W, pos, neg, torch.float32)
        err = np.abs(g.astype(np.float64) - ref["grad"])
        assert abs(loss - ref["loss"]) <= ref["loss_bar"], (loss, ref["loss"], ref["loss_bar"])
        assert (err <= ref["bar"]).all() and not g[ref["K"] == 0].any()
        worst = max(worst, float(np.divide(err, ref["bar"], out=np.zeros_like(err), where=ref["bar"] > 0).max()))
    print(f"n2v bars d={d}: torch f32 autograd reaches {worst:.3f} of the gradient bar at most")


@pytest.mark.parametrize("d", P.ADAM_SIZES)
def test_the_adam_case_stays_under_its_cap(d):
    W, refs, compare, named = P.adam_reference(P.table(d), P.adam_window_sets())
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs)
    assert (~named).sum() >= 5 and all(((r["K"] > 0) != named).any() for r in refs)
    assert P.conditions_hold(P.ref_batch(W, *P.sampled_windows(97, 9, 4, 3, 2, 1)))
    # against torch.optim.Adam in float64 on the oracle's loss
    emb = torch.nn.Parameter(torch.from_numpy(P.table(d)).double()); opt = torch.optim.Adam([emb], lr=0.01)
    for pos, neg in P.adam_window_sets():
        opt.zero_grad(); N.loss(emb, torch.from_numpy(np.array(pos)), torch.from_numpy(np.array(neg))).backward(); opt.step()
    assert np.abs(emb.detach().numpy() - W).max() <= 1e-9


def test_the_corner_cases_meet_their_conditions():
    batch, (wl, ctx, wpn), pos, neg = P.corner_cases()
    rp, col, nn, sp = P.graph()
    assert len(batch) == len(set(batch.tolist())) == 3 and batch[0] == sp["hub"] and pos.shape == (len(batch) * wpn * (wl + 1 - ctx), ctx) and neg.shape == (2, 4)
    W = P.table(P.CORNER_D)
    assert P.conditions_hold(P.ref_batch(W, pos, np.zeros((0, ctx), np.int64))) and P.conditions_hold(P.ref_batch(W, neg[:0], neg))


def test_the_saturation_table_keeps_clear_of_the_undefined_band():
    W, neg, pos, dneg, dpos = P.saturation_table()
    assert dneg.tolist() == [20, 25, 100, -20, -100] and dpos.tolist() == [-25, -40, -100, 20]
    assert not ((dneg > 12) & (dneg < 17.4)).any()
    rows = np.concatenate([neg, pos])
    assert rows.shape[1] == 2 and len(set(rows.ravel().tolist())) == rows.size and ((W != 0).sum(1)[rows.ravel()] == 1).all()
    # the reference's f32 arithmetic does what the test expects of the device: sigmoid exactly 1.0f above 17.4, gradient exactly 0
    w = torch.from_numpy(W).requires_grad_(True)
    out = (w[neg[:3, 0]] * w[neg[:3, 1]]).sum(-1)
    (-torch.log(1 - torch.sigmoid(out) + N.EPS)).sum().backward()
    assert (torch.sigmoid(out) == 1).all() and not w.grad.numpy().any()


@pytest.mark.parametrize("d", [9, 129])
def test_the_edge_cases_hold_exact_dots_and_self_pairs(d):
    for n in (1, 5, 1001):
        W, src, dst, ref = P.edge_case(d, n)
        assert len(src) == n and (src == dst).sum() >= 1 and np.isfinite(ref)
        got = float(N.edge_bce(torch.from_numpy(W).double(), src, dst))
        assert abs(got - ref) <= 1e-12 * ref
    dot = (W[src].astype(np.float64) * W[dst]).sum(1)
    assert dot[1] == 30 and dot[2] == -30
