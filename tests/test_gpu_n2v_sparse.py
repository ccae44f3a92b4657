"""Sparse Adam of the node2vec / metapath2vec producers (ntf_n2v_set_optimizer(1): k_n2v_touch -> k_n2v_compact -> k_n2v_adam_rows in
opentf_amd/csrc/ntf_n2v.hip) against torch.optim.SparseAdam restated in float64 (`sparse_adam_reference`; tests/test_n2v_sparse_host.py pins it to torch's
own and checks every condition the tests here put on their inputs, on any machine).

What is checked: W after several applied steps inside the bar of test_adam_over_steps_that_name_different_rows; rows a step does not name keep the BITS of
W and of both moments (dense Adam moves them); the moments after one step inside bars derived from the gradient's own; a touched row whose gradient is exactly
zero still moves; a row named hundreds of times is updated once; a pending gradient's rows are touched, a consumed one's are not; the edges of the bitmap's
words, of the compaction's waves and workgroups; a metapath handle with its dummy row through both pair kernels; native batches; the contract of the two new
entries; the plugin's `sparse` key.

The helpers need no GPU.  TEST INFRASTRUCTURE ONLY: numpy / torch float64.
"""
import functools
import os

import numpy as np
import pytest
import scipy.sparse
import torch

import n2v_reference
import test_gpu_n2v_parity as P
from n2v_reference import bits, net

pytestmark = pytest.mark.gpu
within_bar = functools.partial(n2v_reference.within_bar, "sparse")

U = P.U
B1, B2, EPS = 0.9, 0.999, 1e-8
LR = 0.01
SIZES = [1, 65, 192, 256]            # NV 1 to 4; a pad column at three of them


# ---------------------------------------------------------------------------------------------------------------- the float64 reference
def step_ref(W, step):
    """reference of one applied step: (pos, neg), or a list of such pairs whose gradients met in the buffer (apply = 0 calls, then the applied one)"""
    if isinstance(step[0], np.ndarray): return P.ref_batch(W, *step)
    return P.combine(*[p for pos, neg in step for p in P.ref_batch(W, pos, neg)["parts"]])


def sparse_adam_reference(W0, sets, lr=LR, b1=B1, b2=B2, eps=EPS):
    """torch.optim._functional.sparse_adam in float64, fed the float64 reference gradients: a row is touched in a step when a window of the step names it
    (`K > 0`: a start or a rest position), whatever its gradient; only touched rows change, bias correction by the global step.
    -> W, m, v after the steps, the per-step references, compare, named - the last three as `adam_reference` of tests/test_gpu_n2v_parity.py has them"""
    W = np.asarray(W0, dtype=np.float64).copy(); m = np.zeros_like(W); v = np.zeros_like(W)
    compare = np.ones(W.shape, dtype=bool); named = np.zeros(len(W), dtype=bool); refs = []
    for t, step in enumerate(sets, 1):
        ref = step_ref(W, step); refs.append(ref)
        g = ref["grad"]; here = ref["K"] > 0
        named |= here
        compare &= ~(here[:, None] & (np.abs(g) < 1e-7))
        m[here] += (1 - b1) * (g[here] - m[here])
        v[here] += (1 - b2) * (g[here] * g[here] - v[here])
        W[here] -= lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m[here] / (np.sqrt(v[here]) + eps)
    return W, m, v, refs, compare, named


@functools.lru_cache(None)
def five_steps(d):
    """the five window sets of `adam_window_sets` on table(d): the reference, computed once and left as it is"""
    out = sparse_adam_reference(P.table(d), P.adam_window_sets())
    for a in out[:3] + out[4:]: a.setflags(write=False)
    return out


@functools.lru_cache(None)
def zero_gradient_case(d=192):
    """row z: all zeros and named by no window of `adam_window_sets`; row a: named by its first set.  Step 1 is that set.  Step 2 names a only as the rest of
    two windows of two nodes that start at z, one positive and one negative: every term on row a is a coefficient times the zero row - exactly 0.0 in float64
    and in f32 alike - while a is touched.  -> W0, the two steps, a, z"""
    sets = P.adam_window_sets()
    named = five_steps(d)[5]
    z = int(np.flatnonzero(~named)[0])
    W0 = P.table(d).copy(); W0[z] = 0.0
    a = int(sets[0][0][0, 1])
    assert a != z
    two = np.array([[z, a]], dtype=np.int64)
    W0.setflags(write=False)
    return W0, [sets[0], (two, two.copy())], a, z


@functools.lru_cache(None)
def hub_case():
    """the hub is the first rest node of every window (K[hub] = 400); window 0 of the positive set starts at a node that is also its own last node"""
    rp, col, nn, sp = P.graph()
    hub = sp["hub"]
    s = np.setdiff1d(np.arange(nn), [hub])[:200]
    pos = np.stack([s, np.full(200, hub), np.roll(s, -1)], 1); pos[0, 2] = pos[0, 0]
    neg = np.stack([s, np.full(200, hub), np.roll(s, -7)], 1)
    return pos.astype(np.int64), neg.astype(np.int64), hub


def two_term_case():
    """windows of two nodes: positive (2 i, 2 i + 1), negative (2 i + 1, 2 i + 2), i < 200 - no row takes more than two gradient terms"""
    i = np.arange(200, dtype=np.int64)
    return np.stack([2 * i, 2 * i + 1], 1), np.stack([2 * i + 1, 2 * i + 2], 1)


BOUNDARY_N = 70000
# the first and last row, both sides of a bitmap word (32 rows), of a wave of k_n2v_compact (64 words = 2048 rows) and of its workgroup (256 words = 8192 rows)
BOUNDARY_ROWS = [0, 31, 32, 63, 64, 2047, 2048, 8191, 8192, 69998, 69999]


def boundary_case():
    W = (torch.rand(BOUNDARY_N, 1, generator=torch.Generator().manual_seed(7)) * 4 - 2).numpy()
    r = BOUNDARY_ROWS
    pos = np.array([[r[0], r[1]], [r[2], r[3]], [r[4], r[5]]], dtype=np.int64)
    neg = np.array([[r[6], r[7]], [r[8], r[9]], [r[10], r[0]]], dtype=np.int64)
    return W, pos, neg


# ================================================================================================================ the GPU tests
_net = functools.partial(net, sparse=True)


@pytest.mark.parametrize("d", SIZES)
def test_five_steps_match_sparse_adam_in_float64(d):
    W0 = P.table(d)
    sets = P.adam_window_sets()
    Wref, mref, vref, refs, compare, named = five_steps(d)
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs) and (~named).sum() >= 5
    net = _net(W0)
    for pos, neg in sets: net.loss_on(pos, neg, lr=LR, apply=True)
    Wd = net.weight(); m, v = net.moments()
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named]))           # rows never named: the input's bits, and moments that are exactly zero
    assert not bits(m[~named]).any() and not bits(v[~named]).any()
    within_bar(Wd, Wref, compare, f"d={d} five steps")
    assert not net.grad().view(np.uint32).any()                         # the step left the gradient zero everywhere


def test_rows_a_step_does_not_name_keep_their_bits():
    """fails under dense Adam, which moves every row that has a moment"""
    d = 65
    W0 = P.table(d)
    refs = five_steps(d)[3]
    net = _net(W0)
    W, (m, v) = net.weight(), net.moments()
    moved = 0
    for (pos, neg), ref in zip(P.adam_window_sets(), refs):
        net.loss_on(pos, neg, lr=LR, apply=True)
        W2, (m2, v2) = net.weight(), net.moments()
        rest = ref["K"] == 0
        assert rest.sum() > 300 and bits(m[rest]).any() == (moved > 0)          # from step 2 on such rows HAVE moments: dense Adam would move them
        for before, after in ((W, W2), (m, m2), (v, v2)): assert np.array_equal(bits(before[rest]), bits(after[rest]))
        assert (bits(W[~rest]) != bits(W2[~rest])).any(1).all()                 # ... and every named row moved
        W, m, v = W2, m2, v2; moved += 1


def test_one_step_from_zero_moments_gives_the_gradients_own_bars():
    d = 129
    W0 = P.table(d)
    pos, neg = P.injected_case()
    ref = P.ref_batch(W0, pos, neg)
    assert P.conditions_hold(ref)
    net = _net(W0)
    net.loss_on(pos, neg, lr=LR, apply=True)
    m, v = (x.astype(np.float64) for x in net.moments())
    g, bar = ref["grad"], ref["bar"]
    em = np.abs(m - (1 - B1) * g); bm = (1 - B1) * bar + 2 * U * np.abs(m)
    ev = np.abs(v - (1 - B2) * g * g); bv = (1 - B2) * (2 * np.abs(g) * bar + bar * bar) + 3 * U * np.abs(v)
    fm = np.divide(em, bm, out=np.zeros_like(em), where=bm > 0); fv = np.divide(ev, bv, out=np.zeros_like(ev), where=bv > 0)
    print(f"n2v sparse adam one step d={d}: exp_avg max err / bar {fm.max():.3f}, exp_avg_sq max err / bar {fv.max():.3f}")
    assert (em <= bm).all() and (ev <= bv).all()


def test_a_touched_row_with_a_zero_gradient_still_moves():
    W0, steps, a, z = zero_gradient_case()
    Wref, mref, vref, refs, compare, named = sparse_adam_reference(W0, steps)
    assert all(P.conditions_hold(r) for r in refs) and refs[1]["K"][a] == 2 and not refs[1]["grad"][a].any()
    net = _net(W0)
    net.loss_on(*steps[0], lr=LR, apply=True)
    W1, (m1, v1) = net.weight(), net.moments()
    assert not bits(W1[z]).any()                                         # z was not named: still the zero row, so step 2's terms on row a are 0.0 on the device too
    net.loss_on(*steps[1], lr=LR, apply=True)
    W2, (m2, v2) = net.weight(), net.moments()
    assert (bits(W2[a]) != bits(W1[a])).mean() > 0.9                     # it moved
    assert (np.abs(m2[a].astype(np.float64) - 0.9 * m1[a].astype(np.float64)) <= 2 * U * np.abs(m2[a])).all() and m1[a].any()
    # the 1e-7 rule of `compare` guards the sign of m / sqrt(v) where f32 does not decide the gradient's; a gradient that is 0.0 on both sides decides nothing:
    # on row a only step 1 counts
    compare = compare.copy(); compare[a] = np.abs(refs[0]["grad"][a]) >= 1e-7
    within_bar(W2, Wref, compare, "zero gradient on a touched row")


def test_a_row_named_hundreds_of_times_is_updated_once():
    d = 192
    W0 = P.table(d)
    pos, neg, hub = hub_case()
    Wref, mref, vref, refs, compare, named = sparse_adam_reference(W0, [(pos, neg)])
    assert P.conditions_hold(refs[0]) and refs[0]["K"][hub] == 400 and (pos[:, 1:] == pos[:, :1]).any()
    net = _net(W0)
    net.loss_on(pos, neg, lr=LR, apply=True)
    Wd = net.weight()
    within_bar(Wd, Wref, compare, "hub in every window")
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named]))


def test_a_pending_gradient_is_part_of_the_step_and_a_consumed_one_is_not():
    d = 192
    W0 = P.table(d)
    A, B = P.adam_window_sets()[:2]
    Wref, mref, vref, refs, compare, named = sparse_adam_reference(W0, [[A, B]])
    in_a = P.ref_batch(W0, *A)["K"] > 0; in_b = P.ref_batch(W0, *B)["K"] > 0
    only_a = in_a & ~in_b
    assert P.conditions_hold(refs[0]) and only_a.sum() > 50 and np.array_equal(named, in_a | in_b)
    net = _net(W0)
    net.loss_on(*A, apply=False)
    net.loss_on(*B, lr=LR, apply=True)
    Wd = net.weight()
    within_bar(Wd, Wref, compare, "A pending, B applied")
    assert (bits(Wd[only_a]) != bits(W0[only_a])).any(1).all()           # the rows only A names were touched
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named])) and not net.grad().view(np.uint32).any()
    # a gradient that was read is gone, and its marks with it
    Wref2, _, _, refs2, compare2, _ = sparse_adam_reference(W0, [B])
    net2 = _net(W0)
    P.parity(net2.loss_on(*A, apply=False), net2.grad(), P.ref_batch(W0, *A), "sparse mode, a gradient read back")
    net2.loss_on(*B, lr=LR, apply=True)
    W2 = net2.weight(); m2, v2 = net2.moments()
    assert np.array_equal(bits(W2[~in_b]), bits(W0[~in_b])) and not bits(m2[~in_b]).any() and not bits(v2[~in_b]).any()
    within_bar(W2, Wref2, compare2, "A consumed, B applied")


def test_bitmap_word_wave_and_workgroup_boundaries():
    from opentf_amd.libntf import Node2Vec
    W0, pos, neg = boundary_case()
    rows = np.array(BOUNDARY_ROWS)
    assert sorted(set(pos.ravel()) | set(neg.ravel())) == BOUNDARY_ROWS
    Wref, mref, vref, refs, compare, named = sparse_adam_reference(W0, [(pos, neg)])
    assert np.array_equal(np.flatnonzero(named), rows)
    net = Node2Vec(np.zeros(BOUNDARY_N + 1, np.int64), np.zeros(0, np.int32), W0, sparse=True)
    net.loss_on(pos, neg, lr=LR, apply=True)
    Wd = net.weight(); m, v = net.moments()
    changed = np.flatnonzero((bits(Wd) != bits(W0)).any(1))
    assert np.array_equal(changed, rows), changed
    assert np.array_equal(np.flatnonzero(m.any(1)), rows) and np.array_equal(np.flatnonzero(v.any(1)), rows)
    within_bar(Wd, Wref, compare, "bitmap boundaries")
    # a second step names two of them: the marks of the first were cleared
    net.loss_on(pos[:1], neg[:0], lr=LR, apply=True)
    W2 = net.weight()
    assert np.array_equal(np.flatnonzero((bits(W2) != bits(Wd)).any(1)), rows[:2])


@pytest.mark.parametrize("pairs", [1, 0])
def test_metapath_handle_with_its_dummy_row(pairs, monkeypatch):
    import test_gpu_m2v as M
    d = 129
    p = M.path(M.NATIVE_PATH)
    W0 = M.table(M.NATIVE_PATH, d)
    sets = [M.replay_step(t, steps=M.ADAM_STEPS)[2:] for t in range(len(M.ADAM_STEPS))]      # few negatives: some rows are named in no step
    Wref, mref, vref, refs, compare, named = sparse_adam_reference(W0, sets)
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs) and all(r["K"][p.total] > 0 for r in refs) and (~named).sum() >= 5
    net = M._net(M.NATIVE_PATH, W0, pairs=pairs, monkeypatch=monkeypatch)
    net.set_optimizer(True)
    for pos, neg in sets: net.loss_on(pos, neg, lr=LR, apply=True)
    Wd = net.weight()
    within_bar(Wd, Wref, compare, f"m2v pairs={pairs}")
    tol = 2e-5 + 1e-4 * np.abs(Wref[p.total])
    assert (np.abs(Wd[p.total] - Wref[p.total]) <= tol)[compare[p.total]].all() and compare[p.total].mean() > 0.9 and (bits(Wd[p.total]) != bits(W0[p.total])).any()
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named]))


def test_contract_of_set_optimizer_and_the_dense_default():
    from opentf_amd.libntf import NTF_EINVAL, NTF_ESTATE, NtfError, lib
    d = 65
    W0 = P.table(d)
    pos, neg = P.adam_window_sets()[0]
    net = _net(W0, sparse=False)
    with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): net._ck(lib().ntf_n2v_set_optimizer(net._h, 2))
    with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): net._ck(lib().ntf_n2v_set_optimizer(net._h, -1))
    net.set_optimizer(True); net.set_optimizer(False); net.set_optimizer(True)          # free before the first step
    net.loss_on(pos, neg, apply=False)
    with pytest.raises(NtfError, match=f"error {NTF_ESTATE}:"): net.set_optimizer(False)  # a gradient is pending
    net.grad()
    net.set_optimizer(True)                                                             # ... and no longer
    net.loss_on(pos, neg, lr=LR, apply=True)
    for kind in (False, True):
        with pytest.raises(NtfError, match=f"error {NTF_ESTATE}:"): net._ck(lib().ntf_n2v_set_optimizer(net._h, int(kind)))
    # the refused calls changed nothing: the handle is still a sparse one
    Wref, _, _, _, compare, named = sparse_adam_reference(W0, [(pos, neg)] * 2)
    net.loss_on(pos, neg, lr=LR, apply=True)
    Wd = net.weight()
    within_bar(Wd, Wref, compare, "after the refusals")
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named]))
    assert lib().ntf_n2v_moments(net._h, None, None) == 0
    # dense Adam is the default, and kind 0 is that default: the same bits, and the existing dense bar.  Two handles agree to the bit only where the gradient
    # itself does: its f32 atomic adds land in an order nobody fixes, and only a sum of at most two terms does not depend on that order (a + b = b + a).  So the
    # bits are compared on windows of two nodes that put at most two terms on a row; the window set above goes against the reference at its bar.
    p2, n2 = two_term_case()
    for wpos, wneg, exact in ((p2, n2, True), (pos, neg, False)):
        plain, zero = _net(W0, sparse=False), _net(W0, sparse=False)
        zero.set_optimizer(False)
        for h in (plain, zero):
            for _ in range(2): h.loss_on(wpos, wneg, lr=LR, apply=True)
        Wp, Wz = plain.weight(), zero.weight()
        if exact: assert np.array_equal(bits(Wp), bits(Wz)) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(plain.moments(), zero.moments()))
        Wdense, refs, cmp_dense, _ = P.adam_reference(W0, [(wpos, wneg)] * 2)
        assert all(P.conditions_hold(r) for r in refs) and (not exact or max(r["K"].max() for r in refs) == 2)
        for Wx in (Wp, Wz):
            err = np.abs(Wx - Wdense); tol = 2e-5 + 1e-4 * np.abs(Wdense)
            assert (err <= tol)[cmp_dense].all()


def test_native_batches_in_sparse_mode():
    d = 129
    rp, col, nn, _ = P.graph()
    W0 = P.table(d)
    B, wl, ctx, wpn, nneg = 97, 9, 4, 3, 2
    net = _net(W0, seed=P.NATIVE_SEED)
    sets = []
    for t in range(3):
        loss = net.train_batch(P.start_nodes(B, 10 + t), wl, ctx, wpn, nneg, LR)
        sets.append(net.last_windows())
        assert np.isfinite(loss) and sets[-1][0].shape == (B * wpn * (wl + 1 - ctx), ctx) and sets[-1][1].shape == (B * wpn * nneg * (wl + 1 - ctx), ctx)
    assert not np.array_equal(sets[0][1], sets[1][1])
    Wref, mref, vref, refs, compare, named = sparse_adam_reference(W0, sets)
    # 5 238 + 10 476 pairs a batch: each mean divides by 12 to 24 times what `adam_window_sets` divides by, so more elements fall under the (unscaled) 1e-7 of
    # `compare` - 4.4e-3 of them on the replayed windows at d = 129, a figure of the reference alone; 99 % of the table must still be compared
    assert (~compare).mean() <= 1e-2 and all(P.conditions_hold(r) for r in refs)
    Wd = net.weight()
    within_bar(Wd, Wref, compare, "three native batches")
    print(f"n2v sparse adam native: {int(named.sum())} of {nn} rows named in three batches, {(~compare).mean():.2e} of the elements left out")
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named]))


@pytest.mark.parametrize("method", ["n2v", "m2v"])
def test_plugin_trains_into_the_sparse_directory(method, tmp_path):
    import test_gpu_m2v as M
    from opentf_amd.mdl.emb.gnn import Gnn
    tv, sp, n, S, Mm = M._toy()
    L4 = [["member", "to", "team"], ["team", "rev_to", "skill"], ["skill", "to", "team"], ["team", "rev_to", "member"]]
    section = M.Cfg(d=16, w=3, e=2, b=8, lr=0.01, es=5, ns=2, spe=2, wl=4, wn=3, sparse=True)
    if method == "m2v": section["metapath_name"] = [L4, "mtstm"]
    cfg = M.Cfg(graph=M.Cfg(structure=[[["skill", "to", "team"], ["member", "to", "team"]], "stm"], dup_edge="add", pre=None), **{method: section})
    t2v = Gnn(str(tmp_path), "cuda:0", 0, cfg, method)
    t2v.learn(tv, sp)
    assert os.path.basename(t2v.output) == f"{method}.b8.e2.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl4.wn3" + (".mtstm" if method == "m2v" else "") + ".sparse"
    ck = torch.load(f"{t2v.output}/f0.pt", map_location="cpu", weights_only=False)
    assert list(ck.keys()) == ["model_state_dict", "cfg", "f", "e", "t_loss", "v_loss", "node_order", "node_offsets"]
    assert list(ck["model_state_dict"].keys()) == ["embedding.weight"]
    W = ck["model_state_dict"]["embedding.weight"].numpy()
    assert W.shape == (S + Mm + n + (method == "m2v"), 16) and np.isfinite(W).all() and np.isfinite(ck["t_loss"]) and np.isfinite(ck["v_loss"])
    lo = Mm if method == "m2v" else 0
    E = t2v.model[lo:lo + S]
    X = t2v.get_dense_vecs(tv, vectype="skill")
    sk = scipy.sparse.csr_matrix(tv["skill"]).astype(np.float64)
    np.testing.assert_allclose(X, np.asarray(sk @ E.astype(np.float64)) / np.asarray(sk.sum(1)), rtol=1e-6, atol=1e-7)
