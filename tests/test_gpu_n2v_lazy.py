"""Lazy dense Adam of the node2vec / metapath2vec producers (ntf_n2v_set_lazy: k_n2v_touch -> k_n2v_compact<false> -> k_n2v_catchup_rows before the pairs,
k_n2v_catchup_rows<.., true> after them, k_n2v_catchup_all for a full flush; opentf_amd/csrc/ntf_n2v.hip).

The claim: the table of dense Adam, bit for bit given bit-identical gradients, while a step writes only the rows its windows name.  So the tests hold a lazy
handle against (a) dense Adam in float64 at the bar of test_adam_over_steps_that_name_different_rows, (b) a DENSE HANDLE fed the same calls, as uint32 views -
on windows of two nodes, where no row takes more than two gradient terms and the f32 atomic adds of the two handles cannot differ (see
test_contract_of_set_optimizer_and_the_dense_default in tests/test_gpu_n2v_sparse.py) - and (c) a host model of the per-row step counter (`Model`), read
through ntf_n2v_lazy_state WITHOUT a flush: an implementation that swept every row every step would pass (a) and (b) and fail (c).

The helpers need no GPU; tests/test_n2v_lazy_host.py checks them and every condition the tests here put on their inputs.  TEST INFRASTRUCTURE ONLY.
"""
import functools
import os

import numpy as np
import pytest
import torch

import n2v_reference
import test_gpu_n2v_parity as P
from n2v_reference import bits, net as _net

pytestmark = pytest.mark.gpu

LR = 0.01
SIZES = [1, 65, 192, 193]            # NV 1 to 4; a pad column at three of them (256 leaves out 1.06e-3 of the elements, over the cap)
BIT_SIZES = [65, 193]
DEFAULT_WINDOW = 4096
within_bar = functools.partial(n2v_reference.within_bar, "lazy")


# ---------------------------------------------------------------------------------------------------------------- the two-term sequence
_I = np.arange(200)
MASKS = [_I >= 0, _I % 2 == 0, _I % 2 == 1, _I % 8 == 3, _I == 199, _I >= 0, _I % 50 == 7, _I % 50 == 7, _I >= 150, _I % 4 == 0, _I % 64 == 63, _I >= 0]
LRS = [1e-2] * 4 + [1e-3] * 4 + [1e-4] * 4


def two_term(mask):
    """windows of two nodes, positive (2 j, 2 j + 1) and negative (2 j + 1, 2 j + 2) for the j of the mask: no row takes more than two gradient terms"""
    j = _I[np.asarray(mask)].astype(np.int64)
    return np.stack([2 * j, 2 * j + 1], 1), np.stack([2 * j + 1, 2 * j + 2], 1)


def sequence():
    """twelve steps (pos, neg, lr): a row stays out for 0, 1, several and many steps, and the lr changes twice"""
    return [two_term(m) + (lr,) for m, lr in zip(MASKS, LRS)]


def rows_of(pos, neg):
    return np.unique(np.concatenate([np.asarray(pos).ravel(), np.asarray(neg).ravel()])).astype(np.int64)


def dense_reference(W0, seq, b1=0.9, b2=0.999, eps=1e-8):
    """P.adam_reference with a learning rate per step: float64 dense Adam fed the float64 reference gradients -> W, the per-step references"""
    W = np.asarray(W0, dtype=np.float64).copy(); m = np.zeros_like(W); v = np.zeros_like(W); refs = []
    for t, (pos, neg, lr) in enumerate(seq, 1):
        ref = P.ref_batch(W, pos, neg); refs.append(ref)
        g = ref["grad"]
        m = b1 * m + (1 - b1) * g; v = b2 * v + (1 - b2) * g * g
        W = W - lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return W, refs


class Model:
    """what ntf_n2v_lazy_state must show, from the contract in include/opentf_amd.h alone: `applied` per row, the handle's steps, the full flushes.
    A row has moments once an applied step named it; a full flush moves exactly those rows."""

    def __init__(self, n, window=DEFAULT_WINDOW):
        self.applied = np.zeros(n, dtype=np.uint32); self.live = np.zeros(n, dtype=bool)
        self.window, self.steps, self.base, self.flushes = window, 0, 0, 0

    def flush(self):
        if self.steps == self.base: return
        self.applied[self.live] = self.steps; self.base = self.steps; self.flushes += 1

    def batch(self, rows, apply=True, pending=()):
        """`rows`: named by this call; `pending`: named by earlier apply = 0 calls whose gradient is still in the buffer"""
        rows = np.union1d(rows, np.asarray(pending, dtype=np.int64)).astype(np.int64)
        self.applied[rows] = self.steps
        if not apply: return
        if self.steps - self.base == self.window: self.flush()
        self.steps += 1
        self.applied[rows] = self.steps; self.live[rows] = True

    def read(self):            # weight() / moments()
        self.flush()

    def edges(self, rows):     # edge_bce with no gradient pending
        self.applied[np.asarray(rows, dtype=np.int64)] = self.steps


def state_is(net, model, tag):
    a, steps, flushes = net.lazy_state()
    assert steps == model.steps and flushes == model.flushes, (tag, steps, model.steps, flushes, model.flushes)
    bad = np.flatnonzero(a != model.applied)
    assert not len(bad), (tag, bad[:8], a[bad[:8]], model.applied[bad[:8]])


@functools.lru_cache(None)
def five_steps(d):
    """P.adam_reference on the five window sets of `adam_window_sets`, computed once and left as it is"""
    out = P.adam_reference(P.table(d), P.adam_window_sets())
    for a in (out[0], out[2], out[3]): a.setflags(write=False)
    return out


def native_sets_replayed():
    """three native batches of (97, 9, 4, 3, 2) of a handle of seed NATIVE_SEED, replayed on the host"""
    rp, col, nn, _ = P.graph()
    B, wl, ctx, wpn, nneg = 97, 9, 4, 3, 2
    sets = []
    for t in range(3):
        b = P.start_nodes(B, 10 + t)
        pos = P.N.windows(torch.from_numpy(P.replay_walks(rp, col, b, B * wpn, wl, P.NATIVE_SEED, t)), ctx).numpy()
        neg = P.N.windows(torch.from_numpy(P.replay_negs(b, B * wpn * nneg, wl, nn, P.NATIVE_SEED, t)), ctx).numpy()
        sets.append((pos, neg))
    return sets


def edge_set():
    """held-out edges for edge_bce after step 8: endpoints left behind since step 6, current ones (14 to 16), a self-pair, and rows no window ever names"""
    src = np.array([0, 1, 14, 15, 6, 7, 300, 398, 399, 400, 401, 550, 554, 0], dtype=np.int64)
    dst = np.array([1, 2, 15, 16, 7, 7, 301, 399, 400, 401, 402, 551, 0, 554], dtype=np.int64)
    return src, dst


def bce64(W, src, dst):
    dot = (W[src].astype(np.float64) * W[dst]).sum(1)
    return float(np.mean(np.maximum(-dot, 0) + np.log1p(np.exp(-np.abs(dot)))))


# ================================================================================================================ the GPU tests
def _same_bits(lazy, dense, tag):
    Wl, Wd = lazy.weight(), dense.weight()
    (ml, vl), (md, vd) = lazy.moments(), dense.moments()
    for name, x, y in (("W", Wl, Wd), ("exp_avg", ml, md), ("exp_avg_sq", vl, vd)):
        ne = bits(x) != bits(y)
        assert not ne.any(), (tag, name, int(ne.sum()), np.argwhere(ne)[:4])
    return Wl


@pytest.mark.parametrize("window", [True, 3])
@pytest.mark.parametrize("d", SIZES)
def test_five_steps_match_dense_adam_in_float64(d, window):
    W0 = P.table(d)
    Wref, refs, compare, named = five_steps(d)
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs) and (~named).sum() >= 5
    net = _net(W0, lazy=window)
    for pos, neg in P.adam_window_sets(): net.loss_on(pos, neg, lr=LR, apply=True)
    a, steps, flushes = net.lazy_state()
    assert steps == 5 and flushes == (0 if window is True else 1) and not a[~named].any()      # window 3: the flush falls before step 4
    Wd = net.weight(); m, v = net.moments()
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named])) and not bits(m[~named]).any() and not bits(v[~named]).any()
    within_bar(Wd, Wref, compare, f"d={d} window={window} five steps")
    assert not net.grad().view(np.uint32).any()


@pytest.mark.parametrize("window,read", [(True, False), (True, True), (1, False), (3, False)])
@pytest.mark.parametrize("d", BIT_SIZES)
def test_twelve_steps_bit_for_bit_against_a_dense_handle_and_rows_left_behind(d, window, read):
    """after every step, BEFORE any read: `applied` is the last step that named the row, or the last full flush if that came later (rows that have moments), 0
    for rows never named.  At the end the three tables are the dense handle's, bit for bit."""
    W0 = P.table(d)
    lazy, dense = _net(W0, lazy=window), _net(W0)
    model = Model(len(W0), DEFAULT_WINDOW if window is True else window)
    behind = 0
    for t, (pos, neg, lr) in enumerate(sequence(), 1):
        for h in (lazy, dense): h.loss_on(pos, neg, lr=lr, apply=True)
        model.batch(rows_of(pos, neg))
        state_is(lazy, model, f"d={d} window={window} step {t}")
        behind = max(behind, int((model.live & (model.applied < t)).sum()))
        if read and t == 4:
            lazy.weight(); model.read()
            state_is(lazy, model, "after weight()")
            assert model.flushes == 1 and (model.applied[model.live] == 4).all() and not model.applied[~model.live].any()
    if window is True: assert behind >= 390 and model.flushes == int(read)          # rows that have moments really were left behind, and no flush came unasked
    else: assert model.flushes == {3: 3, 1: 11}[window]                            # before steps 4, 7 and 10; before every step but the first
    _same_bits(lazy, dense, f"d={d} window={window} read={read}")
    model.read()
    state_is(lazy, model, "after the final reads")
    assert (model.applied[model.live] == 12).all() and model.live.sum() == 401


def test_edge_bce_brings_only_its_endpoints_up_to_date():
    d = 65
    W0 = P.table(d)
    seq = sequence()
    lazy, dense = _net(W0, lazy=True), _net(W0)
    model = Model(len(W0))
    for pos, neg, lr in seq[:8]:
        for h in (lazy, dense): h.loss_on(pos, neg, lr=lr, apply=True)
        model.batch(rows_of(pos, neg))
    src, dst = edge_set()
    ends = np.union1d(src, dst)
    assert (model.applied[ends] < 8).sum() >= 10 and (~model.live[ends]).sum() >= 3
    ref = bce64(dense.weight(), src, dst)
    got = lazy.edge_bce(src, dst)
    model.edges(ends)
    print(f"n2v lazy edge_bce: {got:.8f} ref {ref:.8f} rel {abs(got - ref) / ref:.2e}")
    assert abs(got - ref) <= 1e-6 * ref
    state_is(lazy, model, "after edge_bce")                                         # exactly the endpoints' rows advanced, flushes still 0
    assert model.flushes == 0 and (model.applied[ends] == 8).all()
    # with a gradient pending the marks belong to it: a full flush instead, and the next applied step still applies the pending gradient
    A, B = two_term(_I % 2 == 0), two_term(_I % 2 == 1)
    for h in (lazy, dense): h.loss_on(*A, apply=False)
    model.batch(rows_of(*A), apply=False)
    got = lazy.edge_bce(src, dst); model.flush()
    assert abs(got - ref) <= 1e-6 * ref and model.flushes == 1
    state_is(lazy, model, "edge_bce with a gradient pending")
    for h in (lazy, dense): h.loss_on(*B, lr=1e-3, apply=True)
    model.batch(rows_of(*B), pending=rows_of(*A))
    state_is(lazy, model, "the step after it")
    _same_bits(lazy, dense, "pending gradient across an edge_bce")
    assert not lazy.grad().view(np.uint32).any()


@pytest.mark.parametrize("consumed", [False, True])
def test_pending_and_consumed_gradients(consumed):
    d = 193
    W0 = P.table(d)
    lazy, dense = _net(W0, lazy=True), _net(W0)
    model = Model(len(W0))
    first = sequence()[0]
    for h in (lazy, dense): h.loss_on(first[0], first[1], lr=LR, apply=True)       # so that rows have moments to be left behind with
    model.batch(rows_of(*first[:2]))
    A, B = two_term(_I % 2 == 0), two_term(_I % 2 == 1)
    for h in (lazy, dense): h.loss_on(*A, apply=False)
    model.batch(rows_of(*A), apply=False)
    pending = rows_of(*A)
    if consumed:
        gl, gd = lazy.grad(), dense.grad()
        assert np.array_equal(bits(gl), bits(gd)) and gl.any()
        pending = ()
    for h in (lazy, dense): h.loss_on(*B, lr=LR, apply=True)
    model.batch(rows_of(*B), pending=pending)
    state_is(lazy, model, f"consumed={consumed}")
    if consumed: assert (model.applied[np.setdiff1d(rows_of(*A), rows_of(*B))] == 1).all()   # brought to step 1 for the pairs, and not part of step 2
    _same_bits(lazy, dense, f"A {'consumed' if consumed else 'pending'}, B applied")


@pytest.mark.parametrize("pairs", [1, 0])
def test_metapath_handle_with_its_dummy_row(pairs, monkeypatch):
    import test_gpu_m2v as M
    d = 129
    p = M.path(M.NATIVE_PATH)
    W0 = M.table(M.NATIVE_PATH, d)
    sets = [M.replay_step(t, steps=M.ADAM_STEPS)[2:] for t in range(len(M.ADAM_STEPS))]
    Wref, refs, compare, named = P.adam_reference(W0, sets)
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs) and all(r["K"][p.total] > 0 for r in refs) and (~named).sum() >= 5
    net = M._net(M.NATIVE_PATH, W0, pairs=pairs, monkeypatch=monkeypatch)
    net.set_lazy(True)
    model = Model(len(W0))
    for pos, neg in sets:
        net.loss_on(pos, neg, lr=LR, apply=True); model.batch(rows_of(pos, neg))
    state_is(net, model, f"m2v pairs={pairs}")
    assert (model.live & (model.applied < 3)).sum() >= 5
    Wd = net.weight()
    within_bar(Wd, Wref, compare, f"m2v pairs={pairs}")
    tol = 2e-5 + 1e-4 * np.abs(Wref[p.total])
    assert (np.abs(Wd[p.total] - Wref[p.total]) <= tol)[compare[p.total]].all() and compare[p.total].mean() > 0.9 and (bits(Wd[p.total]) != bits(W0[p.total])).any()
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named]))


def test_native_batches_in_lazy_mode():
    d = 129
    rp, col, nn, _ = P.graph()
    W0 = P.table(d)
    B, wl, ctx, wpn, nneg = 97, 9, 4, 3, 2
    net = _net(W0, lazy=True, seed=P.NATIVE_SEED)
    model = Model(nn)
    sets = []
    for t in range(3):
        loss = net.train_batch(P.start_nodes(B, 10 + t), wl, ctx, wpn, nneg, LR)
        sets.append(net.last_windows())
        model.batch(rows_of(*sets[-1]))
        assert np.isfinite(loss) and sets[-1][0].shape == (B * wpn * (wl + 1 - ctx), ctx) and sets[-1][1].shape == (B * wpn * nneg * (wl + 1 - ctx), ctx)
    assert all(np.array_equal(x, y) for got, want in zip(sets, native_sets_replayed()) for x, y in zip(got, want))
    state_is(net, model, "three native batches")
    Wref, refs, compare, named = P.adam_reference(W0, sets, lr=LR)
    assert (~compare).mean() <= 1e-2 and all(P.conditions_hold(r) for r in refs)      # the cap of test_native_batches_in_sparse_mode, for its reason
    Wd = net.weight()
    within_bar(Wd, Wref, compare, "three native batches")
    print(f"n2v lazy adam native: {int(named.sum())} of {nn} rows named in three batches, {(~compare).mean():.2e} of the elements left out")
    assert np.array_equal(bits(Wd[~named]), bits(W0[~named]))


def test_contract_of_set_lazy_and_lazy_state():
    from opentf_amd.libntf import NTF_EINVAL, NTF_ESTATE, NtfError, lib
    d = 65
    W0 = P.table(d)
    seq = sequence()
    net = _net(W0)
    estate, einval = f"error {NTF_ESTATE}:", f"error {NTF_EINVAL}:"
    with pytest.raises(NtfError, match=estate): net.lazy_state()                     # not a lazy handle
    with pytest.raises(NtfError, match=einval): net.set_lazy(-1)
    net.set_optimizer(True)
    with pytest.raises(NtfError, match=estate): net.set_lazy(8)                      # a sparse handle
    assert net.lazy == 0 and net.sparse
    net.set_optimizer(False)
    net.set_lazy(8); net.set_lazy(0); net.set_lazy(True); net.set_lazy(5)            # free before the first step
    with pytest.raises(NtfError, match=estate): net.set_optimizer(True)              # a lazy handle takes no sparse Adam ...
    with pytest.raises(NtfError, match=einval): net._ck(lib().ntf_n2v_set_optimizer(net._h, 2))
    net.set_optimizer(False)                                                         # ... and kind 0 is what it has
    assert net.lazy == 5 and not net.sparse and net.lazy_state()[1:] == (0, 0)
    assert lib().ntf_n2v_lazy_state(net._h, None, None, None) == 0
    net.loss_on(*seq[0][:2], apply=False)
    for w in (0, 7):
        with pytest.raises(NtfError, match=estate): net.set_lazy(w)                  # a gradient is pending
    net.grad()
    net.set_lazy(5)
    dense = _net(W0)
    model = Model(len(W0), 5)
    for pos, neg, lr in seq[:2]:
        for h in (net, dense): h.loss_on(pos, neg, lr=lr, apply=True)
        model.batch(rows_of(pos, neg))
    for w in (0, 5, 9):
        with pytest.raises(NtfError, match=estate): net.set_lazy(w)                  # a step has been applied
    with pytest.raises(NtfError, match=estate): net.set_optimizer(True)
    with pytest.raises(NtfError, match=einval): net.set_lazy(-3)
    state_is(net, model, "after the refusals")                                      # the refused calls changed nothing: still lazy, window 5
    for pos, neg, lr in seq[2:]:
        for h in (net, dense): h.loss_on(pos, neg, lr=lr, apply=True)
        model.batch(rows_of(pos, neg))
    state_is(net, model, "twelve steps, window 5")
    assert model.flushes == 2                                                       # before steps 6 and 11
    _same_bits(net, dense, "after the refusals")
    # lazy=False, set_lazy(0) and a handle never asked are the same dense handle
    plain, off, unset = _net(W0), _net(W0, lazy=False), _net(W0, lazy=True)
    unset.set_lazy(0)
    for h in (plain, off, unset):
        for pos, neg, lr in seq[:4]: h.loss_on(pos, neg, lr=lr, apply=True)
        with pytest.raises(NtfError, match=estate): h.lazy_state()
    _same_bits(off, plain, "lazy=False"); _same_bits(unset, plain, "set_lazy(0)")


@pytest.mark.parametrize("method", ["n2v", "m2v"])
def test_plugin_with_the_lazy_key_trains_into_the_dense_directory(method, tmp_path, monkeypatch):
    import scipy.sparse
    import test_gpu_m2v as M
    from opentf_amd import libntf
    from opentf_amd.mdl.emb.gnn import Gnn
    cls = libntf.MetaPath2Vec if method == "m2v" else libntf.Node2Vec
    seen = []
    real_init = cls.__init__

    def spy(self, *a, **kw):
        real_init(self, *a, **kw); seen.append((kw.get("lazy"), kw.get("sparse"), self.lazy, self.lazy_state()[2], self.weight()))
    monkeypatch.setattr(cls, "__init__", spy)
    tv, sp, n, S, Mm = M._toy()
    L4 = [["member", "to", "team"], ["team", "rev_to", "skill"], ["skill", "to", "team"], ["team", "rev_to", "member"]]
    section = M.Cfg(d=16, w=3, e=2, b=8, lr=0.01, es=5, ns=2, spe=2, wl=4, wn=3, lazy=True)
    if method == "m2v": section["metapath_name"] = [L4, "mtstm"]
    cfg = M.Cfg(graph=M.Cfg(structure=[[["skill", "to", "team"], ["member", "to", "team"]], "stm"], dup_edge="add", pre=None), **{method: section})
    t2v = Gnn(str(tmp_path), "cuda:0", 0, cfg, method)
    t2v.learn(tv, sp)
    assert len(seen) >= 1 and all(s[:4] == (True, False, DEFAULT_WINDOW, 0) for s in seen)          # the handle was made lazy
    assert os.path.basename(t2v.output) == f"{method}.b8.e2.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl4.wn3" + (".mtstm" if method == "m2v" else "")
    ck = torch.load(f"{t2v.output}/f0.pt", map_location="cpu", weights_only=False)
    assert list(ck.keys()) == ["model_state_dict", "cfg", "f", "e", "t_loss", "v_loss", "node_order", "node_offsets"]
    assert list(ck["model_state_dict"].keys()) == ["embedding.weight"]
    W = ck["model_state_dict"]["embedding.weight"].numpy()
    assert W.shape == (S + Mm + n + (method == "m2v"), 16) and np.isfinite(W).all() and np.isfinite(ck["t_loss"]) and np.isfinite(ck["v_loss"])
    assert W.shape == seen[0][4].shape and (bits(W) != bits(seen[0][4])).any()                        # trained: no longer the initial draw
    lo = Mm if method == "m2v" else 0
    E = t2v.model[lo:lo + S]
    X = t2v.get_dense_vecs(tv, vectype="skill")
    sk = scipy.sparse.csr_matrix(tv["skill"]).astype(np.float64)
    np.testing.assert_allclose(X, np.asarray(sk @ E.astype(np.float64)) / np.asarray(sk.sum(1)), rtol=1e-6, atol=1e-7)
