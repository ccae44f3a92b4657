"""The host side of test_gpu_n2v_lazy.py without a GPU: the two entries and the `lazy` keyword, the plugin's key, the host model of the per-row step counter,
and every condition the GPU tests put on their inputs (the figures in the messages are the float64 reference's alone)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import test_gpu_n2v_lazy as L
import test_gpu_n2v_parity as P
from n2v_reference import global_generators_left_as_found, plugin_cfg as _cfg      # the fixture: autouse


def test_the_two_entries_are_declared_and_bound():
    from opentf_amd import libntf
    assert libntf.SYMBOLS["ntf_n2v_set_lazy"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert libntf.SYMBOLS["ntf_n2v_lazy_state"] == (ctypes.c_int, [ctypes.c_void_p] * 4)
    assert len(libntf.SYMBOLS) == 90
    for cls in (libntf.Node2Vec, libntf.MetaPath2Vec):
        assert inspect.signature(cls.__init__).parameters["lazy"].default is False
        assert callable(cls.set_lazy) and callable(cls.lazy_state)
    assert libntf.Node2Vec.LAZY_WINDOW == L.DEFAULT_WINDOW == 4096


@pytest.mark.parametrize("method", ["n2v", "m2v"])
def test_the_plugin_keeps_the_dense_directory_and_refuses_lazy_with_sparse(method, tmp_path):
    from opentf_amd.mdl.emb.gnn import Gnn
    plain = f"/{method}.b16.e4.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl5.wn3" + (".mtstm" if method == "m2v" else "")
    for kw in ({}, {"lazy": False}, {"lazy": True}, {"lazy": True, "sparse": False}):
        g = Gnn(str(tmp_path), "cpu", 0, _cfg(method, **kw), method)
        assert g._dirname() == plain and g._lazy() == bool(kw.get("lazy"))
    with pytest.raises(ValueError, match="lazy"): Gnn(str(tmp_path), "cpu", 0, _cfg(method, lazy=True, sparse=True), method)
    assert Gnn(str(tmp_path), "cpu", 0, _cfg(method, sparse=True), method)._dirname() == plain + ".sparse"


@pytest.mark.parametrize("d,share", [(1, 0.0), (65, 5.0e-4), (192, 8.3e-4), (193, 6.3e-4)])
def test_the_share_of_left_out_elements_stays_under_its_cap(d, share):
    Wref, refs, compare, named = L.five_steps(d)
    got = float((~compare).mean())
    print(f"dense reference d={d}: {got:.2e} of the elements left out, {int((~named).sum())} rows never named")
    assert got <= 1e-3 and abs(got - share) <= 0.06 * share + 1e-12 and all(P.conditions_hold(r) for r in refs)
    assert (~named).sum() == 37
    K = np.stack([r["K"] > 0 for r in refs])
    assert all((K[t] & ~K[t + 1]).sum() >= 100 for t in range(4))                 # rows with moments that the next step does not name: the ones left behind


@pytest.mark.parametrize("d", L.BIT_SIZES)
def test_the_two_term_sequence_is_what_it_says(d):
    seq = L.sequence()
    assert len(seq) == 12 and [s[2] for s in seq] == [1e-2] * 4 + [1e-3] * 4 + [1e-4] * 4
    W, refs = L.dense_reference(P.table(d), seq)
    assert all(P.conditions_hold(r) for r in refs) and all(r["K"].max() == 2 for r in refs)
    assert all(np.abs(r["grad"][r["K"] > 0]).max(1).min() > 0 for r in refs)     # every named row takes a gradient: it has moments from then on (`Model.live`)
    assert [len(s[0]) for s in seq] == [200, 100, 100, 25, 1, 200, 4, 4, 50, 50, 3, 200]
    # the pending pair of the GPU tests: the even and the odd windows together are the whole set, so still at most two terms on a row
    A, B = L.two_term(L._I % 2 == 0), L.two_term(L._I % 2 == 1)
    both = P.ref_batch(P.table(d), np.concatenate([A[0], B[0]]), np.concatenate([A[1], B[1]]))
    assert both["K"].max() == 2 and len(np.setdiff1d(L.rows_of(*A), L.rows_of(*B))) == 101
    # a row stays out for 0, 1, several and many steps
    last = np.zeros(401, dtype=int); gaps = set()
    for t, (pos, neg, lr) in enumerate(seq, 1):
        r = L.rows_of(pos, neg); gaps |= set((t - last[r])[last[r] > 0]); last[r] = t
    assert {1, 2, 3, 5, 6} <= gaps and max(gaps) >= 6


def test_the_model_follows_the_ring_rule():
    seq = L.sequence()
    for window, flushes in ((L.DEFAULT_WINDOW, 0), (1, 11), (3, 3), (5, 2)):
        m = L.Model(555, window)
        for pos, neg, lr in seq: m.batch(L.rows_of(pos, neg))
        assert (m.flushes, m.steps, int(m.live.sum())) == (flushes, 12, 401) and not m.applied[401:].any()
        assert m.steps - m.base <= window
        extra = int(m.base != 12)                                                   # a read flushes only when some step is outstanding
        m.read(); m.read()
        assert (m.applied[:401] == 12).all() and not m.applied[401:].any() and m.flushes == flushes + extra and m.base == 12
    m = L.Model(555)
    for pos, neg, lr in seq[:8]: m.batch(L.rows_of(pos, neg))
    src, dst = L.edge_set()
    ends = np.union1d(src, dst)
    assert (m.applied[ends] < 8).sum() >= 10 and (~m.live[ends]).sum() >= 3 and (m.applied[ends] == 8).sum() >= 3 and (src == dst).any()
    assert ends.max() < P.graph()[2]


def test_the_metapath_case_names_the_dummy_row_and_leaves_rows_behind():
    import test_gpu_m2v as M
    p = M.path(M.NATIVE_PATH)
    W0 = M.table(M.NATIVE_PATH, 129)
    sets = [M.replay_step(t, steps=M.ADAM_STEPS)[2:] for t in range(len(M.ADAM_STEPS))]
    Wref, refs, compare, named = P.adam_reference(W0, sets)
    got = float((~compare).mean())
    print(f"dense reference on the metapath sets, d=129: {got:.2e} left out, the dummy row named {[int(r['K'][p.total]) for r in refs]} times")
    assert got <= 1e-3 and abs(got - 9.2e-5) <= 0.06 * 9.2e-5 and all(P.conditions_hold(r) for r in refs)
    assert [int(r["K"][p.total]) for r in refs] == [11, 89, 40] and (~named).sum() >= 5 and compare[p.total].mean() > 0.9
    m = L.Model(len(W0))
    for pos, neg in sets: m.batch(L.rows_of(pos, neg))
    assert (m.live & (m.applied < 3)).sum() >= 5


def test_the_native_batches_stay_under_their_cap():
    sets = L.native_sets_replayed()
    assert [s[0].shape for s in sets] == [(97 * 3 * 6, 4)] * 3 and [s[1].shape for s in sets] == [(97 * 3 * 2 * 6, 4)] * 3
    Wref, refs, compare, named = P.adam_reference(P.table(129), sets, lr=L.LR)
    got = float((~compare).mean())
    print(f"dense reference on three replayed native batches, d=129: {got:.2e} of the elements left out")
    assert got <= 1e-2 and abs(got - 4.2e-3) <= 0.06 * 4.2e-3 and all(P.conditions_hold(r) for r in refs)
