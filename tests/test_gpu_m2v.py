"""metapath2vec producer on the MI355X (ntf_m2v_create, k_m2v_walks / k_m2v_negs / k_n2v_pairs<NV, DUMMY> in opentf_amd/csrc/ntf_n2v.hip) against tests/m2v_reference.py:
typed walks and negatives replayed bit for bit from the Philox counters, native batches against the float64 reference of tests/test_gpu_n2v_parity.py inside its
bars (dummy row included), Adam over applied native steps, every refusal of the contract, the `Gnn_m2v` plugin on toy dblp and a learning-signal check.

The helpers (graph, metapaths, tables, replay) need no GPU.  Both forms of the pair kernel are run: NTF_M2V_PAIRS=0 sends a metapath handle's pairs through the
plain k_n2v_pairs<NV, false>, 1 through k_n2v_pairs<NV, true> (the dummy row's terms summed per workgroup), at every NV = 1 .. 4 (d = 9, 65, 129, 256).

Metapaths: member -> team -> member (2 hops), member -> team -> skill -> team -> member (4 hops), skill -> team -> member (2 hops, 3 node positions, NOT a
cycle: it admits walks of at most 3 nodes, longer ones are refused - so its walk lengths are {2, 3}, the cycles' are {2, 5, 9}).
"""
import functools
import os

import numpy as np
import pytest
import scipy.sparse
import torch

import m2v_reference as R
import test_gpu_n2v_parity as P
from n2v_reference import Cfg, toy_dblp
from opentf_amd.synth import zipf_csr

pytestmark = pytest.mark.gpu

N_TEAM, N_SKILL, N_MEMBER = 150, 41, 61          # the last skill and the last member are in no team
PATHS = {"mtm": R.MTM, "mtstm": R.MTSTM, "stm": R.STM}
WALK_NODES = {"mtm": [2, 5, 9], "mtstm": [2, 5, 9], "stm": [2, 3]}
B_WALKS, WPN_WALKS = 16, 20                      # 320 walks: more than one block of 256 threads
SEED = 11


# ---------------------------------------------------------------------------------------------------------------- graph, paths, tables (no GPU)
@functools.lru_cache(None)
def graph():
    """Zipf skill - team - member graph: 150 teams over 40 skills and 60 members, plus one skill and one member that no team holds; every fourth team is DROPPED
    (no member edges in either direction, what the plugin does to the test / validation teams).  -> skill [team, skill], member [team, member] (dropped rows
    emptied), the dropped teams"""
    s_ip, s_ix = zipf_csr(N_TEAM, N_SKILL - 1, 3.0, 1)
    m_ip, m_ix = zipf_csr(N_TEAM, N_MEMBER - 1, 3.0, 2)
    skill = scipy.sparse.csr_matrix((np.ones(len(s_ix), np.uint8), s_ix, s_ip), shape=(N_TEAM, N_SKILL))
    member = scipy.sparse.csr_matrix((np.ones(len(m_ix), np.uint8), m_ix, m_ip), shape=(N_TEAM, N_MEMBER))
    drop = np.arange(0, N_TEAM, 4)
    return skill, member, drop


@functools.lru_cache(None)
def path(name):
    skill, member, drop = graph()
    p = R.Path({"member": N_MEMBER, "skill": N_SKILL, "team": N_TEAM}, PATHS[name], R.hop_csrs(skill, member, drop))
    deg0 = np.diff(p.hops[0][2])
    assert deg0[-1] == 0 and deg0.max() >= 8                       # the start type's last node is the one in no team; a hub exists
    if name != "mtm": assert not np.diff(p.hops[-1][2])[drop].any()  # team -> member: the dropped teams are dead ends
    return p


def hub(name):
    return int(np.argmax(np.diff(path(name).hops[0][2])))


def start_nodes(name, B=B_WALKS, seed=0):
    """B distinct LOCAL start ids: the node in no team and the hub first, the rest drawn"""
    p = path(name)
    n0 = int(p.count[p.hops[0][0]])
    first = [n0 - 1, hub(name)]
    rest = np.setdiff1d(np.arange(n0), first)
    return np.concatenate([first, np.random.default_rng(seed).choice(rest, B - 2, replace=False)]).astype(np.int64)


def dummy_share(rw, p):
    return float((rw == p.total).any(1).mean())


@functools.lru_cache(None)
def replayed_walks(name, nodes, step):
    p = path(name)
    rw = R.replay_walks(p, start_nodes(name), B_WALKS * WPN_WALKS, nodes, SEED, step)
    rw.setflags(write=False)
    return rw


TABLE_SEED = {}      # d -> the seed of its table where seed 0 breaks `conditions_hold` on the batches below (chosen on the CPU; none needed)


@functools.lru_cache(None)
def table(name, d):
    """the well-conditioned regime of tests/test_gpu_n2v_parity.table on [total + 1, d]; the dummy row is an ordinary row"""
    n = path(name).total + 1
    gen = torch.Generator().manual_seed(1000 * TABLE_SEED.get(d, 0) + d)
    W = torch.randn(n, d, generator=gen)
    return (W * (0.03 + 0.16 * torch.rand(n, 1, generator=gen)) * float(np.sqrt(128.0 / d))).float().numpy()


NATIVE_SIZES = [9, 65, 129, 256]
# step -> (B, nodes per walk, context, walks per node, negatives): several windows per walk; one window per walk (the reference's shape); no negatives
NATIVE_STEPS = ((16, 9, 4, 3, 2), (13, 5, 5, 2, 1), (16, 6, 3, 1, 0))
# the Adam test's: few negatives, so that some rows are named in no step and others not in every step
ADAM_STEPS = ((8, 5, 3, 1, 1), (8, 9, 4, 1, 0), (8, 6, 3, 2, 1))
NATIVE_PATH = "mtstm"


@functools.lru_cache(None)
def replay_step(t, name=NATIVE_PATH, seed=SEED, steps=NATIVE_STEPS):
    """what call t of a handle of this seed draws: LOCAL start ids, walks, positive windows, negative windows"""
    p = path(name)
    B, nodes, ctx, wpn, nneg = steps[t]
    batch = start_nodes(name, B, 10 + t)
    rw = R.replay_walks(p, batch, B * wpn, nodes, seed, t)
    pos = R.windows(rw, ctx)
    neg = R.windows(R.replay_negs(p, batch, B * wpn * nneg, nodes, seed, t), ctx) if nneg else np.zeros((0, ctx), np.int64)
    return batch, rw, pos, neg


def _net(name, W, seed=SEED, pairs=None, monkeypatch=None):
    from opentf_amd.libntf import MetaPath2Vec
    if pairs is not None: monkeypatch.setenv("NTF_M2V_PAIRS", str(pairs))
    p = path(name) if isinstance(name, str) else name
    return MetaPath2Vec(p.count, p.hops, W, seed=seed)


# ================================================================================================================ the GPU tests
@pytest.mark.parametrize("name", ["mtm", "mtstm"])
def test_forced_graph_walks_are_the_hand_written_rows(name):
    p = R.forced(PATHS[name])
    net = _net(p, np.zeros((p.total + 1, 8), np.float32), seed=3)
    assert net.dummy == p.total and net.start_count == 4 and net.type_start.tolist() == p.start.tolist()
    for step in (0, 7):
        assert np.array_equal(net.walks(np.tile(np.arange(4), 2), 5, step=step), np.tile(R.FORCED_WALKS[name], (2, 1)))
    if name == "mtm":
        net.train_batch(np.arange(4), 5, 3, 1, 0, 0.0, apply=False)
        assert np.array_equal(net.last_windows()[0], R.FORCED_WINDOWS_MTM)


@pytest.mark.parametrize("name", ["mtm", "mtstm", "stm"])
def test_walks_are_typed_follow_the_hop_csrs_and_replay_bit_for_bit(name):
    p = path(name)
    longest = WALK_NODES[name][-1]
    share = dummy_share(replayed_walks(name, longest, 1), p)
    print(f"m2v walks {name}: {share:.3f} of the replayed walks of {longest} nodes reach the dummy")
    assert 0.05 <= share <= 0.60                                   # on the reference, before any device call
    net = _net(name, np.zeros((p.total + 1, 8), np.float32))
    start = np.tile(start_nodes(name), WPN_WALKS)
    dense = [scipy.sparse.csr_matrix((np.ones(len(col), bool), col, rp), shape=(p.count[s], p.count[d])).toarray() for s, d, rp, col in p.hops]
    for nodes in WALK_NODES[name]:
        rw = net.walks(start, nodes, step=1)
        assert np.array_equal(rw, replayed_walks(name, nodes, 1))                              # bit-equal to the replay
        assert rw.shape == (len(start), nodes) and np.array_equal(rw[:, 0], p.start[p.hops[0][0]] + start)
        for s in range(1, nodes):
            hs, hd, rp, col = p.hops[(s - 1) % p.L]
            a, b = rw[:, s - 1], rw[:, s]
            real_a, real_b = a != p.total, b != p.total
            assert ((b[real_b] >= p.start[hd]) & (b[real_b] < p.start[hd + 1])).all()            # in its type's range, or the dummy
            assert (real_a | ~real_b).all()                                                    # the dummy stays
            la = a[real_a] - p.start[hs]
            deg = np.diff(rp)[la]
            assert np.array_equal(real_b[real_a], deg > 0)                                     # a dead end gives the dummy, and only a dead end does
            both = real_a & real_b
            assert dense[(s - 1) % p.L][a[both] - p.start[hs], b[both] - p.start[hd]].all()     # every real step is an edge of that hop's CSR
    assert not np.array_equal(net.walks(start, WALK_NODES[name][-1], step=2), replayed_walks(name, WALK_NODES[name][-1], 1))


def test_first_hop_from_the_hub_is_uniform():
    """the chi-square of test_device_walks_follow_edges_uniformly_and_tile_the_batch on the hub's first hop"""
    p = path("mtm")
    v = hub("mtm"); _, hd, rp, col = p.hops[0]
    deg = int(rp[v + 1] - rp[v])
    net = _net("mtm", np.zeros((p.total + 1, 8), np.float32), seed=3)
    nxt = net.walks(np.full(60 * deg, v), 2, step=1)[:, 1] - p.start[hd]
    counts = np.array([(nxt == u).sum() for u in col[rp[v]:rp[v + 1]]])
    exp = len(nxt) / deg
    assert counts.sum() == len(nxt) > 50 * deg and ((counts - exp) ** 2 / exp).sum() < 3 * deg + 20


@pytest.mark.parametrize("name", ["mtstm", "stm"])
def test_negatives_replay_bit_for_bit_in_window_row_order(name):
    p = path(name)
    nodes, ctx, wpn, nneg = WALK_NODES[name][-1], 3, 2, 3
    batch = start_nodes(name)
    net = _net(name, table(name, 9))
    net.train_batch(batch, nodes, ctx, wpn, nneg, 0.0, apply=False)
    got_pos, got_neg = net.last_windows()
    rn = R.replay_negs(p, batch, len(batch) * wpn * nneg, nodes, SEED, 0)
    assert got_neg.shape == (len(rn) * (nodes + 1 - ctx), ctx)
    for j in range(nodes + 1 - ctx):                                                       # row j * n_walks + r = nodes j .. j + ctx - 1 of walk r
        assert np.array_equal(got_neg[j * len(rn):(j + 1) * len(rn)], rn[:, j:j + ctx])
    assert (got_neg != p.total).all()
    for s in range(1, nodes):
        t = p.position_type(s)
        assert ((rn[:, s] >= p.start[t]) & (rn[:, s] < p.start[t + 1])).all()
    assert np.array_equal(got_pos, R.windows(R.replay_walks(p, batch, len(batch) * wpn, nodes, SEED, 0), ctx))


@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("d", NATIVE_SIZES)
def test_native_batches_match_float64_with_the_dummy_row(d, pairs, monkeypatch):
    """walks -> windows -> pairs, negatives -> windows -> pairs on a metapath handle, through either form of the pair kernel: loss and every gradient element inside the
    bars of tests/test_gpu_n2v_parity.py.  The dummy row is named by a sizeable share of the pairs - a wrong aggregation of its terms shows on that row."""
    p = path(NATIVE_PATH)
    W = table(NATIVE_PATH, d)
    refs = []
    for t in range(len(NATIVE_STEPS)):
        batch, rw, pos, neg = replay_step(t)
        ref = P.ref_batch(W, pos, neg)
        assert P.conditions_hold(ref) and ref["K"][p.total] > 0 and np.abs(ref["grad"][p.total]).max() > 0
        refs.append(ref)
    assert any((pos[:, 0] == p.total).any() for _, _, pos, _ in map(replay_step, range(len(NATIVE_STEPS))))      # a window that STARTS at the dummy
    net = _net(NATIVE_PATH, W, pairs=pairs, monkeypatch=monkeypatch)
    for t, (B, nodes, ctx, wpn, nneg) in enumerate(NATIVE_STEPS):
        batch, rw, pos, neg = replay_step(t)
        loss = net.train_batch(batch, nodes, ctx, wpn, nneg, 0.0, apply=False)
        got_pos, got_neg = net.last_windows()
        assert np.array_equal(got_pos, pos) and np.array_equal(got_neg, neg)
        g = net.grad()
        P.parity(loss, g, refs[t], f"m2v d={d} pairs={pairs} native step {t}")
        bar = refs[t]["bar"][p.total]
        assert g[p.total].any() and (np.abs(g[p.total] - refs[t]["grad"][p.total]) <= bar).all()
        print(f"m2v d={d} pairs={pairs} step {t}: {int(refs[t]['K'][p.total])} of {int(refs[t]['K'].sum())} terms land on the dummy row")
    assert np.array_equal(net.weight(), W)
    # injected windows may name the dummy row, as a start and as a rest node
    batch, rw, pos, neg = replay_step(0)
    loss = net.loss_on(pos, neg, apply=False)
    P.parity(loss, net.grad(), refs[0], f"m2v d={d} pairs={pairs} injected")


@pytest.mark.parametrize("pairs", [0, 1])
def test_adam_over_three_applied_native_steps(pairs, monkeypatch):
    d = 129
    W0 = table(NATIVE_PATH, d)
    sets = [replay_step(t, steps=ADAM_STEPS)[2:] for t in range(len(ADAM_STEPS))]
    Wref, refs, compare, named = P.adam_reference(W0, sets)
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs) and named[path(NATIVE_PATH).total]
    assert (~named).sum() >= 5 and all(((r["K"] > 0) != named).any() for r in refs)
    net = _net(NATIVE_PATH, W0, pairs=pairs, monkeypatch=monkeypatch)
    for t, (B, nodes, ctx, wpn, nneg) in enumerate(ADAM_STEPS):
        net.train_batch(replay_step(t, steps=ADAM_STEPS)[0], nodes, ctx, wpn, nneg, 0.01, apply=True)
        assert all(np.array_equal(x, y) for x, y in zip(net.last_windows(), sets[t]))
    Wd = net.weight()
    assert np.array_equal(Wd[~named].view(np.uint32), W0[~named].view(np.uint32))           # rows no window ever names: bit for bit
    err = np.abs(Wd - Wref); tol = 2e-5 + 1e-4 * np.abs(Wref)                               # the bars of test_adam_over_steps_that_name_different_rows
    print(f"m2v adam pairs={pairs}: max |W - ref| / tol over the compared elements {float((err / tol)[compare].max()):.3f}, left out {int((~compare).sum())} of {compare.size}")
    assert (err <= tol)[compare].all()


def test_refusals_change_nothing():
    from opentf_amd.libntf import NTF_EINVAL, MetaPath2Vec, NtfError
    p = path("mtstm")
    W = table("mtstm", 9)
    cnt, hops = [int(c) for c in p.count], [tuple(h) for h in p.hops]

    def hop(i, **kw):
        s, d, rp, col = hops[i]
        return (kw.get("s", s), kw.get("d", d), kw.get("rp", rp), kw.get("col", col))
    rp0 = hops[0][2]
    down = rp0.copy(); down[3] = down[4] + 1                                     # rowptr[4] < rowptr[3], the last entry as it was
    late = rp0.copy(); late[0] = 1                                               # does not start at 0
    wide = np.where(np.arange(len(hops[0][3])) == 5, cnt[2], hops[0][3]).astype(np.int32)     # a team id == the team count
    ring = [hops[0], hops[3]]                                                    # member -> team -> member: chains
    creates = {
        "no type": lambda: MetaPath2Vec([], [], np.zeros((1, 9), np.float32)),
        "nine types": lambda: MetaPath2Vec([4] * 9, [(0, 1, np.zeros(5, np.int64), np.zeros(0, np.int32))], np.zeros((37, 9), np.float32)),
        "no hop": lambda: MetaPath2Vec(cnt, [], W),
        "nine hops": lambda: MetaPath2Vec(cnt, (ring * 5)[:9], W),
        "broken chain": lambda: MetaPath2Vec(cnt, [hops[0], hops[2], hops[3]], W),
        "type id": lambda: MetaPath2Vec(cnt, [hop(0, d=3)], W),
        "rowptr start": lambda: MetaPath2Vec(cnt, [hop(0, rp=late)] + hops[1:], W),
        "rowptr order": lambda: MetaPath2Vec(cnt, [hop(0, rp=down)] + hops[1:], W),
        "column": lambda: MetaPath2Vec(cnt, [hop(0, col=wide)] + hops[1:], W),
        "d = 0": lambda: MetaPath2Vec(cnt, hops, np.zeros((p.total + 1, 0), np.float32)),
        "d = 257": lambda: MetaPath2Vec(cnt, hops, np.zeros((p.total + 1, 257), np.float32)),
    }
    for tag, make in creates.items():
        with pytest.raises(NtfError, match=rf"ntf_m2v_create failed \({NTF_EINVAL}\)"): make()
    MetaPath2Vec(cnt, (ring * 4)[:8], W).close()                                  # eight hops are the limit, not beyond it

    # a metapath that is no cycle: walks of more than n_hops + 1 nodes are refused, at walks and at train_batch
    ps = path("stm")
    ws = table("stm", 9)
    net = _net("stm", ws, seed=5)
    bs = start_nodes("stm")
    for call in (lambda: net.walks(bs, 4), lambda: net.train_batch(bs, 4, 3, 2, 1, 0.01), lambda: net.train_batch(bs, 9, 3, 2, 1, 0.01)):
        with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): call()
    assert net.walks(bs, 3).shape == (len(bs), 3)
    # a start id outside the start type (skill: 41 nodes; 41 is a valid ROW of the table, but not a local skill id)
    bad = bs.copy(); bad[-1] = N_SKILL
    neg1 = bs.copy(); neg1[0] = -1
    for b in (bad, neg1):
        with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): net.walks(b, 3)
        with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): net.train_batch(b, 3, 2, 2, 1, 0.01)
    badrows = np.array([[0, ps.total + 1]], np.int64)                              # the dummy row is the last one an injected window may name
    with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): net.loss_on(badrows, badrows[:0], lr=0.01, apply=True)
    assert np.array_equal(net.weight().view(np.uint32), ws.view(np.uint32)) and not net.grad().view(np.uint32).any()
    # none of the refused calls took a step index: the first accepted batch draws what step 0 draws
    net.train_batch(bs, 3, 2, 2, 1, 0.0, apply=False)
    got_pos, got_neg = net.last_windows()
    assert np.array_equal(got_pos, R.windows(R.replay_walks(ps, bs, 2 * len(bs), 3, 5, 0), 2))
    assert np.array_equal(got_neg, R.windows(R.replay_negs(ps, bs, 2 * len(bs), 3, 5, 0), 2))
    with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): net.train_batch(bad, 3, 2, 2, 1, 0.01)
    net.train_batch(bs, 3, 2, 2, 1, 0.0, apply=False)                            # ... and the next one what step 1 draws
    assert np.array_equal(net.last_windows()[0], R.windows(R.replay_walks(ps, bs, 2 * len(bs), 3, 5, 1), 2))


# ---------------------------------------------------------------------------------------------------------------- the plugin
def _toy():
    return toy_dblp()[1:]


def test_gnn_m2v_plugin_on_toy_dblp(tmp_path):
    from opentf_amd.mdl.emb.gnn import Gnn
    tv, sp, n, S, M = _toy()
    L4 = [["member", "to", "team"], ["team", "rev_to", "skill"], ["skill", "to", "team"], ["team", "rev_to", "member"]]
    cfg = Cfg(graph=Cfg(structure=[[["skill", "to", "team"], ["member", "to", "team"]], "stm"], dup_edge="add", pre=None),
              m2v=Cfg(d=16, w=3, e=4, b=8, lr=0.01, es=5, ns=2, spe=2, wl=4, wn=3, metapath_name=[L4, "mtstm"]))
    t2v = Gnn(str(tmp_path), "cuda:0", 0, cfg, "m2v")
    t2v.learn(tv, sp)
    assert os.path.basename(t2v.output) == "m2v.b8.e4.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl4.wn3.mtstm"
    n2v_keys = ["model_state_dict", "cfg", "f", "e", "t_loss", "v_loss", "node_order", "node_offsets"]      # what the n2v branch writes
    for k in range(3):
        ck = torch.load(f"{t2v.output}/f{k}.pt", map_location="cpu", weights_only=False)
        assert list(ck.keys()) == n2v_keys and list(ck["model_state_dict"].keys()) == ["embedding.weight"]
        assert ck["node_order"] == "member|skill|team|dummy" and ck["node_offsets"] == (0, M, M + S, M + S + n + 1)
        W = ck["model_state_dict"]["embedding.weight"].numpy()
        assert W.shape == (S + M + n + 1, 16) and W.dtype == np.float32 and np.isfinite(W).all() and np.isfinite(ck["t_loss"]) and np.isfinite(ck["v_loss"])
        assert os.path.exists(f"{t2v.output}/f{k}.e0.pt") and os.path.exists(f"{t2v.output}/f{k}.e1.pt") and os.path.exists(f"{t2v.output}/f{k}.e3.pt")
    # get_dense_vecs: scipy's mean pool of the SKILL block (rows M .. M + S of the last fold's table), the bar of the g9 gather test
    E = t2v.model[M:M + S]
    X = t2v.get_dense_vecs(tv, vectype="skill")
    sk = scipy.sparse.csr_matrix(tv["skill"]).astype(np.float64)
    ref = np.asarray(sk @ E.astype(np.float64)) / np.asarray(sk.sum(1))
    np.testing.assert_allclose(X, ref, rtol=1e-6, atol=1e-7)
    assert np.array_equal(tv["skill_table"], E) and t2v.get_dense_vecs(tv, "team").shape == (n, 16) and np.array_equal(t2v.get_dense_vecs({}, "member"), t2v.model[:M])
    # a second learn() loads the files instead of retraining
    stamp = os.path.getmtime(f"{t2v.output}/f0.pt")
    t2 = Gnn(str(tmp_path), "cuda:0", 0, cfg, "m2v"); t2.learn(tv, sp)
    assert os.path.getmtime(f"{t2v.output}/f0.pt") == stamp and np.array_equal(t2.model, t2v.model)
    # without the marker: accepted when the row count is total + 1 (PyG's order is the sorted type names), refused otherwise
    ck = torch.load(f"{t2v.output}/f2.pt", map_location="cpu", weights_only=False)
    full = ck["model_state_dict"]["embedding.weight"].clone()
    del ck["node_order"], ck["node_offsets"]; torch.save(ck, f"{t2v.output}/f2.pt")
    t3 = Gnn(str(tmp_path), "cuda:0", 0, cfg, "m2v"); t3.learn(tv, sp)
    assert np.array_equal(t3.model, t2v.model)
    ck["model_state_dict"]["embedding.weight"] = full[:-1].clone(); torch.save(ck, f"{t2v.output}/f2.pt")
    with pytest.raises(RuntimeError, match="without a node order marker"): Gnn(str(tmp_path), "cuda:0", 0, cfg, "m2v").learn(tv, sp)
    ck["node_order"], ck["node_offsets"] = "skill|member|team", (0, S, S + M, S + M + n); torch.save(ck, f"{t2v.output}/f2.pt")
    with pytest.raises(RuntimeError, match="node order"): Gnn(str(tmp_path), "cuda:0", 0, cfg, "m2v").learn(tv, sp)


# ---------------------------------------------------------------------------------------------------------------- learning signal
PLANTED = dict(d=16, b=8, epochs=30, lr=0.05, steps=4, context=3, walks_per_node=5, num_neg=3)
# held-out AUC of the CPU trainer of tests/m2v_reference.py (R.train), seeds 0..4, same graph and hyper-parameters
CPU_AUC = [0.7244, 0.6913, 0.6869, 0.7925, 0.6983]


@functools.lru_cache(None)
def planted():
    """4 communities of 10 members, 4 skills and 20 teams each: a team takes 3 members and 2 skills, each from its own community with probability 0.9.  One
    member edge of every second team is held out.  -> Path (member -> team -> skill -> team -> member) on the remaining graph, held-out (member, team) LOCAL
    pairs, four times as many (member, team) pairs that are no edge at all"""
    rng = np.random.default_rng(0)
    C, nm, ns, nt = 4, 10, 4, 20
    M, S, T = C * nm, C * ns, C * nt
    member = np.zeros((T, M), bool); skill = np.zeros((T, S), bool)
    for t in range(T):
        c = t // nt
        for k in range(3):
            cc = c if rng.random() < 0.9 else int(rng.integers(C))
            member[t, cc * nm + int(rng.integers(nm))] = True
        for k in range(2):
            cc = c if rng.random() < 0.9 else int(rng.integers(C))
            skill[t, cc * ns + int(rng.integers(ns))] = True
    full = member.copy()
    held = []
    for t in range(0, T, 2):
        ms = np.flatnonzero(member[t])
        if len(ms) >= 2: held.append((int(ms[0]), t)); member[t, ms[0]] = False
    held = np.array(held)
    non = np.argwhere(~full.T)
    non = non[rng.choice(len(non), 4 * len(held), replace=False)]
    p = R.Path({"member": M, "skill": S, "team": T}, R.MTSTM, R.hop_csrs(scipy.sparse.csr_matrix(skill.astype(np.uint8)), scipy.sparse.csr_matrix(member.astype(np.uint8))))
    return p, held, non


def held_out_auc(W, p, held, non):
    """P(score of a held-out member-team edge > score of a non-edge), ties half: Mann-Whitney on <e_member, e_team>"""
    W = np.asarray(W, dtype=np.float64)
    m0, t0 = p.start_of("member"), p.start_of("team")
    a = (W[m0 + held[:, 0]] * W[t0 + held[:, 1]]).sum(1); b = (W[m0 + non[:, 0]] * W[t0 + non[:, 1]]).sum(1)
    return float(((a[:, None] > b[None, :]).sum() + 0.5 * (a[:, None] == b[None, :]).sum()) / (len(a) * len(b)))


def test_m2v_learns_structure_held_out_edge_auc():
    """Held-out member-team edges of a planted-community graph against non-edges.  The CPU trainer of tests/m2v_reference.py (torch autograd, torch's generator),
    same graph and hyper-parameters (PLANTED), seeds 0..4, gives 0.7244, 0.6913, 0.6869, 0.7925, 0.6983 (CPU_AUC; the initial table: 0.444); the device must reach
    the lowest of the five minus their range, 0.6869 - 0.1056 = 0.5813."""
    p, held, non = planted()
    h = PLANTED
    lo, rng_ = min(CPU_AUC), max(CPU_AUC) - min(CPU_AUC)
    assert lo > 0.6                                                   # the reference itself learns the structure
    g = torch.Generator().manual_seed(0)
    W0 = torch.empty(p.total + 1, h["d"]).normal_(generator=g).numpy()
    assert abs(held_out_auc(W0, p, held, non) - 0.5) < 0.15           # the initial table is near chance
    net = _net(p, W0, seed=0)
    n0 = int(p.count[p.hops[0][0]])
    for e in range(h["epochs"]):
        perm = torch.randperm(n0, generator=g).numpy()
        for o in range(0, n0, h["b"]):
            net.train_batch(perm[o:o + h["b"]], h["steps"] + 1, h["context"], h["walks_per_node"], h["num_neg"], h["lr"], want_loss=False)
    auc = held_out_auc(net.weight(), p, held, non)
    print(f"m2v planted communities: device held-out AUC {auc:.4f}; CPU trainer {CPU_AUC} (bar {lo - rng_:.4f})")
    assert auc >= lo - rng_
