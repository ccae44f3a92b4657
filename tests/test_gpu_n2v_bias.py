"""node2vec's walk bias on the MI355X (ntf_n2v_set_walk_bias, k_n2v_walks_biased of opentf_amd/csrc/ntf_n2v.hip) against tests/n2v_bias_reference.py: the biased
walks replayed bit for bit from the Philox words - through the rejection stage and through the wave-cooperative scan -, their distribution against the exact
transition probabilities, the uniform route left as it was, training batches, every refusal of the contract, entry multiplicity and the `Gnn` plugin.

The replays are pure Python and are the slow part: the shapes are small, each replay is computed once (lru_cache) and left unchanged."""
import functools
import os

import numpy as np
import pytest
import torch
from scipy.stats import chi2

import n2v_bias_reference as R
import test_gpu_n2v_parity as P

pytestmark = pytest.mark.gpu

SEED = 11
G24_ROWS, G24_NODES = 600, 6          # 600 walks: two workgroups of 256 and a partial one, the last wave of which is partial too (600 = 9 * 64 + 24)


def _net(graph, d=9, seed=SEED, **kw):
    from opentf_amd.libntf import Node2Vec
    rp, col = graph
    W = torch.randn(len(rp) - 1, d, generator=torch.Generator().manual_seed(d)).mul(0.1).numpy()
    return Node2Vec(rp, col, W, seed=seed, **kw), W


@functools.lru_cache(None)
def g24_replay(p, q, step, n_walks=G24_ROWS, nodes=G24_NODES, batch=None):
    rp, col = R.g24()
    b = np.arange(24, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
    rw = R.replay_biased_walks(rp, col, b, n_walks, nodes, SEED, step, p, q)
    rw.setflags(write=False)
    return rw


# ---------------------------------------------------------------------------------------------------------------- 1. replay, G24
@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("p,q", R.SETTINGS)
def test_walks_on_g24_replay_bit_for_bit(p, q, step):
    rp, col = R.g24()
    net, _ = _net(R.g24(), p=p, q=q)
    start = np.tile(np.arange(24, dtype=np.int64), G24_ROWS // 24)
    got = net.walks(start, G24_NODES, step=step)
    want = g24_replay(p, q, step)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    deg = np.diff(rp)
    iso, leaf = np.flatnonzero(deg == 0), np.flatnonzero(deg == 1)
    assert len(iso) == 2 and len(leaf) == 1
    assert (got[np.isin(got[:, 0], iso)] == got[np.isin(got[:, 0], iso)][:, :1]).all()          # an isolated node stays
    assert (got[got[:, 0] == leaf[0], 1] == col[rp[leaf[0]]]).all()                             # the leaf takes its neighbour


# ---------------------------------------------------------------------------------------------------------------- 2. replay through the scan, H301
@functools.lru_cache(None)
def h301_replay():
    rp, col = R.h301()
    stats = {}
    rw = R.replay_biased_walks(rp, col, np.arange(1, 301, dtype=np.int64), 3000, 4, SEED, 2, 8, 8, stats=stats)
    return rw, stats


def test_walks_through_the_cooperative_scan_replay_bit_for_bit():
    """(8, 8) on the hub of 300: a candidate other than the one common neighbour is accepted once in 8, so about one hub step in nine survives 16 rejections and is
    taken by the scan of the hub's row - 5 strides of 64 with a tail of 44.  The replay's own counter says how many"""
    rw, stats = h301_replay()
    hub_scans = sum(1 for v in stats["scan_nodes"] if v == 0)
    print(f"n2v bias H301: {stats['scans']} scans ({hub_scans} of the hub row) of {stats['biased_steps']} biased steps")
    assert hub_scans >= 300
    net, _ = _net(R.h301(), p=8, q=8)
    got = net.walks(np.tile(np.arange(1, 301, dtype=np.int64), 10), 4, step=2)
    assert np.array_equal(got, rw), np.argwhere(got != rw)[:5]


# ---------------------------------------------------------------------------------------------------------------- 3. distribution, G24
@pytest.mark.parametrize("p,q", R.SETTINGS)
def test_device_walks_follow_the_exact_pair_distribution(p, q):
    """40 000 device walks of 3 nodes from the hub of G24: Pearson's chi-square of the (position 1, position 2) counts against `exact_pairs`; cells of expected count
    below 5 are left out and may hold at most 1e-3 of the mass; the bar is the 1e-6 quantile at cells - 1 degrees of freedom"""
    rp, col = R.g24()
    net, _ = _net(R.g24(), p=p, q=q)
    rw = net.walks(np.zeros(40000, dtype=np.int64), 3, step=3)
    Pm = R.exact_pairs(rp, col, 0, p, q)
    stat, cells, left = R.chi_square(rw, Pm, min_expected=5.0)
    bar = float(chi2.isf(1e-6, cells - 1))
    print(f"n2v bias distribution (p, q) = ({p}, {q}): chi-square {stat:.1f} over {cells} cells, bar {bar:.1f}, mass left out {left:.2e}")
    assert left <= 1e-3
    assert stat <= bar


# ---------------------------------------------------------------------------------------------------------------- 4. uniform untouched
def test_p_q_one_is_the_uniform_walk_bit_for_bit():
    """an untouched handle, one set to (1, 1), and one set to (4, 1) and back: k_n2v_walks' walks (`replay_walks` of test_gpu_n2v_parity.py), its windows, and the
    same table after two applied batches.  The tables are compared on batches of ONE positive and ONE negative window row: one wave a launch, so the f32 atomic
    adds of the gradient land in program order and two handles agree to the bit (with several waves a launch their order is nobody's: test_gpu_n2v_sparse.py)."""
    from opentf_amd.libntf import Node2Vec
    rp, col, nn, _ = P.graph()
    W = P.table(65)
    def make(kind):
        net = Node2Vec(rp, col, W, seed=P.NATIVE_SEED)
        if kind == "one": net.set_walk_bias(1, 1)
        if kind == "back": net.set_walk_bias(4, 1); net.set_walk_bias(1.0, 1.0)
        return net
    nets = [make(k) for k in ("untouched", "one", "back")]
    B, wl, ctx, wpn, nneg = P.NATIVE_STEPS[0]
    batch, rw, pos, neg = P.replay_step(0)
    for net in nets:
        assert np.array_equal(net.walks(np.tile(batch, wpn), wl, step=0), rw)
        net.train_batch(batch, wl, ctx, wpn, nneg, 0.0, apply=False)                      # call 0 of the handle: the windows of step 0
        gp, gn = net.last_windows()
        assert np.array_equal(gp, pos) and np.array_equal(gn, neg)
        net.grad()                                                                        # consumed: nothing pending
    hub = np.array([P.graph()[3]["hub"]], dtype=np.int64)
    tables, windows = [], []
    for net in nets:
        for t in (1, 2):                                                                  # calls 1 and 2: one walk of 5 nodes in one window, one negative row
            net.train_batch(hub, 5, 5, 1, 1, 0.01, apply=True)
            windows.append(net.last_windows())
            want = P.replay_walks(rp, col, hub, 1, 5, P.NATIVE_SEED, t)
            assert np.array_equal(windows[-1][0], want) and np.array_equal(windows[-1][1], P.replay_negs(hub, 1, 5, nn, P.NATIVE_SEED, t))
        tables.append(net.weight())
    assert (tables[0].view(np.uint32) != W.view(np.uint32)).any()
    for T in tables[1:]: assert np.array_equal(T.view(np.uint32), tables[0].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 5. training
TRAIN = dict(d=9, B=7, wl=5, w=3, wn=2, ns=2, p=0.25, q=4.0)


@functools.lru_cache(None)
def train_replay(t):
    rp, col = R.g24()
    c = TRAIN
    batch = np.random.default_rng(20 + t).choice(24, c["B"], replace=False).astype(np.int64)
    rw = R.replay_biased_walks(rp, col, batch, c["B"] * c["wn"], c["wl"], SEED, t, c["p"], c["q"])
    pos = P.N.windows(torch.from_numpy(rw), c["w"]).numpy()
    neg = P.N.windows(torch.from_numpy(P.replay_negs(batch, c["B"] * c["wn"] * c["ns"], c["wl"], 24, SEED, t)), c["w"]).numpy()
    return batch, pos, neg


@pytest.mark.parametrize("sparse", [False, True])
def test_training_batches_walk_biased_and_leave_the_negatives_alone(sparse):
    c = TRAIN
    net, W = _net(R.g24(), d=c["d"], sparse=sparse, p=c["p"], q=c["q"])
    for t in range(3):
        batch, pos, neg = train_replay(t)
        loss = net.train_batch(batch, c["wl"], c["w"], c["wn"], c["ns"], 0.01)
        gp, gn = net.last_windows()
        assert np.array_equal(gp, pos) and np.array_equal(gn, neg) and gp.shape == (c["B"] * c["wn"] * (c["wl"] + 1 - c["w"]), c["w"])
        assert np.isfinite(loss)
    Wd = net.weight()
    assert np.isfinite(Wd).all() and (Wd != W).any()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_change_nothing():
    from opentf_amd.libntf import NTF_EINVAL, NTF_ESTATE, Node2Vec, NtfError
    import test_gpu_m2v as M
    start = np.tile(np.arange(24, dtype=np.int64), G24_ROWS // 24)
    net, _ = _net(R.g24(), p=4, q=1)
    want = g24_replay(4, 1, 0)
    assert np.array_equal(net.walks(start, G24_NODES, step=0), want)
    c = TRAIN
    def call(t):          # call t of the handle draws what step t draws: the step index has not moved
        batch = train_replay(t)[0]
        net.train_batch(batch, c["wl"], c["w"], c["wn"], c["ns"], 0.0, apply=False)
        rw = R.replay_biased_walks(*R.g24(), batch, c["B"] * c["wn"], c["wl"], SEED, t, 4, 1)
        assert np.array_equal(net.last_windows()[0], P.N.windows(torch.from_numpy(rw), c["w"]).numpy())
    call(0)
    bad = [0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-5, 1e5, 0.99e-4, 1.01e4]
    for v in bad:
        for p, q in ((v, 2.0), (2.0, v), (v, v)):
            with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:"): net.set_walk_bias(p, q)
            assert (net.p, net.q) == (4.0, 1.0)
        assert np.array_equal(net.walks(start, G24_NODES, step=0), want)
    call(1)
    net.set_walk_bias(1e-4, 1e4); net.set_walk_bias(1e4, 1e-4); net.set_walk_bias(4, 1)          # the ends of the range are inside it
    assert np.array_equal(net.walks(start, G24_NODES, step=0), want)
    # a metapath handle has no p / q
    m2v = M._net(M.NATIVE_PATH, M.table(M.NATIVE_PATH, 9))
    before = m2v.walks(M.start_nodes(M.NATIVE_PATH), 5, step=1)
    with pytest.raises(NtfError, match=f"error {NTF_ESTATE}:"): m2v.set_walk_bias(0.5, 2.0)
    with pytest.raises(NtfError, match=f"error {NTF_ESTATE}:"): m2v.set_walk_bias(1.0, 1.0)
    assert np.array_equal(m2v.walks(M.start_nodes(M.NATIVE_PATH), 5, step=1), before)
    # one descending row: refused, the message names the ordering, and the handle goes on working unbiased
    rp, col = R.g24()
    down = col.copy(); a = int(rp[6]); down[a], down[a + 1] = col[a + 1], col[a]
    assert down[a] > down[a + 1]
    plain, _ = _net((rp, down))
    uniform = P.replay_walks(rp, down, np.arange(24), G24_ROWS, G24_NODES, SEED, 0)
    for _ in range(2):          # the second call answers from the cached check
        with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:.*ascending"): plain.set_walk_bias(0.5, 2.0)
        assert np.array_equal(plain.walks(start, G24_NODES, step=0), uniform)
    plain.set_walk_bias(1, 1)
    with pytest.raises(NtfError, match=f"error {NTF_EINVAL}:.*ascending"): Node2Vec(rp, down, np.zeros((24, 4), np.float32), p=0.5, q=2.0)
    # a descending pair ACROSS a row boundary is no disorder: G24's own CSR has them and is accepted
    assert any(col[rp[i + 1] - 1] > col[rp[i + 1]] for i in range(23) if rp[i + 1] > rp[i] and rp[i + 2] > rp[i + 1])


# ---------------------------------------------------------------------------------------------------------------- 7. multiplicity, D4
@pytest.mark.parametrize("p,q", [(2, 4), (8, 8)])
def test_a_repeated_entry_counts_once_per_entry(p, q):
    rp, col = R.d4()
    net, _ = _net(R.d4(), p=p, q=q)
    start = np.tile(np.arange(4, dtype=np.int64), 100)
    want = R.replay_biased_walks(rp, col, np.arange(4), 400, 5, SEED, 1, p, q)
    assert np.array_equal(net.walks(start, 5, step=1), want)


# ---------------------------------------------------------------------------------------------------------------- 8. the plugin
def test_plugin_trains_a_biased_table_into_its_own_directory(tmp_path):
    import test_gpu_m2v as M
    from opentf_amd.mdl.emb.gnn import Gnn
    tv, sp, n, S, Mm = M._toy()
    tables = {}
    rng_state = torch.get_rng_state()
    for tag, kw in (("biased", dict(p=0.5, q=2.0)), ("plain", {})):
        section = M.Cfg(d=16, w=3, e=2, b=8, lr=0.01, es=5, ns=2, spe=2, wl=4, wn=3, **kw)
        cfg = M.Cfg(graph=M.Cfg(structure=[[["skill", "to", "team"], ["member", "to", "team"]], "stm"], dup_edge="add", pre=None), n2v=section)
        torch.manual_seed(0)
        t2v = Gnn(str(tmp_path / tag), "cuda:0", 0, cfg, "n2v")
        t2v.learn(tv, sp)
        assert os.path.basename(t2v.output) == "n2v.b8.e2.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl4.wn3" + (".p0.5.q2.0" if kw else "")
        ck = torch.load(f"{t2v.output}/f0.pt", map_location="cpu", weights_only=False)
        W = ck["model_state_dict"]["embedding.weight"].numpy()
        assert W.shape == (S + Mm + n, 16) and np.isfinite(W).all() and np.isfinite(ck["t_loss"]) and np.isfinite(ck["v_loss"])
        tables[tag] = W
    torch.set_rng_state(rng_state)
    assert np.abs(tables["biased"] - tables["plain"]).max() > 1e-4
