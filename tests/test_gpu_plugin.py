"""The plugin mirror (opentf_amd.mdl.{fnn,bnn,tntf}, emb.t2v) end to end on a real MI355X: the reference's own
`Fnn.learn` / `Fnn.test` runs on toy dblp (golden g5, produced by importing the reference) must be reproduced —
same seed, same initial weights, same batch order — and every file the reference writes must appear with the
reference's keys and layouts.  Plus size-independent properties at BASELINE.json's full config-2 size."""
import json
import os
import pickle

import numpy as np
import pytest
import scipy.sparse
import torch

from conftest import GOLDEN, golden
from oracle import ntf_oracle as O

pytestmark = pytest.mark.gpu


class Cfg(dict):
    """attribute-dict standing in for an omegaconf DictConfig (missing keys read as None, like optional yaml keys)"""
    def __getattr__(self, k):
        if k.startswith("__"): raise AttributeError(k)
        return self.get(k)


def _toy(name):
    toy = golden(f"toy_{name}")
    n, S, M = [int(v) for v in toy["shape"]]
    skill = scipy.sparse.csr_matrix((np.ones(len(toy["skill_indices"]), np.uint8), toy["skill_indices"], toy["skill_indptr"]), shape=(n, S)).tolil()
    member = scipy.sparse.csr_matrix((np.ones(len(toy["member_indices"]), np.uint8), toy["member_indices"], toy["member_indptr"]), shape=(n, M)).tolil()
    splits = {"test": toy["test"], "folds": {k: {"train": toy[f"train{k}"], "valid": toy[f"valid{k}"]} for k in range(3)}}
    return {"skill": skill, "member": member, "loc": None}, splits


class Scalars:
    rows = []
    def __init__(self, log_dir=None): pass
    def add_scalar(self, tag, scalar_value, global_step): Scalars.rows.append((tag, float(scalar_value), int(global_step)))
    def close(self): pass


@pytest.mark.parametrize("nsd", ["None", "uniform", "unigram", "unigram_b"])
def test_learn_and_test_reproduce_the_reference_run(nsd, tmp_path):
    from opentf_amd.mdl.fnn import Fnn
    g = golden(f"g5_learn_dblp_{nsd}")
    cfg = Cfg(json.loads(str(g["cfg"])))
    tv, splits = _toy("dblp")
    m = Fnn(str(tmp_path), "cuda:0", 0, cfg)
    Scalars.rows = []
    m.writer = Scalars
    m.learn(tv, splits, None)
    ref = json.loads(str(g["scalars"]))
    assert [(t, s) for t, _, s in Scalars.rows][:6] == [(t, s) for t, _, s in ref][:6]
    if nsd == "None":
        # no sampled negatives: nothing random beyond init + batch order, which are reproduced -> the whole trajectory matches
        assert len(Scalars.rows) == len(ref)
        np.testing.assert_allclose([v for _, v, _ in Scalars.rows], [v for _, v, _ in ref], rtol=5e-5)
    else:
        # native samplers draw different negatives than torch's CPU stream: first-epoch losses agree to sampling noise only
        first = {t: v for t, v, s in Scalars.rows if s == 0}
        for t, v, s in ref:
            if s == 0: assert abs(first[t] - v) < 0.1 * abs(v), (t, first[t], v)
    for k in range(3):
        ck = torch.load(f"{m.output}/f{k}.pt", map_location="cpu", weights_only=False)
        assert list(ck.keys()) == ["model_state_dict", "cfg", "f", "e", "t_loss", "v_loss"] and ck["f"] == k
        assert list(ck["model_state_dict"].keys()) == [n[len(f"f{k}."):] for n in g.files if n.startswith(f"f{k}.layers.")]
        if nsd == "None":
            assert ck["e"] == int(g[f"f{k}.e"])
            for name, v in ck["model_state_dict"].items():
                assert v.dtype == torch.float32 and not v.is_cuda
                np.testing.assert_allclose(v.numpy(), g[f"f{k}.{name}"], rtol=2e-3, atol=2e-5)
    m.test(tv, splits, Cfg(per_epoch=False, on_train=False, topK=None))
    for k in range(3):
        pr = torch.load(f"{m.output}/f{k}.test.pred", map_location="cpu", weights_only=False)
        assert list(pr.keys()) == ["y_pred", "uncertainty"] and pr["uncertainty"] is None
        assert tuple(pr["y_pred"].shape) == g[f"f{k}.y_pred"].shape and pr["y_pred"].dtype == torch.float32
        if nsd == "None":
            np.testing.assert_allclose(pr["y_pred"].numpy(), g[f"f{k}.y_pred"], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("weights", [(3, 0.5), None], ids=["tpw3-tnw0.5", "absent"])
def test_learn_hands_the_loss_weights_and_ns_to_the_engine(weights, tmp_path):
    """tpw, tnw and ns of the model's config reach ntf_engine_create as they stand; a config without tpw / tnw trains at 1 and 1"""
    from opentf_amd import libntf
    from opentf_amd.mdl.fnn import Fnn
    cfg = Cfg(b=5, e=1, ns=9, lr=0.01, es=2, h=[16], spe=0, l="bce", nsd="uniform")
    if weights: cfg.update(tpw=weights[0], tnw=weights[1])
    tv, splits = _toy("dblp")
    seen = []
    orig = libntf.Engine.__init__
    def spy(self, dims, *a, **k):
        seen.append((k.get("tpw"), k.get("tnw"), k.get("ns")))
        return orig(self, dims, *a, **k)
    libntf.Engine.__init__ = spy
    try:
        m = Fnn(str(tmp_path), "cuda:0", 0, cfg)
        m.writer = Scalars
        m.learn(tv, splits, None)
    finally:
        libntf.Engine.__init__ = orig
    assert seen and all(s == ((3.0, 0.5, 9) if weights else (1.0, 1.0, 9)) for s in seen), seen
    ck = torch.load(f"{m.output}/f0.pt", map_location="cpu", weights_only=False)
    assert np.isfinite(ck["t_loss"]) and np.isfinite(ck["v_loss"])


def test_bnn_files_layout_topk_and_per_epoch(tmp_path):
    from opentf_amd.mdl.bnn import Bnn
    lay = json.load(open(os.path.join(GOLDEN, "g8_layout.json")))
    ref = next(v for k, v in lay.items() if k.startswith("bnn."))
    tv, splits = _toy("dblp")
    cfg = Cfg(b=6, e=3, ns=3, lr=0.01, es=5, h=[128], spe=2, l="bce", tpw=10, tnw=1, nsd="unigram_b", nmc=4)
    m = Bnn(str(tmp_path), "cuda", 0, cfg)
    assert m.output.endswith("/bnn.b6.e3.ns3.lr0.01.es5.h[128].spe2.lbce.tpw10.tnw1.nsdunigram_b.nmc4")
    m.learn(tv, splits, None)
    assert sorted(f for f in os.listdir(m.output) if f.endswith(".pt")) == sorted([f"f{k}.pt" for k in range(3)] + [f"f{k}.e{e}.pt" for k in range(3) for e in (0, 1)])
    ck = torch.load(f"{m.output}/f0.pt", map_location="cpu", weights_only=False)
    assert ck["cfg"] == cfg and list(ck.keys()) == ref["ckpt_keys"]
    assert {k: [list(v.shape), str(v.dtype)] for k, v in ck["model_state_dict"].items()} == ref["state"]  # committed reference checkpoint layout
    m.test(tv, splits, Cfg(per_epoch=True, on_train=True, topK=5))
    M = tv["member"].shape[1]
    for ps, rows in [("test", splits["test"]), ("train", splits["folds"][0]["train"]), ("valid", splits["folds"][0]["valid"])]:
        for ep in ["", "e0.", "e1."]:
            pr = torch.load(f"{m.output}/f0.{ps}.{ep}pred", map_location="cpu", weights_only=False)
            yp = pr["y_pred"]
            assert yp.is_sparse and yp.is_coalesced() and tuple(yp.shape) == (len(rows), M) and yp._nnz() == len(rows) * 5
            dense = yp.to_dense().numpy()
            assert ((dense > 0).sum(1) == 5).all() and dense.max() <= 1.0
            unc = pr["uncertainty"]
            assert set(unc) == {"pred", "model"} and len(unc["pred"]) == 1 and unc["pred"][0].dtype == np.float32
            assert unc["pred"][0].shape == (len(rows) % 6 or 6,)  # only the LAST batch's uncertainties survive (fnn.py:203 quirk)
            assert (unc["model"][0] > -1e-3).all()  # mutual information is non-negative up to rounding


def test_temporal_streaming_warm_start(tmp_path):
    from opentf_amd.mdl.fnn import Fnn
    from opentf_amd.mdl.tntf import tNtf
    tv, splits = _toy("dblp")
    cfg = Cfg(b=4, e=2, ns=2, lr=0.01, es=5, h=[16], spe=0, l="bce", tpw=10, tnw=1, nsd="uniform")
    inner = Fnn(str(tmp_path), "cuda:0", 0, cfg)
    year_idx = [(0, 2000), (9, 2001), (18, 2002), (26, 2003)]  # 31 teams sorted by year; the last interval is the test set
    t = tNtf(str(tmp_path), "cuda:0", 0, Cfg(tfolds=3, step_ahead=1), inner, year_idx)
    sp = {"test": np.arange(26, 31), "folds": {k: {} for k in range(3)}}
    t.learn(tv, sp, None)
    out = t.output
    assert sorted(d for d in os.listdir(out) if d.isdigit()) == ["2000", "2001", "2002"]
    for y in ["2000", "2001", "2002"]:
        assert all(os.path.exists(f"{out}/{y}/f{k}.pt") for k in range(3)) and os.path.exists(f"{out}/{y}/splits.pkl")
    s01 = pickle.load(open(f"{out}/2001/splits.pkl", "rb"))
    assert set(np.concatenate([s01["folds"][0]["train"], s01["folds"][0]["valid"]])) == set(range(9, 18))
    # warm start: 2001's training began from 2000's weights, so its first-epoch weights differ from a cold init
    w0 = torch.load(f"{out}/2000/f0.pt", weights_only=False)["model_state_dict"]["layers.0.weight"]
    w1 = torch.load(f"{out}/2001/f0.pt", weights_only=False)["model_state_dict"]["layers.0.weight"]
    assert (w0 - w1).abs().max() < 0.2 and not torch.equal(w0, w1)
    t.test(tv, sp, Cfg(per_epoch=False, on_train=False, topK=None))
    assert os.path.exists(f"{inner.output}/f0.test.pred")


def test_tntf_reproduces_the_reference_tntf_run(tmp_path):
    """g13 = the reference's own mdl.tntf.tNtf around its own mdl.fnn.Fnn (nsd=None) on toy dblp, run by tests/golden/make_golden_tntf.py:
    same year directories, same per-interval K-fold splits, same early-stop epochs, loss series, warm-started weights of every
    interval and fold, and the same test predictions from the last interval's models."""
    from opentf_amd.mdl.fnn import Fnn
    from opentf_amd.mdl.tntf import tNtf
    g = golden("g13_tntf_dblp")
    cfg = Cfg(json.loads(str(g["cfg"])))
    tv, _ = _toy("dblp")
    seed = int(g["seed"])
    year_idx = [(int(a), int(b)) for a, b in g["i2y"]]
    inner = Fnn(str(tmp_path), "cuda:0", seed, cfg)
    assert inner.name() == str(g["root_name"])
    t = tNtf(str(tmp_path), "cuda:0", seed, Cfg(tfolds=int(g["tfolds"]), step_ahead=int(g["step_ahead"])), inner, year_idx)
    sp = {"test": g["test"], "folds": {k: {} for k in range(int(g["tfolds"]))}}
    Scalars.rows = []
    inner.writer = Scalars
    t.learn(tv, sp, None)
    years = [int(y) for y in g["years"]]
    assert sorted(int(d) for d in os.listdir(t.output) if d.isdigit()) == years
    assert os.path.relpath(inner.output, t.output) == str(g["last_output_suffix"])
    ref = json.loads(str(g["scalars"]))
    assert [(a, c) for a, _, c in Scalars.rows] == [(a, c) for a, _, c in ref]          # same epochs per interval and fold (early stopping)
    np.testing.assert_allclose([v for _, v, _ in Scalars.rows], [v for _, v, _ in ref], rtol=1e-4)
    for y in years:
        s = pickle.load(open(f"{t.output}/{y}/splits.pkl", "rb"))
        assert np.array_equal(s["test"], g["test"])
        for k in range(3):
            assert np.array_equal(s["folds"][k]["train"], g[f"{y}.train{k}"]) and np.array_equal(s["folds"][k]["valid"], g[f"{y}.valid{k}"])
            ck = torch.load(f"{t.output}/{y}/f{k}.pt", map_location="cpu", weights_only=False)
            assert ck["e"] == int(g[f"{y}.f{k}.e"])
            for name, v in ck["model_state_dict"].items():
                np.testing.assert_allclose(v.numpy(), g[f"{y}.f{k}.{name}"], rtol=2e-3, atol=2e-5)
    t.test(tv, sp, Cfg(per_epoch=False, on_train=False, topK=None))
    for k in range(3):
        pr = torch.load(f"{inner.output}/f{k}.test.pred", map_location="cpu", weights_only=False)
        np.testing.assert_allclose(pr["y_pred"].numpy(), g[f"test.f{k}.y_pred"], rtol=1e-3, atol=1e-5)
    # resume (tntf.py:22-26): a directory that already holds the five years trains nothing more and rewrites nothing
    stamp = {y: os.path.getmtime(f"{t.output}/{y}/f0.pt") for y in years[:-1]}
    inner.output = t.output
    t.learn(tv, sp, None)
    assert all(os.path.getmtime(f"{t.output}/{y}/f0.pt") == stamp[y] for y in years[:-1])


def test_table_t2v_get_dense_vecs_and_meanpool_training(tmp_path):
    from opentf_amd.mdl.emb.t2v import TableT2v
    from opentf_amd.mdl.fnn import Fnn
    g = golden("g9_gather_dblp")
    tv, splits = _toy("dblp")
    t2v = TableT2v(str(tmp_path / "emb"), "cuda:0", 0, Cfg(), "n2v").set_table(g["table"])
    X = t2v.get_dense_vecs(tv, vectype="skill")
    np.testing.assert_allclose(X, g["X"], rtol=1e-6, atol=1e-7)  # the reference expression of gnn.py:485 (golden)
    assert X.shape == (31, 128) and t2v.get_dense_vecs({}, "skill") is t2v.model
    # dense-input mode (what main.py:148-153 hands over) and in-step gather mode give the same training trajectory
    cfg = Cfg(b=8, e=2, ns=0, lr=0.01, es=5, h=[32], spe=0, l="bce", tpw=10, tnw=1, nsd=None)
    a = Fnn(str(tmp_path / "a"), "cuda:0", 3, cfg); a.learn({"skill": X, "member": tv["member"], "original_skill": tv["skill"]}, splits, None)
    b = Fnn(str(tmp_path / "b"), "cuda:0", 3, cfg); b.learn({"skill": X, "member": tv["member"], "original_skill": tv["skill"], "skill_table": g["table"]}, splits, None)
    wa = torch.load(f"{a.output}/f1.pt", weights_only=False)["model_state_dict"]
    wb = torch.load(f"{b.output}/f1.pt", weights_only=False)["model_state_dict"]
    assert all(torch.equal(wa[k], wb[k]) for k in wa)


# --------------------------------------------------------------------------------- full-size properties (config 2)
def test_full_size_fused_equals_generic_path():
    """BASELINE config 2 shapes (M = 233 629 experts, B = 1000, d = H = 128, Bnn, uniform ns=5): the fused MFMA kernels and
    the unfused GEMM + dense-loss path are independent implementations; with the same device seeds they draw the same
    eps / signs / negatives, so loss and every gradient must agree."""
    from opentf_amd import libntf
    from opentf_amd.synth import init_params, zipf_csr
    M, S, N, B = 233_629, 90_671, 50_000, 1000
    s_ip, s_ix = zipf_csr(N, S, 8.57, 1); m_ip, m_ix = zipf_csr(N, M, 3.06, 2)
    table = np.random.default_rng(0).standard_normal((S, 128), dtype=np.float32)
    sd = init_params([128, 128, M], True, 0)
    rows = np.random.default_rng(1).integers(0, N, B)
    res = []
    for fused in (True, False):
        e = libntf.Engine([128, 128, M], bayesian=True, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd="uniform", seed=99, fused=fused)
        e.set_skill_table(table); e.set_skill_csr((s_ip, s_ix)); e.set_member((m_ip, m_ix)); e.load_state_dict(sd)
        ev = e.eval_step(rows); e.set_seed(99, 0)
        loss = e.backward(rows)
        res.append((ev, loss, e.grads()))
        e.close()
    (ev_f, l_f, g_f), (ev_g, l_g, g_g) = res
    assert abs(ev_f - ev_g) <= 2e-6 * abs(ev_g) and abs(l_f - l_g) <= 2e-6 * abs(l_g)
    assert 0.6 * M < l_f < 0.8 * M  # ~ M * softplus(~0) per team at initialisation
    # leaky_relu' jumps 0.01 -> 1 at z = 0: of the 2.3e8 pre-activations per step a handful (~|z| < 1e-7) land on opposite
    # sides of the kink in the two summation orders and move one expert's gradient row by (1-0.01)*sigmoid/B*h.  Those rows
    # are counted and bounded; everything else must agree to rounding.
    for k in g_g:
        scale = np.abs(g_g[k]).max()
        d = np.abs(g_f[k] - g_g[k])
        outliers = d > 2e-5 * scale
        assert outliers.sum() <= 64 * 128, (k, int(outliers.sum()))
        assert d.max() <= 2e-2 * scale, (k, float(d.max()), float(scale))
        assert abs(float(g_f[k].astype(np.float64).sum()) - float(g_g[k].astype(np.float64).sum())) <= 1e-3 * np.abs(g_g[k]).astype(np.float64).sum()


def test_full_size_gather_properties():
    """Whole-dataset gather at dblp size: a constant table pools to the constant; pooling is linear in the table."""
    from opentf_amd import libntf
    from opentf_amd.synth import zipf_csr
    N, S, d = 1_995_708, 90_671, 128
    ip, ix = zipf_csr(N, S, 8.57, 1)
    rng = np.random.default_rng(0)
    T1, T2 = rng.standard_normal((S, d), dtype=np.float32), rng.standard_normal((S, d), dtype=np.float32)
    e = libntf.Engine([d, 1, 1], input_mode=libntf.INPUT_MEANPOOL, max_batch=1, ns=0, nsd=None)
    e.set_skill_csr((ip, ix))
    e.set_skill_table(np.full((S, d), 0.25, np.float32)); X = e.gather_meanpool(n=N)
    assert X.shape == (N, d) and np.abs(X - 0.25).max() < 1e-6
    e.set_skill_table(T1); A = e.gather_meanpool(n=N)
    e.set_skill_table(T2); Bm = e.gather_meanpool(n=N)
    e.set_skill_table(T1 + T2); C = e.gather_meanpool(n=N)
    assert np.abs(C - (A + Bm)).max() < 1e-4
    sample = rng.integers(0, N, 2000)
    assert np.array_equal(A[sample], O.gather_meanpool_fast(ip, ix, T1, sample))  # bit-exact vs the oracle on a sample


def test_pipelined_data_parallel_step_on_rccl_world1():
    """The data-parallel step as the N-GPU bench runs it — deferred dW in expert chunks, asynchronous RCCL all-reduce of each chunk
    on the engine-owned gradient buffer, then Adam — exercised on one GPU (world_size 1, the collective forced): it must leave
    exactly the parameters of the plain single-GPU step."""
    import socket
    import torch.distributed as dist
    from opentf_amd import libntf
    from opentf_amd.dp import DataParallel
    from opentf_amd.synth import init_params, zipf_csr
    M, S, N, B = 140_000, 5_000, 20_000, 600     # 3 expert chunks of 65 536
    s_ip, s_ix = zipf_csr(N, S, 8.57, 1); m_ip, m_ix = zipf_csr(N, M, 3.06, 2)
    table = np.random.default_rng(0).standard_normal((S, 128), dtype=np.float32)
    sd = init_params([128, 128, M], True, 0)
    order = np.random.default_rng(1).integers(0, N, 3 * B)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    os.environ["NTF_DP_FORCE_ALLREDUCE"] = "1"
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        stream = torch.cuda.Stream()
        results = []
        with torch.cuda.stream(stream):
            for mode in ("plain", "pipelined", "pipelined_allreduce", "pipelined_ranges"):
                # "pipelined_ranges" (round 5, the default of a sharded-optimiser run): the operand producer and the forward kernel run range by range behind their own
                # parameter all-gathers (ntf_step_staged_deferred_cb); the first two pipelined modes keep round 4's step (NTF_DP_RANGES=0: every all-gather waited for first)
                os.environ["NTF_DP_RANGES"] = "1" if mode == "pipelined_ranges" else "0"
                e = libntf.Engine([128, 128, M], bayesian=True, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd="uniform", seed=5,
                                  stream=stream.cuda_stream)
                e.set_skill_table(table); e.set_skill_csr((s_ip, s_ix)); e.set_member((m_ip, m_ix)); e.load_state_dict(sd)
                if mode == "plain":
                    loss = e.train_epoch(order, B)
                else:
                    # default: reduce-scatter -> Adam on the owned shard -> all-gather of parameters; "_allreduce": all-reduce + replicated Adam
                    dp = DataParallel(e, shard_optimizer=(mode != "pipelined_allreduce"))
                    assert dp.force_allreduce and dp.n_chunks == 3 and len(dp._rest) == 3 and dp.shard == (mode != "pipelined_allreduce")
                    assert e.fwd_ranges(B) == ([(0, 1), (1, 2), (2, 3)] if mode == "pipelined_ranges" else [])
                    loss = dp.train_epoch(order, B)
                    assert not dp._pending_chunk and not dp._pending
                results.append((loss, e.state_dict()))
                e.close()
        (la, pa) = results[0]
        for lb, pb in results[1:3]:
            assert abs(la - lb) <= 1e-6 * abs(la)
            for k in pa:
                assert np.array_equal(pa[k], pb[k]), k
        # range by range the forward kernel's column groups partition the experts differently: d(hidden) sums its partials in another order - the same step to rounding
        lb, pb = results[3]
        assert abs(la - lb) <= 2e-6 * abs(la), (la, lb)
        for k in pa:
            tol = 2e-5 * float(np.abs(pa[k]).max()) + 1e-9
            assert float((np.abs(pa[k] - pb[k]) > tol).mean()) <= 2e-4, (k, float(np.abs(pa[k] - pb[k]).max()), tol)      # (Adam's first steps: an update can flip where |g| ~ 1e-8)
    finally:
        dist.destroy_process_group()
        os.environ.pop("NTF_DP_FORCE_ALLREDUCE", None); os.environ.pop("NTF_DP_RANGES", None)


@pytest.mark.parametrize("side", ["1", "0"])
def test_deferred_step_joins_its_side_stream_for_whoever_reads_first(side, monkeypatch):
    """Round 5: a deferred-dW step (ntf_step_staged_deferred, a data-parallel rank's) runs its hidden layers' backward and loss reduction on the side stream, beside the dW
    chunks the caller launches next; the join follows the LAST ntf_dw_chunk - or whatever reads the gradients / the loss first.  Gradients read (a) right behind the deferred
    call with NO chunk launched (hidden layers: the reader joins), (b) behind the last chunk, and (c) after abandoning the chunks and stepping again, are those of the plain
    backward of the same batch, bit for bit; the epoch loss accumulates the same sum.  NTF_DP_SIDE_BWD=0 keeps round 4's order on one stream."""
    from opentf_amd import libntf
    from opentf_amd.synth import init_params, zipf_csr
    monkeypatch.setenv("NTF_DP_SIDE_BWD", side)
    M, S, N, B = 140_000, 3_000, 6_000, 500     # 3 expert chunks of 65 536
    s_ip, s_ix = zipf_csr(N, S, 8.57, 1); m_ip, m_ix = zipf_csr(N, M, 3.06, 2)
    table = np.random.default_rng(0).standard_normal((S, 128), dtype=np.float32)
    sd = init_params([128, 128, M], True, 0)
    order = np.random.default_rng(1).integers(0, N, 2 * B)

    def mk():
        e = libntf.Engine([128, 128, M], bayesian=True, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd="uniform", seed=5, fuse_adam=0)
        e.set_skill_table(table); e.set_skill_csr((s_ip, s_ix)); e.set_member((m_ip, m_ix)); e.load_state_dict(sd)
        e.stage_order(order); e.epoch_loss()
        return e
    ref = mk()
    ref.step_staged(0, B, train=True, apply=False); g_ref = ref.grads(); l_ref, _ = ref.epoch_loss()
    ref.step_staged(B, B, train=True, apply=False); g_ref2 = ref.grads(); ref.close()
    hidden = [k for k in g_ref if k.startswith("layers.0.")]

    e = mk()
    assert e.dw_chunks() == 3
    e.step_staged_deferred(0, B, 0, B)
    g = e.grads()                                       # (a) no chunk launched: the reader joins the side stream
    for k in hidden: assert np.array_equal(g[k], g_ref[k]), k
    for k in range(3): e.dw_chunk(k)
    g = e.grads()                                       # (b) behind the last chunk: every gradient
    for k in g_ref: assert np.array_equal(g[k], g_ref[k]), k
    l, steps = e.epoch_loss()
    assert steps == 1 and l == l_ref
    e.step_staged_deferred(0, B, 0, B)                  # (c) abandoned: the next step orders itself behind the chain that is still running
    e.set_seed(5, 1)                                    # (the reference's second step drew with step index 1)
    e.step_staged_deferred(B, B, B, B)
    for k in range(3): e.dw_chunk(k)
    g = e.grads()
    for k in g_ref2: assert np.array_equal(g[k], g_ref2[k]), k
    e.close()


def test_expert_parallel_step_on_rccl_world1():
    """The expert-sharded step as the N-GPU bench runs it - phase 1, RCCL all-reduce of the engine-owned d(hidden) buffer on the engine's stream,
    phase 2, the epoch-end gather of the output layer - exercised on one GPU (world_size 1: the shard is the whole layer, the collective forced):
    it must leave exactly the parameters of the plain single-GPU step."""
    import socket
    import torch.distributed as dist
    from opentf_amd import libntf
    from opentf_amd.ep import ExpertParallel, expert_shards
    from opentf_amd.synth import init_params, zipf_csr
    M, S, N, B = 70_000, 5_000, 20_000, 600
    s_ip, s_ix = zipf_csr(N, S, 8.57, 1); m_ip, m_ix = zipf_csr(N, M, 3.06, 2)
    table = np.random.default_rng(0).standard_normal((S, 128), dtype=np.float32)
    sd = init_params([128, 128, M], True, 0)
    order = np.random.default_rng(1).integers(0, N, 3 * B)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    os.environ["NTF_EP_FORCE_EXCHANGE"] = "1"
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        stream = torch.cuda.Stream()
        results = []
        with torch.cuda.stream(stream):
            for mode in ("plain", "ep"):
                e = libntf.Engine([128, 128, M], bayesian=True, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd="uniform", seed=5, fuse_adam=1,
                                  stream=stream.cuda_stream, expert_shard=expert_shards(M, 1)[0] if mode == "ep" else None)
                e.set_skill_table(table); e.set_skill_csr((s_ip, s_ix)); e.set_member((m_ip, m_ix)); e.load_state_dict(sd)
                if mode == "plain":
                    loss = e.train_epoch(order, B); full = e.state_dict()
                else:
                    ep = ExpertParallel(e)
                    assert ep.force and ep._dh is not None and ep._dh.numel() == B * 128
                    loss = ep.train_epoch(order, B); full = ep.state_dict()
                    v = ep.eval_epoch(order[:B], B); assert np.isfinite(v)
                results.append((loss, full))
                e.close()
        (la, pa), (lb, pb) = results
        assert abs(la - lb) <= 1e-6 * abs(la)
        for k in pa:
            assert np.array_equal(pa[k], pb[k]), k
    finally:
        dist.destroy_process_group()
        os.environ.pop("NTF_EP_FORCE_EXCHANGE", None)


def test_plugin_trains_expert_sharded_under_torch_distributed(tmp_path, monkeypatch):
    """Bnn.learn / test through the expert-sharded branch of the plugin (what `torchrun ... main.py` takes on a multi-GPU node), forced on one GPU:
    sharded engine for learn(), ExpertParallel as the runner, the gathered state_dict in the checkpoints, a whole-model engine for test().
    Same files and - the shard being the whole layer - the weights of the plain single-GPU run."""
    import socket
    import torch.distributed as dist
    from opentf_amd.mdl.bnn import Bnn
    tv, splits = _toy("dblp")
    cfg = Cfg(b=6, e=2, ns=3, lr=0.01, es=5, h=[128], spe=0, l="bce", tpw=10, tnw=1, nsd="uniform", nmc=2)
    plain = Bnn(str(tmp_path / "plain"), "cuda:0", 0, cfg); plain.learn(tv, splits, None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    monkeypatch.setenv("NTF_PARALLEL", "ep"); monkeypatch.setenv("NTF_EP_FORCE_EXCHANGE", "1")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        m = Bnn(str(tmp_path / "ep"), "cuda:0", 0, cfg)
        m.learn(tv, splits, None)
        assert type(m._runner).__name__ == "ExpertParallel"
        m.test(tv, splits, Cfg(per_epoch=False, on_train=False, topK=None))
    finally:
        dist.destroy_process_group()
    for k in range(3):
        a = torch.load(f"{plain.output}/f{k}.pt", map_location="cpu", weights_only=False)
        b = torch.load(f"{m.output}/f{k}.pt", map_location="cpu", weights_only=False)
        assert list(a.keys()) == list(b.keys()) and a["e"] == b["e"]
        assert abs(a["t_loss"] - b["t_loss"]) <= 1e-6 * abs(a["t_loss"]) and abs(a["v_loss"] - b["v_loss"]) <= 1e-6 * abs(a["v_loss"])   # f32 mean vs f64 mean of the same batch losses
        for name in a["model_state_dict"]:
            # toy dblp's skill rows are multi-hot: the first layer's weight gradient is a scatter-add by float atomics, so two runs agree to rounding only
            assert torch.allclose(a["model_state_dict"][name], b["model_state_dict"][name], rtol=1e-4, atol=1e-6), name
        pr = torch.load(f"{m.output}/f{k}.test.pred", map_location="cpu", weights_only=False)
        assert tuple(pr["y_pred"].shape) == (len(splits["test"]), tv["member"].shape[1])


@pytest.mark.parametrize("mode", ["ep", "dp"])
def test_plugin_two_processes_one_gpu(mode, tmp_path):
    """torchrun's situation for real at world size 2: two processes, each with its own engine on this GPU, collectives over gloo (RCCL refuses two ranks on
    one device): Bnn.learn / test in the expert-sharded and the data-parallel form write the files of the single-process run with its weights."""
    import socket
    import subprocess
    import sys
    from opentf_amd.mdl.bnn import Bnn
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import plugin_two_process_check as chk
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import plugin_two_process_check as m; m.worker(%%d, 2, %d, %r, %r)" % (here, port, str(tmp_path), mode)   # (imported, not __main__: the checkpoint pickles m.Cfg)
    procs = [subprocess.Popen([sys.executable, "-c", code % r], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    tv, splits = chk.dataset()
    ref = Bnn(str(tmp_path / "single"), "cuda:0", 0, Cfg(chk.CFG)); ref.learn(tv, splits, None)
    out_dir = [d for d in os.listdir(tmp_path / mode)][0]
    a = torch.load(f"{ref.output}/f0.pt", map_location="cpu", weights_only=False)
    b = torch.load(f"{tmp_path}/{mode}/{out_dir}/f0.pt", map_location="cpu", weights_only=False)
    assert os.path.basename(ref.output) == out_dir and list(a.keys()) == list(b.keys()) and a["e"] == b["e"]
    assert abs(a["t_loss"] - b["t_loss"]) <= 1e-4 * abs(a["t_loss"]) and abs(a["v_loss"] - b["v_loss"]) <= 1e-4 * abs(a["v_loss"])
    for name, v in a["model_state_dict"].items():
        w = b["model_state_dict"][name]
        assert tuple(w.shape) == tuple(v.shape), name
        assert torch.allclose(v, w, rtol=2e-4, atol=2e-5), (name, float((v - w).abs().max()))
    # predictions: under "ep" every rank infers its own experts and rank 0 merges (dense columns, top-K candidates, entropy shares); under "dp" rank 0 alone
    chk.predictions(ref, tv, splits, True)
    for name in ("f0.test.dense.pred", "f0.test.pred"):
        pa = torch.load(f"{ref.output}/{name}", map_location="cpu", weights_only=False)
        pb = torch.load(f"{tmp_path}/{mode}/{out_dir}/{name}", map_location="cpu", weights_only=False)
        ya, yb = pa["y_pred"], pb["y_pred"]
        assert tuple(yb.shape) == (len(splits["test"]), tv["member"].shape[1]) and ya.is_sparse == yb.is_sparse
        if ya.is_sparse:
            assert yb.is_coalesced() and yb._nnz() == ya._nnz() == 5 * len(splits["test"])
            va = np.sort(ya.values().numpy().reshape(-1, 5), axis=1); vb = np.sort(yb.values().numpy().reshape(-1, 5), axis=1)
            np.testing.assert_allclose(vb, va, rtol=2e-3, atol=2e-4)          # the two runs' weights agree to rounding: so do the five largest probabilities
        else:
            np.testing.assert_allclose(yb.numpy(), ya.numpy(), rtol=2e-3, atol=2e-4)
        for key in ("pred", "model"):
            assert len(pb["uncertainty"][key]) == len(pa["uncertainty"][key]) == 1
            np.testing.assert_allclose(pb["uncertainty"][key][0], pa["uncertainty"][key][0], rtol=5e-3, atol=5e-3)


@pytest.mark.parametrize("parallel", ["ep", "dp", "auto"])
def test_bench_multi_rank_launch_on_one_gpu(parallel):
    """the driver's N > 1 launch line (`python -m torch.distributed.run ... bench.py --gpus N ...`) with both ranks on this GPU over gloo: rank handling,
    barriers, the max-over-ranks timing and the single JSON line of bench.py's multi-rank path"""
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--validate-on-one-gpu", "--parallel", parallel,
           "--rows", "20000", "--experts", "4096"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=root, env=os.environ)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["config"]["global_batch"] == 2000
    head = "dp" if parallel == "auto" else parallel        # default: the headline is north_star's form - data parallel, b = 1000 per GPU
    assert d["config"]["parallelism"].startswith(head + "2") and d["value"] > 0 and np.isfinite(d["mean_loss"])
    assert d["roofline"]["kernel"] in ("out_fused_fwd_loss_dh", "out_fused_dw_adam") and d["cpu_baseline"] is None
    assert d["rccl_ranks"] == 2 and d["timed_regions"] >= 2 and d["ms_per_step_spread"] is not None
    if parallel == "auto":   # ... and the other two ways of sharing a step are timed in the same launch
        ew, st = d["ep_weak"], d["strong_b1000"]
        assert ew["parallelism"] == "ep" and ew["scaling"] == "weak" and ew["global_batch"] == 2000 and ew["rows_per_rank"] == 2000 and ew["value"] > 0
        assert st["scaling"] == "strong" and st["global_batch"] == 1000 and st["parallelism"] == "ep" and st["value"] > 0      # (4096 experts shard over 2 ranks)
        assert ew["rccl_payload_bytes_per_step"] == 4 * 2000 * 128 and d["rccl_payload_bytes_per_step"] > 8 * 128 * 4096
        assert np.isfinite(ew["mean_loss"]) and np.isfinite(st["mean_loss"])


@pytest.mark.parametrize("fail", ["ep_weak:build:1", "ep_weak:run"])
def test_bench_headline_survives_a_failing_extra_leg(fail):
    """an exception in the `ep_weak` leg of the N > 1 launch - on ONE rank while it builds its engine (the ranks agree to skip the leg before
    anyone enters a collective), or on every rank inside the leg (the later leg is skipped too: the collectives' state is unknown) - becomes {"error": ...} under
    that key; the data-parallel headline is printed all the same.  Exit code: 0 when the leg was skipped before any collective, non-zero when it failed while
    running (the launcher must see that the collectives' state was left undefined) - the line is on stdout either way"""
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--validate-on-one-gpu", "--parallel", "auto", "--rows", "20000", "--experts", "4096"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=root, env={**os.environ, "NTF_BENCH_FAIL_LEG": fail})
    if fail.startswith("ep_weak:build"): assert p.returncode == 0, p.stderr.decode()[-3000:]
    else: assert p.returncode != 0, "a leg that failed while running must not look like success"
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"].startswith("dp2") and d["value"] > 0 and np.isfinite(d["mean_loss"])
    assert "error" in d["ep_weak"] and "value" not in d["ep_weak"], d["ep_weak"]
    if fail.startswith("ep_weak:build"):
        assert "skipped before any collective" in d["ep_weak"]["error"] and d["strong_b1000"]["value"] > 0
    else:
        assert "injected failure" in d["ep_weak"]["error"] and "error" in d["strong_b1000"]


def test_bench_dump_outputs_are_the_state_after_exactly_the_timed_steps(tmp_path):
    """bench.py --dump-outputs: the same arguments give the same files (the inputs are seeded and exactly --steps steps are timed), one more step gives another
    state, and the dumped loss is the one the JSON line reports"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(steps, out):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rows", "20000", "--experts", "4096",
               "--no-cpu-baseline", "--no-f32-line", "--no-extra-configs", "--no-gather-bench", "--dump-outputs", str(tmp_path / out)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=root)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
        assert len(lines) == 1, lines
        return json.loads(lines[0])
    d = run(3, "a"); run(3, "b"); run(4, "c")
    assert d["steps"] == 3 and d["timed_regions"] == 2
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["mean_loss.npy"] + [f"layers.{l}.{k}.npy" for l in (0, 1) for k in ("mu_weight", "rho_weight", "mu_bias", "rho_bias")])
    loss = np.load(tmp_path / "a" / "mean_loss.npy")
    assert loss.dtype == np.float64 and float(loss) == d["mean_loss"]
    w = np.load(tmp_path / "a" / "layers.1.mu_weight.npy")
    assert w.dtype == np.float32 and w.shape == (4096, 128)
    for n in names:
        np.testing.assert_allclose(np.load(tmp_path / "b" / n), np.load(tmp_path / "a" / n), rtol=1e-5, atol=1e-6, err_msg=n)
    assert np.abs(np.load(tmp_path / "c" / "layers.1.mu_weight.npy") - w).max() > 1e-5      # a fourth Adam step (lr 1e-3) moved the weights
