"""Parity of the HIP engine (through the C ABI) against the oracle and the golden vectors, on a real
MI355X.  Bars: gather bit-exact; logits within 1e-4 relative (north_star); losses/gradients within the
tolerances written at each assert."""
import json
import os

import numpy as np
import pytest
import scipy.sparse
import torch

from conftest import GOLDEN, golden, params_from, draw_noise
from oracle import ntf_oracle as O

pytestmark = pytest.mark.gpu

RTOL_LOGITS = 1e-4  # BASELINE.json north_star: expert-ranking logits within 1e-4 relative


def _engine(*a, **k):
    from opentf_amd.libntf import Engine
    return Engine(*a, **k)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=rtol, atol=atol)


def _csr_from_dense(y):
    m = scipy.sparse.csr_matrix(np.asarray(y) != 0)
    return m.indptr.astype(np.int64), m.indices.astype(np.int32)


# ------------------------------------------------------------------------------------------ gather
def test_gather_bitexact_vs_reference_golden():
    from opentf_amd import libntf
    g = golden("g9_gather_dblp")
    S, d = g["table"].shape
    e = _engine([d, 8, int(g["n_member"])], input_mode=libntf.INPUT_MEANPOOL, max_batch=64)
    e.set_skill_table(g["table"]); e.set_skill_csr((g["indptr"], g["indices"]))
    X = e.gather_meanpool(n=len(g["indptr"]) - 1)
    assert np.array_equal(X, O.gather_meanpool_fast(g["indptr"], g["indices"], g["table"]))
    _close(X, g["X"], 1e-6, 1e-7)  # the reference's own scipy result
    rows = np.array([5, 0, 30, 7, 7])
    assert np.array_equal(e.gather_meanpool(rows=rows), X[rows])


@pytest.mark.parametrize("d,S,N,mean_nnz", [(128, 5000, 20000, 8.57), (256, 3000, 5000, 6.3), (32, 100, 777, 2.0), (100, 64, 300, 40.0), (30, 50, 200, 3.0)])
def test_gather_bitexact_ragged(d, S, N, mean_nnz):
    from opentf_amd import libntf
    rng = np.random.default_rng(d)
    nnz = 1 + rng.poisson(mean_nnz - 1, N)
    nnz[::97] = 0  # empty teams: the reference divides 0/0 -> nan
    nnz[5] = min(S, 200)  # a very long row
    indptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
    indices = np.concatenate([rng.choice(S, k, replace=False) for k in nnz]).astype(np.int32)
    table = rng.standard_normal((S, d)).astype(np.float32)
    e = _engine([d, 8, 16], input_mode=libntf.INPUT_MEANPOOL, max_batch=64)
    e.set_skill_table(table); e.set_skill_csr((indptr, indices))
    X = e.gather_meanpool(n=N)
    ref = O.gather_meanpool_fast(indptr, indices, table)
    assert np.array_equal(np.isnan(X), np.isnan(ref))
    assert np.array_equal(np.nan_to_num(X), np.nan_to_num(ref))


# ------------------------------------------------------------------------------------------ Fnn
@pytest.mark.parametrize("name", ["g1_forward_imdb", "g1_forward_mid", "g1_forward_2h"])
@pytest.mark.parametrize("fused", [False, True])
def test_fnn_logits_vs_reference_golden(name, fused):
    g = golden(name)
    sd = params_from(g, "p.")
    dims = [g["X"].shape[1]] + [sd[f"layers.{i}.weight"].shape[0] for i in range(O.n_layers(sd))]
    e = _engine(dims, max_batch=len(g["X"]), fused=fused)
    e.load_state_dict(sd); e.set_dense_input(g["X"])
    out = e.logits(np.arange(len(g["X"])))
    assert _rel(out, g["logits"]) < RTOL_LOGITS
    _close(out, g["logits"], RTOL_LOGITS, 1e-6)


@pytest.mark.parametrize("tag", ["imdb", "mid"])
@pytest.mark.parametrize("fused", [False, True, "f32"])
def test_fnn_train_steps_vs_reference_golden(tag, fused):
    g = golden(f"g4_step_{tag}")
    sd = params_from(g, "p0.")
    X, y = g["X"], g["y"]
    dims = [X.shape[1]] + [sd[f"layers.{i}.weight"].shape[0] for i in range(O.n_layers(sd))]
    e = _engine(dims, max_batch=len(X), ns=5, nsd="uniform", tpw=float(g["tpw"]), tnw=float(g["tnw"]), lr=float(g["lr"]), fused=bool(fused),
                mfma=fused if isinstance(fused, str) else None)
    e.load_state_dict(sd); e.set_dense_input(X); e.set_member(_csr_from_dense(y))
    rows = np.arange(len(X))
    for s in range(3):
        loss = e.train_step(rows, inject={"neg_idx": g[f"s{s}.idx"]})
        assert abs(loss - float(g[f"s{s}.loss"])) <= 2e-5 * abs(loss), (s, loss, float(g[f"s{s}.loss"]))
        grads, state = e.grads(), e.state_dict()
        for k in sd:
            ref_g = g[f"s{s}.g.{k}"]
            assert _rel(grads[k], ref_g) < 2e-4, (s, k, _rel(grads[k], ref_g))
            _close(state[k], g[f"s{s}.p.{k}"], 1e-3, 2e-5)  # Adam's m/sqrt(v) amplifies grad noise near zero grads


# ------------------------------------------------------------------------------------------ Bnn (oracle, injected noise)
def _bnn_case(D, H, M, B, seed):
    torch.manual_seed(seed)
    sd = O.bnn_init(D, H, M)
    X = torch.randn(B, D)
    y = (torch.rand(B, M) < 0.01).float(); y[torch.arange(B), torch.randint(0, M, (B,))] = 1
    return sd, X, y


@pytest.mark.parametrize("D,H,M,B", [(18, [32], 112, 19), (128, [128], 1500, 70), (40, [64, 32], 300, 33), (128, [128], 5000, 130),
                                     (24, [64], 777, 129), (16, [128], 13, 1), (16, [32], 63, 257), (50, [], 90, 21), (32, [], 100, 40)])
@pytest.mark.parametrize("fused", [False, True, "f32"])
def test_bnn_step_vs_oracle_injected(D, H, M, B, fused):
    """fused=True: the fused kernels in their default arithmetic (fp16x3 split products); "f32": the
    exact-f32 MFMA kernels."""
    sd, X, y = _bnn_case(D, H, M, B, 5)
    e = _engine([D] + H + [M], bayesian=True, max_batch=B, ns=5, nsd="uniform", lr=1e-3, fused=bool(fused), mfma=fused if isinstance(fused, str) else None)
    e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
    rows = np.arange(B)
    opt = O.Adam(sd, 1e-3)
    for s in range(2):
        noise = draw_noise(sd, B)
        neg = O.ns_uniform(y, 5)
        inj = {"neg_idx": neg.numpy(), "eps_w": [n["eps_w"] for n in noise], "eps_b": [n["eps_b"] for n in noise],
               "s_in": [n["s_in"] for n in noise], "s_out": [n["s_out"] for n in noise]}
        # the forward kernel is judged on the weights the ENGINE holds: after an Adam step those differ from the oracle's by up to the state tolerance
        # below (a leaky_relu' kink flip moves one expert's gradient row, and Adam turns any gradient difference into a +-lr step)
        sd_e = {k: torch.from_numpy(v) for k, v in e.state_dict().items()}
        ref_logits = O.bnn_forward(sd_e, X, noise).detach().numpy()
        got = e.logits(rows, inject=inj)
        assert _rel(got, ref_logits) < RTOL_LOGITS
        _close(got, ref_logits, RTOL_LOGITS, 2e-6)
        ref_eval = float(O.batch_loss(sd, X, y, neg, 10.0, 1.0, noise))
        assert abs(e.eval_step(rows, inject=inj) - ref_eval) <= 2e-5 * abs(ref_eval)
        ref_loss, ref_grads = O.train_step(sd, opt, X, y, neg, 10.0, 1.0, noise)
        loss = e.train_step(rows, inject=inj)
        assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
        grads, state = e.grads(), e.state_dict()
        for k in sd:
            assert _rel(grads[k], ref_grads[k].numpy()) < 3e-4, (s, k, _rel(grads[k], ref_grads[k].numpy()))
            _close(state[k], sd[k].numpy(), 1e-3, 2e-5)


@pytest.mark.parametrize("bayesian", [False, True])
@pytest.mark.parametrize("S,H,M,B", [(700, [128], 1500, 90), (90, [64, 32], 300, 33), (3000, [256], 2000, 257)])
def test_multihot_first_layer_step_vs_oracle(bayesian, S, H, M, B):
    """BASELINE config 3's input: the skill row itself (src/mdl/ntf.py:23).  The engine never densifies it — layer 0 is a gather-sum
    of W0 columns and its gradient a scatter-add — and must equal the oracle fed the dense 0/1 matrix."""
    from opentf_amd import libntf
    torch.manual_seed(3)
    sd = O.bnn_init(S, H, M) if bayesian else O.fnn_init(S, H, M)
    rng = np.random.default_rng(S)
    Xd = np.zeros((B, S), np.float32)
    for i in range(B):
        Xd[i, rng.choice(S, 1 + rng.poisson(7.5), replace=False)] = 1
    Xd[3] = 0                                     # a team without skills: only the bias reaches the hidden layer
    X = torch.from_numpy(Xd)
    y = (torch.rand(B, M) < 0.01).float(); y[torch.arange(B), torch.randint(0, M, (B,))] = 1
    e = _engine([S] + H + [M], bayesian=bayesian, input_mode=libntf.INPUT_MULTIHOT, max_batch=B, ns=5, nsd="uniform", lr=1e-3)
    e.load_state_dict(sd); e.set_skill_csr(_csr_from_dense(Xd)); e.set_member(_csr_from_dense(y.numpy()))
    rows = np.arange(B)
    opt = O.Adam(sd, 1e-3)
    for s in range(2):
        noise = draw_noise(sd, B) if bayesian else None
        neg = O.ns_uniform(y, 5)
        inj = {"neg_idx": neg.numpy()}
        if bayesian:
            inj.update({"eps_w": [n["eps_w"] for n in noise], "eps_b": [n["eps_b"] for n in noise],
                        "s_in": [n["s_in"] for n in noise], "s_out": [n["s_out"] for n in noise]})
        ref_logits = (O.bnn_forward(sd, X, noise) if bayesian else O.fnn_forward(sd, X)).detach().numpy()
        got = e.logits(rows, inject=inj)
        assert _rel(got, ref_logits) < RTOL_LOGITS
        ref_loss, ref_grads = O.train_step(sd, opt, X, y, neg, 10.0, 1.0, noise)
        loss = e.train_step(rows, inject=inj)
        assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
        grads, state = e.grads(), e.state_dict()
        for k in sd:
            assert _rel(grads[k], ref_grads[k].numpy()) < 3e-4, (s, k, _rel(grads[k], ref_grads[k].numpy()))
            _close(state[k], sd[k].numpy(), 1e-3, 2e-5)
        # both sides continue from the engine's parameters: a 1e-7 difference left by Adam is enough to put one pre-activation on the
        # other side of leaky_relu's kink, which moves a whole row of dh (seen on this case) — that is not what this test is about
        with torch.no_grad():
            for k in sd: sd[k].copy_(torch.from_numpy(state[k]))


@pytest.mark.parametrize("mfma", ["f32", None])
@pytest.mark.parametrize("bayesian", [False, True])
def test_adam_fused_into_dw_epilogue_equals_flat_adam(bayesian, mfma):
    """cfg.fuse_adam moves the output layer's Adam into the dW kernel's epilogue: same parameters, step for step."""
    sd, X, y = _bnn_case(64, [128], 900, 150, 3)
    if not bayesian:
        torch.manual_seed(3); sd = O.fnn_init(64, [128], 900)
    def run(fuse):
        # the three modes share one product arithmetic (exact-f32 MFMA or the default fp16x3): this test is about WHERE Adam runs
        e = _engine([64, 128, 900], bayesian=bayesian, max_batch=150, ns=4, nsd="uniform", seed=21, lr=1e-2, fuse_adam=fuse, mfma=mfma)
        e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
        losses = [e.train_step(np.arange(150)) for _ in range(4)]
        return losses, e.state_dict()
    (la, pa), (lb, pb), (lc, pc) = run(0), run(1), run(2)
    np.testing.assert_allclose(la, lb, rtol=1e-6); np.testing.assert_allclose(la, lc, rtol=1e-6)
    for k in pa:
        np.testing.assert_allclose(pa[k], pb[k], rtol=1e-5, atol=1e-7)
        assert np.array_equal(pa[k], pc[k]), k  # mode 2 runs the same Adam kernel on the same gradients, only elsewhere in time


@pytest.mark.parametrize("nsd", ["uniform", "unigram", "unigram_b"])
def test_sharded_staged_steps_draw_what_the_single_process_step_draws(nsd):
    """Data-parallel contract with the NATIVE generators: eps is keyed by (seed, step, element), signs and sampled negatives by the
    row's position inside the GLOBAL minibatch, so two ranks' shards (same seed, same step) sum to the single-process gradient."""
    sd, X, y = _bnn_case(64, [128], 700, 96, 11)
    order = np.random.default_rng(2).permutation(96)
    freq = y.numpy().sum(0) / 96.0
    def mk():
        e = _engine([64, 128, 700], bayesian=True, max_batch=96, ns=4, nsd=nsd, seed=77)
        e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
        if nsd == "unigram": e.set_unigram(freq)
        e.stage_order(order); return e
    full, a, b = mk(), mk(), mk()
    lf = full.step_staged(0, 96, 0, 96, train=True, apply=False, want_loss=True); gf = full.grads()
    la = a.step_staged(0, 40, 0, 96, train=True, apply=False, want_loss=True)
    lb = b.step_staged(40, 56, 0, 96, train=True, apply=False, want_loss=True)
    assert abs((la + lb) - lf) <= 1e-5 * abs(lf)
    ga, gb = a.grads(), b.grads()
    for k in gf:
        assert _rel(ga[k] + gb[k], gf[k]) < 2e-4, (k, _rel(ga[k] + gb[k], gf[k]))


def test_split_backward_equals_train_step():
    """ntf_backward over two row shards with global_B, gradients summed == one full-batch gradient."""
    sd, X, y = _bnn_case(32, [32], 200, 24, 9)
    def mk():
        e = _engine([32, 32, 200], bayesian=True, max_batch=24, ns=3, nsd="uniform", fused=False)
        e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy())); return e
    noise = draw_noise(sd, 24); neg = O.ns_uniform(y, 3)
    def inj(sl):
        return {"neg_idx": neg.numpy()[sl], "eps_w": [n["eps_w"] for n in noise], "eps_b": [n["eps_b"] for n in noise],
                "s_in": [n["s_in"][sl] for n in noise], "s_out": [n["s_out"][sl] for n in noise]}
    full = mk(); lf = full.backward(np.arange(24), inject=inj(slice(0, 24))); gf = full.grads()
    a, b = mk(), mk()
    la = a.backward(np.arange(0, 10), global_B=24, inject=inj(slice(0, 10)))
    lb = b.backward(np.arange(10, 24), global_B=24, inject=inj(slice(10, 24)))
    assert abs((la + lb) - lf) <= 1e-5 * abs(lf)
    ga, gb = a.grads(), b.grads()
    for k in gf:
        assert _rel(ga[k] + gb[k], gf[k]) < 1e-4, k


# ------------------------------------------------------------------------------------------ inputs
def test_multihot_input_toy_imdb():
    """BASELINE config 1 shapes: multi-hot skills (S=18) -> h=[32] -> 112 experts."""
    from opentf_amd import libntf
    toy = golden("toy_imdb")
    n, S, M = [int(v) for v in toy["shape"]]
    g = golden("g1_forward_imdb")
    sd = params_from(g, "p.")
    e = _engine([S, 32, M], input_mode=libntf.INPUT_MULTIHOT, max_batch=n)
    e.load_state_dict(sd); e.set_skill_csr((toy["skill_indptr"], toy["skill_indices"]))
    _close(e.logits(np.arange(n)), g["logits"], RTOL_LOGITS, 1e-6)


def test_meanpool_input_feeds_the_model():
    from opentf_amd import libntf
    g = golden("g9_gather_dblp")
    torch.manual_seed(3)
    sd = O.fnn_init(128, [64], int(g["n_member"]))
    n = len(g["indptr"]) - 1
    e = _engine([128, 64, int(g["n_member"])], input_mode=libntf.INPUT_MEANPOOL, max_batch=n)
    e.load_state_dict(sd); e.set_skill_table(g["table"]); e.set_skill_csr((g["indptr"], g["indices"]))
    ref = O.fnn_forward(sd, torch.from_numpy(g["X"])).detach().numpy()
    _close(e.logits(np.arange(n)), ref, RTOL_LOGITS, 1e-6)


# ------------------------------------------------------------------------------------------ native generators
def test_native_uniform_sampler_invariants_and_distribution():
    B, M, ns = 256, 50, 5
    rng = np.random.default_rng(0)
    y = (rng.random((B, M)) < 0.1).astype(np.float32); y[:, 0] = 1
    y[7] = 1; y[7, [3, 9]] = 0  # row with only 2 negatives < ns
    torch.manual_seed(0); sd = O.fnn_init(8, [8], M)
    # the picks are observable through the gradient of the output bias: with tnw=0 ONLY positives and picks get gradient
    e2 = _engine([8, 8, M], max_batch=B, ns=ns, nsd="uniform", tpw=1.0, tnw=0.0, seed=7, fused=False)
    sd2 = {k: torch.zeros_like(v) for k, v in sd.items()}
    e2.load_state_dict(sd2); e2.set_dense_input(np.ones((B, 8), np.float32)); e2.set_member(_csr_from_dense(y))
    hits = np.zeros(M)
    for it in range(200):
        # one row at a time isolates the row's picks in the bias gradient
        r = it % B
        e2.backward(np.array([r]))
        gb = e2.grads()["layers.1.bias"]
        picked = np.nonzero(gb > 0)[0]   # y=0, weight 1 -> +sigmoid(0)=0.5 ; positives give -0.5 ; others 0
        negs_available = int((y[r] == 0).sum())
        assert len(picked) == min(ns, negs_available), (r, picked)
        assert (y[r, picked] == 0).all()
        if negs_available >= ns and r != 7:
            hits[picked] += 1
    # column 0 is always a positive -> never picked; the rest roughly uniform
    assert hits[0] == 0
    expected = hits[1:].mean()
    assert (np.abs(hits[1:] - expected) < 6 * np.sqrt(expected) + 5).all()


@pytest.mark.parametrize("fused", [False, True])
def test_native_unigram_b_sampler_draws_from_the_batch_support(fused):
    """unigram_b (src/mdl/fnn.py:59-76): negatives of a row come from the experts of the CURRENT batch, minus the row's own, with
    probability proportional to their batch frequency.  Identity first layer + one-hot inputs make column i of dW[out] row i's dz."""
    B, M, ns = 64, 300, 4
    rng = np.random.default_rng(3)
    y = np.zeros((B, M), np.float32)
    hot = np.arange(10)                       # ten frequent experts ...
    for i in range(B):
        y[i, rng.choice(hot, 2, replace=False)] = 1
        y[i, 10 + (i % 40)] = 1               # ... and forty rare ones; columns >= 50 never occur in the batch
    sd = {"layers.0.weight": torch.eye(B), "layers.0.bias": torch.zeros(B), "layers.1.weight": torch.zeros(M, B), "layers.1.bias": torch.zeros(M)}
    e = _engine([B, B, M], max_batch=B, ns=ns, nsd="unigram_b", tpw=1.0, tnw=0.0, seed=5, fused=fused)
    e.load_state_dict(sd); e.set_dense_input(np.eye(B, dtype=np.float32)); e.set_member(_csr_from_dense(y))
    hits = np.zeros(M)
    for it in range(60):
        e.backward(np.arange(B))
        dw = e.grads()["layers.1.weight"]      # [M, B]
        for i in range(B):
            picked = np.nonzero(dw[:, i] > 0)[0]
            assert len(picked) == ns, (i, picked)
            assert (y[i, picked] == 0).all() and (picked < 50).all()
            hits[picked] += 1
    freq = y.sum(0)
    assert hits[50:].sum() == 0
    assert hits[:10].min() > 2 * hits[10:50].max()          # frequent experts dominate
    ratio = (hits[:10] / freq[:10]).mean() / (hits[10:50] / freq[10:50]).mean()
    assert 0.5 < ratio < 1.3                                 # ~proportional (without-replacement draws flatten it a little)
    # single-row batch: every weighted expert is a member -> the reference falls back to uniform over all columns
    e1 = _engine([B, B, M], max_batch=B, ns=ns, nsd="unigram_b", tpw=1.0, tnw=0.0, seed=5, fused=fused)
    e1.load_state_dict(sd); e1.set_dense_input(np.eye(B, dtype=np.float32)); e1.set_member(_csr_from_dense(y))
    seen = set()
    for it in range(50):
        e1.backward(np.array([it % B]))
        seen.update(np.nonzero(e1.grads()["layers.1.weight"][:, it % B] > 0)[0].tolist())
    assert max(seen) >= 50 and len(seen) > 100


def test_native_normal_and_sign_statistics():
    from opentf_amd import libntf
    n = 1 << 22
    buf = torch.empty(n, device="cuda")
    assert libntf.lib().ntf_k_fill_normal(None, 1234, 7, 1, n, buf.data_ptr()) == 0
    torch.cuda.synchronize()
    z = buf.double().cpu().numpy()
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 0.01
    assert abs((z ** 3).mean()) < 0.02 and abs((z ** 4).mean() - 3) < 0.05
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 5e-3 and abs(np.corrcoef(z[:-4], z[4:])[0, 1]) < 5e-3
    assert np.abs(z).max() > 4.5  # tails are present
    buf2 = torch.empty(n, device="cuda")
    libntf.lib().ntf_k_fill_normal(None, 1234, 8, 1, n, buf2.data_ptr()); torch.cuda.synchronize()
    assert abs(np.corrcoef(z, buf2.double().cpu().numpy())[0, 1]) < 5e-3  # steps are independent
    rows, cols = 2048, 2048
    s = torch.empty(rows * cols, device="cuda")
    assert libntf.lib().ntf_k_fill_sign(None, 99, 3, 1, rows, cols, s.data_ptr()) == 0
    torch.cuda.synchronize()
    sg = s.cpu().numpy().reshape(rows, cols)
    assert set(np.unique(sg)) == {-1.0, 1.0}
    assert abs(sg.mean()) < 5 / np.sqrt(rows * cols)
    assert np.abs(sg.mean(axis=0)).max() < 6 / np.sqrt(rows) and np.abs(sg.mean(axis=1)).max() < 6 / np.sqrt(cols)
    assert abs((sg[:, :-1] * sg[:, 1:]).mean()) < 5e-3 and abs((sg[:-1] * sg[1:]).mean()) < 5e-3


def test_native_flipout_matches_oracle_in_distribution():
    """With native eps/signs the logits cannot match draw for draw; their mean over many passes must approach
    the deterministic mu-only forward, and their variance the analytic flipout variance."""
    torch.manual_seed(2)
    D, H, M, B = 16, 16, 64, 8
    sd = O.bnn_init(D, [H], M)
    X = torch.randn(B, D)
    e = _engine([D, H, M], bayesian=True, max_batch=B, seed=11)
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    outs = np.stack([e.logits(np.arange(B)) for _ in range(400)])
    ref = np.stack([O.bnn_forward(sd, X, draw_noise(sd, B)).numpy() for _ in range(400)])
    assert np.abs(outs.mean(0) - ref.mean(0)).max() < 6 * ref.std(0).max() / np.sqrt(400) + 1e-3
    assert abs(outs.std(0).mean() / ref.std(0).mean() - 1) < 0.1


# ------------------------------------------------------------------------------------------ inference
def test_forward_probs_topk_and_uncertainty():
    sd, X, y = _bnn_case(32, [32], 700, 20, 4)
    e = _engine([32, 32, 700], bayesian=True, max_batch=20)
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    noises = [draw_noise(sd, 20) for _ in range(3)]
    injs = [{"eps_w": [n["eps_w"] for n in nz], "eps_b": [n["eps_b"] for n in nz], "s_in": [n["s_in"] for n in nz],
             "s_out": [n["s_out"] for n in nz]} for nz in noises]
    mc = O.predict(sd, X, 3, noises).numpy()
    probs, pu, mu = e.forward(np.arange(20), nmc=3, injects=injs, uncertainty=True)
    _close(probs, mc.mean(0), 1e-5, 1e-7)
    _close(pu, O.predictive_entropy(mc), 1e-4, 1e-4)
    _close(mu, O.mutual_information(mc), 1e-3, 2e-4)
    # Fnn path + GPU top-K against torch.topk
    torch.manual_seed(1)
    fsd = O.fnn_init(32, [32], 3000)
    f = _engine([32, 32, 3000], max_batch=20)
    f.load_state_dict(fsd); f.set_dense_input(X.numpy())
    p = f.forward(np.arange(20))
    _close(p, O.predict(fsd, X).numpy(), 1e-5, 1e-7)
    vals, idx = f.forward_topk(np.arange(20), 50)
    tv, ti = torch.topk(torch.from_numpy(p), 50, dim=1)
    assert np.array_equal(vals, tv.numpy())
    assert np.array_equal(np.sort(idx, axis=1), np.sort(ti.numpy(), axis=1))


@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("mfma", [None, "f32"])
def test_forward_probs_uncertainty_h128(bayesian, mfma):
    """H = 128: in the split-product arithmetics the inference runs through the fused forward kernel (probabilities accumulated over the MC
    passes in a transposed buffer, no dense logits); mfma="f32" keeps the generic GEMM route.  Both against the oracle with injected noise."""
    D, M, B, nmc = 24, 1777, 45, 3
    sd, X, y = _bnn_case(D, [128], M, B, 4)
    if not bayesian:
        torch.manual_seed(2); sd = O.fnn_init(D, [128], M); nmc = 1
    e = _engine([D, 128, M], bayesian=bayesian, max_batch=B, mfma=mfma)
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    noises = [draw_noise(sd, B) for _ in range(nmc)] if bayesian else None
    injs = [{"eps_w": [n["eps_w"] for n in nz], "eps_b": [n["eps_b"] for n in nz], "s_in": [n["s_in"] for n in nz],
             "s_out": [n["s_out"] for n in nz]} for nz in noises] if bayesian else None
    mc = O.predict(sd, X, nmc, noises).numpy()
    mc = mc if mc.ndim == 3 else mc[None]
    probs, pu, mu = e.forward(np.arange(B), nmc=nmc, injects=injs, uncertainty=True)
    _close(probs, mc.mean(0), 1e-5, 1e-7)
    _close(pu, O.predictive_entropy(mc), 1e-4, 1e-4)
    if bayesian: _close(mu, O.mutual_information(mc), 1e-3, 2e-4)
    vals, idx = e.forward_topk(np.arange(B), 40, nmc=1) if not bayesian else (None, None)
    if not bayesian:
        order = np.argsort(-probs, axis=1, kind="stable")[:, :40]
        assert np.array_equal(idx, order)


_TOPK_CASES = [(40000, 50, None), (70001, 100, None), (40000, 20, 100), (33000, 256, None), (40000, 257, None), (40000, 2048, None), (2048, 2048, None),
               (70001, 1, None), (40000, 20, 3000), (40000, 50, 1000), (2500, 40, 2040)]


@pytest.mark.parametrize("M,K,ties", _TOPK_CASES, ids=[f"{M}-{K}-{ {None: False, 100: True}.get(g0, g0)}" for M, K, g0 in _TOPK_CASES])
def test_topk_sampled_threshold_path_is_exact(M, K, ties):
    """Rows long enough for the sampled-threshold selection (ntf_select.h, run by k_topk_rows): the result must be the exact, deterministic
    ranking (value descending, expert id ascending among equals) — also when a tie group straddles the K-th place.  K above 256 leaves
    the sampled path for the exact radix selection on a long row (257: the first such K; 2048: the sort's capacity); K = M ranks the
    whole row; K = 1 sorts nothing.
    `ties` is the first column g0 of a group of 300 experts with one probability, the row's largest (None: no such group), so the top K
    are g0 .. g0 + K - 1, all taken by the ordered scan of the ties at the threshold, 1024 columns a round: g0 = 100 finds them in its
    first round; 3000 finds nothing in two whole rounds, then all 20 (the sampled route has fallen through to the radix route, as for
    1000); 1000 takes 24 from round 0 and 26 from round 1; (2500, 40, 2040), a short row that goes to the radix route directly, takes 8
    at the end of round 1 and 32 from round 2."""
    torch.manual_seed(M)
    fsd = O.fnn_init(16, [32], M)
    g0 = ties
    if g0 is not None:   # many experts share one weight row and bias -> identical probabilities
        fsd["layers.1.weight"][g0:g0 + 300] = fsd["layers.1.weight"][g0]; fsd["layers.1.bias"][g0:g0 + 300] = 3.0
    X = torch.randn(12, 16)
    f = _engine([16, 32, M], max_batch=12)
    f.load_state_dict(fsd); f.set_dense_input(X.numpy())
    p = f.forward(np.arange(12))
    if g0 is not None:
        grp = p[:, g0:g0 + 300].view(np.uint32)
        assert (grp == grp[:, :1]).all()                    # in every row the 300 members are bit-equal
        assert (p <= p[:, g0:g0 + 1]).all()                 # and no value is above the group's
    vals, idx = f.forward_topk(np.arange(12), K)
    for i in range(12):
        order = np.lexsort((np.arange(M), -p[i].astype(np.float64)))[:K]     # value desc, id asc
        assert np.array_equal(idx[i], order), i
        assert np.array_equal(vals[i], p[i][order])
        if g0 is not None:
            assert np.array_equal(idx[i], np.arange(g0, g0 + K)), i


@pytest.mark.parametrize("M", [40000, 300])
def test_topk_when_all_but_ten_probabilities_are_exactly_zero(M):
    """An output bias of -1e6 saturates the sigmoid: the last layer's leaky_relu (slope 0.01) leaves a logit of about -1e4, and
    1 / (1 + e^10000) is far below the smallest f32 denormal, so every expert but ten has probability exactly +0.0 (bit pattern 0, the
    smallest key of the radix selection) and the K-th place falls inside that tie group.
    The ten experts with a probability come first, by value; then the ten lowest ids among the zeros, each with value 0.0."""
    K = 20
    torch.manual_seed(M)
    fsd = O.fnn_init(16, [32], M)
    live = np.sort(np.random.default_rng(M).choice(np.arange(15, M), 10, replace=False))     # ids 0..14 stay zero: ten of them must follow
    bias = torch.full((M,), -1.0e6); bias[torch.from_numpy(live)] = 0.0
    fsd["layers.1.bias"] = bias
    X = torch.randn(12, 16)
    f = _engine([16, 32, M], max_batch=12)
    f.load_state_dict(fsd); f.set_dense_input(X.numpy())
    p = f.forward(np.arange(12))
    dead = np.setdiff1d(np.arange(M), live)
    assert not p[:, dead].view(np.uint32).any() and (p[:, live] > 0).all()                   # exactly +0.0, not a denormal, not -0.0
    vals, idx = f.forward_topk(np.arange(12), K)
    for i in range(12):
        order = live[np.lexsort((live, -p[i, live].astype(np.float64)))]
        assert np.array_equal(idx[i, :10], order), i
        assert np.array_equal(vals[i, :10], p[i, order]) and (vals[i, :10] > 0).all()
        assert np.array_equal(idx[i, 10:], np.arange(10)), (i, idx[i, 10:])
        assert not vals[i, 10:].view(np.uint32).any()


def test_topk_refuses_k_above_the_row_or_the_sort_capacity():
    from opentf_amd.libntf import NtfError
    f = _engine([16, 32, 40000], max_batch=4)
    f.load_state_dict(O.fnn_init(16, [32], 40000)); f.set_dense_input(np.zeros((4, 16), np.float32))
    assert f.forward_topk(np.arange(4), 2048)[1].shape == (4, 2048)
    with pytest.raises(NtfError):
        f.forward_topk(np.arange(4), 2049)           # above the LDS sort's capacity
    g = _engine([16, 32, 300], max_batch=4)
    g.load_state_dict(O.fnn_init(16, [32], 300)); g.set_dense_input(np.zeros((4, 16), np.float32))
    assert g.forward_topk(np.arange(4), 300)[1].shape == (4, 300)
    with pytest.raises(NtfError):
        g.forward_topk(np.arange(4), 301)            # K = M + 1
    with pytest.raises(NtfError):
        g.forward_topk(np.arange(4), 0)


def test_epoch_api_matches_step_api():
    sd, X, y = _bnn_case(16, [16], 90, 50, 1)
    fsd = O.fnn_init(16, [16], 90)
    def mk():
        e = _engine([16, 16, 90], max_batch=16, ns=2, nsd="uniform", seed=5)
        e.load_state_dict(fsd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy())); return e
    order = np.random.default_rng(0).permutation(50)
    a, b = mk(), mk()
    mean_a = a.train_epoch(order, 16)
    losses = [b.train_step(order[o:o + 16]) for o in range(0, 50, 16)]
    assert abs(mean_a - np.mean(losses)) <= 1e-6 * abs(mean_a)
    for k, v in a.state_dict().items():
        assert np.array_equal(v, b.state_dict()[k])
    assert abs(a.eval_epoch(order, 16) - np.mean([b.eval_step(order[o:o + 16]) for o in range(0, 50, 16)])) < 1e-5


def test_errors_are_reported_not_swallowed():
    from opentf_amd.libntf import NtfError
    e = _engine([8, 8, 20], max_batch=4)
    with pytest.raises(NtfError):
        e.train_step(np.arange(4))           # nothing resident yet
    e.set_dense_input(np.zeros((10, 8), np.float32)); e.set_member((np.arange(11), np.zeros(10, np.int32)))
    with pytest.raises(NtfError):
        e.train_step(np.arange(5))           # B > max_batch
    with pytest.raises(NtfError):
        e.train_step(np.array([0, 99]))      # row id out of range
    with pytest.raises(NtfError):
        e.set_member((np.array([0, 1]), np.array([20], np.int32)))  # column id out of range


# ------------------------------------------------------------------------------------------ eval-stage metrics
def test_device_ranking_metrics_match_committed_reference_results():
    """opentf_amd.evl.metric (device kernels through the C ABI) against the reference's committed pytrec_eval / skill-coverage
    per-instance tables for its own committed prediction files (tests/golden/g10_metrics.npz), and against the metric oracle."""
    from opentf_amd.evl import metric
    from oracle import metric_oracle as MO
    g = golden("g10_metrics")
    trec = ["P_2,5,10", "recall_2,5,10", "ndcg_cut_2,5,10", "map_cut_2,5,10", "success_2,5,10"]
    for name in [str(n) for n in g["names"]]:
        n, M, S = [int(v) for v in g[f"{name}.shape"]]
        Y = scipy.sparse.csr_matrix((np.ones(len(g[f"{name}.truth_indices"]), np.uint8), g[f"{name}.truth_indices"], g[f"{name}.truth_indptr"]), shape=(n, M))
        X = scipy.sparse.csr_matrix((np.ones(len(g[f"{name}.skill_indices"]), np.uint8), g[f"{name}.skill_indices"], g[f"{name}.skill_indptr"]), shape=(n, S))
        cov = scipy.sparse.csr_matrix((np.ones(len(g[f"{name}.cov_indices"]), np.uint8), g[f"{name}.cov_indices"], g[f"{name}.cov_indptr"]), shape=(M, S))
        yp = g[f"{name}.y_pred"]
        df, df_mean = metric.calculate_metrics(Y, yp, 1000, True, trec)
        dfc, dfc_mean = metric.calculate_skill_coverage(X, yp, cov, True, "2,5,10")
        got = np.concatenate([df.values, dfc.values], axis=1)
        assert list(df.columns) + list(dfc.columns) == [str(c) for c in g[f"{name}.columns"]]
        ties = any(len(np.unique(r)) < len(r) for r in yp)
        if not ties:  # equal scores are ranked differently by trec_eval (document name, descending)
            np.testing.assert_allclose(got, g[f"{name}.expected"], atol=6e-6, err_msg=name)
        np.testing.assert_allclose(df_mean["mean"].values, df.values.mean(0), rtol=1e-12)
        # sparse (top-K) prediction files give the same result as dense ones
        k = min(10, M)
        idx = np.argsort(-yp, axis=1, kind="stable")[:, :k]
        sparse_pred = scipy.sparse.csr_matrix((np.take_along_axis(yp, idx, 1).ravel(), idx.ravel(), np.arange(0, n * k + 1, k)), shape=(n, M))
        df2, _ = metric.calculate_metrics(Y, sparse_pred, 1000, True, trec)
        np.testing.assert_allclose(df2.values, df.values, atol=1e-7)


def test_engine_create_destroy_returns_device_memory():
    """The C ABI owns every device allocation behind the handle (ntf_engine_destroy frees all of it, lazily created buffers included)."""
    import gc
    torch.cuda.synchronize()
    sd, X, y = _bnn_case(64, [128], 20000, 64, 3)
    def cycle():
        e = _engine([64, 128, 20000], bayesian=True, max_batch=64, ns=3, nsd="unigram_b", fuse_adam=2)
        e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
        e.train_step(np.arange(64)); e.eval_step(np.arange(64)); e.forward_topk(np.arange(64), 10, nmc=2, uncertainty=True)
        del e; gc.collect()
    cycle(); torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(8): cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 << 20, (free0, free1)     # one engine of this shape holds ~250 MB


def test_fp16x3_saturates_instead_of_overflowing():
    """fp16x3 scales operands by exact powers of two before their fp16 split; values past the fp16 range saturate (documented) — no inf / NaN."""
    sd, X, y = _bnn_case(16, [128], 300, 20, 1)
    sd["layers.1.mu_weight"][5, :] = 1e4          # absurd weights (|w| >= 256 saturates)
    e = _engine([16, 128, 300], bayesian=True, max_batch=20, ns=3, nsd="uniform")
    e.load_state_dict(sd); e.set_dense_input((X * 1e3).numpy()); e.set_member(_csr_from_dense(y.numpy()))   # and activations in the thousands
    loss = e.train_step(np.arange(20))
    assert np.isfinite(loss)
    assert all(np.isfinite(v).all() for v in e.state_dict().values())
