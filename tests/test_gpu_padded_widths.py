"""The fused output layer at a last hidden width of 96, 160, 192 and 224: the exact-f32 MFMA kernels of the next fused width up (96 on H = 128's, the others on
H = 256's two-half forward, k_out_dh and the hidden-half dW + Adam kernel) run on rows narrower than their tile, in every mfma mode, on one GPU.  Parameter rows keep
exactly W floats; the padding exists only in the h operands and the dh slabs.  Against the oracle and against the engine's own other arms, as test_gpu_h256.py does
for 256 - plus a check that no kernel reads behind the end of a weight row (an inf planted in every other row would come back as a NaN)."""
import numpy as np
import pytest
import torch

from conftest import draw_noise
from oracle import ntf_oracle as O
from opentf_amd.synth import make_dataset, init_params
from test_gpu_ep import _mk
from test_gpu_parity import _engine, _rel, _close, _csr_from_dense, _bnn_case, RTOL_LOGITS

pytestmark = pytest.mark.gpu

WIDTHS = (96, 160, 192, 224)
GENERIC = ("out_fwd_gemm", "out_bwd_dw_gemm", "out_bwd_da_gemm")     # the generic chain's output-layer families (kFamNames)


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    """(as in test_gpu_h256.py) these tests seed and draw from the global generators: each hands them back as it found them"""
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


# ------------------------------------------------------------------------------------------ 1. the path taken
@pytest.mark.parametrize("mfma", [None, "f32"])
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("W", WIDTHS)
def test_train_step_runs_the_fused_kernels(W, bayesian, mfma):
    """[128, W, 20 000]: the fused path is taken - dW chunks exist, the step's calls are in the fused families, none in the generic GEMMs"""
    ds = make_dataset("dblp", d=128, seed=7, n_rows=600, n_experts=20_000)
    e = _mk(ds, [128, W, ds["M"]], bayesian, 256, "uniform", mfma=mfma)
    assert e.dw_chunks() > 0
    e.kernel_times(True)
    e.stage_order(np.arange(512, dtype=np.int64)); e.epoch_loss()
    e.step_staged(0, 256, train=True, apply=True)
    e.step_staged(256, 256, train=True, apply=True)
    kt = e.kernel_times(False)
    for fam in ("out_fused_fwd_loss_dh", "out_fused_dw_adam"):
        assert kt[fam][1] > 0, (fam, kt[fam])
    for fam in GENERIC:
        assert kt[fam][1] == 0, (fam, kt[fam])
    loss, steps = e.epoch_loss()
    assert steps == 2 and np.isfinite(loss)
    assert e.range_fallbacks() == 0
    e.close()


@pytest.mark.parametrize("mfma", [None, "f32"])
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("W", WIDTHS)
def test_inference_runs_the_fused_kernel(W, bayesian, mfma):
    """forward(nmc = 3), forward_topk and logits: calls of the fused forward family, none of the generic output GEMM (counted as test_gpu_infer_f32.py counts them)"""
    from test_gpu_infer_f32 import _family_calls
    got = _family_calls([128, W, 20_000], mfma, bayesian)
    for name, (fused, generic) in got.items():
        assert generic == 0 and fused > 0, (name, fused, generic)


# ------------------------------------------------------------------------------------------ 2. ragged steps against the oracle
def _inject(sd, y, bayesian):
    neg = O.ns_uniform(y, 5)
    inj = {"neg_idx": neg.numpy()}
    noise = draw_noise(sd, y.shape[0]) if bayesian else None
    if bayesian:
        inj.update({"eps_w": [n["eps_w"] for n in noise], "eps_b": [n["eps_b"] for n in noise], "s_in": [n["s_in"] for n in noise], "s_out": [n["s_out"] for n in noise]})
    return neg, noise, inj


# 96 on H = 128's kernels: one ragged expert tile, a single row, one expert into the last 32-expert stage under ragged row blocks; 160 / 192 / 224 on H = 256's: the
# second hidden half 32, 64 and 96 units wide (224 behind a second hidden layer); and the no-hidden-layer model whose dense INPUT has such a width (no d(hidden))
CASES = [(128, [96], 40, 129), (64, [96], 3000, 1), (128, [96], 70_001, 333), (64, [160], 3000, 129), (128, [192], 70_001, 129), (40, [64, 224], 3000, 129),
         (96, [], 3000, 129), (192, [], 70_001, 33)]


@pytest.mark.parametrize("D,H,M,B", CASES)
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("mfma", [None, "f32"])
def test_ragged_steps_vs_oracle_injected(D, H, M, B, bayesian, mfma):
    """two steps that continue from the engine's parameters: logits, evaluation loss, train loss, every gradient and the post-Adam state of each (the body and the
    tolerances of test_gpu_h256.py::test_ragged_256_steps_vs_oracle_injected)"""
    sd, X, y = _bnn_case(D, H, M, B, 5)
    if not bayesian:
        torch.manual_seed(5); sd = O.fnn_init(D, H, M)
    e = _engine([D] + H + [M], bayesian=bayesian, max_batch=B, ns=5, nsd="uniform", lr=1e-3, mfma=mfma)
    assert e.dw_chunks() > 0
    e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
    rows = np.arange(B)
    opt = O.Adam(sd, 1e-3)
    for s in range(2):
        neg, noise, inj = _inject(sd, y, bayesian)
        sd_e = {k: torch.from_numpy(v) for k, v in e.state_dict().items()}
        ref_logits = (O.bnn_forward(sd_e, X, noise) if bayesian else O.fnn_forward(sd_e, X)).detach().numpy()
        got = e.logits(rows, inject=inj)
        assert _rel(got, ref_logits) < RTOL_LOGITS
        ref_eval = float(O.batch_loss(sd, X, y, neg, 10.0, 1.0, noise))
        assert abs(e.eval_step(rows, inject=inj) - ref_eval) <= 2e-5 * abs(ref_eval)
        ref_loss, ref_grads = O.train_step(sd, opt, X, y, neg, 10.0, 1.0, noise)
        loss = e.train_step(rows, inject=inj)
        assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (s, loss, ref_loss)
        grads, state = e.grads(), e.state_dict()
        last = f"layers.{len(H)}."
        for k in sd:
            ref = ref_grads[k].numpy()
            assert grads[k].shape == ref.shape, (k, grads[k].shape)
            if k.startswith(last):
                # a z within rounding of 0 lands on the other side of leaky_relu's kink in another summation order: that (row, expert) pair moves its expert's gradient row
                d = np.abs(grads[k] - ref)
                assert int((d > 3e-4 * float(np.abs(ref).max())).sum()) <= 4 * (ref.shape[1] if ref.ndim == 2 else 1), (s, k)
            else:
                assert _rel(grads[k], ref) < 3e-4, (s, k, _rel(grads[k], ref))
            bad = np.abs(state[k] - sd[k].numpy()) > (1e-3 * np.abs(sd[k].numpy()) + 2e-5)
            assert float(bad.mean()) <= 2e-4, (s, k, float(bad.mean()))     # (Adam's first step: where |g| ~ 1e-8 a rounding difference flips the update)
        with torch.no_grad():       # both sides continue from the engine's parameters (a leaky_relu' kink flip must not compound)
            for k in sd: sd[k].copy_(torch.from_numpy(state[k]))
    assert e.range_fallbacks() == 0
    e.close()


# ------------------------------------------------------------------------------------------ 3. nothing behind a row's end is read
@pytest.mark.parametrize("W", (96, 160, 224))
def test_fnn_logits_do_not_read_the_next_weight_row(W):
    """every odd expert's weight row and bias are +inf.  An even expert's logit does not depend on them; a kernel that fetched a full tile row at the real stride would
    multiply its zero h columns by the next (odd) row's inf: NaN"""
    D, M, B = 64, 2001, 33
    torch.manual_seed(11)
    sd = O.fnn_init(D, [W], M)
    X = torch.randn(B, D)
    ref = O.fnn_forward(sd, X).detach().numpy()
    bad = {k: v.clone() for k, v in sd.items()}
    bad["layers.1.weight"][1::2] = float("inf"); bad["layers.1.bias"][1::2] = float("inf")
    e = _engine([D, W, M], bayesian=False, max_batch=B, ns=5, nsd="uniform")
    e.load_state_dict(bad); e.set_dense_input(X.numpy())
    got = e.logits(np.arange(B))[:, 0::2]
    e.close()
    assert np.isfinite(got).all()
    assert _rel(got, ref[:, 0::2]) < RTOL_LOGITS


@pytest.mark.parametrize("W", (96, 160, 224))
def test_bnn_logits_do_not_read_the_next_perturbation_row(W):
    """the same read through the sigma * eps operand: the injected eps_w of the output layer is +inf on every odd expert's row"""
    D, M, B = 64, 2001, 33
    sd, X, _ = _bnn_case(D, [W], M, B, 12)
    noise = draw_noise(sd, B)
    ref = O.bnn_forward(sd, X, noise).detach().numpy()
    eps_w = [n["eps_w"].clone() for n in noise]
    eps_w[1][1::2] = float("inf")
    inj = {"eps_w": eps_w, "eps_b": [n["eps_b"] for n in noise], "s_in": [n["s_in"] for n in noise], "s_out": [n["s_out"] for n in noise]}
    e = _engine([D, W, M], bayesian=True, max_batch=B, ns=5, nsd="uniform")
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    got = e.logits(np.arange(B), inject=inj)[:, 0::2]
    e.close()
    assert np.isfinite(got).all()
    assert _rel(got, ref[:, 0::2]) < RTOL_LOGITS


# ------------------------------------------------------------------------------------------ 4. multi-hot input
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("W", (96, 192))
def test_multihot_input_vs_oracle(W, bayesian):
    """multi-hot input (the first layer a CSR gather-sum) under a 96- / 192-wide hidden layer"""
    from opentf_amd import libntf
    S, H, M, B = 700, [W], 3000, 129
    torch.manual_seed(3)
    sd = O.bnn_init(S, H, M) if bayesian else O.fnn_init(S, H, M)
    rng = np.random.default_rng(S)
    Xd = np.zeros((B, S), np.float32)
    for i in range(B):
        Xd[i, rng.choice(S, 1 + rng.poisson(7.5), replace=False)] = 1
    X = torch.from_numpy(Xd)
    y = (torch.rand(B, M) < 0.01).float(); y[torch.arange(B), torch.randint(0, M, (B,))] = 1
    e = _engine([S] + H + [M], bayesian=bayesian, input_mode=libntf.INPUT_MULTIHOT, max_batch=B, ns=5, nsd="uniform", lr=1e-3)
    assert e.dw_chunks() > 0
    e.load_state_dict(sd); e.set_skill_csr(_csr_from_dense(Xd)); e.set_member(_csr_from_dense(y.numpy()))
    rows = np.arange(B)
    opt = O.Adam(sd, 1e-3)
    for s in range(2):
        neg, noise, inj = _inject(sd, y, bayesian)
        ref_loss, ref_grads = O.train_step(sd, opt, X, y, neg, 10.0, 1.0, noise)
        loss = e.train_step(rows, inject=inj)
        assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
        grads, state = e.grads(), e.state_dict()
        for k in sd:
            assert _rel(grads[k], ref_grads[k].numpy()) < 3e-4, (s, k, _rel(grads[k], ref_grads[k].numpy()))
            _close(state[k], sd[k].numpy(), 1e-3, 2e-5)
        with torch.no_grad():
            for k in sd: sd[k].copy_(torch.from_numpy(state[k]))
    e.close()


# ------------------------------------------------------------------------------------------ 5. fuse_adam modes
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("W", (96, 192))
def test_fuse_adam_modes_agree(W, bayesian):
    """Adam of the output layer in the dW epilogue (1), as a flat kernel (0) or per chunk on a side stream (2): the same parameters"""
    sd, X, y = _bnn_case(64, [W], 900, 150, 3)
    if not bayesian:
        torch.manual_seed(3); sd = O.fnn_init(64, [W], 900)

    def run(fuse):
        e = _engine([64, W, 900], bayesian=bayesian, max_batch=150, ns=4, nsd="uniform", seed=21, lr=1e-2, fuse_adam=fuse)
        assert e.dw_chunks() > 0
        e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
        losses = [e.train_step(np.arange(150)) for _ in range(4)]
        out = losses, e.state_dict(); e.close()
        return out
    (la, pa), (lb, pb), (lc, pc) = run(0), run(1), run(2)
    np.testing.assert_allclose(la, lb, rtol=1e-6); np.testing.assert_allclose(la, lc, rtol=1e-6)
    for k in pa:
        np.testing.assert_allclose(pa[k], pb[k], rtol=1e-5, atol=1e-7)
        assert np.array_equal(pa[k], pc[k]), k


# ------------------------------------------------------------------------------------------ 6. deferred dW chunks
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("W", (96, 224))
def test_dp_dw_chunks_equal_the_whole_step(W, bayesian):
    """a data-parallel rank's step: ntf_step_staged_deferred, every dW chunk, then Adam - the parameters of the plain step on the same native draws, bit for bit"""
    from opentf_amd import libntf
    from opentf_amd.synth import zipf_csr
    M, S, N, B = 66_000, 3_000, 2_000, 300     # 2 dW chunks of 65 536 experts, the second one ragged
    s_ip, s_ix = zipf_csr(N, S, 8.57, 1); m_ip, m_ix = zipf_csr(N, M, 3.06, 2)
    table = np.random.default_rng(0).standard_normal((S, 128), dtype=np.float32)
    dims = [128, W, M]
    sd = init_params(dims, bayesian, 0)
    order = np.random.default_rng(1).integers(0, N, 2 * B)

    def mk():
        e = libntf.Engine(dims, bayesian=bayesian, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd="uniform", seed=5, fuse_adam=0)
        e.set_skill_table(table); e.set_skill_csr((s_ip, s_ix)); e.set_member((m_ip, m_ix)); e.load_state_dict(sd)
        e.stage_order(order); e.epoch_loss()
        return e
    ref = mk()
    for s in range(2): ref.step_staged(s * B, B, train=True, apply=True)
    p_ref = ref.state_dict(); l_ref = ref.epoch_loss(); ref.close()
    e = mk()
    n = e.dw_chunks()
    assert n == 2
    for s in range(2):
        e.step_staged_deferred(s * B, B, s * B, B)
        for k in range(n): e.dw_chunk(k)
        e.apply()
    p = e.state_dict()
    assert e.epoch_loss() == l_ref
    for k in p_ref: assert np.array_equal(p[k], p_ref[k]), k
    e.close()


# ------------------------------------------------------------------------------------------ 7. native draws
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("W", (96, 192))
def test_three_native_steps_replayed_through_the_oracle(W, bayesian):
    """the non-injected kernels (hashed signs, Philox eps) on a ragged shape, replayed through the oracle from the device's own draws"""
    from test_gpu_replay import _replay
    _replay(D=128, H=W, M=70_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=24, t0=9, bayesian=bayesian, pipelined=False)


@pytest.mark.parametrize("W", (96, 192))
def test_exported_draws_have_the_real_width(W):
    """ntf_get_noise: eps_w [M, W] and s_in [B, W] of the output layer - the real width, not the kernels' tile"""
    D, M, B = 64, 2001, 33
    sd, X, _ = _bnn_case(D, [W], M, B, 13)
    e = _engine([D, W, M], bayesian=True, max_batch=B, ns=5, nsd="uniform", seed=3)
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    e.set_seed(3, 4)
    got = e.logits(np.arange(B))
    noise = e.noise(4, B)
    e.close()
    assert noise[1]["eps_w"].shape == (M, W) and noise[1]["s_in"].shape == (B, W) and noise[1]["s_out"].shape == (B, M)
    ref = O.bnn_forward(sd, X, [{k: torch.from_numpy(v) for k, v in n.items()} for n in noise]).detach().numpy()
    assert _rel(got, ref) < RTOL_LOGITS


# ------------------------------------------------------------------------------------------ 8. layout
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("W", (96, 224))
def test_parameter_layout_is_unpadded(W, bayesian):
    """state_dict() and grads() return [M, W] arrays; load_state_dict followed by state_dict is the identity"""
    D, M, B = 64, 900, 40
    sd, X, y = _bnn_case(D, [W], M, B, 14)
    if not bayesian:
        torch.manual_seed(14); sd = O.fnn_init(D, [W], M)
    e = _engine([D, W, M], bayesian=bayesian, max_batch=B, ns=5, nsd="uniform", fuse_adam=0)
    e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
    st = e.state_dict()
    assert set(st) == set(sd)
    for k in sd:
        assert st[k].shape == tuple(sd[k].shape), k
        assert np.array_equal(st[k], sd[k].numpy()), k
    wkey = "layers.1.mu_weight" if bayesian else "layers.1.weight"
    assert st[wkey].shape == (M, W)
    e.train_step(np.arange(B))
    g = e.grads()
    for k in sd: assert g[k].shape == tuple(sd[k].shape), k
    assert g[wkey].shape == (M, W) and np.isfinite(g[wkey]).all() and float(np.abs(g[wkey]).max()) > 0
    e.close()
