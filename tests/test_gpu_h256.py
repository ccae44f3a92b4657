"""The fused output layer at a last hidden width of 256: exact-f32 MFMA kernels (forward + loss + dz, the separate d(hidden) kernel k_out_dh, the
hidden-half dW + Adam kernel) in every mfma mode, on one GPU, on expert shards and through the data-parallel dW chunks - against the oracle and
against the engine's own single-GPU step."""
import numpy as np
import pytest
import torch

from conftest import draw_noise
from oracle import ntf_oracle as O
from opentf_amd.ep import expert_shards
from opentf_amd.synth import make_dataset, init_params
from test_gpu_ep import _mk, _ep_epoch, _full_epoch, _gathered
from test_gpu_parity import _engine, _rel, _close, _csr_from_dense, _bnn_case, RTOL_LOGITS

pytestmark = pytest.mark.gpu

GENERIC = ("out_fwd_gemm", "out_bwd_dw_gemm", "out_bwd_da_gemm")     # the generic chain's output-layer families (kFamNames)


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    """these tests draw from torch's (and numpy's, Python's) global generators - seeding them, drawing oracle noise and negatives.  Later modules of the
    suite draw from the same generators without seeding them (e.g. the node2vec plugin's initial table and batch order, as the reference's code does):
    each test here hands them back in the state it found them, so that adding this module does not change what any other test draws."""
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


@pytest.mark.parametrize("mfma", [None, "f32"])
@pytest.mark.parametrize("bayesian", [True, False])
def test_h256_train_step_runs_the_fused_kernels(bayesian, mfma):
    """[128, 256, 20 000]: the fused path is taken (dW chunks exist; the step's time is in the fused families, none in the generic GEMMs), and the
    split-product range guard never fires at this width.  (The "loss" family also holds the fused step's loss reduction: it tells nothing here.)"""
    ds = make_dataset("dblp", d=128, seed=7, n_rows=600, n_experts=20_000)
    e = _mk(ds, [128, 256, ds["M"]], bayesian, 256, "uniform", mfma=mfma)
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
    e.close()


@pytest.mark.parametrize("G", [2, 3])
def test_expert_shards_at_256_compute_the_single_engine_step(G):
    """expert shards (two-phase step, d(hidden) summed on the host) of a [128, 256, M] Bnn: the single engine's loss and parameters (and Adam moments through
    them) after a step and a short epoch, its evaluation loss, and its inference columns"""
    B = 256
    ds = make_dataset("dblp", d=128, seed=3, n_rows=1500, n_experts=3000)
    dims = [128, 256, ds["M"]]
    order = np.random.default_rng(4).permutation(ds["N"])[: 2 * B + 77].astype(np.int64)
    shards = expert_shards(ds["M"], G)
    full = _mk(ds, dims, True, B, "uniform")
    eng = [_mk(ds, dims, True, B, "uniform", shard=s, world=G) for s in shards]
    l_full = _full_epoch(full, order[:B], B); l_ep = _ep_epoch(eng, order[:B], B)
    assert abs(l_ep - l_full) <= 2e-6 * abs(l_full), (l_ep, l_full)
    a, b = _gathered(eng), full.state_dict()
    for k in b:
        if k.startswith("layers.1."): assert np.array_equal(a[k], b[k]), f"{k}: the shards' first update differs from the single engine's"
        # (the hidden layers: d(hidden) is summed in another order, and Adam's first step divides by |g| - a last-bit difference shows where g ~ 0)
        else: np.testing.assert_allclose(a[k], b[k], rtol=1e-4, atol=2e-5, err_msg=k)
    l_full = _full_epoch(full, order, B); l_ep = _ep_epoch(eng, order, B)
    assert abs(l_ep - l_full) <= 1e-5 * abs(l_full), (l_ep, l_full)
    a, b = _gathered(eng), full.state_dict()
    for k in b:
        bad = ~np.isclose(a[k], b[k], rtol=1e-4, atol=2e-5)
        assert bad.sum() <= max(1, a[k].size // 50_000), (k, int(bad.sum()), a[k].size)
        np.testing.assert_allclose(a[k], b[k], rtol=1e-4, atol=3 * 1e-3 * 0.1, err_msg=k)
    v_full = _full_epoch(full, order[:300], B, train=False); v_ep = _ep_epoch(eng, order[:300], B, train=False)
    assert abs(v_ep - v_full) <= 1e-5 * abs(v_full), (v_ep, v_full)
    rows = order[:200]
    z_full = full.logits(rows)
    z = np.concatenate([e.logits(rows) for e in eng], axis=1)
    assert z.shape == z_full.shape
    np.testing.assert_allclose(z, z_full, rtol=1e-5, atol=2e-6)      # (inference at 256 runs the generic GEMM, whose tiling follows the shard's width)
    for e in eng + [full]: e.close()


@pytest.mark.parametrize("bayesian", [True, False])
def test_dp_dw_chunks_at_256_equal_the_whole_step(bayesian):
    """a data-parallel rank's step: ntf_step_staged_deferred, every dW chunk, then Adam - the parameters of the plain step on the same native draws, bit for bit"""
    from opentf_amd import libntf
    from opentf_amd.synth import zipf_csr
    M, S, N, B = 140_000, 3_000, 2_000, 300     # 3 dW chunks of 65 536 experts, the last one ragged
    s_ip, s_ix = zipf_csr(N, S, 8.57, 1); m_ip, m_ix = zipf_csr(N, M, 3.06, 2)
    table = np.random.default_rng(0).standard_normal((S, 128), dtype=np.float32)
    dims = [128, 256, M]
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
    assert n == 3
    for s in range(2):
        e.step_staged_deferred(s * B, B, s * B, B)
        for k in range(n): e.dw_chunk(k)
        e.apply()
    p = e.state_dict()
    assert e.epoch_loss() == l_ref
    for k in p_ref: assert np.array_equal(p[k], p_ref[k]), k
    e.close()


@pytest.mark.parametrize("bayesian", [True, False])
def test_config2_full_size_step_at_256_against_the_oracle(bayesian):
    """config 2's shapes with h = [256]: logits, loss, every gradient and the post-Adam parameters against the oracle (tolerances of _full_size_oracle_step)"""
    from test_gpu_round3 import _full_size_oracle_step
    _full_size_oracle_step(D=128, H=256, M=233_629, B=1000, S=4000, mean_s=8.57, mean_m=3.06, seed=31 if bayesian else 32, bayesian=bayesian)


def _inject(sd, y, bayesian):
    neg = O.ns_uniform(y, 5)
    inj = {"neg_idx": neg.numpy()}
    noise = draw_noise(sd, y.shape[0]) if bayesian else None
    if bayesian:
        inj.update({"eps_w": [n["eps_w"] for n in noise], "eps_b": [n["eps_b"] for n in noise], "s_in": [n["s_in"] for n in noise], "s_out": [n["s_out"] for n in noise]})
    return neg, noise, inj


# ragged last expert tiles (M = 40: one tile, fewer than a column group; 3000; 70 001: one expert into the last 32-expert stage), ragged row blocks, a second hidden
# layer, and the no-hidden-layer model whose INPUT is 256 wide (dense input: it runs the same fused kernels, without d(hidden))
CASES = [(128, [256], 40, 129), (64, [256], 3000, 1), (128, [256], 70_001, 333), (40, [64, 256], 3000, 129), (256, [], 3000, 129), (256, [], 70_001, 33)]


@pytest.mark.parametrize("D,H,M,B", CASES)
@pytest.mark.parametrize("bayesian", [True, False])
@pytest.mark.parametrize("mfma", [None, "f32"])
def test_ragged_256_steps_vs_oracle_injected(D, H, M, B, bayesian, mfma):
    sd, X, y = _bnn_case(D, H, M, B, 5)
    if not bayesian:
        torch.manual_seed(5); sd = O.fnn_init(D, H, M)
    e = _engine([D] + H + [M], bayesian=bayesian, max_batch=B, ns=5, nsd="uniform", lr=1e-3, mfma=mfma)
    if not H: assert e.dw_chunks() > 0          # (a [256, M] model takes the fused path)
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
            if k.startswith(last):
                # with B x M up to 2.3e7 logits, a z within rounding of 0 lands on the other side of leaky_relu's kink in another summation order: that (row, expert)
                # pair moves its expert's gradient row (as _full_size_oracle_step allows at config 2's size)
                d = np.abs(grads[k] - ref)
                assert int((d > 3e-4 * float(np.abs(ref).max())).sum()) <= 4 * (ref.shape[1] if ref.ndim == 2 else 1), (s, k)
            else:
                assert _rel(grads[k], ref) < 3e-4, (s, k, _rel(grads[k], ref))
            bad = np.abs(state[k] - sd[k].numpy()) > (1e-3 * np.abs(sd[k].numpy()) + 2e-5)
            assert float(bad.mean()) <= 2e-4, (s, k, float(bad.mean()))     # (Adam's first step: where |g| ~ 1e-8 a rounding difference flips the update)
        with torch.no_grad():       # both sides continue from the engine's parameters (a leaky_relu' kink flip must not compound)
            for k in sd: sd[k].copy_(torch.from_numpy(state[k]))
    e.close()


@pytest.mark.parametrize("bayesian", [True, False])
def test_multihot_input_at_256_vs_oracle(bayesian):
    """multi-hot input (the first layer a CSR gather-sum) under a 256-wide hidden layer"""
    from opentf_amd import libntf
    S, H, M, B = 700, [256], 3000, 129
    torch.manual_seed(3)
    sd = O.bnn_init(S, H, M) if bayesian else O.fnn_init(S, H, M)
    rng = np.random.default_rng(S)
    Xd = np.zeros((B, S), np.float32)
    for i in range(B):
        Xd[i, rng.choice(S, 1 + rng.poisson(7.5), replace=False)] = 1
    X = torch.from_numpy(Xd)
    y = (torch.rand(B, M) < 0.01).float(); y[torch.arange(B), torch.randint(0, M, (B,))] = 1
    e = _engine([S] + H + [M], bayesian=bayesian, input_mode=libntf.INPUT_MULTIHOT, max_batch=B, ns=5, nsd="uniform", lr=1e-3)
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


def test_multihot_input_without_a_hidden_layer_is_refused_at_256():
    """[S = 256, M] with multi-hot input has no hidden layer to gather into: the engine refuses it (as at every width), it does not reach the fused kernels"""
    from opentf_amd import libntf
    with pytest.raises(libntf.NtfError, match="hidden layer"):
        libntf.Engine([256, 3000], bayesian=True, input_mode=libntf.INPUT_MULTIHOT, max_batch=64, ns=5, nsd="uniform")


@pytest.mark.parametrize("bayesian", [True, False])
def test_fuse_adam_modes_agree_at_256(bayesian):
    """Adam of the output layer in the dW epilogue (1), as a flat kernel (0) or per chunk on a side stream (2): the same parameters"""
    sd, X, y = _bnn_case(64, [256], 900, 150, 3)
    if not bayesian:
        torch.manual_seed(3); sd = O.fnn_init(64, [256], 900)

    def run(fuse):
        e = _engine([64, 256, 900], bayesian=bayesian, max_batch=150, ns=4, nsd="uniform", seed=21, lr=1e-2, fuse_adam=fuse)
        e.load_state_dict(sd); e.set_dense_input(X.numpy()); e.set_member(_csr_from_dense(y.numpy()))
        losses = [e.train_step(np.arange(150)) for _ in range(4)]
        out = losses, e.state_dict(); e.close()
        return out
    (la, pa), (lb, pb), (lc, pc) = run(0), run(1), run(2)
    np.testing.assert_allclose(la, lb, rtol=1e-6); np.testing.assert_allclose(la, lc, rtol=1e-6)
    for k in pa:
        np.testing.assert_allclose(pa[k], pb[k], rtol=1e-5, atol=1e-7)
        assert np.array_equal(pa[k], pc[k]), k


@pytest.mark.parametrize("bayesian", [True, False])
def test_three_native_steps_at_256_replayed_through_the_oracle(bayesian):
    """the non-injected kernels (hashed signs, Philox eps) at h = [256] on a ragged shape, replayed through the oracle from the device's own draws"""
    from test_gpu_replay import _replay
    _replay(D=128, H=256, M=70_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=24, t0=9, bayesian=bayesian, pipelined=False)
