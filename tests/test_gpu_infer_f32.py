"""Inference (ntf_forward, ntf_forward_topk, ntf_logits) on the exact-f32 fused kernel k_out_probs at every fused last hidden width - 32, 64, 256, 128 with
mfma = 'f32', and 128 on the default arithmetic behind a raised range flag: the path taken (kernel families), the oracle with every MC pass's noise injected, the
device's own draws replayed, expert shards against the whole engine, and the generic chain (NTF_INFER_F32=0, read when the engine is created) as the other arm."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PATH_CASES = [([128, 256, 20_000], None), ([64, 64, 3000], None), ([64, 32, 3000], None), ([128, 128, 20_000], "f32")]
FUSED, GENERIC = "out_fused_fwd_loss_dh", "out_fwd_gemm"


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    """(as in test_gpu_h256.py) these tests seed and draw from the global generators: each hands them back as it found them"""
    import random
    import torch
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


def _family_calls(dims, mfma, bayesian):
    """calls of the fused forward family and of the generic output GEMM around forward(nmc = 3), forward_topk and logits"""
    from opentf_amd.synth import make_dataset
    from test_gpu_ep import _mk
    ds = make_dataset("dblp", d=dims[0], seed=7, n_rows=400, n_experts=dims[-1])
    e = _mk(ds, dims[:-1] + [ds["M"]], bayesian, 200, "uniform", mfma=mfma)
    rows = np.arange(200, dtype=np.int64)
    out = {}
    for name, call in (("forward", lambda: e.forward(rows, nmc=3)), ("forward_topk", lambda: e.forward_topk(rows, 10, nmc=3)), ("logits", lambda: e.logits(rows))):
        e.kernel_times(True)
        call()
        kt = e.kernel_times(False)
        out[name] = [int(kt[FUSED][1]), int(kt[GENERIC][1])]
    assert e.range_fallbacks() == 0
    e.close()
    return out


def _child_main():
    """the other arm, in a process of its own (the switch is read when an engine is created; the parent's environment stays as it is)"""
    res = []
    for dims, mfma in PATH_CASES:
        for bayesian in (False, True):
            res.append(_family_calls(list(dims), mfma, bayesian))
    print("RESULT " + json.dumps(res))


@pytest.mark.parametrize("bayesian", [False, True])
@pytest.mark.parametrize("dims,mfma", PATH_CASES)
def test_inference_runs_the_fused_f32_kernel(dims, mfma, bayesian):
    got = _family_calls(list(dims), mfma, bayesian)
    for name, (fused, generic) in got.items():
        assert generic == 0 and fused > 0, (name, fused, generic)


def test_switch_off_runs_the_generic_chain_in_a_fresh_process():
    env = dict(os.environ); env["NTF_INFER_F32"] = "0"
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert len(res) == 2 * len(PATH_CASES)
    for got in res:
        for name, (fused, generic) in got.items():
            assert fused == 0 and generic > 0, (name, fused, generic)


# ------------------------------------------------------------------------------------------ oracle parity, every pass's noise injected (tolerances of
# test_gpu_round3.py::test_config2_full_size_inference_against_the_oracle, the logits at RTOL_LOGITS)
def _injects(sd, B, nmc):
    from conftest import draw_noise
    noises = [draw_noise(sd, B) for _ in range(nmc)]
    injs = [{"eps_w": [n["eps_w"] for n in nz], "eps_b": [n["eps_b"] for n in nz], "s_in": [n["s_in"] for n in nz], "s_out": [n["s_out"] for n in nz]} for nz in noises]
    return noises, injs


def _check_against_oracle(e, sd, X, bayesian, nmc, expect_fallbacks=0, big_col=None):
    """logits, MC-mean probabilities, predictive entropy, mutual information and (deterministic model) the device top-K of engine e against the oracle on X"""
    from oracle import ntf_oracle as O
    from test_gpu_parity import _rel, RTOL_LOGITS
    B = X.shape[0]
    rows = np.arange(B)
    if not bayesian: nmc = 1
    noises, injs = _injects(sd, B, nmc) if bayesian else (None, None)
    f0 = e.range_fallbacks()
    e.kernel_times(True)
    ref_logits = O.model_forward(sd, X, noises[0] if bayesian else None).detach().numpy()
    got = e.logits(rows, inject=injs[0] if bayesian else None)
    print("logits rel", _rel(got, ref_logits))
    assert e.range_fallbacks() - f0 == expect_fallbacks
    assert _rel(got, ref_logits) < RTOL_LOGITS
    if big_col is not None:      # one huge column sets the scale of the bar above: the other columns element by element (test_gpu_parity's logit tolerances)
        keep = np.arange(ref_logits.shape[1]) != big_col
        print("logits without the big column: max abs err", float(np.abs(got[:, keep] - ref_logits[:, keep]).max()))
        np.testing.assert_allclose(got[:, keep], ref_logits[:, keep], rtol=RTOL_LOGITS, atol=2e-6)
    mc = O.predict(sd, X, nmc, noises).numpy()
    mc = mc if mc.ndim == 3 else mc[None]
    probs, pu, mu = e.forward(rows, nmc=nmc, injects=injs, uncertainty=True)
    assert e.range_fallbacks() - f0 == 2 * expect_fallbacks
    print("probs max abs err", float(np.abs(probs - mc.mean(0)).max()), "pu", float(np.abs(pu - O.predictive_entropy(mc)).max()),
          "mu", float(np.abs(mu - O.mutual_information(mc)).max()))
    np.testing.assert_allclose(probs, mc.mean(0), rtol=1e-5, atol=2e-7)
    np.testing.assert_allclose(pu, O.predictive_entropy(mc), rtol=1e-4, atol=1e-4)
    if bayesian: np.testing.assert_allclose(mu, O.mutual_information(mc), rtol=1e-3, atol=2e-4)
    else:
        K = min(100, probs.shape[1])
        vals, idx = e.forward_topk(rows, K, nmc=1)
        order = np.argsort(-probs, axis=1, kind="stable")[:, :K]
        assert np.array_equal(idx, order) and np.array_equal(vals, np.take_along_axis(probs, order, axis=1))
    kt = e.kernel_times(False)
    assert kt[GENERIC][1] == 0 and kt[FUSED][1] > 0, (kt[GENERIC], kt[FUSED])


# ragged last expert tiles and row blocks, one row, a second hidden layer, the no-hidden-layer model whose dense input is 256 wide, the narrow widths
SHAPES = [(128, [256], 70_001, 333), (64, [256], 3000, 1), (40, [64, 256], 3000, 129), (256, [], 3000, 129), (24, [64], 777, 129), (16, [32], 63, 257)]


@pytest.mark.parametrize("D,H,M,B", SHAPES)
@pytest.mark.parametrize("bayesian", [True, False])
def test_inference_vs_oracle_injected(D, H, M, B, bayesian):
    import torch
    from oracle import ntf_oracle as O
    from test_gpu_parity import _engine, _bnn_case
    sd, X, _ = _bnn_case(D, H, M, B, 5)
    if not bayesian:
        torch.manual_seed(5); sd = O.fnn_init(D, H, M)
    e = _engine([D] + H + [M], bayesian=bayesian, max_batch=B, ns=5, nsd="uniform", lr=1e-3)
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    _check_against_oracle(e, sd, X, bayesian, 3)
    e.close()


@pytest.mark.parametrize("bayesian", [True, False])
def test_multihot_inference_at_256_vs_oracle(bayesian):
    import torch
    from opentf_amd import libntf
    from oracle import ntf_oracle as O
    from test_gpu_parity import _engine, _csr_from_dense
    S, H, M, B = 700, [256], 3000, 129
    torch.manual_seed(3)
    sd = O.bnn_init(S, H, M) if bayesian else O.fnn_init(S, H, M)
    rng = np.random.default_rng(S)
    Xd = np.zeros((B, S), np.float32)
    for i in range(B):
        Xd[i, rng.choice(S, 1 + rng.poisson(7.5), replace=False)] = 1
    e = _engine([S] + H + [M], bayesian=bayesian, input_mode=libntf.INPUT_MULTIHOT, max_batch=B, ns=5, nsd="uniform", lr=1e-3)
    e.load_state_dict(sd); e.set_skill_csr(_csr_from_dense(Xd))
    _check_against_oracle(e, sd, torch.from_numpy(Xd), bayesian, 3)
    e.close()


@pytest.mark.parametrize("bayesian", [True, False])
def test_config2_size_inference_at_256_vs_oracle(bayesian):
    """config 2's shapes with h = [256]: B = 1000 teams a call, two MC passes (the oracle's [nmc, B, M] tensor and each injected s_out are 0.9 GB a pass)"""
    import torch
    from opentf_amd import libntf
    from oracle import ntf_oracle as O
    from test_gpu_round3 import _host_gib_available
    if _host_gib_available() < 40: pytest.skip("needs ~25 GB of host memory for the oracle's dense tensors")
    D, H, M, B, S = 128, 256, 233_629, 1000, 4000
    torch.manual_seed(41)
    rng = np.random.default_rng(41)
    sd = O.bnn_init(D, [H], M) if bayesian else O.fnn_init(D, [H], M)
    table = rng.standard_normal((S, D)).astype(np.float32)
    nnz = 1 + rng.poisson(7.57, B)
    s_ip = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
    s_ix = np.concatenate([np.sort(rng.choice(S, k, replace=False)) for k in nnz]).astype(np.int32)
    X = torch.from_numpy(O.gather_meanpool_fast(s_ip, s_ix, table))
    e = libntf.Engine([D, H, M], bayesian=bayesian, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd="uniform", tpw=10.0, tnw=1.0, lr=1e-3)
    e.set_skill_table(table); e.set_skill_csr((s_ip, s_ix)); e.load_state_dict(sd)
    _check_against_oracle(e, sd, X, bayesian, 2)
    e.close()


# ------------------------------------------------------------------------------------------ native draws
def test_native_forward_at_256_replayed_through_the_oracle():
    """the non-injected kernel (hashed signs, Philox eps) on a ragged shape: forward(nmc = 3) consumes the step indices t0 .. t0 + 2, whose draws ntf_get_noise exports"""
    import torch
    from oracle import ntf_oracle as O
    from test_gpu_parity import _engine, _bnn_case
    D, H, M, B, t0, nmc = 128, [256], 70_001, 129, 17, 3
    sd, X, _ = _bnn_case(D, H, M, B, 9)
    e = _engine([D] + H + [M], bayesian=True, max_batch=B, ns=5, nsd="uniform", lr=1e-3, seed=9)
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    e.set_seed(9, t0)
    probs, pu, mu = e.forward(np.arange(B), nmc=nmc, uncertainty=True)
    noises = [[{k: torch.from_numpy(v) for k, v in n.items()} for n in e.noise(t0 + p, B)] for p in range(nmc)]
    e.close()
    mc = O.predict(sd, X, nmc, noises).numpy()
    print("probs max abs err", float(np.abs(probs - mc.mean(0)).max()))
    np.testing.assert_allclose(probs, mc.mean(0), rtol=1e-5, atol=2e-7)
    np.testing.assert_allclose(pu, O.predictive_entropy(mc), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(mu, O.mutual_information(mc), rtol=1e-3, atol=2e-4)


# ------------------------------------------------------------------------------------------ expert shards
@pytest.mark.parametrize("G", [2, 3])
def test_expert_shards_at_256_infer_the_whole_engines_columns(G):
    """the fused kernel's per-expert dot product does not depend on the shard's width, and signs / eps are keyed by global expert ids: bit for bit.  The entropies are sums
    over the experts: the shards' add up to the whole engine's, to the rounding of f32 sums taken in another order (2e-6, the bar test_gpu_ep.py sets for the shards' loss sums)"""
    from opentf_amd.ep import expert_shards
    from opentf_amd.synth import make_dataset
    from test_gpu_ep import _mk
    B, nmc = 200, 3
    ds = make_dataset("dblp", d=128, seed=3, n_rows=600, n_experts=3000)
    dims = [128, 256, ds["M"]]
    rows = np.arange(B, dtype=np.int64)
    full = _mk(ds, dims, True, B, "uniform")
    z_full = full.logits(rows); p_full, pu_full, mu_full = full.forward(rows, nmc=nmc, uncertainty=True)
    full.close()
    z, p, pu, mc_ent = [], [], 0.0, 0.0
    for s in expert_shards(ds["M"], G):
        e = _mk(ds, dims, True, B, "uniform", shard=s, world=G)
        z.append(e.logits(rows)); a, b, c = e.forward(rows, nmc=nmc, uncertainty=True); e.close()
        p.append(a); pu = pu + b.astype(np.float64); mc_ent = mc_ent + (b.astype(np.float64) - c.astype(np.float64))
    assert np.array_equal(np.concatenate(z, axis=1), z_full) and np.array_equal(np.concatenate(p, axis=1), p_full)
    ref_mc = pu_full.astype(np.float64) - mu_full.astype(np.float64)
    print("entropy sums rel", float((np.abs(pu - pu_full) / np.abs(pu_full)).max()), float((np.abs(mc_ent - ref_mc) / np.abs(ref_mc)).max()))
    assert (np.abs(pu - pu_full) <= 2e-6 * np.abs(pu_full)).all()
    assert (np.abs(mc_ent - ref_mc) <= 2e-6 * np.abs(ref_mc)).all()


# ------------------------------------------------------------------------------------------ range fallback at 128 on the default arithmetic
@pytest.mark.parametrize("bayesian", [True, False])
def test_range_fallback_at_128_runs_the_fused_f32_kernel(bayesian):
    """one output weight of 1e6 leaves the fp16 window of the scaled split: every call is counted as a fallback and redone on the exact-f32 fused kernel - no dense GEMM"""
    import torch
    from oracle import ntf_oracle as O
    from test_gpu_parity import _engine, _bnn_case
    D, H, M, B = 128, [128], 3000, 129
    sd, X, _ = _bnn_case(D, H, M, B, 5)
    if not bayesian:
        torch.manual_seed(5); sd = O.fnn_init(D, H, M)
    sd["layers.1.mu_weight" if bayesian else "layers.1.weight"][7, 5] = 1e6
    e = _engine([D] + H + [M], bayesian=bayesian, max_batch=B, ns=5, nsd="uniform", lr=1e-3)
    e.load_state_dict(sd); e.set_dense_input(X.numpy())
    _check_against_oracle(e, sd, X, bayesian, 3, expect_fallbacks=1, big_col=7)
    e.close()


# ------------------------------------------------------------------------------------------ both arms of the switch
def _arm_logits(monkeypatch, arm, dims, mfma, bayesian):
    from opentf_amd.synth import make_dataset
    from test_gpu_ep import _mk
    monkeypatch.setenv("NTF_INFER_F32", arm)
    ds = make_dataset("dblp", d=dims[0], seed=7, n_rows=400, n_experts=dims[-1])
    e = _mk(ds, dims[:-1] + [ds["M"]], bayesian, 200, "uniform", mfma=mfma)
    e.set_seed(3, 11)
    z = e.logits(np.arange(200, dtype=np.int64)); e.close()
    return z


@pytest.mark.parametrize("bayesian", [False, True])
@pytest.mark.parametrize("dims,mfma", PATH_CASES)
def test_both_arms_of_the_switch_agree(dims, mfma, bayesian, monkeypatch):
    from test_gpu_parity import _rel, RTOL_LOGITS
    a = _arm_logits(monkeypatch, "1", list(dims), mfma, bayesian)
    b = _arm_logits(monkeypatch, "0", list(dims), mfma, bayesian)
    print("arms rel", _rel(a, b))
    assert _rel(a, b) < RTOL_LOGITS


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path: sys.path.insert(0, root)
    _child_main()
