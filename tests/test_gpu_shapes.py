"""Oracle parity away from the benchmark's shapes: hidden widths that are not multiples of 4 or fall outside the fused set, up to
NTF_MAX_LAYERS layers, batches at the sizes every expert-parallel rank steps (B = G x --batch), the stateless GEMM, and a gradient
buffer written through its raw view between two first-layer sweeps.

Every step injects its random tensors (eps, signs, negatives) or replays the device's own draws, and is compared with
oracle/ntf_oracle.py evaluated in float64 (torch CPU autograd): a high-precision reference, not a second f32 implementation.
Bars (those of the rest of the suite): logits 1e-4 of max |z|; losses 2e-5 relative; every gradient 3e-4 of its tensor's max;
parameters after the default fused step 1e-3 relative + 2e-5 with a 2e-4 fraction budget (Adam's first step is lr * g / (|g| + eps):
where |g| ~ eps a rounding difference in g moves the update by up to 2 lr).

leaky_relu' kink flips: a pre-activation within rounding of 0 may land on the other side of the kink in another summation order,
which moves that unit's whole gradient row.  The oracle marks every (row, unit) with |z| below the rounding scale of its sum
(KINK_C * sqrt(fan-in so far) * 2^-24 * sum of |terms|: the spread of a rounded sum of that many terms, with margin for the split
fp16x3 products); only the gradient rows (and the parameters) of units so marked may exceed the bar."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import draw_noise
from oracle import ntf_oracle as O
from opentf_amd import libntf
from opentf_amd.ep import expert_shards
from test_gpu_parity import _engine

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KINK_C = 8.0            # rounding scale of a pre-activation: KINK_C * sqrt(fan-in so far) * 2^-24 * sum of |terms|
FUSED_H = (32, 64, 128, 256)
FUSED_OUT_H = FUSED_H + (96, 160, 192, 224)      # every last hidden width with fused output-layer kernels (FUSED_H: those with all three engine modes here)
GENERIC_OUT = ("out_fwd_gemm", "out_bwd_dw_gemm", "out_bwd_da_gemm")
FUSED_OUT = ("out_fused_fwd_loss_dh", "out_fused_dw_adam")


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    """these tests seed and draw from torch's (and numpy's, Python's) global generators; later modules draw from the same generators
    without seeding them: each test hands them back in the state it found them, so this module changes no other test's draws."""
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


# ------------------------------------------------------------------------------------------ problem + float64 oracle
def _d64(noise):
    return None if noise is None else [{k: v.double() for k, v in n.items()} for n in noise]


def _inject(neg, noise):
    inj = {"neg_idx": None if neg is None else neg.numpy()}
    if noise is not None:
        inj.update({k: [n[k] for n in noise] for k in ("eps_w", "eps_b", "s_in", "s_out")})
    return inj


def _problem(dims, B, bayesian, seed, ns, multihot=False, mean_m=3.0):
    """parameters (the reference's init), inputs, member CSR / dense labels, one set of Flipout noise and negatives.  Each row has at most
    M - ns positives, so that the oracle's rand + topk sampler (src/mdl/fnn.py:48-56) picks negatives only."""
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    D, H, M = dims[0], list(dims[1:-1]), dims[-1]
    sd = O.bnn_init(D, H, M) if bayesian else O.fnn_init(D, H, M)
    if multihot:      # the team's 0 / 1 skill row (src/mdl/ntf.py:23); one team without skills: only the bias reaches the hidden layer
        Xn = np.zeros((B, D), np.float32)
        for i in range(B):
            Xn[i, rng.choice(D, min(D, 1 + rng.poisson(7.5)), replace=False)] = 1
        Xn[min(3, B - 1)] = 0
        X = torch.from_numpy(Xn)
    else:
        X = torch.randn(B, D)
    mn = np.minimum(1 + rng.poisson(mean_m - 1, B), M - ns)
    m_ip = np.concatenate([[0], np.cumsum(mn)]).astype(np.int64)
    m_ix = np.concatenate([np.sort(rng.choice(M, k, replace=False)) for k in mn]).astype(np.int32)
    y = torch.zeros(B, M)
    y[np.repeat(np.arange(B), mn), m_ix.astype(np.int64)] = 1.0
    noise = draw_noise(sd, B) if bayesian else None
    neg = O.ns_uniform(y, ns) if ns else None
    return {"sd": sd, "X": X, "member": (m_ip, m_ix), "y": y, "noise": noise, "neg": neg, "ns": ns, "multihot": multihot}


def _kink_units(sd, X, noise):
    """per layer [B, out] bool: pre-activations within the rounding scale of their sum (float64)"""
    out, x, fan = [], X, 0
    for i in range(O.n_layers(sd)):
        p = f"layers.{i}."
        if noise is not None:
            nz = noise[i]
            z = O.flipout_linear(x, sd[p + "mu_weight"], sd[p + "rho_weight"], sd[p + "mu_bias"], sd[p + "rho_bias"], nz)
            wabs = sd[p + "mu_weight"].abs() + (O.softplus_rho(sd[p + "rho_weight"]) * nz["eps_w"]).abs()
            babs = sd[p + "mu_bias"].abs() + (O.softplus_rho(sd[p + "rho_bias"]) * nz["eps_b"]).abs()
        else:
            z = F.linear(x, sd[p + "weight"], sd[p + "bias"])
            wabs, babs = sd[p + "weight"].abs(), sd[p + "bias"].abs()
        fan += x.shape[1]
        scale = KINK_C * fan ** 0.5 * U * (x.abs() @ wabs.T + babs)
        out.append((z.abs() <= scale).numpy())
        x = F.leaky_relu(z)
    return out


def _oracle(pb, tpw=10.0, tnw=1.0):
    """logits, loss, every gradient and the parameters after one Adam step, in float64"""
    sd = {k: v.double() for k, v in pb["sd"].items()}
    X, y, nz = pb["X"].double(), pb["y"].double(), _d64(pb["noise"])
    with torch.no_grad():
        logits = O.model_forward(sd, X, nz).numpy()
        kinks = _kink_units(sd, X, nz)
    loss, grads = O.loss_and_grads(sd, X, y, pb["neg"], tpw, tnw, nz)
    new = {k: v.clone() for k, v in sd.items()}
    O.Adam(new, 1e-3).step(new, grads)
    return {"logits": logits, "loss": loss, "grads": {k: v.numpy() for k, v in grads.items()}, "new": {k: v.numpy() for k, v in new.items()},
            "kinks": kinks, "sd64": sd, "X64": X, "nz64": nz}


_CACHE = {}


def _case(key, dims, B, bayesian, seed, ns, **kw):
    """the problem and its oracle, kept for the consecutive tests (engine modes) of one case"""
    if key not in _CACHE:
        _CACHE.clear()
        pb = _problem(dims, B, bayesian, seed, ns, **kw)
        _CACHE[key] = (pb, _oracle(pb))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------ comparisons
def _layer(k):
    return int(k.split(".")[1])


def _check_logits(got, ref, tag):
    zmax = float(np.abs(ref).max())
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= 1e-4 * zmax, (tag, "logits", err, zmax)


def _check_grads(grads, ref, kinks, tag):
    for k, r in ref.items():
        g = grads[k]
        bad = np.abs(g - r) > 3e-4 * float(np.abs(r).max())
        flip = kinks[_layer(k)].any(0)          # units with a pre-activation within rounding of the kink, in any row
        outside = bad[~flip]
        assert not outside.any(), (tag, k, int(outside.sum()), float(np.abs(g - r).max()), float(np.abs(r).max()))


def _check_params(st, ref, kinks, tag):
    for k, r in ref.items():
        a = st[k]
        bad = np.abs(a - r) > (1e-3 * np.abs(r) + 2e-5)
        bad[kinks[_layer(k)].any(0)] = False
        assert float(bad.mean()) <= 2e-4, (tag, k, float(bad.mean()), float(np.abs(a - r).max()))


def _prob_tol(p, zmax):
    """the logit bar carried through the sigmoid: |dp| <= p (1 - p) |dz|"""
    return p * (1.0 - p) * 1e-4 * zmax + 2e-7


def _check_inference(e, pb, orc, rows, tag):
    """Fnn.test (src/mdl/fnn.py:172-219): forward(nmc = 1) probabilities and uncertainty on the injected noise against oracle.predict; the device
    top-K at K = 1 and K = min(M, 2048) against the oracle's probabilities on the device's own draws of that inference step"""
    B, M = len(rows), pb["y"].shape[1]
    zmax = float(np.abs(orc["logits"]).max())
    sd, X = orc["sd64"], orc["X64"]
    bayesian = pb["noise"] is not None
    injs = [_inject(None, pb["noise"])] if bayesian else None
    probs, pu, mu = e.forward(rows, nmc=1, injects=injs, uncertainty=True)
    mc = O.predict(sd, X, 1, [orc["nz64"]] if bayesian else None).numpy().reshape(1, B, M)
    ref = mc[0]
    tol = _prob_tol(ref, zmax)
    assert (np.abs(probs - ref) <= tol).all(), (tag, "probs", float((np.abs(probs - ref) / tol).max()))
    ent_tol = 1e-4 * np.abs(O.predictive_entropy(mc)) + (np.abs(np.log(ref + 1e-15) + 1.0) * tol).sum(1) + 1e-6
    assert (np.abs(pu - O.predictive_entropy(mc)) <= ent_tol).all(), (tag, "predictive entropy")
    assert (np.abs(mu - O.mutual_information(mc)) <= ent_tol).all(), (tag, "mutual information")
    for K in sorted({1, min(M, 2048)}):
        if bayesian: e.set_seed(99, 1000 + K)
        vals, idx = e.forward_topk(rows, K, nmc=1)
        if bayesian:
            nz = [{k: torch.from_numpy(v).double() for k, v in n.items()} for n in e.noise(1000 + K, B)]
            ref = O.predict(sd, X, 1, [nz]).numpy()[0]
            tol = _prob_tol(ref, zmax)
        assert all(len(set(r.tolist())) == K for r in idx) and idx.min() >= 0 and idx.max() < M, (tag, K, "indices")
        assert (np.diff(vals, axis=1) <= 0).all(), (tag, K, "values not in decreasing order")
        top = -np.sort(-ref, axis=1)[:, :K]
        rowtol = tol.max(1, keepdims=True)
        assert (np.abs(vals - top) <= rowtol).all(), (tag, K, "top-K values")
        picked = np.take_along_axis(ref, idx.astype(np.int64), axis=1)
        assert (np.abs(picked - vals) <= rowtol).all(), (tag, K, "top-K ids")


def _make(pb, dims, B, bayesian, mode, fuse_adam, tpw=10.0, tnw=1.0):
    e = _engine(dims, bayesian=bayesian, input_mode=libntf.INPUT_MULTIHOT if pb["multihot"] else libntf.INPUT_DENSE, max_batch=B, ns=pb["ns"],
                nsd="uniform" if pb["ns"] else None, tpw=tpw, tnw=tnw, lr=1e-3, fused=mode != "generic", mfma="f32" if mode == "f32" else None,
                fuse_adam=fuse_adam)
    if pb["multihot"]:
        ip, ix = (np.asarray(a) for a in _csr(pb["X"].numpy()))
        e.set_skill_csr((ip, ix))
    else:
        e.set_dense_input(pb["X"].numpy())
    e.set_member(pb["member"]); e.load_state_dict(pb["sd"])
    return e


def _csr(dense):
    import scipy.sparse
    m = scipy.sparse.csr_matrix(dense != 0)
    return m.indptr.astype(np.int64), m.indices.astype(np.int32)


def _run(pb, orc, dims, B, bayesian, mode, inference=True, tpw=10.0, tnw=1.0, after_backward=None):
    """one injected step on both sides, from identical state (orc: _oracle(pb, tpw, tnw)).  after_backward(engine): further checks on the engine that
    ran backward().  Returns the kernel families the default fused step ran."""
    tag = (dims, B, bayesian, mode)
    rows = np.arange(B)
    inj = _inject(pb["neg"], pb["noise"])
    e = _make(pb, dims, B, bayesian, mode, 0, tpw, tnw)
    try:
        _check_logits(e.logits(rows, inject=inj), orc["logits"], tag)
        if inference: _check_inference(e, pb, orc, rows, tag)
        ev = e.eval_step(rows, inject=inj)
        assert abs(ev - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (tag, "eval loss", ev, orc["loss"])
        loss = e.backward(rows, inject=inj)
        assert abs(loss - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (tag, "loss", loss, orc["loss"])
        _check_grads(e.grads(), orc["grads"], orc["kinks"], tag)
        if after_backward is not None: after_backward(e)
    finally:
        e.close()
    e = _make(pb, dims, B, bayesian, mode, 1, tpw, tnw)      # the plugin's default: the output layer's Adam in the dW epilogue
    try:
        e.kernel_times(True)
        loss = e.train_step(rows, inject=inj)
        kt = e.kernel_times(False)
        assert abs(loss - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (tag, "train loss", loss, orc["loss"])
        _check_params(e.state_dict(), orc["new"], orc["kinks"], tag)
    finally:
        e.close()
    fused = mode != "generic" and len(dims) > 2 and dims[-2] in FUSED_OUT_H
    if len(dims) > 2:
        for fam in (FUSED_OUT if fused else GENERIC_OUT):
            assert kt[fam][1] > 0, (tag, fam, "did not run")
        for fam in (GENERIC_OUT if fused else FUSED_OUT):
            assert kt[fam][1] == 0, (tag, fam, "ran")
    return kt


# ------------------------------------------------------------------------------------------ A. widths x depths
A_CASES = {     # name: dims, B, ns
    "odd_D_h100": ([37, 100, 1001], 257, 5),                        # generic chain, hidden width outside the fused set
    "h3_M65": ([33, 3, 65], 131, 5),                                # tiny hidden width, M just past one 64-tile
    "all_ones": ([16, 1, 1], 70, 0),                                # every dimension 1 but D; no negatives (nsd = None)
    "h512_M4097": ([130, 512, 4097], 300, 5),                       # wide hidden layer, M across the d(hidden) GEMM's split-K threshold
    "odd_then_h128": ([128, 127, 129, 128, 3000], 200, 5),          # odd widths in front of the fused H = 128 output layer
    "four_hidden": ([64, 96, 33, 64, 31, 900], 190, 5),             # every dAct buffer reused
    "eight_layers": ([24, 40, 40, 40, 40, 40, 40, 32, 300], 150, 5),    # NTF_MAX_LAYERS, fused H = 32 output layer
}


def _modes(dims):
    return ("default", "f32", "generic") if dims[-2] in FUSED_H else ("default",)


A_PARAMS = [pytest.param(name, bay, mode, id=f"{name}-{'bnn' if bay else 'fnn'}-{mode}")
            for name, (dims, _, _) in A_CASES.items() for bay in (True, False) for mode in _modes(dims)]


@pytest.mark.parametrize("name,bayesian,mode", A_PARAMS)
def test_width_depth_step_and_inference_against_the_f64_oracle(name, bayesian, mode):
    dims, B, ns = A_CASES[name]
    pb, orc = _case(("A", name, bayesian), dims, B, bayesian, seed=len(dims) * 1000 + dims[1], ns=ns)
    _run(pb, orc, dims, B, bayesian, mode)


@pytest.mark.parametrize("h0,sweeps", [(30, False), (128, True)])
def test_multihot_first_layer_width_and_the_sweep(h0, sweeps):
    """a multi-hot first layer (S = 700) in front of the fused H = 128 output layer.  h[0] = 30 is not a multiple of 4: the one-pass first-layer
    sweep must decline and the step must still equal the oracle; h[0] = 128 (NTF_L0_SWEEP at its default) is the control, where it runs."""
    dims, B = [700, h0, 128, 1500], 90
    pb, orc = _case(("MH", h0), dims, B, True, seed=700 + h0, ns=5, multihot=True)
    _run(pb, orc, dims, B, True, "default")
    # the sweep counter grows only on native steps that take the previous sweep's operands: two staged default steps
    e = _make(pb, dims, B, True, "default", 1)
    e.stage_order(np.concatenate([np.arange(B), np.arange(B)]).astype(np.int64))
    s0 = e.first_layer_sweeps()
    e.step_staged(0, B, train=True, apply=True); e.step_staged(B, B, train=True, apply=True)
    n = e.first_layer_sweeps() - s0
    e.close()
    assert n == (1 if sweeps else 0), (h0, n)


def test_nine_layers_are_refused_at_creation():
    """NTF_MAX_LAYERS = 8: the wrapper refuses a 9-layer dims list before it fills the fixed-size config, and ntf_engine_create itself returns
    NTF_EINVAL for n_layers = 9 before it reads any dims entry"""
    with pytest.raises(libntf.NtfError, match="between 1 and 8 layers"):
        libntf.Engine([16] * 9 + [8], max_batch=4)
    cfg = libntf.ntf_config()
    cfg.abi_version, cfg.device, cfg.n_layers, cfg.max_batch, cfg.ns = libntf.NTF_ABI_VERSION, 0, libntf.NTF_MAX_LAYERS + 1, 4, 0
    for i in range(libntf.NTF_MAX_LAYERS + 1):
        cfg.dims[i] = 16
    h = C.c_void_p()
    rc = libntf.lib().ntf_engine_create(C.byref(cfg), C.byref(h))
    assert rc == -1 and not h.value, rc                              # NTF_EINVAL, no engine
    assert b"n_layers" in libntf.lib().ntf_last_error(None)


def test_retired_merge_bias_arm_is_refused_at_creation(monkeypatch):
    """NTF_MERGE_BIAS=0 (the next step's output-bias operand as a launch of its own) is retired like the old NTF_FWD_KERNEL forms: ntf_engine_create fails with
    NTF_EINVAL and says why; unset, or at its former default 1, the engine is created"""
    monkeypatch.setenv("NTF_MERGE_BIAS", "0")
    with pytest.raises(libntf.NtfError, match=r"ntf_engine_create failed \(-1\): NTF_MERGE_BIAS=0 .* was retired"):
        libntf.Engine([16, 8], max_batch=4)
    monkeypatch.setenv("NTF_MERGE_BIAS", "1")
    libntf.Engine([16, 8], max_batch=4).close()
    monkeypatch.delenv("NTF_MERGE_BIAS")
    libntf.Engine([16, 8], max_batch=4).close()


# ------------------------------------------------------------------------------------------ B. the batch sizes of expert-parallel ranks
B_M = 4500
B_PARAMS = [pytest.param(B, bay, mode, id=f"B{B}-{'bnn' if bay else 'fnn'}-{mode}")
            for B in (1023, 1024, 1025, 2047, 2048, 2049, 8000) for bay in (True, False) for mode in ("default", "f32", "generic")]


@pytest.mark.parametrize("B,bayesian,mode", B_PARAMS)
def test_large_batch_step_against_the_f64_oracle(B, bayesian, mode):
    """[128, 128, 4 500] at B around the row-chunked bias gradient's (1 024) and the split-K weight gradient's (2 048) thresholds and at
    B = 8 000 (the global minibatch every rank steps under --parallel ep at G = 8)"""
    dims = [128, 128, B_M]
    pb, orc = _case(("B", B, bayesian), dims, B, bayesian, seed=B, ns=5)
    _run(pb, orc, dims, B, bayesian, mode, inference=False)


@pytest.mark.parametrize("bayesian", [True, False])
def test_large_batch_with_a_hidden_to_hidden_layer(bayesian):
    """[128, 96, 128, M] at B = 8 000: the hidden weight gradient of layer 1 (96 x 128, 4 tiles) takes the 64-way split-K GEMM, the hidden
    biases the row-chunked reduction; kernel_times shows the hidden-layer families and the fused output layer ran"""
    dims, B = [128, 96, 128, 4100], 8000
    pb, orc = _case(("BH", bayesian), dims, B, bayesian, seed=77, ns=5)
    kt = _run(pb, orc, dims, B, bayesian, "default", inference=False)
    for fam in ("gemm_hidden", "bias_grad"):
        assert kt[fam][1] > 0, (fam, kt[fam])


def _expert_shard_step(dims, B, tpw, tnw, ns, labels=None, seed=31, t0=17, before_compare=None):
    """a Bnn model whose output layer is cut into two expert shards, stepped through ntf_step_staged_ep (d(hidden) summed between phases 1 and 2)
    on the device's own draws: each shard's output-layer gradient and updated parameters against the oracle's columns of that shard, the
    replicated hidden layer's gradient and parameters (after the exchange) against the whole oracle.  labels = (member CSR, dense y): these
    rows in place of _problem's; before_compare(pb, orc): the caller's conditions on the oracle's side, before any device value is compared."""
    H, M = dims[-2], dims[-1]
    pb = _problem(dims, B, True, seed, ns)
    if labels is not None: pb["member"], pb["y"] = labels
    order = np.arange(B, dtype=np.int64)
    shards = expert_shards(M, 2)
    assert shards == [(0, M // 2), (M // 2, M)]
    engines = []
    for s in shards:
        e = libntf.Engine(dims, bayesian=True, input_mode=libntf.INPUT_DENSE, max_batch=B, ns=ns, nsd="uniform", tpw=tpw, tnw=tnw, lr=1e-3,
                          seed=seed, fuse_adam=0, expert_shard=s, ep_world=2)
        e.set_dense_input(pb["X"].numpy()); e.set_member(pb["member"]); e.load_state_dict(pb["sd"])
        e.set_seed(seed, t0); e.stage_order(order); e.epoch_loss()
        engines.append(e)
    try:
        for e in engines:
            e.step_staged_ep(0, B, 1); e.synchronize()
        dh = [e.dh_tensor() for e in engines]
        tot = torch.stack([d[: B * H] for d in dh]).sum(0)
        for d in dh: d[: B * H].copy_(tot)
        torch.cuda.synchronize()
        for e in engines:
            e.step_staged_ep(0, B, 2); e.step_staged_ep(0, B, 3)
        loss = sum(e.epoch_loss()[0] for e in engines)
        negs = [e.negatives(B) for e in engines]
        noises = [e.noise(t0, B) for e in engines]
        grads = [e.grads() for e in engines]
        states = [e.state_dict() for e in engines]
    finally:
        for e in engines: e.close()
    assert np.array_equal(negs[0], negs[1]), "the shards drew different negatives"
    for k in noises[0][0]:
        assert np.array_equal(noises[0][0][k], noises[1][0][k]), f"the shards drew different hidden-layer {k}"
    assert np.array_equal(noises[0][1]["s_in"], noises[1][1]["s_in"]), "the shards drew different input signs of the output layer"
    out = {"eps_w": 0, "eps_b": 0, "s_out": 1}      # the output layer's expert axis
    noise = [{k: torch.from_numpy(v) for k, v in noises[0][0].items()},
             {k: torch.from_numpy(noises[0][1][k] if k == "s_in" else np.concatenate([n[1][k] for n in noises], axis=out[k])) for k in noises[0][1]}]
    pb["noise"], pb["neg"] = noise, torch.from_numpy(negs[0].astype(np.int64))
    assert all(len(set(r.tolist())) == ns for r in negs[0]) and negs[0].min() >= 0 and negs[0].max() < M, "picks not distinct ids in [0, M)"
    enough = (M - pb["y"].sum(1)) >= ns            # rows with at least ns negatives: non-members only (src/mdl/fnn.py:48-56)
    assert bool((pb["y"][torch.arange(B).unsqueeze(1), pb["neg"]] == 0)[enough].all())
    orc = _oracle(pb, tpw, tnw)
    if before_compare is not None: before_compare(pb, orc)
    assert abs(loss - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (loss, orc["loss"])
    kinks = orc["kinks"]
    for si, (lo, hi) in enumerate(shards):
        kk = [kinks[0], kinks[1][:, lo:hi]]
        for k in orc["grads"]:
            sl = slice(lo, hi) if _layer(k) == 1 else slice(None)
            ref = {k: orc["grads"][k][sl]}
            _check_grads({k: grads[si][k]}, ref, kk, ("shard", si))
            _check_params({k: states[si][k]}, {k: orc["new"][k][sl]}, kk, ("shard", si))


def test_expert_shards_at_B8000_against_the_f64_oracle():
    """B = 8 000, [128, 128, 2 x 2 048] cut into two expert shards stepped through ntf_step_staged_ep (d(hidden) summed between phases 1 and 2)
    on the device's own draws: each shard's output-layer gradient and updated parameters against the oracle's columns of that shard, the
    replicated hidden layer's gradient and parameters (after the exchange) against the whole oracle"""
    _expert_shard_step([128, 128, 4096], 8000, 10.0, 1.0, 5)


# ------------------------------------------------------------------------------------------ C. ntf_k_gemm_f32
GEMM_SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 1000)
GEMM_C = 2.0      # |C - A B| <= GEMM_C * k * 2^-24 * (|A| |B|): f32 products and a k-term f32 sum


def _gemm_case(m, n, k, a_kc, b_nc, pad, rng):
    A = rng.standard_normal((m, k)).astype(np.float32)
    Bm = rng.standard_normal((k, n)).astype(np.float32)
    if a_kc: a_dev, sam, sak = torch.from_numpy(A.copy()).cuda(), k, 1            # A(i, p) = A[i * k + p]
    else: a_dev, sam, sak = torch.from_numpy(np.ascontiguousarray(A.T)).cuda(), 1, m     # A(i, p) = A[i + p * m]
    if b_nc: b_dev, sbk, sbn = torch.from_numpy(Bm.copy()).cuda(), n, 1
    else: b_dev, sbk, sbn = torch.from_numpy(np.ascontiguousarray(Bm.T)).cuda(), 1, k
    ldc = n + pad
    c_dev = torch.full((m, ldc), 12345.0, dtype=torch.float32, device="cuda")
    libntf.gemm_f32(m, n, k, a_dev.data_ptr(), sam, sak, b_dev.data_ptr(), sbk, sbn, c_dev.data_ptr(), ldc,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    got = c_dev.cpu().numpy()
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    ref, mag = A64 @ B64, np.abs(A64) @ np.abs(B64)
    err = np.abs(got[:, :n] - ref)
    assert (err <= GEMM_C * k * U * mag).all(), ((m, n, k, a_kc, b_nc), float((err / np.maximum(GEMM_C * k * U * mag, 1e-30)).max()))
    if pad: assert (got[:, n:] == 12345.0).all(), ((m, n, k), "wrote into the padding columns of C")


@pytest.mark.parametrize("a_kc,b_nc", [(True, True), (True, False), (False, True), (False, False)], ids=["sak1-sbn1", "sak1-sbk1", "sam1-sbn1", "sam1-sbk1"])
def test_gemm_f32_against_float64_product(a_kc, b_nc):
    rng = np.random.default_rng(int(a_kc) * 2 + int(b_nc))
    for m in GEMM_SIZES:
        for n in GEMM_SIZES:
            for k in GEMM_SIZES:
                _gemm_case(m, n, k, a_kc, b_nc, 0, rng)
    for m, n in ((1, 1), (33, 65), (64, 64), (127, 31), (1000, 63)):
        _gemm_case(m, n, 4096, a_kc, b_nc, 0, rng)


def test_gemm_f32_leaves_the_padding_of_c_alone():
    rng = np.random.default_rng(5)
    for m, n, k in ((1, 1, 1), (31, 33, 65), (65, 63, 127), (127, 64, 1000), (1000, 127, 32), (64, 1000, 4096)):
        for a_kc in (True, False):
            for b_nc in (True, False):
                _gemm_case(m, n, k, a_kc, b_nc, 7, rng)


# ------------------------------------------------------------------------------------------ D. the gradient buffer written through its raw view
def test_gradient_written_through_the_view_does_not_reach_the_next_swept_step():
    """A multi-hot Bayesian engine on the default path, where the first layer's gradient is a scatter into rows the previous one-pass sweep
    cleared (no memset in front of it).  Between two default train steps the caller writes the gradient buffer through ntf_grad_buffer's view
    (as an all-reduce does); the second step's batch touches skill rows the first did not.  Both steps, replayed through the float64 oracle
    on the device's own draws, must match: a step's gradient does not depend on what the buffer held before it (src/mdl/fnn.py:122-140
    zeroes the gradients every step)."""
    S, H, M, B, seed, t0 = 700, 128, 1500, 90, 41, 5
    dims = [S, H, M]
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    sd = O.bnn_init(S, [H], M)
    Xn = np.zeros((2 * B, S), np.float32)
    for i in range(2 * B):        # batch 1 draws its skills from the first half of the table, batch 2 from the second
        lo = 0 if i < B else S // 2
        Xn[i, lo + rng.choice(S // 2, 1 + rng.poisson(7.5), replace=False)] = 1
    mn = 1 + rng.poisson(2.0, 2 * B)
    m_ip = np.concatenate([[0], np.cumsum(mn)]).astype(np.int64)
    m_ix = np.concatenate([np.sort(rng.choice(M, k, replace=False)) for k in mn]).astype(np.int32)
    y = torch.zeros(2 * B, M); y[np.repeat(np.arange(2 * B), mn), m_ix.astype(np.int64)] = 1.0
    e = libntf.Engine(dims, bayesian=True, input_mode=libntf.INPUT_MULTIHOT, max_batch=B, ns=5, nsd="uniform", tpw=10.0, tnw=1.0, lr=1e-3,
                      seed=seed, fuse_adam=1)
    try:
        e.set_skill_csr(_csr(Xn)); e.set_member((m_ip, m_ix)); e.load_state_dict(sd)
        e.set_seed(seed, t0); e.stage_order(np.arange(2 * B, dtype=np.int64))
        sw0 = e.first_layer_sweeps()
        l1 = e.step_staged(0, B, train=True, apply=True, want_loss=True)
        neg1, nz1, st1 = e.negatives(B).copy(), e.noise(t0, B), e.state_dict()
        e.synchronize()
        e.grad_tensor().fill_(0.5)
        torch.cuda.synchronize()
        l2 = e.step_staged(B, B, train=True, apply=True, want_loss=True)
        neg2, nz2, st2 = e.negatives(B).copy(), e.noise(t0 + 1, B), e.state_dict()
        assert e.first_layer_sweeps() - sw0 == 1, "the second step did not start from the first step's sweep"
    finally:
        e.close()
    X = torch.from_numpy(Xn).double()
    sd_ref = {k: v.double().clone() for k, v in sd.items()}
    opt = O.Adam(sd_ref, 1e-3)
    for step, (l, sl, neg, nz, st) in enumerate(((l1, slice(0, B), neg1, nz1, st1), (l2, slice(B, 2 * B), neg2, nz2, st2)), 1):
        nz = [{k: torch.from_numpy(v).double() for k, v in n.items()} for n in nz]
        ref_loss, _ = O.train_step(sd_ref, opt, X[sl], y[sl].double(), torch.from_numpy(neg.astype(np.int64)), 10.0, 1.0, nz)
        assert abs(l - ref_loss) <= 2e-5 * abs(ref_loss), (step, l, ref_loss)
        for k in sd_ref:
            a, b = st[k], sd_ref[k].numpy()
            bad = np.abs(a - b) > (1e-3 * np.abs(b) + 2e-5)
            assert float(bad.mean()) <= 2e-4, (step, k, float(bad.mean()), float(np.abs(a - b).max()))
