"""The one-kernel step head (opentf_amd/csrc/ntf_head.hip, `k_head`) against the float64 oracle, per element, at d = 64, 128 and 256, on
mean-pooled and on dense rows, with and without Flipout.

The engine takes `k_head` only when nothing is injected, so every oracle test that injects eps, signs and negatives runs the kernel chain in
its place; `k_head` itself was held to that chain (a second f32 implementation sharing its generators, test_gpu_round3.py) and, at d = 128 on
mean-pooled rows only, to a loss and parameter replay (test_gpu_replay.py).  Here a non-injected engine runs one evaluation and one training
step on the cases of tests/head_cases.py; the device's own draws of exactly those steps (`noise(step, B)`, `negatives(B)`) go to the oracle,
and the loss, every element of d loss / d z and every element of every gradient are compared under the suite's bars:
loss 2e-5 relative; dz 1e-4 relative with at most 2 elements astride leaky_relu's kink; logits recovered from dz 1e-4 + 2e-6; gradients 3e-4 of
their tensor's maximum, units with a pre-activation within rounding of the kink exempt and capped (tests/test_head_parity_host.py holds the
reference alone to the same bars).  What catches what:
  * dz is the per-element view of h: the gather (G = D / 4 lanes per row, rows of one to three sub-groups), the k halves, the s_in word index
    `(kb >> 5) + (t4 >> 3)`, s_out, and the weights streamed at d = 256;
  * layers.0.rho_weight / rho_bias: the eps quad index of the head against the export and against what k_flipout_grad_finalize regenerates;
  * the last M % 4 entries of layers.1.mu_bias / rho_bias: the bias workgroups' scalar tail;
  * the losses: the hidden KL and the output-bias KL the head adds.
The replays at the bottom run the PREFETCHED head (issued beside the previous step's dW kernel) at d = 64, 256 and on dense rows."""
import numpy as np
import pytest
import torch

import head_cases as HC
from oracle import ntf_oracle as O
from test_gpu_replay import _replay
from test_gpu_round2 import RTOL_LOGITS, _oracle_last_preact
from test_gpu_shapes import _check_grads, _d64, _oracle

pytestmark = pytest.mark.gpu

T0 = 11      # step index of the evaluation step; the training step takes T0 + 1


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


def _engine(name):
    from opentf_amd import libntf
    c, pb = HC.CASES[name], HC.problem(name)
    dense = c["input"] == "dense"
    e = libntf.Engine(c["dims"], bayesian=c["bayesian"], input_mode=libntf.INPUT_DENSE if dense else libntf.INPUT_MEANPOOL, max_batch=c["B"], ns=c["ns"],
                      nsd="uniform", tpw=c["tpw"], tnw=c["tnw"], lr=1e-3, seed=c["seed"], fuse_adam=0)
    if dense: e.set_dense_input(pb["Xall"])
    else: e.set_skill_table(pb["table"]); e.set_skill_csr(pb["skill"])
    e.set_member(pb["member"]); e.load_state_dict(pb["sd"])
    return e


def _steps(name):
    """one native evaluation step (step index T0) and one native backward (T0 + 1): losses, draws, dz, gradients, kernel families, range fallbacks"""
    c, pb = HC.CASES[name], HC.problem(name)
    B, seed, rows = c["B"], c["seed"], pb["rows"]
    e = _engine(name)
    try:
        e.kernel_times(True)
        e.set_seed(seed, T0)
        loss_ev = e.eval_step(rows)
        neg_ev, noise_ev = e.negatives(B).copy(), (e.noise(T0, B) if c["bayesian"] else None)
        e.set_seed(seed, T0 + 1)
        loss_tr = e.backward(rows)
        neg_tr, noise_tr = e.negatives(B).copy(), (e.noise(T0 + 1, B) if c["bayesian"] else None)
        dz, grads = e.dlogits(B).astype(np.float64), e.grads()
        kt, fallbacks = e.kernel_times(False), e.range_fallbacks()
    finally:
        e.close()
    return {"loss_ev": loss_ev, "pb_ev": HC.with_draws(pb, noise_ev, neg_ev), "loss_tr": loss_tr, "pb_tr": HC.with_draws(pb, noise_tr, neg_tr), "dz": dz, "grads": grads,
            "kt": kt, "fallbacks": fallbacks}


def _dz_oracle(c, pb, orc):
    """d loss / d z of the output layer, its pre-activation z and the logits leaky_relu(z), in float64"""
    z, logit = _oracle_last_preact(orc["sd64"], orc["X64"], orc["nz64"])
    loss = O.bxe(logit, pb["y"].double(), pb["neg"], c["tpw"], c["tnw"]).sum(dim=1).mean()
    (dz_ref,) = torch.autograd.grad(loss, z)
    return dz_ref.numpy(), z.detach().numpy(), logit.detach().numpy()


_CACHE = {}


def _case(name):
    """the device's two steps and the float64 oracle on the device's own draws, kept for the consecutive tests of one case (a failure is kept too: the steps
    are not run again for the next test of the case)"""
    if name not in _CACHE:
        _CACHE.clear()
        try:
            c, dev = HC.CASES[name], _steps(name)
            ev = dev["pb_ev"]      # an evaluation step's loss is the training loss of its draws (src/mdl/fnn.py:148-149), as test_gpu_shapes.py::_run compares it
            dev["orc_ev"] = float(O.batch_loss({k: v.double() for k, v in ev["sd"].items()}, ev["X"].double(), ev["y"].double(), ev["neg"], c["tpw"], c["tnw"], _d64(ev["noise"])))
            dev["orc"] = _oracle(dev["pb_tr"], c["tpw"], c["tnw"])
            dev["dz_ref"], dev["z"], dev["logit"] = _dz_oracle(c, dev["pb_tr"], dev["orc"])
            _CACHE[name] = dev
        except Exception as ex:
            _CACHE[name] = ex
    if isinstance(_CACHE[name], Exception): raise _CACHE[name]
    return _CACHE[name]


def _admissible(pb, ns):
    """distinct non-members, as src/mdl/fnn.py:48-56 draws them"""
    neg, B = pb["neg"], pb["y"].shape[0]
    assert neg.shape == (B, ns) and int(neg.min()) >= 0 and int(neg.max()) < pb["y"].shape[1]
    assert bool((pb["y"][torch.arange(B).unsqueeze(1), neg] == 0).all()), "a sampled negative is a member"
    assert all(len(set(r.tolist())) == ns for r in neg), "a negative drawn twice in one row"


@pytest.mark.parametrize("name", HC.NAMES)
def test_evaluation_and_training_loss_on_the_devices_own_draws(name):
    c, dev = HC.CASES[name], _case(name)
    _admissible(dev["pb_ev"], c["ns"]); _admissible(dev["pb_tr"], c["ns"])
    if c["bayesian"]:
        for a, b in zip(dev["pb_ev"]["noise"], dev["pb_tr"]["noise"]):
            assert set(np.unique(b["s_in"].numpy())) <= {-1.0, 1.0} and set(np.unique(b["s_out"].numpy())) <= {-1.0, 1.0}
            assert not np.array_equal(a["eps_w"].numpy(), b["eps_w"].numpy()), "two step indices, one set of draws"
    print(name, "eval loss", dev["loss_ev"], dev["orc_ev"], abs(dev["loss_ev"] - dev["orc_ev"]) / abs(dev["orc_ev"]),
          "train loss", dev["loss_tr"], dev["orc"]["loss"], abs(dev["loss_tr"] - dev["orc"]["loss"]) / abs(dev["orc"]["loss"]))
    assert np.isfinite(dev["orc_ev"]) and np.isfinite(dev["orc"]["loss"])
    assert abs(dev["loss_ev"] - dev["orc_ev"]) <= 2e-5 * abs(dev["orc_ev"]), (name, "eval loss", dev["loss_ev"], dev["orc_ev"])
    assert abs(dev["loss_tr"] - dev["orc"]["loss"]) <= 2e-5 * abs(dev["orc"]["loss"]), (name, "loss", dev["loss_tr"], dev["orc"]["loss"])


@pytest.mark.parametrize("name", HC.NAMES)
def test_dlogits_and_recovered_logits_elementwise(name):
    c, dev = HC.CASES[name], _case(name)
    B, tnw = c["B"], c["tnw"]
    dz, dz_ref, z, logit = dev["dz"], dev["dz_ref"], dev["z"], dev["logit"]
    assert dz.shape == dz_ref.shape == (B, c["dims"][2])
    # (1) every element of d loss / d z, positives and sampled negatives included; leaky_relu' jumps at z = 0: at most 2 elements astride it, each with |z| < 1e-5
    err = np.abs(dz - dz_ref)
    bad = err > RTOL_LOGITS * np.abs(dz_ref) + 1e-12
    print(name, "dz: elements over the bar", int(bad.sum()), "worst relative error elsewhere", float((err / np.maximum(np.abs(dz_ref), 1e-30))[~bad].max()))
    assert bad.sum() <= 2, (name, int(bad.sum()), float((err / np.maximum(np.abs(dz_ref), 1e-30)).max()))
    assert (np.abs(z[bad]) < 1e-5).all(), (name, z[bad])
    # (2) the logits the kernel computed, recovered from dz on the plain entries: dz = tnw / B * sigmoid(l) * (1 if z > 0 else 0.01), l = leaky_relu(z)
    pb = dev["pb_tr"]
    special = pb["y"].numpy() != 0
    special[np.arange(B)[:, None], pb["neg"].numpy()] = True
    u = dz * B / tnw
    s = np.where(u > 0.25, u, u / 0.01)
    with np.errstate(divide="ignore", invalid="ignore"):
        l_rec = np.log(s) - np.log1p(-s)
    ok = ~special & ~bad & (np.abs(logit) < 8)          # sigmoid saturates beyond: the inversion loses the digits, not the kernel
    assert ok.mean() > 0.95
    lerr, tol = np.abs(l_rec - logit)[ok], (RTOL_LOGITS * np.abs(logit) + 2e-6)[ok]
    print(name, "recovered logits: worst error / bar", float((lerr / tol).max()))
    assert (lerr <= tol).all(), (name, float(lerr.max()), int((lerr > tol).sum()))


@pytest.mark.parametrize("name", HC.NAMES)
def test_every_gradient_elementwise(name):
    c, dev = HC.CASES[name], _case(name)
    orc = dev["orc"]
    hidden, experts = HC.kink_counts(orc["kinks"])      # flags from the device's own draws; capped, so that the exemption cannot hide a failure
    cap_h, cap_e = HC.kink_caps(c["dims"][2])
    assert hidden <= cap_h and experts <= cap_e, (name, hidden, experts)
    assert set(dev["grads"]) == set(orc["grads"])
    print(name, "kink units", (hidden, experts), {k: f"{v:.2e}" for k, v in HC.worst_errors(dev["loss_tr"], dev["grads"], orc).items()})
    _check_grads(dev["grads"], orc["grads"], orc["kinks"], name)


@pytest.mark.parametrize("name", HC.NAMES)
def test_the_one_kernel_head_ran(name):
    dev = _case(name)
    assert dev["kt"]["gather"][1] == 0, (name, "the kernel chain's gather ran", dev["kt"]["gather"])
    assert dev["kt"]["gemm_hidden"][1] >= 2, (name, "no head launch per step", dev["kt"]["gemm_hidden"])
    assert dev["fallbacks"] == 0, (name, dev["fallbacks"])


def test_the_gather_counter_tells_the_chain_from_the_head(monkeypatch):
    """NTF_HEAD=0 (read when the engine is created): the same two steps through the kernel chain launch its gather"""
    monkeypatch.setenv("NTF_HEAD", "0")
    kt = _steps("d64-bnn-meanpool-B33-M1501")["kt"]
    assert kt["gather"][1] >= 1, kt["gather"]


# ------------------------------------------------------------------------------------------ the prefetched head off d = 128 and on dense rows
@pytest.mark.parametrize("D,bayesian,seed", [(64, True, 42), (64, False, 41), (256, True, 45), (256, False, 49)], ids=["d64-bnn", "d64-fnn", "d256-bnn", "d256-fnn"])
def test_three_pipelined_steps_replayed_through_the_oracle_off_d128(D, bayesian, seed):
    """test_gpu_replay.py's three pipelined default steps (its assertions, at the sizes it runs at d = 40) where k_head is the d = 64 or the d = 256 instantiation
    and, from the second step on, is issued for the next batch beside the dW kernel.

    The seeds: _replay's parameter budget (5e-4 of a tensor: 16 of the 32 768 elements of a 128 x 256 layer) has no room for a hidden unit on the other
    side of leaky_relu's kink, which moves that unit's whole row.  At d = 256, Fnn, seed 44 the oracle's pre-activation of (row 5, unit 49) at the third
    step is 1.9e-8; the parameters of the two sides differ by then (Adam's lr * m / (sqrt(v) + eps) where |g| is small: 8e-6) by enough to move that
    sum by 1.9e-5, the device lands on the other side, and 41 elements of row 49 - no element of any other row - leave the bar (the same 41 with
    NTF_HEAD=0, with NTF_HEAD_PREFETCH=0 and with NTF_FNN_PIPE=0: it is not the head's).  At the seeds here no hidden pre-activation, evaluated in float64
    from the oracle's and from the device's parameters of each step, differs in sign; at d = 256, Fnn, seed 49 the smallest |z| of the three steps is
    1.2e-5 / 2.1e-5 / 6.1e-5 against a largest difference of 0 / 4.6e-7 / 1.0e-5 (profiles/head_parity_check.md)."""
    _replay(D=D, H=128, M=20_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=seed, t0=6, bayesian=bayesian, pipelined=True)


def test_three_pipelined_steps_replayed_through_the_oracle_on_dense_rows():
    """the same on INPUT_DENSE: the prefetched head reads the next batch's rows of the dense input"""
    _replay(D=128, H=128, M=20_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=47, t0=13, bayesian=True, pipelined=True, dense=True)
