"""Native-draw replay: the kernels the benchmark times, step for step against the oracle (VERDICT r4 missing #2).

Every other oracle comparison of a train step INJECTS the random tensors (eps, signs, negatives), i.e. runs the `INJ = true` template instantiations of the forward /
dW kernels.  What `bench.py` and the plugin run is the other set: sign words hashed in place (`sign_word`), Flipout eps drawn by Philox inside the operand producer of
the PREVIOUS step's dW epilogue (`nx_eps`) and drawn AGAIN by this step's epilogue for the rho gradient (`cur_eps`), the next batch's sampler / head issued beside the dW
kernel, the lean epilogue, the tail split of the dW launch.  Here a non-injected engine at `set_seed(s, t)` runs three consecutive DEFAULT train steps over a staged
order; the test then fetches the device's own draws for exactly those steps - `ntf_get_noise` (eps_w, eps_b, s_in, s_out per layer), `ntf_get_negatives` - feeds them to
`oracle.train_step` (torch CPU autograd + restated Adam; reference lines src/mdl/fnn.py:122-140 with bayesian-torch's LinearFlipout.forward) and compares the loss of
every step and every parameter (incl. every rho) after the third.  A forward eps that differed from the backward eps, a step counter keyed one off between `nx_eps` and
`cur_eps`, a `sign_word()` that disagreed with the exported signs, a prefetched head run on the wrong batch's negatives: each shows here as a loss or parameter mismatch
(statistical tests cannot see them: the data term of the rho gradient would average to zero)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dataset(rng, N, S, D, M, mean_s, mean_m):
    nnz = np.minimum(1 + rng.poisson(mean_s - 1, N), S)
    s_ip = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
    s_ix = np.concatenate([np.sort(rng.choice(S, k, replace=False)) for k in nnz]).astype(np.int32)
    table = rng.standard_normal((S, D)).astype(np.float32)
    mn = 1 + rng.poisson(mean_m - 1, N)
    m_ip = np.concatenate([[0], np.cumsum(mn)]).astype(np.int64)
    m_ix = np.concatenate([np.sort(rng.choice(M, k, replace=False)) for k in mn]).astype(np.int32)
    return (s_ip, s_ix), table, (m_ip, m_ix)


def _replay(D, H, M, B, S, mean_s, mean_m, seed, t0, nsteps=3, bad_frac=5e-4, nsd="uniform", multihot=False, bayesian=True, pipelined=True, ns=5, tpw=10.0, tnw=1.0, dense=False):
    import torch
    from oracle import ntf_oracle as O
    from opentf_amd import libntf
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    N = (nsteps + 1) * B                                   # one batch more than is stepped: the last step still has a next batch to prefetch a head for
    skill, table, member = _dataset(rng, N, S, D, M, mean_s, mean_m)
    sd = O.bnn_init(D, [H], M) if bayesian else O.fnn_init(D, [H], M)
    order = rng.permutation(N).astype(np.int64)
    if multihot:       # BASELINE config 3's input: the team's 0 / 1 skill row itself (src/mdl/ntf.py:23), D = S
        assert D == S
        Xn = np.zeros((N, S), np.float32); Xn[np.repeat(np.arange(N), np.diff(skill[0])), skill[1].astype(np.int64)] = 1.0
        Xall = torch.from_numpy(Xn); del Xn
    else:
        Xall = torch.from_numpy(O.gather_meanpool_fast(skill[0], skill[1], table))

    def labels(rows):
        y = torch.zeros(len(rows), M)
        for k, r in enumerate(rows): y[k, member[1][member[0][r]: member[0][r + 1]].astype(np.int64)] = 1.0
        return y

    def as_torch(noise):
        return [{k: torch.from_numpy(v) for k, v in n.items()} for n in noise] if noise is not None else None

    assert not (dense and multihot)
    e = libntf.Engine([D, H, M], bayesian=bayesian, input_mode=libntf.INPUT_MULTIHOT if multihot else libntf.INPUT_DENSE if dense else libntf.INPUT_MEANPOOL, max_batch=B, ns=ns, nsd=nsd, tpw=tpw, tnw=tnw, lr=1e-3, seed=seed, fuse_adam=1)     # what bench.py and the plugin create: Adam in the dW epilogue, operands / head prefetched
    if dense: e.set_dense_input(Xall.numpy())      # the engine reads the mean-pooled rows themselves: no table, no skill CSR
    else:
        if not multihot: e.set_skill_table(table)
        e.set_skill_csr(skill)
    e.set_member(member); e.load_state_dict(sd)
    if nsd == "unigram": e.set_unigram(np.bincount(member[1], minlength=M) / N)      # src/mdl/fnn.py:82
    e.stage_order(order)

    # ---- logits of the first batch with the draws of step t0: the shipped inference kernel on native signs / eps against the oracle's forward on the exported tensors
    rows0 = order[:B]
    e.set_seed(seed, t0)
    got = e.logits(rows0)                                   # consumes step index t0
    noise0 = as_torch(e.noise(t0, B)) if bayesian else None
    for n in noise0 or []:
        assert set(np.unique(n["s_in"].numpy())) <= {-1.0, 1.0} and set(np.unique(n["s_out"].numpy())) <= {-1.0, 1.0}
        assert abs(float(n["eps_w"].mean())) < 0.02 and abs(float(n["eps_w"].std()) - 1.0) < 0.02
    ref = O.model_forward(sd, Xall[rows0], noise0).detach().numpy()
    zmax = float(np.abs(ref).max())
    assert float(np.abs(got - ref).max()) <= 1e-4 * zmax, float(np.abs(got - ref).max()) / zmax
    del got, ref

    # ---- three default train steps from the same step index, then their replay through the oracle
    e.set_seed(seed, t0)
    pre0, hit0, sw0 = e.prefetched_steps(), e.head_prefetch_hits(), e.first_layer_sweeps()
    losses, negs, noises = [], [], []
    for k in range(nsteps):
        losses.append(e.step_staged(k * B, B, train=True, apply=True, want_loss=True))
        negs.append(e.negatives(B).copy())
        noises.append(e.noise(t0 + k, B) if bayesian else None)
    # the pipelined default path really ran: steps 2.. started on operands the previous dW epilogue produced, with the head that ran beside that kernel
    if not pipelined: assert e.prefetched_steps() == pre0 and e.head_prefetch_hits() == hit0
    else: assert e.prefetched_steps() - pre0 >= nsteps - 1, (e.prefetched_steps(), pre0)
    if not pipelined or pipelined == "planes_only": pass      # ("planes_only": an input width the one-kernel head does not serve - operands prefetched, head in its own step)
    elif multihot:      # (no one-kernel head for this input; instead: steps 2.. took their first-layer sigma * eps and KL term from the previous step's one-pass sweep)
        import os
        want = 0 if os.environ.get("NTF_L0_SWEEP") == "0" else nsteps - 1
        assert e.first_layer_sweeps() - sw0 == want, (e.first_layer_sweeps(), sw0)
        if os.environ.get("NTF_MH_HEAD") != "0": assert e.head_prefetch_hits() - hit0 >= nsteps - 1, (e.head_prefetch_hits(), hit0)      # (the multi-hot head runs beside the previous dW kernel too)
    else: assert e.head_prefetch_hits() - hit0 >= nsteps - 1, (e.head_prefetch_hits(), hit0)
    st = e.state_dict(); e.close()

    sd_ref = {k: v.clone() for k, v in sd.items()}
    opt = O.Adam(sd_ref, 1e-3)
    for k in range(nsteps):
        rows = order[k * B: (k + 1) * B]
        y = labels(rows)
        neg = torch.from_numpy(negs[k])
        # the device's negatives are admissible draws of src/mdl/fnn.py:48-56 for THIS batch: distinct non-members
        assert bool((y[torch.arange(len(rows)).unsqueeze(1), neg] == 0).all())
        assert all(len(set(r.tolist())) == neg.shape[1] for r in neg)
        ref_loss, _ = O.train_step(sd_ref, opt, Xall[rows], y, neg, tpw, tnw, as_torch(noises[k]))
        assert abs(losses[k] - ref_loss) <= 2e-5 * abs(ref_loss), (k, losses[k], ref_loss)
    worst = {}
    for k in sd:
        a, b = st[k], sd_ref[k].numpy()
        bad = np.abs(a - b) > (1e-3 * np.abs(b) + 2e-5)
        # Adam's first steps move a parameter by ~lr whatever |g| is: where |g| ~ 1e-8 a rounding difference in g flips the update's sign (up to 2 lr per step)
        worst[k] = float(bad.mean())
        assert worst[k] <= bad_frac, (k, worst[k])
        assert float(np.abs(a - b).max()) <= 2e-3 * nsteps + 1e-6, (k, float(np.abs(a - b).max()))
    return worst


def test_three_default_steps_replayed_through_the_oracle_at_config2_size():
    """[128, 128, 233 629], B = 1000 (dblp mt10.ts2 shapes): the benchmark's configuration"""
    _replay(D=128, H=128, M=233_629, B=1000, S=4000, mean_s=8.57, mean_m=3.06, seed=21, t0=5)


def test_three_default_steps_replayed_through_the_oracle_on_a_ragged_shape():
    """a ragged last expert tile (M = 70 001: one expert into a 32-expert sub-tile, a 128-expert half-tile and a 256-expert tile) under a ragged row block (B = 129)"""
    _replay(D=128, H=128, M=70_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=22, t0=40)


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_three_default_fnn_steps_replayed_through_the_oracle(pipe, monkeypatch):
    """The non-Bayesian half of the path (src/mdl/fnn.py alone) on its default pipeline (round 6): the dW + Adam epilogue writes the next step's fp16 planes of mu, the hidden
    backward, the hidden Adam and the next batch's head run beside the dW kernel (asserted: steps 2.. start on prefetched planes and a prefetched head); NTF_FNN_PIPE=0: round
    5's serial step.  Negatives are the device's own draws."""
    monkeypatch.setenv("NTF_FNN_PIPE", pipe)
    _replay(D=128, H=128, M=70_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=25, t0=3, bayesian=False, pipelined=pipe == "1")
    if pipe == "1":
        _replay(D=128, H=128, M=233_629, B=1000, S=4000, mean_s=8.57, mean_m=3.06, seed=26, t0=8, bayesian=False)
        _replay(D=40, H=128, M=20_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=27, t0=2, bayesian=False, pipelined="planes_only")      # d = 40: no k_head, the chain of kernels


@pytest.mark.parametrize("sweep", ["1", "0"])
def test_three_default_steps_replayed_through_the_oracle_on_multihot_input(sweep, monkeypatch):
    """BASELINE config 3's first layer (round 6): multi-hot skill rows into a Flipout layer 0 whose gradient finalisation, Adam and next-step operand are ONE pass
    (launch_flipout_sweep, beside the dW kernel) - the default; NTF_L0_SWEEP=0: the three-kernel chain of round 5.  Both against the oracle on the device's own draws:
    a sweep whose next-step eps were keyed one step off, whose KL term landed in the wrong slot, or that cleared gradient rows the scatter had not flagged shows as a
    loss or parameter mismatch at step 2 or 3.  S = 1 500 skills with 6 per team: most rows of the layer are NOT touched by a batch (their gradient is the KL term alone)."""
    monkeypatch.setenv("NTF_L0_SWEEP", sweep)
    _replay(D=1500, H=128, M=20_001, B=129, S=1500, mean_s=6.0, mean_m=2.5, seed=24, t0=9, multihot=True)


@pytest.mark.parametrize("nsd", ["unigram_b", "unigram"])
def test_three_default_steps_replayed_through_the_oracle_with_the_frequency_samplers(nsd):
    """`unigram_b` is the sampler of every Bnn run the reference commits (its per-batch alias table staged one batch ahead, in the head prefetch); `unigram` the dataset-wide one"""
    _replay(D=128, H=128, M=70_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=23, t0=17, nsd=nsd)


@pytest.mark.parametrize("nsd", ["uniform", "unigram_b"])
def test_negatives_of_a_step_survive_the_next_batchs_prefetched_sampler(nsd):
    """with the head prefetch the next batch's sampler runs beside this step's dW kernel; `ntf_get_negatives` must still return THIS step's draws (they live in
    one of two buffers by step parity).  The same seed and step index without the prefetch (NTF_HEAD_PREFETCH=0 at engine creation) draws the same negatives.
    unigram_b (round 5): the next batch's per-batch alias table is staged beside the dW kernel too - same draws, and the head prefetch now hits for that sampler."""
    import os
    from oracle import ntf_oracle as O
    from opentf_amd import libntf
    import torch
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    D, H, M, B = 128, 128, 20_000, 256
    skill, table, member = _dataset(rng, 4 * B, 700, D, M, 5.0, 2.5)
    sd = O.bnn_init(D, [H], M)
    order = rng.permutation(4 * B).astype(np.int64)
    out = []
    for pf in ("1", "0"):
        old = os.environ.get("NTF_HEAD_PREFETCH")
        os.environ["NTF_HEAD_PREFETCH"] = pf
        try:
            e = libntf.Engine([D, H, M], bayesian=True, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd=nsd, seed=9, fuse_adam=1)
        finally:
            if old is None: os.environ.pop("NTF_HEAD_PREFETCH")
            else: os.environ["NTF_HEAD_PREFETCH"] = old
        e.set_skill_table(table); e.set_skill_csr(skill); e.set_member(member); e.load_state_dict(sd); e.stage_order(order)
        e.set_seed(9, 11)
        got = []
        for k in range(3):
            e.step_staged(k * B, B, train=True, apply=True)
            got.append(e.negatives(B).copy())
        out.append((got, e.head_prefetch_hits())); e.close()
    assert out[0][1] >= 2 and out[1][1] == 0
    for a, b in zip(out[0][0], out[1][0]): np.testing.assert_array_equal(a, b)
    assert not np.array_equal(out[0][0][0], out[0][0][1])
    if nsd == "unigram_b":      # src/mdl/fnn.py:74-76: negatives are experts of the batch itself (weight y.sum(0) / B), never members of the row
        for k, neg in enumerate(out[0][0]):
            rows = order[k * B: (k + 1) * B]
            support = set(np.concatenate([member[1][member[0][r]: member[0][r + 1]] for r in rows]).tolist())
            assert set(neg.ravel().tolist()) <= support


def test_a_row_with_an_outlier_activation_keeps_the_loss_finite():
    """Found by the replay work (round 5): k_out_fwd_h3p takes ONE v_log_f32 for four experts' softplus terms - log((1 + e^-l0)(1 + e^-l1)(1 + e^-l2)(1 + e^-l3)) - and
    that product overflows once four logits of a row average below -22, i.e. pre-activations below -2 200 under leaky_relu: one team with an outlier embedding at step
    1 134 of the benchmark's own run made the step's loss NaN (inf through the compensated sum; the gradients were right - they never went through it).  The kernel now
    clamps l at -21 (softplus and its slope below 7.6e-10 there).  Here: rows whose hidden activation is ~2 000 under output weights ten times the initial scale - thousands
    of logits below -22, runs of four among them - through the
    default training step (injected noise) against the oracle: loss finite and equal to 2e-5, every gradient to 3e-4 of its maximum."""
    import torch
    from conftest import draw_noise
    from oracle import ntf_oracle as O
    from opentf_amd import libntf
    torch.manual_seed(31)
    rng = np.random.default_rng(31)
    D, H, M, B, S = 128, 128, 8000, 128, 300
    skill, table, member = _dataset(rng, B, S, D, M, 4.0, 2.5)
    sd = O.bnn_init(D, [H], M)
    sd["layers.1.mu_weight"] *= 10.0                                     # (weights of a trained model's scale: with |h| ~ 2 000 a third of the outlier row's pre-activations fall below -2 250)
    row = 7
    s0 = int(skill[1][skill[0][row]])                                   # one of row 7's skills: its embedding scaled until the largest hidden activation of the batch reaches ~2 000
    base = table[s0].copy()

    def hidden_max(a):
        table[s0] = base * a
        x = torch.from_numpy(O.gather_meanpool_fast(skill[0], skill[1], table))      # (every row that has this skill moves with it: the largest of them is what is bounded)
        return float(torch.nn.functional.leaky_relu(x @ sd["layers.0.mu_weight"].T + sd["layers.0.mu_bias"]).abs().max())
    lo_a, hi_a = 1.0, 1e5
    for _ in range(60):
        mid = (lo_a * hi_a) ** 0.5
        if hidden_max(mid) < 2000.0: lo_a = mid
        else: hi_a = mid
    assert 1500.0 < hidden_max(lo_a) < 2100.0
    X = torch.from_numpy(O.gather_meanpool_fast(skill[0], skill[1], table))
    y = torch.zeros(B, M)
    for k in range(B): y[k, member[1][member[0][k]: member[0][k + 1]].astype(np.int64)] = 1.0
    noise = draw_noise(sd, B); neg = O.ns_uniform(y, 5)
    z = O.model_forward(sd, X, noise)
    assert int((z < -22.5).sum()) > 200, (int((z < -22.5).sum()), float(z.min()))     # deep in the overflow region (the hidden activation itself stays inside the fp16 window: 4 094)
    inj = {"neg_idx": neg.numpy(), "eps_w": [n["eps_w"] for n in noise], "eps_b": [n["eps_b"] for n in noise], "s_in": [n["s_in"] for n in noise], "s_out": [n["s_out"] for n in noise]}
    ref_loss, ref_grads = O.loss_and_grads(sd, X, y, neg, 10.0, 1.0, noise)
    e = libntf.Engine([D, H, M], bayesian=True, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=5, nsd="uniform", tpw=10.0, tnw=1.0, lr=1e-3, fuse_adam=0)
    e.set_skill_table(table); e.set_skill_csr(skill); e.set_member(member); e.load_state_dict(sd)
    loss = e.backward(np.arange(B), inject=inj)
    assert e.range_fallbacks() == 0                                          # the fp16x3 kernels ran (the activation is inside their window)
    assert np.isfinite(loss) and abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (loss, ref_loss)
    g = e.grads(); e.close()
    for k in sd:
        ref = ref_grads[k].numpy()
        assert float(np.abs(g[k] - ref).max()) <= 3e-4 * float(np.abs(ref).max()), (k, float(np.abs(g[k] - ref).max()), float(np.abs(ref).max()))
