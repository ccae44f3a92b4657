"""Fused Monte-Carlo inference (NTF_INFER_MC=1, read when an engine is created): the MC passes of a Flipout call at h[-1] = 128 inside k_out_probs_mc, against the
per-pass arm (NTF_INFER_MC=0: one k_out_fwd_b6 launch per pass, oracle-checked by test_gpu_infer_f32.py, test_gpu_round3.py and test_gpu_replay.py).  Both arms get the
same seed and the same call sequence, so they draw the same noise.

probs, the top-K and pred_unc are BIT-EQUAL between the arms: the fp16 planes of mu, sigma * eps and h are the same, the MFMA order per accumulator is the same, the
running sum acc = fmaf(pr, 1 / nmc, acc) runs in the same pass order from the same start, and pred_unc is taken from the transposed sums by the same kernels.

model_unc = ent_mean - ent_mc.  ent_mc = (1 / nmc) * sum over passes and experts of t = -p ln(p + 1e-15) >= 0, and every t is the same f32 number in both arms (it goes
into its tile sum by one fmaf in both); only the ORDER of that one f32 sum differs.  A recursive f32 sum of non-negative terms along a tree whose longest chain has d
additions is within d * 2^-24 of the exact sum, relatively (each addition's rounding is at most 2^-24 of a partial sum that never exceeds the total; first order in
2^-24, d < 1000 here).  So |ent_mc(new) - ent_mc(old)| <= (d_new + d_old) * 2^-24 * ent_mc with
  d_new = 16              the lane's 16 terms of a tile (fmaf chain into LossAcc.tile)
        + tiles * passes  the tile sums of one launch in a column group (tiles of the column group x passes of the group; LossAcc adds them with compensation,
                          whose error is smaller than the plain sum's - counted as that many plain additions)
        + 1               the lane-half shuffle add
        + (groups - 1)    a later pass group adds its partial onto the slot the earlier one left (pacc)
        + ncg_tot         k_ent_slots: the slots of every range's column groups, one after the other
        + 2               times 1 / nmc, added to the zeroed ent_mc
  d_old = 16 + tiles + 1 + ncg + 2     one pass, as above with the per-pass kernel's column groups (eval_ncg)
        + (passes - 1)                 ent_mc += each later pass
The interface returns model_unc, not ent_mc: model_unc = fl(ent_mean - ent_mc) on the host, ent_mean bit-equal, so the two model_unc differ by at most the ent_mc
difference plus the two subtractions' own roundings, 2^-24 * |model_unc| each.  The bound is not tuned to what is observed (DESIGN.md section 8 #6 records both)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FUSED = "out_fused_fwd_loss_dh"
H = 128
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    import random
    import torch
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


def _bytes(group, rng):
    return group * rng * (4 * H + 4) + rng * 4 * H


def _cdiv(a, b):
    return -(-a // b)


def _depths(B, M, passes, budget):
    """longest chains of additions of the two arms' ent_mc sums (module docstring); the column groups are those of ntf_fused_common.h (geom / eval_ncg)"""
    from opentf_amd import libntf
    group, rng = libntf.infer_mc_plan(M, H, passes, budget)
    nrb = _cdiv(B, 128)
    ncg_tot, tiles_new = 0, 0
    for lo in range(0, M, rng):
        n = min(M, lo + rng) - lo
        ncg = max(1, min(256 // nrb, _cdiv(n, 64)))
        ncg_tot += ncg
        tiles_new = max(tiles_new, _cdiv(_cdiv(n, 32), ncg))
    d_new = 16 + tiles_new * group + 1 + (_cdiv(passes, group) - 1) + ncg_tot + 2
    ncg_old = max(1, min(2 * 256 // nrb, _cdiv(M, 64), 256))
    d_old = 16 + _cdiv(_cdiv(M, 32), ncg_old) + 1 + ncg_old + 2 + (passes - 1)
    return d_new, d_old


def _dense(dims, B, seed=5, bayesian=True, mfma=None, tweak=None):
    """engine on dims with dense input; tweak(sd) edits the oracle-initialised parameters first"""
    import torch
    from oracle import ntf_oracle as O
    from test_gpu_parity import _engine
    torch.manual_seed(seed)
    sd = (O.bnn_init if bayesian else O.fnn_init)(dims[0], list(dims[1:-1]), dims[-1])
    if tweak: tweak(sd)
    X = torch.randn(B, dims[0]).numpy()
    e = _engine(list(dims), bayesian=bayesian, max_batch=B, ns=5, nsd="uniform", lr=1e-3, mfma=mfma)
    e.load_state_dict(sd); e.set_dense_input(X)
    return e, sd


def _calls(e, B, nmc, K=10):
    rows = np.arange(B, dtype=np.int64)
    e.set_seed(3, 11)
    f0, m0 = e.range_fallbacks(), e.mc_fused_passes()
    probs, pu, mu = e.forward(rows, nmc=nmc, uncertainty=True)
    vals, idx, pu2, mu2 = e.forward_topk(rows, min(K, e.dims[-1]), nmc=nmc, uncertainty=True)
    return {"probs": probs, "pu": pu, "mu": mu, "vals": vals, "idx": idx, "pu2": pu2, "mu2": mu2,
            "fallbacks": e.range_fallbacks() - f0, "mc": e.mc_fused_passes() - m0}


def _arms(monkeypatch, make, B, nmc, budget=None):
    """the same engine and calls under NTF_INFER_MC=1 and =0"""
    out = []
    if budget is not None: monkeypatch.setenv("NTF_INFER_MC_BYTES", str(budget))
    for arm in ("1", "0"):
        monkeypatch.setenv("NTF_INFER_MC", arm)
        e = make()
        out.append(_calls(e, B, nmc))
        e.close()
    return out


def _check(new, old, B, M, nmc, budget=2 << 30, fused=True):
    for k in ("probs", "pu", "vals", "idx", "pu2"):
        assert np.array_equal(new[k], old[k]), k
    assert old["mc"] == 0 and new["mc"] == (2 * nmc if fused else 0)
    assert new["fallbacks"] == old["fallbacks"]
    d_new, d_old = (_depths(B, M, nmc, budget) if fused else (0, 0))
    for a, b, pu in ((new["mu"], old["mu"], old["pu"]), (new["mu2"], old["mu2"], old["pu2"])):
        a, b, pu = a.astype(np.float64), b.astype(np.float64), pu.astype(np.float64)
        ent_mc = (pu - b) * (1 + 2.0 ** -20)      # (the reference arm's, recovered to 2^-24 |model_unc|: rounded up)
        bound = (d_new + d_old) * U * ent_mc + U * (np.abs(a) + np.abs(b))
        diff = np.abs(a - b)
        print(f"model_unc: largest difference {diff.max():.3e} (largest relative to ent_mc {(diff / ent_mc).max():.3e}); bound {bound.min():.3e} .. {bound.max():.3e}, "
              f"d_new {d_new} d_old {d_old}")
        assert (diff <= bound).all()
        if not fused: assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ a. tile groups
def test_tile_groups_ragged_rows_and_tiles(monkeypatch):
    """B = 150: rows 128-149 in a ragged second row block, hence 128 column groups; M: every column group walks two full tile groups and a partial one, one of them a
    tile more, and the layer's last tile is ragged"""
    from opentf_amd import libntf
    B, nmc, G = 150, 3, libntf.NTF_MC_TILE_GROUP
    ncg = 256 // _cdiv(B, 128)
    M = ncg * 32 * (2 * G + 1) + 5
    new, old = _arms(monkeypatch, lambda: _dense([64, H, M], B)[0], B, nmc)
    _check(new, old, B, M, nmc)


# ------------------------------------------------------------------------------------------ b. short column groups, one row
@pytest.mark.parametrize("M", [300, 260, 33])
def test_single_tile_groups_one_row(monkeypatch, M):
    """M = 300: five column groups of two tiles; 260: column groups of one and of two tiles; 33: one column group, its second tile one expert wide"""
    B, nmc = 1, 2
    new, old = _arms(monkeypatch, lambda: _dense([64, H, M], B)[0], B, nmc)
    _check(new, old, B, M, nmc)


# ------------------------------------------------------------------------------------------ c. pass groups chained through pacc; expert ranges
def test_pass_groups_chain_through_the_transposed_buffer(monkeypatch):
    from opentf_amd import libntf
    B, nmc, M = 129, 5, 3000
    budget = _bytes(3, 256) - 1
    assert libntf.infer_mc_plan(M, H, nmc, budget) == (2, 256)      # groups of 2, 2 and 1 passes (over twelve ranges)
    new, old = _arms(monkeypatch, lambda: _dense([64, H, M], B)[0], B, nmc, budget)
    _check(new, old, B, M, nmc, budget)


def test_expert_ranges_with_a_short_last_one(monkeypatch):
    from opentf_amd import libntf
    B, nmc, M = 129, 3, 3000
    budget = _bytes(3, 1024)
    assert libntf.infer_mc_plan(M, H, nmc, budget) == (3, 1024)     # ranges of 1024, 1024 and 952 experts
    new, old = _arms(monkeypatch, lambda: _dense([64, H, M], B)[0], B, nmc, budget)
    _check(new, old, B, M, nmc, budget)


# ------------------------------------------------------------------------------------------ d. hidden layers that differ per pass
def test_two_flipout_hidden_layers(monkeypatch):
    B, nmc, M = 129, 3, 3000
    new, old = _arms(monkeypatch, lambda: _dense([40, 64, H, M], B)[0], B, nmc)
    _check(new, old, B, M, nmc)


def test_multihot_first_layer(monkeypatch):
    """layer 0 is the Flipout gather-sum over the skill CSR"""
    import torch
    from opentf_amd import libntf
    from oracle import ntf_oracle as O
    from test_gpu_parity import _engine, _csr_from_dense
    S, M, B, nmc = 500, 3000, 129, 3
    rng = np.random.default_rng(S)
    Xd = np.zeros((B, S), np.float32)
    for i in range(B):
        Xd[i, rng.choice(S, 1 + rng.poisson(7.5), replace=False)] = 1

    def make():
        torch.manual_seed(3)
        sd = O.bnn_init(S, [H], M)
        e = _engine([S, H, M], bayesian=True, input_mode=libntf.INPUT_MULTIHOT, max_batch=B, ns=5, nsd="uniform", lr=1e-3)
        e.load_state_dict(sd); e.set_skill_csr(_csr_from_dense(Xd))
        return e
    new, old = _arms(monkeypatch, make, B, nmc)
    _check(new, old, B, M, nmc)


# ------------------------------------------------------------------------------------------ e. range fallback
def test_range_fallback_redoes_the_call_on_the_per_pass_path(monkeypatch):
    """one output-layer weight of 300 is outside the fp16 window at scale 256: the fused-MC launches are discarded, the call runs again on the exact-f32 kernel"""
    B, nmc, M = 129, 3, 3000

    def tweak(sd):
        sd["layers.1.mu_weight"][7, 5] = 300.0
    new, old = _arms(monkeypatch, lambda: _dense([64, H, M], B, tweak=tweak)[0], B, nmc)
    assert old["fallbacks"] == 2 and new["fallbacks"] == 2
    _check(new, old, B, M, nmc, fused=False)


# ------------------------------------------------------------------------------------------ f. expert shards
def test_expert_shards_infer_the_whole_engines_columns(monkeypatch):
    from opentf_amd.synth import make_dataset
    from test_gpu_ep import _mk
    monkeypatch.setenv("NTF_INFER_MC", "1")
    B, nmc = 200, 3
    ds = make_dataset("dblp", d=128, seed=3, n_rows=600, n_experts=3000)
    M = ds["M"]
    dims = [128, H, M]
    rows = np.arange(B, dtype=np.int64)
    full = _mk(ds, dims, True, B, "uniform")
    p_full = full.forward(rows, nmc=nmc)
    assert full.mc_fused_passes() == nmc
    full.close()
    cols = []
    for s in ((0, 1536), (1536, M)):
        e = _mk(ds, dims, True, B, "uniform", shard=s, world=2)
        cols.append(e.forward(rows, nmc=nmc))
        assert e.mc_fused_passes() == nmc
        e.close()
    assert np.array_equal(np.concatenate(cols, axis=1), p_full)


# ------------------------------------------------------------------------------------------ g. path and counter
def _train_after_inference(monkeypatch, arm):
    from opentf_amd.synth import make_dataset
    from test_gpu_ep import _mk
    monkeypatch.setenv("NTF_INFER_MC", arm)
    B = 200
    ds = make_dataset("dblp", d=128, seed=7, n_rows=400, n_experts=20_000)
    e = _mk(ds, [128, H, ds["M"]], True, B, "uniform")
    rows = np.arange(B, dtype=np.int64)
    e.train_step(rows)      # leaves the next step's operands prefetched: the inference call must invalidate them
    counts = []
    for call in (lambda: e.forward(rows, nmc=3), lambda: e.forward_topk(rows, 10, nmc=3)):
        m0 = e.mc_fused_passes()
        e.kernel_times(True)
        call()
        counts.append((e.mc_fused_passes() - m0, int(e.kernel_times(False)[FUSED][1])))
    loss = e.train_step(rows)
    w = e.state_dict()["layers.1.mu_weight"].copy()
    e.close()
    return counts, loss, w


def test_path_counter_and_the_step_after(monkeypatch):
    c1, loss1, w1 = _train_after_inference(monkeypatch, "1")
    c0, loss0, w0 = _train_after_inference(monkeypatch, "0")
    assert c1 == [(3, 1), (3, 1)]      # three passes, ONE launch of the fused forward family (one range)
    assert c0 == [(0, 3), (0, 3)]
    assert loss1 == loss0 and np.array_equal(w1, w0)


@pytest.mark.parametrize("case", ["fnn", "nmc1", "injects", "f32", "h64", "h256"])
def test_everything_else_keeps_the_per_pass_path(monkeypatch, case):
    from conftest import draw_noise
    monkeypatch.setenv("NTF_INFER_MC", "1")
    B, M = 129, 3000
    h = {"h64": 64, "h256": 256}.get(case, H)
    e, sd = _dense([64, h, M], B, bayesian=case != "fnn", mfma="f32" if case == "f32" else None)
    rows = np.arange(B, dtype=np.int64)
    nmc = 1 if case == "nmc1" else 3
    injs = None
    if case == "injects":
        noises = [draw_noise(sd, B) for _ in range(nmc)]
        injs = [{"eps_w": [n["eps_w"] for n in nz], "eps_b": [n["eps_b"] for n in nz], "s_in": [n["s_in"] for n in nz], "s_out": [n["s_out"] for n in nz]} for nz in noises]
    e.forward(rows, nmc=nmc, injects=injs)
    if case != "injects": e.forward_topk(rows, 10, nmc=nmc)
    assert e.mc_fused_passes() == 0
    e.close()


def test_switch_off_never_counts(monkeypatch):
    monkeypatch.delenv("NTF_INFER_MC", raising=False)
    B, M = 129, 3000
    e, _ = _dense([64, H, M], B)
    e.forward(np.arange(B, dtype=np.int64), nmc=3)
    assert e.mc_fused_passes() == 0
    e.close()
