"""What the engine's host code (opentf_amd/csrc/ntf_engine.hip) makes the kernels compute, as one SHA-256 per quantity of every case, with the launches it issued:
two libraries of the same ABI launch the same kernels on the same arguments exactly when every line agrees (the suites' tolerances would let a reordered launch,
another stream or another Adam coefficient through).

    NTF_LIB_PATH=<the other build>/libopentf_amd.so python profiles/engine_bits.py > a.txt;  python profiles/engine_bits.py > b.txt;  diff a.txt b.txt

One process per library.  A line is `<case> <quantity> <sha256>`; the loss lines also carry the values (their sums use floating atomics: where one library does
not reproduce them from run to run they are compared by value, profiles/engine_refactor_check.md); a `calls` line holds the per-family launch counts of
kernel_times(True) and the counters prefetched_steps / head_prefetch_hits / first_layer_sweeps / mc_fused_passes / range_fallbacks of the case's engine.
ENGINE_BITS_DUMP=<dir> also keeps every quantity's arrays there.  Cases a-k: the table of profiles/engine_refactor_check.md."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch                                                    # noqa: E402
from opentf_amd import libntf                                   # noqa: E402
from opentf_amd.synth import init_params, make_dataset, zipf_csr  # noqa: E402

M_SMALL = 3000
SWITCHES = ("NTF_INFER_MC", "NTF_INFER_F32", "NTF_SIDE_BWD")
DUMP = os.environ.get("ENGINE_BITS_DUMP")      # a directory: every quantity's arrays as <case>.<quantity>.npz too (for the quantities one library does not reproduce)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays: h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def out(case, what, *arrays, show=None):
    if DUMP: np.savez(os.path.join(DUMP, f"{case}.{what}.npz"), *[np.asarray(a) for a in arrays])
    print(f"{case} {what} {digest(*arrays)}" + ("" if show is None else " " + " ".join(repr(float(v)) for v in show)), flush=True)


def dataset(n_rows, d, M, S=None):
    ds = make_dataset("dblp", d=d, seed=3, n_rows=n_rows, n_experts=M)
    if S: ds["S"] = S; ds["skill"] = zipf_csr(n_rows, S, 8.57, 7)
    ds["X"] = np.random.default_rng(11).standard_normal((n_rows, d)).astype(np.float32) * 0.1
    return ds


def engine(ds, dims, bayesian=True, mode="meanpool", max_batch=96, nsd="uniform", fuse_adam=1, shard=None, world=1, sd=None):
    e = libntf.Engine(dims, bayesian=bayesian, input_mode={"meanpool": libntf.INPUT_MEANPOOL, "dense": libntf.INPUT_DENSE, "multihot": libntf.INPUT_MULTIHOT}[mode],
                      max_batch=max_batch, ns=5, nsd=nsd, tpw=10.0, tnw=1.0, lr=1e-3, seed=5, fuse_adam=fuse_adam, expert_shard=shard, ep_world=world)
    if mode == "dense": e.set_dense_input(ds["X"])
    else:
        if mode == "meanpool": e.set_skill_table(ds["table"])
        e.set_skill_csr(ds["skill"])
    e.set_member(ds["member"])
    e.load_state_dict(sd or init_params(dims[:-1] + [ds["M"]], bayesian, 0))
    if nsd == "unigram": e.set_unigram(np.bincount(ds["member"][1], minlength=ds["M"]) / ds["N"])
    e.kernel_times(True)
    return e


def flat(e):
    e.synchronize()
    m, v = e.moment_tensors()
    return [t.cpu().numpy() for t in (e.param_tensor(), m, v)]


def state(case, e, tag="state"):
    out(case, tag, *flat(e))
    e.params_touched()        # (param_tensor took the raw view: both libraries drop their prefetched operands here alike)


def grads(case, e, tag="grads"):
    out(case, tag, *e.grads().values())


def calls(case, e):
    kt = e.kernel_times(True)
    print(f"{case} calls " + " ".join(f"{k}={c}" for k, (_, c) in kt.items()) + f" | prefetched_steps={e.prefetched_steps()} head_prefetch_hits={e.head_prefetch_hits()} "
          f"first_layer_sweeps={e.first_layer_sweeps()} mc_fused_passes={e.mc_fused_passes()} range_fallbacks={e.range_fallbacks()}", flush=True)


def staged_case(case, e, B, n):
    """a staged order of five batches whose last is short: two train epochs (prefetch hits), a step on another batch than the prefetched one (one stale head),
    an evaluation epoch (the lean chain), then the single-call entries"""
    order = np.random.default_rng(1).permutation(n)[: 4 * B + B // 2 - 8]
    losses = [e.train_epoch(order, B), e.train_epoch(order, B)]
    state(case, e, "state-epochs")
    e.stage_order(order)
    losses += [e.step_staged(0, B, want_loss=True), e.step_staged(2 * B, B, want_loss=True), e.step_staged(3 * B, B, want_loss=True)]
    out(case, "negatives", e.negatives(B))
    s, k = e.epoch_loss()
    losses += [s, k, e.eval_epoch(order, B)]
    rows = order[:B]
    losses += [e.train_step(rows), e.eval_step(rows[: B - 7]), e.backward(rows[: B - 7])]
    grads(case, e); out(case, "dlogits", e.dlogits(B - 7)); out(case, "negatives-backward", e.negatives(B - 7))
    e.apply()
    losses += [e.train_step(rows[:33])]
    state(case, e)
    out(case, "losses", np.asarray(losses, np.float64), show=losses)
    calls(case, e)


def inference(case, e, ds, B):
    rows = np.arange(B)
    out(case, "logits", e.logits(rows))
    p, pu, mu = e.forward(rows, nmc=3, uncertainty=True)
    out(case, "forward-probs", p); out(case, "forward-unc", pu, mu)
    v, i, pu, mu = e.forward_topk(rows, 10, nmc=3, uncertainty=True)
    out(case, "forward_topk", v, i); out(case, "forward_topk-unc", pu, mu)
    srows = np.flatnonzero(np.diff(ds["member"][0]) > 0)[: 2 * B + 5]
    r = e.score_rows(srows, B, nmc=2, K=0, cutoffs=(2, 5, 10), auc=True, K_out=10)
    out(case, "score_rows-dense", r.metrics, np.asarray(r.counts, np.uint64), np.float64(r.auc), r.vals, r.idx)
    r = e.score_rows(srows, B, nmc=2, K=16, cutoffs=(2, 5, 10), auc=True, K_out=16)
    out(case, "score_rows-k16", r.metrics, np.asarray(r.counts, np.uint64), np.float64(r.auc), r.vals, r.idx)
    calls(case, e)


def injected(dims, B, M):
    rng = np.random.default_rng(21)
    L = len(dims) - 1
    sign = lambda *s: np.where(rng.random(s) < 0.5, -1.0, 1.0).astype(np.float32)
    return {"eps_w": [rng.standard_normal((dims[l + 1], dims[l])).astype(np.float32) for l in range(L)], "eps_b": [rng.standard_normal(dims[l + 1]).astype(np.float32) for l in range(L)],
            "s_in": [sign(B, dims[l]) for l in range(L)], "s_out": [sign(B, dims[l + 1]) for l in range(L)], "neg_idx": rng.integers(0, M, (B, 5))}


def main():
    for k in SWITCHES: os.environ.pop(k, None)
    N = 700
    ds = dataset(N, 64, M_SMALL)
    dims = [64, 128, M_SMALL]
    e = engine(ds, dims); staged_case("a", e, 96, N); e.close()
    e = engine(ds, dims, bayesian=False, mode="dense"); staged_case("b", e, 96, N); e.close()
    dsm = dataset(N, 64, M_SMALL, S=300)
    e = engine(dsm, [300, 128, M_SMALL], mode="multihot"); staged_case("c", e, 96, N); e.close()
    for nsd in ("unigram", "unigram_b"):
        e = engine(ds, dims, nsd=nsd); staged_case(f"d-{nsd}", e, 96, N); e.close()
    dse = dataset(2800, 64, M_SMALL)
    e = engine(dse, dims, max_batch=600); staged_case("e", e, 600, 2800); e.close()
    e = engine(ds, dims, fuse_adam=2); staged_case("f", e, 96, N); e.close()
    for H in (64, 96, 48):
        e = engine(ds, [64, H, M_SMALL]); case = f"g-h{H}"
        losses = [e.train_step(np.arange(96)), e.train_step(np.arange(96, 180))]
        state(case, e); p, pu, mu = e.forward(np.arange(50), nmc=2, uncertainty=True); out(case, "forward-probs", p); out(case, "forward-unc", pu, mu); out(case, "losses", np.asarray(losses, np.float64), show=losses)
        calls(case, e); e.close()
    e = engine(ds, dims)
    losses = [e.train_step(np.arange(96)), e.train_step(np.arange(90), inject=injected(dims, 90, M_SMALL)), e.train_step(np.arange(96))]
    state("h", e); out("h", "losses", np.asarray(losses, np.float64), show=losses); calls("h", e); e.close()

    # i: two dW chunks and two forward ranges (the smallest M for which ntf_fwd_ranges returns 2 at B = 160)
    Mi = 65600
    dsi = dataset(400, 64, Mi)
    e = engine(dsi, [64, 128, Mi], max_batch=160, fuse_adam=0)
    e.stage_order(np.arange(400))
    print(f"i ranges fwd_ranges={e.fwd_ranges(160)} dw_chunks={e.dw_chunks()} " + " ".join(str(e.dw_chunk_range(k)) for k in range(e.dw_chunks())), flush=True)
    for tag, cb in (("plain", None), ("cb", lambda j: None)):
        for off in (0, 160):
            e.step_staged_deferred(off, 160, off, 160, before_range=cb)
            for k in range(e.dw_chunks()): e.dw_chunk(k)
            if off == 0: grads(f"i-{tag}", e); out(f"i-{tag}", "dlogits", e.dlogits(160))
            spans = [e.dw_chunk_range(k) for k in range(e.dw_chunks())]
            e.apply_ranges(e.rest_ranges() + [(o, o + cnt) for ow, orr, cnt in spans for o in (ow, orr)])
        state(f"i-{tag}", e)
    s, k = e.epoch_loss(); out("i", "epoch_loss", np.float64(s), np.int64(k), show=[s, k]); calls("i", e); e.close()

    # j: two expert shards of M = 3072 in one process, the d(hidden) sum done here
    Mj = 3072
    dsj = dataset(N, 64, Mj)
    for sb in ("1", "0"):
        os.environ["NTF_SIDE_BWD"] = sb
        for nsd in ("uniform", "unigram_b"):
            case = f"j-side{sb}-{nsd}"
            es = [engine(dsj, [64, 128, Mj], nsd=nsd, shard=sh, world=2, sd=init_params([64, 128, Mj], True, 0)) for sh in ((0, 1536), (1536, Mj))]
            order = np.random.default_rng(2).permutation(N)[:424]
            for e in es: e.stage_order(order)
            for off in range(0, 424, 96):
                b = min(96, 424 - off)
                for e in es: e.step_staged_ep(off, b, 1); e.synchronize()
                dh = [e.dh_tensor() for e in es]
                tot = torch.stack([d[: b * 128] for d in dh]).sum(0)
                for d in dh: d[: b * 128].copy_(tot)
                torch.cuda.synchronize()
                for e in es: e.step_staged_ep(off, b, 2); e.step_staged_ep(off, b, 3)
            for r, e in enumerate(es):
                s, k = e.epoch_loss()
                state(f"{case}-r{r}", e); out(f"{case}-r{r}", "epoch_loss", np.float64(s), np.int64(k), show=[s, k]); calls(f"{case}-r{r}", e); e.close()
    os.environ.pop("NTF_SIDE_BWD")

    # k: inference, under the default, NTF_INFER_MC=1 and NTF_INFER_F32=0; `big`: one weight outside the fp16x3 window (the range fallback's arm)
    big = init_params(dims, True, 0); big["layers.1.mu_weight"][5, 7] = 300.0
    for env in ({}, {"NTF_INFER_MC": "1"}, {"NTF_INFER_F32": "0"}):
        os.environ.update(env)
        tag = "-".join(f"{k[4:]}{v}" for k, v in env.items()) or "default"
        for name, d, sd in (("h128", dims, None), ("h128-big", dims, big), ("h64", [64, 64, M_SMALL], None), ("fnn", dims, None)):
            e = engine(ds, d, bayesian=name != "fnn", sd=sd); inference(f"k-{name}-{tag}", e, ds, 50); e.close()
        for k in env: os.environ.pop(k)


if __name__ == "__main__":
    main()
