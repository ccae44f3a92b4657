#!/usr/bin/env python3
"""Scoring a prediction set inside the engine (`ntf_score_rows`, `Engine.score_rows`) timed against the route it replaces, on the same engine, rows and seed:

  dense   score_rows(K = 0)    against   `forward` loop -> [n, M] on the host -> `micro_auc_device` (upload + count) -> `calculate_metrics` (host ranking + kernel)
  top-K   score_rows(K = 100)  against   `forward_topk` loop -> CSR on the host -> `micro_auc_device` (CSR) -> `calculate_metrics`

  score_time.py [--n 2000] [--experts 233629] [--batch 1000] [--models fnn,bnn] [--nmc 10] [--modes dense,topk] [--K 100] [--rounds 5] [--host-rank-rounds 5] [--out FILE]

Every line is a host clock around a call that ends synchronised.  The two routes of a (model, mode) pair alternate, `--rounds` times, after one untimed call of
each.  The replaced route is timed in its three parts (inference + copy to the host, AUC, ranking metrics); it does NOT include writing and reading the `.pred`
file, which evaluate() pays on top.  Its dense ranking is a stable argsort of the whole [n, M] matrix on the host (`_ranked_topk`), tens of seconds at dblp's
width: `--host-rank-rounds` limits in how many of the rounds that part runs (the line says in how many it did).  Both routes must agree: the integers P, N, U2
EQUAL, the metric table bit for bit - checked in every round, a mismatch ends the run."""
import argparse, json, os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf
from opentf_amd.evl import metric
from opentf_amd.synth import init_params, make_dataset

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--experts", type=int, default=233629)
ap.add_argument("--batch", type=int, default=1000)
ap.add_argument("--models", default="fnn,bnn")
ap.add_argument("--nmc", type=int, default=10)
ap.add_argument("--modes", default="dense,topk")
ap.add_argument("--K", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-rank-rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

NAMES = ["P_2,5,10", "recall_2,5,10", "ndcg_cut_2,5,10", "map_cut_2,5,10", "success_2,5,10"]
CUTS = [2, 5, 10]
n, M, B = a.n, a.experts, a.batch
ds = make_dataset("dblp", d=128, seed=0, n_rows=n, n_experts=M)
rows = np.arange(n, dtype=np.int64)
ip, ix = ds["member"]
Y = sp.csr_matrix((np.ones(len(ix), np.float32), ix, ip), shape=(n, M))
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(json.dumps(r) for r in lines) + "\n")


def ms(t0):
    return round((time.perf_counter() - t0) * 1e3, 2)


def new_route(e, nmc, K):
    e.set_seed(0, 0)
    t0 = time.perf_counter()
    res = e.score_rows(rows, B, nmc=nmc, K=K, cutoffs=CUTS, auc=True)
    return ms(t0), res


def old_route(e, nmc, K, rank):
    """-> ({part: ms}, counts, metric table or None)"""
    e.set_seed(0, 0)
    t = {}
    t0 = time.perf_counter()
    if K:
        parts = [e.forward_topk(rows[o:o + B], K, nmc=nmc) for o in range(0, n, B)]
        v, i = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        o = np.argsort(i, axis=1, kind="stable")
        S = sp.csr_matrix((np.take_along_axis(v, o, 1).ravel(), np.take_along_axis(i, o, 1).ravel(), np.arange(0, n * K + 1, K)), shape=(n, M))
    else:
        S = np.concatenate([e.forward(rows[o:o + B], nmc=nmc) for o in range(0, n, B)])
    t["infer_ms"] = ms(t0)
    t0 = time.perf_counter()
    _, counts = metric.micro_auc_device(Y, S, return_counts=True)
    t["auc_ms"] = ms(t0)
    table = None
    if rank:
        t0 = time.perf_counter()
        df, _ = metric.calculate_metrics(Y, S, K or None, True, NAMES)
        t["metrics_ms"] = ms(t0)
        table = df.values
    return t, counts, table


for model in a.models.split(","):
    bayesian = model == "bnn"
    nmc = a.nmc if bayesian else 1
    dims = [128, 128, M]
    e = libntf.Engine(dims, bayesian=bayesian, input_mode=libntf.INPUT_MEANPOOL, max_batch=B, ns=0, nsd=None)
    e.set_skill_table(ds["table"]); e.set_skill_csr(ds["skill"]); e.set_member(ds["member"])
    e.load_state_dict(init_params(dims, bayesian, 0))
    for mode in a.modes.split(","):
        K = a.K if mode == "topk" else 0
        new_route(e, nmc, K); old_route(e, nmc, K, rank=bool(K))                      # untimed: code objects, allocations (the dense host ranking is not warmed: it is host code)
        new_ms, old = [], {"infer_ms": [], "auc_ms": [], "metrics_ms": []}
        for r in range(a.rounds):
            rank = bool(K) or r < a.host_rank_rounds
            t_new, res = new_route(e, nmc, K)
            t_old, counts, table = old_route(e, nmc, K, rank)
            if tuple(counts) != res.counts: sys.exit(f"{model} {mode}: counts differ: {counts} != {res.counts}")
            if table is not None:
                got = metric._metric_frames(res.metrics, CUTS, NAMES, True)[0].values
                if not np.array_equal(got, table): sys.exit(f"{model} {mode}: metric tables differ")
            new_ms.append(t_new)
            for k, v in t_old.items(): old[k].append(v)
        med = lambda x: float(np.median(x)) if len(x) else None
        old_total = med(old["infer_ms"]) + med(old["auc_ms"]) + (med(old["metrics_ms"]) or 0.0)
        emit({"model": model, "mode": mode, "n": n, "M": M, "B": B, "nmc": nmc, "K": K, "rounds": a.rounds, "score_rows_ms": new_ms, "score_rows_ms_median": med(new_ms),
              "replaced_infer_ms": old["infer_ms"], "replaced_auc_ms": old["auc_ms"], "replaced_metrics_ms": old["metrics_ms"],
              "replaced_ms_median_sum": round(old_total, 2), "host_rank_rounds": len(old["metrics_ms"]), "counts": list(res.counts), "auc": res.auc,
              "range_fallbacks": e.range_fallbacks()})
    e.close()
