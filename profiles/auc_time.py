#!/usr/bin/env python3
"""The eval stage's micro-averaged ROC AUC (src/evl/metric.py:36-41) timed on the device against the host routes it replaces: `ntf_auc_micro_dense` against sklearn's
roc_auc_score on the dense pair, `ntf_auc_micro_csr` against `micro_auc_sparse` (numpy).  The host routes are the reference, never the code under test.

  auc_time.py [--shapes small,dblp,dblp_topk] [--rounds 3] [--host-limit-gb 8] [--json FILE]

small = 500 x 20 000 dense; dblp = 2 000 x 233 629 dense (1.9 GB of scores); dblp_topk = the same shape as a top-100 CSR.  Each with uniform scores and with the
zero-heavy family (90 % exact zeros: where contention on one counter would show).  A call is timed whole (host validation, the positives' table, uploads, kernels,
the integer finish); with NTF_AUC_TIMING=1 the library reports how much of it was upload and how much kernel, and the kernel's rate over the 4 bytes a score is read
against the HBM peak.  A host route that would need more than --host-limit-gb of memory is reported as "not run"."""
import argparse, json, os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["NTF_AUC_TIMING"] = "1"
from opentf_amd.evl import metric

HBM_PEAK = 8.0e12     # bytes / s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="small,dblp,dblp_topk")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--host-limit-gb", type=float, default=8.0)
ap.add_argument("--json", default=None)
a = ap.parse_args()
SHAPES = {"small": (500, 20000, None), "dblp": (2000, 233629, None), "dblp_topk": (2000, 233629, 100)}


def truth(n, M, rng, per_row=5):
    cols = np.sort(rng.integers(0, M, (n, per_row)), axis=1)
    Y = sp.csr_matrix((np.ones(n * per_row, np.float32), cols.ravel(), np.arange(0, n * per_row + 1, per_row)), shape=(n, M))
    Y.sum_duplicates(); Y.data[:] = 1
    return Y


def dense_scores(n, M, fam, rng):
    S = np.empty((n, M), dtype=np.float32)
    for r0 in range(0, n, 250):              # in slabs: no second full-size temporary
        s = rng.random((min(250, n - r0), M), dtype=np.float32)
        if fam == "zero_heavy":
            s[rng.random(s.shape, dtype=np.float32) < 0.9] = 0.0
        S[r0:r0 + len(s)] = s
    return S


def topk_scores(n, M, K, fam, rng, Y):
    """K stored entries a row, the row's truth columns among them"""
    ix = np.empty((n, K), dtype=np.int32)
    for i in range(n):
        t = Y.indices[Y.indptr[i]:Y.indptr[i + 1]]
        c = np.unique(np.concatenate([t, rng.integers(0, M, 2 * K)]))
        extra = np.setdiff1d(c, t)[:K - len(t)]
        ix[i] = np.sort(np.concatenate([t, extra]))
    v = rng.random((n, K), dtype=np.float32)
    if fam == "zero_heavy":
        v[rng.random((n, K)) < 0.9] = 0.0
    return sp.csr_matrix((v.ravel(), ix.ravel(), np.arange(0, n * K + 1, K)), shape=(n, M))


def timed(fn, rounds):
    ms, val = [], None
    for _ in range(rounds):
        t0 = time.perf_counter(); val = fn(); ms.append((time.perf_counter() - t0) * 1e3)
    return val, [round(x, 2) for x in ms]


out = []
for shape in a.shapes.split(","):
    n, M, K = SHAPES[shape]
    for fam in ("uniform", "zero_heavy"):
        rng = np.random.default_rng(5)
        Y = truth(n, M, rng)
        S = dense_scores(n, M, fam, rng) if K is None else topk_scores(n, M, K, fam, rng, Y)
        n_scores = n * M if K is None else S.nnz
        print(f"--- {shape} {fam}: n {n} M {M} " + (f"dense, {n_scores * 4 / 1e9:.2f} GB" if K is None else f"top-{K} CSR, {n_scores} stored"), flush=True)
        metric.micro_auc_device(Y, S)                                                      # first call: HIP start-up, code object load
        (auc, counts), dev_ms = timed(lambda: metric.micro_auc_device(Y, S, return_counts=True), a.rounds)
        rec = {"shape": shape, "family": fam, "n": n, "M": M, "K": K, "device_ms_rounds": dev_ms, "device_ms_median": float(np.median(dev_ms)),
               "counts": list(counts), "auc": auc}
        need_gb = n * M * (8 + 8 + 8 + 1) / 1e9 if K is None else 0.0        # sklearn: f64 copy of the scores, argsort indices, sorted copy, labels
        if need_gb > a.host_limit_gb:
            rec["host"] = f"not run: needs {need_gb:.0f} GB"
        else:
            host_auc, host_ms = timed(lambda: metric.calculate_auc_roc(Y, S)[0], 1)
            rec.update(host_ms=host_ms[0], host_route="micro_auc_sparse" if K is not None else "sklearn", abs_diff=abs(host_auc - auc))
        out.append(rec)
        print(json.dumps(rec), flush=True)
if a.json:
    with open(a.json, "w") as f: json.dump(out, f, indent=1)
