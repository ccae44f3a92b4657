#!/usr/bin/env python3
"""The eval stage's micro ROC curve (`aucroc+`, src/evl/metric.py:36-41) timed on the device against sklearn's roc_curve, and the AUC entries timed from two
builds of the library to show that the curve's arm left their kernels alone.

  roc_time.py [--shapes small,dblp_topk] [--rounds 3] [--host-limit-gb 8] [--parent-lib PATH] [--json FILE]

The shapes are those of profiles/auc_bench.md: small = 500 x 20 000 dense, dblp_topk = 2 000 x 233 629 as a top-100 CSR, each with uniform scores and with the
zero-heavy family (90 % exact zeros).  Part 1, per shape: `micro_roc_device` and `micro_auc_device` in alternating calls, each timed whole, with the library's own
upload / kernel split (NTF_AUC_TIMING=1: an `ntf_roc:` or `ntf_auc:` line on stderr, read back here) - the new arm against the count-only arm on the same input;
and sklearn's `roc_curve` on the same arrays (a dense pair that would need more than --host-limit-gb is reported as "not run").  Part 2, with --parent-lib (a
libopentf_amd.so built from the parent commit): `ntf_auc_micro_dense` on the small shapes from this build and from that one in alternating fresh processes
(NTF_LIB_PATH), `--rounds` processes each, three timed calls a process; the kernel time of each call and the spread over the rounds are reported."""
import argparse, json, os, re, subprocess, sys, tempfile, time
import numpy as np
import scipy.sparse as sp
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
os.environ["NTF_AUC_TIMING"] = "1"

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="small,dblp_topk")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--host-limit-gb", type=float, default=8.0)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--json", default=None)
ap.add_argument("--child", default=None, help="(internal) family of the small shape: time ntf_auc_micro_dense with the library NTF_LIB_PATH names and print one JSON line")
a = ap.parse_args()
SHAPES = {"small": (500, 20000, None), "dblp": (2000, 233629, None), "dblp_topk": (2000, 233629, 100)}
LINE = re.compile(r"(ntf_\w+): .*G = (\d+) \((\w+) counters\): upload ([\d.]+) ms, kernel ([\d.]+) ms")


def truth(n, M, rng, per_row=5):
    cols = np.sort(rng.integers(0, M, (n, per_row)), axis=1)
    Y = sp.csr_matrix((np.ones(n * per_row, np.float32), cols.ravel(), np.arange(0, n * per_row + 1, per_row)), shape=(n, M))
    Y.sum_duplicates(); Y.data[:] = 1
    return Y


def dense_scores(n, M, fam, rng):
    S = rng.random((n, M), dtype=np.float32)
    if fam == "zero_heavy":
        S[rng.random(S.shape, dtype=np.float32) < 0.9] = 0.0
    return S


def topk_scores(n, M, K, fam, rng, Y):
    """K stored entries a row, the row's truth columns among them"""
    ix = np.empty((n, K), dtype=np.int32)
    for i in range(n):
        t = Y.indices[Y.indptr[i]:Y.indptr[i + 1]]
        c = np.unique(np.concatenate([t, rng.integers(0, M, 2 * K)]))
        ix[i] = np.sort(np.concatenate([t, np.setdiff1d(c, t)[:K - len(t)]]))
    v = rng.random((n, K), dtype=np.float32)
    if fam == "zero_heavy":
        v[rng.random((n, K)) < 0.9] = 0.0
    return sp.csr_matrix((v.ravel(), ix.ravel(), np.arange(0, n * K + 1, K)), shape=(n, M))


def inputs(shape, fam):
    """the generators of profiles/auc_time.py, same seed"""
    n, M, K = SHAPES[shape]
    rng = np.random.default_rng(5)
    Y = truth(n, M, rng)
    return Y, (dense_scores(n, M, fam, rng) if K is None else topk_scores(n, M, K, fam, rng, Y))


def with_stderr(fn):
    """fn() with the process's stderr (the library's fprintf included) read back: -> (value, wall ms, [(entry, G, counters, upload ms, kernel ms)])"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        keep = os.dup(2); os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter(); val = fn(); ms = (time.perf_counter() - t0) * 1e3
        finally:
            os.dup2(keep, 2); os.close(keep)
        tmp.seek(0); text = tmp.read().decode(errors="replace")
    return val, ms, [(m[0], int(m[1]), m[2], float(m[3]), float(m[4])) for m in LINE.findall(text)]


def spread(x):
    return round((max(x) - min(x)) / float(np.median(x)) * 100, 1)


if a.child:
    # the entry called through a binding of its own: a parent build has no ntf_roc_* for libntf.lib() to bind
    import ctypes as C
    import torch  # noqa: F401  (the HIP runtime the library shares)
    from opentf_amd import libntf
    l = C.CDLL(os.environ.get("NTF_LIB_PATH") or libntf._LIB_PATH)
    fn = l.ntf_auc_micro_dense
    fn.restype, fn.argtypes = libntf.SYMBOLS["ntf_auc_micro_dense"]
    Y, S = inputs("small", a.child)
    n, M = S.shape
    ip, ix = np.ascontiguousarray(Y.indptr, dtype=np.int64), np.ascontiguousarray(Y.indices, dtype=np.int32)
    counts, auc = np.zeros(3, dtype=np.uint64), C.c_double()
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def call():
        assert fn(0, p(S), n, M, M, p(ip), p(ix), n, None, 0, p(counts), C.byref(auc)) == 0
    call()                                                                                 # first call: HIP start-up, code object load
    kernel = [with_stderr(call)[2][0][4] for _ in range(3)]
    print(json.dumps({"lib": os.environ.get("NTF_LIB_PATH") or "this build", "family": a.child, "kernel_ms": kernel, "counts": [int(c) for c in counts]}), flush=True)
    sys.exit(0)

from opentf_amd.evl import metric
out = []
for shape in [s for s in a.shapes.split(",") if s]:
    n, M, K = SHAPES[shape]
    for fam in ("uniform", "zero_heavy"):
        Y, S = inputs(shape, fam)
        print(f"--- {shape} {fam}: n {n} M {M} " + (f"dense, {n * M * 4 / 1e9:.2f} GB" if K is None else f"top-{K} CSR, {S.nnz} stored"), flush=True)
        metric.micro_roc_device(Y, S); metric.micro_auc_device(Y, S)                       # first calls: HIP start-up, code object load
        rec = {"shape": shape, "family": fam, "roc_ms": [], "roc_upload_ms": [], "roc_kernel_ms": [], "auc_ms": [], "auc_upload_ms": [], "auc_kernel_ms": []}
        for _ in range(a.rounds):
            for name, fn in (("roc", metric.micro_roc_device), ("auc", metric.micro_auc_device)):
                val, ms, lines = with_stderr(lambda: fn(Y, S, return_counts=True))
                rec[f"{name}_ms"].append(round(ms, 2)); rec[f"{name}_upload_ms"].append(lines[0][3]); rec[f"{name}_kernel_ms"].append(lines[0][4])
                rec["G"], rec["counters"] = lines[0][1], lines[0][2]
                if name == "roc": rec["points"], roc_counts = len(val[0]), val[3]
                else: assert val[1] == roc_counts
        need_gb = n * M * (8 + 8 + 8 + 8 + 1) / 1e9                                        # roc_curve: f64 scores, argsort indices, sorted copy, cumulative sums, labels
        if need_gb > a.host_limit_gb:
            rec["sklearn_roc_curve"] = f"not run: needs {need_gb:.0f} GB"
        else:
            from sklearn import metrics as skm
            y, s = Y.toarray().ravel(), (S.toarray() if sp.issparse(S) else S).ravel()
            t0 = time.perf_counter(); fpr, tpr, _ = skm.roc_curve(y, s); rec["sklearn_roc_curve_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["sklearn_points"] = len(fpr)
        out.append(rec)
        print(json.dumps(rec), flush=True)

if a.parent_lib:
    print(f"--- ntf_auc_micro_dense, this build against {a.parent_lib}: kernel ms of 3 calls per fresh process, {a.rounds} alternating rounds", flush=True)
    for fam in ("uniform", "zero_heavy"):
        ab = {"this": [], "parent": []}
        for _ in range(a.rounds):
            for who, lib in (("this", ""), ("parent", os.path.abspath(a.parent_lib))):
                env = dict(os.environ); env.pop("NTF_LIB_PATH", None)
                if lib: env["NTF_LIB_PATH"] = lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", fam], env=env, capture_output=True, text=True, timeout=300, check=True)
                ab[who].append(json.loads(r.stdout.strip().splitlines()[-1])["kernel_ms"])
        rec = {"ab_family": fam}
        for who in ab:
            med = [float(np.median(k)) for k in ab[who]]                                   # one median per round
            rec[who] = {"kernel_ms_rounds": ab[who], "round_medians": med, "median": float(np.median(med)), "spread_over_rounds_pct": spread(med)}
        rec["this_minus_parent_pct"] = round((rec["this"]["median"] / rec["parent"]["median"] - 1) * 100, 1)
        out.append(rec)
        print(json.dumps(rec), flush=True)
if a.json:
    with open(a.json, "w") as f: json.dump(out, f, indent=1)
