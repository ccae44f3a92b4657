#!/usr/bin/env python3
"""`ntf_fair_rerank` (include/opentf_amd_fair.h) timed against the sequential host restatement of the same algorithms (tests/fair_reference.py) on the same box:
n = 2 000 and n = 100 000 ranked rows, K = 100, G = 2, the three algorithms.

  fair_time.py [--rounds 5] [--ref-rows 2000] [--json FILE]

The device call is timed as a whole (it is synchronous: the re-ranked lists come back to the host) and split into upload / kernel / download by the library's own
clock (NTF_FAIR_TIMES=1: one line on stderr per call, read back here).  The host reference is a Python loop per row; it is timed on the first --ref-rows rows and
its time for n rows is that figure scaled by n / ref-rows (rows are independent and alike)."""
import argparse, json, os, re, sys, tempfile, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fair_reference as R
from opentf_amd import libntf

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--ref-rows", type=int, default=2000)
ap.add_argument("--json", default=None)
a = ap.parse_args()


def phases(fn):
    """fn() with fd 2 in a file: -> (result, {upload, kernel, download} ms from the library's line)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2); os.dup2(f.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0); m = re.search(rb"upload ([\d.]+) ms kernel ([\d.]+) ms download ([\d.]+) ms", f.read())
    return res, ({k: float(v) for k, v in zip(("upload", "kernel", "download"), m.groups())} if m else None)


K, G, E = 100, 2, 50_000
rng = np.random.default_rng(0)
group = (rng.random(E) < 0.2).astype(np.uint8)
p = np.array([[0.8, 0.2]])
out = []
for n in (2_000, 100_000):
    idx = np.argsort(rng.random((n, 2 * K)), axis=1)[:, :K].astype(np.int32) + rng.integers(0, E - 2 * K, (n, 1)).astype(np.int32)     # K distinct ids a row
    val = -np.sort(-rng.random((n, K)).astype(np.float32), axis=1)
    for alg in ("det_greedy", "det_cons", "det_relaxed"):
        libntf.fair_rerank(idx, val, group, p, alg)                                   # warm-up (the first call loads the code object)
        os.environ["NTF_FAIR_TIMES"] = "0"
        ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter(); got = libntf.fair_rerank(idx, val, group, p, alg, want_pos=True); ms.append((time.perf_counter() - t0) * 1e3)
        os.environ["NTF_FAIR_TIMES"] = "1"
        split = [phases(lambda: libntf.fair_rerank(idx, val, group, p, alg, want_pos=True))[1] for _ in range(a.rounds)]
        os.environ["NTF_FAIR_TIMES"] = "0"
        m = min(n, a.ref_rows)
        li, lg, lp = idx[:m].tolist(), group.tolist(), p.tolist()
        t0 = time.perf_counter(); ref = R.rerank(li, None, lg, lp, libntf.FAIR_ALGORITHMS[alg], K); ref_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(np.array(ref[2], np.int32), got[2][:m])
        rec = {"n": n, "K": K, "G": G, "algorithm": alg, "device_call_ms_median": round(float(np.median(ms)), 3), "device_call_ms_rounds": [round(x, 3) for x in ms],
               **{f"{k}_ms_median": round(float(np.median([s[k] for s in split])), 3) for k in ("upload", "kernel", "download")},
               "host_reference_rows_timed": m, "host_reference_ms_per_row": round(ref_ms / m, 4), "host_reference_ms_for_n": round(ref_ms / m * n, 1)}
        rec["speedup_whole_call"] = round(rec["host_reference_ms_for_n"] / rec["device_call_ms_median"], 1)
        out.append(rec)
        print(json.dumps(rec), flush=True)
if a.json:
    with open(a.json, "w") as f: json.dump(out, f, indent=1)
