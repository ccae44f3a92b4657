#!/usr/bin/env python3
"""`ntf_fair_constsort` (include/opentf_amd_fairsort.h) timed beside `ntf_fair_rerank`'s DetCons on the same input and against the sequential host restatement
(tests/fair_sort_reference.py) on the same box: n = 2 000 ranked rows at K = 100, G = 2 and at K = 2048, G = 2 and G = 64; plus the skewed-target worst case at
K = 2048 (a group owed 0.5 % whose candidates head the input: each of its entries passes two hundred ranks).

  fair_sort_time.py [--rounds 5] [--ref-rows 20] [--json FILE]

As in fair_time.py: the device call is timed as a whole and split into upload / kernel / download by the library's own clock (NTF_FAIR_TIMES=1).  The two
algorithms alternate round by round.  The host reference is timed on the first --ref-rows rows and scaled to n."""
import argparse, json, os, re, sys, tempfile, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fair_sort_reference as S
from opentf_amd import libntf

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--ref-rows", type=int, default=20)
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
    return res, {k: float(v) for k, v in zip(("upload", "kernel", "download"), m.groups())}


def shape(name, n, K, G, rng):
    """ranked rows of K distinct ids; expert e belongs to group e % G"""
    E = G * max(50_000 // G, 2 * K)
    if name == "worst":                     # p = (0.995, 0.005) and the group owed 0.5 % first in every row
        p = np.array([[0.995, 0.005]])
        n1 = K // 200 + 1                   # what it is owed in K ranks, and one
        idx = np.concatenate([1 + 2 * np.argsort(rng.random((n, E // 2)), axis=1)[:, :n1], 2 * np.argsort(rng.random((n, E // 2)), axis=1)[:, :K - n1]], axis=1)
    else:                                   # a nearly flat target; every candidate's group is drawn from it, so the rows' composition follows it on average
        q = 0.5 + rng.random(G); p = (q / q.sum()).reshape(1, G)
        idx = np.stack([rng.choice(G, size=K, p=p[0]) + G * rng.permutation(E // G)[:K] for _ in range(n)])
    return idx.astype(np.int32), (np.arange(E) % G).astype(np.uint8), p


rng = np.random.default_rng(0)
out = []
for name, n, K, G in (("flat", 2000, 100, 2), ("flat", 2000, 2048, 2), ("flat", 2000, 2048, 64), ("worst", 2000, 2048, 2)):
    idx, group, p = shape(name, n, K, G, rng)
    val = -np.sort(-rng.random((n, K)).astype(np.float32), axis=1)
    calls = {"det_const_sort": lambda: libntf.fair_constsort(idx, val, group, p, want_pos=True, want_tail=True),
             "det_cons": lambda: libntf.fair_rerank(idx, val, group, p, "det_cons", want_pos=True)}
    for fn in calls.values(): fn()                                                    # warm-up (the first call loads the code object)
    ms, split = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(a.rounds):                                                         # alternating rounds
        for k, fn in calls.items():
            os.environ["NTF_FAIR_TIMES"] = "0"
            t0 = time.perf_counter(); got = fn(); ms[k].append((time.perf_counter() - t0) * 1e3)
            os.environ["NTF_FAIR_TIMES"] = "1"
            split[k].append(phases(fn)[1])
            os.environ["NTF_FAIR_TIMES"] = "0"
    got = calls["det_const_sort"]()
    m = min(n, a.ref_rows)
    li, lg, lp = idx[:m].tolist(), group.tolist(), p.tolist()
    st = {}
    t0 = time.perf_counter(); ref = S.constsort(li, lg, lp, K, stats=st); ref_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(np.array(ref[1], np.int32), got[2][:m]) and np.array_equal(np.array(ref[2], np.int32), got[3][:m])
    for k in calls:
        rec = {"shape": name, "n": n, "K": K, "G": G, "algorithm": k, "device_call_ms_median": round(float(np.median(ms[k])), 3),
               "device_call_ms_rounds": [round(x, 3) for x in ms[k]],
               **{f"{ph}_ms_median": round(float(np.median([s[ph] for s in split[k]])), 3) for ph in ("upload", "kernel", "download")}}
        if k == "det_const_sort":
            rec.update({"rows_with_tail": int((got[3] > 0).sum()), "longest_insertion_in_ref_rows": st["longest"], "host_reference_rows_timed": m,
                        "host_reference_ms_per_row": round(ref_ms / m, 3), "host_reference_ms_for_n": round(ref_ms / m * n, 1)})
        out.append(rec)
        print(json.dumps(rec), flush=True)
if a.json:
    with open(a.json, "w") as f: json.dump(out, f, indent=1)
