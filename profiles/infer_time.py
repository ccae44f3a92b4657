#!/usr/bin/env python3
"""`test()`'s inference (src/mdl/fnn.py:200-211 + src/pkgmgr.py:125-134) timed at config 2's expert count: ntf_forward_topk of 1 000 teams, K = 100, Bnn at nmc = 10
and nmc = 1 and Fnn, with the per-family kernel times.

  infer_time.py [--h 128] [--switch NTF_INFER_F32] [--arms 1,0] [--rounds 3] [--json FILE]

--switch: the environment switch whose values --arms lists (read when an engine is created).  NTF_INFER_F32 (the default): 1 = the fused exact-f32 inference kernel
where no split planes exist, 0 = the generic chain there.  NTF_INFER_MC: 1 = the Monte-Carlo passes of a Bnn call at h = 128 inside one kernel, 0 = one pass per launch.
One engine per arm lives through the whole run and the arms are timed in turn, round after round, so that clock and temperature drift falls on both alike (every arm's parameters and [B, M] buffers are resident at once: ~2 GB an arm at h = 256)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf
from opentf_amd.synth import make_dataset, init_params

ap = argparse.ArgumentParser()
ap.add_argument("--h", type=int, default=128)
ap.add_argument("--switch", default="NTF_INFER_F32")
ap.add_argument("--arms", default="1")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
a = ap.parse_args()
arms = a.arms.split(",")
ds = make_dataset("dblp", d=128, seed=0, n_rows=20000)
dims = [128, a.h, ds["M"]]
rows = np.arange(1000)
out = []
for bayes, nmc in ((True, 10), (True, 1), (False, 1)):
    eng = {}
    for arm in arms:
        os.environ[a.switch] = arm
        e = libntf.Engine(dims, bayesian=bayes, input_mode=libntf.INPUT_MEANPOOL, max_batch=1000, ns=5, nsd="uniform", seed=3, fuse_adam=1)
        e.set_skill_table(ds["table"]); e.set_skill_csr(ds["skill"]); e.set_member(ds["member"]); e.load_state_dict(init_params(dims, bayes, 0))
        e.forward_topk(rows, nmc=nmc, K=100)
        eng[arm] = e
    ms = {arm: [] for arm in arms}
    for _round in range(a.rounds):
        for arm in arms:
            t0 = time.perf_counter()
            for _ in range(5): eng[arm].forward_topk(rows, nmc=nmc, K=100)      # (timed without events; the call returns the top-K to the host, i.e. it is synchronous)
            ms[arm].append((time.perf_counter() - t0) / 5 * 1e3)
    for arm in arms:
        e = eng[arm]
        e.kernel_times(enable=True)
        for _ in range(5): e.forward_topk(rows, nmc=nmc, K=100)      # (a second loop with events around every kernel family, for the breakdown only)
        fam = {k: round(v[0] / 5, 3) for k, v in e.kernel_times(enable=False).items() if v[1]}
        rec = {"h": a.h, "bayes": bayes, "nmc": nmc, a.switch: arm, "ms_rounds": [round(x, 3) for x in ms[arm]], "ms_median": round(float(np.median(ms[arm])), 3), "families_ms": fam}
        out.append(rec)
        print("h", a.h, "bayes", bayes, "nmc", nmc, a.switch, arm, "forward_topk(1000 teams, K=100):", rec["ms_median"], "ms (median of", rec["ms_rounds"], ")", fam, flush=True)
        e.close()
if a.json:
    with open(a.json, "w") as f: json.dump(out, f, indent=1)
