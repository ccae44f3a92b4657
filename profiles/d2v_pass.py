"""doc2vec passes over the bench's dblp-shaped corpus (the program profiled for profiles/r3_d2v_kernel_stats.csv); D2V_DIM=64|128|192|256: the vector width (default 128).
One untimed pass of each kind, then six timed PV-DM and four timed PV-DBOW passes (device ms) and their mean / min / max / spread.  Successive passes train the
tables, so the times drift slowly across the rounds - the same drift whatever library NTF_LIB_PATH names (profiles/d2v_refactor_check.md compares two)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf                      # noqa: E402
from opentf_amd.mdl.emb import d2v as P            # noqa: E402
from opentf_amd.synth import make_dataset          # noqa: E402

ds = make_dataset("dblp", d=128, seed=0)
ptr, idx = ds["skill"][0], ds["skill"][1]
keys, count, si, cum, wi = P.build_vocab(idx)
dim = int(os.environ.get("D2V_DIM", "128"))
wv, dv = P.initial_vectors(len(ptr) - 1, len(keys), dim, 0)
net = libntf.Doc2Vec(ptr, wi, si, cum, wv, dv, seed=0)
prog = P.job_progress(ptr)
for dm in (1, 0): net.train_epoch(dm, 5, 0.025, 0.001, 0, progress=prog)
for dm, rounds, name in ((1, 6, "PV-DM"), (0, 4, "PV-DBOW")):
    ms = []
    for r in range(rounds):
        loss, m = net.train_epoch(dm, 5, 0.025, 0.001, 0, progress=prog, want_loss=True, want_ms=True)
        ms.append(m)
        print(f"dm={dm} round {r}: {len(idx)} words, {m:.1f} ms, mean pair loss {loss:.4f}", flush=True)
    a = np.array(ms)
    print(f"{name} d {dim}: mean {a.mean():.3f} ms, median {np.median(a):.3f}, min {a.min():.3f}, max {a.max():.3f}, spread (max - min) {a.max() - a.min():.3f} over {rounds} passes")
net.close()
