"""metapath2vec trainer (ntf_m2v_create) at the bench dataset's size: dblp mt10.ts2 shapes (90 671 skills, 233 629 members, 1 995 708 teams), the metapath
member -> team -> skill -> team -> member, batches of 1000 start members with the reference's settings (w 5 / wl 5 steps = 6 nodes / wn 10 / ns 5), d = 128.
The member edges of 15 % test teams and of one of three validation folds of the rest are dropped, as Gnn.learn drops them.

  python profiles/m2v_time.py            the dummy share, the A/B of the two forms of the pair kernel in alternating rounds, an n2v batch on the same node count
  python profiles/m2v_time.py kernels 0  a short run of one route (0 = k_n2v_pairs<NV, false>, 1 = k_n2v_pairs<NV, true>, the dummy form) for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...)
Results: profiles/m2v_bench.md."""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf
from opentf_amd.mdl.emb.gnn import m2v_graph, stm_graph
from opentf_amd.synth import make_dataset

B, NODES, CTX, WN, NS, LR, D = 1000, 6, 5, 10, 5, 1e-3, 128
METAPATH = [("member", "to", "team"), ("team", "rev_to", "skill"), ("skill", "to", "team"), ("team", "rev_to", "member")]

ds = make_dataset("dblp", d=D, seed=0)
N, S, M = ds["N"], ds["S"], ds["M"]
skill = sp.csr_matrix((np.ones(len(ds["skill"][1]), np.uint8), ds["skill"][1], ds["skill"][0]), shape=(N, S))
member = sp.csr_matrix((np.ones(len(ds["member"][1]), np.uint8), ds["member"][1], ds["member"][0]), shape=(N, M))
perm = np.random.default_rng(2).permutation(N)
n_test = int(0.15 * N)
drop = np.concatenate([perm[:n_test], perm[n_test:][::3]])
t0 = time.perf_counter()
counts, off, hops = m2v_graph(skill, member, drop, METAPATH)
print(f"m2v graph: {counts} nodes (member, skill, team), {len(drop)} of {N} teams dropped, {time.perf_counter() - t0:.1f} s", flush=True)
n = off["dummy"] + 1
w = np.random.default_rng(0).standard_normal((n, D)).astype(np.float32)
order = np.random.default_rng(1).permutation(M)


def make(route):
    os.environ["NTF_M2V_PAIRS"] = str(route)
    return libntf.MetaPath2Vec(counts, hops, w, seed=0)


def run(net, k, first, n_start):
    """k batches, the loss of the last one read back (one synchronisation): ms per batch"""
    t0 = time.perf_counter()
    for i in range(k):
        o = ((first + i) * B) % (n_start - B)
        net.train_batch(order_of[net][o:o + B], *args_of[net], LR, want_loss=(i == k - 1))
    return (time.perf_counter() - t0) / k * 1e3


order_of, args_of = {}, {}
if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    net = make(int(sys.argv[2])); order_of[net] = order; args_of[net] = (NODES, CTX, WN, NS)
    print(f"route {sys.argv[2]}: {run(net, 20, 0, M):.3f} ms per batch over 20 batches", flush=True)
    sys.exit(0)

nets = [make(0), make(1)]
for net in nets: order_of[net] = order; args_of[net] = (NODES, CTX, WN, NS)
nets[0].train_batch(order[:B], NODES, CTX, WN, NS, LR)
pos, neg = nets[0].last_windows()
dummy = off["dummy"]
pp = ((pos[:, 1:] == dummy) | (pos[:, :1] == dummy)).mean(); pn = ((neg[:, 1:] == dummy) | (neg[:, :1] == dummy)).mean()
share = (pp * pos.shape[0] + pn * neg.shape[0]) / (pos.shape[0] + neg.shape[0])
print(f"pairs that name the dummy row: {pp:.4f} of the positive, {pn:.4f} of the negative, {share:.4f} of all ({pos.shape[0]} + {neg.shape[0]} window rows of {CTX})", flush=True)
nets[1].train_batch(order[:B], NODES, CTX, WN, NS, LR)
rounds, k = 6, 30
ms = [[], []]
for r in range(rounds):
    for route in ((0, 1) if r % 2 == 0 else (1, 0)):
        ms[route].append(run(nets[route], k, 1 + r * k, M))
    print(f"round {r}: pairs plain {ms[0][-1]:.3f} ms, pairs dummy {ms[1][-1]:.3f} ms per batch", flush=True)
for route, name in ((0, "pairs plain (k_n2v_pairs<2, false>)"), (1, "pairs dummy (k_n2v_pairs<2, true>)")):
    a = np.array(ms[route])
    print(f"{name}: mean {a.mean():.3f} ms, median {np.median(a):.3f}, min {a.min():.3f}, max {a.max():.3f}, spread (max - min) {a.max() - a.min():.3f} over {rounds} rounds of {k} batches")
for net in nets: net.close()

# the yardstick for the shared kernels: an n2v batch over the same nodes (all types in one graph; 5 nodes per walk = cfg.wl 5)
rowptr, col, off2, n2 = stm_graph(skill, member, drop)
net = libntf.Node2Vec(rowptr, col, w[:n2], seed=0)
order_of[net] = np.random.default_rng(1).permutation(n2); args_of[net] = (5, CTX, WN, NS)
run(net, 1, 0, n2)
a = np.array([run(net, k, 1 + r * k, n2) for r in range(3)])
print(f"n2v on the same {n2} nodes, walks of 5 nodes: {a.mean():.3f} ms per batch (rounds {a.round(3).tolist()})")
