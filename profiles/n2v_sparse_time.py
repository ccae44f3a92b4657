"""Dense against sparse Adam (ntf_n2v_set_optimizer) of the node2vec and metapath2vec trainers at the bench dataset's size: dblp mt10.ts2 shapes from make_dataset,
d = 128, the reference's settings as profiles/m2v_time.py has them (B = 1000, w 5, wn 10, ns 5; walks of 5 nodes for n2v, of 6 nodes over
member -> team -> skill -> team -> member for m2v).  One dense and one sparse handle per producer, alternating rounds; the rows a batch touches are counted from
last_windows().

  python profiles/n2v_sparse_time.py                  both producers, six alternating rounds of 30 batches each
  python profiles/n2v_sparse_time.py kernels n2v|m2v  a short run of the sparse route alone for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...)
Results: profiles/n2v_sparse_bench.md."""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf
from opentf_amd.mdl.emb.gnn import m2v_graph, stm_graph
from opentf_amd.synth import make_dataset

B, CTX, WN, NS, LR, D = 1000, 5, 10, 5, 1e-3, 128
NODES = {"n2v": 5, "m2v": 6}
METAPATH = [("member", "to", "team"), ("team", "rev_to", "skill"), ("skill", "to", "team"), ("team", "rev_to", "member")]
ROUNDS, K = 6, 30

ds = make_dataset("dblp", d=D, seed=0)
N, S, M = ds["N"], ds["S"], ds["M"]
skill = sp.csr_matrix((np.ones(len(ds["skill"][1]), np.uint8), ds["skill"][1], ds["skill"][0]), shape=(N, S))
member = sp.csr_matrix((np.ones(len(ds["member"][1]), np.uint8), ds["member"][1], ds["member"][0]), shape=(N, M))
perm = np.random.default_rng(2).permutation(N)
n_test = int(0.15 * N)
drop = np.concatenate([perm[:n_test], perm[n_test:][::3]])


def producer(which):
    """-> make(sparse) -> handle, the number of table rows, the loader's range"""
    if which == "m2v":
        counts, off, hops = m2v_graph(skill, member, drop, METAPATH)
        n = off["dummy"] + 1
        w = np.random.default_rng(0).standard_normal((n, D)).astype(np.float32)
        return (lambda sparse: libntf.MetaPath2Vec(counts, hops, w, seed=0, sparse=sparse)), n, M
    rowptr, col, off, n = stm_graph(skill, member, drop)
    w = np.random.default_rng(0).standard_normal((n, D)).astype(np.float32)
    return (lambda sparse: libntf.Node2Vec(rowptr, col, w, seed=0, sparse=sparse)), n, n


def run(net, order, nodes, k, first):
    """k batches, the loss of the last one read back (one synchronisation): ms per batch"""
    t0 = time.perf_counter()
    for i in range(k):
        o = ((first + i) * B) % (len(order) - B)
        net.train_batch(order[o:o + B], nodes, CTX, WN, NS, LR, want_loss=(i == k - 1))
    return (time.perf_counter() - t0) / k * 1e3


def touched(net):
    pos, neg = net.last_windows()
    return len(np.unique(np.concatenate([pos.ravel(), neg.ravel()]))), pos.size + neg.size


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    which = sys.argv[2]
    make, n, n_start = producer(which)
    net = make(True)
    order = np.random.default_rng(1).permutation(n_start)
    print(f"{which} sparse: {run(net, order, NODES[which], 20, 0):.3f} ms per batch over 20 batches", flush=True)
    sys.exit(0)

for which in ("n2v", "m2v"):
    t0 = time.perf_counter()
    make, n, n_start = producer(which)
    print(f"{which}: table [{n}, {D}], loader over {n_start} nodes, graph in {time.perf_counter() - t0:.1f} s", flush=True)
    order = np.random.default_rng(1).permutation(n_start)
    nets = [make(False), make(True)]
    for net in nets: run(net, order, NODES[which], 1, 0)
    rows = []
    for i in range(3):
        r, e = touched(nets[1]); rows.append(r)
        run(nets[1], order, NODES[which], 1, 1 + i); run(nets[0], order, NODES[which], 1, 1 + i)
    print(f"{which}: rows touched per batch {rows} of {n} ({np.mean(rows) / n:.4f} of the table), {e} window entries per batch", flush=True)
    ms = [[], []]
    for r in range(ROUNDS):
        for route in ((0, 1) if r % 2 == 0 else (1, 0)):
            ms[route].append(run(nets[route], order, NODES[which], K, 4 + r * K))
        print(f"{which} round {r}: dense {ms[0][-1]:.3f} ms, sparse {ms[1][-1]:.3f} ms per batch", flush=True)
    for route, name in ((0, "dense Adam"), (1, "sparse Adam")):
        a = np.array(ms[route])
        print(f"{which} {name}: mean {a.mean():.3f} ms, median {np.median(a):.3f}, min {a.min():.3f}, max {a.max():.3f}, spread (max - min) {a.max() - a.min():.3f} "
              f"over {ROUNDS} rounds of {K} batches", flush=True)
    for net in nets: net.close()
