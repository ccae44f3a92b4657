"""Dense, sparse and lazy dense Adam (ntf_n2v_set_lazy) of the node2vec and metapath2vec trainers at the bench dataset's size: the shapes and settings of
profiles/n2v_sparse_time.py (dblp mt10.ts2 from make_dataset, d = 128, B = 1000, w 5, wn 10, ns 5; walks of 5 nodes for n2v, of 6 for m2v).  One handle per
optimiser and producer in one run, alternating rounds.  The yardstick of the lazy arm is the dense arm of the same run.

  python profiles/n2v_lazy_time.py                  both producers: six alternating rounds of 30 batches; one full flush after 100, 1000 and 2320 lazy steps
                                                    (2320 = one dblp epoch of n2v batches); one edge_bce over a fold's validation edges on each handle; an epoch's
                                                    worth of batches with the flush that ends it, lazy against dense
  python profiles/n2v_lazy_time.py kernels n2v|m2v  a short run of the lazy route alone for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...)
Results: profiles/n2v_lazy_bench.md."""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf
from opentf_amd.mdl.emb.gnn import m2v_graph, member_team_edges, stm_graph
from opentf_amd.synth import make_dataset

B, CTX, WN, NS, LR, D = 1000, 5, 10, 5, 1e-3, 128
NODES = {"n2v": 5, "m2v": 6}
METAPATH = [("member", "to", "team"), ("team", "rev_to", "skill"), ("skill", "to", "team"), ("team", "rev_to", "member")]
ROUNDS, K = 6, 30
FLUSH_AFTER = (100, 1000, 2320)
EPOCH = 2320
ARMS = ("dense", "sparse", "lazy")

ds = make_dataset("dblp", d=D, seed=0)
N, S, M = ds["N"], ds["S"], ds["M"]
skill = sp.csr_matrix((np.ones(len(ds["skill"][1]), np.uint8), ds["skill"][1], ds["skill"][0]), shape=(N, S))
member = sp.csr_matrix((np.ones(len(ds["member"][1]), np.uint8), ds["member"][1], ds["member"][0]), shape=(N, M))
perm = np.random.default_rng(2).permutation(N)
n_test = int(0.15 * N)
valid = perm[n_test:][::3]
drop = np.concatenate([perm[:n_test], valid])


def producer(which):
    """-> make(arm) -> handle, the number of table rows, the loader's range, the validation edges (global rows)"""
    if which == "m2v":
        counts, off, hops = m2v_graph(skill, member, drop, METAPATH)
        n = off["dummy"] + 1
        w = np.random.default_rng(0).standard_normal((n, D)).astype(np.float32)
        return (lambda arm: libntf.MetaPath2Vec(counts, hops, w, seed=0, sparse=arm == "sparse", lazy=arm == "lazy")), n, M, member_team_edges(member, valid, off)
    rowptr, col, off, n = stm_graph(skill, member, drop)
    w = np.random.default_rng(0).standard_normal((n, D)).astype(np.float32)
    return (lambda arm: libntf.Node2Vec(rowptr, col, w, seed=0, sparse=arm == "sparse", lazy=arm == "lazy")), n, n, member_team_edges(member, valid, off)


def run(net, order, nodes, k, first):
    """k batches, the loss of the last one read back (one synchronisation): ms per batch"""
    t0 = time.perf_counter()
    for i in range(k):
        o = ((first + i) * B) % (len(order) - B)
        net.train_batch(order[o:o + B], nodes, CTX, WN, NS, LR, want_loss=(i == k - 1))
    return (time.perf_counter() - t0) / k * 1e3


def flush_ms(net):
    """one full flush and nothing else: ntf_n2v_moments with no destination brings every row up to date and waits for the stream (the batches before it were
    waited for by their last loss)"""
    t0 = time.perf_counter()
    net._ck(libntf.lib().ntf_n2v_moments(net._h, None, None))
    return (time.perf_counter() - t0) * 1e3


def edge_ms(net, src, dst, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); net.edge_bce(src, dst); out.append((time.perf_counter() - t0) * 1e3)
    return out


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    which = sys.argv[2]
    make, n, n_start, edges = producer(which)
    net = make("lazy")
    order = np.random.default_rng(1).permutation(n_start)
    print(f"{which} lazy: {run(net, order, NODES[which], 200, 0):.3f} ms per batch over 200 batches", flush=True)
    print(f"{which} lazy: full flush after 200 steps {flush_ms(net):.3f} ms", flush=True)
    sys.exit(0)

for which in ("n2v", "m2v"):
    t0 = time.perf_counter()
    make, n, n_start, (vsrc, vdst) = producer(which)
    print(f"{which}: table [{n}, {D}], loader over {n_start} nodes, {len(vsrc)} validation edges, graph in {time.perf_counter() - t0:.1f} s", flush=True)
    order = np.random.default_rng(1).permutation(n_start)
    nets = {arm: make(arm) for arm in ARMS}
    for net in nets.values(): run(net, order, NODES[which], 4, 0)
    ms = {arm: [] for arm in ARMS}
    for r in range(ROUNDS):
        for arm in (ARMS if r % 2 == 0 else ARMS[::-1]):
            ms[arm].append(run(nets[arm], order, NODES[which], K, 4 + r * K))
        print(f"{which} round {r}: " + ", ".join(f"{arm} {ms[arm][-1]:.3f} ms" for arm in ARMS) + " per batch", flush=True)
    for arm in ARMS:
        a = np.array(ms[arm])
        print(f"{which} {arm} Adam: mean {a.mean():.3f} ms, median {np.median(a):.3f}, min {a.min():.3f}, max {a.max():.3f}, spread (max - min) {a.max() - a.min():.3f} "
              f"over {ROUNDS} rounds of {K} batches", flush=True)
    applied, steps, flushes = nets["lazy"].lazy_state()
    print(f"{which} lazy: after {steps} steps {flushes} full flushes; rows with steps outstanding {int((applied < steps).sum() - (applied == 0).sum())}, "
          f"rows never named {int((applied == 0).sum())} of {n}", flush=True)
    for arm in ARMS:
        e = edge_ms(nets[arm], vsrc, vdst)
        print(f"{which} {arm}: edge_bce over {len(vsrc)} edges {', '.join(f'{x:.3f}' for x in e)} ms (first call, then repeats)", flush=True)
    lazy = nets["lazy"]
    print(f"{which} lazy: full flush now ({steps} steps since the start) {flush_ms(lazy):.3f} ms, a second one right after it {flush_ms(lazy):.3f} ms", flush=True)
    first = 4 + ROUNDS * K
    for k in FLUSH_AFTER:
        b = run(lazy, order, NODES[which], k, first); first += k
        print(f"{which} lazy: {k} steps at {b:.3f} ms per batch, then one full flush {flush_ms(lazy):.3f} ms", flush=True)
    # an epoch's worth of batches, the flush that ends it included, against the dense arm's
    t0 = time.perf_counter(); run(lazy, order, NODES[which], EPOCH, first); flush_ms(lazy); lz = (time.perf_counter() - t0) / EPOCH * 1e3
    t0 = time.perf_counter(); run(nets["dense"], order, NODES[which], EPOCH, first); dn = (time.perf_counter() - t0) / EPOCH * 1e3
    print(f"{which} epoch of {EPOCH} batches: lazy with its closing flush {lz:.3f} ms per batch, dense {dn:.3f} ms per batch", flush=True)
    for net in nets.values(): net.close()
