"""node2vec's walk bias (ntf_n2v_set_walk_bias) at the bench dataset's size: dblp mt10.ts2 shapes from make_dataset, d = 128, B = 1000, w 5, wn 10, ns 5, walks of
5 nodes - the settings of profiles/n2v_sparse_time.py.

  python profiles/n2v_bias_time.py unbiased           p = q = 1, dense Adam: ROUNDS rounds of K batches.  Run it alternately with NTF_LIB_PATH naming a library built
                                                      from the parent commit (which lacks the entry: it is then not bound) and without, and compare the two
  python profiles/n2v_bias_time.py biased             (4, 1), (1, 4), (0.25, 4), (8, 8): batch time with dense and with sparse Adam, beside (1, 1) of the same process
  python profiles/n2v_bias_time.py kernels P Q        a short sparse run at (P, Q) for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...)
Results: profiles/n2v_bias_bench.md."""
import ctypes
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf
from opentf_amd.mdl.emb.gnn import stm_graph
from opentf_amd.synth import make_dataset

B, CTX, WN, NS, LR, D, NODES = 1000, 5, 10, 5, 1e-3, 128, 5
SETTINGS = [(4.0, 1.0), (1.0, 4.0), (0.25, 4.0), (8.0, 8.0)]
ROUNDS, K = 4, 30

mode = sys.argv[1] if len(sys.argv) > 1 else "biased"
HAS_BIAS = hasattr(ctypes.CDLL(libntf._LIB_PATH), "ntf_n2v_set_walk_bias")
if not HAS_BIAS: libntf.SYMBOLS.pop("ntf_n2v_set_walk_bias")          # a parent build: everything else of the ABI is the same

t0 = time.perf_counter()
CACHE = os.environ.get("N2V_BIAS_GRAPH_CACHE")          # an .npz path: the graph is built once and read by the later processes of a session
if CACHE and os.path.exists(CACHE):
    z = np.load(CACHE); rowptr, col = z["rowptr"], z["col"]; n = len(rowptr) - 1
else:
    ds = make_dataset("dblp", d=D, seed=0)
    N, S, M = ds["N"], ds["S"], ds["M"]
    skill = sp.csr_matrix((np.ones(len(ds["skill"][1]), np.uint8), ds["skill"][1], ds["skill"][0]), shape=(N, S))
    member = sp.csr_matrix((np.ones(len(ds["member"][1]), np.uint8), ds["member"][1], ds["member"][0]), shape=(N, M))
    perm = np.random.default_rng(2).permutation(N)
    n_test = int(0.15 * N)
    drop = np.concatenate([perm[:n_test], perm[n_test:][::3]])
    rowptr, col, off, n = stm_graph(skill, member, drop)
    if CACHE: np.savez(CACHE, rowptr=rowptr, col=col)
w = np.random.default_rng(0).standard_normal((n, D)).astype(np.float32)
order = np.random.default_rng(1).permutation(n)
deg = np.diff(rowptr)
print(f"n2v: table [{n}, {D}], {len(col)} CSR entries, largest degree {int(deg.max())}, {int((deg >= 2).sum())} nodes of degree >= 2, graph in {time.perf_counter() - t0:.1f} s; "
      f"library {'with' if HAS_BIAS else 'WITHOUT'} ntf_n2v_set_walk_bias ({libntf._LIB_PATH})", flush=True)


def make(sparse, p=1.0, q=1.0):
    net = libntf.Node2Vec(rowptr, col, w, seed=0, sparse=sparse)
    if (p, q) != (1.0, 1.0): net.set_walk_bias(p, q)
    return net


def run(net, k, first):
    """k batches, the loss of the last one read back (one synchronisation): ms per batch"""
    t0 = time.perf_counter()
    for i in range(k):
        o = ((first + i) * B) % (len(order) - B)
        net.train_batch(order[o:o + B], NODES, CTX, WN, NS, LR, want_loss=(i == k - 1))
    return (time.perf_counter() - t0) / k * 1e3


def rounds(net, tag):
    run(net, 2, 0)
    ms = np.array([run(net, K, 2 + r * K) for r in range(ROUNDS)])
    print(f"{tag}: rounds {' '.join(f'{x:.3f}' for x in ms)} ms per batch; mean {ms.mean():.3f}, median {np.median(ms):.3f}, spread (max - min) {ms.max() - ms.min():.3f}", flush=True)
    return ms


if mode == "unbiased":
    net = make(False)
    rounds(net, f"unbiased dense, library {'new' if HAS_BIAS else 'parent'}")
    net.close()
elif mode == "kernels":
    p, q = float(sys.argv[2]), float(sys.argv[3])
    net = make(True, p, q)
    print(f"sparse at (p, q) = ({p}, {q}): {run(net, 20, 0):.3f} ms per batch over 20 batches", flush=True)
    net.close()
else:
    for sparse in (False, True):
        for p, q in [(1.0, 1.0)] + SETTINGS:
            net = make(sparse, p, q)
            rounds(net, f"{'sparse' if sparse else 'dense'} Adam (p, q) = ({p}, {q})")
            net.close()
