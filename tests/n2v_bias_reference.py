"""node2vec's biased (p, q) second-order walk as the device draws it (k_n2v_walks_biased of opentf_amd/csrc/ntf_n2v.hip, ntf_n2v_set_walk_bias), restated for the tests.

torch_cluster's `random_walk(rowptr, col, start, walk_length, p, q)` is what torch_geometric.nn.Node2Vec.pos_sample calls; the package is not installed, so its
published algorithm is restated here and THIS file is the pin (as tests/m2v_reference.py is for MetaPath2Vec).  A walk stands on v and came from t (t == v at the
start and after a stay):
  * deg(v) == 0: it stays; deg(v) == 1: it takes the only neighbour; position 1: a uniform neighbour of v;
  * later, with deg(v) >= 2: x is drawn over the ENTRIES of v's CSR row (a repeated id counts once per entry) with probability proportional to alpha(t, x):
    1 / p when x == t (class 0), 1 when t occurs in the CSR row of x (class 1: torch_cluster's is_neighbor(x, t) looks in the row of x), 1 / q otherwise (class 2).
torch_cluster rejects against max(1 / p, 1, 1 / q) without a bound on the attempts; the device rejects `tries` times and then takes the step by an exact
inverse-CDF scan of v's row over the same integer weights, so the mixture is the same distribution.

The draws (include/opentf_amd.h): thr[k] = floor(prob_k * 2^32) in IEEE double; walk r of call `step` consumes the 32-bit words w_0, w_1, ... where w_i is word
i & 3 of Philox4x32-10(counter (r lo, r hi, BIAS_BASE + (i >> 2), step), key n2v_key(seed, step, 0)) - only steps that draw consume words.  Position 1: one word u,
x = col[a + ((u * deg) >> 32)].  Position >= 2: per attempt two words u_c, u_a; candidate c = col[a + ((u_c * deg) >> 32)], accepted iff u_a < thr[class(c, t)].
After `tries` rejections two more words u_hi, u_lo (in that order) form U = (u_hi << 32) | u_lo; total = sum of thr[class] over the row, target = (U * total) >> 64,
x = the first entry whose inclusive prefix sum exceeds target.

TEST INFRASTRUCTURE ONLY: numpy and the oracle's Philox; imports nothing from opentf_amd.
"""
import bisect
import functools
import math

import numpy as np

from oracle.d2v_oracle import philox4x32

M64 = (1 << 64) - 1
BIAS_BASE = 0x42494153
TRIES = 16


def n2v_key(seed, step, tensor):
    """n2v_key of ntf_n2v.hip: 64-bit mix of (seed, step, tensor), everything modulo 2^64 -> the two Philox key words"""
    x = (seed ^ ((step * 0x9E3779B97F4A7C15 + tensor * 0xBF58476D1CE4E5B9) & M64)) & M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64; x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64; x ^= x >> 31
    return x & 0xFFFFFFFF, x >> 32


def thresholds(p, q):
    """[thr_0, thr_1, thr_2]: the acceptance thresholds of the classes return / common neighbour / explore, in [1, 2^32] for p, q in [1e-4, 1e4]"""
    ip, iq = 1.0 / float(p), 1.0 / float(q)
    mx = max(ip, 1.0, iq)
    return [int(math.floor(x / mx * 4294967296.0)) for x in (ip, 1.0, iq)]


class _Words:
    """the word stream of one walk"""
    def __init__(self, r, step, key):
        self.r, self.step, self.key, self.i, self.block = r, step & 0xFFFFFFFF, key, 0, None

    def __call__(self):
        if self.i & 3 == 0:
            self.block = philox4x32((self.r & 0xFFFFFFFF, self.r >> 32, (BIAS_BASE + (self.i >> 2)) & 0xFFFFFFFF, self.step), self.key)
        w = self.block[self.i & 3]; self.i += 1
        return w


def _rows(rowptr, col):
    rp = [int(x) for x in rowptr]; cl = [int(x) for x in col]
    return rp, cl, [cl[rp[i]:rp[i + 1]] for i in range(len(rp) - 1)]


def _in_row(row, t):
    """t occurs in an ascending row (the device's binary search)"""
    k = bisect.bisect_left(row, t)
    return k < len(row) and row[k] == t


def _cls(rows, x, t):
    return 0 if x == t else 1 if _in_row(rows[x], t) else 2


def replay_biased_walks(rowptr, col, batch, n_walks, walk_length, seed, step, p, q, tries=TRIES, stats=None):
    """the walks [n_walks, walk_length] of call `step` of a handle of this seed under the bias (p, q); row r starts at batch[r % B].  stats (a dict, optional) takes
    'biased_steps' (steps that entered the rejection stage), 'scans' (steps taken by the scan) and 'scan_nodes' (the node each scan stood on)"""
    thr = thresholds(p, q)
    key = n2v_key(seed, step, 0)
    rp, cl, rows = _rows(rowptr, col)
    if stats is not None: stats.update(biased_steps=0, scans=0, scan_nodes=[])
    rw = np.empty((n_walks, walk_length), dtype=np.int64)
    for r in range(n_walks):
        word = _Words(r, step, key)
        cur = prev = int(batch[r % len(batch)]); rw[r, 0] = cur
        for s in range(1, walk_length):
            row = rows[cur]; deg = len(row); nxt = cur
            if deg == 1: nxt = row[0]
            elif deg >= 2 and s == 1: nxt = row[(word() * deg) >> 32]
            elif deg >= 2:
                if stats is not None: stats["biased_steps"] += 1
                nxt = None
                for _ in range(tries):
                    u_c = word(); u_a = word()
                    c = row[(u_c * deg) >> 32]
                    if u_a < thr[_cls(rows, c, prev)]: nxt = c; break
                if nxt is None:
                    u_hi = word(); u_lo = word()
                    U = (u_hi << 32) | u_lo
                    wts = [thr[_cls(rows, x, prev)] for x in row]
                    target = (U * sum(wts)) >> 64
                    acc = 0
                    for x, w in zip(row, wts):
                        acc += w
                        if acc > target: nxt = x; break
                    if stats is not None: stats["scans"] += 1; stats["scan_nodes"].append(cur)
            prev, cur = cur, nxt
            rw[r, s] = cur
    return rw


def exact_pairs(rowptr, col, start, p, q):
    """float64 joint distribution P[x1, x2] of positions 1 and 2 of a walk of 3 nodes from `start`, straight from the definition (1 / p, 1, 1 / q; not the
    thresholds: they differ from these by at most 2^-32 relative to the largest class)"""
    rp, cl, rows = _rows(rowptr, col)
    n = len(rp) - 1
    P = np.zeros((n, n))
    r0 = rows[start]
    if not r0: P[start, start] = 1.0; return P
    for x1 in r0:
        p1 = 1.0 / len(r0)
        r1 = rows[x1]
        if not r1: P[x1, x1] += p1; continue
        if len(r1) == 1: P[x1, r1[0]] += p1; continue
        w = np.array([(1.0 / p, 1.0, 1.0 / q)[_cls(rows, x2, start)] for x2 in r1])
        w /= w.sum()
        for x2, pw in zip(r1, w): P[x1, x2] += p1 * pw
    return P


def chi_square(walks, P, min_expected=5.0):
    """Pearson's statistic of the (position 1, position 2) counts of `walks` [n, 3] against P; cells of expected count below min_expected are left out.
    -> statistic, cells used, the probability mass left out (observations in cells of probability 0 make the statistic infinite)"""
    n = len(walks)
    obs = np.zeros_like(P); np.add.at(obs, (walks[:, 1], walks[:, 2]), 1.0)
    exp = P * n
    use = (exp >= min_expected) & (P > 0)
    if obs[P == 0].any(): return float("inf"), int(use.sum()), float(P[~use].sum())
    return float((((obs - exp) ** 2)[use] / exp[use]).sum()), int(use.sum()), float(P[~use].sum())


def _csr_of(A):
    a, b = np.nonzero(A)
    rowptr = np.zeros(len(A) + 1, dtype=np.int64); np.add.at(rowptr, a + 1, 1)
    return np.cumsum(rowptr), b.astype(np.int32)


G24_DEGREES = [14, 5, 4, 5, 5, 3, 7, 4, 5, 4, 3, 3, 3, 3, 0, 5, 5, 0, 3, 4, 3, 5, 1, 4]


@functools.lru_cache(None)
def g24():
    """24 nodes: random undirected edges until the adjacency matrix holds 80 ones, then node 0 joined to 1 .. 12.  Two isolated nodes (14, 17), one leaf (22), one
    hub (0).  -> rowptr int64, col int32 (rows ascending)"""
    g = np.random.default_rng(5)
    A = np.zeros((24, 24), dtype=np.int64)
    while A.sum() < 80:
        i, j = g.integers(0, 24, 2)
        if i != j: A[i, j] = A[j, i] = 1
    A[0, 1:13] = 1; A[1:13, 0] = 1
    rowptr, col = _csr_of(A)
    assert np.diff(rowptr).tolist() == G24_DEGREES
    return rowptr, col


@functools.lru_cache(None)
def h301():
    """node 0 joined to 1 .. 300 and the edges (i, i + 1) for i = 1, 4, 7, .., 298: the hub row takes 5 strides of 64 with a ragged tail, and two of every three
    hub neighbours are adjacent to another one"""
    A = np.zeros((301, 301), dtype=np.int64)
    A[0, 1:] = 1; A[1:, 0] = 1
    for i in range(1, 299, 3): A[i, i + 1] = A[i + 1, i] = 1
    return _csr_of(A)


@functools.lru_cache(None)
def d4():
    """4 nodes, edges 0-1 (DOUBLED: two entries in either row), 0-2, 0-3, 1-2.  -> rowptr, col with rows ascending, repeats kept"""
    edges = [(0, 1), (0, 1), (0, 2), (0, 3), (1, 2)]
    a = np.array([e[0] for e in edges] + [e[1] for e in edges]); b = np.array([e[1] for e in edges] + [e[0] for e in edges])
    order = np.lexsort((b, a)); a, b = a[order], b[order]
    rowptr = np.zeros(5, dtype=np.int64); np.add.at(rowptr, a + 1, 1)
    return np.cumsum(rowptr), b.astype(np.int32)


SETTINGS = [(4, 1), (1, 4), (0.25, 4), (2, 0.5), (8, 8), (0.01, 100)]
