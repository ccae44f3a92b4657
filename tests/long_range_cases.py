"""The inputs of tests/test_gpu_long_ranges.py, shared with tests/test_select_route_host.py (which shows on the host which path each of them takes): tables and
queries at the sizes where select_topk_row takes its sampled route and k_sims its block-stride loop, and their f64 references, computed once.  No GPU."""
import functools

import numpy as np

import select_route as SR
from test_knn_host import make_queries, make_table, reference_sims
from test_link_host import E as link_E, make_pooled, make_query_rows, make_table as make_link_table, reference_logits

# ------------------------------------------------------------------------------------------------------------------ search: one long range (cases 1 and 2)
LONG_N, LONG_D, LONG_Q = 70001, 96, 65
LONG_TOPN = (1, 10, 256, 257)      # 256: the last K of the sampled route; 257: the first that leaves it
LONG_SEED = {"clustered": 1, "normal": 2}
MERGE_WSB = 4 << 20                # groups of 32 queries, ranges of 32 768 rows
HOST_TOPN = {"clustered": (1, 10, 100, 256), "normal": (1, 10, 256)}


def long_n(n_cu):
    """the rows of cases 1 and 2: 70 001, or as many as make a workgroup of the one-range launch (4 query tiles, per_cu = 1 at dp = 96) take a second row block"""
    return max(LONG_N, SR.rows_that_stride(n_cu, 4, SR.padded(LONG_D)))


def _frozen(*arrays):
    for a in arrays: a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def long_case(kind, N=LONG_N):
    """-> T [N, 96], queries [65, 96], s* [65, N], exclude [65]: none / the best row / the worst row in turn, and for query 63 the best of the sample columns"""
    T = make_table(kind, N, LONG_D, seed=LONG_SEED[kind])
    Qv = make_queries(T, LONG_Q, seed=LONG_SEED[kind])
    ref = reference_sims(T, Qv)
    best, worst = ref.argmax(axis=1), ref.argmin(axis=1)
    ex = np.asarray([(-1, best[q], worst[q])[q % 3] for q in range(LONG_Q)], dtype=np.int64)
    cols = SR.sample_columns(N)
    ex[63] = cols[ref[63, cols].argmax()]
    return _frozen(T, Qv, ref, ex)


def merge_planted(N=LONG_N):
    R = SR.SimsPlan(MERGE_WSB, LONG_Q, N, SR.padded(LONG_D)).R
    return [0, R - 1, R, N - 1]          # id 0, the last id of a range, the first id of the next, N - 1


@functools.lru_cache(maxsize=None)
def merge_case(N=LONG_N):
    """the clustered table with the four best rows of every query planted across the ranges of MERGE_WSB -> T, queries [65, 96], s*"""
    rng = np.random.default_rng(6)
    T = long_case("clustered", N)[0].copy()
    u = rng.standard_normal(LONG_D)
    for j, p in enumerate(merge_planted(N)): T[p] = ((1.0 + j) * (u + 0.02 * rng.standard_normal(LONG_D))).astype(np.float32)
    Qv = (u[None, :] + 0.3 * rng.standard_normal((LONG_Q, LONG_D))).astype(np.float32)
    return _frozen(T, Qv, reference_sims(T, Qv))


# ------------------------------------------------------------------------------------------------------------------ search: the fallbacks of the sampled route (case 3)
FALL_M = 40000                     # sample stride 9


def _circle(theta, scale):
    return (np.stack([np.cos(theta), np.sin(theta), np.zeros_like(theta)], axis=1) * scale[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def aliasing_case():
    """rows (cos t, sin t, 0) times a positive scale: t ~ U(2, 3) on the 4096 sample columns, U(0.1, 1) elsewhere.  Against +e0 the sample sees only the negative sims,
    its threshold lies below 9 values in 10 and the collection overflows ("many"); against -e0 only sample columns lie above the threshold: r of them ("few" for K > r)
    -> T [40000, 3], queries (+e0, -e0), s*"""
    rng = np.random.default_rng(11)
    theta = rng.uniform(0.1, 1.0, FALL_M)
    cols = SR.sample_columns(FALL_M)
    theta[cols] = rng.uniform(2.0, 3.0, len(cols))
    T = _circle(theta, rng.uniform(0.5, 2.0, FALL_M))
    Qv = np.asarray([[1, 0, 0], [-1, 0, 0]], np.float32)
    return _frozen(T, Qv, reference_sims(T, Qv))


ALIAS_ROUTES = {(0, 1): "many", (0, 50): "many", (0, 256): "many", (1, 50): "few", (1, 256): "few"}       # (query, K)
TIE_POSITIVE, TIE_GROUP = 150, 5000
TIE_ROUTES = {100: "sampled", 200: "few", 256: "few"}                                                     # K


@functools.lru_cache(maxsize=None)
def tie_case(zero):
    """t ~ U(2.2, 3) (sims below -0.58 against e0), 150 random rows t ~ U(0.1, 1) (positive sims), 5000 other random rows all (cos 2, sin 2, 0) (sim -0.416, one bit
    pattern) or, zero = True, all zero rows (sim +0.0f).  The threshold falls into the group, exactly 150 values lie above it, and the K-th place of K > 150 lies
    inside the group -> T [40000, 3], queries (e0, e0), s*, the ids of the positive rows, the ids of the group (ascending)"""
    rng = np.random.default_rng(12)
    theta = rng.uniform(2.2, 3.0, FALL_M)
    perm = rng.permutation(FALL_M)
    pos, tie = np.sort(perm[:TIE_POSITIVE]), np.sort(perm[TIE_POSITIVE:TIE_POSITIVE + TIE_GROUP])
    theta[pos] = rng.uniform(0.1, 1.0, TIE_POSITIVE)
    T = _circle(theta, rng.uniform(0.5, 2.0, FALL_M))
    T[tie] = 0 if zero else _circle(np.asarray([2.0]), np.asarray([1.0]))[0]
    Qv = np.asarray([[1, 0, 0], [1, 0, 0]], np.float32)
    return _frozen(T, Qv, reference_sims(T, Qv), pos, tie)


# ------------------------------------------------------------------------------------------------------------------ search: a range at its cap (case 4)
CAP_N, CAP_D, CAP_Q, CAP_TOPN = SR.SIM_MAX_RANGE + 300, 8, 3, 10
CAP_PLANTED = [SR.SIM_MAX_RANGE - 1, SR.SIM_MAX_RANGE]        # the last id of the first range, the first id of the second


@functools.lru_cache(maxsize=None)
def cap_case():
    rng = np.random.default_rng(113)
    T = make_table("clustered", CAP_N, CAP_D, seed=13).copy()
    u = rng.standard_normal(CAP_D)
    for j, p in enumerate(CAP_PLANTED): T[p] = ((1.0 + j) * (u + 0.002 * rng.standard_normal(CAP_D))).astype(np.float32)
    Qv = (u[None, :] + 0.05 * rng.standard_normal((CAP_Q, CAP_D))).astype(np.float32)
    return _frozen(T, Qv, reference_sims(T, Qv))


# ------------------------------------------------------------------------------------------------------------------ link decode: long candidate blocks (case 5)
# (d, n query rows, cand_lo, C, query tiles a workgroup): 4 tiles at dp = 96, 2 at dp = 192, 1 at dp = 256 where two workgroups share a CU
LINK_SHAPES = [(80, 65, 301, 70001, 4), (161, 33, 301, 70001, 2), (256, 5, 0, 131073, 1)]
LINK_K = (10, 256, 257)


def link_c(si, n_cu):
    d, n, lo, Cn, nqt = LINK_SHAPES[si]
    return max(Cn, SR.rows_that_stride(n_cu, nqt, SR.padded(d)))


@functools.lru_cache(maxsize=None)
def link_case(si, Cn=None):
    """-> T [lo + C + 1, d] (its last row: minus the mean of the candidates), query rows [n] (the last one: that row), x* [n, C], E [n, C]"""
    d, n, lo, C0, _ = LINK_SHAPES[si]
    Cn = Cn or C0
    n_rows = lo + Cn + 1
    T = make_link_table(n_rows, d, seed=21 + si)
    cand = T[lo:lo + Cn]
    T[n_rows - 1] = -cand.astype(np.float64).mean(axis=0)
    rows = make_query_rows(n_rows - 1, n, seed=21 + si)
    rows[n - 1] = n_rows - 1
    return _frozen(T, rows, reference_logits(cand, T[rows]), link_E(cand, T[rows]))


def link_pooled(si, Cn=None):
    d, n, lo, C0, _ = LINK_SHAPES[si]
    return make_pooled(0, lo + (Cn or C0), n, seed=21 + si)
