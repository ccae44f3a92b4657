"""`ntf_auc_micro_dense` / `ntf_auc_micro_csr` (ntf_auc.hip) and their Python mirror against an integer Mann-Whitney oracle.

The library returns three integers - P positives, N negatives, U2 = sum over positives of (2 #negatives scored lower + #negatives scored
equal) - and the double U2 / (2 P N).  Integers do not depend on the order of summation, so every case asserts EQUALITY with the oracle,
and the double bit for bit against `float(U2) / (2.0 * float(P) * float(N))`.

The oracle (`oracle_counts`) is not the device's algorithm: the device counts every score into a bucket between the positives' sorted
distinct keys; the oracle stable-sorts the keys of ALL n * M scores and walks the tie groups, in Python ints.  `tests/test_auc_host.py`
checks the oracle itself against sklearn where no GPU is needed.  Where sklearn is named the bar is 1e-12 (tests/test_gpu_eval.py); the
two differ only by sklearn's trapezoid sum in f64 (observed: 1e-16).

Not reachable by a test of a few seconds, reviewed by reading: a 32-bit bucket counter overflows only beyond 4.3e9 scores, and
2 P N >= 2^64 needs n * M beyond 2^32 (see `test_past_32_bits`).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EINVAL = -1            # NTF_EINVAL, include/opentf_amd.h
SENTINEL = 7


# ------------------------------------------------------------------------------------------------------------------ the oracle
def keys_of(x):
    """u32 keys ordered as the f32 values are as real numbers: +-0.0 one key, denormals distinct (numpy compares them unflushed)"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    u = x.view(np.uint32).copy()
    u[x == 0] = 0                                  # -0.0 == 0 is true, a denormal == 0 is not
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def tie_groups(S, lab):
    """(positives, negatives) per group of equal scores, groups by ascending score"""
    k, l = keys_of(S), np.asarray(lab, dtype=bool).ravel()
    assert not np.isnan(np.asarray(S, dtype=np.float32)).any()
    o = np.argsort(k, kind="stable")
    ks, ls = k[o], l[o]
    _, start, cnt = np.unique(ks, return_index=True, return_counts=True)
    pos_g = np.add.reduceat(ls.astype(np.int64), start)
    return pos_g, cnt.astype(np.int64) - pos_g


def counts_from_groups(pos_g, neg_g):
    below = np.concatenate([[0], np.cumsum(neg_g)[:-1]])
    has = pos_g > 0
    u2 = sum(int(p) * (2 * int(b) + int(q)) for p, b, q in zip(pos_g[has], below[has], neg_g[has]))       # Python ints: no width to overflow
    return int(pos_g.sum()), int(neg_g.sum()), u2


def oracle_counts(S, lab):
    """-> (P, N, U2) as Python ints"""
    return counts_from_groups(*tie_groups(S, lab))


def auc_of(counts):
    P, N, U2 = counts
    return float(U2) / (2.0 * float(P) * float(N))


def sklearn_auc(S, lab):
    from sklearn.metrics import roc_auc_score
    return roc_auc_score(np.asarray(lab, dtype=bool).ravel(), np.asarray(S, dtype=np.float64).ravel())


def mixed_groups(S, lab):
    pos_g, neg_g = tie_groups(S, lab)
    return int(((pos_g > 0) & (neg_g > 0)).sum())


# ------------------------------------------------------------------------------------------------------------------ inputs
N_RAG, M_RAG = 37, 1003
FAMILIES = ("uniform", "five_level", "zero_heavy", "logits")


def labels(n, M, density, seed):
    return np.random.default_rng(seed).random((n, M)) < density


def family(name, n, M, seed):
    rng = np.random.default_rng(seed)
    if name == "uniform":
        return rng.random((n, M), dtype=np.float32)
    if name == "five_level":
        return (rng.integers(0, 5, (n, M)) / 4).astype(np.float32)
    if name == "zero_heavy":
        S = np.where(rng.random((n, M)) < 0.9, 0, rng.random((n, M))).astype(np.float32)
        S[rng.random((n, M)) < 0.05] = -0.0
        return S
    if name == "logits":
        return (50 * rng.standard_normal((n, M))).astype(np.float32)
    raise KeyError(name)


def check_family(name, S, lab):
    """the property that makes the family meaningful"""
    if name == "five_level":
        assert set(np.unique(S)) == {0.0, 0.25, 0.5, 0.75, 1.0} and mixed_groups(S, lab) >= 1
    elif name == "zero_heavy":
        assert (S == 0).mean() > 0.85
        for cls in (lab, ~lab):
            z = S[cls][S[cls] == 0]
            assert np.signbit(z).any() and (~np.signbit(z)).any()
    elif name == "logits":
        assert (S < 0).any() and (S > 0).any()
    else:
        assert len(np.unique(S)) > S.size // 2


def truth_csr(lab):
    Y = sp.csr_matrix(np.asarray(lab, dtype=np.int8)); Y.sort_indices()
    return np.ascontiguousarray(Y.indptr, dtype=np.int64), np.ascontiguousarray(Y.indices, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _out():
    return np.full(3, SENTINEL, dtype=np.uint64), C.c_double(-7.0)


def _result(rc, counts, auc):
    return rc, tuple(int(c) for c in counts), auc.value


def auc_dense(S, t_ip, t_ix, rows=None, ld=None, chunk=0, n=None, M=None, n_truth_rows=None, null=()):
    """-> (status, (P, N, U2), auc) of ntf_auc_micro_dense; S [n, M] f32 or, with ld, the padded [n, ld] array"""
    from opentf_amd import libntf
    S = np.ascontiguousarray(S, dtype=np.float32)
    n = S.shape[0] if n is None else n
    ld = S.shape[1] if ld is None else ld
    M = S.shape[1] if M is None else M
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    counts, auc = _out()
    args = dict(scores=_p(S), ip=_p(t_ip), ix=_p(t_ix), counts=_p(counts), auc=C.byref(auc))
    for k in null:
        args[k] = None
    rc = libntf.lib().ntf_auc_micro_dense(0, args["scores"], n, M, ld, args["ip"], args["ix"], len(t_ip) - 1 if n_truth_rows is None else n_truth_rows,
                                          _p(r), int(chunk), args["counts"], args["auc"])
    return _result(rc, counts, auc)


def auc_csr(s_ip, s_ix, s_val, n, M, t_ip, t_ix, rows=None, chunk=0, null=()):
    """-> (status, (P, N, U2), auc) of ntf_auc_micro_csr"""
    from opentf_amd import libntf
    s_ip = np.ascontiguousarray(s_ip, dtype=np.int64); s_ix = np.ascontiguousarray(s_ix, dtype=np.int32); s_val = np.ascontiguousarray(s_val, dtype=np.float32)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    counts, auc = _out()
    args = dict(s_ip=_p(s_ip), ip=_p(t_ip), counts=_p(counts), auc=C.byref(auc))
    for k in null:
        args[k] = None
    rc = libntf.lib().ntf_auc_micro_csr(0, args["s_ip"], _p(s_ix), _p(s_val), n, M, args["ip"], _p(t_ix), len(t_ip) - 1, _p(r), int(chunk), args["counts"], args["auc"])
    return _result(rc, counts, auc)


def assert_exact(got, want):
    rc, counts, auc = got
    assert rc == 0, rc
    assert counts == want, (counts, want)
    assert auc == auc_of(counts)              # bit for bit: one f64 division of exactly representable products' roundings


def assert_refused(got):
    rc, counts, auc = got
    assert rc == EINVAL, rc
    assert counts == (SENTINEL,) * 3 and auc == -7.0, "a refused call wrote its outputs"


# ------------------------------------------------------------------------------------------------------------------ 1. ragged dense
@pytest.mark.parametrize("padded", [False, True], ids=["ld=M", "ld=M+5"])
@pytest.mark.parametrize("name", FAMILIES)
def test_ragged_dense(name, padded):
    lab = labels(N_RAG, M_RAG, 0.02, 11)
    S = family(name, N_RAG, M_RAG, 12)
    check_family(name, S, lab)
    assert M_RAG % 4 and (N_RAG * M_RAG) % 4          # rows and the whole matrix end inside a 16-byte vector
    want = oracle_counts(S, lab)
    ip, ix = truth_csr(lab)
    if padded:
        buf = np.full((N_RAG, M_RAG + 5), np.nan, dtype=np.float32)     # the padding must not be read: a NaN read is refused
        buf[:, :M_RAG] = S
        got = auc_dense(buf, ip, ix, ld=M_RAG + 5, M=M_RAG)
    else:
        got = auc_dense(S, ip, ix)
    assert_exact(got, want)
    assert abs(got[2] - sklearn_auc(S, lab)) <= 1e-12
    print(f"{name}: (P, N, U2) = {got[1]}, auc {got[2]!r}")


# ------------------------------------------------------------------------------------------------------------------ 2. special values
def test_special_values():
    n, M = 4, 64
    f = np.float32
    den = [f(1e-45), f(1e-42), f(1e-39), f(-1e-45)]
    spec = [f(np.inf), f(-np.inf), np.finfo(f).max, -np.finfo(f).max, np.finfo(f).tiny, -np.finfo(f).tiny] + den
    assert all(d != 0 and abs(d) < np.finfo(f).tiny for d in den)
    S = np.zeros((n, M), dtype=f)
    lab = np.zeros((n, M), dtype=bool)
    S[0, :len(spec)] = spec; lab[0, :len(spec)] = True          # every special value as a positive score, zeros as negatives
    S[1, :len(spec)] = spec                                     # ... and once as a negative score: a tie group of both classes each
    S[2, 5] = -0.0; lab[2, 5] = True; lab[2, 6] = True          # a positive at -0.0 and one at +0.0
    S[3, ::7] = -0.0
    want = oracle_counts(S, lab)
    flushed = S.copy(); flushed[np.abs(flushed) < np.finfo(f).tiny] = 0
    assert auc_of(oracle_counts(flushed, lab)) != auc_of(want), "the case would not notice flushed denormals"
    ip, ix = truth_csr(lab)
    assert_exact(auc_dense(S, ip, ix), want)


def test_all_equal_and_smallest():
    lab = labels(4, 64, 0.1, 5)
    ip, ix = truth_csr(lab)
    for value in (0.3, 0.0, -0.0, np.inf):
        got = auc_dense(np.full((4, 64), value, dtype=np.float32), ip, ix)
        assert got[0] == 0 and got[1][2] == got[1][0] * got[1][1] and got[2] == 0.5
    one = np.array([[0, 1]], dtype=bool)
    ip, ix = truth_csr(one)
    assert_exact(auc_dense(np.array([[0.2, 0.7]], dtype=np.float32), ip, ix), (1, 1, 2))
    assert_exact(auc_dense(np.array([[0.7, 0.2]], dtype=np.float32), ip, ix), (1, 1, 0))
    assert_exact(auc_dense(np.array([[-0.0, 0.0]], dtype=np.float32), ip, ix), (1, 1, 1))


# ------------------------------------------------------------------------------------------------------------------ 3. chunks
@pytest.mark.parametrize("name", ["uniform", "zero_heavy"])
def test_chunks(name):
    lab = labels(N_RAG, M_RAG, 0.02, 21)
    S = family(name, N_RAG, M_RAG, 22)
    ip, ix = truth_csr(lab)
    whole = auc_dense(S, ip, ix)
    assert_exact(whole, oracle_counts(S, lab))
    rows_per = 8
    assert -(-N_RAG // rows_per) >= 5 and N_RAG % rows_per != 0          # at least 5 chunks, the last one shorter
    for chunk in (rows_per * M_RAG * 4, rows_per * M_RAG * 4 + 4 * M_RAG - 1, M_RAG * 4, M_RAG * 4 + 3):   # (a budget is rounded DOWN to whole rows)
        got = auc_dense(S, ip, ix, chunk=chunk)
        assert got == whole, (chunk, got, whole)
    buf = np.full((N_RAG, M_RAG + 5), np.nan, dtype=np.float32); buf[:, :M_RAG] = S
    assert auc_dense(buf, ip, ix, ld=M_RAG + 5, M=M_RAG, chunk=3 * M_RAG * 4) == whole


# ------------------------------------------------------------------------------------------------------------------ 4. rows
def test_rows_indirection():
    n, M = N_RAG, M_RAG
    truth = labels(3 * n, M, 0.02, 31)
    rng = np.random.default_rng(32)
    rows = rng.permutation(3 * n)[:n]
    rows[7] = rows[20]                                                   # a repeated truth row
    assert len(set(rows.tolist())) == n - 1 and not np.array_equal(rows, np.sort(rows)) and rows.max() >= n
    lab = truth[rows]
    S = family("zero_heavy", n, M, 33)
    ip, ix = truth_csr(truth)
    assert len(ip) - 1 == 3 * n
    want = oracle_counts(S, lab)
    assert want != oracle_counts(S, truth[:n])                           # ignoring `rows` would show
    assert_exact(auc_dense(S, ip, ix, rows=rows), want)
    D = sp.csr_matrix(S)
    assert_exact(auc_csr(D.indptr, D.indices, D.data, n, M, ip, ix, rows=rows), want)


# ------------------------------------------------------------------------------------------------------------------ 5. past 32 bits
@pytest.fixture(scope="module")
def big():
    n, M = 500, 20000
    rng = np.random.default_rng(7)
    Y = sp.random(n, M, density=5.0 / M, random_state=3, format="csr", dtype=np.float32)
    lab = np.zeros((n, M), dtype=bool); lab[Y.nonzero()] = True
    S = rng.random((n, M), dtype=np.float32) ** 8            # probabilities crowded near 0
    S[rng.random((n, M)) < 0.5] = 0.0                         # half exact zeros
    pos_g, neg_g = tie_groups(S, lab)
    return S, lab, counts_from_groups(pos_g, neg_g), int(((pos_g > 0) & (neg_g > 0)).sum())


def test_past_32_bits(big):
    """U2 and the prefix sums behind it exceed 2^32 here; a 32-bit one fails.  A 32-bit BUCKET COUNTER cannot be made to overflow in a test of
    a few seconds - it needs more than 4.3e9 scores - so the counters' declared width (64 bits in global memory; 32 bits per workgroup in
    LDS, a workgroup seeing a 2048th of a chunk) is reviewed by reading."""
    S, lab, want, mixed = big
    assert want[2] > 2 ** 32 and mixed >= 100
    assert 4.5 <= lab.sum() / len(lab) <= 5.5
    ip, ix = truth_csr(lab)
    got = auc_dense(S, ip, ix)
    assert_exact(got, want)
    assert abs(got[2] - sklearn_auc(S, lab)) <= 1e-12
    assert auc_dense(S, ip, ix, chunk=97 * 20000 * 4) == got             # 6 chunks, the last of 15 rows
    print(f"(P, N, U2) = {got[1]}, auc {got[2]!r}")


# ------------------------------------------------------------------------------------------------------------------ 6. CSR form
def topk_like(n, M, lab, seed, K=10):
    """CSR scores shaped like a top-K prediction file: K stored entries a row, about half of the truth entries among them, the values positive
    except for some stored 0.0 and some stored negatives; row 3 stores nothing"""
    rng = np.random.default_rng(seed)
    ip, ix, val = [0], [], []
    for i in range(n):
        if i == 3:
            ip.append(ip[-1]); continue
        t = np.nonzero(lab[i])[0]
        keep = t[rng.random(len(t)) < 0.5][:K]
        rest = rng.choice(np.setdiff1d(np.arange(M), t), K - len(keep), replace=False)
        cols = np.sort(np.concatenate([keep, rest]))
        v = rng.random(K).astype(np.float32)
        v[rng.random(K) < 0.15] = 0.0
        v[rng.random(K) < 0.15] *= -1
        ix.extend(cols.tolist()); val.extend(v.tolist()); ip.append(ip[-1] + K)
    return np.asarray(ip, np.int64), np.asarray(ix, np.int32), np.asarray(val, np.float32)


@pytest.mark.parametrize("n,M", [(N_RAG, M_RAG), (300, 5000)])
def test_csr_form(n, M):
    lab = labels(n, M, 0.02 if M < 2000 else 0.002, 41)
    s_ip, s_ix, s_val = topk_like(n, M, lab, 42)
    D = np.zeros((n, M), dtype=np.float32)
    r = np.repeat(np.arange(n), np.diff(s_ip))
    D[r, s_ix] = s_val
    stored = np.zeros((n, M), dtype=bool); stored[r, s_ix] = True
    assert (lab & stored).any() and (lab & ~stored).any()                  # truth entries stored and unstored
    assert (s_val == 0).any() and s_val.min() < 0 < s_val.max()            # explicit zeros; the implicit zeros sit in the middle of the order
    assert s_ip[3] == s_ip[4] and len(s_val) == 10 * (n - 1)
    want = oracle_counts(D, lab)
    ip, ix = truth_csr(lab)
    got = auc_csr(s_ip, s_ix, s_val, n, M, ip, ix)
    assert_exact(got, want)
    assert_exact(auc_dense(D, ip, ix), want)
    per = len(s_val) // 3 - 1
    assert -(-len(s_val) // per) >= 3 and len(s_val) % per != 0
    assert auc_csr(s_ip, s_ix, s_val, n, M, ip, ix, chunk=4 * per) == got
    if n == N_RAG:
        assert auc_csr(s_ip, s_ix, s_val, n, M, ip, ix, chunk=4) == got                              # one entry per upload
    assert abs(got[2] - sklearn_auc(D, lab)) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ the kernel's paths
@pytest.mark.parametrize("G", [2047, 2048, 2049, 4097, 5500])
def test_many_distinct_positive_scores(G):
    """The number G of distinct positive scores picks the kernel's path: up to 2047 the 2 G + 1 bucket counters live in LDS, beyond that they
    are global; up to 2048 the whole key table is in LDS, beyond that a sampled table (every 2nd key from 2049, every 4th from 4097) with the
    last levels of the search on the table in global memory.  All scores distinct, exactly G positives."""
    n, M = N_RAG, M_RAG
    rng = np.random.default_rng(G)
    S = (rng.permutation(n * M).astype(np.float32) / np.float32(n * M)).reshape(n, M)
    assert len(np.unique(S)) == n * M
    lab = np.zeros(n * M, dtype=bool); lab[rng.choice(n * M, G, replace=False)] = True
    lab = lab.reshape(n, M)
    want = oracle_counts(S, lab)
    assert want[0] == G
    ip, ix = truth_csr(lab)
    assert_exact(auc_dense(S, ip, ix), want)
    assert_exact(auc_dense(S, ip, ix, chunk=5 * M * 4), want)


def test_global_counters_under_contention():
    """more than 2047 distinct positive scores (global counters) on a matrix that is 90 % exact zeros"""
    n, M = N_RAG, M_RAG
    lab = labels(n, M, 0.8, 51)
    S = family("zero_heavy", n, M, 52)
    assert len(np.unique(S[lab])) > 2047 and (S == 0).mean() > 0.85
    ip, ix = truth_csr(lab)
    assert_exact(auc_dense(S, ip, ix), oracle_counts(S, lab))


# ------------------------------------------------------------------------------------------------------------------ 7. contract
def test_contract():
    n, M = 6, 40
    lab = labels(n, M, 0.1, 61)
    S = family("uniform", n, M, 62)
    ip, ix = truth_csr(lab)
    assert ip[1] - ip[0] >= 2 or ip[2] - ip[1] >= 2
    i2 = int(np.nonzero(np.diff(ip) >= 2)[0][0])          # a truth row with two entries
    assert_exact(auc_dense(S, ip, ix), oracle_counts(S, lab))
    D = sp.csr_matrix(S)
    assert D.nnz == n * M
    d_ip, d_ix, d_val = D.indptr.astype(np.int64), D.indices.astype(np.int32), D.data.astype(np.float32)
    assert_exact(auc_csr(d_ip, d_ix, d_val, n, M, ip, ix), oracle_counts(S, lab))

    def truth_with(at, value):
        bad = ix.copy(); bad[at] = value
        return bad

    def csr_with(at, value, what="ix"):
        a = (d_ix if what == "ix" else d_val).copy(); a[at] = value
        return (d_ip, a, d_val) if what == "ix" else (d_ip, d_ix, a)

    # NaN in a score: at a negative, at a positive, in CSR values
    neg_at, pos_at = np.argwhere(~lab)[0], np.argwhere(lab)[0]
    for at in (neg_at, pos_at):
        bad = S.copy(); bad[tuple(at)] = np.nan
        assert_refused(auc_dense(bad, ip, ix))
    assert_refused(auc_dense(-np.abs(np.full((n, M), np.nan, np.float32)), ip, ix))      # NaN with the sign bit set
    assert_refused(auc_csr(*csr_with(5, np.nan, "val"), n, M, ip, ix))
    # one class only
    empty = np.zeros(n + 1, dtype=np.int64)
    assert_refused(auc_dense(S, empty, np.zeros(1, np.int32)))
    assert_refused(auc_csr(d_ip, d_ix, d_val, n, M, empty, np.zeros(1, np.int32)))
    full_ip, full_ix = truth_csr(np.ones((n, M), dtype=bool))
    assert_refused(auc_dense(S, full_ip, full_ix))
    # truth columns: == M, negative, unsorted, duplicate
    a = int(ip[i2])
    assert_refused(auc_dense(S, ip, truth_with(int(ip[i2 + 1]) - 1, M)))
    assert_refused(auc_dense(S, ip, truth_with(a, -1)))
    swapped = ix.copy(); swapped[a], swapped[a + 1] = ix[a + 1], ix[a]
    assert_refused(auc_dense(S, ip, swapped))
    assert_refused(auc_dense(S, ip, truth_with(a + 1, ix[a])))
    assert_refused(auc_csr(d_ip, d_ix, d_val, n, M, ip, swapped))
    assert_refused(auc_csr(d_ip, d_ix, d_val, n, M, ip, truth_with(a + 1, ix[a])))
    # score columns: == M, negative, unsorted, duplicate
    assert_refused(auc_csr(*csr_with(M - 1, M), n, M, ip, ix))
    assert_refused(auc_csr(*csr_with(0, -1), n, M, ip, ix))
    sw = d_ix.copy(); sw[3], sw[4] = d_ix[4], d_ix[3]
    assert_refused(auc_csr(d_ip, sw, d_val, n, M, ip, ix))
    assert_refused(auc_csr(*csr_with(4, d_ix[3]), n, M, ip, ix))
    # rows out of range
    rows = np.arange(n)
    for bad_row in (n, -1):
        r = rows.copy(); r[2] = bad_row
        assert_refused(auc_dense(S, ip, ix, rows=r))
        assert_refused(auc_csr(d_ip, d_ix, d_val, n, M, ip, ix, rows=r))
    assert_refused(auc_dense(S, ip, ix, n_truth_rows=n - 1))                   # rows NULL and more instances than truth rows
    # sizes
    assert_refused(auc_dense(S, ip, ix, ld=M - 1))
    assert_refused(auc_dense(S, ip, ix, chunk=M * 4 - 1))
    assert_refused(auc_dense(S, ip, ix, chunk=-1))
    assert_refused(auc_csr(d_ip, d_ix, d_val, n, M, ip, ix, chunk=3))
    assert_refused(auc_dense(S, ip, ix, n=0))
    assert_refused(auc_dense(S, ip, ix, M=0, ld=M))
    assert_refused(auc_csr(d_ip, d_ix, d_val, 0, M, ip, ix))
    # null pointers
    for k in ("scores", "ip", "ix", "counts", "auc"):
        assert_refused(auc_dense(S, ip, ix, null=(k,)))
    for k in ("s_ip", "ip", "counts", "auc"):
        assert_refused(auc_csr(d_ip, d_ix, d_val, n, M, ip, ix, null=(k,)))
    # the refusals left nothing behind
    assert_exact(auc_dense(S, ip, ix), oracle_counts(S, lab))


# ------------------------------------------------------------------------------------------------------------------ 8. Python layer
def test_python_layer():
    from opentf_amd.evl import metric
    n, M = 60, 700
    lab = labels(n, M, 0.02, 71)
    Y = sp.csr_matrix(lab.astype(np.float32))
    s_ip, s_ix, s_val = topk_like(n, M, lab, 72)
    Ysp = sp.csr_matrix((s_val, s_ix, s_ip), shape=(n, M))
    D = Ysp.toarray()
    want = oracle_counts(D, lab)
    auc, counts = metric.micro_auc_device(Y, Ysp, return_counts=True)
    assert counts == want and all(type(c) is int for c in counts) and auc == auc_of(want)
    assert metric.micro_auc_device(Y, Ysp) == auc
    assert abs(auc - metric.micro_auc_sparse(Y, Ysp)) <= 1e-12
    assert abs(auc - sklearn_auc(D, lab)) <= 1e-12
    assert metric.micro_auc_device(Y, D, return_counts=True) == (auc, want)
    assert metric.micro_auc_device(Y, D.astype(np.float16).astype(np.float32)) == metric.micro_auc_device(Y, D.astype(np.float16))
    assert metric.micro_auc_device(Y, Ysp, chunk_bytes=64) == auc
    with pytest.raises(TypeError):
        metric.micro_auc_device(Y, D.astype(np.float64))
    # truth with explicit zeros and unsorted indices is cleaned as micro_auc_sparse cleans it
    Yz = Y.copy(); Yz.data[::5] = 0
    assert abs(metric.micro_auc_device(Yz, Ysp) - metric.micro_auc_sparse(Yz, Ysp)) <= 1e-12
    # calculate_auc_roc: device=0 against device=None, dense f32 and sparse
    for pred in (D, Ysp):
        host, none_a = metric.calculate_auc_roc(Y, pred)
        dev, none_b = metric.calculate_auc_roc(Y, pred, device=0)
        assert none_a is None and none_b is None and abs(host - dev) <= 1e-12 and dev == auc


def test_score_predictions_switch(monkeypatch):
    from opentf_amd.evl import metric
    n, M = 60, 700
    member = sp.csr_matrix(labels(3 * n, M, 0.02, 81).astype(np.float32))
    rows = np.random.default_rng(82).permutation(3 * n)[:n]
    s_ip, s_ix, s_val = topk_like(n, M, member[rows].toarray() != 0, 83)
    s_val = np.abs(s_val) + np.float32(0.01)                             # the ranking metrics take non-negative scores
    Ysp = sp.csr_matrix((s_val, s_ix, s_ip), shape=(n, M))
    spec = metric.EvalSpec(10, True, ["P_2,5", "recall_2,5", "ndcg_cut_2,5", "map_cut_2,5", "success_2,5"], ["aucroc"])
    tables = {}
    for pred_name, pred in (("sparse", Ysp), ("dense", Ysp.toarray())):
        for switch in (None, "0", "1"):
            if switch is None:
                monkeypatch.delenv("NTF_AUC_DEVICE", raising=False)
            else:
                monkeypatch.setenv("NTF_AUC_DEVICE", switch)
            tables[pred_name, switch] = metric.score_predictions({"member": member}, rows, pred, spec)
        inst0, mean0, roc0 = tables[pred_name, None]
        inst_off, mean_off, _ = tables[pred_name, "0"]
        inst1, mean1, roc1 = tables[pred_name, "1"]
        assert roc0 is None and roc1 is None
        assert mean_off.equals(mean0) and inst_off.equals(inst0)
        assert list(mean1.index) == list(mean0.index) and inst1.equals(inst0)
        others = [m for m in mean0.index if m != "aucroc"]
        assert len(others) == 10 and np.array_equal(mean1.loc[others, "mean"].values, mean0.loc[others, "mean"].values)
        assert abs(mean1.loc["aucroc", "mean"] - mean0.loc["aucroc", "mean"]) <= 1e-12
        assert mean1.loc["aucroc", "mean"] == auc_of(oracle_counts(Ysp.toarray(), member[rows].toarray() != 0))
