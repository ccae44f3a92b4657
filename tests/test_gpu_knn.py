"""Batched cosine nearest-neighbour search on the MI355X (opentf_amd/csrc/ntf_knn.hip, include/opentf_amd.h ntf_knn_*, libntf.Knn, KeyedVectors.most_similar_batch,
D2v.nearest_teams) against numpy in f64 on the same f32 inputs, s* = (T64 @ q64) / |T64 rows| / |q64|, within E(d) = (2 d + 16) * 2^-24 a sim (derived in
tests/test_knn_host.py, which also holds the reference and the table generators).

Largest |sim - s*| / E(d) seen over the parity cases on the device: 0.061 (N = 33, d = 64, Q = 31; 0.03 - 0.04 at d >= 100, 0.044 at d = 9).
At N = 70 001 and 262 444 (tests/test_gpu_long_ranges.py: the sampled selection route, the block-stride loop of k_sims): 0.057 and 0.075."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from opentf_amd import libntf                                                         # noqa: E402
from opentf_amd.mdl.emb import d2v as P                                               # noqa: E402
from test_knn_host import E, PARITY_CASES, make_queries, make_table, reference_sims   # noqa: E402

UNIT = libntf.Knn.UNIT_BYTES      # the header's smallest unit of work: 32 queries x 256 rows of f32 sims
NEG_INF = np.float32(-np.inf)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def check_lists(idx, sims, ref, d, topn, exclude=None):
    """every property of the contract the reference can decide, for every query; -> the largest |sim - s*| / E(d)"""
    Q, N = ref.shape
    assert idx.shape == (Q, topn) and sims.shape == (Q, topn) and idx.dtype == np.int32 and sims.dtype == np.float32
    tol, worst = E(d), 0.0
    for q in range(Q):
        ex = -1 if exclude is None else int(exclude[q])
        eligible = np.ones(N, bool)
        if ex >= 0: eligible[ex] = False
        n_el = int(eligible.sum())
        n_fill = max(0, topn - n_el)
        ids, sv = idx[q], sims[q]
        # fill slots only at the tail, exactly as many as rows are missing
        assert (ids[topn - n_fill:] == -1).all() and (sv[topn - n_fill:] == NEG_INF).all(), (q, ids, sv)
        ids, sv = ids[:topn - n_fill], sv[:topn - n_fill]
        assert ((ids >= 0) & (ids < N)).all() and len(set(ids.tolist())) == len(ids), (q, ids)
        assert ex not in ids.tolist()
        assert not np.isnan(sv).any() and not np.signbit(sv[sv == 0]).any()
        assert (np.diff(sv) <= 0).all(), (q, sv)
        same = np.diff(sv) == 0
        assert (np.diff(ids)[same] > 0).all(), (q, "ids must ascend among equal sims")
        err = np.abs(sv.astype(np.float64) - ref[q, ids])
        worst = max(worst, float(err.max() / tol))
        assert (err <= tol).all(), (q, float(err.max() / tol))
        if n_el >= topn:
            tau = np.sort(ref[q, eligible])[n_el - topn]           # the topn-th largest s* among the eligible rows
            assert (ref[q, ids] >= tau - 2 * tol).all(), (q, "a returned id lies below the list")
            must = np.flatnonzero(eligible & (ref[q] > tau + 2 * tol))
            assert np.isin(must, ids).all(), (q, "an id clearly inside the list is missing")
        else:
            assert sorted(ids.tolist()) == np.flatnonzero(eligible).tolist()
    return worst


@functools.lru_cache(maxsize=None)
def parity_case(ci):
    N, d, Q, topn = PARITY_CASES[ci]
    T = make_table("clustered" if ci % 2 else "mixed", N, d, seed=ci)
    Qv = make_queries(T, Q, seed=ci)
    for a in (T, Qv): a.setflags(write=False)
    return T, Qv, reference_sims(T, Qv)


@pytest.mark.parametrize("ci", range(len(PARITY_CASES)), ids=["N%d-d%d-Q%d-top%d" % c for c in PARITY_CASES])
def test_parity_with_the_f64_reference(ci):
    N, d, Q, topn = PARITY_CASES[ci]
    T, Qv, ref = parity_case(ci)
    k = libntf.Knn(T)
    assert (k.n_rows, k.d) == (N, d)
    idx, sims, ms = k.query(Qv, topn=topn, want_ms=True)
    worst = check_lists(idx, sims, ref, d, topn)
    print(f"\nN={N} d={d} Q={Q} topn={topn}: max |sim - s*| / E(d) = {worst:.3f}, {ms:.3f} ms")
    assert ms > 0
    # with one row excluded per query (the best one, the worst one, none, round robin)
    order = np.argsort(-ref, axis=1)
    exclude = np.asarray([(-1, order[q, 0], order[q, -1])[q % 3] for q in range(Q)], dtype=np.int64)
    idx2, sims2 = k.query(Qv, topn=topn, exclude=exclude)
    check_lists(idx2, sims2, ref, d, topn, exclude)
    none = exclude < 0
    assert np.array_equal(idx2[none], idx[none]) and np.array_equal(_bits(sims2[none]), _bits(sims[none]))
    k.close(); k.close()
    with pytest.raises(libntf.NtfError, match="closed"):
        k.query(Qv)


def test_signed_values_every_sim_negative():
    """the query is minus the table's mean direction: a selection that orders raw f32 bit patterns returns the MOST negative first"""
    rng = np.random.default_rng(3)
    d, N = 64, 700
    u = rng.standard_normal(d)
    T = (u[None, :] + 0.4 * rng.standard_normal((N, d))).astype(np.float32)
    Qv = np.stack([-T.astype(np.float64).mean(0), -u]).astype(np.float32)
    ref = reference_sims(T, Qv)
    assert (ref < -0.5).all()
    k = libntf.Knn(T)
    for topn in (1, 10, 300):
        idx, sims = k.query(Qv, topn=topn)
        check_lists(idx, sims, ref, d, topn)
        assert (sims < 0).all()
        for q in range(2):
            assert abs(ref[q, idx[q, 0]] - ref[q].max()) <= 2 * E(d)          # the first result is the least negative
    k.close()


def test_exact_ties_go_by_ascending_row_id():
    rng = np.random.default_rng(4)
    d, N = 100, 300
    T = rng.standard_normal((N, d)).astype(np.float32)
    Qv = rng.standard_normal((3, d)).astype(np.float32)
    T[17] = T[250]; T[100] = T[250]; T[101] = T[250]                            # four bit-identical rows: 17 < 100 < 101 < 250
    Qv[0] = T[250] + 0.01 * rng.standard_normal(d).astype(np.float32)           # ... at the top of query 0's list
    k = libntf.Knn(T)
    idx, sims = k.query(Qv, topn=N)
    check_lists(idx, sims, reference_sims(T, Qv), d, N)
    for q in range(3):
        at = [int(np.flatnonzero(idx[q] == i)[0]) for i in (17, 100, 101, 250)]
        assert at == list(range(at[0], at[0] + 4)), (q, at)                     # next to each other, lowest id first
        assert len(set(_bits(sims[q, at]).tolist())) == 1                       # equal sim bits
    assert idx[0, :4].tolist() == [17, 100, 101, 250]
    ex = np.asarray([100, -1, 17], dtype=np.int64)
    idx2, sims2 = k.query(Qv, topn=N, exclude=ex)
    for q in (0, 2):                                                            # the excluded id is absent and the list shifts by one
        keep = idx[q] != ex[q]
        assert np.array_equal(idx2[q, :N - 1], idx[q][keep]) and np.array_equal(_bits(sims2[q, :N - 1]), _bits(sims[q][keep]))
        assert idx2[q, N - 1] == -1 and sims2[q, N - 1] == NEG_INF
    assert np.array_equal(idx2[1], idx[1])
    k.close()
    # a table of one repeated row: ids 0 .. topn-1, with and without an exclusion, on both sides of the 32-row tile and of one selection pass
    for n_rows, topn in ((50, 7), (50, 50), (40000, 33), (40000, 300)):
        k = libntf.Knn(np.tile(T[5], (n_rows, 1)))
        idx, sims = k.query(Qv[:2], topn=topn, exclude=np.asarray([-1, 3]))
        assert idx[0].tolist() == list(range(topn)), (n_rows, topn)
        want = [i for i in range(topn + 1) if i != 3][:topn]
        if n_rows == topn: want = want[:-1] + [-1]
        assert idx[1].tolist() == want, (n_rows, topn)
        assert len(set(_bits(sims[0]).tolist())) == 1
        k.close()


def test_zero_and_near_zero_norms():
    d, N = 9, 40
    rng = np.random.default_rng(5)
    T = rng.standard_normal((N, d)).astype(np.float32)
    T[:, 0] = np.where(np.arange(N) % 2 == 0, np.abs(T[:, 0]) + 0.1, -np.abs(T[:, 0]) - 0.1)      # even ids positive against e0, odd ids negative
    zero_rows, tiny_rows, orth_rows = [4, 21], [9, 30], [2, 13, 38]
    T[zero_rows] = 0
    T[tiny_rows] = np.float32(1e-25)                      # squared norm 9e-50: underflows to 0, below FLT_MIN
    T[orth_rows, 0] = 0                                   # real zeros: orthogonal to e0
    T[13, 1] = -3.0
    T[38, 0] = -1e-45; T[38, 1] = 4.0                     # the smallest denormal against e0, then a row scaling <= 1/4: rounds to -0
    Qv = np.zeros((3, d), np.float32)
    Qv[0, 0] = 1.0                                        # e0
    Qv[2] = np.float32(1e-24)                             # a near-zero query
    zeros = sorted(zero_rows + tiny_rows + orth_rows)
    k = libntf.Knn(T)
    idx, sims = k.query(Qv, topn=N)
    assert not np.signbit(sims[sims == 0]).any() and np.isfinite(sims).all()
    pos = [i for i in range(N) if i % 2 == 0 and i not in zeros]
    n_pos = len(pos)
    assert sorted(idx[0, :n_pos].tolist()) == pos and (sims[0, :n_pos] > 0).all()
    assert idx[0, n_pos:n_pos + len(zeros)].tolist() == zeros                                 # zero rows rank among the real zeros by id
    assert _bits(sims[0, n_pos:n_pos + len(zeros)]).tolist() == [0] * len(zeros)              # exactly +0.0f
    assert (sims[0, n_pos + len(zeros):] < 0).all()
    for q in (1, 2):                                                                          # a zero query: the lowest eligible ids, all +0.0f
        assert idx[q].tolist() == list(range(N)) and not _bits(sims[q]).any()
    idx2, sims2 = k.query(Qv, topn=5, exclude=np.asarray([-1, 0, 2]))
    assert idx2[1].tolist() == [1, 2, 3, 4, 5] and idx2[2].tolist() == [0, 1, 3, 4, 5] and not _bits(sims2[1:]).any()
    k.close()


def test_the_result_does_not_depend_on_batch_or_budget():
    rng = np.random.default_rng(6)
    N, d, Q, topn = 3000, 128, 70, 10
    T = make_table("clustered", N, d, seed=77).copy()
    u = rng.standard_normal(d)
    # 4 units of budget: groups of 32 queries (g = 1), ranges of 256 * floor(4 * 32 KiB / 32 KiB) = 1024 rows - 3 ranges and 3 groups at N = 3000, Q = 70
    small = 4 * UNIT
    g = min(max(small // (8 << 20), 1), 32, -(-Q // 32)); r = min(small // (g * UNIT), 1024, -(-N // 256))       # (32 g = 32 queries a group: c = 1, gw = g)
    assert -(-Q // (32 * g)) >= 2 and -(-N // (256 * r)) >= 3 and r == 4
    planted = [0, 256 * r - 1, 256 * r, N - 1]           # the best rows: id 0, the last id of a range, the first id of the next, N - 1
    for j, p in enumerate(planted): T[p] = ((1.0 + j) * (u + 0.02 * rng.standard_normal(d))).astype(np.float32)
    Qv = (u[None, :] + 0.3 * rng.standard_normal((Q, d))).astype(np.float32)
    ref = reference_sims(T, Qv)
    k = libntf.Knn(T)
    idx, sims = k.query(Qv, topn=topn)
    check_lists(idx, sims, ref, d, topn)
    assert all(sorted(row[:4].tolist()) == planted for row in idx)               # the top of every list straddles the ranges
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    for ws in (small, UNIT, 3 * UNIT, 16 << 20):
        assert same(k.query(Qv, topn=topn, workspace_bytes=ws), (idx, sims)), ws
    a, b = k.query(Qv[:37], topn=topn), k.query(Qv[37:], topn=topn)              # split at an odd point
    assert same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), (idx, sims))
    perm = rng.permutation(Q)
    pi, ps = k.query(Qv[perm], topn=topn, workspace_bytes=small)
    assert same((pi, ps), (idx[perm], sims[perm]))
    ex = rng.integers(-1, N, size=Q); ex[:4] = planted
    e1 = k.query(Qv, topn=topn, exclude=ex)
    e2 = k.query(Qv[perm], topn=topn, exclude=ex[perm], workspace_bytes=small)
    assert same(e2, (e1[0][perm], e1[1][perm]))
    check_lists(e1[0], e1[1], ref, d, topn, ex)
    big = k.query(Qv, topn=2048, workspace_bytes=small)                          # the widest list through 3 merges
    assert same(big, k.query(Qv, topn=2048))
    assert np.array_equal(big[0][:, :topn], idx)
    k.close()


@pytest.mark.parametrize("Q,d", [(128, 128), (100, 100), (1000, 9)])
def test_batches_that_take_the_four_tile_sims_kernel(Q, d):
    """more than 64 queries at d <= 128 run k_knn_sims<4> (128 queries resident a workgroup; the header's c = 4): parity for every query, and the bits of the same
    batch asked for in calls of at most 32 queries (c = 1) and of 33 - 64 (c = 2).  Q = 1000 is 8 chunks of 4 tiles in one group, the last one short"""
    N, topn = 700, 12
    T = make_table("clustered", N, d, seed=40 + d)
    Qv = make_queries(T, Q, seed=40 + d)
    ref = reference_sims(T, Qv)
    k = libntf.Knn(T)
    ex = np.arange(Q, dtype=np.int64) % (N + 1) - 1
    idx, sims = k.query(Qv, topn=topn, exclude=ex)
    check_lists(idx, sims, ref, d, topn, ex)
    for step in (32, 27, 64):
        parts = [k.query(Qv[o:o + step], topn=topn, exclude=ex[o:o + step]) for o in range(0, Q, step)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), idx), step
        assert np.array_equal(_bits(np.concatenate([p[1] for p in parts])), _bits(sims)), step
    perm = np.random.default_rng(Q).permutation(Q)
    pi, ps = k.query(Qv[perm], topn=topn, exclude=ex[perm], workspace_bytes=64 << 20)       # g = 8 (Q = 1000): groups of 256 queries
    assert np.array_equal(pi, idx[perm]) and np.array_equal(_bits(ps), _bits(sims[perm]))
    k.close()


def _raw(h, q, n, topn, ex, ws, idx, sims, ms=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return libntf.lib().ntf_knn_query(h, p(q), n, topn, p(ex), ws, p(idx), p(sims), ms)


def test_refused_calls_leave_the_outputs_alone_and_say_why():
    L = libntf.lib()
    N, d = 50, 12
    rng = np.random.default_rng(7)
    T = rng.standard_normal((N, d)).astype(np.float32)
    Qv = rng.standard_normal((3, d)).astype(np.float32)
    k = libntf.Knn(T)
    h = k._h
    idx = np.full((3, 2048), -7, np.int32); sims = np.full((3, 2048), -7, np.float32)
    ok_ex = np.asarray([-1, 0, N - 1], np.int64)

    def bad(**kw):
        a = dict(q=Qv, n=3, topn=5, ex=ok_ex, ws=0, idx=idx, sims=sims); a.update(kw)
        rc = _raw(h, a["q"], a["n"], a["topn"], a["ex"], a["ws"], a["idx"], a["sims"])
        assert rc == -1, (kw.keys(), rc)
        assert (idx == -7).all() and (sims == -7).all(), kw.keys()
        msg = L.ntf_knn_last_error(h)
        assert msg, kw.keys()
        return msg.decode()

    assert "required" in bad(q=None) and "required" in bad(idx=None) and "required" in bad(sims=None)
    assert "n < 1" in bad(n=0) and "n < 1" in bad(n=-3)
    assert "topn" in bad(topn=0) and "topn" in bad(topn=2049) and "topn" in bad(topn=-1)
    for v in (np.nan, np.inf, -np.inf):
        q = Qv.copy(); q[2, d - 1] = v
        assert "not finite" in bad(q=q)
    q = Qv.copy(); q[1, :] = 1e20                           # finite values, but the f32 squared norm overflows
    assert "overflows" in bad(q=q)
    for v in (N, -2, 2 ** 40):
        assert "exclude" in bad(ex=np.asarray([-1, v, 0], np.int64))
    assert "unit" in bad(ws=UNIT - 1) and "unit" in bad(ws=1)
    assert "workspace_bytes" in bad(ws=-1)
    # and the same arguments, accepted (topn = 2048 on 50 rows; the smallest budget; exclude omitted)
    assert _raw(h, Qv, 3, 2048, None, UNIT, idx, sims) == 0
    assert (idx[:, :N] >= 0).all() and (idx[:, N:] == -1).all() and (sims[:, N:] == NEG_INF).all()
    k.close()

    def create(table, n, dd):
        out = C.c_void_p(0x1234)
        rc = L.ntf_knn_create(0, table.ctypes.data_as(C.c_void_p), n, dd, C.byref(out))
        assert rc == -1 and out.value is None
        msg = L.ntf_knn_last_error(None)
        assert msg
        return msg.decode()
    for v in (np.nan, np.inf, -np.inf):
        t = T.copy(); t[N - 1, d - 1] = v
        assert "not finite" in create(t, N, d)
    t = T.copy(); t[7, :] = -1e20
    assert "overflows" in create(t, N, d)
    t = T.copy(); t[0, 0] = 3e38                            # a single finite value whose square overflows
    assert "overflows" in create(t, N, d)
    with pytest.raises(libntf.NtfError, match="not finite"):
        libntf.Knn(np.full((2, 2), np.nan, np.float32))
    with pytest.raises(libntf.NtfError, match=r"queries must be \[n, 12\]"):
        libntf.Knn(T).query(np.ones((2, 11), np.float32))


def _toy_kv():
    rng = np.random.default_rng(8)
    centres = rng.standard_normal((5, 48))
    V = (centres[np.arange(500) % 5] + 0.2 * rng.standard_normal((500, 48))).astype(np.float32)
    return P.KeyedVectors([f"t{i}" for i in range(500)], V), rng


def test_plugin_most_similar_batch_is_the_host_route():
    kv, rng = _toy_kv()
    d = 48
    Qv = (kv.vectors[rng.integers(500, size=9)] + 0.1 * rng.standard_normal((9, d))).astype(np.float32)
    got = kv.most_similar_batch(Qv, topn=10)
    assert len(got) == 9 and all(len(g) == 10 for g in got)
    tol = 2 * E(d)                                          # both sides are f32
    for q in range(9):
        host = kv.most_similar([Qv[q]], topn=11)
        for j in range(10):
            assert abs(got[q][j][1] - host[j][1]) <= tol
            gap_before = host[j - 1][1] - host[j][1] if j else np.inf
            if min(gap_before, host[j][1] - host[j + 1][1]) > tol:      # the host's order is decided there
                assert got[q][j][0] == host[j][0], (q, j)
    knn = kv._knn
    assert kv.most_similar_batch(Qv[:2], topn=3) == [g[:3] for g in got[:2]] and kv._knn is knn      # the handle is made once
    # exclude_keys drops the key: the nearest key of a stored vector is itself
    own = kv.most_similar_batch(kv.vectors[[3, 40]], topn=4)
    assert [o[0][0] for o in own] == ["t3", "t40"]
    dropped = kv.most_similar_batch(kv.vectors[[3, 40]], topn=4, exclude_keys=["t3", None])
    assert [k_ for k_, _ in dropped[0]][:3] == [k_ for k_, _ in own[0]][1:] and "t3" not in [k_ for k_, _ in dropped[0]]
    assert dropped[1] == own[1]
    short = P.KeyedVectors(["a", "b", "c"], kv.vectors[:3].copy())
    assert [len(x) for x in short.most_similar_batch(kv.vectors[:2], topn=5, exclude_keys=["a", None])] == [2, 3]
    short.close()
    kv.close()
    assert kv._knn is None
    kv.close()


def test_plugin_nearest_teams_is_infer_vecs_then_the_search():
    from test_gpu_d2v_infer import _trained
    model, topic = _trained()
    t = P.D2v.__new__(P.D2v)
    t.model = model
    docs = [[f"s{12 * tp + j}" for j in (0, 3, 5, 7, 9, 11)] for tp in range(4)] + [["s1", "unknown"]]
    vecs, idx, sims = t.nearest_teams(docs, topn=10)
    assert np.array_equal(vecs, t.infer_vecs(docs))
    k = libntf.Knn(model.dv.vectors)
    want_idx, want_sims = k.query(vecs, topn=10)
    k.close()
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx) and np.array_equal(_bits(sims), _bits(want_sims))
    hits = sum(int(topic[i] == tp) for tp in range(4) for i in idx[tp])
    print(f"\nhits {hits} of 40")
    assert hits >= 30                                        # the criterion of the host route's test (tests/test_gpu_d2v_infer.py)
    check_lists(idx, sims, reference_sims(model.dv.vectors, vecs), 64, 10)
    shared = model.dv._knn                                   # one table on the device: the handle most_similar_batch uses
    assert shared is not None and t._infer_net is not None
    near = model.dv.most_similar_batch(vecs[:1], topn=10)
    assert model.dv._knn is shared and [int(k_) for k_, _ in near[0]] == idx[0].tolist()
    t.close()
    assert model.dv._knn is None and t._infer_net is None
    t.close()
