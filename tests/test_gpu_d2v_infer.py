"""Batched doc2vec infer_vector on the MI355X (opentf_amd/csrc/ntf_d2v.hip k_d2v_infer, ntf_d2v_infer; opentf_amd/mdl/emb/d2v.py D2v.infer_vecs): gensim 4.3.3's
infer_vector as src/mdl/emb/d2v.py:96-98 calls it, with this build's Philox streams, against the sequential reference of tests/d2v_reference.py (oracle/d2v_oracle.py
has the draws, the key and the sigmoid table, but no inference pass)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import d2v_oracle as D                      # noqa: E402
from opentf_amd import libntf                           # noqa: E402
from opentf_amd.mdl.emb import d2v as P                 # noqa: E402
from d2v_reference import _query_words, _vocab60, reference_infer      # noqa: E402
from test_d2v import _clustered, _toy_teamsvecs         # noqa: E402

ALPHA, MIN_ALPHA, SEED = 0.025, 0.001, 11
SIGMA = {9: 1.6, 64: 0.8, 100: 0.8, 128: 0.7, 256: 0.6}


@functools.lru_cache(maxsize=None)
def case1(d, dm):
    """48 short queries against random tables.  Shared, read-only: -> dict of inputs + the reference"""
    si, cum = _vocab60()
    V = len(si)
    rng = np.random.default_rng(1000 * d + dm)
    wv = (rng.standard_normal((V, d)) * SIGMA[d]).astype(np.float32)
    s1 = (rng.standard_normal((V, d)) * SIGMA[d]).astype(np.float32)
    lens = 1 + rng.poisson(4, 48); lens[0] = 0; lens[1] = 1
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    q_words = _query_words(rng, int(q_ptr[-1]))                                     # repeats allowed
    ids = 1000 + np.arange(48, dtype=np.int64)
    init = ((rng.random((48, d), dtype=np.float32) * 2 - 1) / d).astype(np.float32) if dm else (rng.standard_normal((48, d)) * 0.35).astype(np.float32)
    c = dict(d=d, dm=dm, si=si, cum=cum, wv=wv, s1=s1, q_ptr=q_ptr, q_words=q_words, ids=ids, init=init, window=5, negative=3, epochs=2)
    c["ref"], c["flagged"], c["units"], c["skipped"] = reference_infer(q_ptr, q_words, ids, init, wv, s1, si, cum, dm, 5, 3, 2, ALPHA, MIN_ALPHA, SEED)
    for a in c.values():
        if isinstance(a, np.ndarray): a.setflags(write=False)
    return c


def _net(c):
    return libntf.Doc2Vec.from_tables(c["wv"], c["s1"], c["si"], c["cum"])


def _infer(net, c, sl=slice(None), **kw):
    qp = c["q_ptr"]
    lo, hi = sl.indices(len(qp) - 1)[:2]
    args = dict(negative=c["negative"], ids=c["ids"][lo:hi])
    args.update(kw)
    return net.infer(qp[lo:hi + 1] - qp[lo], c["q_words"][qp[lo]:qp[hi]], c["init"][lo:hi], c["dm"], c["window"], c["epochs"], ALPHA, MIN_ALPHA, SEED, **args)


def _check_parity(got, c, alpha=ALPHA):
    ref, flagged = c["ref"], c["flagged"]
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all()
    step = 0.003 * alpha * float(np.abs(c["s1"]).max()) * 2              # one bin step of the sigmoid, doubled
    for i in range(len(ref)):
        err, bound = float(np.abs(got[i] - ref[i]).max()), 2e-5 * float(np.abs(ref[i]).max()) + 1e-9
        print(f"query {i}: max|device - ref| {err:.3e}, bound {bound:.3e}, flagged units {int(flagged[i])}")
        assert err <= bound + step * int(flagged[i]), (i, err, bound, int(flagged[i]))


@pytest.mark.parametrize("dm", [1, 0])
@pytest.mark.parametrize("d", [9, 64, 100, 128, 256])
def test_infer_equals_the_sequential_reference(d, dm):
    """48 queries (one empty, one of one word, repeats, words the subsampling drops), every NV instantiation and both padded sizes: to rounding"""
    c = case1(d, dm)
    fragile = int((c["flagged"] > 0).sum())
    print(f"\nd {d} dm {dm}: {c['units']} units, {c['skipped']} skipped for |f| >= 6, {fragile} of 48 queries fragile")
    assert fragile <= 12, fragile                                          # from the reference alone: at most 25 % of the queries may sit on an edge
    assert not np.array_equal(c["ref"][2:], c["init"][2:])
    net = _net(c)
    got = _infer(net, c)
    net.close()
    assert np.array_equal(got[0], c["init"][0])                            # the empty query: its initial row, bit for bit
    _check_parity(got, c)


@pytest.mark.parametrize("dm", [1, 0])
def test_the_parity_cases_reach_the_skip_of_large_f(dm):
    """from the reference alone: at least one vector size per dm takes the |f| >= 6 skip on 20 or more units"""
    skipped = {d: case1(d, dm)["skipped"] for d in (9, 64, 100, 128, 256)}
    assert max(skipped.values()) >= 20, skipped


@functools.lru_cache(maxsize=None)
def case_long():
    """four queries of 1 500 words: past the 1 024-slot ring of kept words"""
    si, cum = _vocab60()
    V, d = len(si), 128
    rng = np.random.default_rng(77)
    wv = (rng.standard_normal((V, d)) * 0.02).astype(np.float32); s1 = (rng.standard_normal((V, d)) * 0.02).astype(np.float32)
    q_ptr = np.arange(5, dtype=np.int64) * 1500
    q_words = _query_words(rng, 6000)
    ids = 1000 + np.arange(4, dtype=np.int64)
    init = ((rng.random((4, d), dtype=np.float32) * 2 - 1) / d).astype(np.float32)
    c = dict(d=d, dm=1, si=si, cum=cum, wv=wv, s1=s1, q_ptr=q_ptr, q_words=q_words, ids=ids, init=init, window=5, negative=1, epochs=1)
    c["ref"], c["flagged"], c["units"], c["skipped"] = reference_infer(q_ptr, q_words, ids, init, wv, s1, si, cum, 1, 5, 1, 1, ALPHA, MIN_ALPHA, SEED)
    return c


def test_documents_longer_than_the_ring_of_kept_words():
    c = case_long()
    moved = float(np.abs(c["ref"] - c["init"]).max())
    print(f"\nlong documents: {c['units']} units, {int((c['flagged'] > 0).sum())} of 4 fragile, the vectors moved by {moved:.3f}")
    assert int((c["flagged"] > 0).sum()) <= 1 and c["units"] > 2 * 4 * 1024 and moved > 100 * 2e-5 * float(np.abs(c["ref"]).max())
    net = _net(c)
    got = _infer(net, c)
    net.close()
    _check_parity(got, c)


def test_the_result_does_not_depend_on_the_schedule():
    """bit for bit: the parallel launch and the one-wave launch, one call and two calls, a query at another place in the batch under the same id"""
    c = case1(128, 1)
    net = _net(c)
    full = _infer(net, c)
    assert np.array_equal(full, _infer(net, c, serial=True))
    assert np.array_equal(full, np.concatenate([_infer(net, c, slice(0, 20)), _infer(net, c, slice(20, 48))]))
    perm = np.random.default_rng(3).permutation(48)
    qp, lens = c["q_ptr"], np.diff(c["q_ptr"])
    p_ptr = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64)
    p_words = np.concatenate([c["q_words"][qp[j]:qp[j + 1]] for j in perm]).astype(np.int32)
    moved = net.infer(p_ptr, p_words, c["init"][perm], 1, 5, 2, ALPHA, MIN_ALPHA, SEED, negative=3, ids=c["ids"][perm])
    assert np.array_equal(moved, full[perm])
    # ... and the id IS part of the function: without ids a query is counted by its place
    assert not np.array_equal(_infer(net, c, ids=None)[2:], full[2:])
    net.close()


@pytest.mark.parametrize("dm", [1, 0])
def test_inference_leaves_every_table_as_it_was(dm):
    c = case1(128, dm)
    net = _net(c)
    before = [net.vectors(w) for w in (0, 1, 2)]
    assert np.array_equal(before[1], c["wv"]) and np.array_equal(before[2], c["s1"])
    got = _infer(net, c)
    assert not np.array_equal(got, c["init"])
    for w in (0, 1, 2): assert np.array_equal(net.vectors(w), before[w]), w
    net.close()


def _raw(net, n, q_ptr, q_words, init, out, ids=None, dm=1, window=5, negative=3, epochs=2, alpha=ALPHA, min_alpha=MIN_ALPHA, h="net"):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return libntf.lib().ntf_d2v_infer(net._h if h == "net" else None, n, p(q_ptr), p(q_words), p(ids), dm, window, negative, epochs, alpha, min_alpha, SEED, 0, p(init), p(out), None)


def test_refused_calls_leave_out_alone_and_say_why():
    c = case1(128, 1)
    net = _net(c)                                                          # a from_tables handle: no corpus
    qp, qw, init = np.array(c["q_ptr"][:5]), np.array(c["q_words"][:c["q_ptr"][4]]), np.array(c["init"][:4])
    out = np.full((4, 128), 7.25, dtype=np.float32)
    bad_ptr0 = qp + 1
    not_mono = qp.copy(); not_mono[2] = not_mono[3] + 1
    for bad in (-1, 60):
        w = qw.copy(); w[-1] = bad
        assert _raw(net, 4, qp, w, init, out) == libntf.NTF_EINVAL and b"vocabulary" in libntf.lib().ntf_d2v_last_error(net._h)
    refused = [dict(h=None), dict(q_ptr=None), dict(q_words=None), dict(init=None), dict(n=0), dict(n=-3), dict(q_ptr=bad_ptr0), dict(q_ptr=not_mono),
               dict(window=0), dict(window=256), dict(negative=-1), dict(negative=9), dict(dm=2), dict(dm=-1), dict(epochs=0),
               dict(alpha=float("nan")), dict(alpha=float("inf")), dict(min_alpha=float("nan")), dict(min_alpha=-float("inf"))]
    for kw in refused:
        a = dict(n=4, q_ptr=qp, q_words=qw, init=init, out=out); a.update(kw)
        assert _raw(net, **a) == libntf.NTF_EINVAL, kw
        assert len(libntf.lib().ntf_d2v_last_error(None if "h" in kw else net._h)) > 0, kw
        assert (out == 7.25).all(), kw
    assert _raw(net, 4, qp, qw, init, None) == libntf.NTF_EINVAL
    # the same arguments, accepted: the call works after the refusals, on a handle that never had a corpus
    assert _raw(net, 4, qp, qw, init, out, ids=np.array(c["ids"][:4])) == 0
    assert np.array_equal(out, _infer(net, c)[:4]) and np.array_equal(out[0], init[0])        # query 0 is empty: its initial row
    with pytest.raises(libntf.NtfError): net.infer(qp, qw, init[:3], 1, 5, 2, ALPHA, MIN_ALPHA, SEED)
    net.close()


@functools.lru_cache(maxsize=None)
def _trained():
    """tests/test_d2v.py test_infer_vec_lands_among_the_documents_of_its_topic's model: its corpus, vocabulary, initial vectors, schedule, seed and hyper-parameters.
    The eight passes run on the device's one-wave trainer, which test_gpu_d2v.py pins to that test's D.train_epoch to rounding (the Python loop takes 10 s)."""
    rng = np.random.default_rng(9)
    ptr, words, topic = _clustered(rng, n_docs=400, topics=4, per_topic=12, L=6)
    v = D.prepare_vocab(ptr, words, sample=0)
    wi = np.asarray([v["index_of"][int(w)] for w in words], dtype=np.int64)
    wv, dv, s1 = D.init_vectors(len(ptr) - 1, len(v["keys"]), 64, 1)
    sch, _ = D.alpha_schedule(8, 0.001, spe=None, alpha=0.05)
    net = libntf.Doc2Vec(ptr, wi, v["sample_int"], v["cum_table"], wv, dv, seed=1)
    for ep, (a0, a1) in enumerate(sch): net.train_epoch(1, 5, a0, a1, ep, serial=True)
    dv, wv, s1 = net.vectors(0), net.vectors(1), net.vectors(2)
    net.close()
    model = P.Doc2VecTables(dv, wv, s1, [f"s{int(k)}" for k in v["keys"]],
                            {"vector_size": 64, "window": 5, "dm": 1, "negative": 5, "ns_exponent": 0.75, "min_alpha": 0.001, "alpha": 0.025, "epochs": 20, "count": v["count"]})
    return model, topic


def test_plugin_infers_held_out_documents_next_to_their_topic():
    model, topic = _trained()
    t = P.D2v.__new__(P.D2v)
    t.model = model
    docs = [[f"s{12 * tp + j}" for j in (0, 3, 5, 7, 9, 11)] for tp in range(4)]
    vecs = t.infer_vecs(docs)
    assert vecs.shape == (4, 64) and vecs.dtype == np.float32
    hits = 0
    for tp in range(4):
        near = model.docvecs.most_similar([vecs[tp]])
        assert len(near) == 10
        hits += sum(topic[int(k)] == tp for k, _ in near)
    print(f"\nhits {hits} of 40")
    assert hits >= 30, hits          # test_d2v.py's criterion for infer_vec: 40 neighbours in all, 25 % would be chance
    assert np.array_equal(t.infer_vecs(docs), vecs)                        # twice: identical bits
    assert np.array_equal(t.infer_vecs(docs[::-1] + [["s1", "unknown"]])[:4][::-1], vecs)     # a document's vector is a function of its words, not of its place
    assert t._infer_net is not None
    t.close()
    assert t._infer_net is None
    t.close()


@pytest.mark.parametrize("embtype", ["skill", "skillmember"])
def test_plugin_team_vectors_are_the_inferred_team_documents(embtype):
    tv = _toy_teamsvecs(np.random.default_rng(2))
    n, S = tv["skill"].shape
    M = tv["member"].shape[1]
    keys = [f"s{j}" for j in range(S)] + ([f"m{j}" for j in range(M)] if embtype == "skillmember" else [])
    rng = np.random.default_rng(4)
    V, d = len(keys), 9
    t = P.D2v.__new__(P.D2v)
    t.cfg = {"embtype": embtype}
    t.model = P.Doc2VecTables(np.zeros((n, d), np.float32), (rng.standard_normal((V, d)) * 0.5).astype(np.float32), (rng.standard_normal((V, d)) * 0.5).astype(np.float32), keys,
                              {"vector_size": d, "window": 5, "dm": 1, "negative": 5, "ns_exponent": 0.75, "min_alpha": 0.001, "alpha": 0.025, "epochs": 3, "seed": 5,
                               "count": np.sort(rng.integers(1, 50, V))[::-1]})
    rows = np.asarray([7, 0, 31, 7])
    ptr, words, key = P.team_documents(tv, embtype)
    docs = [[key(int(w)) for w in words[ptr[i]:ptr[i + 1]]] for i in range(n)]
    got = t.infer_team_vecs(tv, rows)
    assert got.shape == (4, d) and np.array_equal(got, t.infer_vecs([docs[i] for i in rows]))
    assert np.array_equal(got[0], got[3]) and not np.array_equal(got[0], got[1])
    everything = t.infer_team_vecs(tv)
    assert np.array_equal(everything, t.infer_vecs((ptr, words, key))) and np.array_equal(everything[rows], got)        # the (doc_ptr, word ids, key) triple
    t.close()
