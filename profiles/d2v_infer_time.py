"""Batched infer_vector (ntf_d2v_infer) against the host route it stands beside (D2v.infer_vec), for profiles/d2v_infer_bench.md.
100 000 unseen teams at dblp's shape (90 671 skills, 1 + Poisson(7.57) skills a team, d = 128, PV-DM, window 5), epochs 10 and 100, five rounds of device_ms each;
the host route over 200 of the same documents.  The vocabulary tables come from a corpus of the same shape (build_vocab, sample 1e-3); wv / syn1neg are random
(sigma 0.05): the time of a frozen pass does not depend on the values except through the |f| >= 6 skip, which these never take.  One JSON line per configuration.
Table rows read are COUNTED, on a sample of 500 queries, from the same Philox draws the kernel takes (kept words and shrunk windows; a negative draw equal to the
word - 1 in ~10^4 here - is counted as read)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf                      # noqa: E402
from opentf_amd.mdl.emb import d2v as P            # noqa: E402
from opentf_amd.synth import zipf_csr              # noqa: E402

M32 = np.uint64(0xFFFFFFFF)


def philox_x(c0, c1, c2, c3, key):
    """first word of Philox4x32-10, vectorised over uint64 arrays that hold 32-bit values (ntf_d2v.hip d2v_draw)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def epoch_key(seed, epoch):
    M = (1 << 64) - 1
    x = (seed ^ ((epoch * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & M)) & M
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M; x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M; x ^= x >> 31
    return x & 0xFFFFFFFF, x >> 32


def rows_read(q_ptr, q_words, ids, sample_int, window, negative, epochs, seed, n_sample):
    """table rows (wv + syn1neg) the kernel reads per query, mean over the first n_sample queries"""
    total = 0
    for i in range(n_sample):
        w = q_words[q_ptr[i]:q_ptr[i + 1]]
        lo32, hi32 = int(ids[i]) & 0xFFFFFFFF, (int(ids[i]) >> 32) & 0xFFFFFFFF
        for e in range(epochs):
            key = epoch_key(seed, e)
            K = int((sample_int[w].astype(np.uint64) >= philox_x(lo32, hi32, np.arange(len(w), dtype=np.uint64) << np.uint64(8), 0, key)).sum())
            if not K: continue
            pos = np.arange(K, dtype=np.int64)
            b = (philox_x(lo32, hi32, pos.astype(np.uint64) << np.uint64(8), 1, key) % np.uint64(window)).astype(np.int64)
            total += int((np.minimum(K, pos + window + 1 - b) - np.maximum(0, pos - window + b) - 1).sum()) + K * (negative + 1)
    return total / n_sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--host-docs", type=int, default=200)
    ap.add_argument("--epochs", type=int, nargs="+", default=[10, 100]); ap.add_argument("--d", type=int, default=128)
    a = ap.parse_args()
    S, d, window, negative, seed = 90_671, a.d, 5, P.NEGATIVE, 1
    c_ptr, c_idx = zipf_csr(500_000, S, 8.57, 4)                                   # the corpus the vocabulary comes from
    keys, count, si, cum, _ = P.build_vocab(c_idx)
    V = len(keys)
    rank = np.full(S, -1, dtype=np.int64); rank[keys] = np.arange(V)
    q_ptr0, q_idx = zipf_csr(a.n, S, 8.57, 5)                                      # unseen teams of the same shape
    vi = rank[q_idx]
    known = vi >= 0                                                                # out-of-vocabulary skills are dropped on the host, as gensim drops them
    q_ptr = np.concatenate([[0], np.cumsum(np.add.reduceat(known.astype(np.int64), q_ptr0[:-1]))]).astype(np.int64)
    q_words = vi[known].astype(np.int32)
    rng = np.random.default_rng(0)
    wv = (rng.standard_normal((V, d)) * 0.05).astype(np.float32); s1 = (rng.standard_normal((V, d)) * 0.05).astype(np.float32)
    init = ((rng.random((a.n, d), dtype=np.float32) * 2 - 1) / d).astype(np.float32)
    ids = np.arange(a.n, dtype=np.int64) + 7_000_000
    net = libntf.Doc2Vec.from_tables(wv, s1, si, cum)
    net.infer(q_ptr[:1025], q_words[:q_ptr[1024]], init[:1024], 1, window, 2, P.ALPHA, 0.001, seed, negative=negative, ids=ids[:1024])        # untimed
    # the host route: 200 of the same documents through D2v.infer_vec (one doc vector in the model: most_similar over the corpus is not what is timed)
    t = P.D2v.__new__(P.D2v)
    word_keys = [f"s{int(k)}" for k in keys]
    docs = [[f"s{int(x)}" for x in q_idx[q_ptr0[i]:q_ptr0[i + 1]]] for i in range(a.host_docs)]
    for epochs in a.epochs:
        ms = []
        for _ in range(a.rounds):
            out, m = net.infer(q_ptr, q_words, init, 1, window, epochs, P.ALPHA, 0.001, seed, negative=negative, ids=ids, want_ms=True)
            ms.append(round(m, 3))
        assert np.isfinite(out).all() and not np.array_equal(out, init)
        med = float(np.median(ms))
        rows = rows_read(q_ptr, q_words, ids, si, window, negative, epochs, seed, min(500, a.n))
        t.model = P.Doc2VecTables(np.zeros((1, d), np.float32), wv, s1, word_keys, {"vector_size": d, "window": window, "dm": 1, "negative": negative, "ns_exponent": P.NS_EXPONENT,
                                                                                     "min_alpha": 0.001, "alpha": P.ALPHA, "epochs": epochs, "count": count})
        t0 = time.perf_counter()
        for doc in docs: t.infer_vec(doc)
        host_ms = (time.perf_counter() - t0) * 1e3 / len(docs)
        print(json.dumps({"n": a.n, "V": V, "d": d, "dm": 1, "window": window, "negative": negative, "epochs": epochs, "words": int(q_ptr[-1]), "device_ms_rounds": ms,
                          "device_ms_median": med, "device_us_per_query": round(med * 1e3 / a.n, 4), "queries_per_s": round(a.n / (med * 1e-3)), "table_rows_per_query": round(rows, 1),
                          "table_GB_per_s": round(rows * a.n * ((d + 63) // 64 * 64) * 4 / (med * 1e-3) / 1e9, 1), "host_docs": len(docs), "host_ms_per_doc": round(host_ms, 3),
                          "host_over_device": round(host_ms * 1e3 / (med * 1e3 / a.n))}), flush=True)
    net.close()


if __name__ == "__main__":
    main()
