"""Host side of the batched infer_vector (opentf_amd/mdl/emb/d2v.py: vocab_tables, query_csr, infer_init / infer_seeds) against build_vocab and against what
D2v.infer_vec starts from.  No GPU."""
import zlib

import numpy as np
import pytest

from opentf_amd.mdl.emb import d2v as P
from test_d2v import SETS, Z


def _zipf_words(seed=0, n=4000, V=300):
    rng = np.random.default_rng(seed)
    pop = 1.0 / (np.arange(V) + 3.0); pop /= pop.sum()
    return rng.choice(V, n, replace=True, p=pop).astype(np.int64)


@pytest.mark.parametrize("corpus", list(SETS) + ["zipf"])
@pytest.mark.parametrize("sample", [P.SAMPLE, 0.05, 0])
def test_vocab_tables_from_the_counts_alone_are_build_vocabs(corpus, sample):
    words = _zipf_words() if corpus == "zipf" else Z[f"{corpus}_words"]
    keys, count, si, cum, wi = P.build_vocab(words, sample=sample)
    si2, cum2 = P.vocab_tables(count, sample=sample)
    assert si2.dtype == np.uint32 and cum2.dtype == np.uint32
    assert np.array_equal(si, si2) and np.array_equal(cum, cum2)
    if sample == P.SAMPLE:                                   # the defaults are build_vocab's defaults
        d1, d2 = P.vocab_tables(count)
        assert np.array_equal(d1, si) and np.array_equal(d2, cum)
    if corpus != "zipf" and sample == P.SAMPLE: assert np.array_equal(si2, Z[f"{corpus}_sample_int"])       # gensim's own, value for value
    assert np.array_equal(P.vocab_tables(count.tolist(), sample=sample, ns_exponent=0.5)[1], P.build_vocab(words, sample=sample, ns_exponent=0.5)[3])


def test_word_keys_become_vocabulary_indices_in_order_without_the_unknown_ones():
    k2i = {"s3": 0, "s1": 1, "m2": 2, "s10": 3}
    ptr, idx = P.query_csr([["s1", "s99", "s3", "s1"], [], ["nope"], ["s10", "m2"]], k2i)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32
    assert ptr.tolist() == [0, 3, 3, 3, 5] and idx.tolist() == [1, 0, 1, 3, 2]
    ptr, idx = P.query_csr([], k2i)
    assert ptr.tolist() == [0] and len(idx) == 0 and idx.dtype == np.int32


@pytest.mark.parametrize("d", [9, 64, 128])
def test_default_initial_rows_are_what_infer_vec_starts_from(d):
    docs = [["s1", "s5"], [], ["s7"], ["s5", "s1"], ["unknown", "s1"]]
    init, seeds = P.infer_init(docs, d), P.infer_seeds(docs)
    assert init.shape == (5, d) and init.dtype == np.float32 and seeds.dtype == np.int64
    for i, words in enumerate(docs):
        # D2v.infer_vec, literally
        rng = np.random.default_rng(zlib.crc32(" ".join(words).encode()))
        v = ((rng.random(d, dtype=np.float32) * 2 - 1) / d).astype(np.float32)
        assert np.array_equal(init[i], v) and seeds[i] == zlib.crc32(" ".join(words).encode())
    assert not np.array_equal(init[0], init[3])              # the order of the words is part of the seed, as in infer_vec
    assert np.abs(init).max() <= 1.0 / d


def test_infer_vecs_refuses_a_model_without_counts_as_infer_vec_does():
    t = P.D2v.__new__(P.D2v)
    t.model = P.Doc2VecTables(np.zeros((1, 8), np.float32), np.zeros((3, 8), np.float32), np.zeros((3, 8), np.float32), ["s0", "s1", "s2"],
                              {"vector_size": 8, "window": 5, "dm": 1, "negative": 5, "ns_exponent": 0.75, "min_alpha": 0.001, "alpha": 0.025, "epochs": 2})
    with pytest.raises(RuntimeError, match="holds no vocabulary counts") as e1: t.infer_vec(["s1"])
    with pytest.raises(RuntimeError, match="holds no vocabulary counts") as e2: t.infer_vecs([["s1"]])
    assert str(e1.value) == str(e2.value)
    t.close()                                                # nothing was opened: a no-op
