"""Host side of the batched cosine nearest-neighbour search (include/opentf_amd.h ntf_knn_*, opentf_amd/libntf.py Knn, opentf_amd/mdl/emb/d2v.py
KeyedVectors.most_similar_batch) and the reference / tolerance helpers tests/test_gpu_knn.py imports.  No GPU.

The reference is numpy in f64 on the same f32 inputs, s* = (T64 @ q64) / |T64 rows| / |q64|.  The tolerance on a sim is E(d) = (2 d + 16) * 2^-24:
  the fmaf chain is off by at most gamma_d |t| |q| (gamma_d ~ d * 2^-24), each f32 norm by at most gamma_d / 2 + 3 * 2^-24 relative (chain, square root, division),
  the two scalings add 2 * 2^-24.
test_the_bound_holds_on_a_sequential_f32_route runs the header's order of operations in emulated f32 at the GPU file's parity shapes: the largest |sim - s*| / E(d)
it has seen is 0.076 (d = 9, mixed magnitudes); 0.02 - 0.06 at d >= 64."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

EPS = 2.0 ** -24
FLT_MIN = np.float32(1.17549435e-38)
# (N, d, Q, topn) - the parity cases of tests/test_gpu_knn.py
PARITY_CASES = [(1, 1, 1, 1), (31, 9, 1, 10), (33, 64, 31, 33), (257, 100, 33, 10), (3000, 128, 70, 10), (3000, 256, 33, 2048), (40, 128, 5, 43)]


def E(d):
    return (2 * d + 16) * EPS


def reference_sims(T, Q):
    """s* [Q, N] in f64 from the f32 inputs; a zero norm gives 0 (the contract's sim with a zero row or query)"""
    T64, Q64 = np.asarray(T, np.float64), np.asarray(Q, np.float64)
    nt, nq = np.linalg.norm(T64, axis=1), np.linalg.norm(Q64, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (Q64 @ T64.T) / nt[None, :] / nq[:, None]
    s[:, nt == 0] = 0.0
    s[nq == 0, :] = 0.0
    return s


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two f32 is exact in f64; the sum is rounded to f64, then to f32 (a double rounding that differs from fmaf by at most one
    f32 ulp in 2^-29 of the cases - nothing to an error bound)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulated_sims(T, Q):
    """the header's order of operations in f32, sequentially: k-ordered fmaf chains for the dot product and the squared norms, r = 1 / sqrt(n2) (0 below FLT_MIN),
    sim = (dot * rq) * rt -> [Q, N] float32"""
    T, Q = np.asarray(T, np.float32), np.asarray(Q, np.float32)
    dot = np.zeros((len(Q), len(T)), np.float32)
    for k in range(T.shape[1]):
        dot = _fma32(Q[:, k][:, None], T[:, k][None, :], dot)

    def rinv(X):
        n2 = np.zeros(len(X), np.float32)
        for k in range(X.shape[1]): n2 = _fma32(X[:, k], X[:, k], n2)
        with np.errstate(divide="ignore"):
            r = np.float32(1) / np.sqrt(n2, dtype=np.float32)
        return np.where(n2 < FLT_MIN, np.float32(0), r).astype(np.float32)
    rt, rq = rinv(T), rinv(Q)
    sim = (dot * rq[:, None]) * rt[None, :]
    sim[(rq == 0)[:, None] | (rt == 0)[None, :]] = 0
    return sim + np.float32(0)      # -0 -> +0


def make_table(kind, N, d, seed):
    """normal / all-positive / clustered / mixed-magnitude (row scales 1e-6 .. 1e5) tables [N, d] float32"""
    rng = np.random.default_rng(seed)
    if kind == "normal": return rng.standard_normal((N, d)).astype(np.float32)
    if kind == "positive": return (rng.random((N, d)) + 0.05).astype(np.float32)
    centres = rng.standard_normal((8, d))
    T = centres[rng.integers(8, size=N)] + 0.15 * rng.standard_normal((N, d))
    if kind == "mixed": T = T * 10.0 ** rng.uniform(-6, 5, size=(N, 1))
    return T.astype(np.float32)


def make_queries(T, Q, seed):
    """queries near rows of the table (so the top of every list is crowded) [Q, d] float32"""
    rng = np.random.default_rng(seed + 1000)
    pick = T[rng.integers(len(T), size=Q)].astype(np.float64)
    scale = np.maximum(np.abs(pick).max(axis=1, keepdims=True), 1e-30)
    return (pick / scale + 0.2 * rng.standard_normal(pick.shape)).astype(np.float32)


def _header():
    return open(os.path.join(ROOT, "include", "opentf_amd.h")).read()


def test_the_four_symbols_are_declared_exported_and_bound():
    from opentf_amd import libntf
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    assert "typedef struct ntf_knn ntf_knn;" in flat
    assert "int ntf_knn_create(int device, const float* table , int64_t n_rows, int32_t d, ntf_knn** out);" in flat
    assert "void ntf_knn_destroy(ntf_knn* h);" in flat
    assert "const char* ntf_knn_last_error(const ntf_knn* h);" in flat
    assert ("int ntf_knn_query(ntf_knn* h, const float* queries , int64_t n, int32_t topn, const int64_t* exclude , int64_t workspace_bytes, "
            "int32_t* out_idx , float* out_sims , double* device_ms );") in flat
    assert re.search(r"#define NTF_KNN_WORKSPACE_BYTES \(\(int64_t\)256 << 20\)", src)
    assert re.search(r"#define NTF_ABI_VERSION 2\b", src)
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"ntf_knn_create": (C.c_int, [C.c_int, P, I64, I32, C.POINTER(P)]), "ntf_knn_destroy": (None, [P]), "ntf_knn_last_error": (C.c_char_p, [P]),
            "ntf_knn_query": (C.c_int, [P, P, I64, I32, P, I64, P, P, P])}
    for name, sig in want.items():
        assert libntf.SYMBOLS[name] == sig, name
        fn = getattr(libntf.lib(), name)                 # exported, and bound with that signature
        assert fn.restype == sig[0] and list(fn.argtypes) == sig[1]
    assert libntf.Knn.WORKSPACE_BYTES == 256 << 20 and libntf.Knn.UNIT_BYTES == 32 * 256 * 4


def test_knn_has_no_cpu_fallback():
    from opentf_amd import libntf
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(libntf.NtfError, match="no HIP device"):
        libntf.Knn(np.ones((4, 3), np.float32))
    with pytest.raises(libntf.NtfError, match=r"\[rows, d\]"):
        libntf.Knn(np.ones(4, np.float32))


def test_refusals_that_need_no_device():
    """argument checks in front of the device lookup: they answer NTF_EINVAL with a message on any machine"""
    from opentf_amd import libntf
    L = libntf.lib()
    t = np.ones((4, 3), np.float32)
    for table, n, d, out in [(None, 4, 3, True), (t, 0, 3, True), (t, 2 ** 31, 3, True), (t, 4, 0, True), (t, 4, 257, True), (t, 4, 3, False)]:
        h = C.c_void_p(0x1234)
        rc = L.ntf_knn_create(0, None if table is None else table.ctypes.data_as(C.c_void_p), n, d, C.byref(h) if out else None)
        assert rc == -1 and L.ntf_knn_last_error(None)
        assert h.value == (None if out else 0x1234)          # *out is cleared when it can be; never a handle
    idx = np.full((1, 2), -7, np.int32); sims = np.full((1, 2), -7, np.float32)
    assert L.ntf_knn_query(None, t.ctypes.data_as(C.c_void_p), 1, 2, None, 0, idx.ctypes.data_as(C.c_void_p), sims.ctypes.data_as(C.c_void_p), None) == -1
    assert L.ntf_knn_last_error(None) and (idx == -7).all() and (sims == -7).all()
    L.ntf_knn_destroy(None)


def test_most_similar_batch_validates_before_touching_the_library(monkeypatch):
    from opentf_amd import libntf
    from opentf_amd.mdl.emb import d2v as P

    def boom(*a, **k): raise AssertionError("the library was touched")
    monkeypatch.setattr(libntf, "Knn", boom)
    monkeypatch.setattr(libntf, "lib", boom)
    kv = P.KeyedVectors([str(i) for i in range(6)], np.eye(6, 4, dtype=np.float32))
    assert callable(kv.most_similar_batch)
    for bad in (np.ones(4, np.float32), np.ones((2, 5), np.float32), np.ones((2, 2, 4), np.float32)):
        with pytest.raises(ValueError, match="vectors must be"):
            kv.most_similar_batch(bad)
    for topn in (0, 2049):
        with pytest.raises(ValueError, match="topn"):
            kv.most_similar_batch(np.ones((2, 4), np.float32), topn=topn)
    with pytest.raises(ValueError, match="exclude_keys"):
        kv.most_similar_batch(np.ones((2, 4), np.float32), exclude_keys=["0"])
    with pytest.raises(KeyError):
        kv.most_similar_batch(np.ones((2, 4), np.float32), exclude_keys=["0", "nope"])
    assert kv.most_similar_batch(np.ones((0, 4), np.float32)) == []
    with pytest.raises(AssertionError, match="touched"):             # a valid call is the first to reach for the device
        kv.most_similar_batch(np.ones((2, 4), np.float32))
    kv.close(); kv.close()
    # the host route is what it was
    got = kv.most_similar([np.asarray([1, 0.5, 0, 0], np.float32)], topn=2)
    assert [k for k, _ in got] == ["0", "1"]
    assert callable(P.D2v.nearest_teams)


@pytest.mark.parametrize("kind", ["normal", "positive", "clustered", "mixed"])
def test_the_bound_holds_on_a_sequential_f32_route(kind):
    worst = 0.0
    for ci, (N, d, Q, _) in enumerate(PARITY_CASES):
        T = make_table(kind, N, d, seed=ci)
        Qv = make_queries(T, Q, seed=ci)
        ratio = float(np.abs(emulated_sims(T, Qv).astype(np.float64) - reference_sims(T, Qv)).max() / E(d))
        print(f"{kind} N={N} d={d} Q={Q}: max |sim - s*| / E(d) = {ratio:.3f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0
    assert worst <= 1.0


def test_reference_and_emulation_on_zero_norms():
    T = np.zeros((3, 4), np.float32); T[1] = [1, -2, 0, 0]; T[2] = 1e-25
    Q = np.asarray([[0, 0, 0, 0], [1, -2, 0, 0]], np.float32)
    em = emulated_sims(T, Q)
    assert em.tobytes() == np.asarray([[0, 0, 0], [0, 1, 0]], np.float32).tobytes()      # n2 below FLT_MIN: exactly +0.0f
    ref = reference_sims(T, Q)
    assert ref[0].tolist() == [0, 0, 0] and ref[1, 0] == 0 and abs(ref[1, 1] - 1) < 1e-15
