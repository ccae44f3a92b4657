"""Host side of the link decode (include/opentf_amd_link.h ntf_link_*, opentf_amd/libntf.py Link, opentf_amd/mdl/emb/gnn.py Gnn.test / recommend) and the
reference / tolerance helpers tests/test_gpu_link.py imports.  No GPU.

The reference is numpy in f64 on the same f32 inputs, x* = t64 . q64.  The tolerance on a logit is E(i, j) = (d + 2) * 2^-24 * sum_k |t_jk| |q_ik|: a chain of d fused
multiply-adds rounds d times, so it is off by at most gamma_d * sum |t q| with gamma_d = d u / (1 - d u), u = 2^-24, and (d + 2) u covers gamma_d for d <= 256.
The tolerance on a probability is the header's: |p - p*| <= (4 u + 2^-40) p* for |x| <= 30 (expf within 1 ulp = 2 u relative, passed on by 1 + e scaled by
e / (1 + e) < 1; the addition and the correctly rounded division add u each; 2^-40 covers the second-order terms).
test_the_bound_holds_on_a_sequential_f32_route runs the chain in emulated f32: the largest |x - x*| / E it has seen is 0.121 (d = 9; 0.05 - 0.09 at d >= 100)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse
import torch

from conftest import ROOT
from n2v_reference import Cfg, plugin_cfg

U = 2.0 ** -24
P_BOUND = 4 * U + 2.0 ** -40        # relative, |x| <= 30
P_RANGE = 30.0
# (n_rows, d, cand_lo, C, n, K) - the parity cases of tests/test_gpu_link.py: pad columns at d = 9 and 100, the 4-tile workgroup at d = 128 with more than 64
# queries, the 2-tile one at d = 256; candidate blocks that start off a multiple of 32; K = 1, 10, C, C + 5 and 2048
PARITY_CASES = [(40, 9, 7, 33, 1, 1), (300, 100, 0, 257, 31, 10), (1100, 128, 301, 700, 97, 700), (1100, 128, 301, 700, 65, 705), (3400, 256, 301, 3000, 33, 2048),
                (3007, 128, 7, 3000, 97, 10)]


def E(T, Q):
    """[n, C] bound of |x - x*| for candidate rows T [C, d] and query vectors Q [n, d]"""
    d = T.shape[1]
    return (d + 2) * U * (np.abs(np.asarray(Q, np.float64)) @ np.abs(np.asarray(T, np.float64)).T)


def reference_logits(T, Q):
    """x* [n, C] in f64 from the f32 inputs"""
    return np.asarray(Q, np.float64) @ np.asarray(T, np.float64).T


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def rank(x):
    """the contract's order of every row of x [n, C]: value descending, id ascending among equal values -> ids [n, C]"""
    return np.argsort(-np.asarray(x, np.float64), axis=1, kind="stable")


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two f32 is exact in f64; the sum is rounded to f64, then to f32 (a double rounding that differs from fmaf by at most one
    f32 ulp in 2^-29 of the cases - nothing to an error bound)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulated_logits(T, Q):
    """the header's chain in f32, sequentially -> [n, C] float32"""
    T, Q = np.asarray(T, np.float32), np.asarray(Q, np.float32)
    x = np.zeros((len(Q), len(T)), np.float32)
    for k in range(T.shape[1]):
        x = _fma32(Q[:, k][:, None], T[:, k][None, :], x)
    return x + np.float32(0)


def make_table(n_rows, d, seed, scale=1.0):
    """a clustered table [n_rows, d] float32 (8 centres, rows near them) whose dot products are a few units times `scale`^2: the head of every list is crowded"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((8, d))
    T = centres[rng.integers(8, size=n_rows)] + 0.3 * rng.standard_normal((n_rows, d))
    return (T * (scale * 1.7 / np.sqrt(d))).astype(np.float32)


def make_query_rows(n_rows, n, seed):
    """n query rows anywhere in the table (inside the candidate block or not), repeats allowed"""
    return np.random.default_rng(seed + 1000).integers(n_rows, size=n).astype(np.int64)


def make_pooled(lo, hi, n, seed, most=6):
    """a CSR of n non-empty rows over the table rows [lo, hi) -> (ptr int64 [n + 1], items int64)"""
    rng = np.random.default_rng(seed + 2000)
    sizes = 1 + rng.integers(most, size=n)
    items = np.concatenate([np.sort(rng.choice(hi - lo, size=min(s, hi - lo), replace=False)) + lo for s in sizes]).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum([min(s, hi - lo) for s in sizes])]).astype(np.int64)
    return ptr, items


# ------------------------------------------------------------------------------------------------------------------ header, exports, binding
def _flat(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return src, re.sub(r"\s+", " ", src)


def test_header_exports_and_link_symbols_agree():
    from opentf_amd import libntf
    src, flat = _flat("opentf_amd_link.h")
    assert '#include "opentf_amd.h"' in src and "typedef struct ntf_link ntf_link;" in flat
    protos = ["int ntf_link_create(int device, const float* table , int64_t n_rows, int32_t d, int64_t cand_lo, int64_t cand_hi, ntf_link** out);",
              "void ntf_link_destroy(ntf_link* h);",
              "const char* ntf_link_last_error(const ntf_link* h);",
              "int ntf_link_topk (ntf_link* h, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const int64_t* q_items, int32_t K, int64_t workspace_bytes, "
              "int32_t* out_idx, float* out_logit, float* out_prob, double* device_ms);",
              "int ntf_link_dense(ntf_link* h, int64_t n, const int64_t* q_rows, const int64_t* q_ptr, const int64_t* q_items, int64_t workspace_bytes, "
              "float* out_logit, float* out_prob, double* device_ms);"]
    for p in protos:
        assert p in flat, p
    declared = set(re.findall(r"\b(ntf_link_\w+)\s*\(", src))
    assert declared == set(libntf.LINK_SYMBOLS) and len(declared) == 5
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"ntf_link_create": (C.c_int, [C.c_int, P, I64, I32, I64, I64, C.POINTER(P)]), "ntf_link_destroy": (None, [P]), "ntf_link_last_error": (C.c_char_p, [P]),
            "ntf_link_topk": (C.c_int, [P, I64, P, P, P, I32, I64, P, P, P, P]), "ntf_link_dense": (C.c_int, [P, I64, P, P, P, I64, P, P, P])}
    for name, sig in want.items():
        assert libntf.LINK_SYMBOLS[name] == sig, name
        fn = getattr(libntf.lib(), name)                 # exported, and bound with that signature
        assert fn.restype == sig[0] and list(fn.argtypes) == sig[1]
    # a side header: nothing of it in the main header or its table, whose count and version stand
    main_src, _ = _flat("opentf_amd.h")
    assert "ntf_link" not in main_src and not any(k.startswith("ntf_link") for k in libntf.SYMBOLS)
    assert len(libntf.SYMBOLS) == 90 and libntf.NTF_ABI_VERSION == 2 and re.search(r"#define NTF_ABI_VERSION 2\b", main_src)
    assert libntf.lib().ntf_abi_version() == 2
    assert libntf.Link.WORKSPACE_BYTES == 256 << 20 and libntf.Link.UNIT_BYTES == 32 * 256 * 4 and libntf.Link.MAX_K == 2048


def test_refusals_that_need_no_device():
    """argument checks in front of the device lookup: they answer NTF_EINVAL with a message on any machine"""
    from opentf_amd import libntf
    L = libntf.lib()
    t = np.ones((4, 3), np.float32)
    #        table n  d  lo hi out
    cases = [(None, 4, 3, 0, 4, True), (t, 0, 3, 0, 0, True), (t, 2 ** 31, 3, 0, 4, True), (t, 4, 0, 0, 4, True), (t, 4, 257, 0, 4, True),
             (t, 4, 3, -1, 4, True), (t, 4, 3, 0, 5, True), (t, 4, 3, 2, 2, True), (t, 4, 3, 3, 2, True), (t, 4, 3, 0, 4, False)]
    for table, n, d, lo, hi, out in cases:
        h = C.c_void_p(0x1234)
        rc = L.ntf_link_create(0, None if table is None else table.ctypes.data_as(C.c_void_p), n, d, lo, hi, C.byref(h) if out else None)
        assert rc == -1 and L.ntf_link_last_error(None), (n, d, lo, hi)
        assert h.value == (None if out else 0x1234)          # *out is cleared when it can be; never a handle
    idx = np.full((1, 2), -7, np.int32); val = np.full((1, 2), -7, np.float32)
    rows = np.zeros(1, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.ntf_link_topk(None, 1, p(rows), None, None, 2, 0, p(idx), p(val), None, None) == -1
    assert L.ntf_link_dense(None, 1, p(rows), None, None, 0, p(val), None, None) == -1
    assert L.ntf_link_last_error(None) and (idx == -7).all() and (val == -7).all()
    L.ntf_link_destroy(None)


def test_link_has_no_cpu_fallback():
    from opentf_amd import libntf
    with pytest.raises(libntf.NtfError, match=r"\[rows, d\]"):
        libntf.Link(np.ones(4, np.float32), 0, 1)
    if not torch.cuda.is_available():
        with pytest.raises(libntf.NtfError, match="no HIP device"):
            libntf.Link(np.ones((4, 3), np.float32), 0, 4)


# ------------------------------------------------------------------------------------------------------------------ the bounds, on the host
@pytest.mark.parametrize("ci", range(len(PARITY_CASES)))
def test_the_bound_holds_on_a_sequential_f32_route(ci):
    n_rows, d, lo, Cn, n, _ = PARITY_CASES[ci]
    T = make_table(n_rows, d, seed=ci)
    Q = T[make_query_rows(n_rows, min(n, 8), seed=ci)]
    cand = T[lo:lo + Cn]
    ratio = float((np.abs(emulated_logits(cand, Q).astype(np.float64) - reference_logits(cand, Q)) / E(cand, Q)).max())
    print(f"n_rows={n_rows} d={d}: max |x - x*| / E = {ratio:.3f}")
    assert ratio <= 1.0
    for dd in (1, 9, 100, 256):
        assert dd * U / (1 - dd * U) <= (dd + 2) * U          # gamma_d is covered


def test_the_f32_sigmoid_route_keeps_the_probability_bound_when_expf_is_exact_to_an_ulp():
    """1 / (1 + e) in f32 with e = exp(-x) rounded to f32 (half an ulp, inside the documented 1 ulp of expf): the relative error stays under P_BOUND"""
    x = np.linspace(-P_RANGE, P_RANGE, 200001).astype(np.float32)
    e = np.exp(-x.astype(np.float64)).astype(np.float32)
    p = (np.float32(1) / (np.float32(1) + e)).astype(np.float32)
    ref = sigmoid64(x)
    ratio = float((np.abs(p.astype(np.float64) - ref) / ref).max() / P_BOUND)
    print(f"max |p - p*| / p* / bound = {ratio:.3f}")
    assert ratio <= 1.0 and (np.diff(p) >= 0).all()
    assert 4 * U <= P_BOUND <= 40 * U          # a derived bound above a few tens of ulps would hold something other than rounding


# ------------------------------------------------------------------------------------------------------------------ Gnn.test's file plan, with a stub Link
class StubLink:
    """libntf.Link's surface, scoring in numpy: what Gnn.test asks of it is recorded"""
    made = []
    MAX_K = 2048

    def __init__(self, table, cand_lo, cand_hi, device=0):
        self.table, self.lo, self.hi, self.calls, self.closed = np.asarray(table, np.float32), int(cand_lo), int(cand_hi), [], False
        StubLink.made.append(self)

    def _logits(self, rows):
        return (self.table[np.asarray(rows)].astype(np.float64) @ self.table[self.lo:self.hi].astype(np.float64).T).astype(np.float32)

    def topk(self, rows=None, pooled=None, K=10, workspace_bytes=0, want_ms=False):
        assert pooled is None and not self.closed
        self.calls.append(("topk", np.asarray(rows).copy(), int(K)))
        x = self._logits(rows)
        idx = rank(x)[:, :K].astype(np.int32)
        xs = np.take_along_axis(x, idx.astype(np.int64), axis=1)
        return idx, xs, sigmoid64(xs).astype(np.float32)

    def dense(self, rows=None, pooled=None, workspace_bytes=0, want_ms=False, logit=True, prob=True):
        assert pooled is None and not self.closed
        self.calls.append(("dense", np.asarray(rows).copy(), None))
        x = self._logits(rows)
        return (x if logit else None), (sigmoid64(x).astype(np.float32) if prob else None)

    def close(self):
        self.closed = True


def plant_tables(tmp, method, tv, splits, d, seed=0, tables=None, epochs=()):
    """f{k}.pt (and f{k}.e{e}.pt) with this plugin's node-order marker for every fold of `splits`, then a Gnn whose learn() loaded them -> (gnn, {file name: table})"""
    from opentf_amd.mdl.emb.gnn import Gnn
    n_team, S = tv["skill"].shape
    M = tv["member"].shape[1]
    off = {"skill": 0, "member": S, "team": S + M} if method == "n2v" else {"member": 0, "skill": M, "team": M + S, "dummy": M + S + n_team}
    n = S + M + n_team + (method == "m2v")
    cfg = plugin_cfg(method)
    cfg[method]["d"] = d
    w = Gnn(str(tmp), "cuda:0", 0, cfg, method)
    w.output += w._dirname(); os.makedirs(w.output, exist_ok=True); w.offsets = off
    rng = np.random.default_rng(seed)
    files = {}
    for k in splits["folds"].keys():
        for name in [f"f{k}.pt"] + [f"f{k}.e{e}.pt" for e in epochs]:
            W = tables(off, n, name) if tables else rng.standard_normal((n, d)).astype(np.float32) * 0.5
            w._save(W, k, 0, 0.0, 0.0, f"{w.output}/{name}")
            files[name] = W
    g = Gnn(str(tmp), "cuda:0", 0, cfg, method)
    g.learn(tv, splits)
    return g, files, off


def _stub_toy():
    rng = np.random.default_rng(5)
    n_team, S, M = 14, 5, 2100
    skill = scipy.sparse.lil_matrix((n_team, S), dtype=np.uint8); member = scipy.sparse.lil_matrix((n_team, M), dtype=np.uint8)
    for t in range(n_team):
        skill[t, rng.choice(S, 2, replace=False)] = 1
        member[t, rng.choice(M, 3, replace=False)] = 1
    splits = {"test": np.array([1, 12, 5]), "folds": {0: {"train": np.array([0, 2, 3, 4]), "valid": np.array([6, 7])}, 1: {"train": np.array([6, 7, 8]), "valid": np.array([13, 9, 10, 11])}}}
    return {"skill": skill, "member": member, "loc": None}, splits, n_team, S, M


@pytest.mark.parametrize("method", ["n2v", "m2v"])
def test_gnn_test_file_plan_blocks_and_switch_with_a_stub_link(method, tmp_path, monkeypatch):
    from opentf_amd import libntf
    from opentf_amd.mdl.emb.gnn import Gnn
    tv, splits, n_team, S, M = _stub_toy()
    # before learn(): the RuntimeError of _node_emb, nothing touched
    monkeypatch.setattr(libntf, "Link", StubLink)
    with pytest.raises(RuntimeError, match="call learn"):
        Gnn(str(tmp_path / "x"), "cuda:0", 0, plugin_cfg(method), method).test(tv, splits, Cfg(topK=5))
    g, files, off = plant_tables(tmp_path, method, tv, splits, d=8, epochs=(0, 3, 11))
    m_lo, t_lo = (S, S + M) if method == "n2v" else (0, M + S)
    assert g.blocks["member"] == (m_lo, m_lo + M) and g.blocks["team"][0] == t_lo
    learned = g.model
    StubLink.made.clear()
    g.test(tv, splits, Cfg(topK=5, per_epoch=True, on_train=True))
    want_files = {f"f{k}.{s}.{e}pred" for k in (0, 1) for s in ("test", "train", "valid") for e in ("", "e0.", "e3.", "e11.")}
    assert {f for f in os.listdir(g.output) if f.endswith("pred")} == want_files
    assert g.model is learned                                    # get_dense_vecs still reads learn()'s table
    # one Link per loaded table, in Fnn.test's order, the member block as candidates; every earlier one closed
    order = [f"f{k}.{e}pt" for k in (0, 1) for e in ("", "e0.", "e3.", "e11.")]
    assert len(StubLink.made) == len(order) and all(l.closed for l in StubLink.made[:-1])
    for link, name in zip(StubLink.made, order):
        assert np.array_equal(link.table, files[name]) and (link.lo, link.hi) == (m_lo, m_lo + M)
        k = int(name[1])
        sets = [splits["test"], splits["folds"][k]["train"], splits["folds"][k]["valid"]]
        assert [c[0] for c in link.calls] == ["topk"] * 3 and [c[2] for c in link.calls] == [5] * 3
        for (_, rows, _), teams, s in zip(link.calls, sets, ("test", "train", "valid")):
            assert np.array_equal(rows, np.asarray(teams) + t_lo)          # team row = team block start + team id
            e = name[3:-2]
            pr = torch.load(f"{g.output}/f{k}.{s}.{e}pred", map_location="cpu", weights_only=False)
            assert list(pr.keys()) == ["y_pred", "uncertainty"] and pr["uncertainty"] is None
            y = pr["y_pred"]
            assert y.is_sparse and y.is_coalesced() and tuple(y.shape) == (len(teams), M) and y._nnz() == 5 * len(teams)
            x = files[name][np.asarray(teams) + t_lo].astype(np.float64) @ files[name][m_lo:m_lo + M].astype(np.float64).T      # member id = row - member block start
            ids = rank(x.astype(np.float32))[:, :5]
            dense = y.to_dense().numpy()
            assert np.array_equal(np.sort(y.indices().numpy()[1].reshape(len(teams), 5), axis=1), np.sort(ids, axis=1))
            assert np.array_equal(np.take_along_axis(dense, ids, axis=1), sigmoid64(np.take_along_axis(x.astype(np.float32), ids, axis=1)).astype(np.float32))
    # the switch: topK <= 2048 and < M on the device; above 2048 the dense entry and the host's top-K; topK >= M or None: dense files
    for topK, entry, sparse, nnz in [(2048, "topk", True, 2048), (2049, "dense", True, 2049), (M - 1, "dense", True, M - 1), (M, "dense", False, M), (M + 7, "dense", False, M),
                                     (None, "dense", False, M)]:
        StubLink.made.clear()
        g.test(tv, splits, Cfg(topK=topK, per_epoch=False, on_train=False))
        assert len(StubLink.made) == 2 and [c[0] for l in StubLink.made for c in l.calls] == [entry] * 2, topK
        y = torch.load(f"{g.output}/f1.test.pred", map_location="cpu", weights_only=False)["y_pred"]
        assert y.is_sparse == sparse and tuple(y.shape) == (3, M), topK
        assert (y._nnz() if sparse else y.numel()) == 3 * nnz
    g.close(); g.close()
    assert StubLink.made[-1].closed


def test_gnn_delegates_evaluate_and_adila_to_ntf():
    from opentf_amd.mdl.emb.gnn import Gnn
    from opentf_amd.mdl.fnn import Fnn
    from opentf_amd.mdl.ntf import Ntf, coo_from_topk, topk_sparse
    assert Gnn.evaluate is Ntf.evaluate and Gnn.adila is Ntf.adila and Gnn.is_bayesian is False
    assert Fnn._coo_from_topk is coo_from_topk and Fnn._topk_sparse is topk_sparse          # one helper, reached by both classes
    assert callable(Gnn.recommend) and callable(Gnn.close)
