"""ctypes callers of `ntf_roc_micro_dense` / `ntf_roc_micro_csr` (include/opentf_amd_roc.h) with sentinel-filled outputs, shared by tests/test_roc_host.py (the
refusals that return before any device call) and tests/test_gpu_roc.py.  No test in here."""
import ctypes as C

import numpy as np

EINVAL = -1
SENT_U, SENT_F, SENT_N = 7, -7.0, -7


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Curve:
    """the outputs of one call, sentinel-filled before it"""
    def __init__(self, cap):
        cap = max(int(cap), 1)
        self.fps, self.tps = np.full(cap, SENT_U, np.uint64), np.full(cap, SENT_U, np.uint64)
        self.thr = np.full(cap, SENT_F, np.float32)
        self.n, self.counts, self.auc = C.c_int64(SENT_N), np.full(3, SENT_U, np.uint64), C.c_double(SENT_F)

    def tail(self, chunk, cap, null):
        a = dict(fps=_p(self.fps), tps=_p(self.tps), thr=_p(self.thr), n=C.byref(self.n), counts=_p(self.counts), auc=C.byref(self.auc))
        for k in null:
            if k in a: a[k] = None
        return (int(chunk), int(cap), a["fps"], a["tps"], a["thr"], a["n"], a["counts"], a["auc"])

    def untouched(self):
        return ((self.fps == SENT_U).all() and (self.tps == SENT_U).all() and (self.thr == np.float32(SENT_F)).all() and self.n.value == SENT_N
                and (self.counts == SENT_U).all() and self.auc.value == SENT_F)

    def points(self):
        k = self.n.value
        assert 2 <= k <= len(self.fps)
        assert (self.fps[k:] == SENT_U).all() and (self.thr[k:] == np.float32(SENT_F)).all(), "written past n_points"
        return self.fps[:k].copy(), self.tps[:k].copy(), self.thr[:k].copy(), tuple(int(c) for c in self.counts), self.auc.value


def roc_dense(S, t_ip, t_ix, chunk=0, cap=None, null=(), rows=None):
    """-> (status, Curve) of ntf_roc_micro_dense; cap None: 2 P + 2"""
    from opentf_amd import libntf
    S = np.ascontiguousarray(S, dtype=np.float32)
    n, M = S.shape
    cap = 2 * len(t_ix) + 2 if cap is None else cap
    out = Curve(cap)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    rc = libntf.lib().ntf_roc_micro_dense(0, None if "scores" in null else _p(S), n, M, M, _p(t_ip), _p(t_ix), len(t_ip) - 1, _p(r), *out.tail(chunk, cap, null))
    return rc, out


def roc_csr(s_ip, s_ix, s_val, n, M, t_ip, t_ix, chunk=0, cap=None, null=()):
    """-> (status, Curve) of ntf_roc_micro_csr"""
    from opentf_amd import libntf
    s_ip = np.ascontiguousarray(s_ip, dtype=np.int64); s_ix = np.ascontiguousarray(s_ix, dtype=np.int32); s_val = np.ascontiguousarray(s_val, dtype=np.float32)
    cap = 2 * len(t_ix) + 2 if cap is None else cap
    out = Curve(cap)
    rc = libntf.lib().ntf_roc_micro_csr(0, _p(s_ip), _p(s_ix), _p(s_val), n, M, _p(t_ip), _p(t_ix), len(t_ip) - 1, None, *out.tail(chunk, cap, null))
    return rc, out
