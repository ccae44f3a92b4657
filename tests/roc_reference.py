"""The micro ROC curve's contract (include/opentf_amd_roc.h) restated as plain sequential numpy: a stable sort of all n * M (score, label) pairs, then a walk
over the distinct scores from the highest down.  The pin of ntf_roc_micro_dense / ntf_roc_micro_csr and of `micro_roc_device`; tests/test_roc_host.py checks it
against sklearn, tests/test_gpu_roc.py the device against it, bit for bit.  No device, no library."""
import numpy as np
import scipy.sparse as sp


def dense_pair(Y, Y_):
    """(labels [n * M] bool, scores [n * M] f32) of a truth matrix and a prediction, either one dense or scipy sparse (unstored: 0)"""
    y = (Y.toarray() if sp.issparse(Y) else np.asarray(Y)) != 0
    s = Y_.toarray() if sp.issparse(Y_) else np.asarray(Y_)
    assert y.shape == s.shape
    return y.ravel(), np.ascontiguousarray(s, dtype=np.float32).ravel()


def roc_points(labels, scores):
    """-> (fps uint64, tps uint64, thresholds f32, (P, N, U2), G).  Scores compare as real numbers: -0.0 is +0.0, denormals are distinct."""
    labels = np.asarray(labels, dtype=bool).ravel()
    s = np.asarray(scores, dtype=np.float32).ravel()
    assert not np.isnan(s).any()
    s = np.where(s == 0, np.float32(0.0), s)                      # either zero -> +0.0f
    order = np.argsort(s, kind="stable")
    s, labels = s[order], labels[order]
    # runs of equal scores, ascending
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    end = np.concatenate([start[1:], [len(s)]])
    pos = np.add.reduceat(labels.astype(np.int64), start)
    neg = (end - start) - pos
    vals = s[start]
    P, N = int(pos.sum()), int(neg.sum())
    fps, tps, thr = [0], [0], [np.float32(np.inf)]
    f = t = 0
    gap = 0                  # negatives of the current gap that are not emitted yet
    gap_min = None           # its smallest score: the walk descends, so the last one seen
    u2 = 0
    for r in range(len(vals) - 1, -1, -1):
        if pos[r] == 0:
            gap += int(neg[r]); gap_min = vals[r]
            continue
        if gap:
            f += gap; fps.append(f); tps.append(t); thr.append(gap_min); gap = 0
        f += int(neg[r]); t += int(pos[r])
        fps.append(f); tps.append(t); thr.append(vals[r])
    if gap:
        f += gap; fps.append(f); tps.append(t); thr.append(gap_min)
    below = 0
    for r in range(len(vals)):
        u2 += int(pos[r]) * (2 * below + int(neg[r])); below += int(neg[r])
    assert (f, t) == (N, P)
    return (np.array(fps, dtype=np.uint64), np.array(tps, dtype=np.uint64), np.array(thr, dtype=np.float32), (P, N, u2), int((pos > 0).sum()))


def roc_reference(Y, Y_):
    return roc_points(*dense_pair(Y, Y_))


def doubled_trapezoid(fps, tps):
    f = [int(x) for x in fps]; t = [int(x) for x in tps]
    return sum((f[a + 1] - f[a]) * (t[a + 1] + t[a]) for a in range(len(f) - 1))
