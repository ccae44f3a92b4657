"""The doc2vec kernels (opentf_amd/csrc/ntf_d2v.hip k_d2v_epoch, k_d2v_infer) against tests/d2v_reference.py off the one operating point of test_gpu_d2v.py and
test_gpu_d2v_infer.py (window 5, negative 5 / 1 / 3, vocabularies below 1 024 words): other windows and negatives, 129 <= d <= 192, the plain PV-DM branch at
d >= 128, both arms of NTF_D2V_DEFER, the deferred kernel's duplicate rule and its reach, a cumulative table with more than one entry a bucket, the accepted limits
of the window, the refusals of ntf_d2v_train_epoch.  Cases, seeds and the conditions they meet before a device sees them: tests/d2v_reference.py and
tests/test_d2v_paths_host.py.  Every trainer pass is a one-wave launch (`serial`); each test prints its largest |device - reference| / bar (pytest -s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import d2v_reference as R                               # noqa: E402
from opentf_amd import libntf                           # noqa: E402
from test_gpu_d2v_infer import _check_parity, _net      # noqa: E402


def _open(c):
    net = libntf.Doc2Vec(c["ptr"], c["wi"], c["si"], c["cum"], c["wv0"], c["dv0"], seed=c["seed"])
    net.set_vectors(net.SYN1NEG, c["s10"])
    return net


def _pass(c, net=None):
    """one serial pass of the case on the device -> (dv, wv, syn1neg), mean loss"""
    own = net or _open(c)
    loss, _ = own.train_epoch(c["dm"], c["window"], R.ALPHA0, R.ALPHA1, 0, negative=c["negative"], serial=True, want_loss=True)
    got = [own.vectors(w) for w in (own.DV, own.WV, own.SYN1NEG)]
    if net is None: own.close()
    return got, loss


def _check(c, got, loss, tag=""):
    ratios = R.distance(c, got)
    print(f"\n{c['name']}{tag}: max|device - ref| / bar (dv, wv, syn1neg) {[f'{x:.3f}' for x in ratios]}, flagged units {c['stats']['flagged']}, loss {loss:.6f} / ref {c['stats']['loss']:.6f}")
    assert all(g.dtype == np.float32 and np.isfinite(g).all() for g in got)
    assert max(ratios) <= 1, ratios
    assert abs(loss - c["stats"]["loss"]) <= 1e-3 * c["stats"]["loss"], (loss, c["stats"]["loss"])


@pytest.mark.parametrize("name", [n for n in R.TRAIN_SPECS if n[0] in "ACDE"])
def test_one_wave_pass_equals_the_reference(name):
    """A: windows 1 to 10 and negatives 0 to 8, NV = 1 to 4 (PV-DM at d >= 128: the plain branch at NV >= 2); C: the deferred kernel deferring up to the first word
    its reach holds twice (period 11: to the end); D: bucket sizes 2 and 3 of the table search; E: windows 255 (PV-DM) and 127 (PV-DBOW: unit index 254)"""
    c = R.train_case(name)
    _check(c, *_pass(c))


@pytest.mark.parametrize("d", [128, 192, 256])
def test_both_arms_of_the_switch_at_window_five(d, monkeypatch):
    c = R.train_case(f"B-d{d}")
    monkeypatch.delenv("NTF_D2V_DEFER", raising=False)
    deferred, l_d = _pass(c)
    monkeypatch.setenv("NTF_D2V_DEFER", "0")                               # read per call: the plain kernel from here on
    plain, l_p = _pass(c)
    _check(c, deferred, l_d, " deferred")
    _check(c, plain, l_p, " plain")
    apart = [float(np.abs(a.astype(np.float64) - b).max()) / bar for a, b, bar in zip(deferred, plain, R.train_bars(c))]
    print(f"the two arms: {[f'{x:.3f}' for x in apart]} bars apart")
    assert max(apart) <= 2, apart
    assert not all(np.array_equal(a, b) for a, b in zip(deferred, plain))  # two orders of the same additions: were they bit-equal, the switch would not have switched


REFUSED = [("window outside", dict(window=0)), ("window outside", dict(window=256)), ("window outside", dict(dm=0, window=128)), ("negative outside", dict(negative=-1)),
           ("negative outside", dict(negative=9)), ("dm is 0 or 1", dict(dm=2)), ("order is not", dict(order="repeat")), ("progress outside", dict(progress=1.5)),
           ("progress outside", dict(progress=float("nan")))]


def test_refused_passes_name_the_argument_and_leave_the_tables_alone():
    c = R.train_case("A-dm1-w2-n4-d128")
    net = _open(c)
    n = len(c["ptr"]) - 1
    before = [net.vectors(w) for w in (0, 1, 2)]
    assert all(np.array_equal(b, c[t]) for b, t in zip(before, ("dv0", "wv0", "s10")))
    for word, kw in REFUSED:
        a = dict(dm=1, window=2, negative=4, order=None, progress=None); a.update(kw)
        if a["order"] == "repeat": a["order"] = np.concatenate([[1], np.arange(1, n)])
        if a["progress"] is not None: a["progress"] = np.concatenate([np.zeros(n - 1), [a["progress"]]])
        with pytest.raises(libntf.NtfError, match=word):
            net.train_epoch(a["dm"], a["window"], R.ALPHA0, R.ALPHA1, 0, negative=a["negative"], serial=True, order=a["order"], progress=a["progress"], want_loss=True)
        for w in (0, 1, 2): assert np.array_equal(net.vectors(w), before[w]), (kw, w)
    assert libntf.lib().ntf_d2v_train_epoch(None, 1, 2, 4, R.ALPHA0, R.ALPHA1, 0, 1, None, None, None, None) == libntf.NTF_EINVAL
    assert b"handle" in libntf.lib().ntf_d2v_last_error(None)
    _check(c, *_pass(c, net), " after the refusals")                       # the handle is as good as new
    net.close()


@pytest.mark.parametrize("name", list(R.INFER_SPECS))
def test_infer_equals_the_reference(name):
    """windows 1, 2, 10 and negatives 0, 4, 8 at NV = 1 to 4; d2v_table_search inside buckets of 3; one 600-word query at window 255"""
    c = R.infer_case(name)
    net = _net(c)
    got = net.infer(c["q_ptr"], c["q_words"], c["init"], c["dm"], c["window"], c["epochs"], R.I_ALPHA, R.I_MIN_ALPHA, c["seed"], negative=c["negative"], ids=c["ids"])
    net.close()
    step = 2 * 0.003 * R.I_ALPHA * float(np.abs(c["s1"]).max())             # _check_parity's bound, for the one figure DESIGN.md records
    bound = 2e-5 * np.abs(c["ref"]).max(axis=1) + 1e-9 + step * c["flagged"]
    print(f"\n{name}: max|device - ref| / bound over the queries {float((np.abs(got.astype(np.float64) - c['ref']).max(axis=1) / bound).max()):.3f}")
    if len(c["ref"]) == 48: assert np.array_equal(got[0], c["init"][0])    # the empty query: its initial row, bit for bit
    _check_parity(got, c, alpha=R.I_ALPHA)
