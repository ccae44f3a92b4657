"""The host side of node2vec's walk bias without a GPU: the thresholds, the replay of tests/n2v_bias_reference.py against the exact transition probabilities (with the
rejection stage at 16, 2 and 0 attempts - the last is the scan alone), entry multiplicity, the test graphs, and the plugin's directory name."""
import ctypes

import numpy as np
import pytest
from scipy.stats import chi2

import n2v_bias_reference as R
from n2v_reference import plugin_cfg as _cfg


def test_thresholds():
    assert R.thresholds(1, 1) == [2 ** 32] * 3
    assert R.thresholds(4, 1) == [2 ** 30, 2 ** 32, 2 ** 32]
    assert R.thresholds(0.25, 4) == [2 ** 32, 2 ** 30, 2 ** 28]
    for p, q in R.SETTINGS + [(1e-4, 1e4), (1e4, 1e-4), (1e4, 1e4), (1e-4, 1e-4)]:
        thr = R.thresholds(p, q)
        assert all(1 <= t <= 2 ** 32 for t in thr) and max(thr) == 2 ** 32, (p, q, thr)


def test_the_graphs_are_what_they_say():
    rp, col = R.g24()
    assert np.diff(rp).tolist() == R.G24_DEGREES and all((np.diff(col[rp[i]:rp[i + 1]]) > 0).all() for i in range(24))
    rp, col = R.h301()
    deg = np.diff(rp)
    assert deg[0] == 300 and -(-300 // 64) == 5 and 300 % 64 != 0 and sorted(set(deg[1:].tolist())) == [1, 2]
    rp, col = R.d4()
    assert col[rp[0]:rp[1]].tolist() == [1, 1, 2, 3] and col[rp[1]:rp[2]].tolist() == [0, 0, 2]


@pytest.mark.parametrize("p,q,tries", [(0.25, 4, 16), (8, 8, 2), (0.5, 8, 0)])
def test_the_replay_samples_the_exact_pair_distribution(p, q, tries):
    """40 000 walks of 3 nodes from the hub of G24 (seed 11, step 3): Pearson's chi-square of the (position 1, position 2) counts against `exact_pairs`, no cell left out"""
    rp, col = R.g24()
    stats = {}
    rw = R.replay_biased_walks(rp, col, np.zeros(1, np.int64), 40000, 3, 11, 3, p, q, tries=tries, stats=stats)
    P = R.exact_pairs(rp, col, 0, p, q)
    assert abs(P.sum() - 1.0) < 1e-12
    stat, cells, left = R.chi_square(rw, P, min_expected=0.0)
    bar = float(chi2.isf(1e-6, cells - 1))
    print(f"n2v bias reference (p, q) = ({p}, {q}), {tries} tries: chi-square {stat:.1f} over {cells} cells, bar {bar:.1f}; {stats['scans']} scans of {stats['biased_steps']} biased steps")
    assert stat <= bar
    if tries == 0: assert stats["scans"] == stats["biased_steps"] > 30000


@pytest.mark.parametrize("tries", [16, 0])
def test_a_doubled_entry_is_drawn_twice_as_often(tries):
    """D4 from the leaf 3 with (p, q) = (2, 4): the walk 3 -> 0 -> x over row(0) = [1, 1, 2, 3] with t = 3.  Neither 1 nor 2 has 3 in its row (class 2, 1 / 4
    an entry), 3 returns (1 / 2): P(x = 1) = 0.4 over its two entries, P(x = 2) = 0.2, P(x = 3) = 0.4"""
    rp, col = R.d4()
    P = R.exact_pairs(rp, col, 3, 2, 4)
    assert np.allclose(P[0, 1:], [0.4, 0.2, 0.4], rtol=1e-12) and P[0, 1] == 2 * P[0, 2] and abs(P.sum() - 1) < 1e-12
    rw = R.replay_biased_walks(rp, col, np.array([3], np.int64), 40000, 3, 11, 3, 2, 4, tries=tries)
    stat, cells, left = R.chi_square(rw, P, min_expected=0.0)
    bar = float(chi2.isf(1e-6, cells - 1))
    n1, n2 = int((rw[:, 2] == 1).sum()), int((rw[:, 2] == 2).sum())
    print(f"n2v bias D4, {tries} tries: chi-square {stat:.1f} over {cells} cells, bar {bar:.1f}; the doubled entry's node drawn {n1} times, the single one's {n2}")
    assert stat <= bar


def test_p_q_one_is_the_uniform_distribution_over_entries():
    rp, col = R.g24()
    P = R.exact_pairs(rp, col, 0, 1, 1)
    for x1 in col[rp[0]:rp[1]]:
        row = col[rp[x1]:rp[x1 + 1]]
        assert np.allclose(P[x1, row], 1.0 / 14 / len(row))


def test_the_directory_name_takes_the_bias_only_when_it_is_not_one(tmp_path):
    from opentf_amd.mdl.emb.gnn import Gnn
    plain = "/n2v.b16.e4.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl5.wn3"
    name = lambda **kw: Gnn(str(tmp_path), "cpu", 0, _cfg("n2v", **kw), "n2v")._dirname()
    assert name() == plain and name(p=1, q=1) == plain and name(p=1.0) == plain and name(q=1.0, sparse=False) == plain
    assert name(p=0.5, q=2) == plain + ".p0.5.q2.0"
    assert name(p=0.5, q=2.0, sparse=True) == plain + ".p0.5.q2.0.sparse"
    assert name(q=4) == plain + ".p1.0.q4.0" and name(p=0.25) == plain + ".p0.25.q1.0"
    assert name(sparse=True) == plain + ".sparse"


def test_m2v_ignores_the_keys(tmp_path):
    from opentf_amd.mdl.emb.gnn import Gnn
    plain = "/m2v.b16.e4.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl5.wn3.mtstm"
    t2v = Gnn(str(tmp_path), "cpu", 0, _cfg("m2v", p=0.5, q=2.0), "m2v")
    assert t2v._dirname() == plain and t2v._bias() == (1.0, 1.0)


def test_the_entry_is_declared_and_bound():
    import inspect
    from opentf_amd import libntf
    assert libntf.SYMBOLS["ntf_n2v_set_walk_bias"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double])
    sig = inspect.signature(libntf.Node2Vec.__init__).parameters
    assert sig["p"].default == 1.0 and sig["q"].default == 1.0
    assert "p" not in inspect.signature(libntf.MetaPath2Vec.__init__).parameters
