"""metapath2vec producer, the parts that need no GPU: the reference restatement (tests/m2v_reference.py) on a graph whose walks are forced, the per-hop CSRs of
the plugin against scipy, the metapath parser, and the declaration / export / binding of ntf_m2v_create."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse
import torch

import m2v_reference as R
from conftest import ROOT, golden


class Cfg(dict):
    def __getattr__(self, k):
        if k.startswith("__"): raise AttributeError(k)
        return self.get(k)


L4 = [["member", "to", "team"], ["team", "rev_to", "skill"], ["skill", "to", "team"], ["team", "rev_to", "member"]]


def _cfg(metapath_name, wl=5):
    return Cfg(graph=Cfg(structure=[[["skill", "to", "team"], ["member", "to", "team"]], "stm"], dup_edge="add", pre=None),
               m2v=Cfg(d=16, w=3, e=4, b=16, lr=0.01, es=5, ns=2, spe=2, wl=wl, wn=3, metapath_name=metapath_name))


def _toy():
    toy = golden("toy_dblp")
    n, S, M = [int(v) for v in toy["shape"]]
    skill = scipy.sparse.csr_matrix((np.ones(len(toy["skill_indices"]), np.uint8), toy["skill_indices"], toy["skill_indptr"]), shape=(n, S))
    member = scipy.sparse.csr_matrix((np.ones(len(toy["member_indices"]), np.uint8), toy["member_indices"], toy["member_indptr"]), shape=(n, M))
    return toy, skill, member, n, S, M


# ---------------------------------------------------------------------------------------------------------------- forced walks
@pytest.mark.parametrize("name,metapath", [("mtm", R.MTM), ("mtstm", R.MTSTM)])
def test_forced_walks_are_the_hand_written_rows(name, metapath):
    """every node has at most one neighbour per hop, so the draws cannot matter: both restatements must give the rows written out from the semantics"""
    path = R.forced(metapath)
    if name == "mtm": assert path.types == ["member", "team"] and path.start.tolist() == [0, 4, 7] and path.total == 7      # only the types the metapath names
    else: assert path.types == ["member", "skill", "team"] and path.start.tolist() == [0, 4, 6, 9] and path.total == 9
    want = R.FORCED_WALKS[name]
    batch = np.arange(4)
    for seed in (0, 1):
        got = R.pos_sample(path, batch, 4, 3, 2, torch.Generator().manual_seed(seed), as_walks=True).numpy()
        assert np.array_equal(got, np.tile(want, (2, 1)))                                   # batch.repeat(walks_per_node): row r starts at batch[r % B]
        assert np.array_equal(R.replay_walks(path, batch, 8, 5, seed, 3), np.tile(want, (2, 1)))
    if name == "mtm":
        win = R.pos_sample(path, batch, 4, 3, 1, torch.Generator().manual_seed(0)).numpy()
        assert np.array_equal(win, R.FORCED_WINDOWS_MTM) and np.array_equal(R.windows(R.replay_walks(path, batch, 4, 5, 0, 0), 3), R.FORCED_WINDOWS_MTM)
        assert (R.FORCED_WINDOWS_MTM[:, 0] == path.total).sum() == 3                         # windows that START at the dummy exist


def test_a_walk_past_a_metapath_that_is_no_cycle_is_refused():
    path = R.forced(R.STM)
    assert not path.cycle and path.L == 2
    R.pos_sample(path, np.arange(2), 2, 3, 1, torch.Generator().manual_seed(0))
    with pytest.raises(AssertionError): R.pos_sample(path, np.arange(2), 3, 3, 1, torch.Generator().manual_seed(0))


def test_negatives_stay_inside_their_type_and_never_name_the_dummy():
    path = R.forced(R.MTSTM)
    for rw in (R.neg_sample(path, np.arange(4), 8, 3, 3, 2, torch.Generator().manual_seed(0), as_walks=True).numpy(), R.replay_negs(path, np.arange(4), 24, 9, 5, 2)):
        assert rw.shape == (24, 9) and np.array_equal(rw[:, 0], np.tile(np.arange(4), 6))
        for p in range(1, 9):
            t = path.position_type(p)
            assert t == [0, 2, 1, 2, 0, 2, 1, 2, 0][p]
            assert (rw[:, p] >= path.start[t]).all() and (rw[:, p] < path.start[t + 1]).all()
        assert (rw < path.total).all()
        assert len(np.unique(rw[:, 1])) == 3                                                  # all three teams are drawn in 24 rows


# ---------------------------------------------------------------------------------------------------------------- hop CSRs
def test_hop_csrs_match_scipy_on_toy_dblp_with_dropped_teams():
    from opentf_amd.mdl.emb.gnn import M2V_ORDER, M2V_TYPES, m2v_graph
    toy, skill, member, n, S, M = _toy()
    drop = np.concatenate([toy["test"], toy["valid0"]])
    counts, off, hops = m2v_graph(skill.tolil(), member.tolil(), drop, [tuple(h) for h in L4])
    assert list(M2V_TYPES) == sorted(M2V_TYPES) and M2V_ORDER == "member|skill|team|dummy"
    assert counts == [M, S, n] and off == {"member": 0, "skill": M, "team": M + S, "dummy": M + S + n}
    kept = member.toarray().astype(bool); kept[drop] = False
    dense = {(0, 2): kept.T, (2, 1): skill.toarray().astype(bool), (1, 2): skill.toarray().astype(bool).T, (2, 0): kept}
    assert [(s, d) for s, d, _, _ in hops] == [(0, 2), (2, 1), (1, 2), (2, 0)]
    for s, d, rp, col in hops:
        A = dense[(s, d)]
        assert rp.dtype == np.int64 and col.dtype == np.int32 and len(rp) == counts[s] + 1 and rp[0] == 0 and rp[-1] == len(col) == A.sum()
        got = scipy.sparse.csr_matrix((np.ones(len(col), bool), col, rp), shape=(counts[s], counts[d])).toarray()
        assert np.array_equal(got, A)
        assert all((np.diff(col[rp[i]:rp[i + 1]]) > 0).all() for i in range(counts[s]))          # sorted, no duplicate
    assert not np.diff(hops[3][2])[drop].any() and np.diff(hops[3][2]).any()                      # the dropped teams have no member edge left
    # the reference module builds the same CSRs and the same layout
    csrs = R.hop_csrs(skill, member, drop)
    path = R.Path({"member": M, "skill": S, "team": n}, [tuple(h) for h in L4], csrs)
    assert path.types == list(M2V_TYPES) and path.start.tolist() == [0, M, M + S, M + S + n] and path.total == off["dummy"]
    for (s, d, rp, col), (s2, d2, rp2, col2) in zip(hops, path.hops):
        assert (s, d) == (s2, d2) and np.array_equal(rp, rp2) and np.array_equal(col, col2)


# ---------------------------------------------------------------------------------------------------------------- the metapath parser
def test_metapath_parses_both_config_shapes():
    from opentf_amd.mdl.emb.gnn import _metapath
    want = [tuple(h) for h in L4]
    assert _metapath(_cfg([L4, "mtstm"])) == (want, "mtstm")
    assert _metapath(_cfg(L4)) == (want, None)
    assert _metapath(_cfg([[["skill", "to", "team"], ["team", "rev_to", "member"]], "stm"])) == ([("skill", "to", "team"), ("team", "rev_to", "member")], "stm")
    two = [["member", "to", "team"], ["team", "rev_to", "skill"]]               # a bare list of exactly two triples is not mistaken for [path, label]
    with pytest.raises(ValueError, match="chain|visit"): _metapath(_cfg([two[0], two[0]]))
    assert _metapath(_cfg(two))[1] is None


@pytest.mark.parametrize("bad,exc", [
    ([["member", "to", "team"], ["skill", "to", "team"], ["team", "rev_to", "member"]], ValueError),                # broken chain
    ([["member", "to", "team"], ["team", "rev_to", "loc"], ["loc", "to", "team"], ["team", "rev_to", "skill"]], NotImplementedError),   # a type not built here
    ([["member", "to", "team"], ["team", "rev_to", "venue"]], NotImplementedError),                                # unknown type
    ([["member", "to", "team"], ["team", "rev_to", "member"]], ValueError),                                        # skill missing
    ([["member", "cites", "team"], ["team", "rev_to", "skill"]], NotImplementedError),                             # unknown relation
    ([["member", "to", "skill"], ["skill", "to", "team"]], NotImplementedError),                                   # no such edges in stm
    (None, ValueError), ("mtstm", ValueError), ([["member", "team"]], ValueError)])
def test_metapath_refusals(bad, exc, tmp_path):
    from opentf_amd.mdl.emb.gnn import Gnn, _metapath
    with pytest.raises(exc): _metapath(_cfg(bad))
    with pytest.raises(exc): Gnn(str(tmp_path), "cpu", 0, _cfg(bad), "m2v")          # the constructor refuses before any device call


def test_gnn_constructs_for_m2v_and_still_refuses_the_message_passing_models(tmp_path):
    from opentf_amd.mdl.emb.gnn import Gnn
    t = Gnn(str(tmp_path), "cpu", 0, _cfg([L4, "mtstm"]), "m2v")
    assert t.metapath == [tuple(h) for h in L4] and t.metapath_label == "mtstm"
    assert t._dirname() == "/m2v.b16.e4.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl5.wn3.mtstm"
    assert Gnn(str(tmp_path), "cpu", 0, _cfg(L4), "m2v")._dirname() == "/m2v.b16.e4.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl5.wn3"
    for name in ("gcn", "gs", "gat"):
        with pytest.raises(NotImplementedError): Gnn(str(tmp_path), "cpu", 0, _cfg(L4), name)
    stm = [["skill", "to", "team"], ["team", "rev_to", "member"]]                  # not a cycle: wl steps may not outrun it
    Gnn(str(tmp_path), "cpu", 0, _cfg(stm, wl=2), "m2v")
    with pytest.raises(ValueError, match="outrun"): Gnn(str(tmp_path), "cpu", 0, _cfg(stm, wl=3), "m2v")


# ---------------------------------------------------------------------------------------------------------------- declaration, export, binding
def test_m2v_create_is_declared_exported_and_bound():
    from opentf_amd import libntf
    src = open(os.path.join(ROOT, "include", "opentf_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ntf_m2v_create\s*\(", code)
    assert re.search(r"#define\s+NTF_M2V_MAX_TYPES\s+8\b", code) and re.search(r"#define\s+NTF_M2V_MAX_HOPS\s+8\b", code)
    path = os.path.join(ROOT, "opentf_amd", "libopentf_amd.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(path), "ntf_m2v_create")
    assert "ntf_m2v_create" in libntf.SYMBOLS and libntf.lib().ntf_m2v_create.restype is ctypes.c_int
    assert issubclass(libntf.MetaPath2Vec, libntf.Node2Vec) and libntf.MetaPath2Vec._CREATE == "ntf_m2v_create"
    # the constructor's own checks need no device
    with pytest.raises(libntf.NtfError, match="dummy row"):
        libntf.MetaPath2Vec([4, 2, 3], [(0, 2, *R.FORCED_CSRS[("member", "team")])], np.zeros((9, 8), np.float32))
    with pytest.raises(libntf.NtfError, match="rowptr"):
        libntf.MetaPath2Vec([4, 2, 3], [(1, 2, *R.FORCED_CSRS[("member", "team")])], np.zeros((10, 8), np.float32))
