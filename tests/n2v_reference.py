"""What the test files of the node2vec / metapath2vec producers share and none of them owns: the config stand-in of the plugin tests and its n2v / m2v
sections, toy dblp as the plugins take it, the uint32 view, the bar of test_adam_over_steps_that_name_different_rows for the opt-in optimisers, a handle on
`P.graph()`, and the fixture that leaves the global generators as it found them.  The float64 references stay where they are (tests/test_gpu_n2v_parity.py and
the optimisers' own files).  Needs no GPU until `net` is called.  TEST INFRASTRUCTURE ONLY.

`global_generators_left_as_found` is an autouse fixture that works ONLY in a module that imports it BY NAME (pytest collects the fixtures it finds in a test
module's namespace): the import looks unused and is not.  Removing it from a host file removes that file's restore of the torch / numpy / random generators
without any test failing.
"""
import numpy as np
import pytest
import scipy.sparse
import torch


class Cfg(dict):
    def __getattr__(self, k):
        if k.startswith("__"): raise AttributeError(k)
        return self.get(k)


def plugin_cfg(method, **kw):
    """the config of a Gnn plugin (`n2v` or `m2v`) on toy dblp with `kw` added to the method's section"""
    sec = Cfg(d=16, w=3, e=4, b=16, lr=0.01, es=5, ns=2, spe=2, wl=5, wn=3, **kw)
    if method == "m2v":
        sec["metapath_name"] = [[["member", "to", "team"], ["team", "rev_to", "skill"], ["skill", "to", "team"], ["team", "rev_to", "member"]], "mtstm"]
    return Cfg(graph=Cfg(structure=[[["skill", "to", "team"], ["member", "to", "team"]], "stm"], dup_edge="add", pre=None), **{method: sec})


def toy_dblp():
    """-> the golden file, teamsvecs, splits, n, S, M"""
    from conftest import golden
    toy = golden("toy_dblp")
    n, S, M = [int(v) for v in toy["shape"]]
    skill = scipy.sparse.csr_matrix((np.ones(len(toy["skill_indices"]), np.uint8), toy["skill_indices"], toy["skill_indptr"]), shape=(n, S)).tolil()
    member = scipy.sparse.csr_matrix((np.ones(len(toy["member_indices"]), np.uint8), toy["member_indices"], toy["member_indptr"]), shape=(n, M)).tolil()
    splits = {"test": toy["test"], "folds": {k: {"train": toy[f"train{k}"], "valid": toy[f"valid{k}"]} for k in range(3)}}
    return toy, {"skill": skill, "member": member, "loc": None}, splits, n, S, M


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def within_bar(what, Wd, Wref, compare, tag):
    """the bar of test_adam_over_steps_that_name_different_rows on the compared elements; prints the largest err / tol (`what`: the optimiser, for the line)"""
    err = np.abs(Wd.astype(np.float64) - Wref); tol = 2e-5 + 1e-4 * np.abs(Wref)
    worst = float((err / tol)[compare].max()) if compare.any() else 0.0
    print(f"n2v {what} adam {tag}: max |W - ref| / tol over the compared elements {worst:.3f}, left out {int((~compare).sum())} of {compare.size}")
    assert (err <= tol)[compare].all(), (tag, worst)
    return worst


def net(W, seed=0, **kw):
    """a Node2Vec handle over the table W on the graph of tests/test_gpu_n2v_parity.py; kw: sparse, lazy, p, q"""
    import test_gpu_n2v_parity as P
    from opentf_amd.libntf import Node2Vec
    rp, col, nn, _ = P.graph()
    return Node2Vec(rp, col, W, seed=seed, **kw)


@pytest.fixture(autouse=True)       # of the module that imports it by name
def global_generators_left_as_found():
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)
