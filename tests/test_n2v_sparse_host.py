"""The host side of test_gpu_n2v_sparse.py without a GPU: its float64 reference against torch.optim.SparseAdam itself, every condition the GPU tests put on
their inputs, the proof that those inputs tell sparse Adam from dense Adam, and the plugin's directory name."""
import numpy as np
import pytest
import torch

import test_gpu_n2v_parity as P
import test_gpu_n2v_sparse as S
from n2v_reference import global_generators_left_as_found, plugin_cfg as _cfg      # the fixture: autouse


def test_the_reference_is_torch_sparse_adam_in_float64():
    """torch.optim.SparseAdam on a float64 parameter, fed per step the reference's own gradient as a coalesced sparse_coo_tensor over the rows the step names"""
    d = 192
    W0 = P.table(d)
    W, m, v, refs, compare, named = S.five_steps(d)
    p = torch.nn.Parameter(torch.from_numpy(W0.astype(np.float64)))
    opt = torch.optim.SparseAdam([p], lr=S.LR, betas=(S.B1, S.B2), eps=S.EPS)
    for ref in refs:
        rows = np.flatnonzero(ref["K"] > 0)
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(rows)[None], torch.from_numpy(ref["grad"][rows]), size=p.shape).coalesce()
        opt.step()
    st = opt.state[p]
    diffs = [float(np.abs(p.detach().numpy() - W).max()), float(np.abs(st["exp_avg"].numpy() - m).max()), float(np.abs(st["exp_avg_sq"].numpy() - v).max())]
    print(f"sparse_adam_reference against torch.optim.SparseAdam (float64, five steps): largest differences W {diffs[0]:.2e}, m {diffs[1]:.2e}, v {diffs[2]:.2e}")
    assert max(diffs) <= 1e-12 and int(st["step"]) == 5


@pytest.mark.parametrize("d", S.SIZES)
def test_the_share_of_left_out_elements_stays_under_its_cap(d):
    W, m, v, refs, compare, named = S.five_steps(d)
    print(f"sparse reference d={d}: {(~compare).mean():.2e} of the elements left out")
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs)


def test_the_inputs_tell_sparse_adam_from_dense_adam():
    d = 192
    W0 = P.table(d)
    sets = P.adam_window_sets()
    W, m, v, refs, compare, named = S.five_steps(d)
    K = np.stack([r["K"] > 0 for r in refs])
    assert (~named).sum() == 37 and np.array_equal(named, K.any(0))
    assert (K.any(0) & ~K.all(0)).sum() == 499                                   # named in some steps and not in others
    drops = [int((K[t] & ~K[t + 1]).sum()) for t in range(4)]
    assert all(125 <= x <= 134 for x in drops), drops                            # named in step t and not in step t + 1: dense Adam moves them in t + 1
    Wdense, _, cmp_dense, _ = P.adam_reference(W0, sets)
    both = compare & cmp_dense
    apart = np.abs(Wdense - W) > 4 * (2e-5 + 1e-4 * np.abs(W))
    print(f"dense against sparse Adam, float64, d={d}: {apart[both].mean():.3f} of the compared elements more than 4 tol apart")
    assert apart[both].mean() > 0.5
    # rows the windows never name separate them too: both references leave them alone
    assert np.array_equal(Wdense[~named], W0[~named].astype(np.float64)) and np.array_equal(W[~named], W0[~named].astype(np.float64)) and not m[~named].any()


def test_the_zero_gradient_scenario_is_what_it_says():
    W0, steps, a, z = S.zero_gradient_case()
    assert not W0[z].any() and W0[a].all()
    W, m, v, refs, compare, named = S.sparse_adam_reference(W0, steps)
    assert all(P.conditions_hold(r) for r in refs)
    assert refs[0]["K"][a] > 0 and refs[0]["K"][z] == 0 and np.abs(refs[0]["grad"][a]).min() > 0
    assert refs[1]["K"][a] == 2 and (refs[1]["grad"][a] == 0.0).all()            # touched, and a summed gradient of exactly 0.0 ...
    W1, m1, v1, _, _, _ = S.sparse_adam_reference(W0, steps[:1])
    assert (W[a] != W1[a]).all() and np.allclose(m[a], 0.9 * m1[a], rtol=1e-15, atol=0)      # ... and the row still moves, on decayed moments


def test_the_hub_and_boundary_cases_are_what_they_say():
    pos, neg, hub = S.hub_case()
    ref = P.ref_batch(P.table(192), pos, neg)
    assert P.conditions_hold(ref) and ref["K"][hub] == 400 and (pos[0, 0] == pos[0, 2]) and not (neg[:, 1:] == neg[:, :1]).any()
    W0, bp, bn = S.boundary_case()
    assert W0.shape == (S.BOUNDARY_N, 1) and sorted(set(bp.ravel()) | set(bn.ravel())) == S.BOUNDARY_ROWS
    assert {0, 31, 32, 63, 64, 8191, 8192, 69998, 69999} <= set(S.BOUNDARY_ROWS)
    W, m, v, refs, compare, named = S.sparse_adam_reference(W0, [(bp, bn)])
    assert compare[named].all()


def test_the_metapath_case_names_the_dummy_row_and_meets_its_conditions():
    import test_gpu_m2v as M
    p = M.path(M.NATIVE_PATH)
    sets = [M.replay_step(t, steps=M.ADAM_STEPS)[2:] for t in range(len(M.ADAM_STEPS))]      # few negatives: some rows are named in no step
    W, m, v, refs, compare, named = S.sparse_adam_reference(M.table(M.NATIVE_PATH, 129), sets)
    assert (~compare).mean() <= 1e-3 and all(P.conditions_hold(r) for r in refs) and all(r["K"][p.total] > 0 for r in refs)
    assert (~named).sum() >= 5 and compare[p.total].mean() > 0.9


@pytest.mark.parametrize("method", ["n2v", "m2v"])
def test_the_directory_name_takes_the_sparse_suffix_only_when_asked(method, tmp_path):
    from opentf_amd.mdl.emb.gnn import Gnn
    plain = f"/{method}.b16.e4.ns2.lr0.01.es5.spe2.d16.add.stm.w3.wl5.wn3" + (".mtstm" if method == "m2v" else "")
    assert Gnn(str(tmp_path), "cpu", 0, _cfg(method), method)._dirname() == plain
    assert Gnn(str(tmp_path), "cpu", 0, _cfg(method, sparse=False), method)._dirname() == plain
    assert Gnn(str(tmp_path), "cpu", 0, _cfg(method, sparse=True), method)._dirname() == plain + ".sparse"


def test_the_two_entries_are_declared_and_bound():
    import ctypes
    from opentf_amd import libntf
    assert libntf.SYMBOLS["ntf_n2v_set_optimizer"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert libntf.SYMBOLS["ntf_n2v_moments"] == (ctypes.c_int, [ctypes.c_void_p] * 3)
    assert libntf.NTF_ESTATE == -3
