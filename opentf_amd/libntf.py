"""ctypes binding of libopentf_amd.so (include/opentf_amd.h) and a thin `Engine` object over the handle.

There is no CPU fallback: if the shared library is missing or the HIP device cannot be opened, this
module raises.  Build the library with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C opentf_amd/csrc`.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np

NTF_ABI_VERSION = 2
NTF_MAX_LAYERS = 8
NTF_MC_MAX_GROUP = 16     # Monte-Carlo passes per fused-MC launch at most (include/opentf_amd.h)
NTF_MC_TILE_GROUP = 4     # 32-expert tiles a workgroup of that kernel carries across the passes
NTF_EINVAL = -1
NTF_ESTATE = -3
INPUT_DENSE, INPUT_MEANPOOL, INPUT_MULTIHOT = 0, 1, 2
NSD = {None: 0, "": 0, "None": 0, "uniform": 1, "unigram": 2, "unigram_b": 3}
P_WEIGHT, P_BIAS, P_RHO_WEIGHT, P_RHO_BIAS = 0, 1, 2, 3

_RANGE_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_void_p)
_LIB_PATH = os.environ.get("NTF_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libopentf_amd.so")   # (NTF_LIB_PATH: A/B builds of the same ABI)


class NtfError(RuntimeError):
    pass


class ntf_config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p), ("n_layers", C.c_int32),
                ("dims", C.c_int32 * (NTF_MAX_LAYERS + 1)), ("bayesian", C.c_int32), ("input_mode", C.c_int32),
                ("max_batch", C.c_int32), ("ns", C.c_int32), ("nsd", C.c_int32), ("tpw", C.c_float), ("tnw", C.c_float),
                ("lr", C.c_float), ("seed", C.c_uint64), ("fused", C.c_int32), ("fuse_adam", C.c_int32), ("mfma", C.c_int32),
                ("expert_lo", C.c_int32), ("experts_global", C.c_int32), ("ep_world", C.c_int32), ("reserved", C.c_int32 * 2)]


class ntf_inject(C.Structure):
    _fields_ = [("neg_idx", C.c_void_p), ("eps_w", C.c_void_p * NTF_MAX_LAYERS), ("eps_b", C.c_void_p * NTF_MAX_LAYERS),
                ("s_in", C.c_void_p * NTF_MAX_LAYERS), ("s_out", C.c_void_p * NTF_MAX_LAYERS)]


# every symbol declared in include/opentf_amd.h: name -> (restype, argtypes)
_P, _I32, _I64, _F, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint64
SYMBOLS = {
    "ntf_engine_create": (C.c_int, [C.POINTER(ntf_config), C.POINTER(_P)]),
    "ntf_engine_destroy": (None, [_P]),
    "ntf_last_error": (C.c_char_p, [_P]),
    "ntf_abi_version": (C.c_int, []),
    "ntf_set_member_csr": (C.c_int, [_P, _P, _P, _I64]),
    "ntf_set_skill_csr": (C.c_int, [_P, _P, _P, _I64]),
    "ntf_set_skill_table": (C.c_int, [_P, _P, _I64, _I32]),
    "ntf_set_dense_input": (C.c_int, [_P, _P, _I64, _I32]),
    "ntf_set_unigram": (C.c_int, [_P, _P, _I64]),
    "ntf_set_param": (C.c_int, [_P, C.c_int, C.c_int, _P, _I64]),
    "ntf_get_param": (C.c_int, [_P, C.c_int, C.c_int, _P, _I64]),
    "ntf_get_grad": (C.c_int, [_P, C.c_int, C.c_int, _P, _I64]),
    "ntf_reset_optimizer": (C.c_int, [_P]),
    "ntf_set_lr": (C.c_int, [_P, _F]),
    "ntf_set_seed": (C.c_int, [_P, _U64, _U64]),
    "ntf_skip_step": (C.c_int, [_P]),
    "ntf_range_fallbacks": (C.c_int, [_P, C.POINTER(_I64)]),
    "ntf_prefetched_steps": (C.c_int, [_P, C.POINTER(_I64)]),
    "ntf_head_prefetch_hits": (C.c_int, [_P, C.POINTER(_I64)]),
    "ntf_first_layer_sweeps": (C.c_int, [_P, C.POINTER(_I64)]),
    "ntf_get_dlogits": (C.c_int, [_P, _P, _I64]),
    "ntf_get_negatives": (C.c_int, [_P, _P, _I64]),
    "ntf_fwd_ranges": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ntf_step_staged_deferred_cb": (C.c_int, [_P, _I64, C.c_int32, _I64, C.c_int32, _P, _RANGE_CB, _P]),
    "ntf_get_noise": (C.c_int, [_P, _U64, C.c_int32, C.c_int32, C.c_int32, _P, _I64]),
    "ntf_train_step": (C.c_int, [_P, _P, _I32, _P, _P]),
    "ntf_eval_step": (C.c_int, [_P, _P, _I32, _P, _P]),
    "ntf_backward": (C.c_int, [_P, _P, _I32, _I32, _P, _P]),
    "ntf_apply": (C.c_int, [_P]),
    "ntf_apply_ranges": (C.c_int, [_P, _P, _I32]),
    "ntf_train_epoch": (C.c_int, [_P, _P, _I64, _I32, _P]),
    "ntf_eval_epoch": (C.c_int, [_P, _P, _I64, _I32, _P]),
    "ntf_epoch_loss": (C.c_int, [_P, _P, _P]),
    "ntf_stage_order": (C.c_int, [_P, _P, _I64]),
    "ntf_step_staged": (C.c_int, [_P, _I64, _I32, _I64, _I32, _I32, _I32, _P]),
    "ntf_step_staged_deferred": (C.c_int, [_P, _I64, _I32, _I64, _I32, _P]),
    "ntf_dw_chunks": (C.c_int, [_P, C.POINTER(_I32)]),
    "ntf_dw_chunk_range": (C.c_int, [_P, _I32, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64)]),
    "ntf_dw_chunk": (C.c_int, [_P, _I32]),
    "ntf_param_segment": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_I64), C.POINTER(_I64)]),
    "ntf_step_staged_ep": (C.c_int, [_P, _I64, _I32, _I32]),
    "ntf_dh_buffer": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(_I64)]),
    "ntf_forward": (C.c_int, [_P, _P, _I32, _I32, _P, _P, _P, _P]),
    "ntf_logits": (C.c_int, [_P, _P, _I32, _P, _P]),
    "ntf_forward_topk": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    "ntf_infer_mc_plan": (C.c_int, [_I64, _I32, _I32, _I64, C.POINTER(_I32), C.POINTER(_I64)]),
    "ntf_mc_fused_passes": (C.c_int, [_P, C.POINTER(_I64)]),
    "ntf_gather_meanpool": (C.c_int, [_P, _P, _I64, _P]),
    "ntf_grad_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64)]),
    "ntf_moment_buffers": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_I64)]),
    "ntf_param_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64)]),
    "ntf_params_touched": (C.c_int, [_P]),
    "ntf_synchronize": (C.c_int, [_P]),
    "ntf_kernel_times": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "ntf_rank_metrics": (C.c_int, [C.c_int, _P, _I64, _I32, _P, _P, _I64, _P, _P, _I32, _P]),
    "ntf_skill_coverage": (C.c_int, [C.c_int, _P, _I64, _I32, _P, _P, _I64, _P, _P, _P, _I64, _P, _I32, _P]),
    "ntf_auc_micro_dense": (C.c_int, [C.c_int, _P, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _P, _P]),
    "ntf_auc_micro_csr": (C.c_int, [C.c_int, _P, _P, _P, _I64, _I64, _P, _P, _I64, _P, _I64, _P, _P]),
    "ntf_score_rows": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _I32, _P, _P]),
    "ntf_skill_cooccurrence": (C.c_int, [C.c_int, _I64, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P, _P]),
    "ntf_csr_result_fetch": (C.c_int, [_P, _P, _P, _P, _P]),
    "ntf_csr_result_free": (None, [_P]),
    "ntf_n2v_create": (C.c_int, [C.c_int, _I64, _I32, _P, _P, _P, _U64, C.POINTER(_P)]),
    "ntf_n2v_destroy": (None, [_P]),
    "ntf_n2v_last_error": (C.c_char_p, [_P]),
    "ntf_n2v_walks": (C.c_int, [_P, _P, _I64, _I32, _U64, _P]),
    "ntf_n2v_train_batch": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _F, _P, _I64, _P, _I64, _I32, _P]),
    "ntf_n2v_get": (C.c_int, [_P, C.c_int, _P]),
    "ntf_n2v_last_windows": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "ntf_n2v_edge_bce": (C.c_int, [_P, _P, _P, _I64, _P]),
    "ntf_n2v_set_optimizer": (C.c_int, [_P, _I32]),
    "ntf_n2v_moments": (C.c_int, [_P, _P, _P]),
    "ntf_n2v_set_walk_bias": (C.c_int, [_P, C.c_double, C.c_double]),
    "ntf_n2v_set_lazy": (C.c_int, [_P, _I32]),
    "ntf_n2v_lazy_state": (C.c_int, [_P, _P, _P, _P]),
    "ntf_m2v_create": (C.c_int, [C.c_int, _I32, _P, _I32, _P, _P, _P, _P, _I32, _P, _U64, C.POINTER(_P)]),
    "ntf_d2v_create": (C.c_int, [C.c_int, _I64, _I64, _I32, _P, _P, _P, _P, _P, _P, _U64, C.POINTER(_P)]),
    "ntf_d2v_destroy": (None, [_P]),
    "ntf_d2v_last_error": (C.c_char_p, [_P]),
    "ntf_d2v_train_epoch": (C.c_int, [_P, _I32, _I32, _I32, C.c_double, C.c_double, _U64, _I32, _P, _P, _P, _P]),
    "ntf_d2v_get": (C.c_int, [_P, C.c_int, _P]),
    "ntf_d2v_set": (C.c_int, [_P, C.c_int, _P]),
    "ntf_d2v_infer": (C.c_int, [_P, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, C.c_double, C.c_double, _U64, _I32, _P, _P, _P]),
    "ntf_knn_create": (C.c_int, [C.c_int, _P, _I64, _I32, C.POINTER(_P)]),
    "ntf_knn_destroy": (None, [_P]),
    "ntf_knn_last_error": (C.c_char_p, [_P]),
    "ntf_knn_query": (C.c_int, [_P, _P, _I64, _I32, _P, _I64, _P, _P, _P]),
    "ntf_k_gemm_f32": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _I64, _I64, _P, _I64, _I64, _P, _I64]),
    "ntf_k_fill_normal": (C.c_int, [_P, _U64, _U64, C.c_int, _I64, _P]),
    "ntf_k_fill_sign": (C.c_int, [_P, _U64, _U64, C.c_int, C.c_int, C.c_int, _P]),
}

# every symbol declared in include/opentf_amd_fair.h (the fair stage: a header and a table of its own, NTF_ABI_VERSION unchanged)
NTF_FAIR_MAX_GROUPS, NTF_FAIR_MAX_K = 64, 2048
FAIR_DET_GREEDY, FAIR_DET_CONS, FAIR_DET_RELAXED = 0, 1, 2
FAIR_ALGORITHMS = {"det_greedy": FAIR_DET_GREEDY, "det_cons": FAIR_DET_CONS, "det_relaxed": FAIR_DET_RELAXED}
FAIR_SYMBOLS = {
    "ntf_fair_rerank": (C.c_int, [C.c_int, _I32, _P, _P, _I64, _I32, _P, _I64, _I32, _P, _I64, _I32, _P, _P, _P]),
    "ntf_fair_metrics": (C.c_int, [C.c_int, _P, _I64, _I32, _P, _I64, _I32, _P, _I64, _P, _I32, _P, _P]),
}

# every symbol declared in include/opentf_amd_link.h (the link decode of a Gnn table: the second side header, NTF_ABI_VERSION unchanged)
LINK_SYMBOLS = {
    "ntf_link_create": (C.c_int, [C.c_int, _P, _I64, _I32, _I64, _I64, C.POINTER(_P)]),
    "ntf_link_destroy": (None, [_P]),
    "ntf_link_last_error": (C.c_char_p, [_P]),
    "ntf_link_topk": (C.c_int, [_P, _I64, _P, _P, _P, _I32, _I64, _P, _P, _P, _P]),
    "ntf_link_dense": (C.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _P]),
}

# every symbol declared in include/opentf_amd_roc.h (the micro ROC curve beside the AUC: the third side header, NTF_ABI_VERSION unchanged): the AUC entries'
# arguments up to chunk_bytes, then cap_points, fps, tps, thresholds, n_points, out_counts, out_auc
ROC_SYMBOLS = {
    "ntf_roc_micro_dense": (C.c_int, [C.c_int, _P, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P, _P]),
    "ntf_roc_micro_csr": (C.c_int, [C.c_int, _P, _P, _P, _I64, _I64, _P, _P, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P, _P]),
}

# every symbol declared in include/opentf_amd_fairsort.h (DetConstSort and the infeasible measures of the fair stage: the fourth side header, NTF_ABI_VERSION
# unchanged): ntf_fair_rerank's arguments without the algorithm plus out_tail; ntf_fair_metrics' arguments with two int32 outputs
FAIR_CONST_SORT = "det_const_sort"
FAIRSORT_SYMBOLS = {
    "ntf_fair_constsort": (C.c_int, [C.c_int, _P, _P, _I64, _I32, _P, _I64, _I32, _P, _I64, _I32, _P, _P, _P, _P]),
    "ntf_fair_infeasible": (C.c_int, [C.c_int, _P, _I64, _I32, _P, _I64, _I32, _P, _I64, _P, _I32, _P, _P]),
}

_lib = None


def lib():
    """The loaded shared library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NtfError(f"{_LIB_PATH} is missing: build it (make -C opentf_amd/csrc). There is no CPU fallback.")
        import torch  # noqa: F401  (load torch's bundled HIP runtime first: this library must share it, not bring a second copy)
        l = C.CDLL(_LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the library does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        for table in (FAIR_SYMBOLS, LINK_SYMBOLS, ROC_SYMBOLS, FAIRSORT_SYMBOLS):
            for name, (res, args) in table.items():
                fn = getattr(l, name)
                fn.restype, fn.argtypes = res, args
        if l.ntf_abi_version() != NTF_ABI_VERSION:
            raise NtfError("libopentf_amd.so ABI version mismatch")
        _lib = l
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def infer_mc_plan(experts, h, passes, budget_bytes):
    """ntf_infer_mc_plan: (passes per fused-MC launch, experts per launch) under a ring budget in bytes, or None when not even one pass over 256 experts fits
    (or an argument is not positive).  Needs no GPU."""
    g, r = C.c_int32(), C.c_int64()
    rc = lib().ntf_infer_mc_plan(int(experts), int(h), int(passes), int(budget_bytes), C.byref(g), C.byref(r))
    if rc == NTF_EINVAL:
        return None
    if rc != 0:
        raise NtfError(f"ntf_infer_mc_plan failed ({rc})")
    return g.value, r.value


def _fair_inputs(idx, group, p):
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    if idx.ndim != 2:
        raise NtfError(f"ranked ids must be [n, K], got {idx.shape}")
    group = np.ascontiguousarray(group, dtype=np.uint8).reshape(-1)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if p.ndim == 1: p = p.reshape(1, -1)
    if p.ndim != 2:
        raise NtfError(f"the target distribution must be [G], [1, G] or [n, G], got {p.shape}")
    return idx, group, p


def fair_rerank(cand_idx, cand_val, group, p, algorithm, k_out=None, device=0, want_pos=False):
    """ntf_fair_rerank (include/opentf_amd_fair.h): cand_idx [n, K] int32 ranked best first, cand_val [n, K] f32 or None, group [n_experts] uint8, p [G], [1, G] or
    [n, G] f64, algorithm one of FAIR_ALGORITHMS (a name or its code), k_out (None: K).  -> (out_idx [n, k_out] int32, out_val [n, k_out] f32 or None[, out_pos])"""
    idx, group, p = _fair_inputs(cand_idx, group, p)
    val = None if cand_val is None else _f32(cand_val)
    if val is not None and val.shape != idx.shape:
        raise NtfError(f"cand_val {val.shape} does not match cand_idx {idx.shape}")
    alg = FAIR_ALGORITHMS.get(algorithm, algorithm)
    if isinstance(alg, str):
        raise NtfError(f"unknown fair algorithm {algorithm!r}: one of {sorted(FAIR_ALGORITHMS)}")
    n, K = idx.shape
    k_out = K if k_out is None else int(k_out)
    shape = (n, max(k_out, 0))
    out_idx = np.empty(shape, dtype=np.int32)
    out_val = None if val is None else np.empty(shape, dtype=np.float32)
    out_pos = np.empty(shape, dtype=np.int32) if want_pos else None
    rc = lib().ntf_fair_rerank(int(device), int(alg), _ptr(idx), _ptr(val), n, K, _ptr(group), len(group), p.shape[1], _ptr(p), p.shape[0], k_out,
                               _ptr(out_idx), _ptr(out_val), _ptr(out_pos))
    if rc != 0:
        raise NtfError(f"ntf_fair_rerank failed ({rc})" + (": an argument outside the contract of include/opentf_amd_fair.h" if rc == NTF_EINVAL else ""))
    return (out_idx, out_val, out_pos) if want_pos else (out_idx, out_val)


def fair_metrics(idx, group, p, cutoffs, device=0, ndkl=True, skew=True):
    """ntf_fair_metrics (include/opentf_amd_fair.h) of the ranked ids idx [n, K]: -> (ndkl [n, n_cut] f64 or None, skew [n, n_cut, G] f64 or None)"""
    idx, group, p = _fair_inputs(idx, group, p)
    cu = np.ascontiguousarray(np.asarray(cutoffs, dtype=np.int32).reshape(-1))
    n, K = idx.shape
    G = p.shape[1]
    out_n = np.empty((n, len(cu)), dtype=np.float64) if ndkl else None
    out_s = np.empty((n, len(cu), G), dtype=np.float64) if skew else None
    rc = lib().ntf_fair_metrics(int(device), _ptr(idx), n, K, _ptr(group), len(group), G, _ptr(p), p.shape[0], _ptr(cu), len(cu), _ptr(out_n), _ptr(out_s))
    if rc != 0:
        raise NtfError(f"ntf_fair_metrics failed ({rc})" + (": an argument outside the contract of include/opentf_amd_fair.h" if rc == NTF_EINVAL else ""))
    return out_n, out_s


def fair_constsort(cand_idx, cand_val, group, p, k_out=None, device=0, want_pos=False, want_tail=False):
    """ntf_fair_constsort (include/opentf_amd_fairsort.h), arguments as fair_rerank's without the algorithm.  -> (out_idx [n, k_out] int32, out_val [n, k_out] f32 or
    None[, out_pos [n, k_out] int32][, out_tail [n] int32: the ranks the tail rule filled])"""
    idx, group, p = _fair_inputs(cand_idx, group, p)
    val = None if cand_val is None else _f32(cand_val)
    if val is not None and val.shape != idx.shape:
        raise NtfError(f"cand_val {val.shape} does not match cand_idx {idx.shape}")
    n, K = idx.shape
    k_out = K if k_out is None else int(k_out)
    shape = (n, max(k_out, 0))
    out_idx = np.empty(shape, dtype=np.int32)
    out_val = None if val is None else np.empty(shape, dtype=np.float32)
    out_pos = np.empty(shape, dtype=np.int32) if want_pos else None
    out_tail = np.empty(n, dtype=np.int32) if want_tail else None
    rc = lib().ntf_fair_constsort(int(device), _ptr(idx), _ptr(val), n, K, _ptr(group), len(group), p.shape[1], _ptr(p), p.shape[0], k_out,
                                  _ptr(out_idx), _ptr(out_val), _ptr(out_pos), _ptr(out_tail))
    if rc != 0:
        raise NtfError(f"ntf_fair_constsort failed ({rc})" + (": an argument outside the contract of include/opentf_amd_fairsort.h" if rc == NTF_EINVAL else ""))
    return (out_idx, out_val) + ((out_pos,) if want_pos else ()) + ((out_tail,) if want_tail else ())


def fair_infeasible(idx, group, p, cutoffs, device=0, index=True, count=True):
    """ntf_fair_infeasible (include/opentf_amd_fairsort.h) of the ranked ids idx [n, K]: -> (InfeasibleIndex [n, n_cut] int32 or None, InfeasibleCount likewise)"""
    idx, group, p = _fair_inputs(idx, group, p)
    cu = np.ascontiguousarray(np.asarray(cutoffs, dtype=np.int32).reshape(-1))
    n, K = idx.shape
    out_i = np.empty((n, len(cu)), dtype=np.int32) if index else None
    out_c = np.empty((n, len(cu)), dtype=np.int32) if count else None
    rc = lib().ntf_fair_infeasible(int(device), _ptr(idx), n, K, _ptr(group), len(group), p.shape[1], _ptr(p), p.shape[0], _ptr(cu), len(cu), _ptr(out_i), _ptr(out_c))
    if rc != 0:
        raise NtfError(f"ntf_fair_infeasible failed ({rc})" + (": an argument outside the contract of include/opentf_amd_fairsort.h" if rc == NTF_EINVAL else ""))
    return out_i, out_c


class DeviceView:
    """`__cuda_array_interface__` view of an engine-owned HBM buffer (for torch.as_tensor / RCCL)."""

    def __init__(self, ptr, n, owner):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f4", "data": (int(ptr), False), "version": 2, "strides": None}


def gemm_f32(m, n, k, A, sam, sak, B, sbk, sbn, C_, ldc, stream=None):
    """ntf_k_gemm_f32 on caller-owned device memory (addresses as ints): C[i * ldc + j] = sum_p A[i * sam + p * sak] * B[p * sbk + j * sbn]
    for i < m, j < n, f32 MFMA products and accumulation, queued on `stream` (a hipStream_t; None: the null stream).  No synchronisation."""
    rc = lib().ntf_k_gemm_f32(stream, int(m), int(n), int(k), A, int(sam), int(sak), B, int(sbk), int(sbn), C_, int(ldc))
    if rc != 0:
        raise NtfError(f"ntf_k_gemm_f32 failed ({rc})")


class ScoreResult:
    """what `Engine.score_rows` returns; a field that was not asked for is None"""
    __slots__ = ("metrics", "counts", "auc", "vals", "idx")

    def __init__(self, metrics, counts, auc, vals, idx):
        self.metrics, self.counts, self.auc, self.vals, self.idx = metrics, counts, auc, vals, idx


class _Handle:
    """One native handle: the pointer, close / __del__, the return-code check and the raise of a failed create.  A subclass names its three symbols and the word
    its error messages carry after "libopentf_amd"."""

    _CREATE = _DESTROY = _LAST_ERROR = None
    _TAG = ""

    def _create(self, *args):
        self._h = C.c_void_p()
        rc = getattr(lib(), self._CREATE)(*args, C.byref(self._h))
        if rc != 0:
            msg = getattr(lib(), self._LAST_ERROR)(None)
            self._h = None
            raise NtfError(f"{self._CREATE} failed ({rc}): {msg.decode() if msg else ''}")

    def _ck(self, rc):
        if rc != 0:
            raise NtfError(f"libopentf_amd{self._TAG} error {rc}: {getattr(lib(), self._LAST_ERROR)(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(_Handle):
    """One Fnn/Bnn model resident on one MI355X.  dims = [D, *h, M].
    expert_shard = (lo, hi), ep_world = G: this engine owns the experts [lo, hi) of the output layer only (one of G such engines, one per GPU;
    hidden layers replicated; see ntf_config.expert_lo in include/opentf_amd.h and opentf_amd/ep.py).  `dims[-1]` then is hi - lo, `experts_global` is M."""

    _CREATE, _DESTROY, _LAST_ERROR = "ntf_engine_create", "ntf_engine_destroy", "ntf_last_error"

    def __init__(self, dims, bayesian=False, input_mode=INPUT_DENSE, max_batch=1000, ns=5, nsd="uniform", tpw=10.0, tnw=1.0,
                 lr=1e-3, seed=0, device=0, stream=None, fused=True, fuse_adam=False, mfma=None, expert_shard=None, ep_world=1):
        self.dims = [int(d) for d in dims]
        self.experts_global = self.dims[-1]
        self.expert_lo, self.ep_world = 0, int(ep_world)
        if expert_shard is not None:
            lo, hi = (int(v) for v in expert_shard)
            if not 0 <= lo < hi <= self.experts_global:
                raise NtfError(f"expert_shard {expert_shard} outside [0, {self.experts_global})")
            self.expert_lo, self.dims[-1] = lo, hi - lo
        self.L = len(self.dims) - 1
        if not 1 <= self.L <= NTF_MAX_LAYERS:
            raise NtfError("between 1 and 8 layers supported")
        self.bayesian = bool(bayesian)
        self.ns = int(ns) if NSD[nsd] else 0
        self.max_batch = int(max_batch)
        cfg = ntf_config()
        cfg.abi_version, cfg.device, cfg.stream, cfg.n_layers = NTF_ABI_VERSION, int(device), stream, self.L
        for i, d in enumerate(self.dims):
            cfg.dims[i] = d
        cfg.bayesian, cfg.input_mode, cfg.max_batch = int(self.bayesian), int(input_mode), self.max_batch
        cfg.ns, cfg.nsd, cfg.tpw, cfg.tnw, cfg.lr, cfg.seed, cfg.fused = max(self.ns, 0), NSD[nsd], float(tpw), float(tnw), float(lr), int(seed) & (2**64 - 1), int(bool(fused))
        if mfma == "bf16x6": raise ValueError("mfma='bf16x6' was retired in round 6 (fp16x3, the default, has its accuracy at half the matrix work); use None or 'f32'")
        cfg.mfma = {None: 0, "default": 0, "f32": 1, "fp16x3": 3}[mfma] if not isinstance(mfma, int) or isinstance(mfma, bool) else int(mfma)
        cfg.fuse_adam = int(fuse_adam)  # 0: flat Adam kernel; 1: inside the dW epilogue; 2: chunked beside the dW kernel on a side stream
        if expert_shard is not None or self.ep_world > 1:
            cfg.expert_lo, cfg.experts_global, cfg.ep_world = self.expert_lo, self.experts_global, self.ep_world
        self.stream_handle = stream   # the caller's hipStream_t (int) the engine runs on, None: a stream of its own
        self._create(C.byref(cfg))
        self._keep = []

    # ---- data
    @staticmethod
    def _csr(mat_or_tuple):
        if isinstance(mat_or_tuple, tuple):
            indptr, indices = mat_or_tuple
        else:
            import scipy.sparse
            m = scipy.sparse.csr_matrix(mat_or_tuple)
            m.sort_indices()
            indptr, indices = m.indptr, m.indices
        return np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32)

    def set_member(self, member):
        ip, ix = self._csr(member)
        self._ck(lib().ntf_set_member_csr(self._h, _ptr(ip), _ptr(ix), len(ip) - 1))

    def set_skill_csr(self, skill):
        ip, ix = self._csr(skill)
        self._ck(lib().ntf_set_skill_csr(self._h, _ptr(ip), _ptr(ix), len(ip) - 1))

    def set_skill_table(self, table):
        t = _f32(table)
        self._ck(lib().ntf_set_skill_table(self._h, _ptr(t), t.shape[0], t.shape[1]))

    def set_dense_input(self, X):
        x = _f32(X)
        self._ck(lib().ntf_set_dense_input(self._h, _ptr(x), x.shape[0], x.shape[1]))

    def set_unigram(self, freq):
        f = np.ascontiguousarray(np.asarray(freq, dtype=np.float64).reshape(-1))
        self._ck(lib().ntf_set_unigram(self._h, _ptr(f), len(f)))

    # ---- state (reference state_dict layout, src/mdl/fnn.py:20-22 / bayesian-torch LinearFlipout)
    def _kinds(self):
        return ([("mu_weight", P_WEIGHT), ("rho_weight", P_RHO_WEIGHT), ("mu_bias", P_BIAS), ("rho_bias", P_RHO_BIAS)] if self.bayesian
                else [("weight", P_WEIGHT), ("bias", P_BIAS)])

    def _shape(self, layer, kind):
        o, i = self.dims[layer + 1], self.dims[layer]
        return (o, i) if kind in (P_WEIGHT, P_RHO_WEIGHT) else (o,)

    def load_state_dict(self, sd):
        for l in range(self.L):
            for name, kind in self._kinds():
                a = sd[f"layers.{l}.{name}"]
                a = _f32(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
                if l == self.L - 1 and a.shape[0] == self.experts_global != self.dims[-1]:   # an expert shard takes its rows of the whole layer
                    a = _f32(a[self.expert_lo: self.expert_lo + self.dims[-1]])
                if a.shape != self._shape(l, kind):
                    raise NtfError(f"layers.{l}.{name}: shape {a.shape} != {self._shape(l, kind)}")
                self._ck(lib().ntf_set_param(self._h, l, kind, _ptr(a), a.size))

    def state_dict(self):
        sd = OrderedDict()
        for l in range(self.L):
            for name, kind in self._kinds():
                a = np.empty(self._shape(l, kind), dtype=np.float32)
                self._ck(lib().ntf_get_param(self._h, l, kind, _ptr(a), a.size))
                sd[f"layers.{l}.{name}"] = a
        return sd

    def grads(self):
        """p.grad of every parameter after backward()/train_step() (state_dict key order)."""
        sd = OrderedDict()
        for l in range(self.L):
            for name, kind in self._kinds():
                a = np.empty(self._shape(l, kind), dtype=np.float32)
                self._ck(lib().ntf_get_grad(self._h, l, kind, _ptr(a), a.size))
                sd[f"layers.{l}.{name}"] = a
        return sd

    def reset_optimizer(self):
        self._ck(lib().ntf_reset_optimizer(self._h))

    def set_lr(self, lr):
        self._ck(lib().ntf_set_lr(self._h, float(lr)))

    def set_seed(self, seed, step=0):
        self._ck(lib().ntf_set_seed(self._h, int(seed) & (2**64 - 1), int(step)))

    def skip_step(self):
        """advance the generators' step counter without running a step (a data-parallel rank with an empty shard)"""
        self._ck(lib().ntf_skip_step(self._h))

    def range_fallbacks(self):
        """steps / inference calls that ran on the exact-f32 kernels because an operand left the fp16x3 window"""
        n = C.c_int64()
        self._ck(lib().ntf_range_fallbacks(self._h, C.byref(n)))
        return n.value

    def mc_fused_passes(self):
        """Monte-Carlo passes served by fused-MC launches (NTF_INFER_MC=1) whose call was not redone behind a raised range flag"""
        n = C.c_int64()
        self._ck(lib().ntf_mc_fused_passes(self._h, C.byref(n)))
        return n.value

    def prefetched_steps(self):
        """steps that started on output-layer operands written by the previous step's dW + Adam epilogue (no producer pass of their own)"""
        n = C.c_int64()
        self._ck(lib().ntf_prefetched_steps(self._h, C.byref(n)))
        return n.value

    def head_prefetch_hits(self):
        """steps whose sampler / gather / hidden layer had run beside the previous step's dW kernel (include/opentf_amd.h)"""
        n = C.c_int64()
        self._ck(lib().ntf_head_prefetch_hits(self._h, C.byref(n)))
        return n.value

    def first_layer_sweeps(self):
        """steps that started on a multi-hot Flipout first-layer operand written by the previous step's one-pass finalize + Adam + producer (include/opentf_amd.h)"""
        n = C.c_int64()
        self._ck(lib().ntf_first_layer_sweeps(self._h, C.byref(n)))
        return n.value

    def dlogits(self, B):
        """d loss / d z [B, M] of the output layer after the last backward (B = that step's batch)"""
        out = np.empty((int(B), self.dims[-1]), dtype=np.float32)
        self._ck(lib().ntf_get_dlogits(self._h, _ptr(out), out.size))
        return out

    def negatives(self, B):
        """the last step's sampled negatives [B, ns] (global expert ids)"""
        out = np.empty((int(B), int(self.ns)), dtype=np.int64)
        self._ck(lib().ntf_get_negatives(self._h, _ptr(out), out.size))
        return out

    def noise(self, step, B):
        """the device generators' own Flipout draws of step index `step` (include/opentf_amd.h ntf_get_noise), as the oracle's per-layer list of
        {eps_w [out, in], eps_b [out], s_in [B, in], s_out [B, out]}"""
        out = []
        for l in range(len(self.dims) - 1):
            n_in, n_out = int(self.dims[l]), int(self.dims[l + 1])
            d = {"eps_w": np.empty((n_out, n_in), np.float32), "eps_b": np.empty(n_out, np.float32),
                 "s_in": np.empty((int(B), n_in), np.float32), "s_out": np.empty((int(B), n_out), np.float32)}
            for kind, key in enumerate(("eps_w", "eps_b", "s_in", "s_out")):
                self._ck(lib().ntf_get_noise(self._h, int(step), l, kind, int(B), _ptr(d[key]), d[key].size))
            out.append(d)
        return out

    # ---- steps
    def _inject(self, inject, B):
        if not inject:
            return None, []
        keep, st = [], ntf_inject()
        if inject.get("neg_idx") is not None:
            a = np.ascontiguousarray(np.asarray(inject["neg_idx"], dtype=np.int64)); keep.append(a)
            assert a.shape == (B, self.ns), (a.shape, B, self.ns)
            st.neg_idx = a.ctypes.data
        for key in ("eps_w", "eps_b", "s_in", "s_out"):
            for l, a in enumerate(inject.get(key) or []):
                if a is None:
                    continue
                a = _f32(a.detach().cpu().numpy() if hasattr(a, "detach") else a); keep.append(a)
                getattr(st, key)[l] = a.ctypes.data
        return st, keep

    @staticmethod
    def _rows(rows):
        return np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))

    def train_step(self, rows, inject=None, want_loss=True):
        r = self._rows(rows); st, keep = self._inject(inject, len(r)); loss = C.c_float()
        self._ck(lib().ntf_train_step(self._h, _ptr(r), len(r), C.byref(st) if st else None, C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def eval_step(self, rows, inject=None, want_loss=True):
        r = self._rows(rows); st, keep = self._inject(inject, len(r)); loss = C.c_float()
        self._ck(lib().ntf_eval_step(self._h, _ptr(r), len(r), C.byref(st) if st else None, C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def backward(self, rows, global_B=None, inject=None, want_loss=True):
        r = self._rows(rows); st, keep = self._inject(inject, len(r)); loss = C.c_float()
        self._ck(lib().ntf_backward(self._h, _ptr(r), len(r), int(global_B or len(r)), C.byref(st) if st else None, C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def apply(self):
        self._ck(lib().ntf_apply(self._h))

    def apply_ranges(self, ranges):
        """one Adam step on the [lo, hi) float ranges of the flat buffers only (sharded optimiser state, dp.py)"""
        a = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1))
        self._ck(lib().ntf_apply_ranges(self._h, _ptr(a), len(a) // 2))

    def param_tensor(self):
        """torch tensor aliasing the flat parameter buffer in HBM (what the sharded step all-gathers)"""
        import torch
        return torch.as_tensor(self.param_view(), device=f"cuda:{torch.cuda.current_device()}")

    def params_touched(self):
        """after writing parameters through param_tensor() / param_view(): drop operands a fused step prepared from the old values"""
        self._ck(lib().ntf_params_touched(self._h))

    def moment_tensors(self):
        """torch tensors aliasing Adam's exp_avg / exp_avg_sq buffers (flat, the parameters' layout)"""
        import torch
        m, v, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._ck(lib().ntf_moment_buffers(self._h, C.byref(m), C.byref(v), C.byref(n)))
        dev = f"cuda:{torch.cuda.current_device()}"
        return (torch.as_tensor(DeviceView(m.value, n.value, self), device=dev), torch.as_tensor(DeviceView(v.value, n.value, self), device=dev))

    def train_epoch(self, order, B):
        o = self._rows(order); loss = C.c_float()
        self._ck(lib().ntf_train_epoch(self._h, _ptr(o), len(o), int(B), C.byref(loss)))
        return loss.value

    def eval_epoch(self, order, B):
        o = self._rows(order); loss = C.c_float()
        self._ck(lib().ntf_eval_epoch(self._h, _ptr(o), len(o), int(B), C.byref(loss)))
        return loss.value

    def stage_order(self, order):
        o = self._rows(order)
        self._ck(lib().ntf_stage_order(self._h, _ptr(o), len(o)))

    def step_staged(self, offset, B, global_offset=None, global_B=None, train=True, apply=True, want_loss=False):
        loss = C.c_float()
        self._ck(lib().ntf_step_staged(self._h, int(offset), int(B), int(offset if global_offset is None else global_offset),
                                       int(B if global_B is None else global_B), int(train), int(apply), C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    # ---- expert-sharded output layer (see include/opentf_amd.h, opentf_amd/ep.py)
    def step_staged_ep(self, offset, B, phase):
        self._ck(lib().ntf_step_staged_ep(self._h, int(offset), int(B), int(phase)))

    def dh_tensor(self):
        """torch tensor aliasing the [max_batch * h[-1]] buffer of d(hidden): phase 1 leaves this shard's partial sum there, phase 2 reads the total"""
        import torch
        p, n = C.c_void_p(), C.c_int64()
        self._ck(lib().ntf_dh_buffer(self._h, C.byref(p), C.byref(n)))
        if not n.value:
            return None
        return torch.as_tensor(DeviceView(p.value, n.value, self), device=f"cuda:{torch.cuda.current_device()}")

    # ---- data-parallel pipelining (see include/opentf_amd.h)
    def step_staged_deferred(self, offset, B, global_offset, global_B, before_range=None):
        """before_range(j): called in front of forward range j (see fwd_ranges) - the caller orders the engine's stream behind that range's parameter all-gathers there"""
        if before_range is None:
            self._ck(lib().ntf_step_staged_deferred(self._h, int(offset), int(B), int(global_offset), int(global_B), None))
            return
        failure = []

        def _cb(j, _user):
            try:
                before_range(int(j))
                return 0
            except BaseException as ex:      # (never let an exception cross the C frame: report it, re-raise below)
                failure.append(ex)
                return 1
        cb = _RANGE_CB(_cb)
        rc = lib().ntf_step_staged_deferred_cb(self._h, int(offset), int(B), int(global_offset), int(global_B), None, cb, None)
        if failure: raise failure[0]
        self._ck(rc)

    def fwd_ranges(self, B):
        """[(k0, k1), ...]: the dW chunks of each forward range of a data-parallel step of B rows (empty: the head is not pipelined for this model)"""
        n = C.c_int32(); spans = (C.c_int32 * 8)()
        self._ck(lib().ntf_fwd_ranges(self._h, int(B), C.byref(n), spans))
        return [(int(spans[2 * j]), int(spans[2 * j + 1])) for j in range(n.value)]

    def dw_chunks(self):
        n = C.c_int32()
        self._ck(lib().ntf_dw_chunks(self._h, C.byref(n)))
        return n.value

    def dw_chunk_range(self, k):
        ow, orr, cnt = C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(lib().ntf_dw_chunk_range(self._h, int(k), C.byref(ow), C.byref(orr), C.byref(cnt)))
        return ow.value, orr.value, cnt.value

    def dw_chunk(self, k):
        self._ck(lib().ntf_dw_chunk(self._h, int(k)))

    def param_segment(self, layer, kind):
        """(offset, count) in floats of a parameter inside the flat parameter / gradient buffers"""
        o, c = C.c_int64(), C.c_int64()
        self._ck(lib().ntf_param_segment(self._h, int(layer), int(kind), C.byref(o), C.byref(c)))
        return o.value, c.value

    def rest_ranges(self):
        """[lo, hi) float ranges of the flat gradient buffer outside the output layer's weight / rho_weight segments."""
        n = self.grad_view().__cuda_array_interface__["shape"][0]
        cuts = []
        for kind in ([P_WEIGHT, P_RHO_WEIGHT] if self.bayesian else [P_WEIGHT]):
            o, c = C.c_int64(), C.c_int64()
            self._ck(lib().ntf_param_segment(self._h, self.L - 1, kind, C.byref(o), C.byref(c)))
            cuts.append((o.value, o.value + c.value))
        out, pos = [], 0
        for lo, hi in sorted(cuts):
            if lo > pos: out.append((pos, lo))
            pos = hi
        if pos < n: out.append((pos, n))
        return out

    def epoch_loss(self):
        s, k = C.c_double(), C.c_int64()
        self._ck(lib().ntf_epoch_loss(self._h, C.byref(s), C.byref(k)))
        return s.value, k.value

    # ---- inference
    def logits(self, rows, inject=None):
        r = self._rows(rows); st, keep = self._inject(inject, len(r))
        out = np.empty((len(r), self.dims[-1]), dtype=np.float32)
        self._ck(lib().ntf_logits(self._h, _ptr(r), len(r), C.byref(st) if st else None, _ptr(out)))
        return out

    def forward(self, rows, nmc=1, injects=None, uncertainty=False):
        r = self._rows(rows); B = len(r)
        out = np.empty((B, self.dims[-1]), dtype=np.float32)
        pu = np.empty(B, dtype=np.float32) if uncertainty else None
        mu = np.empty(B, dtype=np.float32) if uncertainty else None
        arr, keep = None, []
        if injects:
            arr = (ntf_inject * len(injects))()
            for i, inj in enumerate(injects):
                st, k = self._inject(inj, B); keep.append(k); arr[i] = st
        self._ck(lib().ntf_forward(self._h, _ptr(r), B, int(nmc), arr, _ptr(out), _ptr(pu), _ptr(mu)))
        return (out, pu, mu) if uncertainty else out

    def forward_topk(self, rows, K, nmc=1, uncertainty=False):
        r = self._rows(rows); B = len(r)
        vals = np.empty((B, K), dtype=np.float32); idx = np.empty((B, K), dtype=np.int32)
        pu = np.empty(B, dtype=np.float32) if uncertainty else None
        mu = np.empty(B, dtype=np.float32) if uncertainty else None
        self._ck(lib().ntf_forward_topk(self._h, _ptr(r), B, int(nmc), int(K), _ptr(vals), _ptr(idx), _ptr(pu), _ptr(mu)))
        return (vals, idx, pu, mu) if uncertainty else (vals, idx)

    def score_rows(self, rows, batch, nmc=1, K=0, cutoffs=(), auc=False, K_out=0):
        """ntf_score_rows: the prediction set `rows`, inferred in batches of `batch`, scored on the device against the resident member CSR.  K >= 1: the
        top-K-sparsified prediction (what test() writes with topK = K), K == 0: the dense one.  -> ScoreResult: metrics [n, 5 * len(cutoffs)] f32 in
        ntf_rank_metrics' layout (None without cutoffs), counts (P, N, U2) as Python ints and auc = U2 / (2 P N) (None unless auc), vals / idx [n, K_out]
        (None unless K_out).  Takes the generator steps the forward / forward_topk loop over the same batches would take."""
        r = self._rows(rows); n = len(r)
        cu = np.ascontiguousarray(np.asarray(cutoffs, dtype=np.int32).reshape(-1))
        metrics = np.zeros((n, 5 * len(cu)), dtype=np.float32) if len(cu) else None
        counts, a = (np.zeros(3, dtype=np.uint64), C.c_double()) if auc else (None, None)
        vals = np.zeros((n, int(K_out)), dtype=np.float32) if K_out else None
        idx = np.zeros((n, int(K_out)), dtype=np.int32) if K_out else None
        self._ck(lib().ntf_score_rows(self._h, _ptr(r), n, int(batch), int(nmc), int(K), _ptr(cu) if len(cu) else None, len(cu), _ptr(metrics), _ptr(counts),
                                      C.byref(a) if auc else None, int(K_out), _ptr(vals), _ptr(idx)))
        return ScoreResult(metrics, tuple(int(c) for c in counts) if auc else None, a.value if auc else None, vals, idx)

    def gather_meanpool(self, rows=None, n=None, to_host=True):
        r = None if rows is None else self._rows(rows)
        n = len(r) if r is not None else int(n)
        out = np.empty((n, self._table_d()), dtype=np.float32) if to_host else None
        self._ck(lib().ntf_gather_meanpool(self._h, _ptr(r), n, _ptr(out)))
        return out

    def _table_d(self):
        return self.dims[0]

    # ---- views / measurement
    def grad_view(self):
        p, n = C.c_void_p(), C.c_int64()
        self._ck(lib().ntf_grad_buffer(self._h, C.byref(p), C.byref(n)))
        return DeviceView(p.value, n.value, self)

    def param_view(self):
        p, n = C.c_void_p(), C.c_int64()
        self._ck(lib().ntf_param_buffer(self._h, C.byref(p), C.byref(n)))
        return DeviceView(p.value, n.value, self)

    def grad_tensor(self):
        """torch tensor aliasing the flat gradient buffer in HBM (what RCCL all-reduces)."""
        import torch
        return torch.as_tensor(self.grad_view(), device=f"cuda:{torch.cuda.current_device()}")

    def synchronize(self):
        self._ck(lib().ntf_synchronize(self._h))

    def kernel_times(self, enable=True):
        """enable: False / True (every kernel family) / 2 (only the output layer's forward and dW kernels) / 3 (only its forward kernel) / 4 (only its dW kernel)"""
        cap = 32
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); calls = (C.c_int64 * cap)()
        n = lib().ntf_kernel_times(self._h, int(enable), names, ms, calls, cap)
        return {names[i].decode(): (ms[i], calls[i]) for i in range(min(n, cap))}


class Node2Vec(_Handle):
    """torch_geometric.nn.Node2Vec resident on one MI355X: embedding.weight [num_nodes, d] + dense Adam, or with sparse=True torch.optim.SparseAdam
    over the rows a batch names (include/opentf_amd.h, ntf_n2v_set_optimizer).  p, q: the return and in-out parameters of the walks (ntf_n2v_set_walk_bias);
    (1, 1), the default, is the uniform walk.  lazy=True (or a window in steps): dense Adam's table, bit for bit, with only the rows a batch names written
    (ntf_n2v_set_lazy); not with sparse."""

    _CREATE, _DESTROY, _LAST_ERROR, _TAG = "ntf_n2v_create", "ntf_n2v_destroy", "ntf_n2v_last_error", " n2v"
    LAZY_WINDOW = 4096          # lazy=True: a full flush every 4096 applied steps at the latest, a ring of 32 KB

    def __init__(self, rowptr, col, init_weight, seed=0, device=0, sparse=False, p=1.0, q=1.0, lazy=False):
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64); self.col = np.ascontiguousarray(col, dtype=np.int32)
        w = _f32(init_weight)
        self.num_nodes, self.d = w.shape
        if len(self.rowptr) != self.num_nodes + 1:
            raise NtfError("rowptr must have num_nodes + 1 entries")
        self._create(int(device), self.num_nodes, self.d, _ptr(self.rowptr), _ptr(self.col), _ptr(w), int(seed) & (2**64 - 1))
        self.p, self.q = 1.0, 1.0
        self._choose_optimizer(sparse, lazy)
        if float(p) != 1.0 or float(q) != 1.0: self.set_walk_bias(p, q)

    def _choose_optimizer(self, sparse, lazy):
        """the tail of both constructors: dense Adam unless one of the two opt-in modes is asked for"""
        self.sparse = False; self.lazy = 0
        if sparse: self.set_optimizer(True)
        if lazy: self.set_lazy(lazy)

    def set_walk_bias(self, p, q):
        """node2vec's p (return) and q (in-out), each in [1e-4, 1e4]; (1, 1) is the uniform walk again.  Any time: walks carry no state between calls.  Refused on a
        metapath handle, and on a graph with a CSR row that is not ascending (the handle then goes on unbiased)"""
        self._ck(lib().ntf_n2v_set_walk_bias(self._h, float(p), float(q)))
        self.p, self.q = float(p), float(q)

    def set_optimizer(self, sparse):
        """dense Adam (False / 0) or sparse Adam (True / 1); refused once a step has been applied or while a gradient is pending"""
        self._ck(lib().ntf_n2v_set_optimizer(self._h, int(bool(sparse))))
        self.sparse = bool(sparse)

    def set_lazy(self, window):
        """lazy dense Adam: True = the default window (LAZY_WINDOW steps), False / 0 = off, otherwise the ring's size in steps; refused on a sparse handle, once a
        step has been applied or while a gradient is pending"""
        w = self.LAZY_WINDOW if window is True else int(window)
        self._ck(lib().ntf_n2v_set_lazy(self._h, w))
        self.lazy = w

    def lazy_state(self):
        """(applied [num_nodes] uint32: the Adam steps each row has taken, applied steps of the handle, full flushes so far); reads only, flushes nothing"""
        a = np.empty(self.num_nodes, dtype=np.uint32); steps, flushes = C.c_int64(), C.c_int64()
        self._ck(lib().ntf_n2v_lazy_state(self._h, _ptr(a), C.byref(steps), C.byref(flushes)))
        return a, steps.value, flushes.value

    def walks(self, start, walk_length, step=0):
        s = np.ascontiguousarray(start, dtype=np.int64)
        out = np.empty((len(s), int(walk_length)), dtype=np.int64)
        self._ck(lib().ntf_n2v_walks(self._h, _ptr(s), len(s), int(walk_length), int(step), _ptr(out)))
        return out

    def train_batch(self, batch, walk_length, context, walks_per_node, num_neg, lr, apply=True, want_loss=True):
        b = np.ascontiguousarray(batch, dtype=np.int64); loss = C.c_float()
        self._ck(lib().ntf_n2v_train_batch(self._h, _ptr(b), len(b), int(walk_length), int(context), int(walks_per_node), int(num_neg), float(lr),
                                           None, 0, None, 0, int(apply), C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def loss_on(self, pos_rw, neg_rw, lr=0.0, apply=False):
        """loss (and gradient / Adam step) on GIVEN window rows [n, context]: Node2Vec.loss(pos_rw, neg_rw)"""
        p = np.ascontiguousarray(pos_rw, dtype=np.int64); n = np.ascontiguousarray(neg_rw, dtype=np.int64); loss = C.c_float()
        assert p.shape[1] == n.shape[1]
        self._ck(lib().ntf_n2v_train_batch(self._h, None, 0, max(p.shape[1], 2), p.shape[1], 1, 1, float(lr), _ptr(p), len(p), _ptr(n), len(n), int(apply), C.byref(loss)))
        return loss.value

    def last_windows(self):
        """(positive, negative) window rows [n, context] of the last accepted batch, as the device held them"""
        n_pos, n_neg, ctx = C.c_int64(), C.c_int64(), C.c_int32()
        self._ck(lib().ntf_n2v_last_windows(self._h, C.byref(n_pos), C.byref(n_neg), C.byref(ctx), None, None))
        pos = np.empty((n_pos.value, ctx.value), dtype=np.int64); neg = np.empty((n_neg.value, ctx.value), dtype=np.int64)
        self._ck(lib().ntf_n2v_last_windows(self._h, C.byref(n_pos), C.byref(n_neg), C.byref(ctx), _ptr(pos), _ptr(neg)))
        return pos, neg

    def weight(self):
        out = np.empty((self.num_nodes, self.d), dtype=np.float32)
        self._ck(lib().ntf_n2v_get(self._h, 0, _ptr(out))); return out

    def grad(self):
        out = np.empty((self.num_nodes, self.d), dtype=np.float32)
        self._ck(lib().ntf_n2v_get(self._h, 1, _ptr(out))); return out

    def moments(self):
        """(exp_avg, exp_avg_sq) of the optimiser, [num_nodes, d] each"""
        m = np.empty((self.num_nodes, self.d), dtype=np.float32); v = np.empty((self.num_nodes, self.d), dtype=np.float32)
        self._ck(lib().ntf_n2v_moments(self._h, _ptr(m), _ptr(v))); return m, v

    def edge_bce(self, src, dst):
        s = np.ascontiguousarray(src, dtype=np.int64); t = np.ascontiguousarray(dst, dtype=np.int64); out = C.c_float()
        self._ck(lib().ntf_n2v_edge_bce(self._h, _ptr(s), _ptr(t), len(s), C.byref(out))); return out.value


class MetaPath2Vec(Node2Vec):
    """torch_geometric.nn.MetaPath2Vec resident on one MI355X (include/opentf_amd.h, ntf_m2v_create): a Node2Vec handle over [total + 1, d] that carries a metapath.
    type_counts: node counts in table order (sorted type names); hops: [(src_type, dst_type, rowptr, col)] with LOCAL ids, hop i's dst = hop i + 1's src.
    `walks` / `train_batch` take LOCAL ids of hops[0]'s source type and `walk_length` counts NODES (PyG's walk_length + 1); everything else speaks global rows,
    `dummy` (= total) included."""

    _CREATE = "ntf_m2v_create"

    def __init__(self, type_counts, hops, init_weight, seed=0, device=0, sparse=False, lazy=False):
        tc = np.ascontiguousarray(type_counts, dtype=np.int64).reshape(-1)
        w = _f32(init_weight)
        self.num_nodes, self.d = w.shape
        self.type_start = np.concatenate([[0], np.cumsum(tc)]).astype(np.int64)
        self.dummy = int(self.type_start[-1])
        if self.num_nodes != self.dummy + 1:
            raise NtfError("init_weight must have sum(type_counts) + 1 rows (the last one is the dummy row)")
        hs = np.ascontiguousarray([h[0] for h in hops], dtype=np.int32); hd = np.ascontiguousarray([h[1] for h in hops], dtype=np.int32)
        self._rowptr = [np.ascontiguousarray(h[2], dtype=np.int64) for h in hops]; self._col = [np.ascontiguousarray(h[3], dtype=np.int32) for h in hops]
        for s, rp in zip(hs, self._rowptr):
            if not (0 <= s < len(tc)) or len(rp) != tc[s] + 1:
                raise NtfError("a hop's rowptr must have (node count of its source type) + 1 entries")
        self.start_count = int(tc[hs[0]]) if len(hs) else 0
        rps = (C.c_void_p * max(len(hops), 1))(*[a.ctypes.data for a in self._rowptr])
        cls = (C.c_void_p * max(len(hops), 1))(*[a.ctypes.data if a.size else None for a in self._col])
        self._create(int(device), len(tc), _ptr(tc), len(hops), _ptr(hs), _ptr(hd), rps, cls, self.d, _ptr(w), int(seed) & (2**64 - 1))
        self._choose_optimizer(sparse, lazy)


class Doc2Vec(_Handle):
    """gensim.models.Doc2Vec's tables (doc vectors, word vectors, syn1neg) resident on one MI355X and its negative-sampling trainer (include/opentf_amd.h ntf_d2v_*).
    The documents come as CSR over vocabulary indices together with what build_vocab prepares (sample_int, cum_table) and the initial vectors."""

    _CREATE, _DESTROY, _LAST_ERROR, _TAG = "ntf_d2v_create", "ntf_d2v_destroy", "ntf_d2v_last_error", " d2v"
    DV, WV, SYN1NEG = 0, 1, 2

    def __init__(self, doc_ptr, words, sample_int, cum_table, init_wv, init_dv, seed=0, device=0):
        self.doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64); self.words = np.ascontiguousarray(words, dtype=np.int32)
        si = np.ascontiguousarray(sample_int, dtype=np.uint32); ct = np.ascontiguousarray(cum_table, dtype=np.uint32)
        wv, dv = _f32(init_wv), _f32(init_dv)
        self.n_docs, self.d = dv.shape
        self.n_vocab = wv.shape[0]
        if len(self.doc_ptr) != self.n_docs + 1 or len(si) != self.n_vocab or len(ct) != self.n_vocab or wv.shape[1] != self.d:
            raise NtfError("doc_ptr / sample_int / cum_table / initial vectors do not fit together")
        self._create(int(device), self.n_docs, self.n_vocab, self.d, _ptr(self.doc_ptr), _ptr(self.words), _ptr(si), _ptr(ct), _ptr(wv), _ptr(dv), int(seed) & (2**64 - 1))

    def train_epoch(self, dm, window, alpha_start, alpha_end, epoch, negative=5, serial=False, order=None, progress=None, want_loss=False, want_ms=False):
        """one pass over the documents (gensim train(epochs=1)); returns (mean loss | None, device ms | None)"""
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
        pr = None if progress is None else np.ascontiguousarray(progress, dtype=np.float64)
        loss, ms = C.c_double(), C.c_double()
        self._ck(lib().ntf_d2v_train_epoch(self._h, int(dm), int(window), int(negative), float(alpha_start), float(alpha_end), int(epoch), int(bool(serial)),
                                           _ptr(o) if o is not None else None, _ptr(pr) if pr is not None else None, C.byref(loss) if want_loss else None,
                                           C.byref(ms) if want_ms else None))
        return (loss.value if want_loss else None), (ms.value if want_ms else None)

    @classmethod
    def from_tables(cls, wv, syn1neg, sample_int, cum_table, device=0):
        """a handle for `infer` only: trained tables and the vocabulary's two tables, no corpus (one empty document stands in for it)"""
        wv, s1 = _f32(wv), _f32(syn1neg)
        if s1.shape != wv.shape:
            raise NtfError("wv and syn1neg do not have the same shape")
        net = cls(np.zeros(2, np.int64), np.zeros(1, np.int32), sample_int, cum_table, wv, np.zeros((1, wv.shape[1]), np.float32), device=device)
        net.set_vectors(cls.WV, wv); net.set_vectors(cls.SYN1NEG, s1)
        return net

    def infer(self, q_ptr, q_words, init, dm, window, epochs, alpha, min_alpha, seed, negative=5, ids=None, serial=False, want_ms=False):
        """gensim's infer_vector for a batch of documents that were not in the corpus (ntf_d2v_infer): q_ptr / q_words = the queries as CSR over vocabulary
        indices, init [n, d] their initial vectors, ids (None: 0..n-1) what each query's draws are counted by.  -> [n, d] (, device ms)"""
        qp = np.ascontiguousarray(q_ptr, dtype=np.int64); qw = np.ascontiguousarray(q_words, dtype=np.int32)
        n = len(qp) - 1
        v0 = _f32(init)
        if v0.ndim != 2 or v0.shape != (n, self.d):
            raise NtfError(f"init must be [{n}, {self.d}], got {v0.shape}")
        if len(qp) and len(qw) < int(qp[-1]):
            raise NtfError("q_words is shorter than q_ptr[-1]")
        if len(qw) == 0: qw = np.zeros(1, np.int32)
        qi = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        if qi is not None and len(qi) != n:
            raise NtfError("ids must hold one id per query")
        out = np.empty((n, self.d), dtype=np.float32); ms = C.c_double()
        self._ck(lib().ntf_d2v_infer(self._h, n, _ptr(qp), _ptr(qw), _ptr(qi) if qi is not None else None, int(dm), int(window), int(negative), int(epochs),
                                     float(alpha), float(min_alpha), int(seed) & (2**64 - 1), int(bool(serial)), _ptr(v0), _ptr(out), C.byref(ms) if want_ms else None))
        return (out, ms.value) if want_ms else out

    def vectors(self, what=0):
        out = np.empty((self.n_docs if what == 0 else self.n_vocab, self.d), dtype=np.float32)
        self._ck(lib().ntf_d2v_get(self._h, int(what), _ptr(out))); return out

    def set_vectors(self, what, values):
        v = _f32(values)
        assert v.shape == ((self.n_docs if what == 0 else self.n_vocab), self.d)
        self._ck(lib().ntf_d2v_set(self._h, int(what), _ptr(v)))


class Knn(_Handle):
    """Batched cosine nearest-neighbour search over a [rows, d] float32 table resident on one MI355X (include/opentf_amd.h ntf_knn_*): what
    KeyedVectors.most_similar does one query a call on the host.  The table is uploaded once; `query` never forms [n, rows]."""

    _CREATE, _DESTROY, _LAST_ERROR, _TAG = "ntf_knn_create", "ntf_knn_destroy", "ntf_knn_last_error", " knn"
    WORKSPACE_BYTES = 256 << 20     # NTF_KNN_WORKSPACE_BYTES
    UNIT_BYTES = 32 * 256 * 4        # the smallest unit of work: 32 queries x 256 table rows of f32 sims

    def __init__(self, table, device=0):
        t = _f32(table)
        if t.ndim != 2:
            raise NtfError(f"table must be [rows, d], got {t.shape}")
        self.n_rows, self.d = int(t.shape[0]), int(t.shape[1])
        self._create(int(device), _ptr(t), self.n_rows, self.d)

    def query(self, queries, topn=10, exclude=None, workspace_bytes=0, want_ms=False):
        """the topn most similar rows of every query [n, d], largest sim first, equal sims by ascending row id; exclude [n] (None; -1: none) = a row id never returned
        for that query.  -> (idx [n, topn] int32, sims [n, topn] float32[, device ms]); slots past the eligible rows hold id -1 and sim -inf"""
        if not getattr(self, "_h", None):
            raise NtfError("the Knn handle is closed")
        q = _f32(queries)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise NtfError(f"queries must be [n, {self.d}], got {q.shape}")
        n = int(q.shape[0])
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.int64)
        if ex is not None and ex.shape != (n,):
            raise NtfError("exclude must hold one row id per query")
        idx = np.empty((n, max(int(topn), 0)), dtype=np.int32); sims = np.empty((n, max(int(topn), 0)), dtype=np.float32); ms = C.c_double()
        self._ck(lib().ntf_knn_query(self._h, _ptr(q), n, int(topn), _ptr(ex), int(workspace_bytes), _ptr(idx), _ptr(sims), C.byref(ms) if want_ms else None))
        return (idx, sims, ms.value) if want_ms else (idx, sims)


class Link(_Handle):
    """Link decode over a [rows, d] float32 node-embedding table resident on one MI355X (include/opentf_amd_link.h ntf_link_*): logit <E[query], E[candidate]> and
    its sigmoid for every row of the candidate block [cand_lo, cand_hi), ranked by the logit.  Candidate id j is table row cand_lo + j.  Queries are table rows
    (`rows` [n]) or mean pools of table rows (`pooled` = (ptr [n + 1], items) or a scipy sparse [n, rows] whose column ids are table rows), gathered on the device."""

    _CREATE, _DESTROY, _LAST_ERROR, _TAG = "ntf_link_create", "ntf_link_destroy", "ntf_link_last_error", " link"
    WORKSPACE_BYTES = Knn.WORKSPACE_BYTES
    UNIT_BYTES = Knn.UNIT_BYTES
    MAX_K = 2048

    def __init__(self, table, cand_lo, cand_hi, device=0):
        t = _f32(table)
        if t.ndim != 2:
            raise NtfError(f"table must be [rows, d], got {t.shape}")
        self.n_rows, self.d = int(t.shape[0]), int(t.shape[1])
        self.cand_lo, self.cand_hi = int(cand_lo), int(cand_hi)
        self.n_cand = self.cand_hi - self.cand_lo
        self._create(int(device), _ptr(t), self.n_rows, self.d, self.cand_lo, self.cand_hi)

    def _queries(self, rows, pooled):
        """-> (n, q_rows, q_ptr, q_items): int64 arrays or None, as the C entries take them (which refuse both or neither)"""
        if not getattr(self, "_h", None):
            raise NtfError("the Link handle is closed")
        r = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        ptr = items = None
        if pooled is not None:
            if hasattr(pooled, "tocsr"):
                m = pooled.tocsr(); m.sort_indices()
                pooled = (m.indptr, m.indices)
            ptr = np.ascontiguousarray(np.asarray(pooled[0], dtype=np.int64).reshape(-1))
            items = np.ascontiguousarray(np.asarray(pooled[1], dtype=np.int64).reshape(-1))
            if len(ptr) < 1 or (len(ptr) > 1 and int(ptr[-1]) > len(items)):
                raise NtfError("pooled queries: ptr must hold n + 1 offsets into items")
        n = len(r) if r is not None else (len(ptr) - 1 if ptr is not None else 0)
        return n, r, ptr, items

    def topk(self, rows=None, pooled=None, K=10, workspace_bytes=0, want_ms=False):
        """the K best candidates of every query, largest logit first, equal logits by ascending candidate id -> (idx [n, K] int32, logit [n, K] f32, prob [n, K] f32
        [, device ms]); slots past the C candidates hold id -1, logit -inf and probability 0"""
        n, r, ptr, items = self._queries(rows, pooled)
        shape = (max(n, 0), max(int(K), 0))
        idx = np.empty(shape, dtype=np.int32); logit = np.empty(shape, dtype=np.float32); prob = np.empty(shape, dtype=np.float32); ms = C.c_double()
        self._ck(lib().ntf_link_topk(self._h, n, _ptr(r), _ptr(ptr), _ptr(items), int(K), int(workspace_bytes), _ptr(idx), _ptr(logit), _ptr(prob),
                                     C.byref(ms) if want_ms else None))
        return (idx, logit, prob, ms.value) if want_ms else (idx, logit, prob)

    def dense(self, rows=None, pooled=None, workspace_bytes=0, want_ms=False, logit=True, prob=True):
        """every candidate of every query -> (logit [n, C] f32 or None, prob [n, C] f32 or None[, device ms])"""
        n, r, ptr, items = self._queries(rows, pooled)
        shape = (max(n, 0), self.n_cand)
        lo = np.empty(shape, dtype=np.float32) if logit else None
        pr = np.empty(shape, dtype=np.float32) if prob else None
        ms = C.c_double()
        self._ck(lib().ntf_link_dense(self._h, n, _ptr(r), _ptr(ptr), _ptr(items), int(workspace_bytes), _ptr(lo), _ptr(pr), C.byref(ms) if want_ms else None))
        return (lo, pr, ms.value) if want_ms else (lo, pr)
