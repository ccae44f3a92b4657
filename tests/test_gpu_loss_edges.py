"""The loss side of the engine against the float64 oracle away from its one well-trodden operating point (tpw = 10, tnw = 1, ns <= 5, rows of
a few positives): other weights (tnw != 1, tnw > tpw, tnw = 0, a ratio of 1 000), ns of 9 and 12 (the samplers and the duplicate scans keep 8
entries in registers), and label rows that no other module holds up to the oracle - no positives, 8 / 9 / 65 / 70 positives, and rows with exactly,
fewer than, and no negatives at all (the reference's rand + topk then selects positives, src/mdl/fnn.py:54: such a pick stays the positive it is).

A. one injected step per (width, engine mode, weights): d loss / d z of the output layer for EVERY element, the losses, every gradient, the parameters
   after the default fused-Adam step.  B. the native samplers on the same rows, their draws fed back through the oracle.  C. the default pipeline
   (native draws replayed) and two expert shards at such weights, once each.

Bars.  dz: |dz - ref| <= 1e-4 |ref| + 1e-12, the bar test_gpu_round2.py holds H = 128 to - the logits bar carried through the loss (|d ln dz / dl| <= 1
for either label, so a relative error of dz is at most the absolute error of its logit); where ref is exactly 0 (tnw = 0 off the specials) the device
value must be exactly 0.  Only elements the oracle marks as kink units of the LAST layer (|z| within the rounding scale of its sum, test_gpu_shapes.py)
may exceed it, and the exclusions are capped on the oracle's side before any device value is looked at: at most 2 % of a layer's units, at most 0.05 % of
the B x M elements, and no special (positive or selected negative) of the edge rows 0 to 7 among them.  Losses 2e-5 relative, gradients and parameters
as test_gpu_shapes.py has them (its 2e-4 fraction budget unchanged).
Measured on an MI355X (every case prints its own with pytest -s): the worst |dz - ref| outside the kink units is 0.029 of the bar (h256 / Bnn), 0.012 at
h128, below 0.008 elsewhere, at every weight pair alike."""
import numpy as np
import pytest
import torch

from opentf_amd import libntf
from oracle import ntf_oracle as O
from test_gpu_replay import _replay
from test_gpu_round2 import _oracle_last_preact
from test_gpu_shapes import _global_generators_left_as_found  # noqa: F401  (autouse here too: this module seeds and draws from the global generators)
from test_gpu_shapes import _expert_shard_step, _inject, _oracle, _problem, _run

pytestmark = pytest.mark.gpu

SEED, LABEL_SEED = 31, 131
EDGE_ROWS = 8
KINK_UNIT_CAP, KINK_DZ_CAP = 0.02, 5e-4
WEIGHTS_FULL = ((10.0, 1.0), (1.0, 1.0), (3.0, 0.5), (1.0, 4.0), (5.0, 0.0), (10.0, 0.01))     # control, the plugin's default, ..., tnw above tpw, no dense term, ratio 1 000
WEIGHTS_TWO = ((3.0, 0.5), (1.0, 4.0))
CASES = {       # name: dims, B, ns, engine modes, weights.  M = 1 001: a ragged 32-, 128- and 256-expert tile; B = 131: a ragged row block
    "h128": ([48, 128, 1001], 131, 12, ("default", "f32", "generic"), WEIGHTS_FULL),
    "h64": ([48, 64, 1001], 131, 9, ("default", "generic"), WEIGHTS_TWO),
    "h96": ([48, 96, 1001], 131, 9, ("default",), WEIGHTS_TWO),
    "h256": ([48, 256, 1001], 131, 9, ("default",), WEIGHTS_TWO),
    "h100": ([37, 100, 300], 70, 12, ("default",), WEIGHTS_FULL),          # the generic chain: k_loss_dense + k_loss_special
    "no_hidden": ([48, 300], 70, 9, ("default",), WEIGHTS_TWO),
}
# _problem's seed.  Rows 1, 2 and 7 are specials in (nearly) every column, so a kink-marked element of the output layer in one of these rows is a special
# whatever the label seed is: h256 / Fnn has one at seed 31 (row 7, expert 414) and takes the next seed, checked the same way (test_loss_edges_host.py)
PROBLEM_SEED = {"h256": 32}
NO_NEGATIVES = ("h128", "h100")      # these two once more with nsd = None / ns = 0, at (3, 0.5)


def edge_labels(B, M, ns, seed=LABEL_SEED):
    """member CSR and dense labels: min(1 + Poisson(2), M) positives a row, rows 0 to 7 overwritten with 0, M - 2, M, 70, 65, 9, 8 and M - ns
    positives (no positives; fewer negatives than ns; none; two trips of a 64-lane loop; one past it; one past / exactly the 8 register slots of
    the samplers; exactly ns negatives).  Columns without replacement from a seeded numpy generator."""
    assert B >= EDGE_ROWS and M >= 70 + ns
    rng = np.random.default_rng(seed)
    mn = np.minimum(1 + rng.poisson(2.0, B), M)
    mn[:EDGE_ROWS] = [0, M - 2, M, 70, 65, 9, 8, M - ns]
    m_ip = np.concatenate([[0], np.cumsum(mn)]).astype(np.int64)
    m_ix = np.concatenate([np.sort(rng.choice(M, k, replace=False)) for k in mn]).astype(np.int32)
    y = torch.zeros(B, M)
    y[np.repeat(np.arange(B), mn), m_ix.astype(np.int64)] = 1.0
    return (m_ip, m_ix), y


def _specials(y, neg):
    """[B, M] bool: the positives and the selected negatives"""
    sp = y.numpy() != 0
    if neg is not None: sp[np.arange(len(sp))[:, None], np.asarray(neg)] = True
    return sp


def _dz_reference(orc, y, neg, tpw, tnw):
    """d loss / d z of the output layer, float64 autograd (the construction of test_training_forward_kernel_dlogits_and_logits_elementwise)"""
    z, logit = _oracle_last_preact(orc["sd64"], orc["X64"], orc["nz64"])
    loss = O.bxe(logit, y.double(), neg, tpw, tnw).sum(dim=1).mean()
    (dz,) = torch.autograd.grad(loss, z)
    return dz.numpy()


def _kink_caps(kinks, special, tag):
    """the conditions on the exclusions, on the oracle's side alone"""
    for l, k in enumerate(kinks):
        assert float(k.any(0).mean()) <= KINK_UNIT_CAP, (tag, "layer", l, "kink-marked units", int(k.any(0).sum()), k.shape[1])
    assert float(kinks[-1].mean()) <= KINK_DZ_CAP, (tag, "kink-marked dz elements", int(kinks[-1].sum()), kinks[-1].size)
    hit = kinks[-1][:EDGE_ROWS] & special[:EDGE_ROWS]
    assert not hit.any(), (tag, "a special of the edge rows is kink-marked: change the label seed", np.argwhere(hit).tolist())


def _check_dz(dz, ref, kink, special, tag):
    dz = dz.astype(np.float64)
    assert dz.shape == ref.shape, (tag, dz.shape, ref.shape)
    tol = 1e-4 * np.abs(ref) + 1e-12
    err = np.abs(dz - ref)
    bad = err > tol
    sb = bad[:EDGE_ROWS] & special[:EDGE_ROWS]      # (none of them is kink-marked: _kink_caps)
    assert not sb.any(), (tag, "specials of the edge rows (row, column, dz, ref)", [(int(r), int(c), dz[r, c], ref[r, c]) for r, c in np.argwhere(sb)[:12]])
    out = bad & ~kink
    assert not out.any(), (tag, "dz", int(out.sum()), "rows", np.unique(np.nonzero(out)[0])[:12].tolist(), "special" if (out & special).any() else "dense",
                           "worst |err| / tol", float((err / tol)[out].max()), [(int(r), int(c), dz[r, c], ref[r, c]) for r, c in np.argwhere(out)[:4]])
    zero = ref == 0
    assert (dz[zero] == 0).all(), (tag, "dz not exactly 0 where the oracle's is", int((dz[zero] != 0).sum()))
    return float((err / tol)[~kink].max())


# ------------------------------------------------------------------------------------------ the problems and their oracles (host only)
_PB, _ORC = {}, {}


def _edge_problem(name, bayesian, ns):
    """_problem's parameters, inputs and Flipout noise (seed 31) under the edge-row labels, negatives by the oracle's rand + topk on those labels"""
    key = (name, bayesian, ns)
    if key not in _PB:
        _PB.clear()
        dims, B = CASES[name][0], CASES[name][1]
        pb = _problem(dims, B, bayesian, PROBLEM_SEED.get(name, SEED), ns)
        pb["member"], pb["y"] = edge_labels(B, dims[-1], ns)
        pb["neg"] = O.ns_uniform(pb["y"], ns) if ns else None
        _PB[key] = pb
    return _PB[key]


def _edge_case(name, bayesian, ns, tpw, tnw):
    """problem, oracle, dz reference and special mask of one (case, bayesian, ns, weights), kept for the consecutive engine modes; the caps on the
    kink exclusions are asserted here, before any engine exists"""
    key = (name, bayesian, ns, tpw, tnw)
    if key not in _ORC:
        _ORC.clear()
        pb = _edge_problem(name, bayesian, ns)
        orc = _oracle(pb, tpw, tnw)
        special = _specials(pb["y"], pb["neg"])
        _kink_caps(orc["kinks"], special, key)
        _ORC[key] = (pb, orc, _dz_reference(orc, pb["y"], pb["neg"], tpw, tnw), special)
    return _ORC[key]


# ------------------------------------------------------------------------------------------ A. one injected step, element-wise and whole
def _wid(w):
    return f"tpw{w[0]:g}-tnw{w[1]:g}"


A_PARAMS = [pytest.param(name, bay, ns, w, mode, id=f"{name}-{'bnn' if bay else 'fnn'}-{_wid(w)}-{mode}")
            for name, (_, _, ns, modes, weights) in CASES.items() for bay in (True, False) for w in weights for mode in modes]
A_PARAMS += [pytest.param(name, bay, 0, (3.0, 0.5), "default", id=f"{name}-{'bnn' if bay else 'fnn'}-{_wid((3.0, 0.5))}-no_negatives")
             for name in NO_NEGATIVES for bay in (True, False)]


@pytest.mark.parametrize("name,bayesian,ns,weights,mode", A_PARAMS)
def test_injected_step_at_other_weights_ns_and_row_shapes(name, bayesian, ns, weights, mode):
    dims, B = CASES[name][0], CASES[name][1]
    tpw, tnw = weights
    pb, orc, dz_ref, special = _edge_case(name, bayesian, ns, tpw, tnw)
    tag = (name, "bnn" if bayesian else "fnn", ns, weights, mode)

    def dz_of_the_backward(e):
        worst = _check_dz(e.dlogits(B), dz_ref, orc["kinks"][-1], special, tag)
        print(tag, "loss", orc["loss"], "max |dz|", float(np.abs(dz_ref).max()), "worst |dz - ref| / bar outside the kink units", worst)

    _run(pb, orc, dims, B, bayesian, mode, inference=False, tpw=tpw, tnw=tnw, after_backward=dz_of_the_backward)


# ------------------------------------------------------------------------------------------ B. the native samplers on the same rows
@pytest.mark.parametrize("nsd", ["uniform", "unigram", "unigram_b"])
def test_native_samplers_on_the_edge_rows_fed_back_through_the_oracle(nsd):
    """40 backward steps of a Bnn [48, 128, 300] on injected Flipout noise and the device's OWN negatives, ns = 12 (picks 9 to 12 and positives 9 and up
    live in memory, not in RowSet's registers).  Every row: ns distinct ids; a row with at least ns admissible experts (non-members, of weight > 0
    for the weighted samplers) picks admissible ones only, a row with fewer takes all of them (but a weighted row without any: the reference falls
    back to uniform over all columns, src/mdl/fnn.py:67-69).  Then the loss and dz of that same step against the oracle on those negatives."""
    dims, B, ns, tpw, tnw, steps = [48, 128, 300], 70, 12, 3.0, 0.5, 40
    M = dims[-1]
    pb = _problem(dims, B, True, SEED, ns)
    pb["member"], pb["y"] = edge_labels(B, M, ns)
    pb["neg"] = None
    orc = _oracle({**pb, "neg": None}, tpw, tnw)           # (logits, kinks and the float64 operands: the loss with negatives is formed per step below)
    Y = pb["y"].numpy() != 0
    w = np.ones(M) if nsd == "uniform" else Y.sum(0) / B
    e = libntf.Engine(dims, bayesian=True, input_mode=libntf.INPUT_DENSE, max_batch=B, ns=ns, nsd=nsd, tpw=tpw, tnw=tnw, lr=1e-3, fuse_adam=0)
    e.set_dense_input(pb["X"].numpy()); e.set_member(pb["member"]); e.load_state_dict(pb["sd"])
    if nsd == "unigram": e.set_unigram(w)
    inj = _inject(None, pb["noise"])
    z, logit = _oracle_last_preact(orc["sd64"], orc["X64"], orc["nz64"])
    kl = float(O.get_kl_loss(orc["sd64"])) / B
    y64 = pb["y"].double()
    seen, few_rows = set(), 0
    try:
        e.set_seed(5, 0)
        for step in range(steps):
            loss = e.backward(np.arange(B), inject=inj)
            neg = e.negatives(B)
            dz = e.dlogits(B)
            assert neg.min() >= 0 and neg.max() < M, (nsd, step, int(neg.min()), int(neg.max()))
            for r in range(B):
                picks = neg[r]
                assert len(set(picks.tolist())) == ns, (nsd, step, r, picks)
                adm = (w > 0) & ~Y[r]
                if adm.sum() >= ns: assert adm[picks].all(), (nsd, step, r, picks)
                elif nsd != "uniform" and adm.sum() == 0: continue
                else:
                    few_rows += 1
                    assert adm[picks].sum() == adm.sum(), (nsd, step, r, picks, np.nonzero(adm)[0])
            seen.add(neg.tobytes())
            negt = torch.from_numpy(neg)
            special = _specials(pb["y"], negt)
            _kink_caps(orc["kinks"], special, (nsd, step))
            ref_loss = float(O.bxe(logit, y64, negt, tpw, tnw).sum(dim=1).mean()) + kl
            assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (nsd, step, loss, ref_loss)
            _check_dz(dz, _dz_reference(orc, pb["y"], negt, tpw, tnw), orc["kinks"][-1], special, (nsd, step))
    finally:
        e.close()
    assert len(seen) == steps, (nsd, "steps repeated their draws", len(seen))
    assert few_rows >= steps, (nsd, few_rows)              # row 1 (two negatives) every step; row 2 (none) for the uniform sampler too


# ------------------------------------------------------------------------------------------ C. the default pipeline and expert shards, once each
def test_three_default_steps_replayed_at_other_weights_and_ns():
    """the head prefetch, the prefetched unigram_b table and the dW-epilogue Adam at tpw = 3, tnw = 0.5, ns = 9 (test_gpu_replay.py's bars)"""
    _replay(D=128, H=128, M=20_001, B=129, S=900, mean_s=5.0, mean_m=2.5, seed=29, t0=6, nsd="unigram_b", ns=9, tpw=3.0, tnw=0.5)


def test_expert_shards_on_the_edge_rows_with_tnw_above_tpw():
    """[48, 128, 2 x 512] in two expert shards, B = 131, the edge-row labels, (tpw, tnw) = (1, 4), ns = 12, native draws: the specials of a row fall into
    both shards, rows 1 and 2 draw positives"""
    dims, B, ns = [48, 128, 1024], 131, 12

    def caps(pb, orc):
        _kink_caps(orc["kinks"], _specials(pb["y"], pb["neg"]), "shards")

    _expert_shard_step(dims, B, 1.0, 4.0, ns, labels=edge_labels(B, dims[-1], ns), before_compare=caps)
