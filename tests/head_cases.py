"""Cases for the one-kernel step head (opentf_amd/csrc/ntf_head.hip, `k_head`) against the float64 oracle.
TEST INFRASTRUCTURE ONLY, CPU only: shared by tests/test_head_parity_host.py (which asserts that every case is what it claims to be and that the
reference alone clears the bars) and tests/test_gpu_head_parity.py (which compares the device with the oracle on them).  Deterministic: fixed
seeds, no files.

`k_head` is instantiated for d = 64, 128, 256, with and without Flipout, and reads mean-pooled or dense rows; the engine takes it only when no
random tensor is injected.  A case is small and still reaches both lane halves (kb = half * D / 2), a ragged and a full 32-row block, more than
one row block, every M % 4 (the bias workgroups' scalar tail) and CSR rows of one, two and three sub-groups of G = D / 4 lanes, with more and
fewer than 8 skills inside a sub-group.

`problem(name)` builds a case once per process (treat it as read-only) in the layout tests/test_gpu_shapes.py::_oracle takes, with the host's
own noise and negatives; the GPU test replaces those two by the device's draws."""
import functools

import numpy as np
import torch

H, S, NS, TPW, TNW = 128, 300, 5, 10.0, 1.0
SEED = 7
SHAPES = {64: (33, 1501), 128: (31, 1502), 256: (65, 1503)}      # D: (B, M) of the cross product


def _cases():
    shapes = [(D, B, M, bay, inp) for D, (B, M) in SHAPES.items() for bay in (True, False) for inp in ("meanpool", "dense")]
    shapes += [(D, B, M, True, "meanpool") for D, B, M in ((64, 1, 1501), (256, 32, 1504), (128, 96, 1501))]      # one live row; one full block and M % 4 == 0; three full blocks
    return {f"d{D}-{'bnn' if bay else 'fnn'}-{inp}-B{B}-M{M}": {"dims": [D, H, M], "bayesian": bay, "input": inp, "B": B, "seed": SEED, "ns": NS, "tpw": TPW, "tnw": TNW}
            for D, B, M, bay, inp in shapes}


CASES = _cases()
NAMES = list(CASES)


def row_lengths(D):
    """the skill counts the teams cycle through: below, at and above the 8 table rows a sub-group keeps in flight, and one, two and three sub-groups"""
    G = D // 4
    return [1, 8, 9, G, G + 1, 2 * G + 3]


@functools.lru_cache(maxsize=None)
def problem(name):
    """parameters (the reference's init), the skill CSR and table, the batch's team ids, the mean-pooled input, member CSR and dense labels, and one
    set of Flipout noise and negatives drawn on the host"""
    from conftest import draw_noise
    from oracle import ntf_oracle as O
    c = CASES[name]
    (D, _, M), B, seed, ns = c["dims"], c["B"], c["seed"], c["ns"]
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    N = 2 * B
    sd = O.bnn_init(D, [H], M) if c["bayesian"] else O.fnn_init(D, [H], M)
    cyc = row_lengths(D)
    nnz = np.array([cyc[i % len(cyc)] for i in range(N)])
    s_ip = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
    s_ix = np.concatenate([np.sort(rng.choice(S, k, replace=False)) for k in nnz]).astype(np.int32)
    table = rng.standard_normal((S, D)).astype(np.float32)
    rows = rng.permutation(N)[:B].astype(np.int64)
    Xall = O.gather_meanpool_fast(s_ip, s_ix, table)
    mn = np.minimum(1 + rng.poisson(2.0, N), M - ns)
    m_ip = np.concatenate([[0], np.cumsum(mn)]).astype(np.int64)
    m_ix = np.concatenate([np.sort(rng.choice(M, k, replace=False)) for k in mn]).astype(np.int32)
    y = torch.zeros(B, M)
    for t, r in enumerate(rows): y[t, m_ix[m_ip[r]: m_ip[r + 1]].astype(np.int64)] = 1.0
    noise = draw_noise(sd, B) if c["bayesian"] else None
    neg = O.ns_uniform(y, ns)
    for a in (s_ip, s_ix, table, rows, Xall, m_ip, m_ix): a.setflags(write=False)
    return {"sd": sd, "X": torch.from_numpy(Xall[rows]), "y": y, "noise": noise, "neg": neg, "ns": ns,
            "skill": (s_ip, s_ix), "table": table, "Xall": Xall, "rows": rows, "member": (m_ip, m_ix), "nnz": nnz[rows]}


def kink_counts(kinks):
    """(hidden units, experts) with a pre-activation within rounding of leaky_relu's kink in any row: the units _check_grads exempts"""
    return int(kinks[0].any(0).sum()), int(kinks[1].any(0).sum())


def kink_caps(M):
    return 3, M // 100      # at most 3 of the 128 hidden units, at most 1 % of the experts


def worst_errors(loss, grads, orc):
    """measurements for profiles/head_parity_check.md: the loss's relative error and every gradient's largest error outside the kink units, as a
    share of its tensor's maximum (the quantities held to 2e-5 and 3e-4)"""
    out = {"loss": abs(loss - orc["loss"]) / abs(orc["loss"])}
    for k, r in orc["grads"].items():
        flip = orc["kinks"][int(k.split(".")[1])].any(0)
        out[k] = float(np.abs(np.asarray(grads[k], np.float64) - r)[~flip].max() / np.abs(r).max())
    return out


def with_draws(pb, noise, neg):
    """the same problem on other draws (the device's own): noise as ntf_get_noise returns it, neg [B, ns] int64"""
    out = dict(pb)
    out["noise"] = None if noise is None else [{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in n.items()} for n in noise]
    out["neg"] = torch.from_numpy(np.ascontiguousarray(neg).astype(np.int64))
    return out
