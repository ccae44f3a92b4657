"""Per-element oracle parity for the Flipout KL gradients across rho's range, and Adam from a loaded state at t > 1.

The suite's other Bnn bars (3e-4 of a tensor's largest gradient; parameters after Adam's first step, which sees only the sign of each
gradient) cannot see the KL part of a gradient: klw = kl_share / (n_w * B) puts it orders of magnitude below the data part.  Here every
gradient element gets a bar of its own, derived from the arithmetic, and the parameters the rho grid puts at rho far from the reference init:

- rho on a grid placed per element (every row, unit, tile and bias sees the whole grid): around sigma's series switch (-4.3 .. -4.0), and
  -100 .. 30.  Below rho ~ -17 sigmoid(rho) < 1e-7 and the data part of a rho gradient vanishes: those elements are their KL term alone,
  -klw (sigma - 1/sigma) sigmoid(rho) -> -klw, checked to a few ulp in every layer.
- Each bar is checked against the oracle's own gradients with the KL term doubled, dropped, and sign-flipped: all three must fail it.
- At t > 1 (moments loaded through moment_tensors(), the step counter advanced by steps at lr = 0) Adam's update is proportional to g, so the
  parameter check sees gradient magnitudes, the KL part included.

References: oracle/ntf_oracle.py in float64 on injected noise / negatives, or on the device's own draws replayed through e.noise()."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ntf_oracle as O
from opentf_amd import libntf
from test_gpu_parity import _engine
from test_gpu_shapes import _csr, _d64, _inject, _kink_units, _problem, U

pytestmark = pytest.mark.gpu

RHO_SPREAD = (-100.0, -95.0, -88.0, -87.5, -87.0, -80.0, -60.0, -30.0, -15.0, -10.0, -6.0, -3.0, -1.0, 0.0, 2.0, 10.0, 20.0, 30.0)
RHO_SWITCH = tuple(float(v) for v in np.linspace(-4.3, -4.0, 16))      # the fast finalizers' series / log switch at e = 2^-6 (rho = -4.159)
RHO_GRID = np.array(RHO_SPREAD + RHO_SWITCH)
RHO_HIGH = np.linspace(60.0, 88.0, 15)                                    # sigma eps leaves the fp16 window: the exact-f32 fallback
TPW, TNW, LR, B1, B2, AEPS = 10.0, 1.0, 1e-3, 0.9, 0.999, 1e-8

# bar constants
UP = 8.0 * 2.0 ** -22   # per sqrt(term count): 2^-22 the relative error of an fp16x3 product (ntf_device.h split_pair_h: x = x1 + x2 to 22 bits;
                        # the exact-f32 paths are 4x better), 8 the margin KINK_C gives a rounded sum's spread (test_gpu_shapes.py)
CT = 8.0                # hardware exp2 / log2 / rcp: 1 ulp each, and e^rho carries |rho| ulp of its argument's rounding: CT (4 + |rho|) ulp
SPLIT_LO = 2.0 ** -3    # below 2^-3 (scaled) the lo fp16 plane is subnormal: its absolute step 2^-24 / scale replaces the relative 2^-22
W16, H16 = 256.0, 16.0  # the exact power-of-two scales of the split operands (ntf_engine.hip kW16Scale, kH16Scale)
CLAMP_DZ = 7.6e-10      # the -21 logit clamp of k_out_fwd_h3p moves dz by < 7.6e-10 w / B per expert (ntf_fused.hip)
ADAM_REL = 4e-7         # adam_step's hardware sqrt / rcp: the update to ~3e-7 relative (ntf_device.h)


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    import random
    t, n, r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    yield
    torch.set_rng_state(t); np.random.set_state(n); random.setstate(r)


# ------------------------------------------------------------------------------------------ problems
def _place(shape, grid, salt):
    """grid values placed so that every row, column and 64 x 32 tile holds a mix (steps 3 and 5 are prime to the grid's length)"""
    idx = np.indices(shape)
    k = idx[-1] * 3 + (idx[0] * 5 if len(shape) == 2 else 0) + salt
    return torch.from_numpy(grid[k % len(grid)].astype(np.float32))


def _rho_problem(dims, B, seed, grid, multihot=False, x_scale=0.1):
    """_problem's parameters with rho on the grid and mu from N(0, 0.1) with every 11th element out to |mu| = 3; dense inputs scaled so that
    the hidden activations stay far inside the fp16x3 window (|h| << 4094) at sigma = 30"""
    pb = _problem(dims, B, True, seed, 5, multihot=multihot)
    g = torch.Generator().manual_seed(seed + 1)
    for i in range(len(dims) - 1):
        p = f"layers.{i}."
        for j, k in enumerate(("rho_weight", "rho_bias")):
            pb["sd"][p + k] = _place(tuple(pb["sd"][p + k].shape), grid, 7 * i + j)
        for k in ("mu_weight", "mu_bias"):
            mu = torch.randn(pb["sd"][p + k].shape, generator=g) * 0.1
            flat = mu.view(-1)
            flat[::11] = torch.empty(flat[::11].shape).uniform_(-3.0, 3.0, generator=g)
            pb["sd"][p + k] = mu
    if not multihot:
        pb["X"] = pb["X"] * x_scale
    return pb


# ------------------------------------------------------------------------------------------ float64 oracle and per-element bars
def _kl_grads(sd, B):
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    (O.get_kl_loss(leaf) / B).backward()
    return {k: v.grad for k, v in leaf.items()}


def _floor(a, t):
    """|a|, lifted to t where a != 0: the fp16x3 split's absolute floor expressed in the relative bar's units"""
    m = a.abs()
    return torch.where(m > 0, torch.clamp(m, min=t), m)


def _scales(sd, X, y, neg, nz, tnw=TNW):
    """S, the sum of |terms| of every gradient element: the forward and backward evaluated on absolute values (float64).  The output layer's
    operands are lifted to the split's subnormal threshold; dz carries the forward's error through sigmoid' and the -21 clamp."""
    L = O.n_layers(sd)
    B = X.shape[0]
    fan = B + sum(sd[f"layers.{i}.mu_weight"].shape[1] for i in range(L))
    A, Wabs, Sz, zs = [X.abs()], [], [], []
    x = X
    for i in range(L):
        p = f"layers.{i}."
        sw = O.softplus_rho(sd[p + "rho_weight"]) * nz[i]["eps_w"]
        sb = O.softplus_rho(sd[p + "rho_bias"]) * nz[i]["eps_b"]
        wa, ba, a = sd[p + "mu_weight"].abs() + sw.abs(), sd[p + "mu_bias"].abs() + sb.abs(), A[-1]
        if i == L - 1:
            wa = _floor(sd[p + "mu_weight"], SPLIT_LO / W16) + _floor(sw, SPLIT_LO / W16)
            a = _floor(a, SPLIT_LO / H16)
            A[-1] = a
        Wabs.append(wa)
        Sz.append(a @ wa.T + ba)
        z = O.flipout_linear(x, sd[p + "mu_weight"], sd[p + "rho_weight"], sd[p + "mu_bias"], sd[p + "rho_bias"], nz[i])
        zs.append(z)
        x = F.leaky_relu(z)
        A.append(Sz[-1])
    out = x.detach().clone().requires_grad_(True)
    O.bxe(out, y, neg, TPW, tnw).sum(dim=1).mean().backward()
    cond = y == 1
    if neg is not None:
        cond[torch.arange(B).unsqueeze(1), neg] = True
    wt = torch.where(cond, TPW, tnw)
    dact = torch.where(zs[-1] > 0, 1.0, 0.01)
    dz = out.grad * dact
    s = torch.sigmoid(out.detach())
    t_dz = SPLIT_LO * 2.0 * max(TPW, tnw) / (16384.0 * B)    # dz's scale is 2^floor(log2(16384 B / max(tpw, tnw))) (ntf_engine.hip dz_scale16)
    G = _floor(dz, t_dz) + wt / B * s * (1 - s) * Sz[-1] + (dz != 0) * CLAMP_DZ * wt / B / (UP * fan ** 0.5)
    S = {}
    for i in reversed(range(L)):
        p = f"layers.{i}."
        SW, Sb = G.T @ A[i], G.sum(0)
        sg_w, sg_b = torch.sigmoid(sd[p + "rho_weight"]), torch.sigmoid(sd[p + "rho_bias"])
        S[p + "mu_weight"], S[p + "mu_bias"] = SW, Sb
        S[p + "rho_weight"], S[p + "rho_bias"] = (nz[i]["eps_w"] * sg_w).abs() * SW, (nz[i]["eps_b"] * sg_b).abs() * Sb
        G = G @ Wabs[i]
    return S, fan


def _gbar(S, K, D, rho, fan):
    """|got - ref| <= UP sqrt(fan) S + CT (4 + |rho|) 2^-24 (|K| + |D|) per element"""
    return UP * fan ** 0.5 * S + CT * (4.0 + np.abs(rho)) * U * (np.abs(K) + np.abs(D))


# the engine's Adam takes beta1, beta2 as f32 and 1 - beta from those (ntf_device.h adam_step): 1 - 0.999f = 0.000999987, 1.3e-5 below
# torch's 1e-3, which moves every update by ~6e-6 of itself.  The reference below evaluates the engine's recurrences in float64 with these
# constants, so that its bars can be those of the arithmetic.
C1, C2 = float(np.float32(1) - np.float32(B1)), float(np.float32(1) - np.float32(B2))
B2F = float(np.float32(B2))


def _adam64(p, g, m, v, t, lr):
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    m2 = m + C1 * (g - m)
    v2 = v * B2F + C2 * g * g
    denom = np.sqrt(v2) / np.sqrt(bc2) + AEPS
    upd = lr / bc1 * m2 / denom
    return p - upd, m2, v2, upd, denom


def _adam64_torch(p, g, m, v, t, lr):
    """torch.optim.Adam's update in float64 with the float64 betas"""
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    m2, v2 = B1 * m + (1 - B1) * g, B2 * v + (1 - B2) * g * g
    return p - lr / bc1 * m2 / (np.sqrt(v2) / np.sqrt(bc2) + AEPS)


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _oracle(pb, lr=LR, moments=None, t=1):
    """logits, loss, gradients, their KL parts, per-element gradient bars, and the parameters after one Adam step at step t from the
    given moments (zero by default) with per-element bars"""
    sd = {k: v.double() for k, v in pb["sd"].items()}
    X, y, nz = pb["X"].double(), pb["y"].double(), _d64(pb["noise"])
    B = X.shape[0]
    with torch.no_grad():
        logits = O.model_forward(sd, X, nz).numpy()
        kinks = _kink_units(sd, X, nz)
    tnw = pb.get("tnw", TNW)
    loss, grads = O.loss_and_grads(sd, X, y, pb["neg"], TPW, tnw, nz)
    K = _kl_grads(sd, B)
    S, fan = _scales(sd, X, y, pb["neg"], nz, tnw)
    out = {"logits": logits, "loss": loss, "kinks": kinks, "g": {}, "K": {}, "bar": {}, "new": {}, "pbar": {}, "sd64": sd, "X64": X, "nz64": nz}
    for k in sd:
        g, Kk = grads[k].numpy(), K[k].detach().numpy()
        rho = sd[k.replace("mu_", "rho_")].numpy() if k.split(".")[-1].startswith("rho") else np.zeros_like(g)
        bar = _gbar(S[k].detach().numpy(), Kk, g - Kk, rho, fan)
        m, v = (np.zeros_like(g), np.zeros_like(g)) if moments is None else (moments[0][k], moments[1][k])
        p = sd[k].numpy()
        new, m2, v2, upd, denom = _adam64(p, g, m, v, t, lr)
        # the device's gradient may sit anywhere within its bar: |d update / d g| = (lr / bc1) |(1 - b1) / denom - m' d denom/dg / denom^2|
        # with d denom / dg = (1 - b2) g / (sqrt(bc2) sqrt(v')); both parts bounded separately, times 2 for the second order over the bar
        ddenom = C2 * np.abs(g) / (np.sqrt(1 - B2 ** t) * np.sqrt(np.maximum(v2, 1e-300)))
        sens = lr / (1 - B1 ** t) * (C1 / denom + np.abs(m2) * ddenom / denom ** 2)
        pbar = _ulp(new) + ADAM_REL * np.abs(upd) + 2.0 * sens * bar
        out["g"][k], out["K"][k], out["bar"][k], out["new"][k], out["pbar"][k] = g, Kk, bar, new, pbar
    return out


def _layer(k):
    return int(k.split(".")[1])


def _outside(err, bar, k, kinks):
    bad = err > bar
    bad[kinks[_layer(k)].any(0)] = False      # rows of units within rounding of the leaky_relu kink (test_gpu_shapes.py)
    return bad


MID = (-6.0, 2.0)      # the grid's middle values (the reference init's -3 and the series switch among them)


def _bars_see_the_kl_term(orc, keys, mid_frac=None):
    """the oracle's gradient with its KL part doubled, dropped or sign-flipped fails the bars of each rho_weight tensor in keys.  mid_frac:
    and it fails them on at least that fraction of the elements with rho in MID (where the data part is not 0 in general)"""
    for k in keys:
        g, Kk, bar = orc["g"][k], orc["K"][k], orc["bar"][k]
        rho = orc["sd64"][k].numpy()
        mid = (rho >= MID[0]) & (rho <= MID[1])
        for f in (2.0, 0.0, -1.0):
            bad = _outside(np.abs((g - Kk + f * Kk) - g), bar, k, orc["kinks"])
            assert bad.any(), (k, f, "the bar cannot see the KL term")
            if mid_frac is not None:
                assert bad[mid].mean() >= mid_frac, (k, f, "the bar cannot see the KL term at mid-range rho", float(bad[mid].mean()))


def _check_grads(grads, orc, tag):
    for k, r in orc["g"].items():
        g = grads[k]
        assert np.isfinite(g).all(), (tag, k, "non-finite gradient", int((~np.isfinite(g)).sum()))
        bad = _outside(np.abs(g - r), orc["bar"][k], k, orc["kinks"])
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, np.abs(g - r) / orc["bar"][k], 0)), g.shape)
            rho = orc["sd64"][k.replace("mu_", "rho_")].numpy()[i] if "rho" in k else None
            pytest.fail(f"{tag} {k}: {int(bad.sum())} of {g.size} outside the bar; worst at {i}: got {g[i]!r} ref {r[i]!r} "
                        f"K {orc['K'][k][i]!r} bar {orc['bar'][k][i]!r} rho {rho!r}")


def _check_params(st, orc, tag, keys=None):
    for k in (keys or orc["new"]):
        a, r = st[k], orc["new"][k]
        assert np.isfinite(a).all(), (tag, k, "non-finite parameter", int((~np.isfinite(a)).sum()))
        bad = _outside(np.abs(a - r), orc["pbar"][k], k, orc["kinks"])
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, np.abs(a - r) / orc["pbar"][k], 0)), a.shape)
            pytest.fail(f"{tag} {k}: {int(bad.sum())} of {a.size} outside the bar; worst at {i}: got {a[i]!r} ref {r[i]!r} "
                        f"bar {orc['pbar'][k][i]!r} g {orc['g'][k][i]!r}")


# ------------------------------------------------------------------------------------------ moments
KINDS = (("mu_weight", libntf.P_WEIGHT), ("rho_weight", libntf.P_RHO_WEIGHT), ("mu_bias", libntf.P_BIAS), ("rho_bias", libntf.P_RHO_BIAS))


def _moment_pattern(sd, seed):
    """per element, by index mod 5: m = v = 0; v subnormal; |m| / sqrt(v) = 1; |m| / sqrt(v) = 1e-3; a generic pair"""
    rng = np.random.default_rng(seed)
    M, V = {}, {}
    for k, p in sd.items():
        n = p.numel()
        s = rng.uniform(1e-4, 1e-2, n) * rng.choice([-1.0, 1.0], n)
        m, v = np.zeros(n), np.zeros(n)
        c = np.arange(n) % 5
        m[c == 1], v[c == 1] = s[c == 1] * 1e-3, 1e-40
        m[c == 2], v[c == 2] = s[c == 2], s[c == 2] ** 2
        m[c == 3], v[c == 3] = s[c == 3] * 1e-3, s[c == 3] ** 2
        m[c == 4], v[c == 4] = s[c == 4], np.abs(s[c == 4]) * 1e-2
        M[k] = m.astype(np.float32).reshape(p.shape).astype(np.float64)
        V[k] = v.astype(np.float32).reshape(p.shape).astype(np.float64)
    return M, V


def _transposed(e, l, kind):
    """whether the flat buffers hold this weight as [in, out] (a multi-hot first layer keeps one row per skill): read from the parameters
    once per engine - the parameter view drops the operands a step prefetched, so the first call belongs before the steps (_layouts)"""
    if kind in (libntf.P_BIAS, libntf.P_RHO_BIAS):
        return False
    cache = e.__dict__.setdefault("_kl_layout", {})
    if (l, kind) in cache:
        return cache[(l, kind)]
    o, c = e.param_segment(l, kind)
    flat = e.param_tensor()[o: o + c].cpu().numpy()
    a = e.state_dict()[f"layers.{l}.{dict((k, n) for n, k in KINDS)[kind]}"]
    if np.array_equal(flat, a.reshape(-1)):
        cache[(l, kind)] = False
    else:
        assert np.array_equal(flat, a.T.reshape(-1)), (l, kind, "unknown layout")
        cache[(l, kind)] = True
    return cache[(l, kind)]


def _layouts(e):
    for l in range(e.L):
        for _, kind in KINDS:
            _transposed(e, l, kind)


def _write_moments(e, M, V):
    m, v = e.moment_tensors()
    for l in range(e.L):
        for name, kind in KINDS:
            o, c = e.param_segment(l, kind)
            tr = _transposed(e, l, kind)
            for buf, src in ((m, M), (v, V)):
                a = src[f"layers.{l}.{name}"].astype(np.float32)
                buf[o: o + c].copy_(torch.from_numpy(np.ascontiguousarray(a.T if tr else a).reshape(-1)))
    torch.cuda.synchronize()


def _read_flat(e, t):
    out = {}
    h = t.cpu().numpy()
    for l in range(e.L):
        for name, kind in KINDS:
            o, c = e.param_segment(l, kind)
            shape = e._shape(l, kind)
            a = h[o: o + c]
            out[f"layers.{l}.{name}"] = (a.reshape(shape[::-1]).T if _transposed(e, l, kind) else a.reshape(shape)).copy()
    return out


def _advance(e, rows, inj, steps):
    """steps at lr = 0: the step counter moves on, the parameters do not (bit for bit)"""
    before = e.state_dict()
    e.set_lr(0.0)
    for _ in range(steps):
        e.train_step(rows, inject=inj, want_loss=False)
    after = e.state_dict()
    for k in before:
        assert np.array_equal(before[k], after[k]), (k, "a step at lr = 0 moved a parameter")


def _make(pb, dims, B, bayesian, mode, fuse_adam):
    """test_gpu_shapes._make with the problem's tnw"""
    e = _engine(dims, bayesian=bayesian, input_mode=libntf.INPUT_MULTIHOT if pb["multihot"] else libntf.INPUT_DENSE, max_batch=B, ns=pb["ns"],
                nsd="uniform" if pb["ns"] else None, tpw=TPW, tnw=pb.get("tnw", TNW), lr=LR, fused=mode != "generic",
                mfma="f32" if mode == "f32" else None, fuse_adam=fuse_adam)
    if pb["multihot"]:
        e.set_skill_csr(_csr(pb["X"].numpy()))
    else:
        e.set_dense_input(pb["X"].numpy())
    e.set_member(pb["member"]); e.load_state_dict(pb["sd"])
    return e


# ------------------------------------------------------------------------------------------ 1 + 2: rho across its range, per path
RHO_CASES = {     # name: dims, B, multihot
    "h128": ([64, 128, 20000], 160, False),
    "h128_split": ([64, 128, 3000], 600, False),      # max_batch >= 258 ks: room for the split-K partial slabs (ntf_engine.hip)
    "h128_high": ([64, 128, 3000], 150, False),
    "h128_small": ([64, 128, 300], 40, False),        # just over one 256-expert tile and no multiple of 64, just over one 32-row block
    "h64": ([48, 64, 3000], 150, False),
    "h32": ([40, 32, 2000], 140, False),
    "h256": ([64, 256, 3000], 150, False),
    "h100_generic": ([37, 100, 1001], 130, False),
    "two_hidden": ([64, 96, 128, 3000], 150, False),
}
RHO_RUNS = [   # case, mode, fuse_adam, env
    ("h128", "default", 0, {}), ("h128", "default", 1, {}), ("h128", "default", 2, {}), ("h128_split", "default", 1, {"NTF_DW_KSPLIT": "2"}),
    ("h128", "f32", 1, {}), ("h64", "f32", 1, {}), ("h64", "default", 1, {}), ("h32", "f32", 1, {}), ("h32", "default", 0, {}),
    ("h256", "default", 1, {}), ("h100_generic", "generic", 0, {}), ("two_hidden", "default", 1, {}),
    ("h128_small", "default", 1, {"NTF_FWD_KERNEL": "0"})      # k_out_fwd_b6's training form with d(hidden): the one launch branch of the fused output layer no other test runs
]
_CACHE = {}


def _rho_case(name, grid_name="grid", moments=False, t=1):
    key = (name, grid_name, moments, t)
    if key not in _CACHE:
        _CACHE.clear()
        dims, B, mh = RHO_CASES[name]
        pb = _rho_problem(dims, B, 500 + len(dims) * 10 + dims[-2], RHO_GRID if grid_name == "grid" else RHO_HIGH, multihot=mh)
        mom = _moment_pattern(pb["sd"], 3) if moments else None
        _CACHE[key] = (pb, _oracle(pb, moments=mom, t=t), mom)
    return _CACHE[key]


def _step_and_check(pb, orc, dims, B, mode, fuse_adam, tag, moments=None, t=1, fallback=False):
    rows = np.arange(B)
    inj = _inject(pb["neg"], pb["noise"])
    e = _make(pb, dims, B, True, mode, 0)
    try:
        z = e.logits(rows, inject=inj)
        assert np.isfinite(z).all(), (tag, "non-finite logits")
        zmax = float(np.abs(orc["logits"]).max())
        assert float(np.abs(z - orc["logits"]).max()) <= 1e-4 * zmax, (tag, "logits", float(np.abs(z - orc["logits"]).max()), zmax)
        ev = e.eval_step(rows, inject=inj)
        assert abs(ev - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (tag, "eval loss", ev, orc["loss"])
        loss = e.backward(rows, inject=inj)
        assert abs(loss - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (tag, "loss", loss, orc["loss"])
        _check_grads(e.grads(), orc, tag)
        if mode != "generic":
            assert (e.range_fallbacks() > 0) == fallback, (tag, "range fallbacks", e.range_fallbacks())
    finally:
        e.close()
    e = _make(pb, dims, B, True, mode, fuse_adam)
    try:
        if moments is not None:
            _layouts(e)
            _advance(e, rows, inj, t - 1)
            _write_moments(e, *moments)
            e.set_lr(LR)
        loss = e.train_step(rows, inject=inj)
        assert abs(loss - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (tag, "train loss", loss, orc["loss"])
        _check_params(e.state_dict(), orc, tag)
        if mode != "generic":
            assert (e.range_fallbacks() > 0) == fallback, (tag, "range fallbacks", e.range_fallbacks())
    finally:
        e.close()


@pytest.mark.parametrize("name,mode,fuse_adam,env", [pytest.param(*r, id=f"{r[0]}-{r[1]}-fa{r[2]}" + "".join(f"-{k}{v}" for k, v in r[3].items()))
                                                     for r in RHO_RUNS])
def test_rho_across_its_range_per_element(name, mode, fuse_adam, env, monkeypatch):
    """one injected step with rho on the grid: logits, losses (the KL value included), every gradient at its own bar, the parameters after
    the step; the bars see the KL term of every layer's rho_weight"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dims, B, _ = RHO_CASES[name]
    pb, orc, _ = _rho_case(name)
    _bars_see_the_kl_term(orc, [f"layers.{i}.rho_weight" for i in range(len(dims) - 1)])
    _step_and_check(pb, orc, dims, B, mode, fuse_adam, (name, mode, fuse_adam, tuple(env.items())))


def test_split_k_dw_ran(monkeypatch):
    """NTF_DW_KSPLIT = 2 on h128_split: the dW kernel's K range is split and k_out_dw_finish adds the parts (the runs above check it against the
    oracle); the same sums in another order give other bits than the unsplit kernel somewhere, which shows that the split ran"""
    dims, B, _ = RHO_CASES["h128_split"]
    pb, orc, _ = _rho_case("h128_split")
    inj, g = _inject(pb["neg"], pb["noise"]), {}
    for ks in ("1", "2"):
        monkeypatch.setenv("NTF_DW_KSPLIT", ks)
        e = _make(pb, dims, B, True, "default", 0)
        try:
            e.backward(np.arange(B), inject=inj)
            g[ks] = e.grads()
        finally:
            e.close()
        _check_grads(g[ks], orc, ("ksplit", ks))
    assert not np.array_equal(g["1"]["layers.1.mu_weight"], g["2"]["layers.1.mu_weight"]), "NTF_DW_KSPLIT = 2 did not split the dW kernel"


@pytest.mark.parametrize("t", [2, 1000])
def test_rho_grid_step_from_loaded_moments(t):
    """the fused fp16x3 step at H = 128 (Adam in the dW epilogue) from loaded moments at step t: the update is proportional to g, so the
    parameter bars see the KL part's magnitude on the untouched bulk of the output layer"""
    dims, B, _ = RHO_CASES["h128"]
    pb, orc, mom = _rho_case("h128", moments=True, t=t)
    _bars_see_the_kl_term(orc, ["layers.0.rho_weight", "layers.1.rho_weight"])
    # at t > 1 the parameter bars, not only the gradient bars, reject a KL term doubled / dropped / flipped on the output layer
    k = "layers.1.rho_weight"
    for f in (2.0, 0.0, -1.0):
        g = orc["g"][k] + (f - 1.0) * orc["K"][k]
        new = _adam64(orc["sd64"][k].numpy(), g, mom[0][k], mom[1][k], t, LR)[0]
        assert _outside(np.abs(new - orc["new"][k]), orc["pbar"][k], k, orc["kinks"]).any(), (f, "the parameter bar cannot see the KL term")
    _step_and_check(pb, orc, dims, B, "default", 1, ("h128 loaded", t), moments=mom, t=t)


def test_rho_above_60_runs_the_exact_fallback_and_matches():
    """rho in [60, 88]: sigma eps leaves the fp16 window (|sigma eps| > 255), the H = 128 step falls back to the exact-f32 kernels
    (range_fallbacks() > 0) and still equals the oracle (sigma = rho there, not 80)"""
    dims, B, _ = RHO_CASES["h128_high"]
    pb, orc, _ = _rho_case("h128_high", grid_name="high")
    _step_and_check(pb, orc, dims, B, "default", 1, ("h128 high",), fallback=True)


def test_rho_grid_inference_against_the_oracle():
    """forward(nmc = 2) with injected noise on the grid's parameters: probabilities, predictive entropy and mutual information"""
    dims, B, _ = RHO_CASES["h128"]
    pb, orc, _ = _rho_case("h128")
    rows = np.arange(B)
    noise2 = [pb["noise"], _problem(dims, B, True, 9, 5)["noise"]]
    e = _make(pb, dims, B, True, "default", 1)
    try:
        probs, pu, mi = e.forward(rows, nmc=2, injects=[_inject(None, n) for n in noise2], uncertainty=True)
    finally:
        e.close()
    with torch.no_grad():
        mc = O.predict(orc["sd64"], orc["X64"], 2, [_d64(n) for n in noise2]).numpy().reshape(2, B, -1)
        zmax = max(float(np.abs(O.model_forward(orc["sd64"], orc["X64"], _d64(n)).numpy()).max()) for n in noise2)
    ref = mc.mean(0)
    tol = np.maximum(mc * (1 - mc), 0).max(0) * 1e-4 * zmax + 2e-7       # the logit bar 1e-4 max|z| through sigmoid'
    assert np.isfinite(probs).all() and (np.abs(probs - ref) <= tol).all(), ("probs", float((np.abs(probs - ref) / tol).max()))
    ent_tol = 1e-4 * np.abs(O.predictive_entropy(mc)) + (np.abs(np.log(ref + 1e-15) + 1.0) * tol).sum(1) + 1e-6
    assert (np.abs(pu - O.predictive_entropy(mc)) <= ent_tol).all(), "predictive entropy"
    assert (np.abs(mi - O.mutual_information(mc)) <= 2 * ent_tol).all(), "mutual information"


def test_multihot_first_layer_on_the_rho_grid(monkeypatch):
    """a multi-hot first layer (S = 700) with rho on the grid, at NTF_L0_SWEEP = 1 (k_flipout_sweep: finalize + Adam + next operand in one
    pass) and 0 (k_flipout_grad_finalize + the flat Adam + the stand-alone producer).  Two staged steps at lr = 0, moments written through the
    view, one staged step at t = 3 on the device's own draws, replayed through the float64 oracle: loss (the KL value the producers summed),
    every parameter at its bar; the bars see the first layer's KL term in gradient and parameter."""
    dims, B, seed, t0, t = [700, 128, 1500], 90, 61, 5, 3
    pb = _rho_problem(dims, B, seed, RHO_GRID, multihot=True)
    mom = _moment_pattern(pb["sd"], 5)
    res = {}
    for sweep in ("1", "0"):
        monkeypatch.setenv("NTF_L0_SWEEP", sweep)
        e = _make(pb, dims, B, True, "default", 1)
        try:
            _layouts(e)
            e.set_seed(seed, t0); e.stage_order(np.arange(B, dtype=np.int64))
            p0 = e.state_dict()
            e.set_lr(0.0)
            for _ in range(t - 1):
                e.step_staged(0, B, train=True, apply=True)
            for k, v in e.state_dict().items():
                assert np.array_equal(v, p0[k]), (k, "a step at lr = 0 moved a parameter")
            _write_moments(e, *mom)
            e.set_lr(LR)
            sw0 = e.first_layer_sweeps()
            loss = e.step_staged(0, B, train=True, apply=True, want_loss=True)
            e.synchronize()
            m_t, v_t = e.moment_tensors()
            res[sweep] = (loss, e.negatives(B).copy(), e.noise(t0 + t - 1, B), e.state_dict(), _read_flat(e, m_t), _read_flat(e, v_t))
            assert e.first_layer_sweeps() - sw0 == (1 if sweep == "1" else 0), (sweep, "sweeps")
            assert e.range_fallbacks() == 0, (sweep, e.range_fallbacks())
        finally:
            e.close()
    for sweep, (loss, neg, nz, st, _, _) in res.items():
        pb2 = dict(pb, noise=[{k: torch.from_numpy(v) for k, v in n.items()} for n in nz], neg=torch.from_numpy(neg.astype(np.int64)))
        orc = _oracle(pb2, moments=mom, t=t)
        assert abs(loss - orc["loss"]) <= 2e-5 * abs(orc["loss"]), (sweep, loss, orc["loss"])
        _bars_see_the_kl_term(orc, ["layers.0.rho_weight", "layers.1.rho_weight"])
        k = "layers.0.rho_weight"
        for f in (2.0, 0.0, -1.0):      # at t = 3 from loaded moments the first layer's parameter bars see its KL term as well
            new = _adam64(orc["sd64"][k].numpy(), orc["g"][k] + (f - 1.0) * orc["K"][k], mom[0][k], mom[1][k], t, LR)[0]
            assert _outside(np.abs(new - orc["new"][k]), orc["pbar"][k], k, orc["kinks"]).any(), (f, "the parameter bar cannot see the KL term")
        _check_params(st, orc, ("multihot", sweep))


def test_next_step_operands_from_the_epilogue():
    """a native fused step (Adam in the dW epilogue, which also writes the NEXT step's sigma eps planes and KL from the updated rho through
    softplus_rho_fast) on the rho grid; the next step's loss, on the device's own draws replayed through e.noise(), equals the oracle's at the
    updated parameters"""
    dims, B, _ = RHO_CASES["h128_split"]
    pb, _, _ = _rho_case("h128_split")
    seed, t0 = 17, 3
    e = _make(pb, dims, B, True, "default", 1)
    try:
        e.set_seed(seed, t0); e.stage_order(np.arange(B, dtype=np.int64))
        e.step_staged(0, B, train=True, apply=True)
        st1 = e.state_dict()
        pre0 = e.prefetched_steps()
        loss2 = e.step_staged(0, B, train=True, apply=True, want_loss=True)
        neg2, nz2 = e.negatives(B).copy(), e.noise(t0 + 1, B)
        assert e.prefetched_steps() - pre0 == 1, "the second step did not start on the epilogue's operands"
        assert e.range_fallbacks() == 0, e.range_fallbacks()
    finally:
        e.close()
    sd = {k: torch.from_numpy(v).double() for k, v in st1.items()}
    nz = [{k: torch.from_numpy(v).double() for k, v in n.items()} for n in nz2]
    ref = O.batch_loss(sd, pb["X"].double(), pb["y"].double(), torch.from_numpy(neg2.astype(np.int64)), TPW, TNW, nz).item()
    assert abs(loss2 - ref) <= 2e-5 * abs(ref), (loss2, ref)


# ------------------------------------------------------------------------------------------ 3. Adam from a loaded state
ADAM_DIMS, ADAM_B = [64, 128, 3000], 120


def _adam_engine(pb, fuse_adam):
    return _make(pb, ADAM_DIMS, ADAM_B, True, "default", fuse_adam)


@pytest.mark.parametrize("t", [2, 10, 1000])
@pytest.mark.parametrize("lr", [1e-3, 1e-5])
def test_flat_adam_from_loaded_moments_against_float64(t, lr):
    """apply() on a gradient written through grad_view(), from moments written through moment_tensors() at step t: p, m and v per element
    against float64 Adam (p within ulp(p) / 2 + 4e-7 |update|, ntf_device.h, plus the rounding of m'); where m = v = g = 0, p does not move.  apply_ranges() over
    pieces of the flat buffer from the same state gives the same bits."""
    pb = _problem(ADAM_DIMS, ADAM_B, True, 71, 5)
    rows, inj = np.arange(ADAM_B), _inject(pb["neg"], pb["noise"])
    M, V = _moment_pattern(pb["sd"], t)
    rng = np.random.default_rng(t)
    G = {}
    for k, p in pb["sd"].items():
        g = (rng.standard_normal(p.shape) * 10.0 ** rng.integers(-9, -1, p.shape)).astype(np.float32)
        g.reshape(-1)[::5] = 0.0                               # with m = v = 0 (index mod 5 == 0): no update at all
        G[k] = g
    outs = []
    for ranged in (False, True):
        e = _adam_engine(pb, 0)
        try:
            _layouts(e)
            _advance(e, rows, inj, t - 1)
            p0 = e.state_dict()
            _write_moments(e, M, V)
            e.set_lr(lr)
            gt = e.grad_tensor()
            for l in range(e.L):
                for name, kind in KINDS:
                    o, c = e.param_segment(l, kind)
                    gt[o: o + c].copy_(torch.from_numpy(G[f"layers.{l}.{name}"].reshape(-1)))
            torch.cuda.synchronize()
            if ranged:
                n = gt.numel()
                cuts = [0, 4, 1000, n // 3 & ~3, n // 2 & ~3, n]     # (ranges start 16-byte aligned)
                e.apply_ranges([(a, b) for a, b in zip(cuts[:-1], cuts[1:])])
            else:
                e.apply()
            e.synchronize()
            m_t, v_t = e.moment_tensors()
            outs.append((e.state_dict(), _read_flat(e, m_t), _read_flat(e, v_t)))
        finally:
            e.close()
    (st, m1, v1), (st_r, m1_r, v1_r) = outs
    for k in st:
        assert np.array_equal(st[k], st_r[k]) and np.array_equal(m1[k], m1_r[k]) and np.array_equal(v1[k], v1_r[k]), (k, "apply_ranges != apply")
        p = p0[k].astype(np.float64)
        new, m2, v2, upd, denom = _adam64(p, G[k].astype(np.float64), M[k], V[k], t, lr)
        err = np.abs(st[k] - new)
        # ntf_device.h's bound, plus m' = m + (1 - b1)(g - m) rounded on the scale of |m| + |g|: where m' cancels, that rounding is not
        # relative to m' and passes into the update as (lr / bc1) dm' / denom
        dm = 2 * _ulp(np.abs(M[k]) + np.abs(G[k].astype(np.float64)))
        bar = 0.5 * _ulp(new) + ADAM_REL * np.abs(upd) + lr / (1 - B1 ** t) * dm / denom
        assert (err <= bar).all(), (k, t, lr, int((err > bar).sum()), float((err / np.maximum(bar, 1e-45)).max()))
        g64 = G[k].astype(np.float64)
        # m + (1 - b1)(g - m): three roundings on the scale of |m| + |g| (m' itself may cancel); v b2 + (1 - b2) g g: positive terms
        assert (np.abs(m1[k] - m2) <= 2 * _ulp(np.abs(M[k]) + np.abs(g64)) + 2.0 ** -149).all(), (k, "m")
        assert (np.abs(v1[k] - v2) <= 4 * _ulp(v2) + 2.0 ** -149).all(), (k, "v")
        # against torch.optim.Adam's constants (1 - beta from the float64 betas): the engine's 1 - 0.999f is 1.3e-5 below 1e-3, which may move
        # an update by up to 6.5e-6 of itself (sqrt of v's share) - a bound on that deviation, not part of the reference above
        tor = _adam64_torch(p, G[k].astype(np.float64), M[k], V[k], t, lr)
        assert (np.abs(st[k] - tor) <= bar + 6.5e-6 * np.abs(upd)).all(), (k, "deviation from torch's Adam constants")
        still = (M[k] == 0) & (V[k] == 0) & (G[k] == 0)
        assert np.array_equal(st[k][still], p0[k][still]), (k, "p moved where m = v = g = 0")


@pytest.mark.parametrize("t", [2, 1000])
def test_fused_adam_paths_equal_the_flat_path_bit_for_bit_from_loaded_moments(t):
    """fuse_adam = 1 (Adam in the dW epilogue) and 2 (the flat Adam kernel, chunked beside the dW kernel) from a loaded state at step t equal
    fuse_adam = 0 bit for bit: every path calls adam_step on the same gradient (the output rho bias under fuse_adam 1: see below); a later step of each, with moments written through the view
    between the fused steps, still agrees (no path keeps state derived from the moments it read before)"""
    pb = _problem(ADAM_DIMS, ADAM_B, True, 72, 5)
    rows, inj = np.arange(ADAM_B), _inject(pb["neg"], pb["noise"])
    M, V = _moment_pattern(pb["sd"], 11)
    M2, V2 = _moment_pattern(pb["sd"], 12)
    res = {}
    for fa in (0, 1, 2):
        e = _adam_engine(pb, fa)
        try:
            _layouts(e)
            _advance(e, rows, inj, t - 1)
            _write_moments(e, M, V)
            e.set_lr(LR)
            e.train_step(rows, inject=inj)
            s1 = e.state_dict()
            _write_moments(e, M2, V2)
            e.train_step(rows, inject=inj)
            e.synchronize()
            m_t, v_t = e.moment_tensors()
            res[fa] = (s1, e.state_dict(), _read_flat(e, m_t), _read_flat(e, v_t))
        finally:
            e.close()
    for k in res[0][0]:
        for j in range(4):
            for fa in (1, 2):
                a, b = res[fa][j][k], res[0][j][k]
                if fa == 1 and k == "layers.1.rho_bias":
                    # the one exception: fuse_adam 1 finalizes the output layer's raw rho-bias gradient inside k_adam_ranges (fin_rho),
                    # fuse_adam 0 in k_flipout_grad_finalize; the same expression g z sg + klw kl_a kl_b, contracted into an fma by the
                    # compiler in a different order in the two kernels: g may differ by an ulp, and with it m' by (1 - b1) ulp(g) - on the
                    # scale of the tensor's largest moment, not of m' itself, where m' cancels - v' and p by their rounding
                    assert (np.abs(a - b) <= 2 * _ulp(np.abs(b).max())).all(), (k, j, "fuse_adam 1 vs 0 beyond 2 ulp of the tensor's scale")
                    continue
                assert np.array_equal(a, b), (k, ("p1", "p2", "m2", "v2")[j], f"fuse_adam {fa} != fuse_adam 0", int((a != b).sum()),
                                              float(np.abs(a - b).max()))
