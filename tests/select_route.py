"""A numpy model of the decisions select_topk_row (opentf_amd/csrc/ntf_select.h) makes on a row of reference values - whether the sampled route is entered, the
sample columns, r, the threshold and the number of eligible values above it - and the sims-grid arithmetic of opentf_amd/csrc/ntf_sims.h (sims_lds, per_cu, the grid
width, SimsPlan) as plain functions.  Not a model of the selection's result: tests/test_gpu_long_ranges.py uses it to state which path a case runs, and
tests/test_select_route_host.py to show that the f64 reference alone decides that path.  No GPU.

The constants are read out of the two headers, and the lines that hold the decisions are asserted to stand there as modelled: a changed constant or rule fails here.

Why a margin decides the route.  The device's row is within e of the reference row, value by value.  An order statistic moves by at most the largest move of a value,
so the device's threshold (the r-th largest of the sample) is within e of the reference's, and
    #{ref > thr* + 2 e} <= #{device value > device threshold} <= #{ref > thr* - 2 e}.
If both ends give the same route, the device takes it."""
import os
import re

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "opentf_amd", "csrc")


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def _constants(text, names):
    """`constexpr int NAME = <expression of integers and earlier names>;` -> {NAME: value}; a missing name is a KeyError"""
    found = dict(re.findall(r"constexpr\s+(?:int|int64_t)\s+(\w+)\s*=\s*([^;]+);", text))
    out = {}
    for name in names:
        expr = found[name]
        assert re.fullmatch(r"[\w\s+\-*/()]+", expr), (name, expr)
        out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))
    return out


_SEL_H, _SIMS_H = _read("opentf_amd", "csrc", "ntf_select.h"), _read("opentf_amd", "csrc", "ntf_sims.h")
_c = _constants(_SEL_H, ["SEL_MAX", "SEL_SAMPLE"])
SEL_MAX, SEL_SAMPLE = _c["SEL_MAX"], _c["SEL_SAMPLE"]
_c = _constants(_SIMS_H, ["SIM_KC", "SIM_SLD", "SIM_WAVES", "SIM_RB", "SIM_QUNIT", "SIM_MAX_GROUP", "SIM_MAX_RANGE"])
SIM_KC, SIM_SLD, SIM_WAVES, SIM_RB, SIM_QUNIT, SIM_MAX_GROUP, SIM_MAX_RANGE = (_c[k] for k in ("SIM_KC", "SIM_SLD", "SIM_WAVES", "SIM_RB", "SIM_QUNIT", "SIM_MAX_GROUP",
                                                                                                "SIM_MAX_RANGE"))
_m = re.search(r"#define NTF_KNN_WORKSPACE_BYTES \(\(int64_t\)(\d+) << (\d+)\)", _read("include", "opentf_amd.h"))
WORKSPACE_BYTES = int(_m.group(1)) << int(_m.group(2))          # the default budget of both entries
UNIT_BYTES = SIM_QUNIT * SIM_RB * 4

# the decisions, as the headers state them (whitespace aside); each is modelled below under the name on the left
RULES = {
    "sampled_entered": (_SEL_H, "if (M >= 8 * SEL_SAMPLE && K * 8 <= SEL_MAX) {"),
    "sample stride": (_SEL_H, "const int stride = M / SEL_SAMPLE;"),
    "sample columns": (_SEL_H, "Key::key(row[(int64_t)k * stride])"),
    "sample_rank": (_SEL_H, "int r = (int)((4.5 * K * SEL_SAMPLE) / M) + 1; if (r < 8) r = 8;"),
    "threshold": (_SEL_H, "keys[r < SEL_SAMPLE ? r : SEL_SAMPLE - 1]"),
    "collected": (_SEL_H, "if (u > thr && (!EXCL || c != ex)) { const unsigned p = atomicAdd(&sh.count, 1u); if (p < SEL_MAX)"),
    "accepted": (_SEL_H, "if (cnt >= (unsigned)K && cnt <= SEL_MAX) {"),
    "sims_lds": (_SIMS_H, "return ((size_t)nqt * 32 * (dp + 1) + (size_t)nqt * 32 + (size_t)SIM_WAVES * 32 * SIM_SLD) * sizeof(float);"),
    "per_cu": (_SIMS_H, "const int per_cu = std::max<int>(1, (int)((160u << 10) / lds));"),
    "grid_width": (_SIMS_H, "std::min<int64_t>((rr + SIM_RB - 1) / SIM_RB, (int64_t)n_cu * per_cu)"),
    "block stride": (_SIMS_H, "for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {"),
    "launch_nqt": (_SIMS_H, "const int nqt = std::min(nqt_max, ng > 64 ? 4 : ng > 32 ? 2 : 1);"),
    "plan g": (_SIMS_H, "const int64_t g = std::min<int64_t>(std::max<int64_t>(wsb / ((int64_t)8 << 20), 1), std::min<int64_t>(SIM_MAX_GROUP / SIM_QUNIT, "
                        "(n + SIM_QUNIT - 1) / SIM_QUNIT));"),
    "plan nqt": (_SIMS_H, "nqt_max = (std::min(G, n) > 64 && dp <= 128) ? 4 : (std::min(G, n) > 32) ? 2 : 1;"),
    "plan Gw": (_SIMS_H, "Gw = (g + nqt_max - 1) / nqt_max * nqt_max * SIM_QUNIT;"),
    "plan R": (_SIMS_H, "R = std::min<int64_t>(std::min<int64_t>(wsb / (Gw * SIM_RB * 4), SIM_MAX_RANGE / SIM_RB), (N + SIM_RB - 1) / SIM_RB) * SIM_RB;"),
}


def rule_stands(name):
    text, line = RULES[name]
    flat = lambda s: re.sub(r"\s+", " ", s)
    return flat(line) in flat(text)


# ------------------------------------------------------------------------------------------------------------------ the selection's decisions
def sampled_entered(M, K):
    return M >= 8 * SEL_SAMPLE and K * 8 <= SEL_MAX


def sample_columns(M):
    return np.arange(SEL_SAMPLE, dtype=np.int64) * (M // SEL_SAMPLE)


def sample_rank(M, K):
    return max(int(4.5 * K * SEL_SAMPLE / M) + 1, 8)


def threshold(row, K):
    """the value at index r of the descending sample (the excluded column is part of the sample, as on the device)"""
    M = len(row)
    s = np.sort(np.asarray(row)[sample_columns(M)])[::-1]
    return s[min(sample_rank(M, K), SEL_SAMPLE - 1)]


def count_above(row, t, ex=-1):
    above = np.asarray(row) > t
    return int(above.sum()) - int(0 <= ex < len(row) and above[ex])


def _outcome(count, K):
    return "sampled" if K <= count <= SEL_MAX else "few" if count < K else "many"


def _pinned(row, K, margin, tied):
    """the sample's index r holds a value of the tie group wherever the other values move within the margin"""
    cols = sample_columns(len(row))
    r = min(sample_rank(len(row), K), SEL_SAMPLE - 1)
    s, st = row[cols], tied[cols]
    above = int((~st & (s > row[tied].max() + margin)).sum())
    return above == int((~st & (s > row[tied].min() - margin)).sum()) and above <= r < above + int(st.sum())


def route(row, K, ex=-1, margin=0.0, tied=None):
    """what select_topk_row does with this row: "radix" (the sampled route is not entered), "sampled" (it is, and its candidates are taken), "few" / "many" (it is,
    collects fewer than K / more than SEL_MAX and falls back to the radix route), "undecided" (the two ends of the margin disagree) -> (route, counts at the ends).
    tied: a mask of columns that hold one bit pattern on the device (copies of one table row).  If the threshold is one of them, none of them is above it, and
    the margin is asked of the other columns only."""
    row = np.asarray(row)
    if not sampled_entered(len(row), K):
        return "radix", None
    if tied is not None and _pinned(row, K, margin, tied):
        free = ~tied
        if 0 <= ex < len(row): free[ex] = False
        lo, hi = int((row[free] > row[tied].max() + margin).sum()), int((row[free] > row[tied].min() - margin).sum())
        a, b = _outcome(hi, K), _outcome(lo, K)
        return (a if a == b else "undecided"), (lo, hi)
    t = threshold(row, K)
    hi, lo = count_above(row, t - margin, ex), count_above(row, t + margin, ex)
    a, b = _outcome(hi, K), _outcome(lo, K)
    return (a if a == b else "undecided"), (lo, hi)


# ------------------------------------------------------------------------------------------------------------------ the sims grid and the plan
def padded(d):
    return (d + SIM_KC - 1) // SIM_KC * SIM_KC


def sims_lds(nqt, dp):
    return (nqt * 32 * (dp + 1) + nqt * 32 + SIM_WAVES * 32 * SIM_SLD) * 4


def per_cu(nqt, dp):
    return max(1, (160 << 10) // sims_lds(nqt, dp))


def row_blocks(rr):
    return (rr + SIM_RB - 1) // SIM_RB


def grid_width(rr, n_cu, nqt, dp):
    return min(row_blocks(rr), n_cu * per_cu(nqt, dp))


def strides(rr, n_cu, nqt, dp):
    """a workgroup of the range's launch takes a second row block"""
    return grid_width(rr, n_cu, nqt, dp) < row_blocks(rr)


def rows_that_stride(n_cu, nqt, dp):
    """the smallest range that makes a workgroup take a second row block"""
    return SIM_RB * n_cu * per_cu(nqt, dp) + 1


class SimsPlan:
    """ntf_sims.h SimsPlan: n queries in groups of G, N rows in ranges of R, a workspace of Gw x R floats within wsb (0: the default budget)"""

    def __init__(self, wsb, n, N, dp):
        wsb = wsb or WORKSPACE_BYTES
        g = min(max(wsb // (8 << 20), 1), min(SIM_MAX_GROUP // SIM_QUNIT, (n + SIM_QUNIT - 1) // SIM_QUNIT))
        self.G = g * SIM_QUNIT
        self.nqt = 4 if (min(self.G, n) > 64 and dp <= 128) else 2 if min(self.G, n) > 32 else 1
        self.Gw = (g + self.nqt - 1) // self.nqt * self.nqt * SIM_QUNIT
        self.R = min(wsb // (self.Gw * SIM_RB * 4), SIM_MAX_RANGE // SIM_RB, (N + SIM_RB - 1) // SIM_RB) * SIM_RB
        self.n, self.N = n, N

    def ranges(self):
        return [(r0, min(self.R, self.N - r0)) for r0 in range(0, self.N, self.R)]

    def groups(self):
        return [(g0, min(self.G, self.n - g0)) for g0 in range(0, self.n, self.G)]

    def launch_nqt(self, ng):
        return min(self.nqt, 4 if ng > 64 else 2 if ng > 32 else 1)


def routes_of_call(ref, K, wsb, dp, exclude=None, margin=0.0):
    """the route of every (query, range) of one call on the reference rows ref [n, N] -> {(query, r0): route}"""
    n, N = ref.shape
    out = {}
    for r0, rr in SimsPlan(wsb, n, N, dp).ranges():
        for q in range(n):
            ex = -1 if exclude is None or exclude[q] < 0 else int(exclude[q]) - r0
            out[q, r0] = route(ref[q, r0:r0 + rr], K, ex, margin)[0]
    return out
