"""Case builders for the co-occurrence kernels' paths (opentf_amd/csrc/ntf_cooc.hip) and the profile of what the device does with a case.
TEST INFRASTRUCTURE ONLY, CPU only: shared by tests/test_cooc_host.py (which asserts that every case reaches the branch it is named for) and
tests/test_gpu_cooc_paths.py (which compares the device with the oracle on them).  Deterministic: fixed seeds, no files.

A case is `(m_indptr, m_indices, s_indptr, s_indices, n, M, S, skip)`: the member and the skill matrix of n teams as CSR (ids ascending and
unique inside a row, as a lil matrix keeps them) and the list of skipped teams.  `case(name)` builds it once per process, read-only;
`roles(name)` names the members a test wants to look at; `expected(name, skipped)` is the oracle's result, computed once.

The cases are sized for SORT_MAX = 2048, HIST_WGS = 512, SCAN_BLOCK = 1024 (`SIZED_FOR`); `constants()` reads the values the kernels are
built with out of the source, `profile()` computes with those, so a retuned constant shows in the host test instead of silently moving a
case off its branch.  `python tests/cooc_cases.py` prints the table of profiles/cooc_paths_check.md."""
import functools
import os
import re

import numpy as np

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opentf_amd", "csrc", "ntf_cooc.hip")
SIZED_FOR = {"SORT_MAX": 2048, "HIST_WGS": 512, "SCAN_BLOCK": 1024}
TOP_STRIP = 256                                                   # k_scan_top scans the block sums 256 at a time (its block size)

SORT_WORKS = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048)
SCAN_MS = (262144, 262145, 263169, 600000)
SCAN_FORCED = (0, 1023, 1024, 1025, 262143, 262144, 262145)       # ids with work in every scan_wide case (where M allows), and M - 1
DEGENERATE = ("all_skipped", "skip_repeated", "n1", "n255", "n256", "n257", "no_pairs")
NAMES = (["sort_edges", "hist_edges-1027", "hist_edges-2051", "hist_rounds"] + [f"scan_wide-{M}" for M in SCAN_MS] +
         [f"degenerate-{d}" for d in DEGENERATE])


@functools.lru_cache(maxsize=None)
def constants():
    src = open(HIP).read()
    out = {}
    for k in SIZED_FOR:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % k, src)
        assert m, f"{k} is no longer a `constexpr int` of ntf_cooc.hip: tests/cooc_cases.py cannot tell which path a case takes"
        out[k] = int(m.group(1))
    return out


def _pack(teams, M, S, skip):
    """teams: list of (member ids, skill ids) -> the eight-tuple, read-only"""
    rows_m = [np.unique(np.asarray(m, np.int32)) for m, _ in teams]
    rows_s = [np.unique(np.asarray(s, np.int32)) for _, s in teams]
    def csr(rows, width):
        indptr = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=indptr[1:])
        indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
        assert not len(indices) or (0 <= indices.min() and indices.max() < width)
        return indptr, indices
    m_ip, m_ix = csr(rows_m, M)
    s_ip, s_ix = csr(rows_s, S)
    skip = np.asarray(skip, np.int64)
    for a in (m_ip, m_ix, s_ip, s_ix, skip): a.setflags(write=False)
    return m_ip, m_ix, s_ip, s_ix, len(teams), M, S, skip


def _layers(member, counts):
    """teams of one member that give it exactly `counts[s]` pairs with skill s: team k holds the skills counted more than k times"""
    c = np.asarray(counts, np.int64)
    return [([member], np.nonzero(c > k)[0]) for k in range(int(c.max()))]


def _counts(S, pairs):
    c = np.zeros(S, np.int64)
    for s, v in pairs: assert c[s] == 0; c[s] = v
    return c


def _short_teams(rng, members, S, n, max_members=3, max_skills=10):
    """n teams shared among a few short-row members"""
    return [(rng.choice(members, min(len(members), 1 + rng.integers(0, max_members)), replace=False), rng.choice(S, 1 + rng.integers(0, max_skills), replace=False))
            for _ in range(n)]


# ---------------------------------------------------------------- sort path: the bitonic padding and the SORT_MAX boundary
def _sort_edges():
    rng = np.random.default_rng(2048)
    S = 2051
    teams, skip, r = [], [], {"distinct": {}, "repeated": {}}
    m = 0
    for i, w in enumerate(SORT_WORKS):
        # repeated: w teams of the same single skill -> one run of length w, count w % 256 (nothing at 1024, 2048); 0 and S - 1 are among the skills
        s = (0, S - 1, 1023, 1024)[i % 4] if i < 8 else int(rng.integers(0, S))
        r["repeated"][w] = m
        teams += [([m], [s])] * w
        m += 1
        # distinct: one team of w different skills -> w run heads
        r["distinct"][w] = m
        teams.append(([m], rng.choice(S, w, replace=False)))
        m += 1
        if w == 64: r["no_team"] = m; m += 1                       # an id no team names
        if w == 1024:                                              # a member all of whose teams are skipped
            r["all_skipped"] = m
            skip += [len(teams), len(teams) + 1]
            teams += [([m], rng.choice(S, 40, replace=False)), ([m], rng.choice(S, 3, replace=False))]
            m += 1
    return _pack(teams, m, S, skip), r


# ---------------------------------------------------------------- histogram path: pass edges, wrapped counts, rows that vanish
def _hist_edges(S):
    rng = np.random.default_rng(S)
    W = SIZED_FOR["SORT_MAX"]
    spread = lambda w, shift: np.roll(w // S + (np.arange(S) < w % S), shift)
    full = rng.integers(1, 4, S); full[rng.choice(S, 40, replace=False)] = 257; full[rng.choice(S, 5, replace=False)] = 511; full[[0, 1023, 1024, S - 1]] = (255, 513, 1, 257)
    rows = [("w2049", spread(W + 1, 0)), ("short", None), ("w2050", spread(W + 2, 5)), ("full", full),
            ("multiples", _counts(S, [(0, 256), (5, 256), (1023, 512), (1024, 256), (1000, 256), (300, 256), (S - 1, 256), (700, 256)])), ("short", None),
            ("mixed", _counts(S, [(3, 255), (4, 256), (7, 512), (1022, 257), (1023, 512), (1024, 255), (1025, 256), (S - 1, 257)])),
            ("only_0", _counts(S, [(0, W + 1)])), ("short", None), ("only_1023_1024", _counts(S, [(1023, 1100), (1024, 1200)])),
            ("only_last", _counts(S, [(S - 1, W + 2)])), ("first_and_last", _counts(S, [(0, 1500), (S - 1, 1501)])), ("short", None),
            ("several_x", spread(3 * W + 77, 1000))]
    teams, r, short = [], {}, []
    for m, (name, c) in enumerate(rows):
        if c is None: short.append(m); continue
        r[name] = m
        teams += _layers(m, c)
    r["short"] = short
    teams += _short_teams(rng, short, S, 60)
    # skipped teams: counted, they would take `multiples` off its multiples of 256 and fill the holes of the `only_*` rows
    skip = list(range(len(teams), len(teams) + 6))
    teams += [([r["multiples"], r["only_0"]], [0, 5, 9]), ([r["only_last"], short[0]], rng.choice(S, 30, replace=False)), ([r["multiples"]], [1023]),
              ([r["only_1023_1024"]], [1022, 1025]), ([r["first_and_last"]], [1024]), (short, [1, 2])]
    return _pack(teams, len(rows), S, skip), r


# ---------------------------------------------------------------- histogram path: more long rows than scratch rows
def _hist_rounds():
    rng = np.random.default_rng(512)
    S, n_long, n_short = 1027, 1100, 40
    M = n_long + n_short
    short = list(range(7, M, M // n_short))[:n_short]
    long_ = [m for m in range(M) if m not in set(short)]
    teams = []
    for m in long_:                                                # its own 22 teams of 95-105 skills out of its own 200-skill pool: work >= 2090
        pool = rng.choice(S, 200, replace=False)
        teams += [([m], rng.choice(pool, 95 + rng.integers(0, 11), replace=False)) for _ in range(22)]
    teams += _short_teams(rng, short, S, 300, max_members=4)
    order = rng.permutation(len(teams))                            # a member's teams lie scattered, as in a dataset
    skip = np.nonzero(order >= len(teams) - 30)[0]                 # thirty of the short rows' teams
    return _pack([teams[i] for i in order], M, S, skip), {"long": long_, "short": short}


# ---------------------------------------------------------------- the scan over more than 256 blocks
def _scan_wide(M):
    rng = np.random.default_rng(M)
    S = 1027
    forced = sorted({m for m in SCAN_FORCED if m < M} | {M - 1})
    pool = np.unique(np.concatenate([forced, rng.choice(M, 3000, replace=False)]))
    teams = [([f, rng.choice(pool)], rng.choice(S, 1 + rng.integers(0, 8), replace=False)) for f in forced]       # never skipped
    nf = len(teams)
    teams += _short_teams(rng, pool, S, 3000, max_members=4, max_skills=8)
    hist = [M - 1] + ([int(rng.integers(262146, M - 1))] if M > 262148 else [])                                   # M - 1 sits in the last block
    for h in hist: teams += [([h], rng.choice(S, 100, replace=False)) for _ in range(30)]
    skip = nf + np.arange(0, 3000, 9)
    return _pack(teams, M, S, skip), {"forced": forced, "hist": hist}


def _degenerate(kind):
    rng = np.random.default_rng(7)
    if kind in ("all_skipped", "skip_repeated"):
        M, S = 9, 11
        teams = _short_teams(rng, np.arange(M), S, 12)
        skip = np.arange(12) if kind == "all_skipped" else np.array([3, 3, 7, 0, 7, 3, 11, 11])
        return _pack(teams, M, S, skip), {}
    if kind == "no_pairs":                                         # every team lacks members or lacks skills (or both)
        teams = [([], [1, 2]), ([0, 3], []), ([], []), ([2], []), ([], [0]), ([1, 2, 3], [])]
        return _pack(teams, 4, 3, [1]), {}
    n = int(kind[1:])                                              # n teams of the one member and the one skill: one count of n % 256
    return _pack([([0], [0])] * n, 1, 1, []), {}


@functools.lru_cache(maxsize=None)
def _built(name):
    kind, _, arg = name.partition("-")
    if kind == "sort_edges": return _sort_edges()
    if kind == "hist_edges": return _hist_edges(int(arg))
    if kind == "hist_rounds": return _hist_rounds()
    if kind == "scan_wide": return _scan_wide(int(arg))
    if kind == "degenerate": return _degenerate(arg)
    raise KeyError(name)


def case(name): return _built(name)[0]
def roles(name): return _built(name)[1]


@functools.lru_cache(maxsize=None)
def expected(name, skipped=True):
    """the oracle's (indptr, indices, data) of a case, with its skip list or with none"""
    from oracle import cooc_oracle as CO
    m_ip, m_ix, s_ip, s_ix, n, M, S, skip = case(name)
    out = CO.skill_cooccurrence(m_ip, m_ix, s_ip, s_ix, M, S, skip if skipped else None)
    for a in out: a.setflags(write=False)
    return out


def profile(c, skipped=True):
    """what the device does with a case: the per-member work, the rows per row kernel, the scan's blocks and strips, the histogram's rounds"""
    m_ip, m_ix, s_ip, s_ix, n, M, S, skip = c
    k = constants()
    keep = np.ones(n, bool)
    if skipped and len(skip): keep[skip] = False
    ns = np.diff(s_ip) * keep
    work = np.zeros(M, np.int64)
    np.add.at(work, m_ix, np.repeat(ns, np.diff(m_ip)))
    blocks = max(1, -(-M // k["SCAN_BLOCK"]))
    hist = int((work > k["SORT_MAX"]).sum())
    return {"work": work, "sort_rows": int(((work > 0) & (work <= k["SORT_MAX"])).sum()), "hist_rows": hist, "scan_blocks": blocks,
            "strips": -(-blocks // TOP_STRIP), "rounds": -(-hist // k["HIST_WGS"]), "total": int(work.sum())}


def table():
    lines = ["| case | teams | M | S | skipped | sort rows | hist rows | scan blocks | strips | hist rounds | expanded total | nnz |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in NAMES:
        c = case(name); p = profile(c)
        lines.append(f"| `{name}` | {c[4]} | {c[5]} | {c[6]} | {len(np.unique(c[7]))} | {p['sort_rows']} | {p['hist_rows']} | {p['scan_blocks']} | {p['strips']} | {p['rounds']} | "
                     f"{p['total']} | {len(expected(name)[1])} |")
    return "\n".join(lines)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(table())
