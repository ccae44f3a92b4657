"""Link decode of a Gnn table (ntf_link_topk / ntf_link_dense) against the reference-shaped host route, for profiles/link_bench.md, which this script writes.
dblp mt10.ts2 shapes: a synthetic clustered table of S + M + N = 90 671 + 233 629 + 1 995 708 rows in this plugin's n2v order, d = 128, uploaded WHOLE (1.19 GB on
the device: nothing is cut to fit a budget); candidates = the member block; queries = n team rows, n in {2 000, 20 000}; K = 100, and the dense entry (probabilities
alone).  Five alternating rounds (every configuration in turn, five times) after one untimed call each.  device_ms is the event time of a call from the query gather to
the last kernel (dense: the copies to the host between the kernels included); wall_ms the whole call.  The host route is what the parent commit offers for the same
job, torch.sigmoid(q @ E_m.T) then torch.topk on this box's cores, in batches of 2 000 teams.
--kernel-stats FILE: a `rocprofv3 --kernel-trace --stats --output-format csv` kernel_stats file of a run of this script (taken in a run of its own) whose shares by
kernel are put into the document."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf                      # noqa: E402

F32_MATRIX_TF = 157.3                              # MI355X: dense f32 matrix peak (v_mfma_f32_32x32x2_f32)
S, M, N = 90_671, 233_629, 1_995_708


def kernel_shares(path):
    rows = [r for r in csv.DictReader(open(path))]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = []
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]:
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
        out.append(f"| `{name[:90]}` | {r['Calls']} | {float(r['TotalDurationNs']) / 1e6:.1f} | {100 * float(r['TotalDurationNs']) / total:.1f} % |")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128); ap.add_argument("--k", type=int, default=100); ap.add_argument("--n", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--no-host", action="store_true"); ap.add_argument("--dense-max-n", type=int, default=20000)
    ap.add_argument("--kernel-stats", default=None); ap.add_argument("--tiny", action="store_true", help="a rehearsal at toy shapes")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_bench.md"))
    a = ap.parse_args()
    s, m, n_team = (90, 2336, 19957) if a.tiny else (S, M, N)
    if a.tiny: a.n = [20, 200]
    d, K = a.d, a.k
    import torch
    threads = torch.get_num_threads()
    rng = np.random.default_rng(0)
    rows_total = s + m + n_team
    centres = rng.standard_normal((256, d), dtype=np.float32)
    T = rng.standard_normal((rows_total, d), dtype=np.float32)
    T *= np.float32(0.3)
    T += centres[rng.integers(256, size=rows_total)]
    T *= np.float32(1.7 / np.sqrt(d))
    m_lo, t_lo = s, s + m
    queries = {n: t_lo + rng.choice(n_team, size=n, replace=False).astype(np.int64) for n in a.n}
    t0 = time.perf_counter()
    link = libntf.Link(T, m_lo, m_lo + m)
    create_s = time.perf_counter() - t0
    configs = [("topk", n) for n in a.n] + [("dense", n) for n in a.n if n <= a.dense_max_n]

    def call(kind, n):
        t0 = time.perf_counter()
        if kind == "topk": idx, _, prob, ms = link.topk(rows=queries[n], K=K, want_ms=True); sig = (idx, prob)
        else: _, prob, ms = link.dense(rows=queries[n], logit=False, want_ms=True); sig = (prob[:: max(1, n // 50)].copy(),)
        return ms, (time.perf_counter() - t0) * 1e3, sig
    first = {c: call(*c)[2] for c in configs}                       # untimed
    dev, wall = {c: [] for c in configs}, {c: [] for c in configs}
    for _ in range(a.rounds):
        for c in configs:
            ms, w, sig = call(*c)
            dev[c].append(round(ms, 3)); wall[c].append(round(w, 1))
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(sig, first[c]))
    # the host route, in batches of 2 000 teams (a [20 000, M] f32 matrix is 18.7 GB), on the same table
    host = {}
    if not a.no_host:
        Em = torch.from_numpy(T[m_lo:m_lo + m])
        for n in a.n:
            t0 = time.perf_counter()
            got = []
            for o in range(0, n, 2000):
                q = torch.from_numpy(T[queries[n][o:o + 2000]])
                got.append(torch.topk(torch.sigmoid(q @ Em.T), K, dim=1)[1].numpy())
            host[n] = round((time.perf_counter() - t0) * 1e3, 1)
            ids = np.concatenate(got)
            agree = float((ids[:, 0] == first[("topk", n)][0][:, 0]).mean())
            assert agree > 0.99, agree                              # (f32 sums in another order: the first id may differ where two logits are an ulp apart)
    link.close()
    lines, rows = [], []
    for kind, n in configs:
        med = float(np.median(dev[(kind, n)]))
        rec = {"entry": kind, "n": n, "M": m, "table_rows": rows_total, "d": d, "K": K if kind == "topk" else None, "device_ms_rounds": dev[(kind, n)], "device_ms_median": round(med, 3),
               "wall_ms_median": round(float(np.median(wall[(kind, n)])), 1), "device_ms_per_1000_teams": round(med * 1000 / n, 3),
               "f32_TFLOPs_of_the_whole_call": round(2.0 * n * m * d / (med * 1e-3) / 1e12, 2), "host_ms": host.get(n), "host_threads": threads}
        lines.append(json.dumps(rec)); print(lines[-1], flush=True)
        h = f"{host[n]:.0f} ({host[n] * 1000 / n:.0f} per 1 000; {host[n] / rec['wall_ms_median']:.1f} x the wall time)" if (n in host and kind == "topk") else "-"
        rows.append(f"| {kind} | {n} | {med:.2f} | {rec['wall_ms_median']:.0f} | {rec['device_ms_per_1000_teams']:.2f} | {rec['f32_TFLOPs_of_the_whole_call']:.1f} "
                    f"({100 * rec['f32_TFLOPs_of_the_whole_call'] / F32_MATRIX_TF:.1f} % of {F32_MATRIX_TF:g}) | {h} |")
    shares = ""
    if a.kernel_stats:
        # the profiled run made two calls of every configuration (the untimed one and its single round): the sims kernel's work in it, 2 n M d a call
        sims_ms = sum(float(r["TotalDurationNs"]) for r in csv.DictReader(open(a.kernel_stats)) if "k_sims" in r["Name"]) / 1e6
        flop = 2 * sum(2.0 * n * m * d for _, n in configs)
        roof = (f"\n`k_sims` alone: {flop / 1e12:.2f} TFLOP (2 n M d a call, two calls of every configuration) in {sims_ms:.1f} ms = {flop / sims_ms / 1e9:.1f} TFLOP/s, "
                f"{100 * flop / sims_ms / 1e9 / F32_MATRIX_TF:.1f} % of the {F32_MATRIX_TF:g} TFLOP/s exact-f32 MFMA roof.\n") if sims_ms else ""
        shares = ("\n## Device time by kernel\n\n`rocprofv3 --kernel-trace --stats` over one run of this script with `--rounds 1 --no-host` (a run of its own; every configuration twice, "
                  "the untimed call and one round):\n\n| kernel | calls | total ms | share |\n|---|---|---|---|\n" + "\n".join(kernel_shares(a.kernel_stats)) + "\n") + roof
    md = f"""# Link decode of a Gnn table on the device (`ntf_link_topk`, `ntf_link_dense`) against the host route (`torch.sigmoid(q @ E_m.T)`, `torch.topk`)

`python profiles/link_bench.py` on one MI355X.  dblp `mt10.ts2` shapes: a synthetic clustered table of S + M + N = {s:,} + {m:,} + {n_team:,} rows, d = {d}
({rows_total * ((d + 31) // 32 * 32) * 4 / 1e9:.2f} GB on the device: the WHOLE table is uploaded, {create_s:.2f} s with the finite check), candidates = the member block, queries = team rows
gathered on the device, K = {K}, the dense entry asked for probabilities alone, the default workspace (256 MiB).  `device ms` is the event time of one call from the
query gather to the last kernel - for the dense entry the copies of [n, M] to pageable host memory lie between the kernels and are inside it; `wall` is the whole call.
{a.rounds} alternating rounds (every configuration in turn) after one untimed call each, medians below; the results of every round are bit-identical to the untimed call's.
`TFLOP/s` is 2 n M d over the device time of the WHOLE call (selection or copies included): an end-to-end rate, not the sims kernel's.
The host route runs on the same box with {threads} torch threads, in batches of 2 000 teams, top-{K}; its first id agrees with the device's for more than 99 % of the teams.

```
{chr(10).join(lines)}
```

| entry | n | device ms | wall ms | device ms / 1 000 teams | TFLOP/s of the call | host route ms |
|---|---|---|---|---|---|---|
{chr(10).join(rows)}
{shares}"""
    with open(a.out, "w") as f: f.write(md)


if __name__ == "__main__":
    main()
