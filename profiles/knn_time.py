"""Batched cosine nearest-neighbour search (ntf_knn_query) against the host route it stands beside (KeyedVectors.most_similar), for profiles/knn_bench.md, which this
script writes.  A synthetic clustered table at dblp's shape (1 995 708 teams, d = 128: 256 centres + 0.3 sigma of noise), topn = 10, Q in {1, 32, 1000} queries drawn
near rows of the table; five alternating rounds (every Q in turn, five times) after one untimed call per Q.  device_ms is the event time around the sims / selection
kernels of a call; wall_ms is the whole call with the upload of the queries and the copy back.  The host route is timed on the same box and table, one query a call."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from opentf_amd import libntf                      # noqa: E402
from opentf_amd.mdl.emb import d2v as P            # noqa: E402

HBM_TBS, F32_MATRIX_TF = 8.0, 157.3                # MI355X: HBM3E peak, dense f32 matrix peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_995_708); ap.add_argument("--d", type=int, default=128); ap.add_argument("--topn", type=int, default=10)
    ap.add_argument("--q", type=int, nargs="+", default=[1, 32, 1000]); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--host-queries", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "knn_bench.md"))
    a = ap.parse_args()
    N, d = a.n, a.d
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((256, d), dtype=np.float32)
    T = rng.standard_normal((N, d), dtype=np.float32)
    T *= np.float32(0.3)
    T += centres[rng.integers(256, size=N)]
    queries = {Q: (T[rng.integers(N, size=Q)] + np.float32(0.1) * rng.standard_normal((Q, d), dtype=np.float32)).astype(np.float32) for Q in a.q}
    t0 = time.perf_counter()
    knn = libntf.Knn(T)
    create_s = time.perf_counter() - t0
    dev, wall, first = {Q: [] for Q in a.q}, {Q: [] for Q in a.q}, {}
    for Q in a.q: first[Q] = knn.query(queries[Q], topn=a.topn)                      # untimed
    for _ in range(a.rounds):
        for Q in a.q:
            t0 = time.perf_counter()
            idx, sims, ms = knn.query(queries[Q], topn=a.topn, want_ms=True)
            wall[Q].append(round((time.perf_counter() - t0) * 1e3, 3)); dev[Q].append(round(ms, 4))
            assert np.array_equal(idx, first[Q][0]) and np.array_equal(sims.view(np.uint32), first[Q][1].view(np.uint32))
    knn.close()
    # the replaced route: one query a call over the same table
    kv = P.KeyedVectors(range(N), T)
    host = []
    for i in range(a.host_queries):
        t0 = time.perf_counter()
        near = kv.most_similar([queries[max(a.q)][i]], topn=a.topn)
        host.append(round((time.perf_counter() - t0) * 1e3, 1))
        assert [k for k, _ in near][0] == int(first[max(a.q)][0][i, 0]) or abs(near[0][1] - float(first[max(a.q)][1][i, 0])) < 1e-4
    host_ms = float(np.median(host))
    dp = (d + 31) // 32 * 32
    lines, rows = [], []
    for Q in a.q:
        med = float(np.median(dev[Q]))
        rec = {"n_rows": N, "d": d, "topn": a.topn, "Q": Q, "device_ms_rounds": dev[Q], "device_ms_median": round(med, 4), "wall_ms_median": round(float(np.median(wall[Q])), 3),
               "device_us_per_query": round(med * 1e3 / Q, 3), "table_TB_per_s": round(N * dp * 4 / (med * 1e-3) / 1e12, 3), "f32_TFLOPs": round(2.0 * Q * N * d / (med * 1e-3) / 1e12, 2),
               "host_ms_per_query_rounds": host, "host_ms_per_query": host_ms, "host_over_device_per_query": round(host_ms / (med / Q), 1)}
        lines.append(json.dumps(rec)); print(lines[-1], flush=True)
        bound = (f"{100 * rec['table_TB_per_s'] / HBM_TBS:.1f} % of {HBM_TBS:g} TB/s (one read of the table)" if Q <= 32
                 else f"{100 * rec['f32_TFLOPs'] / F32_MATRIX_TF:.1f} % of {F32_MATRIX_TF:g} TF (2 Q N d)")
        rows.append(f"| {Q} | {med:.3f} | {rec['wall_ms_median']:.2f} | {rec['device_us_per_query']:.1f} | {rec['table_TB_per_s']:.2f} | {rec['f32_TFLOPs']:.1f} | {bound} | {rec['host_over_device_per_query']:.0f} x |")
    md = f"""# Batched cosine nearest neighbours on the device (`ntf_knn_query`) against the host route (`KeyedVectors.most_similar`)

`python profiles/knn_time.py` on one MI355X.  A synthetic clustered table of {N:,} rows, d = {d} (256 centres + 0.3 sigma of noise; {N * dp * 4 / 1e9:.2f} GB on the device),
topn = {a.topn}, queries drawn near rows of the table, the default workspace (256 MiB).  `device_ms` is the event time around the sims / selection kernels of one call,
`wall` the whole call with the upload of the queries and the copy back; {a.rounds} alternating rounds (every Q in turn) after one untimed call per Q, medians below.
Creating the handle (upload of the table and the norm pass) took {create_s:.2f} s.  The host route is the same function at the parent commit, `most_similar`, on the same
box and table: it re-normalises the table and argsorts all sims on every call - {host_ms:.0f} ms a query (median of {host}).

```
{chr(10).join(lines)}
```

| Q | device ms | wall ms | device us / query | table TB/s | f32 TFLOP/s | against the bound | host / device, per query |
|---|---|---|---|---|---|---|---|
{chr(10).join(rows)}
"""
    with open(a.out, "w") as f: f.write(md)


if __name__ == "__main__":
    main()
