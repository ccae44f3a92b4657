"""The ORDER of the kernels the node2vec / metapath2vec producers launch, for comparing two builds of the library (profiles/n2v_step_paths_check.md).

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/n2v_launch_order.py run
        for each of the six handle kinds (n2v and m2v, each dense / sparse / lazy) at tiny shapes: an applied native batch, an apply = 0 batch followed by an
        applied one, an injected call, edge_bce, weight().  One process per library (NTF_LIB_PATH selects it), no counters in the same run.
  python profiles/n2v_launch_order.py names DIR          the kernel names of the trace under DIR in dispatch order, one a line (template arguments kept)
  python profiles/n2v_launch_order.py diff DIR_A DIR_B   a unified diff of the two lists; `k_n2v_compact` / `k_n2v_compact_keep` are read as `k_n2v_compact<true>` / `<false>`
"""
import csv
import difflib
import glob
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

METAPATH = [("member", "to", "team"), ("team", "rev_to", "skill"), ("skill", "to", "team"), ("team", "rev_to", "member")]
D, B, NODES, CTX, WPN, NEG, LR = 65, 8, 5, 3, 2, 2, 0.01


def run():
    import numpy as np
    import scipy.sparse as sp
    from opentf_amd import libntf
    from opentf_amd.mdl.emb.gnn import m2v_graph, stm_graph
    from opentf_amd.synth import zipf_csr
    n_team, n_skill, n_member = 150, 40, 60
    (s_ip, s_ix), (m_ip, m_ix) = zipf_csr(n_team, n_skill, 3.0, 1), zipf_csr(n_team, n_member, 3.0, 2)
    skill = sp.csr_matrix((np.ones(len(s_ix), np.uint8), s_ix, s_ip), shape=(n_team, n_skill))
    member = sp.csr_matrix((np.ones(len(m_ix), np.uint8), m_ix, m_ip), shape=(n_team, n_member))
    drop = np.arange(0, n_team, 4)
    rowptr, col, _, n = stm_graph(skill, member, drop)
    counts, off, hops = m2v_graph(skill, member, drop, METAPATH)
    rng = np.random.default_rng(0)
    for which in ("n2v", "m2v"):
        rows = n if which == "n2v" else off["dummy"] + 1
        w = (0.1 * rng.standard_normal((rows, D))).astype(np.float32)
        for arm in ("dense", "sparse", "lazy"):
            kw = dict(seed=0, sparse=arm == "sparse", lazy=arm == "lazy")
            net = libntf.Node2Vec(rowptr, col, w, **kw) if which == "n2v" else libntf.MetaPath2Vec(counts, hops, w, **kw)
            batch = np.arange(B, dtype=np.int64)
            net.train_batch(batch, NODES, CTX, WPN, NEG, LR)
            net.train_batch(batch + 1, NODES, CTX, WPN, NEG, LR, apply=False)
            net.train_batch(batch + 2, NODES, CTX, WPN, NEG, LR)
            pos = rng.integers(0, rows - 1, (6, CTX)); neg = rng.integers(0, rows - 1, (9, CTX))
            net.loss_on(pos, neg, lr=LR, apply=True)
            net.edge_bce(pos[:, 0], pos[:, 1])
            net.weight()
            print(f"{which} {arm}: done", flush=True)
            net.close()


def names(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    ren = {"k_n2v_compact": "k_n2v_compact<true>", "k_n2v_compact_keep": "k_n2v_compact<false>"}
    out = []
    for r in rows:
        k = re.sub(r"^void ", "", re.sub(r"\(.*", "", r["Kernel_Name"]))
        out.append(ren.get(k, k))
    return out


if __name__ == "__main__":
    if sys.argv[1] == "run": run()
    elif sys.argv[1] == "names": print("\n".join(names(sys.argv[2])))
    else:
        a, b = names(sys.argv[2]), names(sys.argv[3])
        for group in difflib.SequenceMatcher(None, a, b, autojunk=False).get_grouped_opcodes(2):      # autojunk would take the names that repeat for noise
            print(f"@@ a {group[0][1] + 1}..{group[-1][2]}, b {group[0][3] + 1}..{group[-1][4]}")
            for tag, i1, i2, j1, j2 in group:
                if tag == "equal": print("".join(f"  {x}\n" for x in a[i1:i2]), end="")
                else: print("".join(f"- {x}\n" for x in a[i1:i2]) + "".join(f"+ {x}\n" for x in b[j1:j2]), end="")
