"""CPU reference of the metapath2vec producer (ntf_m2v_create in opentf_amd/csrc/ntf_n2v.hip).  TEST INFRASTRUCTURE ONLY: nothing under opentf_amd/ imports it.

The reference trains its `m2v` table with `torch_geometric.nn.MetaPath2Vec` (torch_geometric 2.6.1), which is not installed here.  This file restates its published
algorithm, on the same footing oracle/n2v_oracle.py has for Node2Vec:
  * the node types that appear in the metapath, sorted by name, own consecutive row blocks; row `total` is the dummy row (`Embedding(count + 1, d)`);
  * pos_sample: batch.repeat(walks_per_node), step i over edge type metapath[i % L]: a uniformly drawn neighbour, or the dummy from a node without one and from
    the dummy itself; per-position offsets added, everything above the dummy clamped to it;
  * neg_sample: batch.repeat(walks_per_node * num_neg), position i + 1 = offset + randint(count of metapath[i % L]'s destination type);
  * windows and loss: Node2Vec's (oracle.n2v_oracle.windows / loss).
PyG's `walk_length` counts STEPS: `pos_sample` / `neg_sample` / `train` below take `steps`; the device ABI and the `replay_*` functions count NODES (= steps + 1).
`replay_walks` / `replay_negs` restate what k_m2v_walks / k_m2v_negs draw from their Philox counters.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse
import torch

from oracle import n2v_oracle as N
from oracle.d2v_oracle import philox4x32

from test_gpu_n2v_parity import n2v_key          # the key mix of ntf_n2v.hip, restated once (that module's helpers need no GPU)


def _csr(mat):
    m = scipy.sparse.csr_matrix(mat); m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int32)


def hop_csrs(skill, member, drop_teams=()):
    """{(src type, dst type): (rowptr int64, col int32 LOCAL ids)} of the 'stm' structure from the [team, skill] / [team, member] matrices; the member edges of
    `drop_teams` are removed in both directions, as the reference's graph drops them"""
    skill = scipy.sparse.csr_matrix(skill); member = scipy.sparse.lil_matrix(scipy.sparse.csr_matrix(member))
    for t in drop_teams: member[int(t)] = 0
    member = scipy.sparse.csr_matrix(member); member.eliminate_zeros()
    return {("skill", "team"): _csr(skill.T), ("team", "skill"): _csr(skill), ("member", "team"): _csr(member.T), ("team", "member"): _csr(member)}


class Path:
    """a metapath over typed CSRs: `types` sorted names, `count` / `start` per type in that order, `total` (= the dummy row), `hops` = [(src id, dst id, rowptr, col)]"""

    def __init__(self, counts, metapath, csrs):
        names = sorted({t for s, _, d in metapath for t in (s, d)})
        self.types = names
        self.count = np.array([counts[t] for t in names], dtype=np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.count)]).astype(np.int64)
        self.total = int(self.start[-1])
        for a, b in zip(metapath[:-1], metapath[1:]): assert a[2] == b[0], "the metapath does not chain"
        self.cycle = metapath[-1][2] == metapath[0][0]
        self.hops = [(names.index(s), names.index(d), *csrs[(s, d)]) for s, _, d in metapath]
        for s, d, rp, col in self.hops: assert len(rp) == self.count[s] + 1 and (len(col) == 0 or col.max() < self.count[d])

    @property
    def L(self): return len(self.hops)

    def start_of(self, name): return int(self.start[self.types.index(name)])

    def position_type(self, p):
        """type id of position p of a walk"""
        return self.hops[0][0] if p == 0 else self.hops[(p - 1) % self.L][1]

    def offsets(self, nodes):
        return torch.tensor([int(self.start[self.position_type(p)]) for p in range(nodes)], dtype=torch.long)


def pos_sample(path, batch, steps, context, walks_per_node, generator, as_walks=False):
    """MetaPath2Vec.pos_sample: `steps` + 1 nodes per walk; inside the loop the dummy is `total` as a LOCAL id, as PyG keeps it"""
    assert steps <= path.L or path.cycle
    batch = torch.as_tensor(batch, dtype=torch.long).repeat(walks_per_node)
    rws = [batch]
    for i in range(steps):
        s, d, rp, col = path.hops[i % path.L]
        rp_t, col_t = torch.as_tensor(rp), torch.as_tensor(col).long()
        mask = batch >= path.total
        sub = batch.clamp(min=0, max=len(rp) - 2)
        count = rp_t[sub + 1] - rp_t[sub]
        rand = torch.rand(len(sub), generator=generator) * count.to(torch.float32)
        idx = (rand.long() + rp_t[sub]).clamp(max=max(len(col) - 1, 0))
        nxt = col_t[idx] if len(col) else idx.clone()
        nxt[mask | (count == 0)] = path.total
        batch = nxt; rws.append(batch)
    rw = torch.stack(rws, dim=-1) + path.offsets(steps + 1).view(1, -1)
    rw[rw > path.total] = path.total
    return rw if as_walks else N.windows(rw, context)


def neg_sample(path, batch, steps, context, walks_per_node, num_neg, generator, as_walks=False):
    batch = torch.as_tensor(batch, dtype=torch.long).repeat(walks_per_node * num_neg)
    rws = [batch]
    for i in range(steps):
        rws.append(torch.randint(0, int(path.count[path.hops[i % path.L][1]]), (len(batch),), generator=generator))
    rw = torch.stack(rws, dim=-1) + path.offsets(steps + 1).view(1, -1)
    return rw if as_walks else N.windows(rw, context)


def replay_walks(path, batch, n_walks, nodes, seed, step):
    """k_m2v_walks: row r starts at LOCAL batch[r % B]; step s over hop (s - 1) % L takes word (s - 1) & 3 of Philox(counter (r lo, r hi, (s - 1) >> 2, step),
    key tensor 0): col[a + ((u * deg) >> 32)], or the dummy from a node of degree 0 and from the dummy - the slot is consumed either way.  -> GLOBAL ids [n_walks, nodes]"""
    key = n2v_key(seed, step, 0)
    rw = np.empty((n_walks, nodes), dtype=np.int64)
    for r in range(n_walks):
        cur = int(batch[r % len(batch)]); rw[r, 0] = path.start[path.hops[0][0]] + cur
        for s in range(1, nodes):
            if (s - 1) & 3 == 0: rnd = philox4x32((r & 0xFFFFFFFF, r >> 32, (s - 1) >> 2, step & 0xFFFFFFFF), key)
            _, d, rp, col = path.hops[(s - 1) % path.L]
            if cur >= 0:
                a = int(rp[cur]); deg = int(rp[cur + 1]) - a
                cur = int(col[a + ((rnd[(s - 1) & 3] * deg) >> 32)]) if deg > 0 else -1
            rw[r, s] = path.start[d] + cur if cur >= 0 else path.total
    return rw


def replay_negs(path, batch, n_rows, nodes, seed, step):
    """k_m2v_negs: start[dst] + ((u * count[dst]) >> 32) of Philox(counter (r lo, r hi, 0x4E454700 + ((s - 1) >> 2), step), key tensor 1)"""
    key = n2v_key(seed, step, 1)
    rw = np.empty((n_rows, nodes), dtype=np.int64)
    for r in range(n_rows):
        rw[r, 0] = path.start[path.hops[0][0]] + int(batch[r % len(batch)])
        for s in range(1, nodes):
            if (s - 1) & 3 == 0: rnd = philox4x32((r & 0xFFFFFFFF, r >> 32, (0x4E454700 + ((s - 1) >> 2)) & 0xFFFFFFFF, step & 0xFFFFFFFF), key)
            d = path.hops[(s - 1) % path.L][1]
            rw[r, s] = path.start[d] + ((rnd[(s - 1) & 3] * int(path.count[d])) >> 32)
    return rw


def windows(rw, context):
    return N.windows(torch.as_tensor(rw), context).numpy()


def train(path, d, b, epochs, lr, steps, context, walks_per_node, num_neg, seed=0):
    """_train_rw's loop without validation, shaped like oracle.n2v_oracle.train: -> (weight [total + 1, d], per-epoch mean batch loss); dense Adam"""
    g = torch.Generator().manual_seed(seed)
    emb = torch.nn.Embedding(path.total + 1, d)
    with torch.no_grad(): emb.weight.normal_(generator=g)
    opt = torch.optim.Adam(emb.parameters(), lr=lr)
    n0, hist = int(path.count[path.hops[0][0]]), []
    for _ in range(epochs):
        perm = torch.randperm(n0, generator=g)
        tot, nb = 0.0, 0
        for o in range(0, n0, b):
            batch = perm[o:o + b]
            opt.zero_grad()
            l = N.loss(emb.weight, pos_sample(path, batch, steps, context, walks_per_node, g), neg_sample(path, batch, steps, context, walks_per_node, num_neg, g))
            l.backward(); opt.step()
            tot += float(l.detach()); nb += 1
        hist.append(tot / nb)
    return emb.weight.detach(), hist


# ---------------------------------------------------------------------------------------------------------------- the forced graph
# members m0..m3, skills s0 s1, teams t0..t2; a metapath that names all three: sorted types member | skill | team -> rows 0..3 | 4 5 | 6 7 8, dummy 9.
# At most one neighbour per hop:
#   member -> team : m0 t0, m1 t1, m2 -, m3 t2        team -> member : t0 m1, t1 m0, t2 -  (t2 is a dropped team, m2 a member in no team; m3 -> t2 is kept on
#   purpose although PyG's graph is symmetric: the test is about the walk rule, and a one-way edge keeps every step forced)
#   team -> skill  : t0 s1, t1 s0, t2 s0              skill -> team  : s0 t1, s1 t0
FORCED_COUNTS = {"member": 4, "skill": 2, "team": 3}


def _one(n_src, pairs):
    rp = np.zeros(n_src + 1, dtype=np.int64); col = []
    for s in range(n_src):
        if s in pairs: col.append(pairs[s])
        rp[s + 1] = len(col)
    return rp, np.asarray(col, dtype=np.int32)


FORCED_CSRS = {("member", "team"): _one(4, {0: 0, 1: 1, 3: 2}), ("team", "member"): _one(3, {0: 1, 1: 0}),
               ("team", "skill"): _one(3, {0: 1, 1: 0, 2: 0}), ("skill", "team"): _one(2, {0: 1, 1: 0})}
MTM = [("member", "to", "team"), ("team", "rev_to", "member")]
MTSTM = [("member", "to", "team"), ("team", "rev_to", "skill"), ("skill", "to", "team"), ("team", "rev_to", "member")]
STM = [("skill", "to", "team"), ("team", "rev_to", "member")]


def forced(metapath):
    return Path(FORCED_COUNTS, metapath, FORCED_CSRS)


# walks of 5 nodes from members 0, 1, 2, 3, written out by hand
FORCED_WALKS = {
    # member -> team -> member names two types only: PyG gives rows to the types that APPEAR in the metapath, so here member | team -> rows 0..3 | 4 5 6, dummy 7
    "mtm": np.array([[0, 4, 1, 5, 0],        # m0 t0 m1 t1 m0
                     [1, 5, 0, 4, 1],        # m1 t1 m0 t0 m1
                     [2, 7, 7, 7, 7],        # m2 has no team: dummy, and the dummy stays
                     [3, 6, 7, 7, 7]]),      # m3 t2, t2 has no member
    "mtstm": np.array([[0, 6, 5, 6, 1],      # m0 t0 s1 t0 m1
                       [1, 7, 4, 7, 0],      # m1 t1 s0 t1 m0
                       [2, 9, 9, 9, 9],
                       [3, 8, 4, 7, 0]]),    # m3 t2 s0 t1 m0
}
# windows of context 3 of the "mtm" walks: row j * 4 + r = nodes j .. j + 2 of walk r; three of them START at the dummy
FORCED_WINDOWS_MTM = np.array([[0, 4, 1], [1, 5, 0], [2, 7, 7], [3, 6, 7],
                               [4, 1, 5], [5, 0, 4], [7, 7, 7], [6, 7, 7],
                               [1, 5, 0], [0, 4, 1], [7, 7, 7], [7, 7, 7]])
