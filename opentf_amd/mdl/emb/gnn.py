"""`Gnn` with the node2vec method (`data.embedding.class_method=mdl.amd.emb.gnn.Gnn_n2v`): the reference's team2vec plugin
(src/mdl/emb/gnn.py) for its random-walk branch, trained on the MI355X, and the bridge that puts the CSR gather of
`get_dense_vecs` on the hot path of the UNMODIFIED caller.

What the caller (src/main.py:100-153) does and what it gets here:
  * `t2v = cls(output, acceleration, seed, cfg, method)`; `t2v.learn(teamsvecs, splits)`                       (main.py:112,122)
      per fold: the 'stm' graph (skill - team - member) without the member-team edges of the test and of that fold's validation teams
      (gnn.py:84-116), `torch_geometric.nn.Node2Vec` (its `p` / `q` read from the n2v section, absent = 1) trained by `_train_rw` (gnn.py:401-453: shuffled node batches, Adam,
      ReduceLROnPlateau on v_loss, EarlyStopping, `f{k}.pt` / `f{k}.e{e}.pt` checkpoints holding `embedding.weight`).  Here the walks,
      the skip-gram loss, its gradient and the dense Adam (or, with `sparse: true` in the method's section, sparse Adam; with `lazy: true`, dense Adam writing only the rows a batch names) run in `opentf_amd/csrc/ntf_n2v.hip`; control flow, file names and
      checkpoint keys are the reference's.  An existing `f{k}.pt` is loaded instead, as gnn.py:402-405 does: one written by THIS plugin carries the node order its rows are
      sliced by; one the reference trained follows the node-store order of ITS pickled graph (`{structure}.{dup_edge}.graph.pkl` beside the splits directory,
      gnn.py:21-23) - that file is read (opentf_amd/mdl/emb/pyg_reader.py: a restricted unpickler, no torch_geometric) and the rows are re-stacked; without the graph file
      such a table is refused rather than sliced wrong.
  * `skill_vecs = t2v.get_dense_vecs(teamsvecs, vectype='skill')`                                                  (main.py:148)
      the mean-pool `(skill @ E_skill) / skill.sum(1)` (gnn.py:484-486) by the gather kernel, returned as the dense [N, d] matrix the
      caller stores in `teamsvecs['skill']` — AND `teamsvecs['skill_table'] = E_skill` is registered, so that the Fnn / Bnn plugin of this
      package (opentf_amd/mdl/fnn.py) finds the table and runs the gather INSIDE every training step from `original_skill`
      (which main.py:152 stores itself) instead of reading pre-pooled rows.

  * `t2v.test(teamsvecs, splits, testcfg)`; `t2v.evaluate(...)`; `t2v.adila(...)`            (the reference's CI matrix lists Gnn under cmd=[train,test,eval]; gnn.py:512-545)
      the table as a recommender: every member scored for a team by the link decode sigmoid(<E[team], E[member]>) - the logit of v_loss, over the very member-team edges
      learn() held out - on the device (`opentf_amd/csrc/ntf_link.hip`, `libntf.Link`), `.pred` files in this package's Fnn.test's format, then Ntf's evaluate / adila on
      them.  `recommend(skill_rows)` does the same for teams outside the graph from the mean pool of their skills' rows.

Node ids of the homogeneous graph: [skills | members | teams].  (PyG's HeteroData orders the three blocks by Python set iteration, i.e.
arbitrarily per process; consumers select by type, gnn.py:505-509, so the order is not part of the contract.)

The metapath2vec method (`...Gnn_m2v`) goes through the same loop: `torch_geometric.nn.MetaPath2Vec` over the metapath of the `m2v` section (`_metapath`), per-hop
CSRs of the same stm structure (`m2v_graph`), the table [members | skills | teams | dummy row] (PyG sorts the type names; `Embedding(count + 1, d)`), the loader over
the metapath's start type, walks of `wl` STEPS (= wl + 1 nodes on the device).  INTEGRATION.md §2b lists what is not pinned against the reference tree.
"""
from __future__ import annotations

import logging
import os
import re
import time

import numpy as np
import scipy.sparse

from ..earlystopping import EarlyStopping, PlateauLR
from ..fnn import index_order, parse_devices
from ..ntf import Ntf, cfg_get, coo_from_topk, dist_rank, summary_writer, topk_sparse
from .t2v import T2v, gather_meanpool

log = logging.getLogger(__name__)


def _csr(mat):
    m = scipy.sparse.csr_matrix(mat)
    m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int64)


def stm_graph(skill, member, drop_teams=()):
    """(rowptr int64, col int32, offsets, num_nodes) of the undirected skill-team-member graph; member-team edges of `drop_teams` removed"""
    s_ip, s_ix = _csr(skill)
    m_ip, m_ix = _csr(member)
    n_team, S, M = skill.shape[0], skill.shape[1], member.shape[1]
    off = {"skill": 0, "member": S, "team": S + M}
    n = S + M + n_team
    team_of_s = np.repeat(np.arange(n_team, dtype=np.int64), np.diff(s_ip))
    team_of_m = np.repeat(np.arange(n_team, dtype=np.int64), np.diff(m_ip))
    keep = ~np.isin(team_of_m, np.asarray(list(drop_teams), dtype=np.int64))
    src = np.concatenate([s_ix + off["skill"], m_ix[keep] + off["member"]])
    dst = np.concatenate([team_of_s + off["team"], team_of_m[keep] + off["team"]])
    a, b = np.concatenate([src, dst]), np.concatenate([dst, src])
    order = np.lexsort((b, a))
    a, b = a[order], b[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, a + 1, 1)
    return np.cumsum(rowptr), b.astype(np.int32), off, n


def member_team_edges(member, teams, off):
    """homogeneous (member node, team node) pairs of the given teams, both directions (gnn.py:100-104,118-124)"""
    sub = scipy.sparse.csr_matrix(member)[np.asarray(teams, dtype=np.int64)]
    t = np.repeat(np.asarray(teams, dtype=np.int64), np.diff(sub.indptr)) + off["team"]
    m = sub.indices.astype(np.int64) + off["member"]
    return np.concatenate([m, t]), np.concatenate([t, m])


NODE_ORDER = "skill|member|team"     # row blocks of the table this plugin trains (stm_graph)

# ---- metapath2vec (`m2v`): torch_geometric.nn.MetaPath2Vec's table - the node types sorted by name, then the dummy row
M2V_TYPES = ("member", "skill", "team")
M2V_ORDER = "|".join(M2V_TYPES) + "|dummy"
_M2V_RELATIONS = ("to", "rev_to")


def _metapath(cfg):
    """(list of (src, rel, dst), label or None) of the m2v section's `metapath_name` (the ONE place that key is read): either `[[triples...], "label"]`, as
    `graph.structure` is written, or a bare list of triples.  Checked here, before any device call: relations `to` / `rev_to`, node types skill / member / team
    (anything else, `loc` included, is not built here), every hop one of the four skill-team / member-team directions, a chain (a hop's destination is the next
    hop's source), and all three types present (the skill block feeds get_dense_vecs, v_loss needs member and team rows)."""
    raw = cfg_get(cfg_get(cfg, "m2v"), "metapath_name")
    if raw is None or isinstance(raw, str) or len(raw) == 0:
        raise ValueError("m2v: metapath_name must be a list of [src, rel, dst] triples, or [[triples...], 'label']")
    raw, label = list(raw), None
    if len(raw) == 2 and isinstance(raw[1], str) and not isinstance(raw[0], str) and len(raw[0]) and not isinstance(raw[0][0], str):
        raw, label = list(raw[0]), raw[1]
    path = []
    for hop in raw:
        if isinstance(hop, str) or len(hop) != 3 or not all(isinstance(x, str) for x in hop):
            raise ValueError(f"m2v: a metapath entry must be a [src, rel, dst] triple of names, got {hop!r}")
        s, r, d = (str(x) for x in hop)
        if r not in _M2V_RELATIONS: raise NotImplementedError(f"m2v: relation {r!r} (only {_M2V_RELATIONS} are built here)")
        for t in (s, d):
            if t not in M2V_TYPES: raise NotImplementedError(f"m2v: node type {t!r} (only {M2V_TYPES} are built here)")
        if "team" not in (s, d) or s == d: raise NotImplementedError(f"m2v: no {s} -> {d} edges in the skill-team-member graph")
        path.append((s, r, d))
    for a, b in zip(path[:-1], path[1:]):
        if a[2] != b[0]: raise ValueError(f"m2v: the metapath does not chain: {a} is followed by {b}")
    missing = [t for t in M2V_TYPES if t not in {x for s, _, d in path for x in (s, d)}]
    if missing: raise ValueError(f"m2v: the metapath must visit skill, member and team; missing {missing}")
    return path, label


def m2v_graph(skill, member, drop_teams, metapath):
    """(type counts in table order, offsets {type: first row} + 'dummy', hops [(src id, dst id, rowptr int64, col int32 LOCAL ids)]) of a metapath over the stm
    structure.  The CSR of a hop is chosen by its (src, dst) types alone: skill -> team is skill.T, team -> skill is skill, member -> team / team -> member are
    member.T / member without the rows of `drop_teams` (exactly the member-team edges stm_graph drops)."""
    skill = scipy.sparse.csr_matrix(skill); member = scipy.sparse.csr_matrix(member)
    keep = np.ones(member.shape[0], dtype=bool); keep[np.asarray(list(drop_teams), dtype=np.int64)] = False
    member = scipy.sparse.diags(keep.astype(member.dtype)) @ member
    member.eliminate_zeros()
    count = {"member": member.shape[1], "skill": skill.shape[1], "team": skill.shape[0]}
    mats = {("skill", "team"): lambda: skill.T, ("team", "skill"): lambda: skill, ("member", "team"): lambda: member.T, ("team", "member"): lambda: member}
    off, at = {}, 0
    for t in M2V_TYPES: off[t] = at; at += count[t]
    off["dummy"] = at
    csr, hops = {}, []
    for s, _, d in metapath:
        if (s, d) not in csr:
            rp, cl = _csr(mats[(s, d)]())
            csr[(s, d)] = (rp, cl.astype(np.int32))
        hops.append((M2V_TYPES.index(s), M2V_TYPES.index(d), *csr[(s, d)]))
    return [count[t] for t in M2V_TYPES], off, hops


def _barrier():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


_WAIT_GROUP = None


def _wait_group():
    """a gloo group of its own with a week's timeout: the ranks other than 0 sit in a collective on it for as long as rank 0 trains a fold (up to cfg.e epochs) -
    on the default group that wait is cut by the process group's watchdog after 10 (nccl) / 30 (gloo) minutes and the job is torn down"""
    global _WAIT_GROUP
    import datetime
    import torch.distributed as dist
    if _WAIT_GROUP is None:
        _WAIT_GROUP = dist.new_group(backend="gloo", timeout=datetime.timedelta(days=7))       # a collective itself: learn() creates it up front, where the ranks are together
    return _WAIT_GROUP


def _sync_torch_rng():
    """rank 0's torch CPU generator state on every rank (a collective: also orders the ranks behind rank 0's file writes); on the long-timeout group, see _wait_group"""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return
    box = [torch.get_rng_state() if dist.get_rank() == 0 else None]
    dist.broadcast_object_list(box, src=0, group=_wait_group(), device=torch.device("cpu"))
    if dist.get_rank() != 0: torch.set_rng_state(box[0])


def _rank0_says(flag):
    """rank 0's value of a bool on every rank (file-system checks that must come out the same job-wide)"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return bool(flag)
    box = [bool(flag)]
    dist.broadcast_object_list(box, src=0)
    return box[0]


class Gnn(T2v):
    def __init__(self, output, device, seed, cfg, model):
        super().__init__(output, device, seed, cfg, model)
        if self.name not in ("n2v", "m2v"):
            raise NotImplementedError(f"opentf_amd trains the random-walk tables (n2v, m2v) on the device; '{self.name}' stays the reference's mdl.emb.gnn.Gnn")
        self.metapath, self.metapath_label = _metapath(cfg) if self.name == "m2v" else (None, None)      # refused here, before any device call
        if self.metapath and int(cfg_get(self._mcfg(), "wl") or 0) > len(self.metapath) and self.metapath[-1][2] != self.metapath[0][0]:
            raise ValueError("m2v: wl steps outrun the metapath, which does not end on its start type")
        if self._lazy() and self._sparse():     # before any device call, as above
            raise ValueError(f"{self.name}: `lazy` is a mode of dense Adam and `sparse` another optimiser; set one of them")
        self.writer = summary_writer()
        self.offsets = None
        self.blocks = None      # {node type: (first row, end row)} of the loaded table
        self.n_nodes = None     # rows of the table learn() trained or loaded
        self._link = self._link_table = None      # the libntf.Link test() / recommend() keep, and the table it holds

    def _mcfg(self):
        return cfg_get(self.cfg, self.name)

    def _sparse(self):
        """the `sparse` key of the n2v / m2v section (Node2Vec / MetaPath2Vec(sparse=True) trained with torch.optim.SparseAdam); absent or false: dense Adam"""
        return bool(cfg_get(self._mcfg(), "sparse"))

    def _lazy(self):
        """the `lazy` key of the n2v / m2v section: dense Adam that writes only the rows a batch names (ntf_n2v_set_lazy).  The table is dense Adam's, bit for bit,
        so the key is not part of the directory name and a lazy run may load or leave an f{k}.pt of a plain dense run"""
        return bool(cfg_get(self._mcfg(), "lazy"))

    def _bias(self):
        """(p, q) of the n2v section (src/mdl/emb/__config__.yaml:69-70), absent = 1.0; m2v ignores the keys, as MetaPath2Vec has neither"""
        if self.name != "n2v": return 1.0, 1.0
        p, q = cfg_get(self._mcfg(), "p"), cfg_get(self._mcfg(), "q")
        return (1.0 if p is None else float(p)), (1.0 if q is None else float(q))

    def _dirname(self):
        m, g = self._mcfg(), cfg_get(self.cfg, "graph")
        structure = cfg_get(g, "structure")
        name = (f"/{self.name}.b{cfg_get(m, 'b')}.e{cfg_get(m, 'e')}.ns{cfg_get(m, 'ns')}.lr{cfg_get(m, 'lr')}.es{cfg_get(m, 'es')}.spe{cfg_get(m, 'spe')}"
                f".d{cfg_get(m, 'd')}.{cfg_get(g, 'dup_edge')}.{structure[1]}")
        name += ".pre" if cfg_get(g, "pre") else ""
        name += f".w{cfg_get(m, 'w')}.wl{cfg_get(m, 'wl')}.wn{cfg_get(m, 'wn')}"
        name += f".{self.metapath_label}" if self.name == "m2v" and self.metapath_label else ""
        p, q = self._bias()
        name += f".p{float(p)}.q{float(q)}" if (p != 1.0 or q != 1.0) else ""      # default runs keep the reference's name; biased tables never share an f{k}.pt with them
        return name + (".sparse" if self._sparse() else "")      # the last part: tables of the two optimisers never share an f{k}.pt

    def learn(self, teamsvecs, splits=None, time_indexes=None):
        import torch
        from ... import libntf
        m = self._mcfg()
        structure = cfg_get(cfg_get(self.cfg, "graph"), "structure")
        if structure[1] != "stm":
            raise NotImplementedError("only the skill-team-member ('stm') graph structure is built here")
        self.graph_file = self.output + f"/../{structure[1]}.{cfg_get(cfg_get(self.cfg, 'graph'), 'dup_edge') or 'dup'}.graph.pkl"      # gnn.py:21
        self.output += self._dirname()
        os.makedirs(self.output, exist_ok=True)
        skill = teamsvecs.get("original_skill", teamsvecs["skill"]) if hasattr(teamsvecs, "get") else teamsvecs["skill"]
        member = teamsvecs["member"]
        d = int(cfg_get(m, "d"))
        w = None
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            _barrier(); _wait_group()      # the long-timeout group is made HERE, all ranks arriving together: made lazily inside _sync_torch_rng, rank 0 would reach new_group only
                                           # after training the whole first fold, and the others' wait inside gloo's connect would be cut by the store's own (short) timeout
        for foldidx in splits["folds"].keys():
            drop = np.concatenate([np.asarray(splits["test"]), np.asarray(splits["folds"][foldidx]["valid"])])
            seed = int(self.seed or 0) + 7919 * int(foldidx)
            if self.name == "m2v":
                counts, off, hops = m2v_graph(skill, member, drop, self.metapath)
                n, n_start = off["dummy"] + 1, counts[hops[0][0]]
            else:
                rowptr, col, off, n = stm_graph(skill, member, drop)
                n_start = n
            self.offsets, self.n_nodes = off, n
            init = torch.nn.Embedding(n, d).weight.detach().numpy()       # the draw Node2Vec's / MetaPath2Vec's constructor makes (gnn.py:153-160): Embedding(count + 1, d) for m2v
            if self.name == "m2v": make_net = lambda: libntf.MetaPath2Vec(counts, hops, init, seed=seed, device=parse_devices(self.device)[0], sparse=self._sparse(), lazy=self._lazy())
            else:
                p, q = self._bias()
                make_net = lambda: libntf.Node2Vec(rowptr, col, init, seed=seed, device=parse_devices(self.device)[0], sparse=self._sparse(), p=p, q=q, lazy=self._lazy())
            path = f"{self.output}/f{foldidx}.pt"
            _barrier()                                                     # torchrun: nobody looks for the file while rank 0 may still be writing the previous one
            if not _rank0_says(os.path.exists(path)):                      # gnn.py:402-405: a trained table is loaded, not retrained (rank 0 decides for the job)
                # ONE trainer (as d2v.py): the table's gradient sums are f32 atomics - run per rank, losses, early-stop epochs and tables would differ between
                # the ranks - and no collective sits inside a loop whose trip count a rank decides for itself; the other ranks wait below and read rank 0's file
                if dist_rank() == 0:
                    if w is None: w = self.writer(log_dir=f"{self.output}/logs4tboard/run_{int(time.time())}")
                    self._train_fold(make_net, n_start, member, splits, foldidx, off, m, w, path)
                _sync_torch_rng()                                          # (also the barrier) the trainer's loader shuffles consumed torch's CPU generator: the next fold's initial draw stays job-wide
            self.model = self._load_fold(path, off, n)
        if w is not None: w.close()

    def _train_fold(self, make_net, n, member, splits, foldidx, off, m, w, path):
        """`_train_rw` (gnn.py:401-453) for one fold on this rank's device; writes f{k}.e{e}.pt / f{k}.pt.  n: the loader's range - every node for n2v, the nodes of
        the metapath's start type for m2v (MetaPath2Vec.loader: range(num_nodes_dict[metapath[0][0]]))"""
        b, lr = int(cfg_get(m, "b")), float(cfg_get(m, "lr"))
        wl, ctx, wn, ns = int(cfg_get(m, "wl")), int(cfg_get(m, "w")), int(cfg_get(m, "wn")), int(cfg_get(m, "ns"))
        spe = cfg_get(m, "spe")
        val_src, val_dst = member_team_edges(member, splits["folds"][foldidx]["valid"], off)
        assert len(val_src), "Empty valid member-team edge set!"
        if self.name == "m2v": wl += 1              # MetaPath2Vec's walk_length counts STEPS, the device counts nodes per walk
        net = make_net()
        scheduler = PlateauLR(lr, factor=0.1, patience=2)
        earlystopping = EarlyStopping(patience=int(cfg_get(m, "es")), verbose=True, delta=0, trace_func=log.info)
        cur_lr, e, t_loss, v_loss = lr, -1, 0.0, 0.0
        for e in range(int(cfg_get(m, "e"))):
            order = index_order(n, b, True)                            # DataLoader(range(num_nodes), batch_size=b, shuffle=True)
            nb, t_loss = 0, 0.0
            for o in range(0, n, b):
                t_loss += net.train_batch(order[o:o + b], wl, ctx, wn, ns, cur_lr); nb += 1
            t_loss /= nb
            v_loss = net.edge_bce(val_src, val_dst) / len(val_src)     # the reference divides the mean once more (gnn.py:433)
            w.add_scalar(tag=f"{foldidx}_t_loss", scalar_value=t_loss, global_step=e)
            w.add_scalar(tag=f"{foldidx}_v_loss", scalar_value=v_loss, global_step=e)
            log.info(f"Fold {foldidx}/{len(splits['folds']) - 1}, Epoch {e}, Train Loss: {t_loss:.4f}, Valid Loss: {v_loss:.4f}")
            if spe and (e == 0 or ((e + 1) % spe) == 0):
                self._save(net.weight(), foldidx, e, t_loss, v_loss, f"{self.output}/f{foldidx}.e{e}.pt")
            cur_lr = scheduler.step(v_loss)
            if earlystopping(v_loss, None).early_stop:
                log.info(f"Early stopping triggered at epoch: {e}")
                break
        weight = net.weight()
        net.close()
        self._save(weight, foldidx, e, t_loss, v_loss, path)

    def _load_fold(self, path, off, n):
        """gnn.py:402-405.  A table THIS plugin saved carries its node order ([skills | members | teams], stm_graph).  A table the reference trained follows the order in
        which its pickled HeteroData holds the node stores (src/mdl/emb/gnn.py:29-47: the iteration order of a Python set, recorded only in `*.graph.pkl`): that file is
        read and the row blocks are re-stacked; a foreign table without its graph file is refused - sliced by the wrong order it would train silently on the wrong rows."""
        from . import pyg_reader
        ref = pyg_reader.reference_table(path)      # restricted unpickler, the ONLY load of the file: the pickled cfg (omegaconf or not) resolves to inert holders, this plugin's
                                                    # node_order / node_offsets markers are plain builtins and come through it - plugin or reference is decided from those alone
        if getattr(self, "name", "n2v") == "m2v":
            return self._load_fold_m2v(path, ref, off, n)
        self.blocks = {"skill": (off["skill"], off["member"]), "member": (off["member"], off["team"]), "team": (off["team"], n)}
        if ref["node_order"] is not None and ref["node_order"] != NODE_ORDER:
            raise RuntimeError(f"{path}: node order {ref['node_order']!r}, this build writes and reads {NODE_ORDER!r}")
        if ref["node_order"] == NODE_ORDER:
            if ref["node_offsets"] != (off["skill"], off["member"], off["team"], n):
                raise RuntimeError(f"{path}: written for node offsets {ref['node_offsets']}, teamsvecs gives {(off['skill'], off['member'], off['team'], n)}")
            log.info(f"Loading the model {path} ...")
            return ref["weight"]
        graph = getattr(self, "graph_file", None)
        if not graph or not os.path.exists(graph):
            raise RuntimeError(f"{path} was not written by opentf_amd.mdl.emb.gnn and the graph file that holds its node order ({graph}) is missing: "
                               "remove the table to retrain it on the device, or put the reference's *.graph.pkl back")
        blocks = pyg_reader.node_blocks(graph)
        weight, counts = pyg_reader.blocks_to_order(ref["weight"], blocks, NODE_ORDER.split("|"))
        want = {"skill": off["member"] - off["skill"], "member": off["team"] - off["member"], "team": n - off["team"]}
        if counts != want:
            raise RuntimeError(f"{path}: the graph {graph} has {counts} nodes, teamsvecs has {want}")
        log.info(f"Loading the model {path} (trained by the reference: rows re-stacked from {[t for t, _ in blocks]} of {os.path.basename(graph)}) ...")
        return weight

    def _load_fold_m2v(self, path, ref, off, n):
        """MetaPath2Vec orders its row blocks by the sorted type names, whatever the process: a table without this plugin's marker (one the reference trained) is
        accepted when its row count is total + 1, and refused otherwise; a marked one must carry this order and these offsets."""
        want = tuple(off[t] for t in M2V_TYPES) + (n,)
        if ref["node_order"] is not None:
            if ref["node_order"] != M2V_ORDER:
                raise RuntimeError(f"{path}: node order {ref['node_order']!r}, an m2v table of this build has {M2V_ORDER!r}")
            if ref["node_offsets"] != want:
                raise RuntimeError(f"{path}: written for node offsets {ref['node_offsets']}, teamsvecs gives {want}")
        elif ref["weight"].shape[0] != n:
            raise RuntimeError(f"{path}: {ref['weight'].shape[0]} rows without a node order marker; teamsvecs gives {n} "
                               f"({' + '.join(M2V_TYPES)} + the dummy row)")
        self.blocks = {t: (off[t], off[u]) for t, u in zip(M2V_TYPES, M2V_TYPES[1:] + ("dummy",))}
        log.info(f"Loading the model {path} ...")
        return ref["weight"]

    def _save(self, weight, foldidx, e, t_loss, v_loss, path):
        """keys and order of gnn.py:445,453, + the node order the rows are sliced by (the first row of each block, then the row count); written whole, then moved
        into place.  Called by the training rank only: no collective"""
        import torch
        off = self.offsets
        order = M2V_ORDER if self.name == "m2v" else NODE_ORDER
        tmp = f"{path}.tmp.{os.getpid()}"
        torch.save({"model_state_dict": {"embedding.weight": torch.from_numpy(np.ascontiguousarray(weight))}, "cfg": self.cfg, "f": foldidx, "e": e,
                    "t_loss": t_loss, "v_loss": v_loss, "node_order": order,
                    "node_offsets": tuple(int(off[t]) for t in order.split("|") if t != "dummy") + (int(weight.shape[0]),)}, tmp)
        os.replace(tmp, path)

    def _node_emb(self, teamsvecs, node_type):
        if self.model is None:
            raise RuntimeError("no trained table: call learn() first")
        lo, hi = self.blocks[node_type]          # the row blocks of the table _load_fold loaded
        return self.model[lo:hi]

    def get_dense_vecs(self, teamsvecs, vectype="skill"):
        """gnn.py:484-486.  For 'skill' the table is also registered as teamsvecs['skill_table'] (see the module docstring)."""
        if vectype not in ("skill", "member") or vectype not in teamsvecs:
            return self._node_emb(teamsvecs, vectype)
        table = np.ascontiguousarray(self._node_emb(teamsvecs, vectype), dtype=np.float32)
        rows = teamsvecs.get("original_skill", teamsvecs[vectype]) if (vectype == "skill" and hasattr(teamsvecs, "get")) else teamsvecs[vectype]
        dense = gather_meanpool(rows, table, self.device)
        if vectype == "skill":
            teamsvecs["skill_table"] = table
        return dense

    # ---- the table as a recommender (src/mdl/emb/gnn.py:512-545): every member scored for a team by the link decode sigmoid(<E[team], E[member]>), the logit of
    # v_loss over exactly the member-team edges learn() held out (include/opentf_amd_link.h; INTEGRATION.md §2b: PyG's dot-product decode restated, not pinned)
    is_bayesian = False
    evaluate = Ntf.evaluate      # both need `output`, `cfg` and `seed` only; they read the .pred files test() writes
    adila = Ntf.adila
    _eval_engine = Ntf._eval_engine      # NTF_EVAL_ENGINE=1: "Gnn owns no engine", the files are read

    def _link_for(self, table):
        """the Link over `table` with the member block as candidates; one handle is kept, a new table replaces it"""
        from ... import libntf
        if self._link is None or self._link_table is not table:
            self.close()
            lo, hi = self.blocks["member"]
            self._link, self._link_table = libntf.Link(table, lo, hi, device=parse_devices(self.device)[0]), table
        return self._link

    def close(self):
        """frees the device handle test() / recommend() keep"""
        if self._link is not None:
            self._link.close()
        self._link = self._link_table = None

    def test(self, teamsvecs, splits, testcfg):
        """The flow of this package's Fnn.test: per fold `f{k}.pt` (+ `f{k}.e{e}.pt` with per_epoch) through _load_fold, the teams of the pred set as QUERY ROWS of
        the table (team block start + team id: no vector crosses the host), the member block as candidates (member id = row - member block start), and
        `f{k}.{set}.[e{e}.]pred` = {'y_pred': sparse COO of the topK probabilities (topK < M) or the dense [n, M] probabilities, 'uncertainty': None}."""
        import torch
        from ... import libntf
        self._node_emb(teamsvecs, "member")      # RuntimeError before learn()
        assert os.path.isdir(self.output), f"No folder for {self.output} exist!"
        if dist_rank() != 0:                     # one writer, as Fnn.test: the others wait so that evaluate() finds complete files
            _barrier(); return
        learned = self.model
        (m_lo, m_hi), t_lo = self.blocks["member"], self.blocks["team"][0]
        M = m_hi - m_lo
        topK = cfg_get(testcfg, "topK")
        sparse_out = bool(topK) and topK < M
        on_gpu_topk = sparse_out and topK <= libntf.Link.MAX_K
        for foldidx in splits["folds"].keys():
            modelfiles = [f"{self.output}/f{foldidx}.pt"]
            if cfg_get(testcfg, "per_epoch"):
                modelfiles += [f"{self.output}/{_}" for _ in os.listdir(self.output) if re.match(rf"f{foldidx}.e\d+.pt", _)]
            for modelfile in sorted(sorted(modelfiles), key=len):
                link = self._link_for(self._load_fold(modelfile, self.offsets, self.n_nodes))
                for pred_set in (["test", "train", "valid"] if cfg_get(testcfg, "on_train") else ["test"]):
                    teams = np.asarray(splits["test"] if pred_set == "test" else splits["folds"][foldidx][pred_set], dtype=np.int64)
                    rows = teams + t_lo
                    if len(rows) == 0:
                        y_pred = torch.empty(0, M)
                    elif on_gpu_topk:
                        idx, _, prob = link.topk(rows=rows, K=int(topK))
                        y_pred = coo_from_topk(prob, idx, (len(rows), M))
                    else:
                        y_pred = torch.from_numpy(link.dense(rows=rows, logit=False)[1])
                        if sparse_out:
                            y_pred = topk_sparse(y_pred, int(topK))
                    match = re.search(r"(e\d+)\.pt$", os.path.basename(modelfile))
                    epoch = (match.group(1) + ".") if match else ""
                    torch.save({"y_pred": y_pred, "uncertainty": None}, f"{self.output}/f{foldidx}.{pred_set}.{epoch}pred", pickle_protocol=4)
                    log.info(f"{self.name} model predictions for fold{foldidx}.{pred_set}.{epoch} has saved at {self.output}/f{foldidx}.{pred_set}.{epoch}pred")
        self.model = learned                     # get_dense_vecs keeps reading the table learn() left
        _barrier()

    def recommend(self, skill_rows, topn=10):
        """Teams that are not in the graph: each row of `skill_rows` (scipy sparse [n, S], or a list of skill-id lists) is the mean pool of its skills' rows of the
        table - get_dense_vecs' pool, on the device - scored against every member.  -> (idx [n, topn] int32 member ids, prob [n, topn] f32), best first."""
        self._node_emb(None, "member")           # RuntimeError before learn()
        s_lo, s_hi = self.blocks["skill"]
        if hasattr(skill_rows, "tocsr"):
            ptr, items = _csr(skill_rows)
        else:
            lists = [np.asarray(r, dtype=np.int64).reshape(-1) for r in skill_rows]
            ptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
            items = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, dtype=np.int64)
        if len(items) and (items.min() < 0 or items.max() >= s_hi - s_lo):
            raise ValueError(f"recommend: a skill id outside [0, {s_hi - s_lo})")
        idx, _, prob = self._link_for(self.model).topk(pooled=(ptr, items + s_lo), K=int(topn))
        return idx, prob
