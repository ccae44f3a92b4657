"""Host references of the doc2vec kernels (opentf_amd/csrc/ntf_d2v.hip) for tests/test_d2v_paths_host.py and tests/test_gpu_d2v_paths.py.  HELPERS, no test.

reference_train   oracle.d2v_oracle.train_epoch's arithmetic (its draw, sigmoid_table and epoch_key), bit for bit, that also counts what a test has to know about a
                  case: units run, units skipped for |f| >= 6, FLAGGED units (f within 16 * 2^-24 * sum |l1_q syn1neg_q| of a bin edge of the sigmoid table or of
                  +-6, where another summation order may take another bin: a discrete jump, not rounding), negative draws equal to the predicted word, the largest
                  context and the largest PV-DBOW unit index
reference_infer   the sequential infer_vector of tests/test_gpu_d2v_infer.py, moved here unchanged
variants          four WRONG trainers, written as variants of the reference (never of device code), whose distance from it the host test measures - a parity case
                  that a wrong kernel of that kind would pass checks nothing:
                    "no_flush"   PV-DM additions to a word row deferred until the position leaves every later window (reach 2 * 5), a window row read as memory +
                                 the pending sum of ITS OWN position - without the flush when one reach holds the same word twice
                    "top_le"     the two-level search of the cumulative table with `<=` for `<` at the first level
                    "neg1_lost"  draws 5 to 8 taken from the first Philox word
                    "window5"    the shrink b = draw % 5 whatever the window
cases             every trainer case runs serial, one pass (epoch 0), alpha 0.025 -> 0.02, tables N(0, 0.1^2) from TABLE_SEED[name] (default 0): the first seed
                  at which the reference flags at most 2 units and meets the other conditions of tests/test_d2v_paths_host.py.
"""
import functools

import numpy as np

from oracle import d2v_oracle as D
from opentf_amd.mdl.emb import d2v as P

EPS = 2.0 ** -24
ALPHA0, ALPHA1, SEED = 0.025, 0.02, 3
BAR = 2e-5            # tests/test_gpu_d2v.py's bar for a serial pass (case `zipf`: 4 800 kept positions through 60 rows of syn1neg); no case here has more kept positions
DEFER_WINDOW = 5      # the window at which the launcher takes the deferred PV-DM kernel


def _bin(f):
    """what the unit does with f: below / above the table, or its bin (the f32 arithmetic of D.sigmoid_table)"""
    f = np.float32(f)
    if f <= -D.MAX_EXP: return -1
    if f >= D.MAX_EXP: return D.EXP_TABLE_SIZE
    return int((f + np.float32(D.MAX_EXP)) * np.float32(D.EXP_TABLE_SIZE / D.MAX_EXP / 2))


# ------------------------------------------------------------------------------------------------ the trainer
def _target(cum, v, variant):
    if variant != "top_le": return int(np.searchsorted(cum, np.uint32(v), side="left"))
    V = len(cum)
    top_s = (V + 1023) // 1024
    top = cum[np.minimum((np.arange((V + top_s - 1) // top_s) + 1) * top_s, V) - 1]
    b = int(np.searchsorted(top, np.uint32(v), side="right"))          # the first bucket whose last entry is > v: one too far when v EQUALS a bucket's last entry
    lo, hi = b * top_s, min((b + 1) * top_s, V)
    return lo + int(np.searchsorted(cum[lo:hi], np.uint32(v), side="left"))


def _unit(x, word, syn1neg, cum, alpha, key, doc, pos, unit, negative, st, variant):
    work = np.zeros_like(x)
    r = None
    for k in range(negative + 1):
        if k == 0: target, label = word, np.float32(1)
        else:
            if r is None: r = D.draw(key, doc, pos, unit, D.SLOT_NEG0) + D.draw(key, doc, pos, unit, D.SLOT_NEG0 if variant == "neg1_lost" else D.SLOT_NEG1)
            target = _target(cum, r[k - 1] % int(cum[-1]), variant)
            if target == word:
                st["self_draws"] += 1
                continue
            label = np.float32(0)
        x64, r64 = x.astype(np.float64), syn1neg[target].astype(np.float64)
        f64 = np.dot(x64, r64)
        margin = 16 * EPS * float(np.dot(np.abs(x64), np.abs(r64)))
        st["units"] += 1
        if _bin(f64 - margin) != _bin(f64 + margin): st["flagged"] += 1
        f = np.float32(f64)
        if f <= -D.MAX_EXP or f >= D.MAX_EXP:
            st["skipped"] += 1
            continue
        s = D.sigmoid_table(f)
        st["loss_sum"] += -np.log(max(float(s if label else 1 - s), 1e-30)); st["loss_n"] += 1
        g = np.float32((label - s) * np.float32(alpha))
        work += g * syn1neg[target]
        syn1neg[target] += g * x
    return work


def reference_train(doc_ptr, words_v, sample_int, cum, wv, dv, syn1neg, dm, window, negative, alpha_start, alpha_end, seed, epoch, order=None, progress=None, variant=None):
    """one sequential pass, in place -> dict(loss, units, skipped, flagged, self_draws, kept, max_ctx, max_unit)"""
    key = D.epoch_key(seed, epoch)
    n = len(doc_ptr) - 1
    order = np.arange(n) if order is None else np.asarray(order)
    si = [int(x) for x in sample_int]
    st = dict(units=0, skipped=0, flagged=0, self_draws=0, kept=0, max_ctx=0, max_unit=0, loss_sum=0.0, loss_n=0)
    no_flush = variant == "no_flush" and dm and window == DEFER_WINDOW
    zero = np.zeros(wv.shape[1], np.float32)
    for rank, doc in enumerate(order.tolist()):
        alpha = np.float32(alpha_start - (alpha_start - alpha_end) * (rank / n if progress is None else float(progress[rank])))
        w = words_v[doc_ptr[doc]:doc_ptr[doc + 1]]
        kept = [int(x) for p, x in enumerate(w.tolist()) if si[x] >= D.draw(key, doc, p, 0, D.SLOT_KEEP)[0]][:D.MAX_DOCUMENT_LEN]
        K = len(kept)
        st["kept"] += K
        pend = {}
        for i in range(K):
            b = D.draw(key, doc, i, 0, D.SLOT_WINDOW)[0] % (5 if variant == "window5" else window)
            lo, hi = max(0, i - window + b), min(K, i + window + 1 - b)
            ctx = [m for m in range(lo, hi) if m != i]
            st["max_ctx"] = max(st["max_ctx"], len(ctx))
            if dm:
                l1 = dv[doc].copy()
                for m in ctx: l1 += wv[kept[m]] + pend.get(m, zero) if no_flush else wv[kept[m]]
                l1 *= np.float32(1.0) / np.float32(len(ctx) + 1)
                work = _unit(l1, kept[i], syn1neg, cum, alpha, key, doc, i, 0, negative, st, variant)
                dv[doc] += work
                if no_flush:
                    for m in ctx: pend[m] = pend.get(m, zero) + work
                    if i - DEFER_WINDOW >= 0: wv[kept[i - DEFER_WINDOW]] += pend.pop(i - DEFER_WINDOW, zero)
                else:
                    for m in ctx: wv[kept[m]] += work
            else:
                for u, m in enumerate(ctx):
                    wv[kept[m]] += _unit(wv[kept[m]].copy(), kept[i], syn1neg, cum, alpha, key, doc, i, 1 + u, negative, st, variant)
                    st["max_unit"] = max(st["max_unit"], 1 + u)
                dv[doc] += _unit(dv[doc].copy(), kept[i], syn1neg, cum, alpha, key, doc, i, 0, negative, st, variant)
        for m in sorted(pend): wv[kept[m]] += pend[m]
    st["loss"] = st.pop("loss_sum") / max(st.pop("loss_n"), 1)
    return st


# ------------------------------------------------------------------------------------------------ infer_vector
def reference_infer(q_ptr, q_words, ids, init, wv, s1, sample_int, cum, dm, window, negative, epochs, alpha, min_alpha, seed):
    """the issue's / the header's semantics, one query after the other: f32 vectors, f in f64 rounded once.  -> (out [n, d], flagged units per query, units, units
    skipped for |f| >= 6).  A unit is flagged when f lies within 16 * 2^-24 * sum |l1_q syn1neg_q| of a bin edge or of +-6: the device sums f in another order (at
    most 4 sequential adds, 6 tree levels, 1 product rounding; headroom for the drift of v), and another bin is a discrete jump, not rounding."""
    n = len(q_ptr) - 1
    out = np.array(init, dtype=np.float32, copy=True)
    flagged = np.zeros(n, dtype=np.int64)
    units = skipped = 0
    delta = (alpha - min_alpha) / max(epochs - 1, 1)
    si = [int(x) for x in sample_int]
    for i in range(n):
        v = out[i].copy()
        doc = int(ids[i]) if ids is not None else i
        w = [int(x) for x in q_words[q_ptr[i]:q_ptr[i + 1]]]
        a = alpha
        for e in range(epochs):
            key = D.epoch_key(seed, e)
            af = np.float32(a)
            kept = [x for p, x in enumerate(w) if si[x] >= D.draw(key, doc, p, 0, D.SLOT_KEEP)[0]][:D.MAX_DOCUMENT_LEN]
            K = len(kept)
            for pos in range(K):
                b = D.draw(key, doc, pos, 0, D.SLOT_WINDOW)[0] % window
                lo, hi = max(0, pos - window + b), min(K, pos + window + 1 - b)
                if dm:
                    l1 = v.copy()
                    for m in range(lo, hi):
                        if m != pos: l1 += wv[kept[m]]
                    l1 *= np.float32(1.0) / np.float32(hi - lo)
                else:
                    l1 = v
                work = np.zeros_like(v)
                r = D.draw(key, doc, pos, 0, D.SLOT_NEG0) + D.draw(key, doc, pos, 0, D.SLOT_NEG1)
                for k in range(negative + 1):
                    if k == 0: t, label = kept[pos], np.float32(1)
                    else:
                        t = int(np.searchsorted(cum, np.uint32(r[k - 1] % int(cum[-1])), side="left"))
                        if t == kept[pos]: continue
                        label = np.float32(0)
                    prod = l1.astype(np.float64) * s1[t].astype(np.float64)
                    f64 = float(prod.sum())
                    margin = 16 * EPS * float(np.abs(prod).sum())
                    units += 1
                    if _bin(f64 - margin) != _bin(f64 + margin): flagged[i] += 1
                    f = np.float32(f64)
                    if f <= -D.MAX_EXP or f >= D.MAX_EXP:
                        skipped += 1
                        continue
                    g = np.float32((label - D.sigmoid_table(f)) * af)
                    work += g * s1[t]
                v = v + work
            a -= delta
        out[i] = v
    return out, flagged, units, skipped


# ------------------------------------------------------------------------------------------------ vocabularies and corpora
POP = 1.0 / (np.arange(60) + 1.0) ** 1.5
POP /= POP.sum()


def _vocab60():
    """sample_int / cum_table of a 60-word Zipf corpus at sample = 0.05: the two most frequent words (vocabulary indices 0 and 1) are dropped 54 % and 9 % of the time"""
    words = np.random.default_rng(0).choice(60, 20000, replace=True, p=POP).astype(np.int64)
    keys, count, si, cum, wi = P.build_vocab(words, sample=0.05)
    assert len(keys) == 60 and si[0] < 0.6 * 2 ** 32 and si[1] < 2 ** 32 - 1
    return si, cum


def _query_words(rng, n):
    """vocabulary indices drawn by the corpus' own frequencies (index = frequency rank): the subsampled words are the common ones"""
    return rng.choice(60, n, replace=True, p=POP).astype(np.int32)


def _csr(docs):
    return np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.int64), np.concatenate([np.asarray(x, np.int64) for x in docs])


def _built(ptr, words, sample):
    keys, count, si, cum, wi = P.build_vocab(words, sample=sample)
    return ptr, np.asarray(wi, np.int64), si, cum


def search_tables(V):
    """the two hand-made cumulative tables of case D: equality with an entry the common case at both levels and at every bucket end; plateaus, where bisect_left has to
    return the first of equal entries.  The plateaus' last entry stands 8 above the one before it (V odd: one entry appended; V even: the second of the last pair
    raised), so that the one-entry last bucket is drawn; arange never draws its last index (a draw is below cum_table[-1] = cum_table[-2] + 1)"""
    plateaus = np.repeat(np.arange(1, V // 2 + 1), 2)[:V]
    if V % 2: plateaus = np.concatenate([plateaus, [plateaus[-1] + 8]])
    else: plateaus[-1] += 8
    return {"arange": np.arange(1, V + 1).astype(np.uint32), "plateaus": plateaus.astype(np.uint32)}


@functools.lru_cache(maxsize=None)
def corpus(kind, *a):
    """-> (doc_ptr, vocabulary indices of the words, sample_int, cum_table)"""
    if kind == "A":                # 120 documents of 1 + Poisson(7) distinct words over 60, Zipf, the frequent ones subsampled
        rng = np.random.default_rng(0)
        pop = 1.0 / (np.arange(60) + 3.0); pop /= pop.sum()
        ptr, wi, si, cum = _built(*_csr([rng.choice(60, k, replace=False, p=pop) for k in np.minimum(1 + rng.poisson(7, 120), 60)]), 0.05)
        return ptr[:a[0] + 1], wi[:ptr[a[0]]], si, cum          # the first a[0] documents; the vocabulary is the whole corpus'
    if kind == "C":                # 30 fresh words, then a tail of period P: the deferred kernel defers up to the position whose reach first holds a word twice
        return _built(*_csr([np.concatenate([np.arange(100, 130), np.arange(120) % a[0]]), np.arange(200, 220)]), 0)
    if kind == "D":                # V words, no subsampling, a hand-made cumulative table
        V, table = a
        rng = np.random.default_rng(0)
        ptr, words = _csr([rng.integers(0, V, k) for k in 1 + rng.poisson(7, 60)])
        return ptr, words, np.full(V, 0xFFFFFFFF, np.uint32), search_tables(V)[table]
    if kind == "E":                # the accepted limits of the window, documents longer than 2 * window + 1.  Words of a 60-word Zipf law; one document alone:
        rng = np.random.default_rng(2)      # that many DISTINCT words (PV-DBOW at window 127 runs 32 000 positive units: on 60 words every dot product passes 6)
        pop = 1.0 / (np.arange(60) + 3.0); pop /= pop.sum()
        return _built(*_csr([rng.choice(60, k, replace=True, p=pop) for k in a] if len(a) > 1 else [rng.permutation(a[0])]), 0)
    raise KeyError(kind)


def seed_with_a_full_window(n_kept, window, doc=0, epoch=0, first=SEED):
    """the first handle seed >= `first` at which a position with `window` kept words on both sides draws the shrink b = 0 (SLOT_WINDOW alone: no training)"""
    for seed in range(first, first + 200):
        key = D.epoch_key(seed, epoch)
        if any(D.draw(key, doc, i, 0, D.SLOT_WINDOW)[0] % window == 0 for i in range(window, n_kept - window)): return seed
    raise AssertionError("no seed below first + 200")


E_SEED = {1: 3, 0: 7}              # seed_with_a_full_window(600, 255) / (300, 127); test_d2v_paths_host.py asserts both


# PV-DBOW runs one unit per (position, window word).  At (10, 8) the 120 documents make 61 000 units, of which the reference flags 10 to 32 at table seeds 0 to 2
# (the tables grow through the pass): that case alone takes the first 15 documents (7 222 units), at every d
A_DOCS_DBOW = {10: 15}


def _train_specs():
    s = {}
    for dm in (1, 0):
        for w, ng in ((1, 0), (2, 4), (4, 5), (6, 5), (10, 8)):
            for d in (64, 128, 129, 192, 256) if (w, ng) in ((1, 0), (10, 8)) else (128,):
                s[f"A-dm{dm}-w{w}-n{ng}-d{d}"] = dict(corpus=("A", 120 if dm else A_DOCS_DBOW.get(w, 120)), dm=dm, window=w, negative=ng, d=d)
        for V in (1025, 2500):
            for table in ("arange", "plateaus"):
                s[f"D-dm{dm}-V{V}-{table}"] = dict(corpus=("D", V, table), dm=dm, window=3, negative=8, d=64)
    for d in (128, 192, 256): s[f"B-d{d}"] = dict(corpus=("A", 120), dm=1, window=5, negative=5, d=d)
    for p in (3, 5, 8, 9, 10, 11): s[f"C-P{p}"] = dict(corpus=("C", p), dm=1, window=5, negative=5, d=128)
    s["E-dm1"] = dict(corpus=("E", 600, 40), dm=1, window=255, negative=1, d=64, seed=E_SEED[1])
    s["E-dm0"] = dict(corpus=("E", 300), dm=0, window=127, negative=0, d=64, seed=E_SEED[0])
    return s


TRAIN_SPECS = _train_specs()
TABLE_SEED = {"A-dm0-w2-n4-d128": 5, "A-dm0-w6-n5-d128": 6, "A-dm1-w10-n8-d129": 1, "A-dm0-w10-n8-d129": 1, "A-dm0-w10-n8-d256": 2}      # name -> seed of the three tables (default 0): the first at which the reference flags <= 2 units (and, in A at window 1, takes the skip)


def tables(spec, V, n_docs, table_seed):
    """wv, dv, syn1neg ~ N(0, 0.1^2).  Window 1 of case A: |f| >= 6 cannot happen between such tables, so document 0's vector and the syn1neg row of its rarest word
    are set to 4.5 * (one +-1 / sqrt(d) vector) - no entry larger than the normal ones' largest at d >= 128 - and f is 20.25 / (context + 1) >= 6.75 there"""
    d = spec["d"]
    rng = np.random.default_rng(table_seed)
    wv, dv, s1 = ((rng.standard_normal((r, d)) * 0.1).astype(np.float32) for r in (V, n_docs, V))
    if spec["corpus"][0] == "A" and spec["window"] == 1:
        ptr, wi = corpus(*spec["corpus"])[:2]
        u = (4.5 / np.sqrt(d) * np.where(rng.random(d) < 0.5, -1.0, 1.0)).astype(np.float32)
        dv[0] = u; s1[int(wi[ptr[0]:ptr[1]].max())] = u
    return wv, dv, s1


@functools.lru_cache(maxsize=None)
def train_case(name, variant=None, table_seed=None):
    """inputs, the reference's three tables after the pass and what it counted; shared, read-only"""
    spec = TRAIN_SPECS[name]
    ptr, wi, si, cum = corpus(*spec["corpus"])
    wv, dv, s1 = tables(spec, len(si), len(ptr) - 1, TABLE_SEED.get(name, 0) if table_seed is None else table_seed)
    c = dict(spec, name=name, ptr=ptr, wi=wi, si=si, cum=cum, wv0=wv, dv0=dv, s10=s1, seed=spec.get("seed", SEED))
    c["dv"], c["wv"], c["s1"] = dv.copy(), wv.copy(), s1.copy()
    c["stats"] = reference_train(ptr, wi, si, cum, c["wv"], c["dv"], c["s1"], spec["dm"], spec["window"], spec["negative"], ALPHA0, ALPHA1, c["seed"], 0, variant=variant)
    for a in c.values():
        if isinstance(a, np.ndarray): a.setflags(write=False)
    return c


def train_bars(c):
    """per table (dv, wv, syn1neg): BAR * max|ref| + 1e-9 + flagged * step, step = one bin of the sigmoid table (0.003, doubled) * alpha * the largest entry it multiplies"""
    step = 2 * 0.003 * ALPHA0 * max(float(np.abs(c[t]).max()) for t in ("dv", "wv", "s1"))
    return [BAR * float(np.abs(c[t]).max()) + 1e-9 + c["stats"]["flagged"] * step for t in ("dv", "wv", "s1")]


def distance(c, other):
    """max|other - ref| / bar of the three tables; other = a case dict or the three tables"""
    o = [other[t] for t in ("dv", "wv", "s1")] if isinstance(other, dict) else other
    return [float(np.abs(np.asarray(g, np.float64) - c[t]).max()) / b for g, t, b in zip(o, ("dv", "wv", "s1"), train_bars(c))]


# ------------------------------------------------------------------------------------------------ inference cases, built like tests/test_gpu_d2v_infer.py case1
I_ALPHA, I_MIN_ALPHA, I_SEED = 0.025, 0.001, 11
SIGMA = {64: 0.8, 129: 0.7, 192: 0.65, 256: 0.6}
I_SEED_LONG = 17                   # seed_with_a_full_window(600, 255, doc=1000, first=11); asserted in test_d2v_paths_host.py


def _infer_specs():
    s = {}
    for dm in (1, 0):
        for w, ng in ((1, 0), (2, 4), (10, 8)):
            for d in (64, 129, 192, 256): s[f"dm{dm}-w{w}-n{ng}-d{d}"] = dict(vocab="zipf60", dm=dm, window=w, negative=ng, d=d)
        for table in ("arange", "plateaus"): s[f"dm{dm}-V2500-{table}"] = dict(vocab=table, dm=dm, window=3, negative=8, d=64)
    s["long-w255"] = dict(vocab="zipf60", dm=1, window=255, negative=1, d=64, long=True, seed=I_SEED_LONG)
    return s


INFER_SPECS = _infer_specs()


@functools.lru_cache(maxsize=None)
def infer_case(name):
    spec = INFER_SPECS[name]
    d, dm = spec["d"], spec["dm"]
    if spec["vocab"] == "zipf60": si, cum = _vocab60()
    else: si, cum = np.full(2500, 0xFFFFFFFF, np.uint32), search_tables(2500)[spec["vocab"]]
    V = len(si)
    rng = np.random.default_rng(1000 * d + 10 * spec["window"] + dm)
    sigma = 0.02 if spec.get("long") else SIGMA[d]                       # (the long query: test_gpu_d2v_infer.py case_long's tables)
    wv = (rng.standard_normal((V, d)) * sigma).astype(np.float32)
    s1 = (rng.standard_normal((V, d)) * sigma).astype(np.float32)
    if spec.get("long"): lens, epochs = np.asarray([600, 40, 40, 40]), 1       # query 0 (id 1000): 600 kept words, sample_int all ones below
    else:
        lens, epochs = 1 + rng.poisson(4, 48), 2
        lens[0] = 0; lens[1] = 1
    n = len(lens)
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    q_words = _query_words(rng, int(q_ptr[-1])) if V == 60 else rng.integers(0, V, int(q_ptr[-1])).astype(np.int32)
    if spec.get("long"): si = np.full(V, 0xFFFFFFFF, np.uint32)
    ids = 1000 + np.arange(n, dtype=np.int64)
    init = ((rng.random((n, d), dtype=np.float32) * 2 - 1) / d).astype(np.float32) if dm else (rng.standard_normal((n, d)) * 0.35).astype(np.float32)
    c = dict(name=name, d=d, dm=dm, si=si, cum=cum, wv=wv, s1=s1, q_ptr=q_ptr, q_words=q_words, ids=ids, init=init, window=spec["window"], negative=spec["negative"],
             epochs=epochs, seed=spec.get("seed", I_SEED))
    c["ref"], c["flagged"], c["units"], c["skipped"] = reference_infer(q_ptr, q_words, ids, init, wv, s1, si, cum, dm, spec["window"], spec["negative"], epochs,
                                                                       I_ALPHA, I_MIN_ALPHA, c["seed"])
    for a in c.values():
        if isinstance(a, np.ndarray): a.setflags(write=False)
    return c
