"""What the doc2vec kernels (opentf_amd/csrc/ntf_d2v.hip k_d2v_epoch, k_d2v_infer) compute on the suites' small cases, as one SHA-256 per case over the raw bytes:
a trainer case hashes dv, wv, syn1neg and the mean loss (f64) of a one-wave (`serial`) pass, an inference case the inferred vectors.  Two libraries of the same
ABI compute the same thing exactly when every line agrees (the suites' tolerances would let a reordered sum through):

    NTF_LIB_PATH=<the other build>/libopentf_amd.so python profiles/d2v_bits.py > a.txt;  python profiles/d2v_bits.py > b.txt;  cmp a.txt b.txt

One process per library.  Cases: every TRAIN_SPECS case of tests/d2v_reference.py (B-d128 / 192 / 256 under both arms of NTF_D2V_DEFER), every INFER_SPECS case in
the default parallel launch (inference does not depend on the schedule), and the d x dm cases of tests/test_gpu_d2v.py and tests/test_gpu_d2v_infer.py.  Only the
cases' INPUTS are built: the host references the suites compare against are not run (profiles/d2v_refactor_check.md has the last comparison)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import d2v_reference as R                               # noqa: E402
R.reference_infer = lambda *a, **k: (None, None, 0, 0)  # infer_case / case1 build the inputs and then call it: the inputs are all this script needs
import test_gpu_d2v as T                                # noqa: E402
import test_gpu_d2v_infer as TI                         # noqa: E402
from oracle import d2v_oracle as D                      # noqa: E402
from opentf_amd import libntf                           # noqa: E402
from opentf_amd.mdl.emb import d2v as P                 # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays: h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def tables_of(net, loss):
    return digest(*(net.vectors(w) for w in (net.DV, net.WV, net.SYN1NEG)), np.float64(loss))


def train_spec(name):
    spec = R.TRAIN_SPECS[name]
    ptr, wi, si, cum = R.corpus(*spec["corpus"])
    wv, dv, s1 = R.tables(spec, len(si), len(ptr) - 1, R.TABLE_SEED.get(name, 0))
    net = libntf.Doc2Vec(ptr, wi, si, cum, wv, dv, seed=spec.get("seed", R.SEED))
    net.set_vectors(net.SYN1NEG, s1)
    loss, _ = net.train_epoch(spec["dm"], spec["window"], R.ALPHA0, R.ALPHA1, 0, negative=spec["negative"], serial=True, want_loss=True)
    out = tables_of(net, loss)
    net.close()
    return out


def train_suite(case, d, dm):
    """tests/test_gpu_d2v.py test_one_wave_pass_equals_the_sequential_oracle's device side: two serial passes at window 5, negative 5"""
    ptr, words, sample = T.CASES[case]()
    keys, count, si, cum, wi = P.build_vocab(words, sample=sample)
    wv, dv, s1 = D.init_vectors(len(ptr) - 1, len(keys), d, 3)
    order = np.random.default_rng(1).permutation(len(ptr) - 1) if case == "zipf" else None
    progress = D.job_progress(ptr, order, batch_words=100) if case == "zipf" else None
    net = libntf.Doc2Vec(ptr, wi, si, cum, wv, dv, seed=3)
    for ep, (a0, a1) in enumerate(D.alpha_schedule(2, 0.001, spe=1)[0]):
        loss, _ = net.train_epoch(dm, 5, a0, a1, ep, serial=True, order=order, progress=progress, want_loss=True)
    out = tables_of(net, loss)
    net.close()
    return out


def suite_runs(case, d, dm):
    """the cases that test does not skip"""
    if case.startswith("toy") or case == "long_docs": return d == 128
    if case == "capped_doc": return d == 64 and dm == 1
    return True


def infer(c, alpha, min_alpha, seed):
    net = TI._net(c)
    got = net.infer(c["q_ptr"], c["q_words"], c["init"], c["dm"], c["window"], c["epochs"], alpha, min_alpha, seed, negative=c["negative"], ids=c["ids"])
    net.close()
    return digest(got)


def main():
    os.environ.pop("NTF_D2V_DEFER", None)
    for name in R.TRAIN_SPECS:
        if name.startswith("B-"):
            print(f"train {name} deferred {train_spec(name)}", flush=True)
            os.environ["NTF_D2V_DEFER"] = "0"              # read per call
            print(f"train {name} plain {train_spec(name)}", flush=True)
            del os.environ["NTF_D2V_DEFER"]
        else: print(f"train {name} {train_spec(name)}", flush=True)
    for case in T.CASES:
        for d in (9, 64, 100, 128, 256):
            for dm in (1, 0):
                if suite_runs(case, d, dm): print(f"train suite-{case}-d{d}-dm{dm} {train_suite(case, d, dm)}", flush=True)
    for name in R.INFER_SPECS:
        c = R.infer_case(name)
        print(f"infer {name} {infer(c, R.I_ALPHA, R.I_MIN_ALPHA, c['seed'])}", flush=True)
    for d in (9, 64, 100, 128, 256):
        for dm in (1, 0): print(f"infer suite-d{d}-dm{dm} {infer(TI.case1(d, dm), TI.ALPHA, TI.MIN_ALPHA, TI.SEED)}", flush=True)


if __name__ == "__main__":
    main()
