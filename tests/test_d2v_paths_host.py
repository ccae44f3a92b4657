"""The host side of tests/test_gpu_d2v_paths.py (doc2vec kernels off window 5, negative 5 and small vocabularies): tests/d2v_reference.py's trainer against
oracle/d2v_oracle.py, every condition a case has to meet BEFORE a device sees it - taken from the reference alone - and how far four wrong kernels would land from
the reference on the cases meant to catch them.  No GPU."""
import numpy as np
import pytest

import d2v_reference as R
from oracle import d2v_oracle as D

TABLES = (("dv", "dv0"), ("wv", "wv0"), ("s1", "s10"))


@pytest.mark.parametrize("name", ["A-dm1-w2-n4-d128", "A-dm0-w10-n8-d64"])
def test_reference_train_is_the_oracles_pass_bit_for_bit(name):
    c = R.train_case(name)
    wv, dv, s1 = c["wv0"].copy(), c["dv0"].copy(), c["s10"].copy()
    loss = D.train_epoch(c["ptr"], c["wi"], {"sample_int": c["si"], "cum_table": c["cum"]}, wv, dv, s1, c["dm"], c["window"], R.ALPHA0, R.ALPHA1, c["seed"], 0,
                         negative=c["negative"], return_loss=True)
    assert np.array_equal(dv, c["dv"]) and np.array_equal(wv, c["wv"]) and np.array_equal(s1, c["s1"]) and loss == c["stats"]["loss"]
    assert not np.array_equal(s1, c["s10"])


@pytest.mark.parametrize("name", list(R.TRAIN_SPECS))
def test_every_trainer_case_meets_its_conditions(name):
    c = R.train_case(name)
    st, bars = c["stats"], R.train_bars(c)
    moved = [float(np.abs(c[a].astype(np.float64) - c[b]).max()) / bar for (a, b), bar in zip(TABLES, bars)]
    print(f"\n{name}: {st}, bars {[f'{b:.2e}' for b in bars]}, moved by {[round(m) for m in moved]} bars")
    assert st["flagged"] <= 2, st                                          # the allowance for another bin of the sigmoid table stays at two steps
    assert st["kept"] <= 4800, st                                          # the bar is tests/test_gpu_d2v.py's for that many kept positions
    assert min(moved) >= 100, moved                                        # a kernel that left a table alone would be 100 bars away
    assert c["negative"] == 0 or st["self_draws"] >= 1, st                 # a negative draw equal to the predicted word takes the `continue`
    assert all(np.isfinite(c[t]).all() for t, _ in TABLES)


@pytest.mark.parametrize("dm", [1, 0])
def test_case_a_takes_the_skip_of_large_f(dm):
    assert sum(R.train_case(n)["stats"]["skipped"] for n, s in R.TRAIN_SPECS.items() if n.startswith("A-") and s["dm"] == dm) >= 1


@pytest.mark.parametrize("p", [3, 5, 8, 9, 10, 11])
def test_deferral_without_the_duplicate_flush_shows_up_to_a_period_of_ten(p):
    """the reach of the rule: two kept positions within 2 * 5 of each other.  A tail of period 10 needs the flush, one of period 11 does not"""
    c = R.train_case(f"C-P{p}")
    dist = R.distance(c, R.train_case(f"C-P{p}", "no_flush"))
    print(f"\nperiod {p}: deferral without the flush is {[f'{x:.2f}' for x in dist]} bars (dv, wv, syn1neg) from the reference")
    if p <= 10: assert max(dist) >= 10, dist
    else: assert max(dist) <= 1, dist


@pytest.mark.parametrize("variant", ["top_le", "neg1_lost"])
@pytest.mark.parametrize("name", [n for n in R.TRAIN_SPECS if n.startswith("D-")])
def test_a_wrong_table_search_or_a_lost_philox_word_shows_on_case_d(name, variant):
    c = R.train_case(name)
    dist = R.distance(c, R.train_case(name, variant))
    print(f"\n{name}, {variant}: {[f'{x:.0f}' for x in dist]} bars from the reference")
    assert max(dist) >= 10, dist


@pytest.mark.parametrize("name", ["A-dm1-w2-n4-d128", "A-dm1-w10-n8-d128", "A-dm0-w10-n8-d64"])
def test_a_window_fixed_at_five_shows_on_case_a(name):
    c = R.train_case(name)
    dist = R.distance(c, R.train_case(name, "window5"))
    print(f"\n{name}, b = draw % 5: {[f'{x:.0f}' for x in dist]} bars from the reference")
    assert max(dist) >= 10, dist


def test_the_limits_of_the_window_are_reached():
    """seeds from the SLOT_WINDOW draws alone: a position with `window` kept words on both sides that draws b = 0"""
    assert R.E_SEED == {1: R.seed_with_a_full_window(600, 255), 0: R.seed_with_a_full_window(300, 127)}
    assert R.I_SEED_LONG == R.seed_with_a_full_window(600, 255, doc=1000, first=R.I_SEED)
    e1, e0 = R.train_case("E-dm1")["stats"], R.train_case("E-dm0")["stats"]
    assert e1["max_ctx"] == 2 * 255 and e1["kept"] == 640
    assert e0["max_ctx"] == 2 * 127 and e0["max_unit"] == 254 and e0["kept"] == 300        # 254: the largest unit index 8 bits of the Philox counter hold beside unit 0


@pytest.mark.parametrize("name", list(R.INFER_SPECS))
def test_every_inference_case_meets_its_conditions(name):
    c = R.infer_case(name)
    n, fragile = len(c["ref"]), int((c["flagged"] > 0).sum())
    print(f"\n{name}: {c['units']} units, {c['skipped']} skipped for |f| >= 6, {fragile} of {n} queries fragile")
    assert fragile <= n // 4, fragile                                      # tests/test_gpu_d2v_infer.py's rule: at most 25 % of the queries may sit on an edge
    first = 0 if n == 4 else 2                                             # (the 48-query cases: query 0 is empty)
    moved = np.abs(c["ref"][first:].astype(np.float64) - c["init"][first:]).max(axis=1)
    far = moved >= 100 * (2e-5 * np.abs(c["ref"][first:]).max(axis=1) + 1e-9)      # (a short query may lose every word to the subsampling and stay where it was)
    assert far.mean() >= 0.75 and far[0], far
    assert n == 4 or np.array_equal(c["ref"][0], c["init"][0])
