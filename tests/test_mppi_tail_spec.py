"""CPU: the float64 restatement of a solve's tail (tests/mppi_tail_spec.py), its cases (tests/mppi_tail_cases.py) and the checker of
tests/test_gpu_mppi_tail.py, without a GPU.

  * the float32 CPU oracle's w and U* lie within the derived bound of the spec on every case: the bound is not tighter than the reference;
  * oracle.rollout(U*) is the oracle's X* bit for bit on every case;
  * every case keeps what it promises (one-hot: exactly one-hot on the oracle; ladder: half the levels above 1e-6, no row without weight);
  * the checker passes the oracle's own outputs and rejects each of seven corruptions of them, on the smallest case where the corruption
    can occur at all (in the spirit of FUZZ_BREAK);
  * tests/golden/mppi_tail.json is what tests/golden/make_golden_mppi_tail.py records, and every recorded yardstick is below 1."""
import importlib.util
import json
import os

import numpy as np
import pytest

import mppi_tail_cases as TC
from mppi_tail_spec import n_sum, ratios, tail
from test_gpu_mppi_tail import check_tail


def _one_hot_cases():
    for T in TC.HORIZONS:
        yield from TC.sweep_cases(2, T=T)
    for rows in (2, 65):
        yield from TC.sweep_cases(rows, lam=TC.LAMBDAS[1])
    for B, K in ((3, 130), (9, 130), (3, 4160), (9, 5121)):
        yield TC.batch(B, K, TC.BASE_T)


def _check_case(case):
    from oracle import oracle as O
    worst = dict(w=0.0, U=0.0, sum=0.0)
    for ref in (False, True):
        for b, inst in enumerate(case["inst"]):
            orc = TC.reference(case, b, ref)
            TC.conditions(case, b, orc)
            r = ratios(orc["w"], orc["Ustar"], tail(orc["cost"], orc["U"], case["lam"]))
            assert max(r.values()) <= 1.0, (case["name"], b, ref, r)
            assert np.array_equal(O.rollout(TC.oracle_params(case, b, ref), inst["R"], inst["state"], orc["Ustar"]), orc["Xstar"]), (case["name"], b, ref)
            check_tail(orc, case, b, ref)
            worst = {k: max(worst[k], r[k]) for k in worst}
    return worst


@pytest.mark.parametrize("rows", TC.ROWS)
def test_one_hot_cases_hold_on_the_oracle_at_every_row_count(rows):
    for case in TC.sweep_cases(rows):
        _check_case(case)


def test_one_hot_cases_hold_on_the_oracle_at_every_horizon_lambda_and_in_batches():
    seen = set()
    for case in _one_hot_cases():
        _check_case(case)
        seen.add((case["T"], case["lam"], len(case["inst"])))
    assert {T for T, _, _ in seen} >= set(TC.HORIZONS) and {l for _, l, _ in seen} == set(TC.LAMBDAS) and {B for _, _, B in seen} == {1, 3, 9}


def test_batches_give_every_instance_another_kstar_and_goal():
    for B, K in ((3, 130), (9, 130), (9, 4160)):
        case = TC.batch(B, K, TC.BASE_T)
        ks = [i["kstar"] for i in case["inst"]]
        assert ks[:3] == [0, 64, K - 1] and len(set(ks[:8])) == min(B, 8)
        assert len({tuple(i["goal"]) for i in case["inst"]}) == B
        if B == 9:
            assert set(ks) == set(TC.kstars(K))


def test_spread_cases_lie_within_the_bound_and_the_golden_records_them():
    spec = importlib.util.spec_from_file_location("make_golden_mppi_tail", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_mppi_tail.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gold = json.load(open(gen.GOLDEN))["cases"]
    cases = TC.yardstick_cases()
    assert sorted(gold) == sorted(c["name"] for c in cases)
    for case in cases:
        worst = _check_case(case)
        now, rec = gen.record(case), gold[case["name"]]
        print(f"{case['name']}: z spread {now['z_spread']:.3g}, oracle/bound w {worst['w']:.3g} U* {worst['U']:.3g} sum {worst['sum']:.3g}")
        for k in ("K", "T"):
            assert now[k] == rec[k]
        for k in ("lam", "z_spread", "w_bound_max", "Ustar_bound_max"):       # inputs and the bound: NumPy float64 arithmetic, no libm of float32
            assert now[k] == pytest.approx(rec[k], rel=1e-9), (case["name"], k)
        for k in ("oracle_w_over_bound", "oracle_Ustar_over_bound", "oracle_sum_over_bound"):
            assert 0.0 <= rec[k] < 1.0 and now[k] < 1.0, (case["name"], k, rec[k], now[k])


def test_ladder_spreads_are_the_three_asked_for():
    got = [tail(TC.reference(c)["cost"], TC.reference(c)["U"], c["lam"])["spread"] for c in (TC.ladder(K, s) for K, s in TC.LADDER)]
    assert [round(g) for g in got] == [3, 20, 80], got


def test_bound_counts_its_roundings_and_stays_far_below_the_fixed_tolerances():
    """The derived bound is what the ingredients give: a few times 1e-6 of a weight at the row counts of the suite -- where the fixed
    w_abs <= 2e-6 of test_gpu_fuzz.py lets 0.8 % of a uniform weight at K = 4160 through."""
    c = TC.ladder(4160, 3.0)
    o = TC.reference(c)
    s = tail(o["cost"], o["U"], c["lam"])
    rel = float((s["w_bound"] / s["w"]).max())
    assert n_sum(4160) == 64 + 65 + 5 + 2 and n_sum(64) == 64 + 1 + 1 + 2 and n_sum(65600) == 64 + 1025 + 65 + 2
    assert 2 ** -24 * n_sum(4160) < rel < 2e-5


# ---- the checker rejects what it is there to reject ----------------------------------------------------------------------------------
def _row_part(orc, row):
    """sum over the rollouts of one 64-rollout row of w_k U[k]: the row's contribution to U*."""
    sl = slice(64 * row, 64 * row + 64)
    return (orc["w"][sl].astype(np.float64)[:, None, None] * orc["U"][sl].astype(np.float64)).sum(0)


def _rescaled(case, orc, num=None, S_terms=None):
    """w and U* with other exponentials: `num` in place of e_k = exp(z_k - m) in the numerators, `S_terms` summed for S."""
    z = (-orc["cost"]) / np.float32(case["lam"])
    num = np.exp((z - z.max()).astype(np.float64)) if num is None else num
    S = num.sum() if S_terms is None else S_terms.sum()
    w = num / S
    return w.astype(np.float32), (w[:, None, None] * orc["U"].astype(np.float64)).sum(0).astype(np.float32)


def _with(case, orc, w=None, Ustar=None, Xstar=None, reroll=True):
    from oracle import oracle as O
    out = dict(orc)
    if w is not None:
        out["w"] = w
    if Ustar is not None:
        out["Ustar"] = Ustar.astype(np.float32)
        if reroll:                                       # a merge that is wrong is wrong before the tail rolls U* out: X* stays consistent
            i = case["inst"][0]
            out["Xstar"] = O.rollout(TC.oracle_params(case), i["R"], i["state"], out["Ustar"])
    if Xstar is not None:
        out["Xstar"] = Xstar
    return out


def _corruptions():
    # two rows, every row carries weight: a dropped or doubled row is the smallest error of its kind
    lad = TC.ladder(128, 80.0)
    o = TC.reference(lad)
    yield "one row's contribution dropped from U*", lad, _with(lad, o, Ustar=o["Ustar"].astype(np.float64) - _row_part(o, 1))
    yield "one row counted twice", lad, _with(lad, o, Ustar=o["Ustar"].astype(np.float64) + _row_part(o, 0))
    # a ragged last row (K = 65: one rollout and 63 padded lanes), the weight in it
    rag = TC.one_hot(65, TC.BASE_T, 64)
    o = TC.reference(rag)
    z = (-o["cost"]) / np.float32(rag["lam"])
    pad = 63 * np.exp(np.float64(0.0))                   # 63 lanes with exp(0) against the row's own maximum, which is the global one here
    w = (o["w"].astype(np.float64) / (1 + pad)).astype(np.float32)
    yield "padded lanes of a ragged row counted with weight exp(0)", rag, _with(rag, o, w=w, Ustar=o["Ustar"].astype(np.float64) / (1 + pad))
    # two levels need more than 64 rows; the groups' maxima differ only where the weight sits in one group
    two = TC.one_hot(4160, TC.BASE_T, 0)
    o = TC.reference(two)
    z = (-o["cost"]) / np.float32(two["lam"])
    group = np.arange(4160) // (64 * 16)
    gmax = np.array([z[group == g].max() for g in range(group.max() + 1)])
    w, us = _rescaled(two, o, num=np.exp((z - gmax[group]).astype(np.float64)))
    yield "scales taken against the group's maximum instead of the global one", two, _with(two, o, w=w, Ustar=us)
    # S not rescaled: the rows' sums added as they are, each relative to its own maximum (two rows are enough)
    one = TC.one_hot(128, TC.BASE_T, 0)
    o = TC.reference(one)
    z = (-o["cost"]) / np.float32(one["lam"])
    rmax = np.array([z[:64].max(), z[64:].max()])[np.arange(128) // 64]
    w, us = _rescaled(one, o, S_terms=np.exp((z - rmax).astype(np.float64)))
    yield "S not rescaled", one, _with(one, o, w=w, Ustar=us)
    sw = o["Ustar"].copy()
    sw[[2, 3], 1] = sw[[3, 2], 1]
    assert not np.array_equal(sw, o["Ustar"])
    yield "two columns of U* swapped", one, _with(one, o, Ustar=sw)
    early = o["Xstar"].copy()
    early[-1] = o["Xstar"][-3]                           # slot T - 2 holds the un-clamped state after T - 1 steps (the aliased slots): one step early
    assert not np.array_equal(early, o["Xstar"])
    yield "the last state of X* taken one step early", one, _with(one, o, Xstar=early)


_CORRUPTIONS = ("one row's contribution dropped from U*", "one row counted twice", "padded lanes of a ragged row counted with weight exp(0)",
                "scales taken against the group's maximum instead of the global one", "S not rescaled", "two columns of U* swapped",
                "the last state of X* taken one step early")


@pytest.mark.parametrize("what", _CORRUPTIONS)
def test_checker_rejects(what):
    found = {name: (case, bad) for name, case, bad in _corruptions()}
    assert sorted(found) == sorted(_CORRUPTIONS)
    case, bad = found[what]
    check_tail(TC.reference(case), case)                 # the uncorrupted outputs pass
    with pytest.raises(AssertionError):
        check_tail(bad, case)
