"""CPU: the NumPy statement of the CL-RRT plan-follow-replan loop (tests/clrrt_loop_spec.py) against the reference's recorded
episodes (tests/golden/clrrt_loop.npz: the unmodified CLRRT and the real PlanetaryEnv, test/test_cl_rrt.py:167-200).  The spec is
fed the recorded plans and slip draws and runs each episode FREE (its own states feed the next iteration), so every replan
decision is its own.

Equal: every event, every replan iteration, the plan index of every iteration, the outcome and its iteration, the actions.
Within tolerance: states and deviations.  tests/test_gpu_env.py holds one teacher-forced step to 1e-6 against the reference
(sin / cos of SLEEF against the spec's); a free segment of n steps between two plans accumulates at most n of them, and a plan
resets nothing of the state, so the bound asserted at iteration t is 1e-6 * (steps taken so far).  Measured here: 0 in the state
and 0 in the deviation on all three episodes (the oracle's step and the fused norm reproduce the capture's torch build bit for
bit) -- inside the bound, and inside half the fixture's smallest |dev - 1| (1.69e-3), which is what keeps a replan decision from
flipping."""
import os

import numpy as np
import pytest

import clrrt_loop_spec as L

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clrrt_loop.npz")
STEP_TOL = 1e-6


@pytest.fixture(scope="module")
def fx():
    return np.load(FX)


@pytest.fixture(scope="module")
def runs(fx):
    out = {}
    n = int(fx["params"][3])
    for name in fx["episodes"].tolist():
        p, MU, SG, plans = L.fixture_episode(fx, name)
        rover = L.Rover(p, MU, SG, float(fx["goal_threshold"]), fx[f"{name}__state"][0], lambda k, s, plans=plans: plans[k],
                        delta_t=float(fx["delta_t"]), time_limit=float(fx["time_limit"]))
        out[name] = (rover.run(n, fx[f"{name}__z"]), rover)
    return out


def test_fixture_holds_the_three_kinds_of_episode(fx):
    assert fx["status_names"].tolist()[L.NO_PLAN] == "NO_PLAN" and fx["event_names"].tolist() == ["STEP", "REPLAN", "FROZEN"]
    assert int(fx["s10__status"]) == L.GOAL and int(fx["s10__n_plans"]) == 1
    assert int((fx["s14__event"] == L.REPLAN).sum()) >= 3
    assert int(fx["s04__status"]) == L.NO_PLAN
    for name in fx["episodes"].tolist():
        d = fx[f"{name}__dev"]
        assert np.abs(d[np.isfinite(d)] - 1).min() >= 1e-3


@pytest.mark.parametrize("name", ["s10", "s14", "s04"])
def test_spec_reproduces_the_reference_episode(fx, runs, name):
    got, rover = runs[name]
    assert np.array_equal(got["events"], fx[f"{name}__event"].astype(np.int32))
    assert np.array_equal(got["plan_index"], fx[f"{name}__plan_idx"])
    assert np.array_equal(np.nonzero(got["events"] == L.REPLAN)[0] + 1, fx[f"{name}__plan_iter"][1:])
    assert (rover.status, rover.done_iter, rover.n_plans) == (int(fx[f"{name}__status"]), int(fx[f"{name}__done_iter"]), int(fx[f"{name}__n_plans"]))
    assert np.array_equal(got["actions"], fx[f"{name}__action"], equal_nan=True)
    assert np.array_equal(got["rewards"], fx[f"{name}__reward"], equal_nan=True)
    steps = np.cumsum(got["events"] == L.STEP)
    ds = np.abs(got["states"][1:] - fx[f"{name}__state"][1:]).max(axis=1)
    dd = np.abs(got["deviations"] - fx[f"{name}__dev"])
    assert np.array_equal(np.isnan(got["deviations"]), np.isnan(fx[f"{name}__dev"]))
    print(f"{name}: largest state difference {ds.max():.3e}, deviation difference {np.nanmax(dd):.3e}, {int(steps[-1])} steps")
    assert (ds <= STEP_TOL * np.maximum(steps, 1)).all()
    assert (dd[~np.isnan(dd)] <= STEP_TOL * np.maximum(steps, 1)[~np.isnan(dd)]).all()
    assert max(ds.max(), np.nanmax(dd)) <= 8e-4


def test_time_limit_is_the_float64_accumulation():
    assert L.limit_steps(0.1, 100.0) == 1001          # 1000 additions of 0.1 give 99.99999999999859
    assert L.limit_steps(0.1, 0.5) == 6               # 0.1 * 5 accumulates to exactly 0.5: not yet over
    assert L.limit_steps(0.1, 0.3) == 3               # 0.1 + 0.1 + 0.1 = 0.30000000000000004 > 0.3
