"""CPU: the A* field oracle (tests/astar_oracle.py) -- its two solvers agree, and over its field the reference's forward()
outcomes are met on every fixture map of tests/golden/astar.npz (made by the unmodified reference, make_golden_astar.py)."""
import os

import numpy as np
import pytest

import astar_oracle as A

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = A.load_fixtures(os.path.join(HERE, "golden", "astar.npz"))


def _goal(fx):
    return A.pos_to_index(fx["goal_pos"], fx["x0"], fx["y0"], fx["res"])


@pytest.mark.parametrize("name", ["instance", "flat", "maze", "unreachable", "origin_res03", "err_start", "err_goal_coll"])
def test_dijkstra_equals_vectorised_relaxation(name):
    fx = FIX[name]
    args = (fx["heights"], fx["risk"], fx["thr"], fx["res"], _goal(fx))
    D1, D2 = A.field_dijkstra(*args), A.field_relax(*args)
    assert np.array_equal(D1, D2)


@pytest.mark.parametrize("name", sorted(FIX))
def test_oracle_meets_reference_fixtures(name):
    fx = FIX[name]
    Dn = A.solve(fx["heights"], fx["risk"], fx["thr"], fx["res"], _goal(fx))
    got = [A.forward_like(fx, Dn, s) for s in fx["starts"]]
    identical, tied, cheaper, fails = A.census(fx, got)
    print(f"{name}: {identical} identical, {tied} equal-cost, {cheaper} cheaper than the reference's path")
    assert not fails, fails


def test_fixture_covers_the_issue_cases():
    st = {n: fx["status"] for n, fx in FIX.items()}
    assert (st["unreachable"] == 1).any()
    msgs = {str(m) for fx in FIX.values() for m in fx["messages"] if m}
    assert msgs == {"Start or goal position is out of bounds.", "Goal position is not traversable."}
    assert FIX["rect200x300"]["heights"].shape == (200, 300) and FIX["smooth512"]["heights"].shape == (512, 512)
    assert FIX["origin_res03"]["res"] == 0.3 and FIX["origin_res03"]["x0"] != 0.0
    for n in ("smooth256", "maze"):                       # a start just left of x_limits[0] maps to column 0
        fx = FIX[n]
        assert any(s[0] < fx["x0"] and A.pos_to_index(s, fx["x0"], fx["y0"], fx["res"])[0] == 0 for s in fx["starts"])
    assert max(len(p) for p in FIX["maze"]["paths"]) > 1000  # long hop counts


def test_threshold_reading_collision_is_risk_at_or_below():
    """risk <= threshold is a collision (astar.py:182-192): equality blocks, NaN does not."""
    risk = np.full((8, 16), 0.9, np.float32)
    risk[:, 8] = np.float32(0.25)
    risk[7, 8] = np.nan
    D, nxt = A.solve(np.zeros_like(risk), risk, 0.25, 0.5, (13, 0))
    p = A.walk(nxt, (2, 0))
    assert [n for n in p if n[0] == 8] == [(8, 7)]
    assert np.isinf(D[:6, 8]).all()
