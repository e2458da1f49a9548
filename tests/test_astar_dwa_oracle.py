"""CPU: the rules of the A* + DWA closed loop (tests/astar_dwa_oracle.py, stated from the reference) that the device loop
(csrc/astar_dwa.hip, tests/test_gpu_astar_dwa.py) follows: truncation of the start cell, the edge start, None with and without a
previous path, and a short free-running episode."""
import numpy as np
import pytest

import astar_dwa_oracle as L
import astar_maps as M

G, RES, THR, T = 64, 0.5, 0.2, 50


def _risk(seed=1):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:G, 0:G]
    return (0.5 + 0.3 * np.sin(xx / 7.0 + seed) * np.cos(yy / 9.0) + 0.05 * rng.random((G, G))).astype(np.float32)


def _loop(risk, goal=(26.0, 25.0)):
    mu = np.full((G, G), 0.25, np.float32)
    sg = np.full((G, G), 0.05, np.float32)
    return L.Loop(M.smooth_heights(G, G, 5), risk, THR, RES, goal, T, mu, sg)


def test_start_cell_truncates_not_floors():
    assert L.start_cell((-0.2, 3.0), 0.0, 0.0, RES) == (0, 6)                 # floor would give -1: out of bounds
    assert L.start_cell((-0.5, 3.0), 0.0, 0.0, RES) == (-1, 6)
    assert L.start_cell((31.99, 0.0), 0.0, 0.0, RES) == (63, 0)
    assert L.start_cell((G * RES, 0.0), 0.0, 0.0, RES) == (G, 0)             # the environment clamps x to x_limits[1]: cell G


def test_edge_start_stops_the_episode():
    lp = _loop(_risk())
    assert lp.step(0, np.float32([G * RES, 10.0, 0.0]), 0.0) is None
    assert (lp.status, lp.status_step) == (L.OUT_OF_BOUNDS, 0)
    lp = _loop(_risk())
    assert lp.step(0, np.float32([-0.4, 10.0, 0.0]), 0.0) is not None          # truncates to cell 0: in bounds
    assert lp.status == L.OK


def test_goal_out_of_bounds_or_in_collision():
    lp = _loop(_risk(), goal=(G * RES + 0.1, 5.0))
    assert lp.step(0, np.float32([5.0, 5.0, 0.0]), 0.0) is None and lp.status == L.OUT_OF_BOUNDS
    risk = _risk()
    risk[50, 50] = 0.1
    lp = _loop(risk, goal=(25.25, 25.25))
    assert lp.step(0, np.float32([5.0, 5.0, 0.0]), 0.0) is None and lp.status == L.GOAL_COLLISION


def test_none_without_a_previous_path_targets_the_goal():
    risk = _risk()
    risk[8:15, 8:15] = 0.05                                                     # a low-risk patch: collisions for A*
    lp = _loop(risk)
    state = np.float32([5.75, 5.75, 0.3])                                       # cell (11, 11): all 8 neighbours in the patch
    status, path = lp.astar(state)
    assert status == L.OK and path is None
    ns, rw, term, sg, a = lp.step(0, state, 0.1)
    assert np.array_equal(sg, np.float32([26.0, 25.0])) and lp.path is None


def test_none_with_a_previous_path_keeps_it():
    risk = _risk()
    risk[8:15, 8:15] = 0.05
    lp = _loop(risk)
    outside = np.float32([3.0, 3.0, 0.6])
    lp.step(0, outside, 0.0)
    kept = lp.path.copy()
    assert np.array_equal(kept[0], L.path_points([L.start_cell(outside, 0, 0, RES)], RES)[0])   # the start cell is on the path
    ns, rw, term, sg, a = lp.step(1, np.float32([5.75, 5.75, 0.6]), 0.0)
    assert lp.path is not None and np.array_equal(lp.path, kept)
    assert np.any(np.all(kept == sg, axis=1))                                   # the sub-goal was picked on the kept path


def test_window_matches_the_reference_formula():
    w = L.window(np.float32([0.3, -0.2]), (0.5, 0.5), 0.1, 10, 10)
    assert w.shape == (100, 2) and w.dtype == np.float32
    f = np.float32
    assert w[0, 0] == f(0.3) - f(0.5) * f(0.1) and w[-1, 0] == f(0.3) + f(0.5) * f(0.1)
    assert w[0, 1] == f(-0.2) - f(0.5) * f(0.1) and w[-1, 1] == f(-0.2) + f(0.5) * f(0.1)
    assert np.all(w[:10, 0] == w[0, 0])                                         # v major


def test_free_running_episode_is_deterministic_and_on_the_path():
    risk = _risk(3)
    runs = []
    for _ in range(2):
        lp = _loop(risk)
        st = np.float32([4.0, 5.0, 0.7])
        rows = []
        rng = np.random.default_rng(0)
        for j in range(40):
            out = lp.step(j, st, np.float32(rng.standard_normal()))
            assert out is not None
            st, rw, term, sg, a = out
            assert np.any(np.all(lp.path == sg, axis=1)) or np.array_equal(sg, lp.goal_pos)
            rows.append(np.concatenate([st, [rw], sg, a]))
        runs.append(np.stack(rows))
    assert np.array_equal(runs[0], runs[1])
    assert np.linalg.norm(runs[0][-1, :2] - np.float32([4.0, 5.0])) > 1.0       # it moved toward the goal


# ---- the reference fixture (tests/golden/make_golden_astar_dwa.py): the reference's own loop, teacher-forced step by step ----
import os  # noqa: E402

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "astar_dwa_loop.npz")
MARGIN = 1e-5      # argmin compared exactly where the reference's best cost is this clear of the next distinct one (relative)


def _fx():
    with np.load(FIX) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["smooth", "patch", "inside", "edge"])
def test_oracle_loop_replays_the_reference_fixture(name):
    fx = _fx()
    lp = L.fixture_loop(fx, name)
    n = len(fx[f"{name}__z"])
    exact = 0
    for j in range(n):
        st = fx[f"{name}__state"][j]
        assert L.start_cell(st, 0.0, 0.0, lp.res) == tuple(fx[f"{name}__cell"][j])
        status, path = lp.astar(st)
        assert status == L.OK
        assert (path is None and fx[f"{name}__path_len"][j] == -1) or (path is not None and len(path) == fx[f"{name}__path_len"][j])
        out = lp.step(j, st, float(fx[f"{name}__z"][j]), teacher=(fx[f"{name}__prev"][j], L.root_path(lp, fx[f"{name}__root"][j] if
                                                                                                     fx[f"{name}__path_len"][j] < 0 else (-1, -1))))
        ns, rw, term, sg, a = out
        assert np.array_equal(sg, fx[f"{name}__sub_goal"][j]), (name, j)
        if fx[f"{name}__margin"][j] >= MARGIN:
            # the same candidate: torch.linspace's vectorised head may differ from the scalar form in the last bit (dwa_device.h)
            w = L.window(fx[f"{name}__prev"][j], lp.a_lim, lp.dwa_dt, lp.nv, lp.nw, lp.u_min, lp.u_max)
            ref = fx[f"{name}__action"][j]
            assert int(np.argmin(np.abs(w - a).sum(1))) == int(np.argmin(np.abs(w - ref).sum(1))), (name, j)
            assert np.abs(a - ref).max() <= 1e-6, (name, j)
            assert np.abs(ns - fx[f"{name}__next_state"][j]).max() <= 1e-4, (name, j)
            exact += 1
        assert term == bool(fx[f"{name}__terminated"][j])
    assert exact >= 0.8 * n
    rs = int(fx[f"{name}__raise_step"])
    if rs >= 0:                                      # AStar.forward raised from the last stored next state: the same step here
        assert rs == n
        assert lp.step(rs, fx[f"{name}__next_state"][n - 1], 0.0) is None
        assert (lp.status, lp.status_step) == (L.OUT_OF_BOUNDS, rs) and str(fx[f"{name}__message"]) == "Start or goal position is out of bounds."


def test_fixture_covers_the_rules():
    fx = _fx()
    assert (fx["patch__path_len"] < 0).sum() > 0 and (fx["patch__root"][fx["patch__path_len"] < 0] >= 0).all()   # None keeps a path
    assert (fx["inside__root"][:, 0] < 0).sum() > 0                                                            # None before any path
    assert int(fx["edge__raise_step"]) > 0 and int(fx["smooth__raise_step"]) == -1
    assert os.path.getsize(FIX) < 1 << 20
