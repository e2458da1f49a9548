"""CPU: the rules of the A* + DWA closed loop (tests/astar_dwa_oracle.py, stated from the reference) that the device loop
(csrc/astar_dwa.hip, tests/test_gpu_astar_dwa.py) follows: truncation of the start cell, the edge start, None with and without a
previous path, and a short free-running episode; the grid limits, the bearing margin and the measured error of the host's atan2f
that set the ambiguity band DELTA; and the oracle free-running on every scenario of tests/test_gpu_astar_dwa_oracle.py."""
import numpy as np
import pytest

import astar_dwa_oracle as L
import astar_dwa_scenarios as S
import astar_maps as M
from oracle import oracle as O

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


# ---- limits, the bearing margin, the host's atan2f ---------------------------------------------------------------------------
def test_a_non_zero_origin_moves_the_cells_but_not_the_path_points():
    lim = (-8.0, 24.0)
    assert L.start_cell((-8.0, -7.6), lim[0], lim[0], RES) == (0, 0)
    assert L.start_cell((-8.4, 3.0), lim[0], lim[0], RES) == (0, 22)            # truncation, not floor, about the origin too
    assert L.start_cell((-8.5, 3.0), lim[0], lim[0], RES) == (-1, 22)
    assert L.start_cell((24.0, 0.0), lim[0], lim[0], RES) == (G, 16)            # the upper limit, where the environment clamps
    mu = np.full((G, G), 0.25, np.float32)
    mk = lambda goal: L.Loop(M.smooth_heights(G, G, 5), _risk(), THR, RES, goal, T, mu, np.full((G, G), 0.05, np.float32), x_limits=lim)
    lp = mk((10.0, 9.0))
    assert lp.goal == (36, 34) and (lp.p.x0, lp.p.y0, lp.pe.x0, lp.pe.x_hi, lp.pe.y_lo) == (-8.0, -8.0, -8.0, 24.0, -8.0)
    state = np.float32([-3.0, -2.0, 0.6])
    status, path = lp.astar(state)
    assert status == L.OK and np.array_equal(path[0], np.float32([10, 12]) * np.float32(RES))    # cell (10, 12); x_limits[0] ignored
    assert np.array_equal(path[-1], np.float32([36, 34]) * np.float32(RES))
    ns, rw, term, sg, a = lp.step(0, state, 0.0)
    assert np.any(np.all(path == sg, axis=1))
    # the edge start: x = x_limits[1] indexes to G
    lp = mk((10.0, 9.0))
    assert lp.step(0, np.float32([24.0, 3.0, 0.0]), 0.0) is None and (lp.status, lp.status_step) == (L.OUT_OF_BOUNDS, 0)
    lp = mk((10.0, 9.0))
    assert lp.step(0, np.float32([-8.4, 3.0, 0.0]), 0.0) is not None and lp.status == L.OK
    # a goal that is in bounds only about the origin, and one that is out of bounds only about it
    assert mk((-7.0, -7.0)).goal_in and not mk((25.0, 9.0)).goal_in


def test_bearing_margin_on_hand_made_paths():
    sel = np.float32([2.0, 3.0, 0.0])
    far = np.float32([[6.0, 3.0], [2.0, 7.0], [5.0, 7.0]])                      # dead ahead; exactly abeam; 53 degrees off
    assert L.bearing_margin(far[:1], sel, 1.0) == pytest.approx(np.pi / 2)
    assert L.bearing_margin(far, sel, 1.0) == 0.0                              # atan2(4, 0) - 0 is pi/2 in float64
    assert L.bearing_margin(far[[0, 2]], sel, 1.0) == pytest.approx(np.pi / 2 - np.arctan2(4.0, 3.0))
    assert L.bearing_margin(far, sel, 4.5) == pytest.approx(np.pi / 2 - np.arctan2(4.0, 3.0))    # the abeam point is within the look-ahead
    assert L.bearing_margin(far, sel, 5.0) == np.inf                           # dist == lookahead is not beyond it: no point left
    assert L.bearing_margin(np.float32([[2.0, -1.0]]), sel, 1.0) == 0.0        # abeam on the other side
    # the heading enters unwrapped, in float64 from the float32 value
    th = np.float32(0.3)
    got = L.bearing_margin(far[1:2], np.float32([2.0, 3.0, th]), 1.0)
    assert got == abs(abs(np.pi / 2 - np.float64(th)) - np.pi / 2) and got > 0.29
    assert L.bearing_margin(far[:1], np.float32([2.0, 3.0, -3.0]), 1.0) == pytest.approx(3.0 - np.pi / 2)   # |0 - (-3)| = 3: unwrapped
    # a one-ulp nudge off abeam is inside the band, a coarse one is outside
    near = np.float32([[np.nextafter(np.float32(2.0), np.float32(3.0)), 7.0]])
    assert 0.0 < L.bearing_margin(near, sel, 1.0) <= L.DELTA
    assert L.bearing_margin(np.float32([[2.001, 7.0]]), sel, 1.0) > L.DELTA


def test_loop_bearing_margin_uses_the_step_s_path_and_slot_0_state():
    risk = _risk()
    risk[8:15, 8:15] = 0.05
    lp = _loop(risk)
    state = np.float32([5.75, 5.75, 0.3])                                       # no path from here and none kept
    assert lp.bearing_margin(state) == np.inf and lp.path is None
    outside = np.float32([3.0, 3.0, 0.6])
    m = lp.bearing_margin(outside)                                              # the fresh path, although none is kept yet
    fresh = lp.astar(outside)[1]
    a0 = L.window(lp.prev, lp.a_lim, lp.dwa_dt, lp.nv, lp.nw)[0]
    sel = O.dwa_sub_goal(lp.p, lp.risk, outside, a0, fresh, lp.look)[1]
    assert lp.path is None and m == L.bearing_margin(fresh, sel, lp.look) and 0.0 < m < np.pi / 2
    lp.step(0, outside, 0.0)
    kept = lp.path.copy()
    sel = O.dwa_sub_goal(lp.p, lp.risk, state, L.window(lp.prev, lp.a_lim, lp.dwa_dt, lp.nv, lp.nw)[0], kept, lp.look)[1]
    assert lp.bearing_margin(state) == L.bearing_margin(kept, sel, lp.look)     # the kept path where the cell has none
    assert not np.array_equal(sel, state)                                       # ... seen from the slot-0 state, not the start
    assert lp.bearing_margin(np.float32([G * RES, 3.0, 0.0])) == np.inf         # AStar.forward raises: nothing is picked
    assert np.array_equal(lp.path, kept) and lp.status == L.OK                  # and asking changes nothing


def test_host_atan2f_error_is_the_recorded_one():
    """E_host of the ambiguity band: glibc's atan2f (what oracle_dwa_sub_goal calls) against float64 arctan2 of the same inputs."""
    dy, dx = L.atan2_pairs()
    e = L.atan2_ulp_error(O.atan2f(dy, dx), dy, dx)
    print(f"E_host = {e:.4f} ulp over {len(dy)} pairs")
    assert e <= L.ATAN2_E_HOST
    ax_y = np.float32([0, 0, -0.0, -0.0, 0, 0, -0.0, -0.0, 1, -1, 1, -1])
    ax_x = np.float32([0, -0.0, 0, -0.0, 1, -1, 1, -1, 0, 0, -0.0, -0.0])
    assert np.array_equal(O.atan2f(ax_y, ax_x).view(np.uint32), np.arctan2(ax_y, ax_x).view(np.uint32))
    assert L.DELTA == (max(L.ATAN2_E_DEV, L.ATAN2_E_HOST) + 1) * 2.0 ** -22


# ---- the scenarios of tests/test_gpu_astar_dwa_oracle.py, oracle alone: few steps hang on the last bits of atan2f ----------------
CAP = 0.02         # of a scenario's steps may have bearing_margin <= DELTA (and are then not compared on the device)


@pytest.mark.parametrize("name", S.SCENARIOS)
def test_free_running_scenarios_stay_under_the_cap_on_ambiguous_steps(name):
    sc = S.scenario(name)
    statuses, kept_idx = [], []
    for b in range(len(sc["starts"])):
        ran, flagged, lp, idx, kept = S.free_run(sc, b)
        print(f"{name}[{b}]: {flagged} of {ran} steps within DELTA = {L.DELTA:.3e}; status {lp.status} at {lp.status_step}")
        assert flagged <= CAP * sc["n"], (name, b, flagged)
        statuses.append(lp.status)
        kept_idx += [i for i, k in zip(idx, kept) if k and i is not None]
    # what each scenario is there for, from the oracle's side
    if name == "late_fallback":
        assert max(kept_idx) >= 64
    if name == "general33":
        assert L.OK in statuses and sc["G"] ** 2 % 4 != 0
    if name.startswith("last_byte_"):            # two rovers stand in the last cell of their slices: one has a hop there, one has none
        hop, none = (1, 2) if name == "last_byte_a" else (2, 1)
        loops = [S.oracle_loop(sc, b) for b in range(3)]
        assert sc["G"] ** 2 % 4 != 0 and loops[hop].nxt[32, 32] < 8 and loops[none].nxt[32, 32] == 255
        for b in (hop, none):
            st = S.initial_state(sc, b)
            assert L.start_cell(st, 0.0, 0.0, sc["res"]) == (32, 32) and (loops[b].astar(st)[1] is None) == (b == none)
        assert statuses == [L.OK] * 3
    if name == "big416":
        assert S.lds_bytes(sc, 0) > 160 * 1024
    if name.startswith("spiral_"):
        assert len(lp.path) > 1024
    if name in ("case_edge", "case_goal_collision"):
        assert statuses[0] != L.OK


# ---- the inputs of tests/test_gpu_dwa_subgoal.py, oracle alone -------------------------------------------------------------------
def test_sub_goal_cases_are_clear_of_the_band_and_pick_what_they_are_built_to_pick():
    import dwa_subgoal_cases as D
    for name, cfg in D.all_fixed():
        assert D.margin(cfg) > L.DELTA, name
        if "expect" in cfg:
            a0 = L.window(cfg["prev"][0], D.A_LIM, D.DWA_DT, cfg["nv"], cfg["nw"], *cfg["bounds"])[0]
            sg, sel, idx = O.dwa_sub_goal(D.params(cfg), D.risk_map(cfg["geo"][0]), cfg["states"][0], a0, cfg["path"], cfg["look"])
            assert idx == cfg["expect"], (name, idx)
            if name.startswith(("tie", "look", "none")):
                assert np.array_equal(sel[:2], cfg["states"][0, :2]), name     # v = 0: the slot-0 position is the start, exactly


def test_at_most_two_fuzz_seeds_are_redrawn():
    import dwa_subgoal_cases as D
    drawn = [D.fuzz_case(s) for s in D.FUZZ_SEEDS]
    print("redrawn seeds:", [s for s, (c, r) in zip(D.FUZZ_SEEDS, drawn) if r])
    assert len(D.FUZZ_SEEDS) == 24 and sum(r for c, r in drawn) <= 2
    assert all(D.margin(c) > L.DELTA for c, r in drawn)
    assert sum(c["path"] is not None for c, r in drawn) >= 18 and len({c["geo"] for c, r in drawn}) == 3


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
