"""GPU: DWA.forward's path -> sub-goal stage (dwa_window_kernel in csrc/mppi_kernels.hip with csrc/dwa_device.h, driven through
bn_mppi_dwa_forward_async) on synthetic float paths, held to the CPU oracle per instance: the window against
astar_dwa_oracle.window, the stage goal against oracle.dwa_sub_goal bit for bit, and the rollouts, costs and argmin against
oracle.dwa on the device's own candidates bit for bit.  The inputs come from tests/dwa_subgoal_cases.py, which
tests/test_astar_dwa_oracle.py checks on the CPU to be clear of the atan2f ambiguity band."""
import ctypes as C
import functools

import numpy as np
import pytest

import astar_dwa_oracle as L
import dwa_subgoal_cases as D
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _planner(geo, lds, bounds, B):
    from benchnav_amd import NativeMPPI
    G, res, xl = geo
    pl = NativeMPPI(horizon=D.T, num_samples=64, grid_size=G, resolution=res, x_limits=xl, y_limits=xl, u_min=bounds[0], u_max=bounds[1],
                    stuck_threshold=D.THR, num_instances=B, shared_map=True, lds_window=lds, stream=0)
    pl.set_map(D.risk_map(G))
    pl.set_goal(D.goal_of(geo))
    return pl


def _forward(cfg):
    """One bn_mppi_dwa_forward_async: dict(actions (B, NA, 2), goal (B, 2), X (B, NA, T + 1, 3), cost (B, NA), best_action (B, 2),
    best_states (B, T + 1, 3))."""
    import torch
    from benchnav_amd import _capi
    from benchnav_amd.astar import _DevArray
    B, NA = len(cfg["states"]), cfg["nv"] * cfg["nw"]
    pl = _planner(cfg["geo"], cfg["lds"], cfg["bounds"], B)
    lib, h = pl._lib, pl._h
    state = torch.from_numpy(cfg["states"]).cuda()
    prev = torch.from_numpy(cfg["prev"].copy()).cuda()
    path = None if cfg["path"] is None else torch.from_numpy(cfg["path"]).cuda()
    best_states = torch.empty(B, D.T + 1, 3, device="cuda")
    _capi.check(lib.bn_mppi_dwa_forward_async(h, C.c_void_p(state.data_ptr()), C.c_void_p(prev.data_ptr()), (C.c_float * 2)(*D.A_LIM),
                                              D.DWA_DT, cfg["nv"], cfg["nw"], None if path is None else C.c_void_p(path.data_ptr()),
                                              0 if path is None else path.shape[0], cfg["look"], C.c_void_p(best_states.data_ptr())))
    a, g, x, c = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    _capi.check(lib.bn_mppi_dwa_candidates(h, NA, C.byref(a), C.byref(g)))
    _capi.check(lib.bn_mppi_dwa_buffers(h, NA, C.byref(x), C.byref(c), None))
    torch.cuda.synchronize()
    view = lambda p, shape: torch.as_tensor(_DevArray(p.value, shape), device="cuda").cpu().numpy().copy()
    return dict(actions=view(a, (B, NA, 2)), goal=view(g, (B, 2)), X=view(x, (B, NA, D.T + 1, 3)), cost=view(c, (B, NA)),
                best_action=prev.cpu().numpy(), best_states=best_states.cpu().numpy())


def _check(name, cfg):
    assert D.margin(cfg) > L.DELTA, name                                     # by the oracle alone, before the device runs
    got = _forward(cfg)
    p, risk = D.params(cfg), D.risk_map(cfg["geo"][0])
    picks = []
    for b in range(len(cfg["states"])):
        w = L.window(cfg["prev"][b], D.A_LIM, D.DWA_DT, cfg["nv"], cfg["nw"], *cfg["bounds"])
        act = got["actions"][b]
        assert np.abs(act - w).max() <= 1e-6 and np.array_equal(act[0], w[0]), (name, b)
        if cfg["path"] is None:
            sg, idx = D.goal_of(cfg["geo"]), None
        else:
            sg, sel, idx = O.dwa_sub_goal(p, risk, cfg["states"][b], act[0], cfg["path"], cfg["look"])
        assert np.array_equal(got["goal"][b], sg), (name, b, idx, got["goal"][b], sg)
        orc = O.dwa(p, risk, cfg["states"][b], act, got["goal"][b])
        assert np.array_equal(got["X"][b], orc["X"]) and np.array_equal(got["cost"][b], orc["cost"]), (name, b)
        assert np.array_equal(got["best_action"][b], act[orc["best"]]), (name, b)
        assert np.array_equal(got["best_states"][b], orc["X"][orc["best"]]), (name, b)
        picks.append(idx)
    if "expect" in cfg:                                                      # what the case is built to pick, stated without the oracle
        assert picks[0] == cfg["expect"] and np.array_equal(got["goal"][0], cfg["path"][cfg["expect"]]), (name, picks)
    return picks


@pytest.mark.parametrize("P", D.LENGTHS)
def test_path_lengths_at_and_across_the_256_lane_stride(P):
    _check(f"length{P}", D.length_case(P))


@pytest.mark.parametrize("name,cfg", D.tie_cases(), ids=[n for n, c in D.tie_cases()])
def test_exact_ties_pick_the_lowest_index(name, cfg):
    i = cfg["expect"]
    dx, dy = cfg["path"][:, 0] - np.float32(8.0), cfg["path"][:, 1] - np.float32(8.0)
    d = np.sqrt(dx * dx + dy * dy)                                           # float32, as the rule computes it
    assert (d == d[i]).sum() == 3 and d.min() == d[i]                        # three points at the nearest distance, to the bit
    _check(name, cfg)


@pytest.mark.parametrize("name,cfg", D.lookahead_cases() + D.nothing_ahead_cases() + D.unwrapped_cases(),
                         ids=[n for n, c in D.lookahead_cases() + D.nothing_ahead_cases() + D.unwrapped_cases()])
def test_look_ahead_edge_nothing_ahead_and_the_unwrapped_bearing(name, cfg):
    _check(name, cfg)


@pytest.mark.parametrize("kind", ["inside", "one_side", "both_sides", "outside"])
@pytest.mark.parametrize("nv,nw", D.SHAPES)
def test_window_shapes_and_cuts(nv, nw, kind):
    _check(f"shape{nv}x{nw}_{kind}", D.shape_case(nv, nw, kind))


def test_five_states_on_one_shared_path():
    cfg = D.batch_case()
    picks = _check("batch", cfg)
    assert len(set(picks)) >= 3                                             # the instances do pick differently


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("g", range(len(D.GEOS)))
def test_geometries(g, lds):
    _check(f"geo{g}_{int(lds)}", D.geometry_case(D.GEOS[g], lds))


@pytest.mark.parametrize("seed", D.FUZZ_SEEDS)
def test_random_sub_goal_configuration_matches_oracle(seed):
    cfg, redrawn = D.fuzz_case(seed)
    _check(f"fuzz{seed}{'r' if redrawn else ''}", cfg)
