"""GPU: the fused A* + DWA loop reading its path through the A* jump tables (AStarDWALoop(walk="jump"), bn_astar_dwa_set_walk(1),
csrc/astar_dwa.hip) against the serial next-hop walk, bit for bit: on a valid field both visit the same nodes in the same order."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_astar_dwa as T

pytestmark = pytest.mark.gpu

STEPS = 40


def _z(n, B, seed=21):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, B)).astype(np.float32)).cuda()


def _run(name, walk, z, nv=T.NV, nw=T.NW, chunks=None):
    """One B = 1 episode of case `name`: run()'s six arrays, the status steps and the environment's state afterwards."""
    from benchnav_amd import AStarDWALoop
    heights, risk, start, goal, kw = T._case(name)
    pl, env = T._env(1, risk, start, goal, **kw)
    loop = AStarDWALoop(env, heights, risk, T.THR, T.A_LIM, T.DWA_DT, nv, nw, T.LOOK, walk=walk)
    assert loop.walk == walk
    env.reset()
    n = z.shape[0]
    if chunks is None:
        out = loop.run(n, z=z)
    else:
        parts, at = [], 0
        for k in chunks:
            parts.append(loop.run(k, z=z[at:at + k].contiguous()))
            at += k
        out = (np.concatenate([parts[0][0]] + [p[0][1:] for p in parts[1:]]),) + \
              tuple(np.concatenate([p[i] for p in parts]) for i in (1, 2, 3)) + (parts[-1][4], parts[-1][5])
    return out + (loop.status_step.copy(), env._robot_state.cpu().numpy(), env._steps)


def _same(a, b, what):
    assert len(a) == len(b) == 9
    for i, (x, y) in enumerate(zip(a, b)):
        assert T._eq(x, y), (what, i)


@pytest.fixture(scope="module")
def serial():
    """The serial walk's episodes, computed once per (case, candidates) and shared."""
    cache = {}

    def get(name, nv=T.NV, nw=T.NW, n=STEPS):
        key = (name, nv, nw, n)
        if key not in cache:
            cache[key] = _run(name, "serial", _z(n, 1), nv, nw)
        return cache[key]
    return get


@pytest.mark.parametrize("name", T.CASES)
def test_jump_walk_equals_serial_walk(name, serial):
    from benchnav_amd import _capi
    want = serial(name)
    got = _run(name, "jump", _z(STEPS, 1))
    _same(got, want, name)
    if name == "goal_collision":
        assert got[5][0] == _capi.BN_AD_GOAL_COLLISION
    if name in ("smooth", "maze", "low_risk_patch"):       # a path from the first step on: every stage goal is one of its points
        assert got[5][0] == _capi.BN_AD_OK and np.isfinite(got[3]).all()


@pytest.mark.parametrize("nv,nw", [(3, 5), (32, 32)])
def test_maze_segments_and_lane_counts(nv, nw, serial):
    """Paths of ~2000 nodes: 64 lanes walk them in ~32 segments; 1024 lanes use the stride of 1024 and level 10."""
    want = serial("maze", nv, nw)
    got = _run("maze", "jump", _z(STEPS, 1), nv, nw)
    _same(got, want, (nv, nw))
    # the sub-goal is a path point (a cell corner), not the goal: the walk found the nearest node ahead
    assert not np.array_equal(got[3][0, 0], np.float32(T._case("maze")[3]))


def test_batch_of_four_equals_single_serial_runs(serial):
    from benchnav_amd import _capi
    names = ("smooth", "maze", "disconnected", "goal_collision")
    cases = [T._case(n) for n in names]
    H = np.stack([c[0] for c in cases]); R = np.stack([c[1] for c in cases])
    S = np.float32([c[2] for c in cases]); Gp = np.float32([c[3] for c in cases])
    z = _z(STEPS, 1).repeat(1, 4).contiguous()             # every instance gets the single runs' draws
    pl, env = T._env(4, R, S, Gp)
    loop = T._loop(env, H, R, walk="jump")
    env.reset()
    out = loop.run(STEPS, z=z)
    state = env._robot_state.cpu().numpy()
    for b, name in enumerate(names):
        one = serial(name)
        assert T._eq(state[b], one[7][0]) and env._steps == one[8], name       # the environment ends where the single run's does
        for i in range(4):
            assert T._eq(out[i][:, b], one[i][:, 0]), (name, i)
        assert out[4][b] == one[4][0] and out[5][b] == one[5][0] and loop.status_step[b] == one[6][0], name
    assert out[5].tolist() == [0, 0, 0, _capi.BN_AD_GOAL_COLLISION]


def test_chunked_jump_calls_equal_one_call(serial):
    want = serial("maze", n=20)
    got = _run("maze", "jump", _z(20, 1), chunks=(7, 13))
    _same(got, want, "7 + 13")


def test_root_fallback_under_the_jump_walk():
    """A reachable start sets the root; the rover is then put inside the low-risk patch, where A* has no path (None): the
    walk runs from the root cell."""
    heights, risk, start, goal, kw = T._case("low_risk_patch")
    inside = np.float32([[30.3 * T.RES, 30.6 * T.RES, 0.4]])
    z = _z(10, 1, seed=4)
    outs = {}
    for walk in ("serial", "jump"):
        pl, env = T._env(1, risk, start, goal)
        loop = T._loop(env, heights, risk, walk=walk)
        env.reset()
        first = loop.run(4, z=z[:4].contiguous())
        buf = np.empty((8, 2), np.int32)
        assert pl._lib.bn_astar_path(loop._astar, 0, 30, 30, buf.ctypes.data_as(C.POINTER(C.c_int32)), 8) == 0     # None
        env._robot_state = torch.from_numpy(inside).cuda()
        second = loop.run(6, z=z[4:].contiguous())
        assert second[5][0] == 0 and np.isfinite(second[3]).all()
        assert not np.array_equal(second[3][0, 0], np.float32(goal))       # a point of the kept path, not the goal
        outs[walk] = first + second + (loop.status_step.copy(), env._robot_state.cpu().numpy())
    for i, (x, y) in enumerate(zip(outs["jump"], outs["serial"])):
        assert T._eq(x, y), i


def test_walk_selection_errors():
    from benchnav_amd import _capi, AStarDWALoop
    heights, risk, start, goal, kw = T._case("smooth")
    pl, env = T._env(1, risk, start, goal)
    with pytest.raises(ValueError, match="walk"):
        AStarDWALoop(env, heights, risk, T.THR, T.A_LIM, T.DWA_DT, walk="doubling")
    loop = T._loop(env, heights, risk)                     # the default: the serial walk, no tables
    assert loop.walk == "serial"
    lib, h = pl._lib, pl._h
    hp, jp, lv, eb = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
    assert lib.bn_astar_jump_buffers(loop._astar, 0, C.byref(hp), C.byref(jp), C.byref(lv), C.byref(eb)) == _capi.BN_ERR_STATE
    env.reset()
    alim = (C.c_float * 2)(*T.A_LIM)
    prev = torch.zeros(1, 2, device="cuda")
    st = env._robot_state.contiguous()

    def episode():
        return lib.bn_astar_dwa_episode_async(h, loop._astar, 3, C.c_void_p(st.data_ptr()), _capi.BN_MEM_DEVICE, C.c_void_p(prev.data_ptr()),
                                              alim, T.DWA_DT, T.NV, T.NW, T.LOOK, None)
    assert lib.bn_astar_dwa_set_walk(h, 2) == _capi.BN_ERR_INVALID
    assert lib.bn_astar_dwa_set_walk(h, 1) == 0
    assert episode() == _capi.BN_ERR_STATE and b"jump tables" in lib.bn_last_error()
    assert lib.bn_astar_jump_build_async(loop._astar, None) == 0
    assert episode() == 0
    assert lib.bn_astar_dwa_set_walk(h, 0) == 0
    assert episode() == 0
    assert lib.bn_mppi_sync(h) == 0
