"""GPU: the fused A* + DWA closed loop (benchnav_amd.AStarDWALoop, bn_astar_dwa_episode_async, csrc/astar_dwa.hip) against the
same loop composed from the library's stand-alone calls -- bn_astar_path -> bn_mppi_dwa_forward_async -> bn_mppi_env_step, the
path built on the host as AStar.forward builds it -- bit for bit, free-running; batches against single runs; chunked calls; the
drop-in classes (AStar, DWA, BatchedPlanetaryEnv) driven like test_astar_dwa.py; argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import astar_maps as M
from astar_dwa_scenarios import G, RES, THR, T, A_LIM, DWA_DT, NV, NW, LOOK, CASES     # the problem, shared with the oracle tests
from astar_dwa_scenarios import case as _case, smooth_risk as _smooth_risk

pytestmark = pytest.mark.gpu

STEPS = 300


def _env(B, risks, starts, goals, freeze=False, **kw):
    from benchnav_amd import NativeMPPI
    from benchnav_amd.env import BatchedPlanetaryEnv
    pl = NativeMPPI(horizon=T, num_samples=64, grid_size=G, resolution=RES, num_instances=B, shared_map=(B == 1), stream=0,
                    stuck_threshold=THR, **kw)
    mean = (np.float32(0.2) + np.float32(0.1) * _smooth_risk(99, 0.0, 1.0)).astype(np.float32)     # the latent slip model
    std = np.full((G, G), 0.05, np.float32)
    env = BatchedPlanetaryEnv(pl, mean, std, starts, goals, stuck_threshold=THR, goal_threshold=1.0, seed=7, freeze_on_goal=freeze)
    return pl, env


def _loop(env, heights, risks, **kw):
    from benchnav_amd import AStarDWALoop
    return AStarDWALoop(env, heights, risks, THR, A_LIM, DWA_DT, NV, NW, LOOK, **kw)


def _composed(pl, env, loop, n, z):
    """The loop from the library's separate calls, B = 1 (bn_mppi_dwa_forward_async takes one path for all instances)."""
    from benchnav_amd import _capi
    from benchnav_amd.astar import _DevArray
    lib, h, dev = pl._lib, pl._h, env._dev
    state = env._robot_state.clone()
    prev = torch.zeros(1, 2, device=dev)
    reward = torch.empty(1, device=dev)
    term = torch.empty(1, dtype=torch.int32, device=dev)
    alim = (C.c_float * 2)(*A_LIM)
    buf = np.empty((G * G, 2), np.int32)
    goal = env._goal_pos.cpu().numpy()[0]
    gx, gy = loop.pos_to_index(goal)
    goal_in = 0 <= gx < G and 0 <= gy < G
    goal_col = goal_in and loop._risks[0][gy, gx] <= np.float32(THR)
    path = None
    nan2 = np.full(2, np.nan, np.float32)
    S, R, A, SG = [state.cpu().numpy()[0]], [], [], []
    status, status_step, done = 0, -1, -1
    for j in range(n):
        s = S[-1]
        if status == 0:
            ix, iy = loop.pos_to_index(s[:2])
            if not (0 <= ix < G and 0 <= iy < G) or not goal_in:
                status, status_step = _capi.BN_AD_OUT_OF_BOUNDS, j
            elif goal_col:
                status, status_step = _capi.BN_AD_GOAL_COLLISION, j
        if status != 0:
            S.append(s); R.append(np.float32(np.nan)); A.append(nan2); SG.append(nan2)
            continue
        cnt = lib.bn_astar_path(loop._astar, 0, ix, iy, buf.ctypes.data_as(C.POINTER(C.c_int32)), buf.shape[0])
        assert cnt >= 0
        if cnt > 0:                                                   # else None: update_reference_path keeps the previous path
            path = torch.from_numpy(buf[:cnt].astype(np.float32) * np.float32(RES)).to(dev).contiguous()
        _capi.check(lib.bn_mppi_dwa_forward_async(h, C.c_void_p(state.data_ptr()), C.c_void_p(prev.data_ptr()), alim, DWA_DT, NV, NW,
                                                  None if path is None else C.c_void_p(path.data_ptr()),
                                                  0 if path is None else path.shape[0], LOOK, None))
        g = C.c_void_p()
        _capi.check(lib.bn_mppi_dwa_candidates(h, NV * NW, None, C.byref(g)))
        SG.append(torch.as_tensor(_DevArray(g.value, (2,)), device=dev).cpu().numpy().copy())
        A.append(prev.cpu().numpy()[0].copy())
        zj = z[j:j + 1].contiguous()
        _capi.check(lib.bn_mppi_env_step(h, C.c_void_p(prev.data_ptr()), C.c_void_p(state.data_ptr()), C.c_void_p(reward.data_ptr()),
                                         C.c_void_p(term.data_ptr()), C.c_void_p(zj.data_ptr()), j))
        S.append(state.cpu().numpy()[0].copy())
        R.append(reward.cpu().numpy()[0])
        if done < 0 and int(term.cpu()[0]):
            done = j
    return (np.stack(S)[:, None], np.asarray(R, np.float32)[:, None], np.stack(A)[:, None], np.stack(SG)[:, None],
            done, status, status_step)


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("name", CASES)
def test_fused_equals_composed_library_loop(name):
    from benchnav_amd import _capi
    heights, risk, start, goal, kw = _case(name)
    pl, env = _env(1, risk, start, goal, **kw)
    loop = _loop(env, heights, risk)
    env.reset()
    z = torch.from_numpy(np.random.default_rng(11).standard_normal((STEPS, 1)).astype(np.float32)).cuda()
    ref = _composed(pl, env, loop, STEPS, z)
    states, rewards, actions, sub_goals, done, status = loop.run(STEPS, z=z)
    for what, got, want in (("states", states, ref[0]), ("rewards", rewards, ref[1]), ("actions", actions, ref[2]),
                            ("sub_goals", sub_goals, ref[3])):
        bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
        assert bad.size == 0, f"{name}: {what} differ first at step {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    assert (int(done[0]), int(status[0]), int(loop.status_step[0])) == (ref[4], ref[5], ref[6])
    if name == "edge":
        assert status[0] == _capi.BN_AD_OUT_OF_BOUNDS and loop.status_step[0] > 0
        with pytest.raises(ValueError, match="Start or goal position is out of bounds."):
            loop.raise_for_status()
    elif name == "goal_collision":
        assert status[0] == _capi.BN_AD_GOAL_COLLISION and loop.status_step[0] == 0
        with pytest.raises(ValueError, match="Goal position is not traversable."):
            loop.raise_for_status()
    else:
        assert status[0] == _capi.BN_AD_OK
        loop.raise_for_status()
    if name == "disconnected":                 # no path left of the wall: until the rover first crosses it the stage goal is the goal
        left = np.floor(states[:-1, 0, 0] / RES) < 20
        n_left = int(np.argmin(left)) if not left.all() else len(left)
        assert n_left > 0 and np.all(sub_goals[:n_left, 0] == np.float32(goal))
    if name == "low_risk_patch":               # the rover crossed the patch, where the path is None and the previous one is kept
        ix = np.floor(states[:-1, 0, 0] / RES).astype(int)
        iy = np.floor(states[:-1, 0, 1] / RES).astype(int)
        assert np.any((ix - 30) ** 2 + (iy - 30) ** 2 <= 16), "the episode never entered the patch interior"


def _batch_case(k):
    rng = np.random.default_rng(100 + k)
    heights = M.smooth_heights(G, G, 200 + k)
    risk = _smooth_risk(300 + k)
    if k % 3 == 1:
        c = rng.integers(20, 44, 2)
        yy, xx = np.mgrid[0:G, 0:G]
        risk[(xx - c[0]) ** 2 + (yy - c[1]) ** 2 <= 25] = 0.05
    start = rng.uniform(2.0, 12.0, 2).astype(np.float32)
    goal = rng.uniform(18.0, 30.0, 2).astype(np.float32)
    if k % 7 == 3:
        goal[0] = 31.9                         # near the edge
    if k % 9 == 4:                             # a goal in collision: this instance stops at step 0
        risk[int(goal[1] / RES), int(goal[0] / RES)] = 0.1
    if k % 9 == 7:                             # a start on the x = G * res edge: out of bounds at step 0
        start[0] = G * RES
    return heights, risk, start, goal


def test_batch_of_64_equals_single_runs():
    B, n = 64, 200
    cases = [_batch_case(k) for k in range(B)]
    H = np.stack([c[0] for c in cases]); R = np.stack([c[1] for c in cases])
    S = np.stack([c[2] for c in cases]); Gp = np.stack([c[3] for c in cases])
    z = torch.from_numpy(np.random.default_rng(5).standard_normal((n, B)).astype(np.float32)).cuda()
    pl, env = _env(B, R, S, Gp)
    loop = _loop(env, H, R)
    env.reset()
    out = loop.run(n, z=z)
    assert set(out[5]) >= {0, 1, 2}            # running, out of bounds and goal-collision instances in one batch
    for b in range(B):                         # every instance against its own B = 1 run
        pl1, env1 = _env(1, R[b], S[b], Gp[b])
        loop1 = _loop(env1, H[b], R[b])
        env1.reset()
        one = loop1.run(n, z=z[:, b:b + 1].contiguous())
        for i in range(4):
            assert _eq(out[i][:, b], one[i][:, 0]), (b, i)
        assert out[4][b] == one[4][0] and out[5][b] == one[5][0], b
        del loop1, env1, pl1


def test_chunked_calls_equal_one_call():
    heights, risk, start, goal, kw = _case("low_risk_patch")
    kw = {}
    n, k = 400, 260                            # k crosses the 256 steps of one launch
    z = torch.from_numpy(np.random.default_rng(3).standard_normal((n, 1)).astype(np.float32)).cuda()
    pl, env = _env(1, risk, start, goal)
    loop = _loop(env, heights, risk)
    env.reset()
    whole = loop.run(n, z=z)
    env.reset()
    first = loop.run(k, z=z[:k].contiguous())
    second = loop.run(n - k, z=z[k:].contiguous())
    assert _eq(whole[0][:k + 1], first[0]) and _eq(whole[0][k:], second[0])
    for i in (1, 2, 3):
        assert _eq(whole[i], np.concatenate([first[i], second[i]])), i
    assert np.array_equal(whole[4], second[4]) and np.array_equal(whole[5], second[5])
    # Philox draws (no z): the same
    env.reset()
    whole = loop.run(n)
    env.reset()
    first, second = loop.run(k), loop.run(n - k)
    assert _eq(whole[0][k:], second[0]) and _eq(whole[2], np.concatenate([first[2], second[2]]))


def test_drop_in_classes_loop_matches_run():
    """test_astar_dwa.py:179-211 with benchnav_amd.AStar, DWA and BatchedPlanetaryEnv (B = 1, Philox draws) next to run()."""
    from benchnav_amd import AStar, DWA
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    heights, risk, start, goal, kw = _case("smooth")
    n = 250
    pl, env = _env(1, risk, start, goal)
    loop = _loop(env, heights, risk)
    state = env.reset(seed=0)
    fused = loop.run(n)

    pl2, env2 = _env(1, risk, start, goal)
    gm = FakeGridMap(G, RES)
    gm.tensors = {"heights": torch.from_numpy(heights).cuda()}
    dyn = FakeDynamics(torch.from_numpy(risk).cuda(), gm)
    solver = DWA(horizon=T, dim_state=3, dim_control=2, dynamics=dyn, objectives=FakeObjectives(torch.tensor(goal), THR),
                 a_lim=torch.tensor(A_LIM), delta_t=DWA_DT, num_lin_vel=NV, num_ang_vel=NW)
    astar = AStar(grid_map=gm, goal_pos=torch.tensor(goal), dynamics=dyn, stuck_threshold=THR)
    state = env2.reset(seed=0)[0]
    states, actions, goal_step = [state.cpu().numpy()], [], -1
    for j in range(n):
        with torch.no_grad():
            reference_path = astar.forward(state=state)
            solver.update_reference_path(reference_path)
            action_seq, state_seq = solver.forward(state=state)
        st, reward, is_terminated, is_truncated = env2.step(action_seq[0, :].reshape(1, 2))
        state = st[0]
        states.append(state.cpu().numpy())
        actions.append(action_seq[0].cpu().numpy())
        if goal_step < 0 and bool(is_terminated[0]):
            goal_step = j
    assert np.array_equal(np.stack(states), fused[0][:, 0])
    assert np.array_equal(np.stack(actions), fused[2][:, 0])
    assert goal_step == int(fused[4][0])


def test_argument_errors():
    from benchnav_amd import _capi, AStarDWALoop
    heights, risk, start, goal, kw = _case("smooth")
    pl, env = _env(2, np.stack([risk, risk]), start, goal)
    loop = _loop(env, heights, risk)
    lib, h = pl._lib, pl._h
    alim = (C.c_float * 2)(*A_LIM)
    prev = torch.zeros(2, 2, device="cuda")
    st = env._robot_state.contiguous()

    def call(a, nv=NV, nw=NW, states=st):
        return lib.bn_astar_dwa_episode_async(h, a, 5, C.c_void_p(states.data_ptr()), _capi.BN_MEM_DEVICE, C.c_void_p(prev.data_ptr()),
                                              alim, DWA_DT, nv, nw, LOOK, None)

    def astar(B, n):
        a = C.c_void_p()
        assert lib.bn_astar_create(0, n, n, B, C.byref(a)) == 0
        for b in range(B):
            hh, rr = np.ascontiguousarray(heights[:n, :n]), np.ascontiguousarray(risk[:n, :n])
            assert lib.bn_astar_set_map(a, b, C.c_void_p(hh.ctypes.data), C.c_void_p(rr.ctypes.data), _capi.BN_MEM_HOST, THR, RES) == 0
            assert lib.bn_astar_set_goal(a, b, 5, 5) == 0
        return a

    unsolved = astar(2, G)
    assert call(unsolved) == _capi.BN_ERR_STATE and b"solve" in lib.bn_last_error()
    wrong_b = astar(1, G)
    assert lib.bn_astar_solve_async(wrong_b, None) == 0
    assert call(wrong_b) == _capi.BN_ERR_INVALID and b"instances" in lib.bn_last_error()
    wrong_g = astar(2, 32)
    assert lib.bn_astar_solve_async(wrong_g, None) == 0
    assert call(wrong_g) == _capi.BN_ERR_INVALID and b"grid" in lib.bn_last_error()
    assert call(loop._astar, nv=33, nw=32) == _capi.BN_ERR_INVALID and b"1024" in lib.bn_last_error()
    assert call(None) == _capi.BN_ERR_INVALID
    assert lib.bn_astar_dwa_episode_async(h, loop._astar, 0, C.c_void_p(st.data_ptr()), _capi.BN_MEM_DEVICE, C.c_void_p(prev.data_ptr()),
                                          alim, DWA_DT, NV, NW, LOOK, None) == _capi.BN_ERR_INVALID
    assert call(loop._astar) == 0
    for a in (unsolved, wrong_b, wrong_g):
        lib.bn_astar_destroy(a)
    # a handle without an environment
    from benchnav_amd import NativeMPPI
    bare = NativeMPPI(horizon=T, num_samples=64, grid_size=G, resolution=RES, num_instances=2, stream=0)
    bare.set_map(risk)
    bare.set_goal(np.asarray(goal, np.float32))
    assert lib.bn_astar_dwa_episode_async(bare._h, loop._astar, 5, C.c_void_p(st.data_ptr()), _capi.BN_MEM_DEVICE,
                                          C.c_void_p(prev.data_ptr()), alim, DWA_DT, NV, NW, LOOK, None) == _capi.BN_ERR_STATE
    assert b"env_attach" in lib.bn_last_error()
    # Python: shapes of the maps and of z, and a loop out of step with its environment
    with pytest.raises(ValueError, match="heights"):
        AStarDWALoop(env, heights[:10], risk, THR, A_LIM, DWA_DT)
    with pytest.raises(ValueError, match="1024"):
        AStarDWALoop(env, heights, risk, THR, A_LIM, DWA_DT, num_lin_vel=64, num_ang_vel=17)
    env.reset()
    with pytest.raises(ValueError, match="z must be"):
        loop.run(4, z=torch.zeros(3, 2, device="cuda"))
    env.step(torch.zeros(2, 2, device="cuda"))
    with pytest.raises(RuntimeError, match="since its reset"):
        loop.run(4)


# ---- the reference fixture (tests/golden/make_golden_astar_dwa.py): one teacher-forced run() step from every stored step ----
MARGIN = 1e-5      # the chosen candidate is compared where the reference's best cost is this clear of the next distinct one


@pytest.mark.parametrize("name", ["smooth", "patch", "inside", "edge"])
def test_one_step_runs_against_the_reference_fixture(name):
    import os
    from benchnav_amd import _capi
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "astar_dwa_loop.npz")) as z:
        fx = {k: z[k] for k in z.files}
    f = lambda k: fx[f"{name}__{k}"]
    mean = f("mean")
    kw = {} if bool(f("steer")) else dict(u_min=(0.5, 0.0), u_max=(1.0, 0.0))
    from benchnav_amd import NativeMPPI, AStarDWALoop
    from benchnav_amd.env import BatchedPlanetaryEnv
    pl = NativeMPPI(horizon=int(fx["T"]), num_samples=64, grid_size=G, resolution=RES, stream=0, stuck_threshold=float(fx["thr"]), **kw)
    n = len(f("z"))
    env = BatchedPlanetaryEnv(pl, mean, np.full((G, G), float(fx["std"]), np.float32), f("state")[0, :2], f("goal"),
                              stuck_threshold=float(fx["thr"]), goal_threshold=float(fx["goal_threshold"]))
    loop = AStarDWALoop(env, f("heights"), mean, float(fx["thr"]), tuple(fx["a_lim"]), float(fx["delta_t"]), int(fx["nv"]),
                        int(fx["nw"]), float(fx["lookahead"]))

    def one(state, prev, root, z):
        env.reset()
        env._robot_state = torch.from_numpy(np.asarray(state, np.float32)).reshape(1, 3).cuda()
        loop._prev.copy_(torch.from_numpy(np.asarray(prev, np.float32)).reshape(1, 2))
        loop.set_root(0, None if root[0] < 0 else root)
        return loop.run(1, z=torch.tensor([[z]], dtype=torch.float32))

    exact = 0
    for j in range(n):
        states, rewards, actions, sub_goals, done, status = one(f("state")[j], f("prev")[j], f("root")[j], float(f("z")[j]))
        assert status[0] == _capi.BN_AD_OK, (name, j)
        assert np.array_equal(sub_goals[0, 0], f("sub_goal")[j]), (name, j, sub_goals[0, 0], f("sub_goal")[j])
        if f("margin")[j] >= MARGIN:
            import astar_dwa_oracle as L
            w = L.window(f("prev")[j], tuple(fx["a_lim"]), float(fx["delta_t"]), int(fx["nv"]), int(fx["nw"]),
                         *((kw["u_min"], kw["u_max"]) if kw else ((0.0, -1.0), (1.0, 1.0))))
            got, ref = actions[0, 0], f("action")[j]
            assert int(np.argmin(np.abs(w - got).sum(1))) == int(np.argmin(np.abs(w - ref).sum(1))), (name, j)
            assert np.abs(got - ref).max() <= 1e-6, (name, j)
            assert np.abs(states[1, 0] - f("next_state")[j]).max() <= 1e-4, (name, j)      # test_dwa.py's dwa.npz tolerance
            exact += 1
    assert exact >= 0.8 * n
    rs = int(f("raise_step"))
    if rs >= 0:                                # AStar.forward raised from the last stored next state: status at that step
        states, rewards, actions, sub_goals, done, status = one(f("next_state")[n - 1], f("action")[n - 1], (-1, -1), 0.0)
        assert status[0] == _capi.BN_AD_OUT_OF_BOUNDS and loop.status_step[0] == 0 and np.isnan(actions[0, 0]).all()
        with pytest.raises(ValueError, match="Start or goal position is out of bounds."):
            loop.raise_for_status()
