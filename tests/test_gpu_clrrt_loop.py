"""GPU: benchnav_amd.CLRRTLoop (bn_clrrt_loop_run, csrc/clrrt_loop.hip) against the reference's recorded episodes
(tests/golden/clrrt_loop.npz) and the NumPy spec (tests/clrrt_loop_spec.py).

1. the follow kernel teacher-forced per plan segment of the three episodes (set_plans, the recorded state and z);
2. the follow kernel against the spec on synthetic plans: the global-memory path past the LDS budget, PLAN_EXHAUSTED, a replan
   flagged on iteration 1, TIME_LIMIT, and the LDS staging forced off (`run(..., stage_in_lds=False)`, the test-only knob) and on;
3. the fused loop with injected samples and z, B = 1, the three episodes, WHOLE: tests/clrrt_spec.py calls steers marginal in
   every plan of this fixture (the start heading points at the goal along the map's diagonal), so no plan is left out;
4. masks and batches: a batch against single runs, an inactive rover's bytes, chunked calls, reset, raise_for_status.

Measured on an MI355X: see FOLLOW_TOL and STATE_TOL below."""
import os

import numpy as np
import pytest
import torch

import clrrt_loop_spec as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G, RES, THR = 64, 0.5, 0.2
# Largest |state|, |reward|, |deviation| difference against the fixture, measured on an MI355X:
#   teacher-forced segments (test 1): 0 on every one of the seven segments -> asserted equal (FOLLOW_TOL = 0);
#   free-running fused episodes (test 3): 7.63e-6 (s14; s10 3.81e-6, s04 0) -> asserted 3e-5 (3.9 x).  There the PLANS are the
#   device planner's, which differ from the recorded ones by DESIGN.md 4.7's 5.9e-6 in actions and states (float32
#   transcendentals of the Dubins words); the follow kernel adds nothing to that.
# Condition, not measurement: both stay below half the fixture's smallest |dev - 1| (1.69e-3), or a replan decision could flip
# inside the tolerance.
FOLLOW_TOL = 0.0
STATE_TOL = 3e-5
assert FOLLOW_TOL <= STATE_TOL <= 8e-4
EPISODES = ("s10", "s14", "s04")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "clrrt_loop.npz"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_logs(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _make(fx, B, scale, starts=None, goals=None, seeds=None, time_limit=None):
    """(env, planner, loop): B rovers on the fixture's map with the latent model scaled by `scale`."""
    from benchnav_amd import CLRRT, CLRRTLoop, NativeMPPI
    from benchnav_amd.env import BatchedPlanetaryEnv
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    mean = fx["mean"]
    pl = NativeMPPI(horizon=8, num_samples=64, grid_size=G, resolution=RES, num_instances=B, shared_map=True, stream=0, stuck_threshold=THR)
    lat = np.clip(mean * np.float32(scale), 0.0, 0.7).astype(np.float32)
    std = np.full((G, G), float(fx["std"]), np.float32)
    starts = fx["start"] if starts is None else np.asarray(starts, np.float32)
    goals = fx["goal"] if goals is None else np.asarray(goals, np.float32)
    env = BatchedPlanetaryEnv(pl, lat, std, starts, goals, delta_t=float(fx["delta_t"]), time_limit=float(fx["time_limit"]) if time_limit is None else time_limit,
                              stuck_threshold=THR, goal_threshold=float(fx["goal_threshold"]), seed=1)
    gm = FakeGridMap(G, RES)
    iters, max_seqs, seed, _ = (int(v) for v in fx["params"])
    planner = CLRRT(3, 2, FakeDynamics(mean, gm), FakeObjectives(torch.as_tensor(fx["goal"].copy()), THR), gm, delta_t=float(fx["delta_t"]),
                    max_iterations=iters, max_seqs=max_seqs, seed=seed)
    loop = CLRRTLoop(env, planner, seeds=seeds)
    env.reset(seed=0)
    return env, planner, loop


def _z(fx, name, t0, n):
    z = np.nan_to_num(fx[f"{name}__z"][t0:t0 + n], nan=0.0).astype(np.float32)
    return torch.from_numpy(z[:, None].copy())


# ---- 1. the follow kernel, teacher-forced per plan segment --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def segments(fx):
    """Every plan segment of the three episodes through set_plans: (episode, plan, first iteration, log)."""
    out = []
    N = int(fx["params"][3])
    for name in EPISODES:
        env, planner, loop = _make(fx, 1, float(fx[f"{name}__scale"]))
        its = fx[f"{name}__plan_iter"].tolist()
        for k, t0 in enumerate(its):
            if not bool(fx[f"{name}__p{k}__found"]):
                continue
            t1 = its[k + 1] if k + 1 < len(its) else N            # up to and including the next replan flag (iteration t1 - 1) or the end
            env.reset(seed=0)
            env._robot_state = torch.as_tensor(fx[f"{name}__state"][t0][None].copy(), device=env._dev)
            loop.set_plans(fx[f"{name}__p{k}__actions"][None], fx[f"{name}__p{k}__states"][None], iteration=t0)
            out.append((name, k, t0, loop.run(t1 - t0, z=_z(fx, name, t0, t1 - t0))))
        loop.close()
    return out


def test_follow_kernel_teacher_forced_segments(fx, segments):
    worst = 0.0
    for name, k, t0, g in segments:
        n = len(g["events"])
        sl = slice(t0, t0 + n)
        assert np.array_equal(g["events"][:, 0], fx[f"{name}__event"][sl].astype(np.int32)), (name, k)
        assert np.array_equal(_bits(g["actions"][:, 0]), _bits(fx[f"{name}__action"][sl])), (name, k)       # action_index, through the actions
        last = k + 1 == int(fx[f"{name}__n_plans"]) or not bool(fx[f"{name}__p{k + 1}__found"])
        want_status = int(fx[f"{name}__status"]) if last and int(fx[f"{name}__status"]) in (L.GOAL, L.TIME_LIMIT, L.PLAN_EXHAUSTED) else L.RUNNING
        assert int(g["status"][0]) == want_status, (name, k)
        if want_status != L.RUNNING:
            assert int(g["done_iter"][0]) == int(fx[f"{name}__done_iter"])
        flags = np.nonzero(g["events"][:, 0] == L.REPLAN)[0]
        if k + 1 < int(fx[f"{name}__n_plans"]):
            assert flags.tolist() == [n - 1], (name, k)                                                  # the replan iteration
        else:
            assert flags.size == 0
        ds = float(np.abs(g["states"][1:, 0] - fx[f"{name}__state"][t0 + 1:t0 + n + 1]).max())
        dr = float(np.nanmax(np.abs(g["rewards"][:, 0] - fx[f"{name}__reward"][sl])))
        assert np.array_equal(np.isnan(g["deviations"][:, 0]), np.isnan(fx[f"{name}__dev"][sl]))
        dd = float(np.nanmax(np.abs(g["deviations"][:, 0] - fx[f"{name}__dev"][sl])))
        print(f"{name} plan {k}: {n} iterations from {t0}: state {ds:.3e} reward {dr:.3e} deviation {dd:.3e}")
        worst = max(worst, ds, dr, dd)
    print(f"largest difference {worst:.3e}, asserted {FOLLOW_TOL:.1e}")
    assert worst <= FOLLOW_TOL


# ---- 2. the follow kernel against the spec on synthetic plans ------------------------------------------------------------------------
def _synthetic(fx):
    """B = 3: a straight plan of 9000 states (past the LDS budget) the rover stays on; a plan of 3 states; a plan 5 m off the track."""
    starts = np.float32([[6.0, 6.0], [10.0, 20.0], [20.0, 8.0]])
    goals = np.float32([[28.0, 28.0], [26.0, 20.0], [20.0, 26.0]])
    th = np.arctan2(goals[:, 1] - starts[:, 1], goals[:, 0] - starts[:, 0]).astype(np.float32)
    Ls = (8999, 2, 500)
    Lm = max(Ls)
    actions = np.zeros((3, Lm, 2), np.float32)
    states = np.zeros((3, Lm + 1, 3), np.float32)
    for b, Lb in enumerate(Ls):
        step = np.float32(0.002 if b == 0 else 0.05)
        d = np.arange(Lb + 1, dtype=np.float32) * step
        off = np.float32(5.0 if b == 2 else 0.0)
        states[b, :Lb + 1, 0] = starts[b, 0] + d * np.cos(th[b]) - off * np.sin(th[b])
        states[b, :Lb + 1, 1] = starts[b, 1] + d * np.sin(th[b]) + off * np.cos(th[b])
        states[b, :Lb + 1, 2] = th[b]
        actions[b, :Lb, 0] = np.float32(0.8)
    return starts, goals, actions, states, np.int32(Ls)


@pytest.fixture(scope="module")
def synthetic(fx):
    starts, goals, actions, states, Ls = _synthetic(fx)
    n = 8
    z = torch.from_numpy(np.random.default_rng(3).standard_normal((n, 3)).astype(np.float32))
    env, planner, loop = _make(fx, 3, 1.0, starts, goals, time_limit=0.5)
    runs = []
    for lds in (True, False):
        env.reset(seed=0)
        loop.set_plans(actions, states, Ls)
        runs.append(loop.run(n, z=z, samples=torch.zeros(0, 3, int(fx["params"][0]), 3), stage_in_lds=lds))
    s0 = env._initialize_robot_state().cpu().numpy()
    loop.close()
    return runs, (starts, goals, actions, states, Ls, z.numpy(), s0, n)


def test_follow_kernel_lds_and_global_paths_are_bit_identical(synthetic):
    (a, b), _ = synthetic
    assert _same_logs(a, b)


def test_follow_kernel_equals_the_spec_on_synthetic_plans(fx, synthetic):
    (g, _), (starts, goals, actions, states, Ls, z, s0, n) = synthetic
    from oracle import oracle as O
    MU = fx["mean"].astype(np.float32)
    SG = np.full_like(MU, float(fx["std"]))
    for b in range(3):
        p = O.make_params(1, 1, G, RES, goals[b], thr=THR, dt=float(fx["delta_t"]))
        rover = L.Rover(p, MU, SG, float(fx["goal_threshold"]), s0[b], lambda k, s: None, delta_t=float(fx["delta_t"]), time_limit=0.5)     # no table: every plan asked for is NO_PLAN
        rover.set_plan(actions[b, :Ls[b]], states[b, :Ls[b] + 1])
        want = rover.run(n, z[:, b])
        assert np.array_equal(g["events"][:, b], want["events"]), b
        assert (int(g["status"][b]), int(g["done_iter"][b])) == (rover.status, rover.done_iter), b
        assert np.array_equal(_bits(g["actions"][:, b]), _bits(want["actions"])), b
        assert np.abs(g["states"][:, b] - want["states"]).max() <= 1e-6 * n
        m = ~np.isnan(want["deviations"])
        assert np.array_equal(np.isnan(g["deviations"][:, b]), ~m) and (np.abs(g["deviations"][:, b][m] - want["deviations"][m]) <= 1e-6 * n).all()
    # the kinds this case is for
    assert int(g["status"][0]) == L.TIME_LIMIT and int(g["steps"][0]) == L.limit_steps(float(fx["delta_t"]), 0.5) == 6 and int(g["done_iter"][0]) == 5
    assert int(g["status"][1]) == L.PLAN_EXHAUSTED and int(g["done_iter"][1]) == 2
    assert g["events"][:3, 2].tolist() == [L.STEP, L.REPLAN, L.FROZEN] and int(g["status"][2]) == L.NO_PLAN and int(g["done_iter"][2]) == 2


# ---- 3. the fused loop, injected samples and z ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused(fx):
    out = {}
    N = int(fx["params"][3])
    for name in EPISODES:
        env, planner, loop = _make(fx, 1, float(fx[f"{name}__scale"]))
        tables = np.stack([fx[f"{name}__p{k}__samples"] for k in range(int(fx[f"{name}__n_plans"]))])[:, None]
        g = loop.run(N, z=_z(fx, name, 0, N), samples=torch.from_numpy(tables.copy()))
        out[name] = (g, loop)
    return out


@pytest.mark.parametrize("name", EPISODES)
def test_fused_loop_reproduces_the_reference_episode(fx, fused, name):
    g, loop = fused[name]
    assert np.allclose(loop._goal_nodes[0], fx[f"{name}__goal_node"], atol=1e-6)
    assert int(g["plans"][0]) == int(fx[f"{name}__n_plans"])
    assert np.array_equal(g["events"][:, 0], fx[f"{name}__event"].astype(np.int32))
    assert np.array_equal(g["plan_index"][:, 0], fx[f"{name}__plan_idx"])
    assert (np.nonzero(g["events"][:, 0] == L.REPLAN)[0] + 1).tolist() == fx[f"{name}__plan_iter"][1:].tolist()
    assert (int(g["status"][0]), int(g["done_iter"][0])) == (int(fx[f"{name}__status"]), int(fx[f"{name}__done_iter"]))
    ds = float(np.abs(g["states"][:, 0] - fx[f"{name}__state"]).max())
    print(f"{name}: free-running state difference {ds:.3e}")
    assert ds <= STATE_TOL


def test_raise_for_status_raises_for_the_no_plan_rover(fused):
    with pytest.raises(TypeError, match="None"):
        fused["s04"][1].raise_for_status()
    fused["s10"][1].raise_for_status()                       # GOAL is a regular end


# ---- 4. masks and batches ------------------------------------------------------------------------------------------------------------
STARTS3 = np.float32([[8.0, 8.0], [6.0, 12.0], [12.0, 5.0]])
SEEDS3 = [5, 6, 7]
N4 = 1000


@pytest.fixture(scope="module")
def batch(fx):
    z = torch.from_numpy(np.random.default_rng(11).standard_normal((N4, 3)).astype(np.float32))
    env, planner, loop = _make(fx, 3, 1.4, STARTS3, None, SEEDS3)
    return env, loop, z, loop.run(N4, z=z)


def test_batch_equals_single_runs(fx, batch):
    env, loop, z, g = batch
    assert (g["plans"] >= 2).any(), "the case is for replans"
    for b in range(3):
        _, _, one = _make(fx, 1, 1.4, STARTS3[b:b + 1], None, SEEDS3[b:b + 1])
        s = one.run(N4, z=z[:, b:b + 1].contiguous())
        one.close()
        for k in g:
            assert np.array_equal(_bits(np.ascontiguousarray(g[k][:, b] if g[k].ndim > 1 else g[k][b:b + 1])),
                                  _bits(np.ascontiguousarray(s[k][:, 0] if s[k].ndim > 1 else s[k]))), (b, k)


def test_two_runs_equal_one_and_reset_resets(fx, batch):
    env, loop, z, g = batch
    env.reset(seed=0)                                         # also resets the loop
    assert loop._iters == 0 and not loop.status.any()
    a = loop.run(N4 // 2, z=z[:N4 // 2])
    b = loop.run(N4 - N4 // 2, z=z[N4 // 2:])
    for k in ("rewards", "actions", "deviations", "plan_index", "events"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(g[k])), k
    assert np.array_equal(_bits(np.concatenate([a["states"], b["states"][1:]])), _bits(g["states"]))
    for k in ("done_iter", "status", "plans", "steps"):
        assert np.array_equal(b[k], g[k]), k
    assert np.allclose(loop.elapsed, g["steps"] * float(fx["delta_t"]))


def test_inactive_rover_keeps_every_byte(fx, batch):
    from benchnav_amd import _capi
    env, loop, z, g = batch
    pi = g["plan_index"]
    # an iteration at which one rover takes a new plan and another does not
    pick = next(((t, b, o) for t in range(1, N4) for b in range(3) for o in range(3)
                 if o != b and pi[t, b] > pi[t - 1, b] and pi[t, o] == pi[t - 1, o] and g["events"][t, o] == L.STEP), None)
    assert pick is not None
    t, b, o = pick
    env.reset(seed=0)
    loop.run(t, z=z[:t])                                      # rover b was flagged by iteration t - 1; nothing has been asked for yet
    h = loop._handle
    it, S, cap, pc = h.iters, h.S, h.iters + 1, h.path_cap
    B = 3
    bufs = [(_capi.BN_CLRRT_BUF_NODES, (B, cap * 3), "<f4"), (_capi.BN_CLRRT_BUF_EDGES, (B, cap), "<i4"), (_capi.BN_CLRRT_BUF_COSTS, (B, cap), "<f4"),
            (_capi.BN_CLRRT_BUF_COUNTS, (B, 1), "<i4"), (_capi.BN_CLRRT_BUF_SEQ_LENGTHS, (B, cap), "<i4"), (_capi.BN_CLRRT_BUF_CONTROLLERS, (B, cap * 4), "<f4"),
            (_capi.BN_CLRRT_BUF_ACTION_SEQS, (B, cap * S * 2), "<f4"), (_capi.BN_CLRRT_BUF_STATE_SEQS, (B, cap * (S + 1) * 3), "<f4"),
            (_capi.BN_CLRRT_BUF_SAMPLES, (B, it * 3), "<f4"), (_capi.BN_CLRRT_BUF_PATH_ACTIONS, (B, pc * 2), "<f4"),
            (_capi.BN_CLRRT_BUF_PATH_STATES, (B, (pc + 1) * 3), "<f4"), (_capi.BN_CLRRT_BUF_RESULTS, (B, 6), "<i4"),
            (_capi.BN_CLRRT_BUF_MT_STATE, (B, 624), "<i4"), (_capi.BN_CLRRT_BUF_MT_POS, (B, 1), "<i4")]
    snap = lambda: [loop.buffer(w, shp, ty).view(torch.int32).cpu().numpy().copy() for w, shp, ty in bufs]
    before = snap()
    one = loop.run(1, z=z[t:t + 1])
    after = snap()
    assert int(one["plans"][b]) == int(pi[t, b]) + 1 and int(one["plans"][o]) == int(pi[t, o]) + 1 == int(pi[t - 1, o]) + 1
    for (w, _, _), x, y in zip(bufs, before, after):
        assert np.array_equal(x[o], y[o]), f"buffer {w}: the inactive rover's bytes changed"
    changed = [w for (w, _, _), x, y in zip(bufs, before, after) if not np.array_equal(x[b], y[b])]
    assert _capi.BN_CLRRT_BUF_MT_STATE in changed or _capi.BN_CLRRT_BUF_MT_POS in changed, "the replanning rover's stream did not advance"
    assert _capi.BN_CLRRT_BUF_PATH_STATES in changed


def test_run_refuses_another_planner_handle_and_set_plans_keeps_the_counters_together(fx):
    import ctypes as C
    from benchnav_amd import _capi
    from benchnav_amd.clrrt import _Handle
    env, planner, loop = _make(fx, 1, 1.0)
    other = _Handle(loop._lib, loop._dev, 1, planner)
    state = env._robot_state.clone()
    rc = loop._lib.bn_clrrt_loop_run(loop._h, other.h, 1, C.c_void_p(state.data_ptr()), None, None, 0, 0, None)
    assert rc == _capi.BN_ERR_INVALID and b"bn_clrrt_loop_reset was given" in loop._lib.bn_last_error()
    loop.set_plans(fx["s10__p0__actions"][None], fx["s10__p0__states"][None], iteration=7)
    assert (loop._iters, env._steps, env._draws) == (7, 7, 7)
    loop.run(3)
    assert (loop._iters, env._steps, env._draws) == (10, 10, 10)
    other.close()
    loop.close()
