"""GPU: per-rover risk maps in the CL-RRT handle (bn_clrrt_set_instance_maps) and the loop's device views, held bit for bit to code
that was there before them: a handle whose instances plan on one map each against single-instance planners constructed on those
maps.

1. plan_batch and steer_batch with `risk_maps`: B = 3 instances with the SAME start, goal and seed on three maps -- the loop
   fixture's map (tests/golden/clrrt_loop.npz) scaled by three factors, one with a block of risk 1 between start and goal --
   against three B = 1 planners; at least two instances' paths differ, so a handle that read map 0 for everyone cannot pass.
2. plan_batch without `risk_maps` behind one with it: the bits of a fresh planner.
3. CLRRTLoop with per-rover maps, injected z, seeds (5, 6, 7), 1000 iterations, against three B = 1 loops on their maps.
4. run(n, log=False) + episode_buffers(): the views are the arrays run(n) downloads, and the done_step / stopped words are
   benchmark.clrrt_outcome_words of the downloaded status, for a batch with a GOAL, a TIME_LIMIT and a NO_PLAN rover."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G, RES, THR = 64, 0.5, 0.2
SCALES = (1.0, 1.3, 0.8)                       # of the fixture's map; the third carries the block
START = np.float32([8.0, 8.0, 0.7853982])
GOAL = np.float32([24.0, 24.0])
SEED = 42


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "clrrt_loop.npz"))


@pytest.fixture(scope="module")
def maps(fx):
    """(3, G, G): the fixture's map times SCALES, the last with risk 1 on the 4 m square around (16, 16), half way to the goal."""
    m = np.stack([np.clip(fx["mean"] * np.float32(s), 0.0, 0.95) for s in SCALES]).astype(np.float32)
    m[2, 28:36, 28:36] = 1.0
    m.setflags(write=False)
    return m


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint8)


def _planner(fx, risk, **kw):
    from benchnav_amd import CLRRT
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    gm = FakeGridMap(G, RES)
    iters, max_seqs, _, _ = (int(v) for v in fx["params"])
    kw.setdefault("max_iterations", iters)
    return CLRRT(3, 2, FakeDynamics(np.array(risk), gm), FakeObjectives(torch.as_tensor(fx["goal"].copy()), THR), gm, delta_t=float(fx["delta_t"]),
                 max_seqs=max_seqs, seed=SEED, **kw)


def _exposed(pl, ret, b):
    """What plan_batch exposes of instance b, as bytes: the returned sequences, the tree (its n nodes: nodes, edges, costs, sequence
    lengths, controllers, action and state sequences), the iteration log, the result row and the path buffers in full."""
    from benchnav_amd import _capi
    actions, states, lengths, found = ret
    h = pl._last_handle
    t = pl.batch_tree(b)
    n = t.nodes_count
    L = int(lengths[b])
    out = {"length": L, "found": bool(found[b]), "n": n, "actions": _bits(actions[b, :L]), "states": _bits(states[b, :L + 1])}
    for k in ("nodes", "edges", "costs", "seq_lengths", "controllers_states", "action_seqs", "state_seqs"):
        out[k] = _bits(getattr(t, k)[:n])
    for k in ("near_goal_counts", "picks", "node_counts", "nearest", "feasible"):
        out[k] = _bits(pl.last_batch[k][b])
    out["results"] = _bits(h.buffer(_capi.BN_CLRRT_BUF_RESULTS, (h.B, 6), "<i4")[b])
    out["path_actions"] = _bits(h.buffer(_capi.BN_CLRRT_BUF_PATH_ACTIONS, (h.B, h.path_cap, 2))[b])
    out["path_states"] = _bits(h.buffer(_capi.BN_CLRRT_BUF_PATH_STATES, (h.B, h.path_cap + 1, 3))[b])
    out["samples"] = _bits(pl.sample_table()[0][b])
    return out


def _assert_same(got, want, ctx):
    assert got.keys() == want.keys()
    for k in got:
        assert np.array_equal(got[k], want[k]), (ctx, k)


@pytest.fixture(scope="module")
def singles(fx, maps):
    """Instance b's plan by a B = 1 planner constructed on map b: the code as it was before per-instance maps."""
    out = []
    for b in range(3):
        pl = _planner(fx, maps[b])
        ret = pl.plan_batch(START[None], GOAL[None], [SEED])
        out.append(_exposed(pl, ret, 0))
    return out


# ---- 1. a batch on three maps equals three single-map planners ---------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host", "numpy"])
def test_plan_batch_on_three_maps_equals_three_single_map_planners(fx, maps, singles, where):
    pl = _planner(fx, maps[0])
    rm = {"device": lambda: torch.from_numpy(maps.copy()).cuda(), "host": lambda: torch.from_numpy(maps.copy()), "numpy": lambda: maps}[where]()
    ret = pl.plan_batch(np.repeat(START[None], 3, 0), np.repeat(GOAL[None], 3, 0), [SEED] * 3, risk_maps=rm)
    got = [_exposed(pl, ret, b) for b in range(3)]
    for b in range(3):
        _assert_same(got[b], singles[b], f"instance {b}, maps from {where}")
    # same start, goal and samples: only the maps tell the instances apart
    assert np.array_equal(got[0]["samples"], got[1]["samples"]) and np.array_equal(got[0]["samples"], got[2]["samples"])
    found = [g["found"] for g in got]
    paths = [g["path_states"].tobytes() for g in got]
    print(f"found {found}, lengths {[g['length'] for g in got]}, nodes {[g['n'] for g in got]}")
    assert sum(found) >= 2, "the case needs two paths to compare"
    assert any(found[a] and found[b] and paths[a] != paths[b] for a in range(3) for b in range(a + 1, 3)), "every instance planned the same path"
    assert len({g["state_seqs"].tobytes() for g in got}) == 3, "three maps, three trees"


def test_grow_from_samples_takes_the_maps_too(fx, maps, singles):
    pl = _planner(fx, maps[0])
    one = _planner(fx, maps[2])
    samples = torch.from_numpy(np.frombuffer(singles[0]["samples"].tobytes(), np.float32).reshape(1, -1, 3).copy())
    ret = pl.grow_from_samples(np.repeat(START[None], 3, 0), samples.repeat(3, 1, 1), np.repeat(GOAL[None], 3, 0), risk_maps=maps)
    want = one.grow_from_samples(START[None], samples, GOAL[None])
    a, b = _exposed(pl, ret, 2), _exposed(one, want, 0)
    for k in ("nodes", "edges", "costs", "action_seqs", "state_seqs", "path_states", "results"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["state_seqs"], singles[2]["state_seqs"])            # the stream's samples again


def test_steer_batch_on_three_maps_equals_three_single_map_planners(fx, maps):
    f = np.float32([[8.0, 8.0, 0.3]] * 3)
    c = np.float32([[0.1, 0.02, -0.05, 0.01]] * 3)
    t = np.float32([[13.0, 11.0, 1.2]] * 3)
    pl = _planner(fx, maps[0])
    got = pl.steer_batch(f, c, t, risk_maps=torch.from_numpy(maps.copy()).cuda())
    for b in range(3):
        want = _planner(fx, maps[b]).steer_batch(f[b:b + 1], c[b:b + 1], t[b:b + 1])
        for k in got:
            assert np.array_equal(_bits(got[k][b]), _bits(want[k][0])), (b, k)
    assert not np.array_equal(_bits(got["states"][0]), _bits(got["states"][1])), "two maps, one closed-loop trajectory"
    # ... and without the maps the handle steers on the planner's own map again
    back = pl.steer_batch(f, c, t)
    want = _planner(fx, maps[0]).steer_batch(f, c, t)
    for k in ("feasible", "length", "word", "points", "cost", "controllers", "path"):
        assert np.array_equal(_bits(back[k]), _bits(want[k])), k
    for b in range(3):                                     # (behind a steer's length its rows keep what the previous steer wrote)
        n = int(want["length"][b])
        assert np.array_equal(_bits(back["actions"][b, :n]), _bits(want["actions"][b, :n])), b
        assert np.array_equal(_bits(back["states"][b, :n + 1]), _bits(want["states"][b, :n + 1])), b


# ---- 2. back to the shared map ---------------------------------------------------------------------------------------------------------
def test_plan_batch_without_maps_after_one_with_maps_is_a_fresh_planners(fx, maps):
    starts, goals, seeds = np.repeat(START[None], 3, 0), np.repeat(GOAL[None], 3, 0), [SEED, 7, 9]
    pl = _planner(fx, maps[1])
    pl.plan_batch(starts, goals, seeds, risk_maps=maps)
    ret = pl.plan_batch(starts, goals, seeds)
    fresh = _planner(fx, maps[1])
    want = fresh.plan_batch(starts, goals, seeds)
    for b in range(3):
        _assert_same(_exposed(pl, ret, b), _exposed(fresh, want, b), f"instance {b}")


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------
STARTS3 = np.float32([[8.0, 8.0], [6.0, 12.0], [12.0, 5.0]])
SEEDS3 = [5, 6, 7]
N_LOOP = 1000


def _loop(fx, B, starts, goals, planner_map, seeds, risk_maps=None, time_limit=None, scale=1.4):
    from benchnav_amd import CLRRTLoop, NativeMPPI
    from benchnav_amd.env import BatchedPlanetaryEnv
    pl = NativeMPPI(horizon=8, num_samples=64, grid_size=G, resolution=RES, num_instances=B, shared_map=True, stream=0, stuck_threshold=THR)
    lat = np.clip(fx["mean"] * np.float32(scale), 0.0, 0.7).astype(np.float32)
    env = BatchedPlanetaryEnv(pl, lat, np.full((G, G), float(fx["std"]), np.float32), np.asarray(starts, np.float32), np.asarray(goals, np.float32),
                              delta_t=float(fx["delta_t"]), time_limit=float(fx["time_limit"]) if time_limit is None else time_limit,
                              stuck_threshold=THR, goal_threshold=float(fx["goal_threshold"]), seed=1)
    loop = CLRRTLoop(env, _planner(fx, planner_map), seeds=seeds, risk_maps=risk_maps)
    env.reset(seed=0)
    return env, loop


def test_loop_on_per_rover_maps_equals_single_loops_on_their_maps(fx, maps):
    z = torch.from_numpy(np.random.default_rng(11).standard_normal((N_LOOP, 3)).astype(np.float32))
    goals = np.repeat(fx["goal"][None], 3, 0)
    env, loop = _loop(fx, 3, STARTS3, goals, maps[0], SEEDS3, risk_maps=torch.from_numpy(maps.copy()).cuda())
    g = loop.run(N_LOOP, z=z)
    loop.close()
    print(f"status {g['status'].tolist()} plans {g['plans'].tolist()} steps {g['steps'].tolist()}")
    assert (g["plans"] >= 2).any(), "the case is for replans"
    for b in range(3):
        _, one = _loop(fx, 1, STARTS3[b:b + 1], goals[b:b + 1], maps[b], SEEDS3[b:b + 1])
        s = one.run(N_LOOP, z=z[:, b:b + 1].contiguous())
        one.close()
        for k in g:
            assert np.array_equal(_bits(g[k][:, b] if g[k].ndim > 1 else g[k][b:b + 1]), _bits(s[k][:, 0] if s[k].ndim > 1 else s[k])), (b, k)


def test_set_risk_maps_between_episodes_changes_the_maps_without_a_new_handle(fx, maps):
    z = torch.from_numpy(np.random.default_rng(12).standard_normal((60, 2)).astype(np.float32))
    goals = np.repeat(fx["goal"][None], 2, 0)
    env, loop = _loop(fx, 2, STARTS3[:2], goals, maps[0], SEEDS3[:2])
    handle = loop._handle.h.value
    runs = []
    for rm in (None, maps[[2, 1]], None, maps[[2, 1]]):
        loop.set_risk_maps(rm)
        env.reset(seed=0)
        runs.append(loop.run(60, z=z))
    assert loop._handle.h.value == handle
    loop.close()
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[2][k])) and np.array_equal(_bits(runs[1][k]), _bits(runs[3][k])), k
    assert not np.array_equal(_bits(runs[0]["states"]), _bits(runs[1]["states"])), "the maps changed nothing"


# ---- 4. the device views -----------------------------------------------------------------------------------------------------------------
def test_episode_buffers_are_the_downloaded_log_and_the_outcome_words(fx):
    """Three rovers on installed plans and no sample table (every plan asked for is NO_PLAN), a 2 s limit (20 steps): a goal 1.3 m
    ahead on a straight plan (GOAL), a far goal on a long straight plan (TIME_LIMIT), a plan 5 m beside the rover (a replan is
    flagged on iteration 1: NO_PLAN)."""
    from benchnav_amd import _capi
    from benchnav_amd.benchmark import clrrt_outcome_words, max_steps
    starts = np.float32([[8.0, 8.0], [10.0, 20.0], [20.0, 8.0]])
    goals = np.float32([[9.3, 8.0], [26.0, 20.0], [20.0, 26.0]])
    th = np.arctan2(goals[:, 1] - starts[:, 1], goals[:, 0] - starts[:, 0]).astype(np.float32)
    L, n = 400, 50
    d = np.arange(L + 1, dtype=np.float32) * np.float32(0.05)
    states = np.zeros((3, L + 1, 3), np.float32)
    actions = np.zeros((3, L, 2), np.float32)
    for b in range(3):
        off = np.float32(5.0 if b == 2 else 0.0)
        states[b, :, 0] = starts[b, 0] + d * np.cos(th[b]) - off * np.sin(th[b])
        states[b, :, 1] = starts[b, 1] + d * np.sin(th[b]) + off * np.cos(th[b])
        states[b, :, 2] = th[b]
        actions[b, :, 0] = 1.0
    z = torch.from_numpy(np.random.default_rng(4).standard_normal((n, 3)).astype(np.float32))
    none = torch.zeros(0, 3, int(fx["params"][0]), 3)
    env, loop = _loop(fx, 3, starts, goals, fx["mean"], SEEDS3, time_limit=2.0, scale=1.0)
    loop.set_plans(actions, states)
    assert loop.run(n, z=z, samples=none, log=False) is None
    assert not loop.status.any(), "log=False leaves the host words alone"
    sp, rp, dp, tp, n_got, cap = loop.episode_buffers()
    assert n_got == n and cap >= n
    view = lambda p, shape, ty="<f4": loop._handle.view(p, shape, ty).cpu().numpy()
    got = {"states": view(sp, (cap + 1, 3, 3))[:n + 1], "rewards": view(rp, (cap, 3))[:n], "done_step": view(dp, (3,), "<i4"),
           "stopped": view(tp, (3,), "<i4")}
    status_dev, plans_dev = (t.cpu().numpy() for t in loop.rover_buffers())
    assert (env._steps, loop._iters) == (n, n)
    env.reset(seed=0)
    loop.set_plans(actions, states)
    want = loop.run(n, z=z, samples=none)
    loop.close()
    print(f"status {want['status'].tolist()} done_iter {want['done_iter'].tolist()} steps {want['steps'].tolist()}")
    assert want["status"].tolist() == [_capi.BN_CL_GOAL, _capi.BN_CL_TIME_LIMIT, _capi.BN_CL_NO_PLAN]
    assert int(want["steps"][1]) == max_steps(2.0, float(fx["delta_t"])) == 20 and int(want["done_iter"][2]) == 2
    assert np.array_equal(_bits(got["states"]), _bits(want["states"])) and np.array_equal(_bits(got["rewards"]), _bits(want["rewards"]))
    done_step, stopped = clrrt_outcome_words(want["status"], want["done_iter"])
    assert np.array_equal(got["done_step"], done_step) and np.array_equal(got["stopped"], stopped)
    assert got["done_step"].tolist() == [int(want["done_iter"][0]), -1, -1] and got["stopped"].tolist() == [0, 0, _capi.BN_CL_NO_PLAN]
    assert np.array_equal(status_dev, want["status"]) and np.array_equal(plans_dev, want["plans"])
