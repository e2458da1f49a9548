"""GPU: Benchmark.run("cl_rrt") -- a CL-RRT campaign (per-rover risk maps set device to device, CLRRTLoop.run(log=False), scores from
the loop's device views) against the same chunks composed by hand from what the package had before it: infer_risk_map per map, a
CLRRT built the reference's way, one CLRRTLoop per setting on its rovers' maps, the host log of loop.run, and the NumPy spec of
tests/benchmark_spec.py fed with benchmark.clrrt_outcome_words.

The problem is test_gpu_campaign.py's: three seeded 64 x 64 maps at 0.5 m per cell, the latent model as the prediction, trials = 2
and chunk = 4 (six episodes: a full chunk and a short one), three settings, a 2 s time limit (20 control steps, 40 loop
iterations).  Maps 0 and 2 have their goals 1.3 m ahead of a start with heading 0, map 1 has its goal 22 m away.  The planner runs
the loop fixture's parameters (60 samples per plan, 250 closed-loop steps per steer).

Bounds: outcome, steps, time, reward_min, stuck_steps and plans are exact; path_length, reward_sum and final_distance lie within
benchmark_spec.metric_bound(value, rows, 1), rows = 40 log rows (test_gpu_scores.py cites where the square root's bound comes from)."""
import functools

import numpy as np
import pytest

import benchmark_spec as S

f32 = np.float32
pytestmark = pytest.mark.gpu

G, RES, M = 64, 0.5, 3
TRIALS, CHUNK, SEED, NUM_SAMPLES = 2, 4, 5, 200
DT, LIMIT, THR, GOAL_THR = 0.1, 2.0, 0.1, 1.0
SETTINGS = ["expected_value", "var@0.9", "cvar@0.9"]
PAIRS = [("expected_value", None), ("var", 0.9), ("cvar", 0.9)]
STARTS = f32([[8.0, 8.0], [8.0, 8.0], [16.0, 10.0]])
GOALS = f32([[9.3, 8.0], [24.0, 24.0], [16.0, 11.3]])
CL_KW = dict(max_iterations=60, max_seqs=250)
EXACT = ("outcome", "steps", "time", "reward_min", "stuck_steps")
BOUNDED = ("path_length", "reward_sum", "final_distance")
U_SQRT = 1
STEPS, ROWS = 20, 40


@functools.lru_cache(maxsize=None)
def _latent(blocked_map=None):
    from benchnav_amd import synth
    mean = np.stack([(f32(0.3) + f32(0.2) * synth.smooth_risk_map(G, 100 + m).numpy() / f32(0.95)).astype(f32) for m in range(M)])
    std = np.full((M, G, G), 0.03, f32)
    if blocked_map is not None:                    # the start cell of that map slips fully (test_gpu_campaign.py)
        ix, iy = int(STARTS[blocked_map][0] / RES), int(STARTS[blocked_map][1] / RES)
        mean[blocked_map, iy, ix], std[blocked_map, iy, ix] = 1.0, 1e-4
    mean.setflags(write=False); std.setflags(write=False)
    return mean, std


def _dataset(blocked_map=None):
    import torch
    from benchnav_amd.dataset import TerrainDataset
    mean, std = _latent(blocked_map)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    zeros = torch.zeros(M, G, G, device="cuda")
    return TerrainDataset(zeros.clone(), zeros.clone(), dev(mean), dev(std), torch.zeros(M, 3, G, G, device="cuda"),
                          torch.zeros(M, G, G, dtype=torch.int32, device="cuda"), seeds=list(range(M)))


def _run(blocked_map=None, starts=STARTS, goals=GOALS):
    from benchnav_amd.benchmark import Benchmark
    bench = Benchmark(_dataset(blocked_map), None, start_pos=starts, goal_pos=goals, delta_t=DT, time_limit=LIMIT, stuck_threshold=THR,
                      goal_threshold=GOAL_THR, trials=TRIALS, chunk=CHUNK, seed=SEED, num_samples=NUM_SAMPLES, resolution=RES)
    return bench.run("cl_rrt", SETTINGS, **CL_KW)


@functools.lru_cache(maxsize=None)
def _report():
    return _run()


@functools.lru_cache(maxsize=None)
def _oracle():
    """The campaign by hand: {field: (C, M, trials)} from host logs and the NumPy spec, and the loops' status words."""
    import torch
    from benchnav_amd import CLRRT, CLRRTLoop, NativeMPPI
    from benchnav_amd.benchmark import clrrt_iterations, clrrt_outcome_words, planner_seed
    from benchnav_amd.env import BatchedPlanetaryEnv
    from benchnav_amd.risk import infer_risk_map
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    mean, std = _latent()
    assert S.max_steps(LIMIT, DT) == STEPS and clrrt_iterations(STEPS) == ROWS
    E = M * TRIALS
    mean, std = mean.copy(), std.copy()
    risk = np.stack([np.stack([infer_risk_map(torch.from_numpy(mean[m]), torch.from_numpy(std[m]), metric, q, num_samples=NUM_SAMPLES,
                                              seed=(SEED + m) % 2 ** 64).cpu().numpy() for m in range(M)]) for metric, q in PAIRS])
    out = {k: [[None] * E for _ in PAIRS] for k in S.FIELDS + ("plans", "status")}
    gm = FakeGridMap(G, RES)
    rrt = CLRRT(3, 2, FakeDynamics(np.zeros((G, G), f32), gm), FakeObjectives(torch.zeros(2), THR), gm, delta_t=DT, goal_threshold=GOAL_THR,
                seed=SEED, **CL_KW)
    for j in range((E + CHUNK - 1) // CHUNK):
        e0 = j * CHUNK
        B = min(CHUNK, E - e0)
        maps = [(e0 + i) // TRIALS for i in range(B)]
        with NativeMPPI(grid_size=G, resolution=RES, num_instances=B, shared_map=False, stuck_threshold=THR,
                        stream=torch.cuda.current_stream().cuda_stream, horizon=8, num_samples=64) as pl:
            env = BatchedPlanetaryEnv(pl, mean[maps], std[maps], STARTS[maps], GOALS[maps], delta_t=DT, time_limit=LIMIT, stuck_threshold=THR,
                                      goal_threshold=GOAL_THR, seed=(SEED + j) % 2 ** 64, freeze_on_goal=True)
            for c in range(len(PAIRS)):
                loop = CLRRTLoop(env, rrt, seeds=[planner_seed(SEED, e0 + i) for i in range(B)], risk_maps=risk[c, maps])
                env.reset(seed=(SEED + j) % 2 ** 64)
                log = loop.run(ROWS)
                loop.close()
                done, stopped = clrrt_outcome_words(log["status"], log["done_iter"])
                got = S.score_episodes(log["states"], log["rewards"], GOALS[maps], None, done, stopped, None, THR, DT)
                got["plans"], got["status"] = log["plans"], log["status"]
                for k in out:
                    out[k][c][e0:e0 + B] = list(got[k])
    return {k: np.array(v).reshape(len(PAIRS), M, TRIALS) for k, v in out.items()}


def _compare(report, want, ctx):
    for k in EXACT + ("plans",):
        got, ref = getattr(report, k), want[k]
        same = (got == ref) | ((got != got) & (ref != ref))
        assert same.all(), f"{ctx}: {k}: {got[~same]} vs {ref[~same]}"
    for k in BOUNDED:
        got, ref = getattr(report, k), want[k]
        assert (np.abs(got - ref) <= S.metric_bound(ref, ROWS, U_SQRT)).all(), f"{ctx}: {k}: {got} vs {ref}"


def test_report_equals_the_hand_composed_campaign():
    from benchnav_amd import _capi
    want = _oracle()
    print(f"\noracle: outcomes {want['outcome'].tolist()} status {want['status'].tolist()} steps {want['steps'].tolist()} plans {want['plans'].tolist()}")
    outcomes = set(want["outcome"].ravel().tolist())
    assert S.GOAL in outcomes and S.TIME_LIMIT in outcomes, f"the inputs must reach a goal and a time limit, got {want['outcome'].tolist()}"
    assert (want["status"] != _capi.BN_CL_RUNNING).all(), "40 iterations end every rover"
    rep = _report()
    assert (rep.planner, rep.seed, rep.chunk, rep.trials, rep.max_steps) == ("cl_rrt", SEED, CHUNK, TRIALS, STEPS)
    assert rep.outcome.shape == (len(SETTINGS), M, TRIALS) and rep.outcome.dtype == np.int32 and rep.time.dtype == np.float64
    assert rep.plans.shape == (len(SETTINGS), M, TRIALS) and rep.plans.dtype == np.int32 and (rep.plans >= 1).all()
    _compare(rep, want, "cl_rrt")
    print(f"cl_rrt: outcomes {rep.outcome.tolist()} steps {rep.steps.tolist()} plans {rep.plans.tolist()}\n{rep.table()}")
    assert (rep.steps <= STEPS).all() and (rep.steps[rep.outcome == S.TIME_LIMIT] == STEPS).all()
    rows = rep.summary()
    assert [r["setting"] for r in rows] == SETTINGS
    for c, r in enumerate(rows):
        oc = want["outcome"][c].ravel()
        assert r["valid"] == M * TRIALS and r["counts"]["GOAL"] == int((oc == S.GOAL).sum())
        assert r["counts"]["STOPPED"] == int((oc == S.STOPPED).sum())


def test_two_runs_are_bit_identical(tmp_path):
    import json
    a, b = _report(), _run()
    for k in S.FIELDS + ("plans",):
        assert np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)), k
    path = tmp_path / "report.json"
    b.to_json(str(path))
    back = json.loads(path.read_text())
    assert (back["planner"], back["seed"], back["chunk"], back["trials"], back["settings"]) == ("cl_rrt", SEED, CHUNK, TRIALS, SETTINGS)
    assert back["episodes"]["steps"] == a.steps.tolist() and back["episodes"]["plans"] == a.plans.tolist()


def test_an_untraversable_start_is_invalid_and_touches_no_other_episode():
    from benchnav_amd.benchmark import INVALID
    base, rep = _report(), _run(blocked_map=1)
    assert (rep.outcome[:, 1] == INVALID).all() and (rep.outcome[:, [0, 2]] != INVALID).all()
    for k in S.FIELDS + ("plans",):                    # maps 0 and 2 share chunks with map 1's episodes: their rows keep their bits
        assert np.array_equal(getattr(rep, k)[:, [0, 2]].view(np.uint8), getattr(base, k)[:, [0, 2]].view(np.uint8)), k
    for r in rep.summary():
        assert r["valid"] == 2 * TRIALS and r["counts"]["INVALID"] == TRIALS


def test_a_rover_that_cannot_plan_is_stopped_alone():
    """Map 1's goal 0.5 m from its start: the start node is the cheapest node within the goal threshold, forward() has no sequence
    to return (the reference raises there), the rover stops at iteration 0 and its chunk neighbours do not notice."""
    from benchnav_amd.benchmark import STOPPED
    goals = GOALS.copy()
    goals[1] = (8.5, 8.0)
    base, rep = _report(), _run(goals=goals)
    assert (rep.outcome[:, 1] == STOPPED).all() and (rep.steps[:, 1] == 0).all() and (rep.time[:, 1] == 0.0).all()
    assert (rep.final_distance[:, 1] == 0.5).all() and np.isnan(rep.reward_min[:, 1]).all() and (rep.plans[:, 1] == 1).all()
    for k in S.FIELDS + ("plans",):
        assert np.array_equal(getattr(rep, k)[:, [0, 2]].view(np.uint8), getattr(base, k)[:, [0, 2]].view(np.uint8)), k
    assert all(r["counts"]["STOPPED"] >= TRIALS for r in rep.summary())


def test_unknown_planner_keywords_are_refused():
    from benchnav_amd.benchmark import Benchmark
    bench = Benchmark(_dataset(), None, start_pos=STARTS, goal_pos=GOALS, delta_t=DT, time_limit=LIMIT, trials=1, chunk=CHUNK, resolution=RES)
    with pytest.raises(TypeError, match="horizon"):
        bench.run("cl_rrt", SETTINGS[:1], horizon=10)
