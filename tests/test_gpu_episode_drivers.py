"""GPU: what the closed loops share (benchnav_amd/_episodes.py: EpisodeLoop) and the episode drivers of Benchmark.run
(benchnav_amd/benchmark.py), on the smallest fixtures of the loops' own tests -- the "smooth" case of test_gpu_astar_dwa.py and the
map of test_gpu_clrrt_loop.py -- with B = 2 rovers and n = 3 rows.

1. the environment's counters after a run, per loop, with the log and without it (the table in EpisodeLoop._advance), and the
   environment's state against the log's last row, bit for bit;
2. the one-driver guard and the shape check of injected slip draws, with each loop's own text;
3. CLRRTLoop as a context manager;
4. the three drivers on one chunk of test_gpu_campaign.py's problem: score_inputs() and words() against the objects they wrap."""
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_astar_dwa as A
import test_gpu_campaign as T
import test_gpu_clrrt_loop as CL
from astar_dwa_scenarios import case as _case

pytestmark = pytest.mark.gpu

B, N = 2, 3
STARTS = np.float32([[5.0, 6.0], [6.0, 5.0]])


def _astar_dwa():
    heights, risk, _, goal, kw = _case("smooth")
    pl, env = A._env(B, risk, STARTS, np.float32([goal, goal]), **kw)
    loop = A._loop(env, heights, risk)
    env.reset()
    return env, loop


def _clrrt():
    fx = np.load(os.path.join(CL.HERE, "golden", "clrrt_loop.npz"))
    env, _, loop = CL._make(fx, B, 1.0, CL.STARTS3[:B], None, CL.SEEDS3[:B])
    return env, loop


def _last_row(loop, n):
    """The last state row of the latest run's device log (AStarDWALoop is a Handle itself, CLRRTLoop owns one)."""
    owner = loop if hasattr(loop, "view") else loop._handle
    return owner.view(loop.episode_buffers()[0], (n + 1, B, 3))[-1]


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)).view(np.uint32)


def test_astar_dwa_run_moves_the_counters_as_env_run_does():
    env, loop = _astar_dwa()
    dt = env._delta_t
    assert (env._steps, env._draws, env._elapsed_time) == (0, 0, 0.0)
    states = loop.run(N)[0]
    assert (env._steps, env._draws, env._elapsed_time) == (N, 0, 0.0 + N * dt)
    assert np.array_equal(_bits(env._robot_state), _bits(states[-1]))
    assert loop.run(N, log=False) is None                                  # continues the episode
    assert (env._steps, env._draws, env._elapsed_time) == (2 * N, 0, (0.0 + N * dt) + N * dt)
    assert loop.episode_buffers()[4] == N
    assert np.array_equal(_bits(env._robot_state), _bits(_last_row(loop, N)))
    loop.close()


def test_clrrt_run_counts_draws_and_takes_its_time_from_the_rovers_steps():
    env, loop = _clrrt()
    dt = env._delta_t
    assert (env._steps, env._draws, env._elapsed_time) == (0, 0, 0.0)
    log = loop.run(N)
    assert log["steps"].tolist() == [N] * B, "the case is for rovers that step in every iteration"
    elapsed = 0.0
    for _ in range(N):                                                     # each rover's own time, accumulated step by step
        elapsed += dt
    assert (env._steps, env._draws, env._elapsed_time) == (N, N, elapsed)
    assert np.array_equal(_bits(env._robot_state), _bits(log["states"][-1]))
    assert loop.run(N, log=False) is None
    assert (env._steps, env._draws, env._elapsed_time) == (2 * N, 2 * N, elapsed)       # without the log the time stays
    assert loop.episode_buffers()[4] == N
    assert np.array_equal(_bits(env._robot_state), _bits(_last_row(loop, N)))
    loop.close()


@pytest.mark.parametrize("make, noun, mine", [(_astar_dwa, "steps", f"{N}"), (_clrrt, "iterations", f"{N} iterations")])
def test_one_driver_per_episode_and_the_shape_of_injected_draws(make, noun, mine):
    env, loop = make()
    loop.run(N)
    with pytest.raises(ValueError, match="^" + re.escape(f"z must be (n_{noun}, B) = {(N, B)}, got {(N + 1, B)}") + "$"):
        loop.run(N, z=torch.zeros(N + 1, B))
    with pytest.raises(ValueError, match=f"^n_{noun} must be >= 1$"):
        loop.run(0)
    assert env._steps == N, "a refused run moves nothing"
    env.step(torch.zeros(B, 2, device=env._dev))
    text = f"the environment has taken {N + 1} steps since its reset, this loop {mine}: drive an episode either with env.step or with run()"
    with pytest.raises(RuntimeError, match="^" + re.escape(text) + "$"):
        loop.run(N)
    env.reset()                                                            # a reset brings the two together again
    loop.run(N, log=False)
    assert env._steps == N
    loop.close()


def test_clrrt_loop_is_a_context_manager():
    from benchnav_amd import CLRRTLoop
    env, first = _clrrt()
    first.close()
    first.close()                                                          # idempotent
    with CLRRTLoop(env, first.planner, seeds=CL.SEEDS3[:B]) as loop:
        handle = loop._handle
        assert handle.h and loop.run(N, log=False) is None
    assert loop._handle is None and not handle.h
    env.reset()                                                            # finds both loops registered, both closed
    assert env._steps == 0


@pytest.mark.parametrize("planner", ["mppi", "astar_dwa", "cl_rrt"])
def test_a_driver_reports_what_its_planner_left_on_the_device(planner):
    from benchnav_amd import benchmark
    from benchnav_amd.astar_dwa import AStarDWALoop
    from benchnav_amd.benchmark import Benchmark
    bench = Benchmark(T._dataset(), None, start_pos=T.STARTS, goal_pos=T.GOALS, delta_t=T.DT, time_limit=T.LIMIT, stuck_threshold=T.THR,
                      goal_threshold=T.GOAL_THR, trials=1, chunk=B, seed=T.SEED, num_samples=T.NUM_SAMPLES, resolution=T.RES)
    kw = {"mppi": T.MPPI_KW, "astar_dwa": {}, "cl_rrt": {"max_iterations": 60, "max_seqs": 250}}[planner]
    drv = benchmark.DRIVERS[planner](bench, kw)
    rows = drv.rows(N)
    risk = bench.risk_maps(["expected_value", "cvar@0.9"])
    e0, pl, env, idx, invalid = bench._chunk({}, drv.handle_kwargs(kw), 0)
    with pl:
        assert (e0, pl.B, idx.tolist()) == (0, B, [0, 1]) and not invalid.any()
        drv.open(pl, env, 0, idx)
        for c in range(2):
            drv.set_risk_maps(risk[c, idx].contiguous())
            env.reset(seed=benchmark.chunk_seed(bench.seed, 0))
            pl.set_mean(None)
            drv.run(rows)
            assert env._steps == rows
            got, words = drv.score_inputs(), drv.words()
            if planner == "mppi":
                assert drv.loops == [] and got == pl.episode_buffers()[:3] + (None,) and pl.episode_buffers()[3] == rows
            else:
                assert got == drv.loops[-1].episode_buffers()[:4] and drv.loops[-1].episode_buffers()[4] == rows
                assert len(drv.loops) == (c + 1 if planner == "astar_dwa" else 1)
            assert len(got) == 4 and all(got[:3]) and tuple(words) == drv.word_names == (("status", "plans") if planner == "cl_rrt" else ())
            for view, want in zip(words.values(), drv.loops[0].rover_buffers() if words else ()):
                assert view.dtype == torch.int32 and tuple(view.shape) == (B,) and view.data_ptr() == want.data_ptr()
        loops = list(drv.loops)
        assert all(loop._handle for loop in loops), "the loops of earlier settings live until close()"
        assert all(isinstance(loop, AStarDWALoop) for loop in loops) or planner != "astar_dwa"
        torch.cuda.current_stream(bench.dev).synchronize()
        drv.close()
        assert drv.loops == [] and all(loop._handle is None for loop in loops)
