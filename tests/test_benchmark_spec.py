"""CPU: the benchmark stage's rules that need no device.

  a. tests/benchmark_spec.py, the float64 NumPy scoring spec the GPU tests use as their reference, against hand-computed values on
     hand-written logs (3-4-5 triangles, so every distance is exact);
  b. benchmark.max_steps, the episode -> (chunk, instance) rule and the two seed rules;
  c. the new C entry points: declared, exported, bound, and without a GPU refused with BN_ERR_NO_DEVICE and "no CPU fallback"."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import benchmark_spec as S
from benchnav_amd import _capi, benchmark as BM

f32 = np.float32
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _states(*xy):
    return np.array([[x, y, 0.0] for x, y in xy], f32)


def _one(states, rewards, goal, end, done, **kw):
    return S.score_episode(states, np.array(rewards, f32), np.array(goal, f32), end, done, **kw)


# ---- a. the spec on hand-written logs -------------------------------------------------------------------------------------------
def test_single_step_episode_that_reaches_its_goal():
    r = _one(_states((0, 0), (3, 4)), [0.5], (3, 4), 1, 0)
    assert r == {"outcome": S.GOAL, "steps": 1, "time": 0.1, "path_length": 5.0, "reward_sum": 0.5, "reward_min": f32(0.5),
                 "stuck_steps": 0, "final_distance": 0.0}


def test_end_step_zero_counts_nothing():
    r = _one(_states((0, 0), (3, 4), (6, 8)), [0.5, 0.5], (3, 4), 0, -1)
    assert (r["outcome"], r["steps"], r["time"], r["path_length"], r["reward_sum"], r["stuck_steps"]) == (S.TIME_LIMIT, 0, 0.0, 0.0, 0.0, 0)
    assert np.isnan(r["reward_min"]) and r["reward_min"].dtype == f32
    assert r["final_distance"] == 5.0                       # from the start: no row was walked


def test_goal_at_the_first_step_counts_one_row():
    states, done = _states((0, 0), (3, 4), (3, 4), (3, 4)), np.array([0])
    assert S.default_end_step(done, 3).tolist() == [1]      # done_step is the 0-based step index: k + 1 rows count
    r = _one(states, [0.75, 0.5, 0.05], (3, 4), 1, 0)
    assert (r["outcome"], r["steps"], r["time"], r["path_length"], r["reward_min"], r["stuck_steps"]) == (S.GOAL, 1, 0.1, 5.0, f32(0.75), 0)


def test_goal_never_reached_walks_every_row():
    assert S.default_end_step(np.array([-1]), 3).tolist() == [3]
    r = _one(_states((0, 0), (3, 4), (6, 8), (6, 8)), [0.5, 0.05, 0.1], (6, 20), 3, -1)
    assert (r["outcome"], r["steps"], r["path_length"], r["final_distance"]) == (S.TIME_LIMIT, 3, 10.0, 12.0)
    assert r["time"] == 0.1 + 0.1 + 0.1 == 0.30000000000000004          # three float64 additions, not 3 * 0.1
    assert r["reward_sum"] == (0.5 + float(f32(0.05))) + float(f32(0.1))
    assert r["reward_min"] == f32(0.05)
    assert r["stuck_steps"] == 2                             # 0.05 and float32(0.1) <= float32(0.1); 0.5 is not


def test_nan_rows_in_the_middle_and_at_the_end_are_no_steps():
    r = _one(_states((0, 0), (3, 4), (3, 4), (6, 8), (6, 8)), [0.5, NAN, 0.25, NAN], (6, 8), 4, -1, stopped=2)
    assert (r["outcome"], r["steps"], r["time"], r["path_length"], r["reward_sum"], r["reward_min"]) == (S.STOPPED, 2, 0.2, 10.0, 0.75, f32(0.25))
    assert r["final_distance"] == 0.0
    # a NaN row's state is still the rover's position: the next counted row measures from it, not from the last counted state
    r = _one(_states((0, 0), (3, 4), (6, 8), (9, 12)), [0.5, NAN, 0.5], (9, 12), 3, -1)
    assert (r["steps"], r["path_length"]) == (2, 10.0)
    # NaN rows only: nothing counted, the final distance is from where the rover stands
    r = _one(_states((0, 0), (0, 0), (0, 0)), [NAN, NAN], (3, 4), 2, -1, stopped=1)
    assert (r["outcome"], r["steps"], r["time"], r["final_distance"]) == (S.STOPPED, 0, 0.0, 5.0) and np.isnan(r["reward_min"])


def test_outcome_precedence():
    st, rw = _states((0, 0), (3, 4)), [0.5]
    assert _one(st, rw, (3, 4), 1, 0, stopped=1, invalid=True)["outcome"] == S.INVALID        # invalid beats done
    assert _one(st, rw, (3, 4), 1, 0, stopped=1)["outcome"] == S.GOAL                         # done beats stopped
    assert _one(st, rw, (3, 4), 1, -1, stopped=1)["outcome"] == S.STOPPED
    assert _one(st, rw, (3, 4), 1, -1)["outcome"] == S.TIME_LIMIT


def test_batched_spec_is_the_per_episode_loop():
    states = np.stack([_states((0, 0), (3, 4), (6, 8)), _states((1, 1), (1, 1), (4, 5))], axis=1)     # (3, 2, 3)
    rewards = np.array([[0.5, NAN], [0.25, 0.05]], f32)
    goals = np.array([[6, 8], [4, 5]], f32)
    got = S.score_episodes(states, rewards, goals, None, np.array([1, -1]), stopped=np.array([0, 3]), invalid=np.array([False, False]))
    assert got["outcome"].tolist() == [S.GOAL, S.STOPPED] and got["steps"].tolist() == [2, 1]
    assert got["path_length"].tolist() == [10.0, 5.0] and got["stuck_steps"].tolist() == [0, 1]
    assert got["outcome"].dtype == np.int32 and got["reward_min"].dtype == f32 and got["time"].dtype == np.float64


# ---- b. steps, slots, seeds -------------------------------------------------------------------------------------------------------
def test_max_steps_is_the_float64_accumulation():
    for fn in (S.max_steps, BM.max_steps):
        assert fn(100.0, 0.1) == 1001                        # a thousand additions of 0.1 stay below 100
        assert fn(2.0, 0.1) == 20                            # the twentieth sum is 2.0000000000000004
        assert fn(0.5, 0.1) == 6                             # five additions give exactly 0.5, which does not exceed it
        assert fn(0.3, 0.1) == 3                             # 0.30000000000000004 > 0.3
    with pytest.raises(ValueError):
        BM.max_steps(1.0, 0.0)


def test_episode_slots_and_seeds():
    trials, chunk = 2, 4
    slots = [BM.episode_slot(m * trials + r, chunk) for m in range(3) for r in range(trials)]
    assert slots == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1)]       # one full chunk and a short one
    assert BM.chunk_seed(7, 0) == 7 and BM.chunk_seed(7, 3) == 10
    assert BM.chunk_seed(2 ** 64 - 1, 1) == 0 and BM.risk_seed(2 ** 64 - 2, 5) == 3          # mod 2^64
    assert BM.risk_seed(7, 2) == 9


def test_settings_parse():
    assert BM.parse_setting("expected_value") == ("expected_value", None)
    assert BM.parse_setting("var@0.9") == ("var", 0.9) and BM.parse_setting(("cvar", 0.5)) == ("cvar", 0.5)
    assert [BM.setting_name(s) for s in ("expected_value", ("var", 0.9), "cvar@0.999")] == ["expected_value", "var@0.9", "cvar@0.999"]
    assert BM.OUTCOMES == ("GOAL", "TIME_LIMIT", "STOPPED", "INVALID")
    assert (BM.GOAL, BM.TIME_LIMIT, BM.STOPPED, BM.INVALID) == (S.GOAL, S.TIME_LIMIT, S.STOPPED, S.INVALID)


def test_report_summary_leaves_invalid_episodes_out():
    z = lambda dt: np.zeros((1, 2, 2), dt)
    arrays = {"outcome": np.array([[[BM.GOAL, BM.TIME_LIMIT], [BM.INVALID, BM.GOAL]]], np.int32), "steps": np.array([[[10, 20], [5, 30]]], np.int32),
              "time": np.array([[[1.0, 2.0], [0.5, 3.0]]]), "path_length": np.array([[[4.0, 1.0], [9.0, 6.0]]]),
              "reward_sum": np.array([[[5.0, 10.0], [1.0, 15.0]]]), "reward_min": z(f32), "stuck_steps": np.array([[[0, 3], [9, 3]]], np.int32),
              "final_distance": z(np.float64)}
    row = BM.Report("mppi", ["var@0.9"], arrays, seed=1, chunk=4, trials=2, max_steps=20, delta_t=0.1, time_limit=2.0).summary()[0]
    assert row["valid"] == 3 and row["counts"] == {"GOAL": 2, "TIME_LIMIT": 1, "STOPPED": 0, "INVALID": 1}
    assert row["rates"] == {"GOAL": 2 / 3, "TIME_LIMIT": 1 / 3, "STOPPED": 0.0}
    assert (row["time_to_goal_mean"], row["time_to_goal_median"], row["path_length_mean"]) == (2.0, 2.0, 5.0)
    assert row["stuck_steps_mean"] == 2.0 and row["reward_mean"] == 0.5


# ---- c. the C entry points ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("bn_risk_maps_infer", "bn_episode_score", "bn_score_last_error", "bn_mppi_episode_buffers", "bn_astar_dwa_episode_buffers")


def test_new_functions_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "benchnav_mppi.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in _capi.SYMBOLS and getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    assert lib.bn_mppi_episode_buffers(None, None, None, None, None, None) == _capi.BN_ERR_INVALID
    assert lib.bn_astar_dwa_episode_buffers(None, None, None, None, None, None, None) == _capi.BN_ERR_INVALID


def _risk_maps_call(lib, n_settings=1, num_samples=1000, confidence=0.9):
    buf = np.ones(4, f32)
    metrics = (C.c_int * max(n_settings, 1))(*[_capi.BN_RISK_VAR] * max(n_settings, 1))
    conf = (C.c_float * max(n_settings, 1))(*[confidence] * max(n_settings, 1))
    return lib.bn_risk_maps_infer(0, None, buf.ctypes.data, buf.ctypes.data, 1, 2, metrics, conf, n_settings, num_samples, None, None, buf.ctypes.data)


def _score_call(lib, n=1, B=1):
    buf = np.zeros(16, np.float64)
    p = buf.ctypes.data
    return lib.bn_episode_score(0, None, p, p, p, None, p, None, None, n, B, 0.1, 0.1, p, p, p, p, p, p, p, p)


def test_arguments_are_refused_before_the_device_is_touched():
    lib = _capi.load()
    for kw in (dict(n_settings=0), dict(n_settings=17), dict(num_samples=1), dict(num_samples=4097), dict(confidence=1.5)):
        assert _risk_maps_call(lib, **kw) == _capi.BN_ERR_INVALID, kw
    assert b"num_settings" in (_risk_maps_call(lib, n_settings=17), lib.bn_risk_last_error())[1]
    assert _score_call(lib, n=0) == _capi.BN_ERR_INVALID and _score_call(lib, B=0) == _capi.BN_ERR_INVALID
    assert b"n_steps" in (_score_call(lib, n=0), lib.bn_score_last_error())[1]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_present(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_gpu():
    lib = _capi.load()
    assert _risk_maps_call(lib) == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_risk_last_error()
    assert _score_call(lib) == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_score_last_error()
    import torch
    from benchnav_amd.risk import infer_risk_maps
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infer_risk_maps(torch.zeros(1, 2, 2), torch.ones(1, 2, 2), [("var", 0.9)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BM.score_episodes(np.zeros((2, 1, 3), f32), np.zeros((1, 1), f32), np.zeros((1, 2), f32), None, np.zeros(1, np.int32))
