"""CPU: the rules of a CL-RRT benchmark campaign that need no device (benchnav_amd/benchmark.py) -- the planner's name, the
iteration bound, the planner seed, the outcome words of a CLRRTLoop's status -- and the entry points the campaign added to the C
ABI: bound in _capi.SYMBOLS, declared by the header and exported by the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

from benchnav_amd import _capi, benchmark, build

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "benchnav_mppi.h")
NEW_SYMBOLS = ("bn_clrrt_set_instance_maps", "bn_clrrt_loop_episode_buffers", "bn_clrrt_loop_rover_buffers")


def test_cl_rrt_is_a_planner_of_the_benchmark():
    assert "cl_rrt" in benchmark.PLANNERS and benchmark.PLANNERS[:2] == ("mppi", "astar_dwa")


def test_clrrt_iterations_is_twice_the_step_limit():
    assert benchmark.clrrt_iterations(1) == 2
    assert benchmark.clrrt_iterations(20) == 40
    assert benchmark.clrrt_iterations(benchmark.max_steps(100.0, 0.1)) == 2002
    assert isinstance(benchmark.clrrt_iterations(np.int64(7)), int)


def test_planner_seed_adds_the_episode_and_wraps_at_two_to_the_32():
    assert benchmark.planner_seed(5, 0) == 5 and benchmark.planner_seed(5, 7) == 12
    assert benchmark.planner_seed(2 ** 32 - 1, 0) == 2 ** 32 - 1
    assert benchmark.planner_seed(2 ** 32 - 1, 1) == 0 and benchmark.planner_seed(2 ** 32 - 2, 5) == 3
    assert benchmark.planner_seed(2 ** 40 + 3, 4) == 7                      # a 64-bit campaign seed keeps its low word
    assert all(0 <= benchmark.planner_seed(s, e) < 2 ** 32 for s in (0, 2 ** 63, 2 ** 64 - 1) for e in (0, 1, 10 ** 6))
    # beside its neighbours, which wrap at 2^64
    assert benchmark.chunk_seed(2 ** 32 - 1, 1) == 2 ** 32 and benchmark.risk_seed(2 ** 64 - 1, 1) == 0


@pytest.mark.parametrize("done", [-1, 0, 37])
def test_clrrt_outcome_words_over_every_status(done):
    names = ("RUNNING", "GOAL", "TIME_LIMIT", "NO_PLAN", "NO_SEQUENCE", "PLAN_EXHAUSTED", "PATH_OVERFLOW", "OUT_OF_BOUNDS")
    codes = [getattr(_capi, "BN_CL_" + n) for n in names]
    assert codes == list(range(8))
    status = np.array(codes, np.int32)
    done_step, stopped = benchmark.clrrt_outcome_words(status, np.full(8, done, np.int32))
    assert done_step.dtype == np.int32 and stopped.dtype == np.int32
    assert done_step.tolist() == [-1, done, -1, -1, -1, -1, -1, -1]           # only a GOAL has a goal step
    assert stopped.tolist() == [0, 0, 0, 3, 4, 5, 6, 7]                       # RUNNING, GOAL and TIME_LIMIT are no stop
    # plain sequences too, and each rover by its own done_iter
    d, s = benchmark.clrrt_outcome_words([1, 1, 5], [4, 9, 2])
    assert d.tolist() == [4, 9, -1] and s.tolist() == [0, 0, 5]


def test_the_campaign_entry_points_are_bound_declared_and_exported():
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS, name
    text = open(HEADER).read()
    decl = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))       # as test_capi_symbols.py reads it
    assert set(NEW_SYMBOLS) <= decl
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_library()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported
    assert re.search(r"int bn_clrrt_set_instance_maps\(bn_clrrt_t \*h, void \*stream, const void \*risks, int where, double stuck_threshold\);",
                     text)


def test_null_arguments_are_refused_before_the_device():
    import ctypes as C
    lib = _capi.load()
    assert lib.bn_clrrt_set_instance_maps(None, None, None, _capi.BN_MEM_HOST, 0.1) == _capi.BN_ERR_INVALID
    assert b"null" in lib.bn_clrrt_last_error()
    p = C.c_void_p()
    assert lib.bn_clrrt_loop_episode_buffers(None, C.byref(p), None, None, None, None, None) == _capi.BN_ERR_INVALID
    assert lib.bn_clrrt_loop_rover_buffers(None, C.byref(p), None) == _capi.BN_ERR_INVALID


def test_a_report_lists_plans_only_where_it_has_them():
    arrays = {name: np.zeros((1, 2, 1), np.float64 if "float" in str(dt) else np.int32) for name, dt in benchmark.FIELDS}
    base = benchmark.Report("mppi", ["expected_value"], arrays, 0, 4, 1, 20, 0.1, 2.0)
    assert base.plans is None and "plans" not in base.to_dict()["episodes"]
    rep = benchmark.Report("cl_rrt", ["expected_value"], dict(arrays, plans=np.array([[[1], [3]]], np.int32)), 0, 4, 1, 20, 0.1, 2.0)
    assert rep.to_dict()["episodes"]["plans"] == [[[1], [3]]]
    assert set(rep.to_dict()["episodes"]) - {"plans"} == set(base.to_dict()["episodes"])
