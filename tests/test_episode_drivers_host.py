"""CPU: the episode drivers Benchmark.run looks up by planner name (benchnav_amd/benchmark.py) -- the registry, the rows of an
episode's log, the keywords of a chunk's NativeMPPI and the CL-RRT driver's keyword check.  None of it needs a device."""
import pytest

from benchnav_amd import benchmark

NAMES = ("mppi", "astar_dwa", "cl_rrt")


def test_the_planners_are_the_registry_keys_in_order():
    assert benchmark.PLANNERS == NAMES
    assert benchmark.PLANNERS == tuple(benchmark.DRIVERS)
    assert all(issubclass(d, benchmark.EpisodeDriver) for d in benchmark.DRIVERS.values())


def test_rows_of_an_episode_log():
    assert [benchmark.DRIVERS[name].rows(20) for name in NAMES] == [20, 20, 40]


@pytest.mark.parametrize("kw, mppi, astar_dwa", [
    ({}, {"horizon": 50, "num_samples": 1024}, {"horizon": 10, "num_samples": 64}),
    ({"horizon": 12}, {"horizon": 12, "num_samples": 1024}, {"horizon": 12, "num_samples": 64}),
    ({"horizon": 12, "num_samples": 256, "seed": 3}, {"horizon": 12, "num_samples": 256, "seed": 3}, {"horizon": 12, "num_samples": 64}),
])
def test_handle_kwargs(kw, mppi, astar_dwa):
    given = dict(kw)
    assert benchmark.DRIVERS["mppi"].handle_kwargs(kw) == mppi                      # the caller's keywords over the two defaults
    assert benchmark.DRIVERS["astar_dwa"].handle_kwargs(kw) == astar_dwa            # the horizon only: num_samples and seed are dropped
    assert benchmark.DRIVERS["cl_rrt"].handle_kwargs(kw) == {"horizon": 8, "num_samples": 64}       # nothing of the caller's
    assert kw == given, "handle_kwargs must not change the caller's dict"


def test_the_clrrt_driver_refuses_an_unknown_keyword():
    with pytest.raises(TypeError, match=r"^unknown cl_rrt keywords: \['horizon', 'walk'\]$"):
        benchmark.DRIVERS["cl_rrt"](None, {"max_iterations": 60, "walk": "jump", "horizon": 12})
    drv = benchmark.DRIVERS["cl_rrt"](None, {"max_iterations": 60, "max_seqs": 250, "delta_distance": 5, "goal_sample_rate": 0.25, "path_cap": None})
    assert drv.kw["max_iterations"] == 60 and drv.loops == [] and drv.word_names == ("status", "plans")
