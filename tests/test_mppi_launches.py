"""CPU: the launch-log golden (tests/golden/mppi_launches.json, recorded on an MI355X from the commit before the solve path moved onto
the launch decision of csrc/mppi_launch.h; profiles/mppi_launch_refactor.txt) covers every launch path the plan golden shows, the
smaller configurations it uses decide what the sweep entries they stand for decide (bn_mppi_debug_plan, no device), and the export
refuses what it must.  tests/test_gpu_mppi_launches.py replays the script on a device."""
import ctypes as C

from benchnav_amd import _capi

import mppi_launches_spec as spec
import mppi_plan_spec as plan_spec

gen = spec.gen


def test_every_launch_path_of_the_plan_golden_has_a_configuration():
    plan = plan_spec.golden()
    paths = {spec.path_key(e["config"], e["decided"], e["observed"]["arithmetic"], e["observed"]["host_paced"]): e["name"]
             for e in plan["entries"] if e["observed"]["status"] == _capi.BN_OK}
    by_name = {e["name"]: e for e in plan["entries"]}
    covered = set()
    for name, like, entry, _ in gen.CONFIGS:
        e = by_name[like]
        covered.add(spec.path_key(e["config"], e["decided"], e["observed"]["arithmetic"], e["observed"]["host_paced"]))
    assert covered == set(paths), [paths[k] for k in set(paths) - covered]
    recorded = spec.golden()
    assert list(recorded["configs"]) == [c[0] for c in gen.CONFIGS]
    assert recorded["fields"] == gen.fields(_capi)
    for name, c in recorded["configs"].items():
        assert c["like"] == [like for n, like, _, _ in gen.CONFIGS if n == name][0]
        for step, s in c["steps"].items():
            assert 1 <= len(s["records"]) <= 2, (name, step)               # at most two alternatives, and only where the recipe allows them
            assert len(s["records"]) == 1 or (step.endswith("_busy") and f"{name}/{step}" in recorded["alternatives"]), (name, step)


def test_smaller_configurations_decide_what_their_sweep_entries_decide():
    lib = _capi.load()
    n_cus = plan_spec.golden()["n_cus"]
    for name, like, entry, _ in gen.CONFIGS:
        if entry is None:
            continue
        (s0, p0), (s1, p1) = plan_spec.plan(lib, _capi, gen.SWEEP[like], n_cus), plan_spec.plan(lib, _capi, entry, n_cus)
        assert s0 == s1 == _capi.BN_OK, name
        same = gen.PATH_KEY + ("ref_order", "slip_on", "pipelined", "may_overlap", "n_streams", "has_X", "has_U", "has_granules", "has_alt",
                               "has_ticket_buffers")
        assert {k: p0[k] for k in same} == {k: p1[k] for k in same}, name
        assert entry.get("flags", ()) == gen.SWEEP[like].get("flags", ()), name


def test_the_launch_log_export_checks_its_arguments():
    lib = _capi.load()
    rec = (_capi.LaunchRecord * 1)()
    assert lib.bn_mppi_debug_launch_log(None, rec, 1) == _capi.BN_ERR_INVALID
    assert lib.bn_mppi_debug_launch_log(None, None, 0) == _capi.BN_ERR_INVALID
    assert C.sizeof(_capi.LaunchRecord) == 33 * 4 + 4 + 6 * 8          # 33 int32, padding, 6 uint64: include/benchnav_mppi.h
