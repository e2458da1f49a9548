"""GPU: the solve path launches what it launched before it moved onto the launch decision (csrc/mppi_launch.h).  The script of
tests/golden/make_golden_mppi_launches.py runs on one configuration per launch path; where the device has the recorded CU count its
launch log (bn_mppi_debug_launch_log) is compared record by record with tests/golden/mppi_launches.json, recorded from the commit
before (profiles/mppi_launch_refactor.txt); elsewhere the log is non-empty and every step's wait values are monotonic."""
import pytest
import torch

from mppi_launches_spec import gen, golden

pytestmark = pytest.mark.gpu

GOLD = golden()
F = {name: i for i, name in enumerate(GOLD["fields"])}


def describe(name, step, want, got):
    for alt in want:
        if len(alt) != len(got):
            continue
        for i, (a, b) in enumerate(zip(alt, got)):
            if a != b:
                return f"{name}/{step} launch {i}: " + ", ".join(f"{f} {a[j]} -> {b[j]}" for f, j in F.items() if a[j] != b[j])
    return f"{name}/{step}: {[len(a) for a in want]} launches recorded, {len(got)} made"


@pytest.mark.parametrize("name", [c[0] for c in gen.CONFIGS])
def test_launch_log_is_the_recorded_one(name):
    from benchnav_amd import _capi
    lib, want = _capi.load(), GOLD["configs"][name]
    got = gen.run_script(lib, _capi, name)
    assert got["recoveries"] == 0
    assert got["overlap_mode"] == want["overlap_mode"]
    assert list(got["steps"]) == list(want["steps"])
    assert sum(len(s["records"]) for s in got["steps"].values()) > 0
    same_device = torch.cuda.get_device_properties(0).multi_processor_count == GOLD["n_cus"]
    for step, s in got["steps"].items():
        assert s["status"] == want["steps"][step]["status"], (name, step, lib.bn_last_error())
        if same_device:
            assert gen.matches(want["steps"][step], s), describe(name, step, want["steps"][step]["records"], s["records"])
        # the counters only grow: what a launch waits for is at least what the launch before it waited for
        rollouts = [r for r in s["records"] if r[F["entry"]] != 5]
        assert all(a[F["solve"]] < b[F["solve"]] for a, b in zip(rollouts, rollouts[1:])), (name, step)
        for field, by in (("wait_tail", None), ("wait_tail_self", None), ("wait_part", "prev_slot"), ("wait_part_self", "cur_slot")):
            for slot in ({r[F[by]] for r in rollouts} if by else {None}):
                seq = [r[F[field]] for r in rollouts if (by is None or r[F[by]] == slot) and r[F[field]]]
                assert seq == sorted(seq), (name, step, field, slot)
