"""GPU: a live handle is what its plan says.  Every configuration of the sweep (tests/golden/make_golden_mppi_plan.py) is created and
destroyed -- no solve runs -- and shows the observables bn_mppi_debug_plan predicts for this device's CU count, and those of
tests/golden/mppi_plan.json where the device has the recorded count.  Afterwards the device's free memory is where it was."""
import pytest
import torch

from mppi_plan_spec import BN_OK, comparable, gen, golden, plan, predict

pytestmark = pytest.mark.gpu


def test_live_handles_show_what_the_plan_predicts():
    from benchnav_amd import _capi
    lib, gold = _capi.load(), golden()
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    recorded = {e["name"]: e["observed"] for e in gold["entries"]}

    def sweep():
        for name, entry in gen.SWEEP:
            status, p = plan(lib, _capi, entry, n_cus)
            got = gen.observe(lib, _capi, entry)
            assert got["status"] == status, (name, lib.bn_last_error())
            if status != BN_OK:
                continue
            # (overlap is compared as "capable or not", pacing as "paces or not": which of the one-stream modes, and whether the
            # request words sit behind the BAR, is the machine's answer, not the plan's)
            assert comparable(got) == predict(entry, p), name
            if n_cus == gold["n_cus"]:
                assert comparable(got) == comparable(recorded[name]), name

    sweep()                                            # (the first pass also opens whatever the runtime keeps: code objects, its own pools)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    sweep()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
