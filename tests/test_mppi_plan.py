"""CPU: what bn_mppi_create decides -- kernel family, overlap, streams, windows, which buffers exist and how large -- equals
tests/golden/mppi_plan.json for every configuration of the sweep.  The golden was recorded from live handles on an MI355X on the
commit before the decisions moved into plan_mppi (csrc/mppi_plan.h; tests/golden/make_golden_mppi_plan.py,
profiles/mppi_create_refactor.txt); bn_mppi_debug_plan shows the plan here without a device.  No parity test notices a handle that
picks another kernel -- all families compute the same bits -- so this is what holds the policy."""
import pytest

from benchnav_amd import _capi
from mppi_plan_spec import BN_OK, comparable, gen, golden, plan, predict

GOLD = golden()
ENTRIES = {e["name"]: e for e in GOLD["entries"]}
BN_ERR_INVALID = -1


def test_the_golden_holds_the_whole_sweep():
    """The sweep itself: a shrunken golden cannot pass."""
    assert GOLD["n_cus"] == 256
    assert [e["name"] for e in GOLD["entries"]] == [name for name, _ in gen.SWEEP]
    assert len(gen.SWEEP) == 62
    for name, entry in gen.SWEEP:
        assert ENTRIES[name]["config"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in entry.items()}, name
    refused = [e["name"] for e in GOLD["entries"] if e["observed"]["status"] != BN_OK]
    assert refused == ["sampled_t400_refused", "t40000_refused"]
    assert all(sorted(e["decided"]) == sorted(gen.DECIDED) for e in GOLD["entries"] if e["name"] not in refused)
    # every branch of the policy is taken by some entry (256 CUs)
    d = {name: e.get("decided", {}) for name, e in ENTRIES.items()}
    assert d["headline"]["lat_kernel"] and d["headline_b64"]["role_overlap"] and d["headline_b300"]["wave_kernel"]
    assert d["b14_lat_edge"]["lat_kernel"] and not d["b15_role_edge"]["lat_kernel"]
    assert not d["k4096_pipelined_edge"]["ticket_mode"] and d["k4160_ticket_edge"]["ticket_mode"] and d["k8192_ticket"]["ticket_overlap"]
    assert d["sampled"]["ticket_mode"] and d["sampled_reference_order"]["slow_path"] and d["t400_slow"]["slow_path"]
    assert d["headline_b300"]["lds_park"] and not d["resolution_0p3_b64"]["lds_park"] and d["resolution_0p3_b64"]["wave_kernel"]
    assert d["wide_limits"]["WN"] == 0 and d["no_lds_window"]["WN"] == 0 and d["window_overflows_role_lds"]["WN"] == 0
    assert d["t400_slow"]["WN"] == 65 and d["t400_slow_big_window"]["WN"] == 0 and d["tiny_grid"]["WN"] == 9
    assert d["no_pipeline"]["n_streams"] == 1 and d["no_overlap_b64"]["n_streams"] == 1 and d["k70000_two_launches"]["n_streams"] == 1
    assert d["b400_snapshots_capped"]["snap_cap"] == 3495 and d["b30000_snapshot_floor"]["snap_cap"] == 64
    assert d["sampled"]["resident_wgs"] != d["headline"]["resident_wgs"]          # the fused sampled kernel's own figure
    for name, flag in (("store_controls", "STORE_CONTROLS"), ("shared_map_b64", "SHARED_MAP"), ("no_lds_window", "NO_LDS_WINDOW"),
                       ("no_pipeline", "NO_PIPELINE"), ("role_kernel_b1", "ROLE_KERNEL"), ("lat_kernel_b64", "LAT_KERNEL"),
                       ("wave_kernel_b8", "WAVE_KERNEL"), ("no_overlap_b1", "NO_OVERLAP"), ("host_paced_small", "HOST_PACED"),
                       ("private_stream", "PRIVATE_STREAM"), ("lean", "LEAN"), ("sampled", "SAMPLED_SLIP"), ("reference_order", "REFERENCE_ORDER")):
        assert ENTRIES[name]["config"]["flags"] == [flag], name
    o = {name: e["observed"] for name, e in ENTRIES.items()}
    assert o["big_step"]["arithmetic"] == 1 and o["resolution_0p3"]["fast_quotient"] == 1 and o["host_paced_small"]["host_paced"] > 0
    assert o["host_paced_b2_does_not_pace"]["host_paced"] == 0 and o["host_paced_profile_does_not_pace"]["host_paced"] == 0


@pytest.mark.parametrize("name", [name for name, _ in gen.SWEEP])
def test_the_plan_equals_the_recorded_handle(name):
    lib = _capi.load()
    entry, want = dict(gen.SWEEP)[name], ENTRIES[name]
    status, p = plan(lib, _capi, entry, GOLD["n_cus"])
    assert status == want["observed"]["status"], lib.bn_last_error()
    if status != BN_OK:
        assert status == BN_ERR_INVALID and b"even on the slow path" in lib.bn_last_error()
        return
    assert p["n_cus"] == GOLD["n_cus"]
    assert {k: int(p[k]) for k in gen.DECIDED} == want["decided"]                  # what no export of a handle shows
    assert predict(entry, p) == comparable(want["observed"])                       # what the exports show, buffers included
    # the plan's own consistency: derived fields the golden covers only through the above
    K = entry.get("num_samples", 1024)
    assert p["nblk"] == -(-K // 64) and p["Kp"] == 64 * p["nblk"] and p["slip_on"] == int("SAMPLED_SLIP" in entry.get("flags", ()))
    assert p["wave_kernel"] == int(p["pipelined"] and p["want_wave"]) and p["has_alt"] == p["may_overlap"] == int(p["n_streams"] > 1)
    assert p["map_stride"] == (0 if p["n_maps"] == 1 else entry.get("grid_size", 64) ** 2)
    assert p["has_ticket_buffers"] == int(p["slip_on"] or p["ticket_det"]) and p["has_slip_std"] == p["slip_on"]


def test_the_plan_refuses_what_create_refuses():
    """The argument checks live in the plan: same status, same message, no device."""
    lib = _capi.load()
    for entry, text in ((dict(horizon=0), b"must be >= 1"), (dict(resolution=0.0), b"must be positive"),
                        (dict(flags=("LEAN", "SAMPLED_SLIP")), b"BN_FLAG_LEAN is not available"), (dict(x_hi=10.0), b"limits")):
        status, _ = plan(lib, _capi, entry, 256)
        assert status == BN_ERR_INVALID and text in lib.bn_last_error(), entry
    info = _capi.PlanInfo()                            # struct_size not set: refused like a config of another ABI
    assert lib.bn_mppi_debug_plan(gen.config(lib, _capi, {}), 256, info) == BN_ERR_INVALID and b"struct_size" in lib.bn_last_error()
    assert lib.bn_mppi_debug_plan(None, 256, info) == BN_ERR_INVALID


def test_the_cu_count_moves_the_kernel_choice_and_nothing_else():
    """15 instances of K=1024 are 16 x 17 workgroups: the latency kernel on 304 CUs, the role kernel on 256."""
    lib = _capi.load()
    entry = dict(gen.SWEEP)["b15_role_edge"]
    _, small = plan(lib, _capi, entry, 256)
    _, large = plan(lib, _capi, entry, 304)
    assert (small["lat_kernel"], large["lat_kernel"]) == (0, 1) and (small["has_granules"], large["has_granules"]) == (0, 1)
    assert large["resident_wgs"] * 256 == small["resident_wgs"] * 304
    same = [k for k in small if k not in ("n_cus", "lat_kernel", "role_overlap", "has_granules", "resident_wgs")]
    assert {k: small[k] for k in same} == {k: large[k] for k in same}
