"""Records tests/golden/mppi_plan.json: what bn_mppi_create decides for a fixed sweep of configurations, as a live handle shows it.

Run on an MI355X, on a build of the commit BEFORE the handle moved onto the plan (csrc/mppi_plan.h), never on a later one:

    python tests/golden/make_golden_mppi_plan.py [--decided FILE]

Every entry of SWEEP is created and destroyed (no solve runs); per handle the script reads bn_mppi_arithmetic,
bn_mppi_launches_per_solve, bn_mppi_launches_per_forward, bn_mppi_host_paced, bn_mppi_row_pitch, bn_mppi_fast_quotient, whether
bn_mppi_overlap_mode is 3, both byte counts, and bn_mppi_device_buffer's status and size for all twelve buffer ids.  A
configuration create refuses is recorded with its status.

--decided FILE: one JSON object per line, one line per handle that was created, in sweep order: the decisions no export shows
(WN, reach, lds_park, n_streams, snap_cap, resident_wgs, wave_kernel, lat_kernel, role_overlap, ticket_mode, ticket_overlap,
slow_path), printed by a throw-away patch at the end of that commit's bn_mppi_create (profiles/mppi_create_refactor.txt says
which).  They go into the same JSON under "decided".

tests/test_mppi_plan.py and tests/test_gpu_mppi_plan.py import SWEEP, config() and observe() from here."""
import ctypes as C
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mppi_plan.json")
FLAGS = dict(STORE_CONTROLS=1, SHARED_MAP=2, NO_LDS_WINDOW=4, PROFILE=8, PRIVATE_STREAM=16, NO_PIPELINE=32, SAMPLED_SLIP=64,
             WAVE_KERNEL=128, ROLE_KERNEL=256, LEAN=512, LAT_KERNEL=1024, NO_OVERLAP=2048, REFERENCE_ORDER=4096, HOST_PACED=8192)
N_BUFFERS = 12
DECIDED = ("WN", "reach", "lds_park", "n_streams", "snap_cap", "resident_wgs", "wave_kernel", "lat_kernel", "role_overlap", "ticket_mode",
           "ticket_overlap", "slow_path")

# name -> what differs from K=1024, T=50, G=64, B=1, resolution 0.5, limits [0, G * resolution], the defaults of bn_mppi_config_init.
# `flags` is a tuple of FLAGS names; x_hi widens the limits; every other key is a field of bn_mppi_config.
SWEEP = [
    ("headline", dict(grid_size=256)),
    ("headline_b64", dict(grid_size=256, num_instances=64)),                      # role kernel, overlapped
    ("headline_b300", dict(grid_size=256, num_instances=300)),                    # one-wave kernel
    ("small", dict(num_samples=128, horizon=10)),
    ("b14_lat_edge", dict(num_instances=14)),                                     # 15 x 17 = 255 workgroups: the last latency launch
    ("b15_role_edge", dict(num_instances=15)),                                    # 16 x 17 = 272 > 256
    ("k4096_pipelined_edge", dict(num_samples=4096)),                             # 64 workgroups: still merged by every workgroup
    ("k4160_ticket_edge", dict(num_samples=4160)),                                # 65: the ticket merge
    ("k8192_ticket", dict(num_samples=8192)),
    ("k8192_ticket_b8", dict(num_samples=8192, num_instances=8)),
    ("k16384_t100", dict(num_samples=16384, horizon=100, grid_size=128)),         # two-level merge rows in the tail
    ("k70000_two_launches", dict(num_samples=70000, horizon=10)),                 # more than 1024 workgroups: no ticket merge either
    ("k2112_b300_no_wave", dict(num_samples=2112, horizon=20, num_instances=300)),   # 33 workgroups per instance: the one-wave kernel stops at 32
    ("k2048_b300_wave", dict(num_samples=2048, horizon=20, num_instances=300)),
    ("short_horizon_b300", dict(num_samples=128, horizon=10, num_instances=300)),
    ("t200_no_latency_kernel", dict(horizon=200, resolution=2.0)),                # the latency kernel's ring does not fit the LDS
    ("k2048_no_granules", dict(num_samples=2048)),                                # latency kernel, 32 workgroups per instance: rows are not republished
    ("lean", dict(flags=("LEAN",))),
    ("lean_b64", dict(num_instances=64, flags=("LEAN",))),
    ("lean_b300", dict(num_instances=300, flags=("LEAN",))),
    ("sampled", dict(flags=("SAMPLED_SLIP",))),
    ("sampled_b8", dict(num_instances=8, flags=("SAMPLED_SLIP",))),
    ("sampled_k8192", dict(num_samples=8192, flags=("SAMPLED_SLIP",))),
    ("sampled_reference_order", dict(flags=("SAMPLED_SLIP", "REFERENCE_ORDER"))),  # slow path
    ("sampled_no_pipeline", dict(flags=("SAMPLED_SLIP", "NO_PIPELINE"))),
    ("sampled_tail_window_too_big", dict(horizon=63, grid_size=256, resolution=0.1, flags=("SAMPLED_SLIP",))),   # 129 x 129 window
    ("sampled_t400_refused", dict(horizon=400, flags=("SAMPLED_SLIP",))),         # the sampled slow path keeps a control tile: refused
    ("window_overflows_role_lds", dict(horizon=100, grid_size=256, resolution=0.125)),   # a 163 x 163 window: global gather, still the role kernel
    ("t400_slow", dict(horizon=400)),                                             # the control tile overflows the role kernels' LDS
    ("t400_slow_big_window", dict(horizon=400, grid_size=256, resolution=0.125)),  # ... and the whole map does not fit the one-wave kernel's
    ("t400_slow_b4_store", dict(horizon=400, num_instances=4, flags=("STORE_CONTROLS",))),
    ("t40000_refused", dict(horizon=40000, num_samples=64, grid_size=8, resolution=1.0)),   # ... and the slow path's
    ("resolution_0p3", dict(resolution=0.3)),                                     # not a power of two: the quotient check
    ("resolution_0p3_b64", dict(resolution=0.3, num_instances=64)),
    ("tiny_grid", dict(grid_size=8, resolution=1.0)),                             # the reach exceeds the map
    ("wide_limits", dict(x_hi=40.0)),                                             # 80 cells of limits over a 64-cell grid
    ("big_step", dict(dt=0.6)),                                                   # dt |omega| > 0.5: the reference-order arithmetic
    ("huge_step", dict(dt=3.5, resolution=4.0)),                                  # dt |omega| > 3: the general heading wrap
    ("reference_order", dict(flags=("REFERENCE_ORDER",))),
    ("reference_order_b300", dict(num_instances=300, flags=("REFERENCE_ORDER",))),
    ("lambda_0p3", dict(lambda_=0.3)),                                            # no exact reciprocal
    ("store_controls", dict(flags=("STORE_CONTROLS",))),
    ("shared_map_b64", dict(num_instances=64, flags=("SHARED_MAP",))),
    ("no_lds_window", dict(flags=("NO_LDS_WINDOW",))),
    ("no_pipeline", dict(flags=("NO_PIPELINE",))),
    ("role_kernel_b1", dict(flags=("ROLE_KERNEL",))),
    ("role_kernel_b300", dict(num_instances=300, flags=("ROLE_KERNEL",))),
    ("lat_kernel_b64", dict(num_instances=64, flags=("LAT_KERNEL",))),
    ("wave_kernel_b8", dict(num_instances=8, flags=("WAVE_KERNEL",))),
    ("wave_kernel_b8_store", dict(num_instances=8, flags=("WAVE_KERNEL", "STORE_CONTROLS"))),
    ("no_overlap_b1", dict(flags=("NO_OVERLAP",))),
    ("no_overlap_b64", dict(num_instances=64, flags=("NO_OVERLAP",))),
    ("no_overlap_k8192", dict(num_samples=8192, flags=("NO_OVERLAP",))),
    ("host_paced_small", dict(num_samples=128, horizon=10, flags=("HOST_PACED",))),
    ("host_paced_headline", dict(grid_size=256, flags=("HOST_PACED",))),
    ("host_paced_b2_does_not_pace", dict(num_instances=2, flags=("HOST_PACED",))),
    ("host_paced_profile_does_not_pace", dict(flags=("HOST_PACED", "PROFILE"))),
    ("private_stream", dict(grid_size=256, flags=("PRIVATE_STREAM",))),
    ("private_stream_b64", dict(num_instances=64, flags=("PRIVATE_STREAM",))),
    ("profile", dict(flags=("PROFILE",))),
    ("b400_snapshots_capped", dict(num_samples=128, horizon=10, num_instances=400)),            # 16 MB of snapshots: fewer than 4096 entries
    ("b30000_snapshot_floor", dict(num_samples=64, horizon=5, grid_size=8, resolution=1.0, num_instances=30000, flags=("SHARED_MAP",))),
]


def flag_bits(entry):
    bits = 0
    for name in entry.get("flags", ()):
        bits |= FLAGS[name]
    return bits


def config(lib, capi, entry):
    cfg = capi.Config()
    lib.bn_mppi_config_init(C.byref(cfg))
    for key, value in entry.items():
        if key not in ("flags", "x_hi"):
            setattr(cfg, key, value)
    cfg.x_limits[1] = cfg.y_limits[1] = cfg.grid_size * cfg.resolution
    if "x_hi" in entry:
        cfg.x_limits[1] = entry["x_hi"]
    cfg.flags = flag_bits(entry)
    return cfg


def observe(lib, capi, entry):
    """Create, read what the exports show, destroy."""
    cfg, h = config(lib, capi, entry), C.c_void_p()
    status = lib.bn_mppi_create(C.byref(cfg), C.byref(h))
    if status != capi.BN_OK:
        return dict(status=status)
    try:
        buffers = []
        for buf_id in range(N_BUFFERS):
            ptr, nbytes = C.c_void_p(), C.c_size_t(0)
            buffers.append([lib.bn_mppi_device_buffer(h, buf_id, C.byref(ptr), C.byref(nbytes)), nbytes.value])
        return dict(status=status, arithmetic=lib.bn_mppi_arithmetic(h), launches_per_solve=lib.bn_mppi_launches_per_solve(h),
                    launches_per_forward=lib.bn_mppi_launches_per_forward(h), host_paced=lib.bn_mppi_host_paced(h),
                    row_pitch=lib.bn_mppi_row_pitch(h), fast_quotient=lib.bn_mppi_fast_quotient(h),
                    never_overlaps=int(lib.bn_mppi_overlap_mode(h) == 3),
                    algorithmic_bytes=[lib.bn_mppi_algorithmic_bytes(h, noise) for noise in (capi.BN_NOISE_PHILOX, capi.BN_NOISE_DEVICE_KT2)],
                    algorithmic_bytes_window=[lib.bn_mppi_algorithmic_bytes_window(h, noise) for noise in (capi.BN_NOISE_PHILOX, capi.BN_NOISE_DEVICE_KT2)],
                    buffers=buffers)
    finally:
        lib.bn_mppi_destroy(h)


def main(argv):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from benchnav_amd import _capi
    lib = _capi.load()
    decided = None
    if "--decided" in argv:
        path = argv[argv.index("--decided") + 1]
        open(path, "w").close()                        # the patched create appends to it
        os.environ["BN_PLAN_DUMP"] = path
    entries = []
    for name, entry in SWEEP:
        entries.append(dict(name=name, config={k: (list(v) if isinstance(v, tuple) else v) for k, v in entry.items()}, observed=observe(lib, _capi, entry)))
    if "--decided" in argv:
        decided = [json.loads(line) for line in open(path)]
        created = [e for e in entries if e["observed"]["status"] == _capi.BN_OK]
        assert len(decided) == len(created), (len(decided), len(created))
        for e, d in zip(created, decided):
            assert sorted(d) == sorted(DECIDED), sorted(d)
            e["decided"] = d
    out = dict(n_cus=torch.cuda.get_device_properties(0).multi_processor_count, entries=entries)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {len(entries)} entries, {out['n_cus']} CUs, decided {'merged' if decided else 'absent'}")


if __name__ == "__main__":
    main(sys.argv[1:])
