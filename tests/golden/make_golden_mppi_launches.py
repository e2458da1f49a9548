"""Records tests/golden/mppi_launches.json: the launch log (bn_mppi_debug_launch_log) of one fixed script of calls, for one
configuration per launch path of the MPPI handle.

Run on an MI355X, on a build of the commit BEFORE the solve path moved onto the launch decision (csrc/mppi_launch.h) that carries the
throw-away patch profiles/mppi_launch_refactor.txt describes (it fills the same record from that commit's SolveParams in front of
every launch), never on a later one:

    python tests/golden/make_golden_mppi_launches.py [RUNS]

CONFIGS: for every distinct launch path tests/golden/mppi_plan.json shows (PATH_KEY over its "decided" values and flags) the
smallest entry of make_golden_mppi_plan.SWEEP that has it, or a smaller configuration that decides the same (`like` names the sweep
entry it stands for; tests/test_mppi_launches.py holds that on the CPU with bn_mppi_debug_plan).

The script (run_script) per configuration, one handle alive at a time, the log read after every step:
  solve          one bn_mppi_solve
  async2_flush   two bn_mppi_solve_async and a bn_mppi_flush
  batchN_idle    bn_mppi_solve_n_async of N = 3, 4, 17 solves (odd, even, at least kEagerTailMinBatch) behind a bn_mppi_sync
  batchN_busy    ... directly behind a pending bn_mppi_solve_async; device states and Philox noise throughout
  host_kt2       one solve with BN_NOISE_HOST_KT2
  forward        one instance: four bn_mppi_forward_state_async + bn_mppi_first_action steps (the host-paced loop where the handle paces)
  shard          one bn_mppi_shard_rollout_async + bn_mppi_shard_finish_async
  episode        (configurations marked so) bn_mppi_env_attach and one bn_mppi_episode_async of 5 steps
Every step ends with bn_mppi_sync.  Every batch stays under 64 solves (no tuner window closes) and every launch fits one residency
round, so nothing in the log depends on a hipStreamQuery race -- except whether the stream of a batchN_busy step is still busy when
the batch is enqueued: the script runs RUNS times (default 3) and a step whose log differed between runs keeps both versions (two
at most; the file says which steps needed it under "alternatives").

tests/test_gpu_mppi_launches.py imports CONFIGS, run_script() and matches() from here."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "mppi_launches.json")
_spec = importlib.util.spec_from_file_location("make_golden_mppi_plan", os.path.join(HERE, "make_golden_mppi_plan.py"))
plan_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_gen)
SWEEP = dict(plan_gen.SWEEP)

# what tells two launch paths apart: "decided" values of the plan golden, then flags / observables
PATH_KEY = ("lat_kernel", "wave_kernel", "role_overlap", "ticket_mode", "ticket_overlap", "slow_path")
PATH_FLAGS = ("SAMPLED_SLIP", "LEAN", "STORE_CONTROLS")              # + arithmetic (reference order) and host_paced of "observed"

# name -> (the sweep entry it stands for, its configuration: None = the sweep entry itself, runs the episode step)
CONFIGS = [
    ("small", "small", None, False),
    ("host_paced_small", "host_paced_small", None, False),
    ("store_controls", "store_controls", None, False),
    ("lean", "lean", None, False),
    ("reference_order", "reference_order", None, False),
    ("role_kernel_b1", "role_kernel_b1", None, True),
    ("lean_b15", "lean_b64", dict(num_instances=15, flags=("LEAN",)), False),
    ("wave_kernel_b8", "wave_kernel_b8", None, False),
    ("wave_kernel_b8_store", "wave_kernel_b8_store", None, False),
    ("lean_b300_small", "lean_b300", dict(num_samples=128, horizon=10, num_instances=300, flags=("LEAN",)), False),
    ("reference_order_b300_small", "reference_order_b300", dict(num_samples=128, horizon=10, num_instances=300, flags=("REFERENCE_ORDER",)), False),
    ("k4160_ticket_edge", "k4160_ticket_edge", None, False),
    ("no_overlap_k8192", "no_overlap_k8192", None, False),
    ("sampled", "sampled", None, False),
    ("no_pipeline", "no_pipeline", None, False),
    ("sampled_no_pipeline", "sampled_no_pipeline", None, False),
    ("sampled_reference_order", "sampled_reference_order", None, False),
    ("t400_slow", "t400_slow", None, False),
    ("t400_slow_b4_store", "t400_slow_b4_store", None, False),
]
BATCHES = (3, 4, 17)


def entry_of(name):
    for n, like, entry, _ in CONFIGS:
        if n == name:
            return entry if entry is not None else SWEEP[like]
    raise KeyError(name)


def fields(capi):
    return [n for n, _ in capi.LaunchRecord._fields_]


def run_script(lib, capi, name):
    """{"steps": {step: {"status": [...], "records": [[...], ...]}}, "overlap_mode", "recoveries", "host_paced"} of one configuration."""
    import torch
    entry = entry_of(name)
    episode = [c[3] for c in CONFIGS if c[0] == name][0]
    cfg, h = plan_gen.config(lib, capi, entry), C.c_void_p()
    assert lib.bn_mppi_create(C.byref(cfg), C.byref(h)) == capi.BN_OK, lib.bn_last_error()
    names = fields(capi)
    buf = (capi.LaunchRecord * 256)()
    steps = {}
    try:
        B, K, T, G = cfg.num_instances, cfg.num_samples, cfg.horizon, cfg.grid_size
        PH, DEV, HOST = capi.BN_NOISE_PHILOX, capi.BN_MEM_DEVICE, capi.BN_MEM_HOST
        assert lib.bn_mppi_debug_launch_log(h, None, 0) == 0

        def done(step, *status):
            status = list(status) + [lib.bn_mppi_sync(h)]
            n = lib.bn_mppi_debug_launch_log(h, buf, 256)
            steps[step] = dict(status=status, records=[[int(getattr(buf[i], f)) for f in names] for i in range(n)])

        yy, xx = np.mgrid[0:G, 0:G]
        risk = np.ascontiguousarray(0.05 + 0.3 * ((xx * 7 + yy * 3) % 11) / 11.0, np.float32)
        goal = (C.c_float * 2)(0.8 * G * cfg.resolution, 0.7 * G * cfg.resolution)
        status = [lib.bn_mppi_set_map(h, -1, C.c_void_p(risk.ctypes.data), HOST)]
        if "SAMPLED_SLIP" in entry.get("flags", ()):
            std = np.full((G, G), 0.05, np.float32)
            status.append(lib.bn_mppi_set_slip_std(h, -1, C.c_void_p(std.ctypes.data), HOST))
        status.append(lib.bn_mppi_set_goal(h, -1, goal))
        states = np.zeros((B, 3), np.float32)
        states[:, 0] = 4.0 + 0.01 * (np.arange(B) % 100)
        states[:, 1] = 5.0
        states[:, 2] = 0.3
        d_states = torch.from_numpy(states).cuda()
        sp = C.c_void_p(d_states.data_ptr())
        done("setup", *status)
        done("solve", lib.bn_mppi_solve(h, sp, DEV, None, PH, None, None))
        done("async2_flush", lib.bn_mppi_solve_async(h, sp, DEV, None, PH), lib.bn_mppi_solve_async(h, sp, DEV, None, PH), lib.bn_mppi_flush(h))
        for n in BATCHES:
            done(f"batch{n}_idle", lib.bn_mppi_solve_n_async(h, n, sp, DEV, None, PH, 1, 0))
            done(f"batch{n}_busy", lib.bn_mppi_solve_async(h, sp, DEV, None, PH), lib.bn_mppi_solve_n_async(h, n, sp, DEV, None, PH, 1, 0))
        eps = np.random.default_rng(1).standard_normal((B, K, T, 2), np.float32)
        done("host_kt2", lib.bn_mppi_solve_async(h, sp, DEV, C.c_void_p(eps.ctypes.data), capi.BN_NOISE_HOST_KT2))
        if B == 1:
            out = torch.zeros(T * 2 + (T + 1) * 3, device="cuda")
            act, status = (C.c_float * 2)(), []
            st = states[0].copy()
            for _ in range(4):
                status.append(lib.bn_mppi_forward_state_async(h, C.c_void_p(st.ctypes.data), None, PH, C.c_void_p(out.data_ptr())))
                status.append(lib.bn_mppi_first_action(h, 0, act))
                st[0] += 0.02
            done("forward", *status)
        ptr, nwg, per = C.c_void_p(), C.c_int32(), C.c_int32()
        status = [lib.bn_mppi_shard_rollout_async(h, sp, DEV, None, PH), lib.bn_mppi_shard_partials(h, C.byref(ptr), C.byref(nwg), C.byref(per))]
        status.append(lib.bn_mppi_shard_finish_async(h, ptr, nwg) if status == [capi.BN_OK, capi.BN_OK] else None)
        done("shard", *status)
        if episode:
            mean, std = np.full((1, G, G), 0.2, np.float32), np.full((1, G, G), 0.02, np.float32)
            done("episode", lib.bn_mppi_env_attach(h, C.c_void_p(mean.ctypes.data), C.c_void_p(std.ctypes.data), HOST, 0.5, 0.1, 1),
                 lib.bn_mppi_episode_async(h, 5, C.c_void_p(states.ctypes.data), HOST, None, PH, 1, 0, None))
        return dict(steps=steps, overlap_mode=lib.bn_mppi_overlap_mode(h), recoveries=lib.bn_mppi_recovery_count(h),
                    host_paced=int(lib.bn_mppi_host_paced(h) > 0))
    finally:
        lib.bn_mppi_destroy(h)


def matches(step_golden, step_live):
    """A live step against the golden's: the same statuses and one of the recorded logs."""
    return step_live["status"] == step_golden["status"] and step_live["records"] in step_golden["records"]


def main(argv):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from benchnav_amd import _capi
    lib = _capi.load()
    runs = int(argv[0]) if argv else 3
    configs, alternatives = {}, []
    for name, like, _, _ in CONFIGS:
        seen = [run_script(lib, _capi, name) for _ in range(runs)]
        first = seen[0]
        assert all(s["recoveries"] == 0 for s in seen), name
        assert all((s["overlap_mode"], s["host_paced"], list(s["steps"])) == (first["overlap_mode"], first["host_paced"], list(first["steps"])) for s in seen), name
        steps = {}
        for step in first["steps"]:
            assert all(s["steps"][step]["status"] == first["steps"][step]["status"] for s in seen), (name, step)
            logs = []
            for s in seen:
                if s["steps"][step]["records"] not in logs:
                    logs.append(s["steps"][step]["records"])
            assert len(logs) <= 2 and (len(logs) == 1 or step.endswith("_busy")), (name, step, len(logs))
            if len(logs) > 1:
                alternatives.append(f"{name}/{step}")
            steps[step] = dict(status=first["steps"][step]["status"], records=logs)
        configs[name] = dict(like=like, overlap_mode=first["overlap_mode"], host_paced=first["host_paced"], steps=steps)
    head = dict(n_cus=torch.cuda.get_device_properties(0).multi_processor_count, fields=fields(_capi), alternatives=alternatives)
    with open(GOLDEN, "w") as f:                     # one record per line
        f.write("{\n" + "".join(f' "{k}": {json.dumps(v)},\n' for k, v in head.items()) + ' "configs": {\n')
        for ci, (name, c) in enumerate(configs.items()):
            f.write(f'  "{name}": {{"like": "{c["like"]}", "overlap_mode": {c["overlap_mode"]}, "host_paced": {c["host_paced"]}, "steps": {{\n')
            for si, (step, s) in enumerate(c["steps"].items()):
                f.write(f'   "{step}": {{"status": {json.dumps(s["status"])}, "records": [\n')
                f.write(",\n".join("    [" + ",\n     ".join(json.dumps(r, separators=(",", ":")) for r in log) + "]" for log in s["records"]))
                f.write("]}" + ("," if si + 1 < len(c["steps"]) else "") + "\n")
            f.write("  }}" + ("," if ci + 1 < len(configs) else "") + "\n")
        f.write(" }\n}\n")
    json.load(open(GOLDEN))
    print(f"{GOLDEN}: {len(configs)} configurations, {head['n_cus']} CUs, two logs kept for {alternatives or 'no step'}")


if __name__ == "__main__":
    main(sys.argv[1:])
