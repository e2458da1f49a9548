#!/usr/bin/env python3
"""Plans per second of benchnav_amd.RRT (csrc/rrt_kernels.hip): the device time of one batch of plans, events around
bn_rrt_plan_async (seeds passed, so every repeat does the same work: samples + growth + goal test / path), median of --reps
after a warm-up.  Shapes: B = 1 / 64 / 256 planners at 1000 iterations on a 64 x 64-cell map (limits (0, 32), start (8, 8), goal
(24, 24), delta 5, rate 0.1: the fixture's first geometry), and B = 1 at 8192 iterations, which keeps the nodes in global memory.
Every shape runs with both widths of the growth kernel (one wave, 256 threads), and the growth + path alone is timed too
(events around bn_rrt_grow_from_samples_async on the device's own sample table).

The reference's CPU time per 1000-iteration plan is the one stored in tests/golden/rrt.npz when the fixture was captured (another
machine's CPU than the GPU host's: the two columns are not one experiment).

    python tools/rrt_rate.py [--reps 5] [--out profiles/rrt_rates.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(1, 1000), (64, 1000), (256, 1000), (1, 8192)]


def measure(B, iters, workgroup, reps):
    from benchnav_amd import RRT, _capi
    from benchnav_amd.rrt import _check
    gm = types.SimpleNamespace(resolution=0.5, x_limits=(0.0, 32.0), y_limits=(0.0, 32.0))
    pl = RRT(gm, torch.tensor([24.0, 24.0]), max_iterations=iters, delta_distance=5, goal_sample_rate=0.1, workgroup=workgroup)
    h = pl._handle(B)
    starts = np.tile(np.array([[8.0, 8.0]], np.float32), (B, 1))
    goals = np.tile(np.array([[24.0, 24.0]], np.float32), (B, 1))
    seeds = np.arange(B, dtype=np.uint64)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)

    def plan():
        _check(pl._lib, pl._lib.bn_rrt_plan_async(h.h, sp, starts.ctypes.data, goals.ctypes.data, seeds.ctypes.data))

    plan()
    stream.synchronize()
    samples = h.buffer(_capi.BN_RRT_BUF_SAMPLES, (B, iters, 2)).clone()     # the caller's copy of the sample table

    def grow():
        _check(pl._lib, pl._lib.bn_rrt_grow_from_samples_async(h.h, sp, starts.ctypes.data, goals.ctypes.data, samples.data_ptr(), _capi.BN_MEM_DEVICE))

    out = {}
    for name, fn in (("plan_ms", plan), ("grow_ms", grow)):
        fn()
        fn()                                                             # warm-up
        stream.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out[name] = round(float(np.median(times)), 4)
        out[name + "_all"] = [round(t, 4) for t in times]
    res = h.buffer(_capi.BN_RRT_BUF_RESULTS, (B, 4), "<i4").cpu().numpy()
    return {"B": B, "iterations": iters, "workgroup": workgroup, "node_storage": pl.node_storage(B), **out,
            "plans_per_s": round(1e3 * B / out["plan_ms"], 1), "ms_per_plan": round(out["plan_ms"] / B, 4), "found": int(res[:, 0].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrt_rates.json"))
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "rrt.npz"))
    ref = [float(v) for v in z["ref_seconds_per_1000"]]
    rows = []
    for B, iters in SHAPES:
        for workgroup in (64, 256):
            rows.append(measure(B, iters, workgroup, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    doc = {"what": "benchnav_amd.RRT: device time of one batch of plans (events around bn_rrt_plan_async, median of %d after a warm-up) "
                   "on one MI355X, both widths of the growth kernel; grow_ms = growth + goal test / path alone" % args.reps,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "reference_cpu": {"what": "the unmodified reference's forward(), 1000 iterations, wall seconds per plan on the CPU the fixture "
                                     "was captured on (tests/golden/rrt.npz, torch %s)" % str(z["torch_version"]),
                             "seconds_per_plan": [round(v, 4) for v in ref], "median": round(float(np.median(ref)), 4)},
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
