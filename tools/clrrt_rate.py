#!/usr/bin/env python3
"""Plans per second of benchnav_amd.CLRRT (csrc/clrrt_kernels.hip): the device time of one batch of plans, events around
bn_clrrt_plan_async (seeds passed, so every repeat does the same work: samples + growth + goal test / path), median of --reps
after a warm-up.  Shapes: B = 1 / 64 / 256 planners at 60 iterations and B = 1 / 64 at the reference's default 500 iterations
with max_seqs 250, on the first fixture plan's 64 x 64-cell map at 0.5 m (start (8, 8, 0.3), goal (24, 24), delta 5, rate 0.25).
The growth + path alone is timed too (events around bn_clrrt_grow_from_samples_async on the device's own sample table).

The reference's CPU seconds are the ones stored in tests/golden/clrrt.npz when the fixture was captured (another machine's CPU
than the GPU host's, and 60- and 50-iteration plans: the two columns are set side by side, not divided into one another).

    python tools/clrrt_rate.py [--reps 5] [--out profiles/clrrt_rates.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(1, 60), (64, 60), (256, 60), (1, 500), (64, 500)]


def measure(B, iters, reps):
    import clrrt_cases as Cs
    from benchnav_amd import _capi
    from benchnav_amd.clrrt import _check
    pl = Cs.planner(0, max_iterations=iters)
    h = pl._handle(B)
    starts = np.tile(np.array([[8.0, 8.0, 0.3]], np.float32), (B, 1))
    goals = np.tile(np.array([[24.0, 24.0, 0.7853982]], np.float32), (B, 1))
    seeds = np.arange(B, dtype=np.uint64) + 42
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)

    def plan():
        _check(pl._lib, pl._lib.bn_clrrt_plan_async(h.h, sp, starts.ctypes.data, goals.ctypes.data, seeds.ctypes.data))

    plan()
    stream.synchronize()
    samples = h.buffer(_capi.BN_CLRRT_BUF_SAMPLES, (B, iters, 3)).clone()

    def grow():
        _check(pl._lib, pl._lib.bn_clrrt_grow_from_samples_async(h.h, sp, starts.ctypes.data, goals.ctypes.data, samples.data_ptr(), _capi.BN_MEM_DEVICE))

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
    res = h.buffer(_capi.BN_CLRRT_BUF_RESULTS, (B, 6), "<i4").cpu().numpy()
    lens = h.buffer(_capi.BN_CLRRT_BUF_SEQ_LENGTHS, (B, iters + 1), "<i4").cpu().numpy()
    return {"B": B, "iterations": iters, "max_seqs": h.S, **out, "plans_per_s": round(1e3 * B / out["plan_ms"], 2),
            "ms_per_plan": round(out["plan_ms"] / B, 4), "found": int(res[:, 0].sum()), "nodes_mean": round(float(res[:, 5].mean()), 1),
            "closed_loop_steps_kept_mean": round(float(lens.sum(1).mean()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clrrt_rates.json"))
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "clrrt.npz"))
    ref = [{"plan": k, "call": j, "iterations": int(z[f"p{k}_params"][0]), "max_seqs": int(z[f"p{k}_params"][3]),
            "seconds": round(float(z[f"p{k}_{j}_seconds"]), 3)} for k in range(int(z["n_plans"])) for j in range(int(z[f"p{k}_params"][7]))]
    rows = []
    for B, iters in SHAPES:
        rows.append(measure(B, iters, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    doc = {"what": "benchnav_amd.CLRRT: device time of one batch of plans (events around bn_clrrt_plan_async, median of %d after a warm-up) "
                   "on one MI355X; grow_ms = growth + goal test / path alone" % args.reps,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "reference_cpu": {"what": "the unmodified reference's forward(), wall seconds per plan on the CPU the fixture was captured on, with "
                                     "the capture's recording wrappers around it (tests/golden/clrrt.npz, torch %s, NumPy %s)"
                                     % (str(z["torch_version"]), str(z["numpy_version"])), "plans": ref},
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
