#!/usr/bin/env python3
"""Map instances per second of benchnav_amd.TerrainGenerator (csrc/terrain_kernels.hip) for B x G with DatasetGenerator's
defaults (3 craters, fBm): the device time of one generation (events around bn_terrain_generate_async, median of --reps) and,
separately, the host's draws (terrain.replay_draws per instance, median over 16 seeds).  Every shape runs twice: without the
colouring step, and with it (4 of 10 classes, the library's own noise; rows marked "coloring": true), same method.

With --draws device the draws are made on the device (generate(..., draws="device")): the timed window is the draws kernel plus
the generation (events around bn_terrain_draw_async + bn_terrain_generate_async), the draws kernel is also timed on its own
("draws_ms"), there is no host draw, and the end-to-end rate is B over that window.  Both modes also report "call_inst_per_s":
B over the wall time of one whole generate() call (parameters, draws, launch, read-back, output copies; median of --reps).

    python tools/terrain_rate.py [--batches 1 64 256] [--grids 64 256 512] [--reps 5] [--no-coloring] [--draws host|device]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--grids", type=int, nargs="+", default=[64, 256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=float, default=0.5)
    ap.add_argument("--no-coloring", action="store_true", help="skip the legs with the colouring step")
    ap.add_argument("--draws", choices=["host", "device"], default="host", help="where the random draws are made")
    args = ap.parse_args()
    device = args.draws == "device"
    mode = {"draws": "device"} if device else {}
    from benchnav_amd.terrain import TerrainGenerator, occupancies, replay_draws, slip_models
    warnings.simplefilter("ignore")
    rows = []
    for G in args.grids:
        for coloring in ([False] if args.no_coloring else [False, True]):
            host = [0.0] if device else []
            for s in ([] if device else range(16)):
                t0 = time.perf_counter()
                replay_draws(s, G, args.res, **({"coloring": True} if coloring else {}))
                host.append(time.perf_counter() - t0)
            host_ms = 1e3 * float(np.median(host))
            for B in args.batches:
                with TerrainGenerator(G, args.res, batch=B) as gen:
                    kw = {"slip_models": slip_models(10), "occupancy": occupancies(10)[0]} if coloring else {"slip_models": slip_models(1)}
                    gen.generate(range(B), **kw, **mode)                     # warm-up; the draws and the colouring inputs stay set
                    stream = torch.cuda.current_stream()
                    keys = np.arange(B, dtype=np.uint64)
                    times, draw_times, calls = [], [], []
                    for _ in range(args.reps):
                        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                        e0.record(stream)
                        if device:
                            gen._check(gen._lib.bn_terrain_draw_async(gen._handle, keys.ctypes.data, C.c_void_p(stream.cuda_stream)))
                            e1.record(stream)
                        gen._check(gen._lib.bn_terrain_generate_async(gen._handle, C.c_void_p(stream.cuda_stream)))
                        e2.record(stream)
                        e2.synchronize()
                        times.append(e0.elapsed_time(e2))
                        if device:
                            draw_times.append(e0.elapsed_time(e1))
                    for _ in range(args.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        gen.generate(range(B), **kw, **mode)
                        torch.cuda.synchronize()
                        calls.append(time.perf_counter() - t0)
                dev_ms = float(np.median(times))
                row = {"G": G, "B": B, "coloring": coloring, "draws": args.draws, "device_ms": round(dev_ms, 3),
                       "device_inst_per_s": round(1e3 * B / dev_ms, 1), "host_draw_ms_per_inst": round(host_ms, 3),
                       "end_to_end_inst_per_s": round(1e3 * B / (dev_ms + B * host_ms), 1),
                       "call_inst_per_s": round(B / float(np.median(calls)), 1)}
                if device:
                    row["draws_ms"] = round(float(np.median(draw_times)), 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
