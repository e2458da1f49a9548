#!/usr/bin/env python3
"""Map instances per second of benchnav_amd.TerrainGenerator (csrc/terrain_kernels.hip) for B x G with DatasetGenerator's
defaults (3 craters, fBm): the device time of one generation (events around bn_terrain_generate_async, median of --reps) and,
separately, the host's draws (terrain.replay_draws per instance, median over 16 seeds).  Every shape runs twice: without the
colouring step, and with it (4 of 10 classes, the library's own noise; rows marked "coloring": true), same method.

    python tools/terrain_rate.py [--batches 1 64 256] [--grids 64 256 512] [--reps 5] [--no-coloring]
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
    args = ap.parse_args()
    from benchnav_amd.terrain import TerrainGenerator, occupancies, replay_draws, slip_models
    warnings.simplefilter("ignore")
    rows = []
    for G in args.grids:
        for coloring in ([False] if args.no_coloring else [False, True]):
            host = []
            for s in range(16):
                t0 = time.perf_counter()
                replay_draws(s, G, args.res, **({"coloring": True} if coloring else {}))
                host.append(time.perf_counter() - t0)
            host_ms = 1e3 * float(np.median(host))
            for B in args.batches:
                with TerrainGenerator(G, args.res, batch=B) as gen:
                    if coloring:                                             # warm-up; the draws and the colouring inputs stay set
                        gen.generate(range(B), slip_models=slip_models(10), occupancy=occupancies(10)[0])
                    else:
                        gen.generate(range(B), slip_models=slip_models(1))
                    stream = torch.cuda.current_stream()
                    times = []
                    for _ in range(args.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        gen._check(gen._lib.bn_terrain_generate_async(gen._handle, C.c_void_p(stream.cuda_stream)))
                        e1.record(stream)
                        e1.synchronize()
                        times.append(e0.elapsed_time(e1))
                dev_ms = float(np.median(times))
                row = {"G": G, "B": B, "coloring": coloring, "device_ms": round(dev_ms, 3), "device_inst_per_s": round(1e3 * B / dev_ms, 1),
                       "host_draw_ms_per_inst": round(host_ms, 3),
                       "end_to_end_inst_per_s": round(1e3 * B / (dev_ms + B * host_ms), 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
