#!/usr/bin/env python3
"""A* global planner rates: the field solve (HIP events around its kernels, bn_astar_kernel_ms) and the jump-table build behind
it (bn_astar_jump_ms) for 256^2 and 512^2 maps (--sizes),
smooth / i.i.d. / serpentine-maze terrain, B = 1, 8, 64 instances per launch (each with its own goal); and AStar.forward()
wall time per call (the host walk of the next-hop map + the path tensor).

    python tools/astar_rate.py [--reps 10] [--sizes 64 256 512] [--no-forward] [--no-jump] [--out result.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchnav_amd import AStar, _capi, synth  # noqa: E402

THR, RES = 0.25, 0.5


def maps(kind, G):
    if kind == "smooth":
        return synth.smooth_height_map(G, G, 1).numpy(), synth.smooth_risk_map(G, 2).numpy()
    if kind == "iid":
        return synth.iid_height_map(G, G, 3).numpy(), synth.iid_risk_map(G, 4).numpy()
    return synth.smooth_height_map(G, G, 5, amplitude=0.3).numpy(), synth.serpentine_risk_map(G, G, period=4).numpy()


def goals(risk, B, seed):
    fy, fx = np.nonzero(~(risk <= np.float32(THR)))
    if B == 1:                                  # the far corner of the map from the walls' gaps: the longest field
        j = int(np.argmax(fy * risk.shape[1] + fx))
        return [(int(fx[j]), int(fy[j]))]
    idx = np.random.default_rng(seed).choice(len(fx), B, replace=False)
    return [(int(fx[j]), int(fy[j])) for j in idx]


def solve_ms(lib, kind, G, B, reps, jump=True):
    h_map, r_map = maps(kind, G)
    h = C.c_void_p()
    rc = lib.bn_astar_create(0, G, G, B, C.byref(h))
    if rc:
        raise RuntimeError(lib.bn_astar_last_error())
    try:
        for b, g in enumerate(goals(r_map, B, G + B)):
            assert lib.bn_astar_set_map(h, b, h_map.ctypes.data, r_map.ctypes.data, _capi.BN_MEM_HOST, THR, RES) == 0
            assert lib.bn_astar_set_goal(h, b, *g) == 0
        ms, t, tj = C.c_float(), [], []
        for i in range(reps + 2):
            assert lib.bn_astar_solve_async(h, None) == 0
            if lib.bn_astar_kernel_ms(h, C.byref(ms)) != 0:
                raise RuntimeError(lib.bn_astar_last_error())
            if i >= 2:
                t.append(ms.value)
            if not jump:                                           # the solve alone: no tables are allocated
                continue
            assert lib.bn_astar_jump_build_async(h, None) == 0     # the jump tables behind this solve
            if lib.bn_astar_jump_ms(h, C.byref(ms)) != 0:
                raise RuntimeError(lib.bn_astar_last_error())
            if i >= 2:
                tj.append(ms.value)
        tj = tj or [float("nan")]
        return float(np.median(t)), float(np.min(t)), float(np.max(t)), float(np.median(tj)), float(np.min(tj)), float(np.max(tj))
    finally:
        lib.bn_astar_destroy(h)


def forward_us(kind, G, calls):
    h_map, r_map = maps(kind, G)
    g = goals(r_map, 1, 0)[0]
    gm = types.SimpleNamespace(tensors={"heights": torch.from_numpy(h_map).cuda()}, resolution=RES, x_limits=(0.0, G * RES), y_limits=(0.0, G * RES))
    dyn = types.SimpleNamespace(_traversability_model=types.SimpleNamespace(_risks=torch.from_numpy(r_map).cuda()))
    planner = AStar(gm, torch.tensor([(g[0] + 0.5) * RES, (g[1] + 0.5) * RES]), dyn, THR, device="cuda")
    fy, fx = np.nonzero(~(r_map <= np.float32(THR)))
    rng = np.random.default_rng(1)
    starts = [torch.tensor([(fx[j] + 0.5) * RES, (fy[j] + 0.5) * RES, 0.0], dtype=torch.float32, device="cuda") for j in rng.choice(len(fx), calls)]
    planner.forward(starts[0])                  # waits for the field solve
    torch.cuda.synchronize()
    t, lens = [], []
    for s in starts:
        t0 = time.perf_counter()
        p = planner.forward(s)
        t.append(time.perf_counter() - t0)
        lens.append(0 if p is None else p.shape[0])
    planner.close()
    return float(np.median(t) * 1e6), float(np.percentile(t, 90) * 1e6), float(np.median(lens))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512], help="map edge lengths")
    ap.add_argument("--no-forward", action="store_true", help="solve and table-build times only")
    ap.add_argument("--no-jump", action="store_true", help="time the solve alone: the jump tables are neither allocated nor built")
    a = ap.parse_args()
    lib = _capi.load()
    rows = []
    for G in a.sizes:
        for kind in ("smooth", "iid", "maze"):
            for B in (1, 8, 64):
                med, lo, hi, jmed, jlo, jhi = solve_ms(lib, kind, G, B, a.reps, not a.no_jump)
                rows.append(dict(what="solve", G=G, kind=kind, B=B, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4)))
                if not a.no_jump:
                    rows[-1].update(jump_ms_median=round(jmed, 4), jump_ms_min=round(jlo, 4), jump_ms_max=round(jhi, 4))
                print(json.dumps(rows[-1]), flush=True)
            if a.no_forward:
                continue
            med, p90, plen = forward_us(kind, G, a.calls)
            rows.append(dict(what="forward", G=G, kind=kind, us_median=round(med, 1), us_p90=round(p90, 1), median_path_nodes=plen))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
