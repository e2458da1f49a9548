#!/usr/bin/env python3
"""Generate tests/golden/rrt.npz by running the reference RRT planner (build container only).

Runs the *unmodified* reference `RRT` (src/planners/global_planners/sampling_based/rrt.py, with its `Tree`) on CPU and stores
plain arrays: each case's inputs, the tree after forward() (`nodes[:n]` float32, `edges[:n]` int32, `costs[:n]`), the
`_goal_node_indices` list, the returned path (or that it was None), the reference's wall time per plan and the torch version.
Nothing of the reference itself is stored.

    python tests/golden/make_golden_rrt.py

Recipe of make_golden.py: the reference's src and root on sys.path, `opensimplex` stubbed (it only seeds, set_randomness).
RRT reads grid_map.resolution, .x_limits and .y_limits only (rrt.py:59-61), so the map is a small namespace holding those.

Keys: `n_cases`, `torch_version`, `ref_seconds_per_1000` and per case k `c{k}_params` (x0, x1, y0, y1, sx, sy, gx, gy, delta,
rate as float64), `c{k}_iters`, `c{k}_seed` (uint64), `c{k}_calls`, and per call j `c{k}_{j}_nodes/edges/costs/goal_idx/path/found/
seconds`.
"""
from __future__ import annotations

import os
import sys
import time
import types

import numpy as np
import torch

REF = os.environ.get("BENCHNAV_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REF, "src"), REF]
_stub = types.ModuleType("opensimplex")
_stub.seed = lambda s: None
_stub.noise2 = lambda x, y: 0.0
sys.modules["opensimplex"] = _stub

from src.planners.global_planners.sampling_based.rrt import RRT  # noqa: E402

SEEDS = [0, 1, 42, 2 ** 31 - 1, 2 ** 32 - 1]
# (limits, start, goal, iterations, delta, rate)
GEOMETRIES = [
    ((0.0, 32.0), (8.0, 8.0), (24.0, 24.0), 1000, 5, 0.1),
    ((0.0, 9.9), (1.1, 2.3), (8.7, 9.1), 300, 1.5, 0.1),
    ((0.0, 32.0), (2.0, 30.0), (30.0, 1.5), 64, 5, 0.25),
    ((0.0, 128.0), (5.0, 5.0), (120.0, 120.0), 200, 5, 0.1),
]


def cases():
    out = [(g, s, 1) for g in GEOMETRIES for s in SEEDS]
    out.append((GEOMETRIES[1], 7, 2))                                               # two consecutive forward() calls on one planner
    out.append((((0.0, 32.0), (8.0, 8.0), (24.0, 24.0), 3, 5, 0.1), 42, 1))        # three iterations: no path
    return out


def run(geometry, seed, calls):
    lim, start, goal, iters, delta, rate = geometry
    gm = types.SimpleNamespace(resolution=0.5, x_limits=lim, y_limits=lim)
    planner = RRT(gm, torch.tensor(goal, dtype=torch.float32), max_iterations=iters, delta_distance=delta, goal_sample_rate=rate,
                  device="cpu", seed=seed)
    got = []
    for _ in range(calls):
        t0 = time.perf_counter()
        path = planner(torch.tensor(start, dtype=torch.float32))
        dt = time.perf_counter() - t0
        n = planner.tree.nodes_count
        got.append({
            "nodes": planner.tree.nodes[:n].numpy().astype(np.float32).copy(),
            "edges": planner.tree.edges[:n].numpy().astype(np.int32),
            "costs": planner.tree.costs[:n].numpy().astype(np.float32).copy(),
            "goal_idx": np.asarray(planner._goal_node_indices, np.int32),
            "path": (path.numpy().astype(np.float32) if path is not None else np.zeros((0, 2), np.float32)),
            "found": np.bool_(path is not None),
            "seconds": np.float64(dt),
        })
    return got


def main():
    arrays = {"torch_version": np.array(torch.__version__)}
    few, tied, secs = 0, 0, []
    cs = cases()
    for k, (geometry, seed, calls) in enumerate(cs):
        lim, start, goal, iters, delta, rate = geometry
        arrays[f"c{k}_params"] = np.array([lim[0], lim[1], lim[0], lim[1], start[0], start[1], goal[0], goal[1], delta, rate], np.float64)
        arrays[f"c{k}_iters"] = np.int32(iters)
        arrays[f"c{k}_seed"] = np.uint64(seed)
        arrays[f"c{k}_calls"] = np.int32(calls)
        for j, r in enumerate(run(geometry, seed, calls)):
            for name, v in r.items():
                arrays[f"c{k}_{j}_{name}"] = v
            m = len(r["goal_idx"])
            if 2 <= m <= 16:
                few += 1
                c = r["costs"][r["goal_idx"]]
                tied += bool(len(np.unique(c)) < m)
            if iters == 1000:
                secs.append(float(r["seconds"]))
            print(f"case {k}: seed {seed} iters {iters} call {j}: {len(r['nodes'])} nodes, {m} near the goal, "
                  f"path {len(r['path'])} rows, {r['seconds']:.3f} s")
    assert few >= 6 and tied >= 1, (few, tied)       # the tie rule of DESIGN.md 4.6 is exercised where the reference's sort is stable
    arrays["n_cases"] = np.int32(len(cs))
    arrays["ref_seconds_per_1000"] = np.array(secs, np.float64)   # the reference's CPU time per 1000-iteration plan at capture
    out = os.path.join(HERE, "rrt.npz")
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {os.path.getsize(out)} bytes; {few} cases with 2-16 near-goal nodes, {tied} of them with a cost tie")


if __name__ == "__main__":
    main()
