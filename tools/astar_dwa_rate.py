"""Control steps per second of the A* + DWA loop on one MI355X: the host-composed loop of test_astar_dwa.py (AStar.forward ->
DWA.update_reference_path -> DWA.forward -> env.step) against the fused device loop (AStarDWALoop.run, one workgroup per rover),
on the test_astar_dwa.py problem (G = 64, res 0.5, T = 50, 10 x 10 candidates, a_lim 0.5 / 0.5) and at 256^2.

Also the time per step on the serpentine maze (astar_maps.spiral: paths of ~G^2 / 2 nodes) and the next-hop walk's share of it,
by difference against the smooth map's step at the same G (paths of ~100 nodes: the rest of the step is the same work).  Times
are wall clock over one run() call: the chained launches plus one read-back of the log.

    python tools/astar_dwa_rate.py [--steps 500] [--json out.json] [--walk {serial,jump}]
    python tools/astar_dwa_rate.py --case maze64 --walk jump [--batch 64]     (one fused case, one JSON line)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/astar_dwa_rate.py --case maze256 --steps 200
        (one fused B = 1 case alone -- smooth64, smooth256, maze64, maze256 -- for the kernel time per step: the astar_dwa_kernel
         total of the stats divided by steps + 20 warm-up steps)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]
import astar_maps as M                              # noqa: E402

RES, THR, T = 0.5, 0.2, 50


def smooth_risk(G, seed):
    from benchnav_amd import synth
    r = synth.smooth_risk_map(G, seed).numpy()
    return (0.3 + 0.65 * (r - r.min()) / (r.max() - r.min())).astype(np.float32)


def make(G, B, risk, heights, start, goal, walk="serial"):
    from benchnav_amd import AStarDWALoop, NativeMPPI
    from benchnav_amd.env import BatchedPlanetaryEnv
    pl = NativeMPPI(horizon=T, num_samples=64, grid_size=G, resolution=RES, num_instances=B, shared_map=True, stream=0, stuck_threshold=THR)
    mean = np.full((G, G), 0.25, np.float32)
    std = np.full((G, G), 0.05, np.float32)
    env = BatchedPlanetaryEnv(pl, mean, std, start, goal, stuck_threshold=THR, goal_threshold=1.0, seed=7)
    loop = AStarDWALoop(env, heights, risk, THR, (0.5, 0.5), 0.1, walk=walk)
    return pl, env, loop


def fused(G, B, risk, heights, start, goal, steps, walk="serial"):
    pl, env, loop = make(G, B, risk, heights, start, goal, walk)
    env.reset()
    loop.run(20)                                    # warm-up (code objects, LDS attribute)
    env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = loop.run(steps)                           # (returns after the log is read back)
    wall = time.perf_counter() - t0
    return dict(B=B, walk=walk, steps=steps, wall_s=wall, steps_per_s=steps / wall, rover_steps_per_s=B * steps / wall,
                us_per_step=wall * 1e6 / steps, status=np.bincount(out[5], minlength=4).tolist())


def composed(G, risk, heights, start, goal, steps):
    from benchnav_amd import AStar, DWA, NativeMPPI
    from benchnav_amd.env import BatchedPlanetaryEnv
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    pl = NativeMPPI(horizon=T, num_samples=64, grid_size=G, resolution=RES, num_instances=1, stream=0, stuck_threshold=THR)
    env = BatchedPlanetaryEnv(pl, np.full((G, G), 0.25, np.float32), np.full((G, G), 0.05, np.float32), start, goal,
                              stuck_threshold=THR, goal_threshold=1.0, seed=7)
    gm = FakeGridMap(G, RES)
    gm.tensors = {"heights": torch.from_numpy(heights).cuda()}
    dyn = FakeDynamics(torch.from_numpy(risk).cuda(), gm)
    solver = DWA(horizon=T, dim_state=3, dim_control=2, dynamics=dyn, objectives=FakeObjectives(torch.tensor(goal), THR),
                 a_lim=torch.tensor([0.5, 0.5]), delta_t=0.1, num_lin_vel=10, num_ang_vel=10)
    astar = AStar(grid_map=gm, goal_pos=torch.tensor(goal), dynamics=dyn, stuck_threshold=THR)
    state = env.reset(seed=0)[0]

    def step(state):
        with torch.no_grad():
            path = astar.forward(state=state)
            solver.update_reference_path(path)
            action_seq, _ = solver.forward(state=state)
        st, _, _, _ = env.step(action_seq[0, :].reshape(1, 2))
        return st[0]

    for _ in range(20):
        state = step(state)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        state = step(state)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return dict(B=1, steps=steps, wall_s=wall, steps_per_s=steps / wall, us_per_step=wall * 1e6 / steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--json", default=None)
    ap.add_argument("--case", default=None, choices=["smooth64", "smooth256", "maze64", "maze256"])
    ap.add_argument("--walk", default="serial", choices=["serial", "jump"],
                    help="how the fused kernel reads the path: lane 0 walks next, or every lane through the A* jump tables")
    ap.add_argument("--batch", type=int, default=1, help="instances of a --case run")
    args = ap.parse_args()
    n, wk = args.steps, args.walk
    if args.case:
        G = int(args.case.lstrip("smothaze"))
        if args.case.startswith("maze"):
            h, risk, thr, _, gcell = M.spiral(G)
            r = fused(G, args.batch, risk.astype(np.float32), h, np.float32([0.3, 0.3]),
                      np.float32([(gcell[0] + 0.5) * RES, (gcell[1] + 0.5) * RES]), n, wk)
        else:
            r = fused(G, args.batch, smooth_risk(G, 1), M.smooth_heights(G, G, 5), np.float32([0.15 * G * RES] * 2),
                      np.float32([0.8 * G * RES] * 2), n, wk)
        print(json.dumps({args.case: r}))
        return
    res = {}
    for G in (64, 256):
        heights = M.smooth_heights(G, G, 5)
        risk = smooth_risk(G, 1)
        ext = G * RES
        start, goal = np.float32([0.15 * ext, 0.15 * ext]), np.float32([0.8 * ext, 0.8 * ext])
        r = {"composed_B1": composed(G, risk, heights, start, goal, n)}
        for B in (1, 64, 256):
            r[f"fused_B{B}"] = fused(G, B, risk, heights, start, goal, n, wk)
        r["speedup_B1"] = r["fused_B1"]["steps_per_s"] / r["composed_B1"]["steps_per_s"]
        res[f"G{G}"] = r
    # the maze: the walk is the only part of the step that grows with the path, so its share is the difference to the smooth map
    for G in (64, 256):
        h, risk, thr, _, gcell = M.spiral(G)
        goal = np.float32([(gcell[0] + 0.5) * RES, (gcell[1] + 0.5) * RES])
        maze = fused(G, 1, risk.astype(np.float32), h, np.float32([0.3, 0.3]), goal, n, wk)
        smooth = res[f"G{G}"]["fused_B1"]["us_per_step"]
        res[f"maze_G{G}"] = dict(fused_B1=maze, walk_share=1.0 - smooth / maze["us_per_step"])
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
