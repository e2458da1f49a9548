#!/usr/bin/env python3
"""Rates of benchnav_amd.CLRRTLoop (csrc/clrrt_loop.hip): the plan-follow-replan loop of test/test_cl_rrt.py:167-200 on the
device, on the fixture's s = 1.4 case (tests/golden/clrrt_loop.npz: 64 x 64 cells of 0.5 m, latent slip 1.4 x the predicted one,
start (8, 8), goal (24, 24), 60 iterations x 250 closed-loop steps per plan), 1000 loop iterations, B = 1 / 64 / 256 rovers with
their own planner seeds and Philox slip draws.  Per B, median of --reps runs after a warm-up run:
  wall_us_per_iteration     host wall clock of run(1000) (stream idle before and after) / 1000
  follow_us_per_step        HIP events around the follow launches, summed / the largest step count of a rover
  plan_share                1 - follow time / wall: the masked plans and the host's look at the pending counter, once per round
and, at B = 1, the HOST-COMPOSED loop from the parts that exist without this class, in alternating runs with the fused one:
CLRRT.forward, then per control step the torch deviation (torch.norm + torch.min + the comparison's host read) and
BatchedPlanetaryEnv.step.  Behind the shared-map cases, B = 64 / 256 with one risk map per rover (CLRRTLoop(..., risk_maps=...): the
fixture's map times a factor in [0.8, 1.3] that cycles over eleven values); --shared-only leaves those out, for runs against a
commit that has no such maps.  Every repeat goes to the JSON.

    python tools/clrrt_loop_rate.py [--reps 5] [--shared-only] [--out profiles/clrrt_loop_rates.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, SCALE, G, RES, THR = 1000, 1.4, 64, 0.5, 0.2


def rover_maps(fx, B):
    """(B, G, G): rover b's risk map, the fixture's times 0.8 + 0.05 (b mod 11)."""
    return np.stack([np.clip(fx["mean"] * np.float32(0.8 + 0.05 * (b % 11)), 0.0, 0.95) for b in range(B)]).astype(np.float32)


def make(fx, B, per_rover=False):
    from benchnav_amd import CLRRT, CLRRTLoop, NativeMPPI
    from benchnav_amd.env import BatchedPlanetaryEnv
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    mean = fx["mean"]
    pl = NativeMPPI(horizon=8, num_samples=64, grid_size=G, resolution=RES, num_instances=B, shared_map=True, stream=0, stuck_threshold=THR)
    lat = np.clip(mean * np.float32(SCALE), 0.0, 0.7).astype(np.float32)
    env = BatchedPlanetaryEnv(pl, lat, np.full((G, G), float(fx["std"]), np.float32), fx["start"], fx["goal"], delta_t=0.1, time_limit=100.0,
                              stuck_threshold=0.0, goal_threshold=1.0, seed=1)      # (the constructor's sampled collision check of the start, 2.3 % per
                                                                                    # rover at the planner's 0.2, would refuse a batch of 256; the loop does not read it)
    gm = FakeGridMap(G, RES)
    planner = CLRRT(3, 2, FakeDynamics(mean, gm), FakeObjectives(torch.as_tensor(fx["goal"].copy()), THR), gm, delta_t=0.1, max_iterations=60,
                    max_seqs=250, seed=42)
    kw = {"risk_maps": torch.from_numpy(rover_maps(fx, B)).cuda()} if per_rover else {}
    loop = CLRRTLoop(env, planner, seeds=[42 + b for b in range(B)], **kw)
    return env, planner, loop


def fused_run(env, loop):
    env.reset(seed=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    log = loop.run(N)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return wall, loop.follow_ms, log


def composed_run(env, planner):
    """The reference's loop on the host, B = 1: forward(), the torch deviation and env.step per control step."""
    env.reset(seed=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    state = env._robot_state
    plans = steps = 0
    t_plan = 0.0
    replan, idx = True, 0
    action_seq = state_seq = None
    for t in range(N):
        if t == 0 or replan:
            p0 = time.perf_counter()
            action_seq, state_seq = planner.forward(state[0])
            t_plan += time.perf_counter() - p0
            plans += 1
            if action_seq is None:
                break
            idx, replan = 0, False
        if t > 0:
            deviation = torch.min(torch.norm(state_seq[:, :, :2] - state[0, :2], dim=2))
            replan = bool(deviation > 1.0)
            if replan:
                continue
        if idx >= action_seq.shape[0]:
            break
        action = action_seq[idx:idx + 1]
        idx += 1
        state, reward, term, trunc = env.step(action)
        steps += 1
        if bool(term[0]) or trunc:
            break
    torch.cuda.synchronize()
    return time.perf_counter() - t0, t_plan, plans, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shared-only", action="store_true", help="only the cases in which every rover plans on the planner's one map")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clrrt_loop_rates.json"))
    args = ap.parse_args()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "clrrt_loop.npz"))
    rows = []
    cases = [(1, False), (64, False), (256, False)] + ([] if args.shared_only else [(64, True), (256, True)])
    for B, per_rover in cases:
        env, planner, loop = make(fx, B, per_rover)
        fused_run(env, loop)                                            # warm-up
        if B == 1:
            composed_run(env, planner)
        walls, follows, comp = [], [], []
        log = None
        for _ in range(args.reps):                                      # alternating runs
            w, f, log = fused_run(env, loop)
            walls.append(w); follows.append(f)
            if B == 1:
                comp.append(composed_run(env, planner))
        steps = int(log["steps"].max())
        wall, follow = float(np.median(walls)), float(np.median(follows))
        row = {"B": B, "maps": "per_rover" if per_rover else "shared", "iterations": N, "steps_max": steps, "plans_mean": round(float(log["plans"].mean()), 2), "plans_max": int(log["plans"].max()),
               "status_counts": np.bincount(log["status"], minlength=8).tolist(),
               "wall_us_per_iteration": round(1e6 * wall / N, 3), "wall_us_per_rover_iteration": round(1e6 * wall / N / B, 4),
               "follow_us_per_step": round(1e3 * follow / max(steps, 1), 3), "plan_share": round(1.0 - 1e-3 * follow / wall, 4),
               "wall_s_all": [round(w, 6) for w in walls], "follow_ms_all": [round(f, 4) for f in follows]}
        if B == 1:
            cw = float(np.median([c[0] for c in comp]))
            cp = float(np.median([c[1] for c in comp]))
            row["host_composed"] = {"wall_us_per_iteration": round(1e6 * cw / N, 3), "plan_share": round(cp / cw, 4),
                                    "us_per_step_without_plans": round(1e6 * (cw - cp) / max(comp[-1][3], 1), 3), "plans": comp[-1][2], "steps": comp[-1][3],
                                    "wall_s_all": [round(c[0], 6) for c in comp], "plan_s_all": [round(c[1], 6) for c in comp]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        loop.close()
    doc = {"what": "benchnav_amd.CLRRTLoop on the s = 1.4 case of tests/golden/clrrt_loop.npz, 1000 loop iterations, own planner seeds and Philox slip "
                   "draws: median of %d runs after a warm-up, every repeat listed; host_composed = CLRRT.forward + torch deviation + "
                   "BatchedPlanetaryEnv.step per control step at the same commit, in alternating runs" % args.reps,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
