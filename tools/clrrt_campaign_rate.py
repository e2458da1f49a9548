#!/usr/bin/env python3
"""Wall time of a CL-RRT benchmark campaign chunk: 64 episodes (64 seeded 64 x 64 maps at 0.5 m, one trial each, the latent model as
the prediction, start (8, 8), goal (24, 24), a 100 s limit: 1001 control steps, 2002 loop iterations) under three risk settings.
  campaign        Benchmark.run("cl_rrt", settings): risk maps, per-rover maps set device to device, CLRRTLoop.run(log=False),
                  scores from the loop's device views; the whole call / the number of settings
  hand_composed   the same chunk from the parts: one CLRRTLoop per setting on its rovers' maps, loop.run with its host log, the
                  NumPy spec of tests/benchmark_spec.py with benchmark.clrrt_outcome_words; per setting, the run and the scoring
                  apart (the risk maps and the environment are made once, outside the clock)
Host clock between device synchronisations, median of --reps after a warm-up, every repeat listed.  Measured once, not a pass
condition.

    python tools/clrrt_campaign_rate.py [--reps 3] [--max-iterations 500] [--max-seqs 250] [--out profiles/clrrt_campaign_rates.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

G, RES, M, SEED = 64, 0.5, 64, 0
DT, LIMIT, THR, GOAL_THR = 0.1, 100.0, 0.1, 1.0
SETTINGS = ["expected_value", "var@0.9", "cvar@0.9"]
START, GOAL = (8.0, 8.0), (24.0, 24.0)


def latent():
    from benchnav_amd import synth
    f32 = np.float32
    mean = np.stack([(f32(0.3) + f32(0.2) * synth.smooth_risk_map(G, 100 + m).numpy() / f32(0.95)).astype(f32) for m in range(M)])
    return mean, np.full((M, G, G), 0.03, f32)


def bench_for(mean, std):
    from benchnav_amd.benchmark import Benchmark
    from benchnav_amd.dataset import TerrainDataset
    zeros = torch.zeros(M, G, G, device="cuda")
    ds = TerrainDataset(zeros.clone(), zeros.clone(), torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda(),
                        torch.zeros(M, 3, G, G, device="cuda"), torch.zeros(M, G, G, dtype=torch.int32, device="cuda"), seeds=list(range(M)))
    return Benchmark(ds, None, start_pos=START, goal_pos=GOAL, delta_t=DT, time_limit=LIMIT, stuck_threshold=THR, goal_threshold=GOAL_THR,
                     trials=1, chunk=M, seed=SEED, resolution=RES)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=500)
    ap.add_argument("--max-seqs", type=int, default=250)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clrrt_campaign_rates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clrrt_campaign_rate.py needs an MI355X (gfx950) device")
    import benchmark_spec as S
    from benchnav_amd import CLRRT, CLRRTLoop, NativeMPPI
    from benchnav_amd.benchmark import OUTCOMES, clrrt_iterations, clrrt_outcome_words, planner_seed
    from benchnav_amd.env import BatchedPlanetaryEnv
    kw = dict(max_iterations=args.max_iterations, max_seqs=args.max_seqs)
    mean, std = latent()
    bench = bench_for(mean, std)
    rows = clrrt_iterations(bench.max_steps)

    # ---- the campaign ----
    bench.run("cl_rrt", SETTINGS, **kw)                                             # warm-up
    walls, report = [], None
    for _ in range(args.reps):
        w, report = timed(lambda: bench.run("cl_rrt", SETTINGS, **kw))
        walls.append(w)
    campaign = {"wall_s": round(statistics.median(walls), 4), "wall_s_per_setting": round(statistics.median(walls) / len(SETTINGS), 4),
                "wall_s_all": [round(w, 4) for w in walls],
                "outcome_counts": [{name: int((report.outcome[c] == code).sum()) for code, name in enumerate(OUTCOMES)} for c in range(len(SETTINGS))],
                "plans_mean": [round(float(report.plans[c].mean()), 2) for c in range(len(SETTINGS))],
                "steps_mean": [round(float(report.steps[c].mean()), 1) for c in range(len(SETTINGS))]}
    print(json.dumps({"campaign": campaign}), flush=True)

    # ---- the same chunk by hand ----
    risk = bench.risk_maps(SETTINGS)
    goals = np.broadcast_to(np.float32(GOAL), (M, 2)).copy()
    rrt = CLRRT.from_parameters(G, RES, stuck_threshold=THR, delta_t=DT, goal_threshold=GOAL_THR, seed=SEED, **kw)
    run_s, score_s, same = [[] for _ in SETTINGS], [[] for _ in SETTINGS], True
    with NativeMPPI(grid_size=G, resolution=RES, num_instances=M, shared_map=False, stuck_threshold=THR, horizon=8, num_samples=64,
                    stream=torch.cuda.current_stream().cuda_stream) as pl:
        env = BatchedPlanetaryEnv(pl, mean, std, START, GOAL, delta_t=DT, time_limit=LIMIT, stuck_threshold=THR, goal_threshold=GOAL_THR, seed=SEED,
                                  freeze_on_goal=True, check_positions=False)
        for rep in range(args.reps + 1):                                            # the first is the warm-up
            for c in range(len(SETTINGS)):
                def episode():
                    loop = CLRRTLoop(env, rrt, seeds=[planner_seed(SEED, e) for e in range(M)], risk_maps=risk[c])
                    env.reset(seed=SEED)
                    log = loop.run(rows)
                    loop.close()
                    return log
                w, log = timed(episode)
                t0 = time.perf_counter()
                done, stopped = clrrt_outcome_words(log["status"], log["done_iter"])
                got = S.score_episodes(log["states"], log["rewards"], goals, None, done, stopped, None, THR, DT)
                ws = time.perf_counter() - t0
                if rep:
                    run_s[c].append(w)
                    score_s[c].append(ws)
                    valid = report.outcome[c, :, 0] != 3                            # the hand-composed chunk makes no collision draws
                    same = same and bool((got["steps"][valid] == report.steps[c, :, 0][valid]).all())
    med = lambda v: statistics.median(v)
    run_total, score_total = sum(med(v) for v in run_s), sum(med(v) for v in score_s)      # over the settings, each at its median
    hand = {"wall_s": round(run_total + score_total, 4), "wall_s_per_setting": round((run_total + score_total) / len(SETTINGS), 4),
            "run_with_host_log_s": round(run_total, 4), "numpy_spec_s": round(score_total, 4),
            "run_s_all": [[round(w, 4) for w in v] for v in run_s], "score_s_all": [[round(w, 4) for w in v] for v in score_s],
            "steps_equal_to_campaign": same}
    doc = {"what": "a 64-episode CL-RRT campaign chunk (64 maps of 64 x 64 cells at 0.5 m, one trial, start (8, 8), goal (24, 24), 100 s limit = 1001 "
                   "steps = %d loop iterations, max_iterations %d, max_seqs %d) under %d settings: host clock between device synchronisations, "
                   "median of %d after a warm-up, every repeat listed; measured once, not a pass condition" % (rows, args.max_iterations, args.max_seqs,
                                                                                                                 len(SETTINGS), args.reps),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "settings": SETTINGS, "campaign": campaign, "hand_composed": hand}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"hand_composed": hand}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
