#!/usr/bin/env python3
"""The benchmark stage end to end on the device: a test split, its predictions, risk maps under three risk settings, a planner
driving every map, and the summary table -- what the reference spreads over its test_*.py drivers, one map at a time.

    python tools/run_benchmark.py [--planner mppi|astar_dwa|cl_rrt] [--data-directory DIR | --grid-size 64 --environments 10 --test-instances 1]
                                  [--models DIR] [--trials 1] [--chunk 64] [--seed 0] [--out report.json]
                                  [--max-iterations 500] [--max-seqs 250]                                    # cl_rrt
                                  [--tasks sampled [--min-separation 10] [--connectivity 4] [--kappa 0] [--task-seed 0]]
    python tools/run_benchmark.py --rates [--baseline-lib libbenchnav_mppi.so]      # -> profiles/benchmark_rates.json

The split is test subset 1: read from --data-directory (the reference's files), or generated in memory with the seeds
tools/make_models.py's chain reaches (--train-instances / --valid-instances say how far the chain has run).  --models is the --out
directory of tools/make_models.py (its classifier and slip regressors predict the slip); without it the latent model is the
predictor.  --tasks sampled draws every episode's start and goal inside one connected region of the latent model's passable ground
(benchnav_amd/tasks.py) instead of --start / --goal, and the table gains an `spl` column.  --rates measures the two new device operations instead (host clock to a device synchronise, medians of 5):
infer_risk_maps against one infer_risk_map call per map and setting -- through --baseline-lib, a library built from another
commit, when one is given -- and the scoring of 4096 episodes of 1001 steps from the device views against the log download plus the
NumPy spec of tests/benchmark_spec.py."""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SETTINGS = ["expected_value", "var@0.9", "cvar@0.9"]


def load_split(args):
    from benchnav_amd.dataset import DatasetGenerator, TerrainDataset
    from benchnav_amd.terrain import slip_models
    if args.data_directory and os.path.isdir(os.path.join(args.data_directory, "test", f"subset{args.subset:02d}")):
        return TerrainDataset.from_directory(args.data_directory, "test", args.subset, device="cuda")
    info = {"environment_seed": 0, "last_instance_seed": args.environments * (args.train_instances + args.valid_instances)}
    gen = DatasetGenerator(slip_models(args.total_classes), None, "test", args.grid_size, args.resolution, args.environments, args.test_instances,
                           num_total_terrain_classes=args.total_classes, num_selected_terrain_classes=args.selected_classes, subset_index=1,
                           batch=args.batch, seed_information=info)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return gen.generate_dataset()


def load_predictor(models: str, classes: int, dev):
    from benchnav_amd.gp import TraversabilityPredictor, load_slip_regressors
    from benchnav_amd.unet import load_terrain_classifier

    def only(pattern):
        found = sorted(glob.glob(os.path.join(models, pattern), recursive=True))
        if not found:
            raise SystemExit(f"--models {models}: nothing matches {pattern}")
        return found[-1]
    classifier = load_terrain_classifier(only("classifier/**/best_model.pth"), classes=classes, device=dev)
    model_directory = os.path.dirname(os.path.dirname(only("regressors/**/models/00_class.pth")))
    return TraversabilityPredictor(classifier, load_slip_regressors(classes, model_directory, models, device=dev), device=dev)


def median_ms(fn, repeats=5):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def risk_rates(baseline_lib):
    from benchnav_amd import _capi
    from benchnav_amd.risk import _METRICS, infer_risk_maps
    from benchnav_amd.benchmark import parse_setting
    M, G, n = 64, 256, 1000
    g = torch.Generator().manual_seed(0)
    mean = (0.1 + 0.5 * torch.rand(M, G, G, generator=g)).cuda()
    std = (0.02 + 0.1 * torch.rand(M, G, G, generator=g)).cuda()
    out = torch.empty(G, G, device="cuda")
    base = _capi.load()
    if baseline_lib:
        base = C.CDLL(baseline_lib)
        base.bn_risk_map_infer.restype, base.bn_risk_map_infer.argtypes = _capi.SYMBOLS["bn_risk_map_infer"]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def singles(settings):
        for metric, q in settings:
            for m in range(M):
                rc = base.bn_risk_map_infer(0, stream, C.c_void_p(mean[m].data_ptr()), C.c_void_p(std[m].data_ptr()), _capi.BN_MEM_DEVICE, G,
                                            _METRICS[metric], float(q or 0.0), n, None, _capi.BN_MEM_DEVICE, m, C.c_void_p(out.data_ptr()),
                                            _capi.BN_MEM_DEVICE)
                assert rc == 0, rc
    rows = {}
    for name, names in (("expected_value, var@0.9, cvar@0.9", SETTINGS), ("var@0.9, cvar@0.95, var@0.5", ["var@0.9", "cvar@0.95", "var@0.5"])):
        settings = [parse_setting(s) for s in names]
        batched = median_ms(lambda: infer_risk_maps(mean, std, settings, num_samples=n, seeds=list(range(M))))
        single = median_ms(lambda: singles(settings))
        rows[name] = {"infer_risk_maps_ms": round(batched, 3), "single_calls": M * len(settings), "single_calls_ms": round(single, 3),
                      "ratio": round(single / batched, 2)}
    return {"maps": M, "grid_size": G, "num_samples": n, "single_call_kernel": "the library given as --baseline-lib" if baseline_lib else
            "this build's risk_map_kernel", "settings": rows}


def score_rates():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import benchmark_spec as S
    from benchnav_amd import NativeMPPI
    from benchnav_amd.benchmark import _empty_scores, _score_pointers
    from benchnav_amd.env import BatchedPlanetaryEnv
    B, n, G, res = 4096, 1001, 64, 0.5
    g = torch.Generator().manual_seed(1)
    mean = (0.2 + 0.3 * torch.rand(G, G, generator=g)).numpy()
    std = np.full((G, G), 0.05, np.float32)
    starts = (4.0 + 8.0 * torch.rand(B, 2, generator=g)).numpy()
    goals = (18.0 + 10.0 * torch.rand(B, 2, generator=g)).numpy()
    dev = torch.device("cuda", torch.cuda.current_device())
    with NativeMPPI(horizon=10, num_samples=64, grid_size=G, resolution=res, num_instances=B, shared_map=True, stuck_threshold=0.1,
                    overlap=False, stream=torch.cuda.current_stream().cuda_stream) as pl:
        pl.set_map(mean)
        env = BatchedPlanetaryEnv(pl, mean, std, starts, goals, freeze_on_goal=True, check_positions=False)
        env.reset(seed=0)
        t0 = time.perf_counter()
        env.run(n, log=False)
        torch.cuda.synchronize()
        episode_ms = (time.perf_counter() - t0) * 1e3
        states, rewards, done, _, _ = pl.episode_buffers()
        out = _empty_scores(B, dev)
        device_ms = median_ms(lambda: _score_pointers(dev, n, B, states, rewards, env._goal_pos.data_ptr(), None, done, None, None, 0.1, 0.1, out))
        download_ms = median_ms(pl.episode_log)
        st, rw, dn = pl.episode_log()
        t0 = time.perf_counter()
        want = S.score_episodes(st, rw, goals, None, dn, None, None, 0.1, 0.1)
        spec_ms = (time.perf_counter() - t0) * 1e3                       # one pass: a Python loop over 4.1 M rows
        got = {k: v.cpu().numpy() for k, v in out.items()}
        exact = all(np.array_equal(got[k], want[k], equal_nan=True) for k in ("outcome", "steps", "time", "reward_min", "stuck_steps"))
        within = all((np.abs(got[k] - want[k]) <= S.metric_bound(want[k], n)).all() for k in ("path_length", "reward_sum", "final_distance"))
    return {"episodes": B, "steps": n, "episode_ms": round(episode_ms, 1), "score_from_device_views_ms": round(device_ms, 3),
            "log_download_ms": round(download_ms, 3), "numpy_spec_ms_one_pass": round(spec_ms, 1),
            "ratio": round((download_ms + spec_ms) / device_ms, 1), "goal_episodes": int((want["outcome"] == S.GOAL).sum()),
            "equal_to_spec": bool(exact and within)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--planner", default="mppi", choices=["mppi", "astar_dwa", "cl_rrt"])
    ap.add_argument("--data-directory", default=None, help="read test/subsetNN from the reference's files here")
    ap.add_argument("--subset", type=int, default=1)
    ap.add_argument("--models", default=None, help="the --out directory of tools/make_models.py; default: the latent model predicts")
    ap.add_argument("--grid-size", type=int, default=64)
    ap.add_argument("--resolution", type=float, default=0.5)
    ap.add_argument("--environments", type=int, default=10)
    ap.add_argument("--train-instances", type=int, default=8)
    ap.add_argument("--valid-instances", type=int, default=2)
    ap.add_argument("--test-instances", type=int, default=1)
    ap.add_argument("--total-classes", type=int, default=10)
    ap.add_argument("--selected-classes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16, help="maps per generation launch")
    ap.add_argument("--start", type=float, nargs=2, default=None, help="x y in metres (default: 0.2 of the extent)")
    ap.add_argument("--goal", type=float, nargs=2, default=None, help="x y in metres (default: 0.8 of the extent)")
    ap.add_argument("--time-limit", type=float, default=100.0)
    ap.add_argument("--trials", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=None)
    ap.add_argument("--num-samples", type=int, default=None, help="MPPI rollouts per solve")
    ap.add_argument("--max-iterations", type=int, default=None, help="cl_rrt: samples per plan (the reference's 500)")
    ap.add_argument("--max-seqs", type=int, default=None, help="cl_rrt: closed-loop steps per steer (the reference's 250)")
    ap.add_argument("--tasks", default="fixed", choices=["fixed", "sampled"], help="fixed: --start / --goal for every map; sampled: a TaskSet")
    ap.add_argument("--min-separation", type=float, default=None, help="--tasks sampled: metres between start and goal at least (default: 0.3 of the extent)")
    ap.add_argument("--connectivity", type=int, default=4, choices=[4, 8], help="--tasks sampled: of the regions a pair must share")
    ap.add_argument("--kappa", type=float, default=0.0, help="--tasks sampled: passable is judged at the latent slip mean + kappa std")
    ap.add_argument("--task-seed", type=int, default=0, help="--tasks sampled: the seed of the draws")
    ap.add_argument("--out", default=None, help="write the report (per-episode arrays and summary) as JSON")
    ap.add_argument("--rates", action="store_true", help="measure the risk-map and scoring kernels instead -> profiles/benchmark_rates.json")
    ap.add_argument("--baseline-lib", default=None, help="--rates: time the single-map calls through this library (another commit's build)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/run_benchmark.py needs an MI355X (gfx950) device")
    if args.rates:
        rates = {"device": torch.cuda.get_device_name(0), "method": "host clock to a device synchronise, medians of 5; measured once, not a pass condition",
                 "risk_maps": risk_rates(args.baseline_lib), "scores": score_rates()}
        path = os.path.join(ROOT, "profiles", "benchmark_rates.json")
        with open(path, "w") as f:
            json.dump(rates, f, indent=1)
            f.write("\n")
        print(json.dumps(rates))
        return
    from benchnav_amd.benchmark import Benchmark
    split = load_split(args)
    dev = split.device
    predictor = load_predictor(args.models, args.total_classes, dev) if args.models else None
    extent = split.grid_size * args.resolution
    start = args.start or (0.2 * extent, 0.2 * extent)
    goal = args.goal or (0.8 * extent, 0.8 * extent)
    tasks = None
    if args.tasks == "sampled":
        from benchnav_amd.tasks import TaskSet
        tasks = TaskSet.sample(split, args.trials, args.task_seed, min_separation=0.3 * extent if args.min_separation is None else args.min_separation,
                               connectivity=args.connectivity, kappa=args.kappa, resolution=args.resolution, chunk=args.chunk)
        print(f"tasks: {int(tasks.valid.sum())} of {tasks.valid.size} pairs found, mean optimal length "
              f"{float(np.mean(tasks.optimal_length[tasks.valid])) if tasks.valid.any() else float('nan'):.2f} m")
    bench = Benchmark(split, predictor, start_pos=start, goal_pos=goal, time_limit=args.time_limit, trials=args.trials, chunk=args.chunk,
                      seed=args.seed, resolution=args.resolution, tasks=tasks)
    kw = {k: v for k, v in (("horizon", args.horizon), ("num_samples", args.num_samples)) if v is not None}
    if args.planner == "astar_dwa":
        kw.pop("num_samples", None)
    if args.planner == "cl_rrt":
        kw = {k: v for k, v in (("max_iterations", args.max_iterations), ("max_seqs", args.max_seqs)) if v is not None}
    t0 = time.perf_counter()
    report = bench.run(args.planner, SETTINGS, **kw)
    seconds = time.perf_counter() - t0
    print(f"{args.planner}: {len(split)} maps x {args.trials} trials x {len(SETTINGS)} settings, {bench.max_steps} steps each, "
          f"{'trained models' if predictor else 'latent model'} as predictor, {seconds:.2f} s")
    print(report.table())
    if args.out:
        report.to_json(args.out)


if __name__ == "__main__":
    main()
