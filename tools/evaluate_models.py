#!/usr/bin/env python3
"""How good are the trained models?  The evaluation stage on a test split: the classifier's confusion matrix, the slip regressors'
bias / error / calibration per terrain class and slope bin, and how the risk maps built on them compare with the slip the
environment would draw (benchnav_amd/evaluate.py) -- the numbers behind the reference's eyeball-only
scripts/test_terrain_classifier.py and scripts/test_slip_regressors.py.

    python tools/evaluate_models.py [--models DIR] [--data-directory DIR | --grid-size 64 --environments 10 --test-instances 1]
                                    [--settings expected_value var@0.9 cvar@0.9] [--chunk 64] [--bins 6] [--max-slope 30] [--seed 0]
                                    [--out evaluation.json]

The split is test subset 1, read or generated as tools/run_benchmark.py does; --models is the --out directory of
tools/make_models.py, loaded as its step 4 does.  Without --models the latent model is the prediction (every error is 0: a check
of the pipeline, and of the risk settings' calibration alone) and no confusion matrix is made."""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--models", default=None, help="the --out directory of tools/make_models.py; default: the latent model predicts")
    ap.add_argument("--data-directory", default=None, help="read test/subsetNN from the reference's files here")
    ap.add_argument("--subset", type=int, default=1)
    ap.add_argument("--grid-size", type=int, default=64)
    ap.add_argument("--resolution", type=float, default=0.5)
    ap.add_argument("--environments", type=int, default=10)
    ap.add_argument("--train-instances", type=int, default=8)
    ap.add_argument("--valid-instances", type=int, default=2)
    ap.add_argument("--test-instances", type=int, default=1)
    ap.add_argument("--total-classes", type=int, default=10)
    ap.add_argument("--selected-classes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16, help="maps per generation launch")
    ap.add_argument("--settings", nargs="*", default=["expected_value", "var@0.9", "cvar@0.9"], help="risk settings to calibrate (none: skip the risk maps)")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--bins", type=int, default=6)
    ap.add_argument("--max-slope", type=float, default=30.0)
    ap.add_argument("--stuck-threshold", type=float, default=0.1)
    ap.add_argument("--num-samples", type=int, default=1000, help="samples per cell of the risk maps")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the report (tables and figures) as JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/evaluate_models.py needs an MI355X (gfx950) device")
    from run_benchmark import load_predictor, load_split
    from benchnav_amd.evaluate import Evaluator
    split = load_split(args)
    predictor = load_predictor(args.models, args.total_classes, split.device) if args.models else None
    ev = Evaluator(split, predictor, num_classes=args.total_classes, chunk=args.chunk, bins=args.bins, max_slope=args.max_slope,
                   stuck_threshold=args.stuck_threshold, seed=args.seed, num_samples=args.num_samples)
    t0 = time.perf_counter()
    report = ev.run(args.settings)
    seconds = time.perf_counter() - t0
    print(f"{len(split)} maps of {split.grid_size} x {split.grid_size}, {'trained models' if predictor else 'latent model'} as predictor, "
          f"{len(args.settings)} risk settings, {seconds:.2f} s")
    print(report.table())
    if args.out:
        report.to_json(args.out)


if __name__ == "__main__":
    main()
