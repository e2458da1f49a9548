#!/usr/bin/env python3
"""From seeds to trained models in one run, end to end on the device: what the reference spreads over
scripts/generate_terrain_dataset.py, scripts/train_terrain_classifier.py and scripts/train_slip_regressors.py.

  1. DatasetGenerator: the train, valid and test (subset 1) splits, in memory and, with --data-directory, as the reference's files;
  2. ClassifierTrainer on TerrainClassificationDataset(train / valid)  -> <out>/classifier/.../models/best_model.pth;
  3. SlipRegressorTrainer on SlipRegressionDataset(train)              -> <out>/regressors/.../models/NN_class.pth and
                                                                          <out>/slip_observations/NN_class.pth;
  4. load_terrain_classifier + load_slip_regressors read both back;
  5. TraversabilityPredictor.predict: a Normal of (G, G) per map; Evaluator.run on the test split: the classifier's confusion matrix, the
     regressors' errors against the latent model per class and slope bin, the risk maps' calibration (tools/evaluate_models.py).

    python tools/make_models.py --out /tmp/models [--grid-size 64] [--environments 10] [--train-instances 8] [--epochs 2] [--iterations 20]

The defaults are small (a minute or so on one MI355X); the reference's sizes are --environments 10 --train-instances 100
--valid-instances 10 --test-instances 10 --epochs 100 --iterations 100 --num-samples 9999."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="directory for the models (default: a temporary directory)")
    ap.add_argument("--data-directory", default=None, help="also write the splits as the reference's files here")
    ap.add_argument("--grid-size", type=int, default=64)
    ap.add_argument("--resolution", type=float, default=0.5)
    ap.add_argument("--environments", type=int, default=10)
    ap.add_argument("--train-instances", type=int, default=8)
    ap.add_argument("--valid-instances", type=int, default=2)
    ap.add_argument("--test-instances", type=int, default=1)
    ap.add_argument("--total-classes", type=int, default=10)
    ap.add_argument("--selected-classes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16, help="maps per generation launch")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=16, help="the classifier's batch size")
    ap.add_argument("--learning-rate", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--iterations", type=int, default=20, help="Adam steps per slip regressor")
    ap.add_argument("--regressor-learning-rate", type=float, default=0.1)
    ap.add_argument("--num-samples", type=int, default=1000, help="training points per slip regressor (the reference: 9999)")
    ap.add_argument("--seed", type=int, default=0, help="torch.manual_seed: the loaders' and the gather's orders, the classifier's weights")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/make_models.py needs an MI355X (gfx950) device")
    from benchnav_amd.dataset import DatasetGenerator, SlipRegressionDataset, TerrainClassificationDataset, TraversabilityPredictionDataset
    from benchnav_amd.evaluate import Evaluator
    from benchnav_amd.gp import SlipRegressorTrainer, TraversabilityPredictor, load_slip_regressors
    from benchnav_amd.terrain import slip_models
    from benchnav_amd.unet import load_terrain_classifier
    from benchnav_amd.unet_train import ClassifierTrainer, init_state_dict

    out = args.out or tempfile.mkdtemp(prefix="benchnav_models_")
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    T = args.total_classes
    models = slip_models(T)
    torch.manual_seed(args.seed)
    times = {}

    def generate(split, instances, info, subset=None):
        gen = DatasetGenerator(models, args.data_directory, split, args.grid_size, args.resolution, args.environments, instances,
                               num_total_terrain_classes=T, num_selected_terrain_classes=args.selected_classes, subset_index=subset,
                               batch=args.batch, seed_information=info)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return gen.generate_dataset()

    t0 = time.perf_counter()
    train = generate("train", args.train_instances, None)
    valid = generate("valid", args.valid_instances, train.seed_information)
    test = generate("test", args.test_instances, valid.seed_information, subset=1)
    torch.cuda.synchronize()
    times["generate_s"] = time.perf_counter() - t0
    print(f"splits: train {len(train)} maps (seeds {int(train.seeds[0])}..{int(train.seeds[-1])}), valid {len(valid)}, test {len(test)}")

    t0 = time.perf_counter()
    p = Params(batch_size=args.batch_size, learning_rate=args.learning_rate, weight_decay=args.weight_decay, num_epochs=args.epochs, classes=T, device=dev)
    clf_trainer = ClassifierTrainer(init_state_dict(T, seed=args.seed), os.path.join(out, "classifier"), p, TerrainClassificationDataset(train),
                                    TerrainClassificationDataset(valid))
    clf_trainer.train()
    clf_trainer.model.close()
    times["classifier_s"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    q = Params(batch_size=args.batch_size, learning_rate=args.regressor_learning_rate, num_iterations=args.iterations)
    reg_trainer = SlipRegressorTrainer(dev, os.path.join(out, "regressors"), out, T, q, SlipRegressionDataset(train))
    phis, slips = reg_trainer.load_data(num_samples=args.num_samples)
    for k in range(T):
        reg_trainer.train(k, phis[k], slips[k])
    times["regressors_s"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    classifier = load_terrain_classifier(os.path.join(clf_trainer.model_saving_path, "best_model.pth"), classes=T, device=dev)
    regressors = load_slip_regressors(T, reg_trainer.model_directory, out, device=dev)
    predictor = TraversabilityPredictor(classifier, regressors, device=dev)
    view = TraversabilityPredictionDataset(test)
    colors, slopes, _, _ = view[0]
    pred = predictor.predict(colors, slopes)
    assert isinstance(pred, torch.distributions.Normal) and tuple(pred.mean.shape) == (args.grid_size, args.grid_size)
    # every map of the test split through the evaluation stage: one pass on the device, one download (benchnav_amd/evaluate.py)
    evaluation = Evaluator(test, predictor, num_classes=T, seed=args.seed).run(["expected_value", "var@0.9", "cvar@0.9"])
    pixel_accuracy = evaluation.summary()["classification"]["pixel_accuracy"]
    rows = [r for r in evaluation.summary()["slip"]["per_class"] if r["count"]]
    mean_abs_error = sum(r["mae"] * r["count"] for r in rows) / sum(r["count"] for r in rows) if rows else None
    times["predict_s"] = time.perf_counter() - t0
    report = {"out": out, "maps": {"train": len(train), "valid": len(valid), "test": len(test)}, "grid_size": args.grid_size,
              "classifier": {"epochs": args.epochs, "train_loss": clf_trainer.history["train_epoch"], "valid_loss": clf_trainer.history["valid_epoch"],
                             "test_pixel_accuracy": pixel_accuracy},
              "regressors": {"iterations": args.iterations, "points": [int(phis[k].numel()) for k in range(T)]},
              "prediction": {"shape": [args.grid_size, args.grid_size], "mean_abs_error_of_the_slip_mean": mean_abs_error},
              "evaluation": evaluation.to_dict(),
              "seconds": {k: round(v, 3) for k, v in times.items()}}
    print(json.dumps(report))
    print(evaluation.table())
    print(f"predict: Normal(mean, std) of shape ({args.grid_size}, {args.grid_size}) for {len(view)} test maps")


if __name__ == "__main__":
    main()
