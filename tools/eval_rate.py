#!/usr/bin/env python3
"""What the evaluation stage costs: Evaluator.run for 64 maps of 64 x 64 and of 256 x 256 against the two figures that
tools/make_models.py composed from torch ops before the stage existed -- per map, the mean absolute error of the slip mean and the
pixel accuracy, each read back with a host synchronise.

    python tools/eval_rate.py            # -> profiles/eval_rates.json

Both sides start from the same device arrays (a synthetic split: the predictions and the predicted classes are given, so that
neither side pays for a model).  Evaluator.run computes far more than the two figures: the confusion matrix, eight sums and two
counts per (class, slope bin), the slip observations they need, and one download.  `kernels_ms` is its three launches alone
(confusion_matrix and slip_metrics on all 64 maps).  Host clock to a device synchronise, medians of 5, the two sides alternating;
measured once, not a pass condition."""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MAPS, CLASSES, REPEATS = 64, 10, 5


class _Given:
    """predict_classes and predict_maps that hand out stored device arrays, in the evaluator's map order."""
    terrain_classifier = None

    def __init__(self, classes, mean, std):
        self.classes, self.mean, self.std, self.at, self.at_maps = classes, mean, std, 0, 0

    def predict_classes(self, colors):
        B = colors.shape[0]
        out = self.classes[self.at:self.at + B]
        self.at = (self.at + B) % self.classes.shape[0]
        return out

    def predict_maps(self, slopes, colors=None):
        B = slopes.shape[0]
        out = self.mean[self.at_maps:self.at_maps + B], self.std[self.at_maps:self.at_maps + B]
        self.at_maps = (self.at_maps + B) % self.mean.shape[0]
        return out


def split_of(G: int):
    from benchnav_amd.dataset import TerrainDataset
    g = torch.Generator(device="cuda").manual_seed(G)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=g)
    classes = torch.randint(0, CLASSES, (MAPS, G, G), device="cuda", generator=g, dtype=torch.int32)
    data = TerrainDataset(torch.zeros(MAPS, G, G, device="cuda"), 30.0 * rand(MAPS, G, G), 0.1 + 0.6 * rand(MAPS, G, G), 0.02 + 0.1 * rand(MAPS, G, G),
                          rand(MAPS, 3, G, G), classes, list(range(MAPS)))
    wrong = rand(MAPS, G, G) < 0.1
    pred = torch.where(wrong, torch.randint(0, CLASSES, (MAPS, G, G), device="cuda", generator=g, dtype=torch.int32), classes)
    mean = data.latent_mean + 0.05 * (rand(MAPS, G, G) - 0.5)
    std = data.latent_std * (0.5 + rand(MAPS, G, G))
    return data, pred, mean, std


def rates(G: int) -> dict:
    from benchnav_amd.evaluate import Evaluator, confusion_matrix, slip_metrics
    data, pred, mean, std = split_of(G)
    given = _Given(pred, mean, std)
    ev = Evaluator(data, predictor=given, classifier=given, num_classes=CLASSES, chunk=MAPS)

    def torch_ops():                                    # tools/make_models.py step 5 before the stage: two figures, two synchronises per map
        mean_err, pixel_acc = [], []
        for m in range(MAPS):
            mean_err.append(float((mean[m] - data.latent_mean[m]).abs().mean()))
            pixel_acc.append(float((pred[m].to(torch.int64) == data.classes(m)).float().mean()))
        return sum(mean_err) / MAPS, sum(pixel_acc) / MAPS

    def kernels():
        confusion_matrix(pred, data.t_classes, CLASSES)
        slip_metrics(mean, std, data.latent_mean, data.latent_std, data.t_classes, data.slopes, CLASSES)

    sides = {"evaluator_run_ms": ev.run, "kernels_ms": kernels, "torch_ops_ms": torch_ops}
    times = {k: [] for k in sides}
    for fn in sides.values():                           # warm-up: allocator, first launches
        fn()
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for k, fn in sides.items():                     # alternating
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    report, (mae, acc) = ev.run(), torch_ops()
    cl, sl = report.summary()["classification"], report.summary()["slip"]
    n = sum(r["count"] for r in sl["per_class"])
    row = {k: round(statistics.median(v), 3) for k, v in times.items()}
    row.update({"maps": MAPS, "grid_size": G, "classes": CLASSES,
                "pixel_accuracy": {"evaluator": cl["pixel_accuracy"], "torch_ops": acc},
                "mean_abs_error": {"evaluator": sum(r["mae"] * r["count"] for r in sl["per_class"] if r["count"]) / n, "torch_ops": mae}})
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_rate.py needs an MI355X (gfx950) device")
    doc = {"device": torch.cuda.get_device_name(0),
           "method": "host clock to a device synchronise, medians of 5, alternating; measured once, not a pass condition",
           "rows": [rates(64), rates(256)]}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "eval_rates.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
