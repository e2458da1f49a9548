#!/usr/bin/env python3
"""Rates of the dataset stage (benchnav_amd/dataset.py, csrc/dataset_kernels.hip) on one MI355X.  None of them is a pass
condition and nothing here is tuned: they say what the stage costs as it stands.

  generate   maps per second of DatasetGenerator.generate_dataset, memory only and with the reference's files written;
  load_data  one SlipRegressorTrainer.load_data on the device dataset (three launches over the split) against the generic loader
             path over the same files: a dataset that reads `torch.load`-ed items from disk and samples the latent model on the
             host, as the reference's SlipRegressionDataset does, through DataLoader and load_data's masking;
  classifier one epoch's DATA path (no training step): DataLoader batches of (colours, classes) from the device dataset against a
             dataset that reads each item's file, batches moved to the device.

Method: host clock around work that ends in a device synchronise; every measurement is warmed up once and repeated --reps times,
the figure is the median and the samples are kept.

    python tools/dataset_rate.py [--reps 5] [--environments 10] [--instances 100] [--grid-size 64] [--out profiles/dataset_rates.json]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    """seconds: (median, samples) of fn() + synchronise, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), [round(v, 5) for v in out]


class FileItems(torch.utils.data.Dataset):
    """The generic path: one file read per item (io.load_instance), in the sorted file order."""

    def __init__(self, folder, kind):
        self.paths = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f != "seed_information.pt")
        self.kind = kind

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from benchnav_amd.io import load_instance
        inst = load_instance(self.paths[i])
        if self.kind == "classification":
            return inst.tensors["colors"], inst.tensors["t_classes"]
        return inst.tensors["slopes"], torch.distributions.Normal(inst.latent_mean, inst.latent_std).sample(), inst.tensors["t_classes"]


class Params:
    batch_size, learning_rate, num_iterations = 16, 0.1, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--environments", type=int, default=10)
    ap.add_argument("--instances", type=int, default=100)       # 10 x 100: the reference's train split
    ap.add_argument("--grid-size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--num-samples", type=int, default=9999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_rates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dataset_rate.py needs an MI355X (gfx950) device")
    from benchnav_amd.dataset import DatasetGenerator, SlipRegressionDataset, TerrainClassificationDataset
    from benchnav_amd.gp import SlipRegressorTrainer
    from benchnav_amd.terrain import slip_models

    T, G, M = 10, args.grid_size, args.environments * args.instances
    models = slip_models(T)
    root = tempfile.mkdtemp(prefix="benchnav_dataset_rate_")
    work = tempfile.mkdtemp(prefix="benchnav_dataset_rate_models_")
    warnings.simplefilter("ignore")
    try:
        def generate(directory):
            return DatasetGenerator(models, directory, "train", G, 0.5, args.environments, args.instances, num_total_terrain_classes=T,
                                    num_selected_terrain_classes=4, batch=args.batch).generate_dataset()
        mem_s, mem_all = timed(lambda: generate(None), args.reps)
        file_s, file_all = timed(lambda: generate(root), args.reps)
        train = generate(root)
        folder = os.path.join(root, "train")

        dev = torch.device("cuda", torch.cuda.current_device())
        on_device = SlipRegressorTrainer(dev, work, work, T, Params(), SlipRegressionDataset(train))
        generic = SlipRegressorTrainer(dev, work, work, T, Params(), FileItems(folder, "regression"))
        dev_s, dev_all = timed(lambda: on_device.load_data(args.num_samples), args.reps)
        gen_s, gen_all = timed(lambda: generic.load_data(args.num_samples), args.reps)
        counts = [int(v.numel()) for v in on_device.load_data(args.num_samples)[0].values()]

        def epoch(dataset):
            n = 0
            for colors, classes in torch.utils.data.DataLoader(dataset, batch_size=args.batch, shuffle=True):
                n += colors.to(dev).shape[0] + 0 * classes.to(dev).shape[0]
            return n
        cdev_s, cdev_all = timed(lambda: epoch(TerrainClassificationDataset(train)), args.reps)
        cfile_s, cfile_all = timed(lambda: epoch(FileItems(folder, "classification")), args.reps)
    finally:
        shutil.rmtree(root, ignore_errors=True)
        shutil.rmtree(work, ignore_errors=True)
    out = {"what": "benchnav_amd.dataset on one MI355X: host clock around work that ends in a device synchronise, one warm-up, median of "
                   f"{args.reps} samples.  Not a pass condition; nothing is tuned.",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "maps": M, "grid_size": G, "batch": args.batch,
           "generate": {"memory_only_maps_per_s": round(M / mem_s, 1), "with_files_maps_per_s": round(M / file_s, 1),
                        "memory_only_s": round(mem_s, 4), "with_files_s": round(file_s, 4), "samples_s": {"memory_only": mem_all, "with_files": file_all}},
           "load_data": {"num_samples": args.num_samples, "points_per_class": counts, "device_gather_s": round(dev_s, 5),
                         "generic_loader_over_files_s": round(gen_s, 4), "generic_over_device": round(gen_s / dev_s, 1),
                         "samples_s": {"device_gather": dev_all, "generic_loader": gen_all}},
           "classifier_epoch_data_path": {"device_dataset_s": round(cdev_s, 5), "files_read_per_item_s": round(cfile_s, 4),
                                          "files_over_device": round(cfile_s / cdev_s, 1), "samples_s": {"device_dataset": cdev_all, "files": cfile_all}}}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
