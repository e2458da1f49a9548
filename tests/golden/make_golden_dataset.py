#!/usr/bin/env python3
"""Generate the dataset-layout fixture by importing the reference (build container only).

Drives the *unmodified* reference DatasetGenerator (src/data/dataset_generator.py) in-process, without its worker pool, through
train -> valid -> test subset 1 -> test subset 2 with environment_count = 3 and instance counts 4 / 2 / 2: `set_seed`,
`generate_occupancy_distribution` and `generate_and_save_environment_group` are the reference's own; `generate_map_instance` is
replaced by a stub that only records the seed and the occupancy row it was called with (no map is generated), and the split's
seed_information.pt is written with the two keys generate_dataset writes (:131-152), because that method itself cannot run
without the pool.  Recorded per split in tests/golden/dataset_layout.json: the seed information, and for every file its name
relative to the data directory, its seed and its occupancy row.

Recipe of make_golden_colouring.py: the reference's src and root on sys.path, `opensimplex` stubbed, `tqdm` stubbed if missing.

    python tests/golden/make_golden_dataset.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import types

import torch

REF = os.environ.get("BENCHNAV_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REF, "src"), REF]

_stub = types.ModuleType("opensimplex")
_stub.seed = lambda s: None
_stub.noise2 = lambda x, y: 0.0
sys.modules["opensimplex"] = _stub
try:
    import tqdm  # noqa: F401
except ImportError:
    _tq = types.ModuleType("tqdm")
    _tq.tqdm = lambda *a, **k: None
    sys.modules["tqdm"] = _tq
import matplotlib  # noqa: E402
matplotlib.use("Agg")

from src.data.dataset_generator import DatasetGenerator  # noqa: E402

# 2 of 3 classes: with three environments the reference's balance_occupancy_distribution raises an IndexError for the dataset
# script's 4 of 10 (and for 2 of 4, 2 of 6, 3 of 10, ...): a swap with exactly one candidate indexes a 0-dimensional tensor
# (:248-255; benchnav_amd.terrain.occupancies documents it).  With 2 of 3 it returns a table.
ENVIRONMENTS, TOTAL, SELECTED = 3, 3, 2
SPLITS = (("train", None, 4), ("valid", None, 2), ("test", 1, 2), ("test", 2, 2))


def run_split(root, split, subset, instances):
    gen = DatasetGenerator(slip_models={}, data_directory=root, data_split=split, grid_size=8, resolution=0.5, environment_count=ENVIRONMENTS,
                           instance_count=instances, num_total_terrain_classes=TOTAL, num_selected_terrain_classes=SELECTED,
                           subset_index=subset, device="cpu")
    calls = []

    def record(seed, occupancy):
        calls.append((int(seed), [float(v) for v in occupancy]))
        return types.SimpleNamespace(tensors={"call": torch.tensor(len(calls) - 1)}, distributions={})
    gen.generate_map_instance = record
    environment_seed, base = gen.set_seed()
    occupancies = gen.generate_occupancy_distribution(seed=environment_seed)
    for e in range(ENVIRONMENTS):
        gen.generate_and_save_environment_group(e, base + e * instances, occupancies[e, :])
    folder = os.path.join(root, "test", f"subset{subset:02d}") if split == "test" else os.path.join(root, split)
    files = []
    for name in sorted(os.listdir(folder)):
        call = int(torch.load(os.path.join(folder, name), weights_only=True)["tensors"]["call"])
        files.append({"name": os.path.relpath(os.path.join(folder, name), root), "seed": calls[call][0], "occupancy": calls[call][1]})
    info = {"environment_seed": int(environment_seed), "last_instance_seed": int(base + ENVIRONMENTS * instances)}
    torch.save(info, os.path.join(folder, "seed_information.pt"))
    return {"data_split": split, "subset_index": subset, "environment_count": ENVIRONMENTS, "instance_count": instances,
            "num_total_terrain_classes": TOTAL, "num_selected_terrain_classes": SELECTED, "set_seed": [int(environment_seed), int(base)],
            "seed_information": info, "files": files}


def main():
    with tempfile.TemporaryDirectory() as root:
        out = [run_split(root, *s) for s in SPLITS]
    path = os.path.join(HERE, "dataset_layout.json")
    with open(path, "w") as f:
        json.dump({"splits": out}, f, indent=1)
    for s in out:
        print(s["data_split"], s["subset_index"], s["set_seed"], s["seed_information"], len(s["files"]), "files")
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
