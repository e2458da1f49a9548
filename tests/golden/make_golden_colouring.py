#!/usr/bin/env python3
"""Generate the colouring fixture by importing the reference (build container only).

Runs the *unmodified* reference on CPU -- GridMap(seed) -> TerrainGeometry.set_terrain_geometry -> TerrainColoring
.set_terrain_class_coloring(occupancy) -> TerrainTraversability.set_traversability(models), the steps of DatasetGenerator
.generate_map_instance (src/data/dataset_generator.py:310-358) -- and stores plain arrays in tests/golden/colouring.npz:

  per case   its parameters (as terrain.npz stores them), the occupancy it was given, the noise field the reference saw
             (float32, as it stored it), heights, t_classes (int8), colours, slopes, latent mean / std (or that set_traversability
             raised, and how many cells stayed -1), the two uniforms create_shading drew, the light vector it built, the slip models
  copper/C   the copper rows plt.cm.copper(Normalize(0, C - 1)(i)) for C = 1..16, float32
  occ/E_T_S_seed   DatasetGenerator.generate_occupancy_distribution(seed) for (environments, classes, selected) =
             (10, 10, 4), (100, 10, 4), (25, 10, 3) at seeds 0 and 1

Recipe of make_golden_terrain.py: the reference's src and root on sys.path, `opensimplex` stubbed.  Its noise2 is a smooth
stand-in of this file's own (a sum of sinusoids whose phases depend on the case), NOT OpenSimplex: the tests feed the recorded
field back, so what matters is only that the reference ran on it.  The draws and the light vector are observed by wrapping
torch.rand and torch.tensor for the duration of create_shading; nothing of the reference is stored.

    python tests/golden/make_golden_colouring.py
"""
from __future__ import annotations

import math
import os
import sys
import types
import warnings
import zipfile

import numpy as np
import torch

REF = os.environ.get("BENCHNAV_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REF, "src"), REF, os.path.dirname(HERE)]

_noise_phase = [0.0]
_noise_seen = []


def _noise2(x, y):
    """The stand-in: smooth, a few features across a map at the reference's feature size of 20 cells."""
    p = _noise_phase[0]
    v = (0.5 * math.sin(1.3 * x + 0.7 * y + 0.4 + p) + 0.3 * math.sin(2.1 * y - 0.9 * x + 1.1 + 2.0 * p)
         + 0.2 * math.sin(3.3 * x + 2.9 * y + 3.0 * p))
    _noise_seen.append(v)
    return v


_stub = types.ModuleType("opensimplex")
_stub.seed = lambda s: None
_stub.noise2 = _noise2
sys.modules["opensimplex"] = _stub
import matplotlib  # noqa: E402
matplotlib.use("Agg")

from src.environments.grid_map import GridMap  # noqa: E402
from src.environments.terrain_properties import TerrainColoring, TerrainGeometry, TerrainTraversability  # noqa: E402
from src.data.slip_models_generator import SlipModelsGenerator  # noqa: E402
from src.data.dataset_generator import DatasetGenerator  # noqa: E402

import colouring_oracle as CO  # noqa: E402

SLIP_RANGES = dict(slip_sensitivity_minmax=(1.0, 9.0), slip_nonlinearity_minmax=(1.4, 2.0), slip_offset_minmax=(0.0, 0.1),
                   noise_scale_minmax=(0.1, 0.2))            # scripts/generate_terrain_dataset.py:31-34
GEOM_KEYS = ("is_fractal", "is_crater", "num_craters", "crater_margin", "min_angle", "max_angle", "min_radius", "max_radius")
DEFAULTS = dict(is_fractal=True, is_crater=True, num_craters=3, crater_margin=5, min_angle=10, max_angle=20, min_radius=5,
                max_radius=10)
SMALL = dict(num_craters=2, min_radius=2, max_radius=4)
LOWER, UPPER, AMBIENT = 0.8, 1.0, 0.1                         # set_terrain_class_coloring's defaults


def occupancy_table(E, T, S, seed):
    gen = DatasetGenerator(slip_models={}, data_directory="", data_split="train", grid_size=64, resolution=0.5, environment_count=E,
                           instance_count=1, num_total_terrain_classes=T, num_selected_terrain_classes=S, device="cpu")
    return gen.generate_occupancy_distribution(seed).numpy().astype(np.float32)


def run_case(G, res, seed, geom, occupancy):
    occupancy = np.asarray(occupancy, np.float32)
    models = SlipModelsGenerator(num_total_terrain_classes=occupancy.size, device="cpu", **SLIP_RANGES).generate_slip_models()
    gm = GridMap(grid_size=G, resolution=res, seed=seed, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        TerrainGeometry(gm).set_terrain_geometry(**geom)
    draws, lights = [], []
    real_rand, real_tensor, real_shading = torch.rand, torch.tensor, TerrainColoring.create_shading

    def shading(self, *a, **k):
        def rand(*aa, **kk):
            out = real_rand(*aa, **kk)
            draws.append(out.detach().clone().reshape(-1))
            return out

        def tensor(*aa, **kk):
            out = real_tensor(*aa, **kk)
            lights.append(out.detach().clone())
            return out
        torch.rand, torch.tensor = rand, tensor
        try:
            return real_shading(self, *a, **k)
        finally:
            torch.rand, torch.tensor = real_rand, real_tensor

    _noise_phase[0] = 0.37 * seed
    del _noise_seen[:]
    TerrainColoring.create_shading = shading
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            TerrainColoring(gm).set_terrain_class_coloring(torch.from_numpy(occupancy.copy()), LOWER, UPPER, AMBIENT)
    finally:
        TerrainColoring.create_shading = real_shading
    unassigned_warned = any("not been assigned" in str(x.message) for x in w)
    noise = torch.tensor(_noise_seen, dtype=torch.float64).reshape(G, G).to(torch.float32).numpy()    # noise_data[y, x] = value
    t_classes = gm.tensors["t_classes"].numpy()
    assert len(draws) == 2 and len(lights) == 1 and lights[0].shape == (3,)
    assert unassigned_warned == bool((t_classes == -1).any())
    raised = False
    try:
        TerrainTraversability(gm).set_traversability(models)
    except ValueError as e:
        assert "exceeds the number of slip models" in str(e)
        raised = True
    out = dict(G=np.int32(G), res=np.float64(res), seed=np.int64(seed), geom=np.array([float(geom[k]) for k in GEOM_KEYS]),
               occupancy=occupancy, noise=noise, heights=gm.tensors["heights"].numpy().astype(np.float32),
               t_classes=t_classes.astype(np.int8), colors=gm.tensors["colors"].numpy().astype(np.float32),
               light_uniforms=torch.cat(draws).numpy().astype(np.float32), light=lights[0].numpy().astype(np.float32),
               thresholds=np.array([LOWER, UPPER]), ambient=np.float64(AMBIENT), raised=np.bool_(raised),
               unassigned=np.int64((t_classes == -1).sum()),
               models=np.array([[m.slip_sensitivity, m.slip_nonlinearity, m.slip_offset, m.base_noise_scale, m.slope_noise_scale]
                                for m in models.values()], np.float64))
    if not raised:
        lat = gm.distributions["latent_models"]
        out["slopes"] = gm.tensors["slopes"].numpy().astype(np.float32)
        out["mean"] = lat.mean.numpy().astype(np.float32)
        out["std"] = lat.stddev.numpy().astype(np.float32)
    return out


def main():
    arrays, names = {}, []
    for E, T, S in ((10, 10, 4), (100, 10, 4), (25, 10, 3)):
        for seed in (0, 1):
            arrays[f"occ/{E}_{T}_{S}_{seed}"] = occupancy_table(E, T, S, seed)
    table = arrays["occ/10_10_4_0"]
    four_of_ten = arrays["occ/10_10_4_1"][5]
    cases = {
        # name: (G, res, seed, geometry overrides, occupancy)
        "g64_row0": (64, 0.5, 30, {}, table[0]),
        "g64_row1": (64, 0.5, 31, {}, table[1]),
        "g64_row2": (64, 0.5, 32, {}, table[2]),
        "g33_thirds": (33, 0.5, 33, SMALL, [1 / 3, 1 / 3, 1 / 3]),
        "g64_ramp": (64, 0.5, 34, {}, [0.1, 0.2, 0.3, 0.4]),
        "g50_fifths": (50, 0.5, 35, SMALL, [0.2] * 5),
        "g128_four_of_ten": (128, 0.5, 36, {}, four_of_ten),
        "g64_one": (64, 0.5, 37, {}, [1.0]),
        "g64_unassigned": (64, 0.5, 38, {}, [0.0, 0.5, 0.0, 0.3]),
    }
    for name, (G, res, seed, over, occ) in cases.items():
        out = run_case(G, res, seed, dict(DEFAULTS, **over), occ)
        for key, v in out.items():
            arrays[f"{name}/{key}"] = v
        names.append(name)
        print(name, "classes", sorted(set(out["t_classes"].ravel().tolist())), "unassigned", int(out["unassigned"]), "raised", bool(out["raised"]))
    for C in range(1, 17):
        arrays[f"copper/{C}"] = CO.copper_reference(C)
    arrays["cases"] = np.array(names)
    path = os.path.join(HERE, "colouring.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:        # np.savez_compressed at the highest level
        for key, v in arrays.items():
            with z.open(key + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
