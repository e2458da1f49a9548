#!/usr/bin/env python3
"""Generate the terrain-generation fixtures by importing the reference (build container only).

Runs the *unmodified* reference on CPU -- GridMap(seed) + TerrainGeometry.set_terrain_geometry + TerrainTraversability
.set_traversability with SlipModelsGenerator models, the steps of DatasetGenerator.generate_map_instance
(src/data/dataset_generator.py:310-358) minus the colouring -- and stores plain arrays:

  tests/golden/terrain.npz           every case but the two largest: per case its parameters, the crater table the reference
                                     placed (centre x, y, radius, angle), the uniforms it drew, heights, slopes, latent mean / std,
                                     and per crater, in placement order, what generate_crater's torch.linspace (n), torch.tan and
                                     torch.sqrt (n x n profile distances) returned: torch's CPU linspace and sqrt depend on the
                                     CPU's vector width, so the tests take the reference's own values; the small case also holds
                                     the scaled spectrum ifft2 received
  tests/golden/terrain_256_fbm.npz   256^2, fBm only
  tests/golden/terrain_256_both.npz  256^2, craters and fBm

Recipe of make_golden.py: the reference's src and root on sys.path, `opensimplex` stubbed (it only seeds, set_randomness).
The draws, the distances and the spectrum are observed by wrapping torch.rand, torch.linspace, torch.tan,
torch.sqrt, torch.fft.ifft2 and TerrainGeometry.generate_crater for the duration of one call; nothing of the reference is stored.

    python tests/golden/make_golden_terrain.py
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np
import torch

REF = os.environ.get("BENCHNAV_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REF, "src"), REF]
_stub = types.ModuleType("opensimplex")
_stub.seed = lambda s: None
_stub.noise2 = lambda x, y: 0.0
sys.modules["opensimplex"] = _stub
import matplotlib  # noqa: E402
matplotlib.use("Agg")

from src.environments.grid_map import GridMap  # noqa: E402
from src.environments.terrain_properties import TerrainGeometry, TerrainTraversability  # noqa: E402
from src.data.slip_models_generator import SlipModelsGenerator  # noqa: E402

SLIP_RANGES = dict(slip_sensitivity_minmax=(1.0, 9.0), slip_nonlinearity_minmax=(1.4, 2.0), slip_offset_minmax=(0.0, 0.1),
                   noise_scale_minmax=(0.1, 0.2))            # scripts/generate_terrain_dataset.py:31-34
GEOM_KEYS = ("is_fractal", "is_crater", "num_craters", "crater_margin", "min_angle", "max_angle", "min_radius", "max_radius")
DEFAULTS = dict(is_fractal=True, is_crater=True, num_craters=3, crater_margin=5, min_angle=10, max_angle=20, min_radius=5,
                max_radius=10)


def run_case(G, res, seed, geom, num_classes=1, t_classes=None, keep_spectrum=False):
    models = SlipModelsGenerator(num_total_terrain_classes=num_classes, device="cpu", **SLIP_RANGES).generate_slip_models()
    draws, craters, spectrum, dists, lins, negtan = [], [], [], [], [], []
    real_rand, real_ifft2, real_crater = torch.rand, torch.fft.ifft2, TerrainGeometry.generate_crater

    def rand(*a, **k):
        out = real_rand(*a, **k)
        draws.append(out.detach().clone().reshape(-1))
        return out

    def ifft2(x, *a, **k):
        spectrum.append(x.detach().clone())
        return real_ifft2(x, *a, **k)

    def crater(self, heights, angle, radius, center):
        craters.append([float(center[0]), float(center[1]), float(radius), float(angle)])
        real_sqrt, real_lin, real_tan = torch.sqrt, torch.linspace, torch.tan
        lin_calls = []

        def sqrt(x, *a, **k):                   # generate_crater's only sqrt: the profile distances (:167)
            out = real_sqrt(x, *a, **k)
            dists.append(out.detach().clone().reshape(-1))
            return out

        def linspace(*a, **k):                  # called twice with the same arguments (:161-165)
            out = real_lin(*a, **k)
            lin_calls.append(out.detach().clone())
            return out

        def tan(x, *a, **k):
            out = real_tan(x, *a, **k)
            negtan.append(-float(out))
            return out
        torch.sqrt, torch.linspace, torch.tan = sqrt, linspace, tan
        try:
            return real_crater(self, heights, angle, radius, center)
        finally:
            torch.sqrt, torch.linspace, torch.tan = real_sqrt, real_lin, real_tan
            lins.append(lin_calls[0])

    gm = GridMap(grid_size=G, resolution=res, seed=seed, device="cpu")
    torch.rand, torch.fft.ifft2, TerrainGeometry.generate_crater = rand, ifft2, crater
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            TerrainGeometry(gm).set_terrain_geometry(**geom)
    finally:
        torch.rand, torch.fft.ifft2, TerrainGeometry.generate_crater = real_rand, real_ifft2, real_crater
    gave_up = any("1000 attempts" in str(x.message) for x in w)
    if t_classes is not None:
        gm.tensors["t_classes"] = torch.from_numpy(t_classes)
    TerrainTraversability(gm).set_traversability(models)
    lat = gm.distributions["latent_models"]
    out = dict(G=np.int32(G), res=np.float64(res), seed=np.int64(seed), gave_up=np.bool_(gave_up),
               geom=np.array([float(geom[k]) for k in GEOM_KEYS]),
               uniforms=torch.cat(draws).numpy().astype(np.float32) if draws else np.zeros(0, np.float32),
               craters=np.array(craters, np.float64).reshape(-1, 4),
               crater_dist=torch.cat(dists).numpy().astype(np.float32) if dists else np.zeros(0, np.float32),
               crater_lin=torch.cat(lins).numpy().astype(np.float32) if lins else np.zeros(0, np.float32),
               crater_negtan=np.array(negtan, np.float32),
               heights=gm.tensors["heights"].numpy().astype(np.float32), slopes=gm.tensors["slopes"].numpy().astype(np.float32),
               mean=lat.mean.numpy().astype(np.float32), std=lat.stddev.numpy().astype(np.float32),
               models=np.array([[m.slip_sensitivity, m.slip_nonlinearity, m.slip_offset, m.base_noise_scale, m.slope_noise_scale]
                                for m in models.values()], np.float64))
    if t_classes is not None:
        out["t_classes"] = t_classes.astype(np.int64)
    if keep_spectrum:
        out["spectrum"] = spectrum[0].numpy().astype(np.complex64)
    return out


def stripes(G, k, seed):
    """A k-class map: seeded random horizontal and vertical bands (what matters is that every class has cells)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, k, G)
    cols = rng.integers(0, k, G)
    t = (rows[:, None] + cols[None, :]) % k
    return t.astype(np.int64)


CASES = {
    # name: (G, res, seed, geometry overrides, classes, t_classes, spectrum?)
    "small": (14, 0.5, 3, dict(num_craters=2, crater_margin=1, min_radius=1, max_radius=2), 1, None, True),
    "g64_s0": (64, 0.5, 0, {}, 1, None, False),
    "g64_s1": (64, 0.5, 1, {}, 1, None, False),
    "g64_s7": (64, 0.5, 7, {}, 1, None, False),
    "giveup": (16, 0.5, 5, {}, 1, None, False),
    "border": (64, 0.5, 11, dict(is_fractal=False), 1, None, False),
    "odd33": (33, 0.5, 2, dict(num_craters=2, min_radius=2, max_radius=4), 1, None, False),
    "odd50": (50, 0.5, 4, dict(num_craters=2, min_radius=2, max_radius=4), 1, None, False),
    "classes3": (64, 0.5, 9, {}, 3, "stripes", False),
    "g256_crater": (256, 0.5, 21, dict(is_fractal=False, num_craters=12), 1, None, False),
}
BIG = {
    "terrain_256_fbm": (256, 0.5, 22, dict(is_crater=False), 1, None, False),
    "terrain_256_both": (256, 0.5, 23, dict(num_craters=12), 1, None, False),
}


def main():
    arrays = {}
    names = []
    for name, (G, res, seed, over, k, tc, spec) in CASES.items():
        geom = dict(DEFAULTS, **over)
        tcl = stripes(G, k, seed) if tc == "stripes" else None
        out = run_case(G, res, seed, geom, k, tcl, spec)
        for key, v in out.items():
            arrays[f"{name}/{key}"] = v
        names.append(name)
        print(name, "craters", len(out["craters"]), "gave_up", bool(out["gave_up"]), "uniforms", out["uniforms"].size)
    arrays["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "terrain.npz"), **arrays)
    for fname, (G, res, seed, over, k, tc, spec) in BIG.items():
        out = run_case(G, res, seed, dict(DEFAULTS, **over), k, None, spec)
        np.savez_compressed(os.path.join(HERE, fname + ".npz"), **out)
        print(fname, "craters", len(out["craters"]))
    for f in ["terrain.npz"] + [b + ".npz" for b in BIG]:
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
