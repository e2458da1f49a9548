"""BenchNav map instances generated on the GPU: terrain geometry (craters + fBm heights, Horn slopes) and the latent slip model.

Mirror of the reference's `DatasetGenerator.generate_map_instance` (src/data/dataset_generator.py:310-358) without its colouring
step: `TerrainGeometry.set_terrain_geometry` (src/environments/terrain_properties.py:37-134), `TerrainTraversability
.set_traversability` (:527-579) with `SlipModel.model_mean / model_stddev` (src/environments/slip_model.py), and the slip models of
`SlipModelsGenerator.generate_slip_models` (src/data/slip_models_generator.py).

The random draws stay on the host, in the reference's order on torch's CPU generator (`GridMap(seed=...)` seeds it,
grid_map.py:52): the crater rejection loop touches a few scalars per attempt, and the fBm phases are then ONE `torch.rand(n)`,
which on torch's CPU generator equals n successive `torch.rand(1)` calls (tests/test_terrain_host.py asserts this).  A reference
run on a CUDA generator draws another stream: parity with it is out of scope.  Each crater's profile coordinates and slope come
from the reference's own torch calls (linspace, tan) on the host; torch's CPU linspace depends on the CPU's vector width, so,
like the reference's own output, they can differ by an ulp between CPUs.  The device (csrc/terrain_kernels.hip) does the
arithmetic for B instances per launch: crater carving with a min-shift after every crater, the fBm spectrum, a dense 2-D inverse
DFT in float64, the Horn slopes and the per-class slip maps.

Only `start_pos = goal_pos = None` is supported (how DatasetGenerator calls set_terrain_geometry); with a start and a goal the
reference's overlap test compares a (2, 1, 2) centre table per coordinate, a path not mirrored here.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _capi

# the dataset script's ranges (scripts/generate_terrain_dataset.py:31-34), the defaults of slip_models()
SLIP_SENSITIVITY_MINMAX = (1.0, 9.0)
SLIP_NONLINEARITY_MINMAX = (1.4, 2.0)
SLIP_OFFSET_MINMAX = (0.0, 0.1)
NOISE_SCALE_MINMAX = (0.1, 0.2)
MAX_ATTEMPTS = 1000                       # terrain_properties.py:124


@dataclass
class SlipParams:
    """The fields of the reference's SlipModel that its mean / stddev read (slip_model.py:13-47); a reference SlipModel works
    wherever one of these is accepted."""
    slip_sensitivity: float
    slip_nonlinearity: float
    slip_offset: float
    base_noise_scale: float = 0.05
    slope_noise_scale: float = 0.0


def _uniform(g: torch.Generator, lo: float, hi: float) -> float:
    return (torch.rand(1, generator=g) * (hi - lo) + lo).item()          # SlipModelsGenerator.uniform_sampling


def slip_models(num_classes: int, slip_sensitivity_minmax=SLIP_SENSITIVITY_MINMAX, slip_nonlinearity_minmax=SLIP_NONLINEARITY_MINMAX,
                slip_offset_minmax=SLIP_OFFSET_MINMAX, noise_scale_minmax=NOISE_SCALE_MINMAX) -> List[SlipParams]:
    """SlipModelsGenerator.generate_slip_models: class c reseeds with c and draws four uniforms (slip_models_generator.py:67-117)."""
    for lo, hi in (slip_sensitivity_minmax, slip_nonlinearity_minmax, slip_offset_minmax, noise_scale_minmax):
        if lo >= hi:
            raise ValueError("The minimum value must be less than the maximum value.")
    out = []
    for c in range(num_classes):
        g = torch.Generator().manual_seed(c)
        s, n, o, b = (_uniform(g, *mm) for mm in (slip_sensitivity_minmax, slip_nonlinearity_minmax, slip_offset_minmax,
                                                  noise_scale_minmax))
        out.append(SlipParams(s, n, o, b))
    return out


_default_slip_models = slip_models           # generate()'s slip_models argument shadows the function


@dataclass
class Crater:
    """One placed crater and what generate_crater (terrain_properties.py:136-210) derives from it, as float32 torch computes it."""
    center: np.ndarray            # (2,) float32, metres (x, y)
    radius: float                 # a float32 value
    angle: float                  # degrees, a Python float (rand().item() * (max - min) + min)
    n: int                        # profile points per axis: ceil(f32(2 r) / f32(res))
    bounds: tuple                 # (sx, sy, ex, ey, psx, psy): the padded-grid slice [sy:ey, sx:ex] and the profile's origin in it
    lin: np.ndarray               # (n,) float32 linspace(-r, r, n)
    neg_tan: float                # float32 -tan(deg2rad(f32(angle)))


@dataclass
class Draws:
    craters: List[Crater]
    attempts: int
    gave_up: bool
    phases: np.ndarray            # (n,) float32 uniforms of generate_fractal_surface, empty without fBm


def num_phases(grid_size: int) -> int:
    h = (grid_size + 2) // 2
    return (h + 1) ** 2 + (h - 1) ** 2


def _crater_plan(G: int, res: float, center: torch.Tensor, radius: float, angle: float) -> Crater:
    N = G + 2
    n = int(torch.ceil(torch.tensor(2 * radius) / torch.tensor(res)).item())                       # :155-160
    lin = torch.linspace(-radius, radius, n)                                                       # :161-165
    neg_tan = -torch.tan(torch.deg2rad(torch.tensor(angle)))                                      # :170-173
    # GridMap.get_grid_indices_from_positions (grid_map.py:183-210) on the UNPADDED map, clamped to [0, G-1]
    x0 = G * res / 2 - G / 2 * res
    ci = ((center - torch.tensor([x0, x0])) / res).floor().int().clamp(0, G - 1)
    cx, cy = int(ci[0]), int(ci[1])
    sx, sy = max(cx - n // 2, 0), max(cy - n // 2, 0)                                              # :180-190
    ex, ey = min(cx + n // 2, N), min(cy + n // 2, N)
    psx, psy = max(n // 2 - cx, 0), max(n // 2 - cy, 0)
    if psx + (ex - sx) > n or psy + (ey - sy) > n:
        raise ValueError(f"crater of radius {radius} does not fit a {G}x{G} map: the reference's slices disagree in shape")
    return Crater(center.numpy().astype(np.float32), float(radius), float(angle), n, (sx, sy, ex, ey, psx, psy),
                  lin.numpy().astype(np.float32), float(neg_tan))


def replay_draws(seed: int, grid_size: int, resolution: float, is_fractal: bool = True, is_crater: bool = True, num_craters: int = 3,
                 crater_margin: float = 5, min_angle: float = 10, max_angle: float = 20, min_radius: float = 5,
                 max_radius: float = 10) -> Draws:
    """The reference's random draws for one instance seeded with `seed`, on a private CPU generator: the crater rejection loop
    (terrain_properties.py:70-129) and then the fBm phases (:254-286) as one torch.rand(n)."""
    g = torch.Generator().manual_seed(int(seed))
    G, res, N = grid_size, resolution, grid_size + 2
    x0 = G * res / 2 - G / 2 * res                                                                 # GridMap.x_limits[0]
    craters, count, gave_up = [], 0, False
    if is_crater:
        positions, radii = torch.empty((0, 2)), torch.full((0,), 5.0)
        while len(craters) < num_craters:
            center = torch.rand(2, generator=g) * ((N - 1) * res - x0) + x0
            radius = (torch.rand(1, generator=g) * (max_radius - min_radius) + min_radius).item()
            dist = torch.norm(positions - center, dim=1)                                          # check_circle_overlap
            if not (dist < (radii + radius + crater_margin)).any().item():
                angle = torch.rand(1, generator=g).item() * (max_angle - min_angle) + min_angle
                craters.append(_crater_plan(G, res, center, radius, angle))
                positions = torch.cat((positions, center.unsqueeze(0)), dim=0)
                radii = torch.cat((radii, torch.tensor([radius])), dim=0)
            count += 1
            if count > MAX_ATTEMPTS:
                warnings.warn("Failed to place all craters after 1000 attempts. Consider adjusting the parameters.")
                gave_up = True
                break
    phases = torch.rand(num_phases(G), generator=g).numpy() if is_fractal else np.zeros(0, np.float32)
    return Draws(craters, count, gave_up, phases)


def _as_param_table(models):
    """((C, 6) float32 rows, number of models): the rows are (present, f32(sens * 1e-3), nonlinearity, offset, base noise, slope noise) for class indices 0..C-1."""
    items = dict(enumerate(models)) if isinstance(models, (list, tuple)) else dict(models)
    C_ = max(items) + 1 if items else 0
    tab = np.zeros((C_, 6), np.float32)
    for c, m in items.items():
        tab[c] = (1.0, m.slip_sensitivity * 1e-3, m.slip_nonlinearity, m.slip_offset, m.base_noise_scale, m.slope_noise_scale)
    return tab, len(items)


@dataclass
class Terrain:
    """Device tensors of B generated instances, (B, G, G) float32 each, and the per-instance draws."""
    heights: torch.Tensor
    slopes: torch.Tensor
    latent_mean: torch.Tensor
    latent_std: torch.Tensor
    t_classes: torch.Tensor                    # (B, G, G) int64 on the host, as the reference stores it
    craters: List[np.ndarray]                  # per instance (k, 4) float64 rows (x, y, radius, angle)
    draws: List[Draws] = field(default_factory=list)


class TerrainGenerator:
    """B map instances of one grid size per launch.

        gen = TerrainGenerator(64, 0.5, batch=8)
        t = gen.generate(seeds=range(8))            # DatasetGenerator.generate_map_instance(seed) minus the colouring
        insts = gen.to_instances()                  # io.MapInstance: io.save_instance / io.planner_inputs take them
    """

    def __init__(self, grid_size: int, resolution: float, batch: int = 1, roughness_exponent: float = 0.75,
                 amplitude_gain: float = 10, device_id: Optional[int] = None) -> None:
        if not torch.cuda.is_available():
            raise RuntimeError("benchnav_amd.TerrainGenerator needs an MI355X (gfx950) device; there is no CPU fallback")
        self.grid_size, self.resolution, self.batch = int(grid_size), float(resolution), int(batch)
        self.roughness_exponent, self.amplitude_gain = float(roughness_exponent), float(amplitude_gain)
        self._dev = torch.device("cuda", torch.cuda.current_device() if device_id is None else device_id)
        self._lib = _capi.load()
        h = C.c_void_p()
        self._check(self._lib.bn_terrain_create(self._dev.index, self.grid_size, self.batch, C.byref(h)))
        self._handle = h
        self._last: Optional[Terrain] = None

    def generate(self, seeds: Sequence[int], is_fractal: bool = True, is_crater: bool = True, num_craters: int = 3,
                 crater_margin: float = 5, min_angle: float = 10, max_angle: float = 20, min_radius: float = 5,
                 max_radius: float = 10, t_classes=None, slip_models=None, start_pos=None, goal_pos=None) -> Terrain:
        if start_pos is not None or goal_pos is not None:
            raise NotImplementedError("start_pos / goal_pos crater avoidance is not mirrored (DatasetGenerator passes neither)")
        seeds = [int(s) for s in seeds]
        B, G = self.batch, self.grid_size
        if len(seeds) != B:
            raise ValueError(f"expected {B} seeds, got {len(seeds)}")
        draws = [replay_draws(s, G, self.resolution, is_fractal, is_crater, num_craters, crater_margin, min_angle, max_angle,
                              min_radius, max_radius) for s in seeds]
        return self.generate_from_draws(draws, is_fractal, t_classes, slip_models)

    def generate_from_draws(self, draws: List[Draws], is_fractal: bool = True, t_classes=None, slip_models=None) -> Terrain:
        """generate() on given draws (one Draws per instance, e.g. from replay_draws): the device half alone."""
        if len(draws) != self.batch:
            raise ValueError(f"expected {self.batch} draws, got {len(draws)}")
        self.upload_draws(draws, is_fractal)
        cls = self._class_maps(t_classes)
        models = _default_slip_models(1) if slip_models is None else slip_models
        tab, nmodels = _as_param_table(models)
        present = np.unique(cls)
        if present.min() < 0 or present.max() >= nmodels:                                        # set_traversability :556-559
            raise ValueError("The number of terrain classes exceeds the number of slip models.")
        cls32 = np.ascontiguousarray(cls, dtype=np.int32)
        self._check(self._lib.bn_terrain_set_slip(self._handle, cls32.ctypes.data, tab.ctypes.data, tab.shape[0]))
        self._check(self._lib.bn_terrain_generate_async(self._handle, C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)))
        out = self.outputs()
        self._last = Terrain(*out, t_classes=torch.from_numpy(cls.astype(np.int64)),
                             craters=[np.array([[c.center[0], c.center[1], c.radius, c.angle] for c in d.craters], np.float64).reshape(-1, 4)
                                      for d in draws], draws=draws)
        return self._last

    def upload_draws(self, draws: List[Draws], is_fractal: bool) -> None:
        """Ship the draws of B instances: the crater tables (int bounds + float32 radius, -tan, linspace) and the phases."""
        B, G = self.batch, self.grid_size
        maxc = max([len(d.craters) for d in draws] + [1])
        count = np.array([len(d.craters) for d in draws], np.int32)
        ints = np.zeros((B, maxc, 8), np.int32)
        vals = np.zeros((B, maxc, 2), np.float32)
        lins, off = [], 0
        for b, d in enumerate(draws):
            for j, c in enumerate(d.craters):
                ints[b, j] = (*c.bounds, c.n, off)
                vals[b, j] = (c.radius, c.neg_tan)
                lins.append(c.lin)
                off += c.n
        lin = np.concatenate(lins).astype(np.float32) if lins else np.zeros(1, np.float32)
        nph = num_phases(G)
        ph = np.zeros((B, nph), np.float32)
        if is_fractal:
            ph[:] = np.stack([d.phases for d in draws])
        self._check(self._lib.bn_terrain_set_geometry(self._handle, self.resolution, self.roughness_exponent, self.amplitude_gain,
                                                      int(bool(is_fractal))))
        self._check(self._lib.bn_terrain_set_draws(self._handle, ph.ctypes.data, count.ctypes.data, ints.ctypes.data,
                                                   vals.ctypes.data, maxc, lin.ctypes.data, int(lin.size)))

    def _class_maps(self, t_classes) -> np.ndarray:
        B, G = self.batch, self.grid_size
        if t_classes is None:
            return np.zeros((B, G, G), np.int64)
        t = t_classes.detach().cpu().numpy() if isinstance(t_classes, torch.Tensor) else np.asarray(t_classes)
        if t.shape == (G, G):
            t = np.broadcast_to(t, (B, G, G))
        if t.shape != (B, G, G):
            raise ValueError(f"t_classes must be ({G}, {G}) or ({B}, {G}, {G}), got {t.shape}")
        if not np.issubdtype(t.dtype, np.integer):
            if not np.array_equal(t, np.round(t)):
                raise ValueError("t_classes must hold integer class indices")
        return np.ascontiguousarray(t.astype(np.int64))

    def outputs(self):
        """(heights, slopes, latent_mean, latent_std) of the last generate(), (B, G, G) float32 device tensors (copies)."""
        from .astar import _DevArray
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self._lib.bn_terrain_buffers(self._handle, *[C.byref(p) for p in ptrs]))
        shape = (self.batch, self.grid_size, self.grid_size)
        with torch.cuda.device(self._dev):
            return tuple(torch.as_tensor(_DevArray(p.value, shape), device=self._dev).clone() for p in ptrs)

    def spectrum(self, instance: int = 0) -> np.ndarray:
        """Test hook: the scaled fBm spectrum of `instance` that the inverse DFT reads, (G+2, G+2) complex64."""
        N = self.grid_size + 2
        buf = np.empty((N, N, 2), np.float32)
        self._check(self._lib.bn_terrain_spectrum(self._handle, instance, buf.ctypes.data))
        return buf[..., 0] + 1j * buf[..., 1]

    def to_instances(self):
        """The last generate() as io.MapInstance objects (CPU tensors, the reference's on-disk layout; colours are zero)."""
        from .io import MapInstance
        t = self._last
        if t is None:
            raise RuntimeError("generate() has not run")
        G = self.grid_size
        out = []
        for b in range(self.batch):
            tensors = {"heights": t.heights[b].cpu(), "slopes": t.slopes[b].cpu(), "t_classes": t.t_classes[b].clone(),
                       "colors": torch.zeros(3, G, G)}
            out.append(MapInstance(grid_size=G, tensors=tensors, latent_mean=t.latent_mean[b].cpu(),
                                   latent_std=t.latent_std[b].cpu(), extra={"craters": t.craters[b]}))
        return out

    def _check(self, code):
        if code < 0:
            raise _capi.BenchnavError(code, self._lib.bn_terrain_last_error().decode("utf-8", "replace"))

    def close(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            self._lib.bn_terrain_destroy(h)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
