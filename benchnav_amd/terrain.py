"""BenchNav map instances generated on the GPU: terrain geometry (craters + fBm heights, Horn slopes), terrain classes with shaded
colours, and the latent slip model.

Mirror of the reference's `DatasetGenerator.generate_map_instance` (src/data/dataset_generator.py:310-358):
`TerrainGeometry.set_terrain_geometry` (src/environments/terrain_properties.py:37-134), on request `TerrainColoring
.set_terrain_class_coloring` (:364-523), `TerrainTraversability.set_traversability` (:527-579) with `SlipModel.model_mean /
model_stddev` (src/environments/slip_model.py), and the slip models of `SlipModelsGenerator.generate_slip_models`
(src/data/slip_models_generator.py).

Colouring is opt-in (`generate(..., occupancy=...)`).  Its noise field is an input: the caller's (with the real `opensimplex`'s
field the classes are the reference's on that field), or the library's own seeded gradient noise (not OpenSimplex).
The two uniforms of the light source are replayed after the fBm phases and the light vector is built with the reference's torch
calls; the class thresholds are torch's float32 cumsum; the copper colour table is computed here without matplotlib.

By default the random draws are made on the host, in the reference's order on torch's CPU generator (`GridMap(seed=...)` seeds it,
grid_map.py:52): the crater rejection loop touches a few scalars per attempt, and the fBm phases are then ONE `torch.rand(n)`,
which on torch's CPU generator equals n successive `torch.rand(1)` calls (tests/test_terrain_host.py asserts this).  A reference
run on a CUDA generator draws another stream: parity with it is out of scope.  Each crater's profile coordinates and slope come
from the reference's own torch calls (linspace, tan) on the host; torch's CPU linspace depends on the CPU's vector width, so,
like the reference's own output, they can differ by an ulp between CPUs.  The device (csrc/terrain_kernels.hip) does the
arithmetic for B instances per launch: crater carving with a min-shift after every crater, the fBm spectrum, a dense 2-D inverse
DFT in float64, the Horn slopes and the per-class slip maps.

`generate(..., draws="device")` makes the same draws on the device instead (terrain_draws_kernel: torch's MT19937 stream per
seed, the crater loop, the crater tables, the phases, the light source), so a batch of seeds becomes a batch of
instances with no per-instance host work; one small read-back then fills the crater tables of the result.

Only `start_pos = goal_pos = None` is supported (how DatasetGenerator calls set_terrain_geometry); with a start and a goal the
reference's overlap test compares a (2, 1, 2) centre table per coordinate, a path not mirrored here.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi
from ._device import Handle, resolve_device, stream_ptr

# the dataset script's ranges (scripts/generate_terrain_dataset.py:31-34), the defaults of slip_models()
SLIP_SENSITIVITY_MINMAX = (1.0, 9.0)
SLIP_NONLINEARITY_MINMAX = (1.4, 2.0)
SLIP_OFFSET_MINMAX = (0.0, 0.1)
NOISE_SCALE_MINMAX = (0.1, 0.2)
MAX_ATTEMPTS = 1000                       # terrain_properties.py:124
MAX_COLOR_CLASSES = 64                    # the colour table lives in LDS (csrc/terrain_kernels.hip)


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
    seed: Optional[int] = None                    # the instance seed (keys the library's own noise)
    light_uniforms: Optional[np.ndarray] = None   # (2,) float32: create_shading's light angle and z draws, with coloring only
    light: Optional[np.ndarray] = None            # (3,) float32 light vector as the reference's torch calls build it


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


def _light_draws(g: torch.Generator, lower_threshold: float, upper_threshold: float) -> Tuple[np.ndarray, np.ndarray]:
    """create_shading's two draws on `g` and its light vector, with the reference's own torch calls (:511-517)."""
    u_angle, u_z = torch.rand(1, generator=g), torch.rand(1, generator=g)
    light_angle = u_angle * (2 * torch.pi)
    z = u_z * (upper_threshold - lower_threshold) + lower_threshold
    radius = torch.sqrt(1 - z**2)
    light = torch.tensor([radius * torch.cos(light_angle), radius * torch.sin(light_angle), z])
    return torch.cat((u_angle, u_z)).numpy().astype(np.float32), light.numpy().astype(np.float32)


def light_source(seed_or_generator: Union[int, torch.Generator], lower_threshold: float = 0.8, upper_threshold: float = 1.0) -> np.ndarray:
    """The (3,) float32 light vector of create_shading (terrain_properties.py:511-517): two uniforms (angle, then z) from a CPU
    generator seeded with the given seed, or from the given generator where it stands."""
    g = seed_or_generator if isinstance(seed_or_generator, torch.Generator) else torch.Generator().manual_seed(int(seed_or_generator))
    return _light_draws(g, lower_threshold, upper_threshold)[1]


def _copper_lut() -> np.ndarray:
    """matplotlib's 256-entry copper table, (256, 3) float64: three piecewise-linear channels through linspace(0, 1, 256)
    (red rises to 1 at 0.809524, green to 0.7812 and blue to 0.4975 at 1), built the way LinearSegmentedColormap interpolates."""
    xind = 255 * np.linspace(0, 1, 256)
    lut = np.empty((256, 3))
    for ch, data in enumerate((((0.0, 0.0, 0.0), (0.809524, 1.0, 1.0), (1.0, 1.0, 1.0)),
                               ((0.0, 0.0, 0.0), (1.0, 0.7812, 0.7812)), ((0.0, 0.0, 0.0), (1.0, 0.4975, 0.4975)))):
        adata = np.array(data)
        x, y0, y1 = adata[:, 0] * 255, adata[:, 1], adata[:, 2]
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut[:, ch] = np.clip(np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0.0, 1.0)
    return lut


def _copper_table(num_classes: int) -> np.ndarray:
    """(C, 3) float32: plt.cm.copper(Normalize(0, C - 1)(i))[:3] for i = 0..C-1 (create_color_map :462-470), without matplotlib.
    C = 1 gives black: Normalize(0, 0) maps everything to 0."""
    C_ = int(num_classes)
    if C_ < 1 or C_ > MAX_COLOR_CLASSES:
        raise ValueError(f"colouring supports 1 to {MAX_COLOR_CLASSES} terrain classes, got {C_}")
    v = np.zeros(C_) if C_ == 1 else np.arange(C_, dtype=np.float64) / (C_ - 1)
    idx = (v * 256).astype(np.int64)          # Colormap.__call__: X * N truncated, X == 1 in the last entry
    idx[idx >= 256] = 255
    return _copper_lut()[idx].astype(np.float32)


def occupancies(environment_count: int, num_total_terrain_classes: int = 10, num_selected_terrain_classes: int = 4,
                seed: int = 0) -> torch.Tensor:
    """(environments, classes) float32 occupancy rows: DatasetGenerator.generate_occupancy_distribution and
    balance_occupancy_distribution (dataset_generator.py:192-264) on a private CPU generator: a randperm per environment picks
    the selected classes (1 / selected each), then up to 1000 rounds swap a selection from every over-represented class to the
    first under-represented one that has a candidate environment.

    Where the reference returns a table this is that table.  Where a swap has exactly one candidate the reference raises an
    IndexError (its nonzero(...).squeeze() is 0-dimensional there and it indexes [0]); here that single candidate is taken, the
    evident intent."""
    E, T, S = int(environment_count), int(num_total_terrain_classes), int(num_selected_terrain_classes)
    g = torch.Generator().manual_seed(int(seed))
    occ = torch.zeros(E, T)
    for e in range(E):
        occ[e, torch.randperm(T, generator=g)[:S]] = 1 / S
    expected = S * E / T
    current = torch.sum(occ == 1 / S, dim=0)
    for _ in range(1000):
        over_classes = torch.where(current > expected)[0]
        under_classes = torch.where(current < expected)[0]
        if len(over_classes) == 0 or len(under_classes) == 0:
            break
        for over in over_classes:
            for under in under_classes:
                candidates = torch.nonzero((occ[:, over] == 1 / S) & (occ[:, under] == 0), as_tuple=False).reshape(-1)
                if candidates.numel() > 0:
                    e = candidates[0].item()
                    occ[e, over] = 0
                    occ[e, under] = 1 / S
                    current[over] -= 1
                    current[under] += 1
                    break
    return occ


def replay_draws(seed: int, grid_size: int, resolution: float, is_fractal: bool = True, is_crater: bool = True, num_craters: int = 3,
                 crater_margin: float = 5, min_angle: float = 10, max_angle: float = 20, min_radius: float = 5,
                 max_radius: float = 10, coloring: Union[None, bool, Tuple[float, float]] = None) -> Draws:
    """The reference's random draws for one instance seeded with `seed`, on a private CPU generator: the crater rejection loop
    (terrain_properties.py:70-129), then the fBm phases (:254-286) as one torch.rand(n), and with `coloring` (True, or the pair
    (lower_threshold, upper_threshold); True means (0.8, 1.0)) the two draws of create_shading's light source (:511-512)."""
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
    d = Draws(craters, count, gave_up, phases, seed=int(seed))
    if coloring is not None and coloring is not False:
        lo, hi = (0.8, 1.0) if coloring is True else coloring
        d.light_uniforms, d.light = _light_draws(g, float(lo), float(hi))
    return d


def check_draw_records(records: np.ndarray, radii: np.ndarray, grid_size: int) -> None:
    """What replay_draws raises, from the device draws' records ((B, 4) int32: attempts, gave_up, status, craters placed) and the
    (B, slots) float32 radii: the ValueError of the first crater whose slices disagree in shape (status = 1 + its index), else one
    "Failed to place all craters" warning if an instance gave up."""
    for b in np.flatnonzero(records[:, 2] != 0):
        radius = float(radii[b, int(records[b, 2]) - 1])
        raise ValueError(f"crater of radius {radius} does not fit a {grid_size}x{grid_size} map: the reference's slices disagree in shape")
    if records[:, 1].any():
        warnings.warn("Failed to place all craters after 1000 attempts. Consider adjusting the parameters.")


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
    """Device tensors of B generated instances, (B, G, G) float32 each, and the per-instance draws.  With colouring, `colors`
    are the shaded colours, `noise` the raw noise field the classes were cut from and `light` the light vectors; without,
    `colors` are zero and the other two None."""
    heights: torch.Tensor
    slopes: torch.Tensor
    latent_mean: torch.Tensor
    latent_std: torch.Tensor
    t_classes: torch.Tensor                    # (B, G, G) int64 on the host, as the reference stores it
    craters: List[np.ndarray]                  # per instance (k, 4) float64 rows (x, y, radius, angle)
    draws: List[Draws] = field(default_factory=list)
    colors: Optional[torch.Tensor] = None      # (B, 3, G, G) float32, device
    noise: Optional[torch.Tensor] = None       # (B, G, G) float32, device
    light: Optional[np.ndarray] = None         # (B, 3) float32
    classes_device: Optional[torch.Tensor] = None   # (B, G, G) int32, device: the class buffer t_classes was copied from (colouring only)


class TerrainGenerator(Handle):
    """B map instances of one grid size per launch.

        gen = TerrainGenerator(64, 0.5, batch=8)
        t = gen.generate(seeds=range(8))            # DatasetGenerator.generate_map_instance(seed) minus the colouring
        occ = occupancies(10)                       # ... and with it: 4 of 10 classes per environment
        t = gen.generate(seeds=range(8), occupancy=occ[0], slip_models=slip_models(10))
        insts = gen.to_instances()                  # io.MapInstance: io.save_instance / io.planner_inputs take them
    """
    family = "terrain"

    def __init__(self, grid_size: int, resolution: float, batch: int = 1, roughness_exponent: float = 0.75,
                 amplitude_gain: float = 10, device_id: Optional[int] = None) -> None:
        self.dev = self._dev = resolve_device(None if device_id is None else torch.device("cuda", device_id), "TerrainGenerator")
        self.grid_size, self.resolution, self.batch = int(grid_size), float(resolution), int(batch)
        self.roughness_exponent, self.amplitude_gain = float(roughness_exponent), float(amplitude_gain)
        self._lib = _capi.load()
        h = C.c_void_p()
        self._check(self._lib.bn_terrain_create(self._dev.index, self.grid_size, self.batch, C.byref(h)))
        self._handle = h
        self._last: Optional[Terrain] = None

    def generate(self, seeds: Sequence[int], is_fractal: bool = True, is_crater: bool = True, num_craters: int = 3,
                 crater_margin: float = 5, min_angle: float = 10, max_angle: float = 20, min_radius: float = 5,
                 max_radius: float = 10, t_classes=None, slip_models=None, start_pos=None, goal_pos=None, occupancy=None, noise=None,
                 feature_size: float = 20, lower_threshold: float = 0.8, upper_threshold: float = 1.0,
                 ambient_intensity: float = 0.1, draws: str = "host") -> Terrain:
        """B instances from B seeds.  `occupancy` ((C,) or (B, C) class ratios, e.g. rows of occupancies()) asks for the colouring
        step: the terrain classes are cut from a noise field -- `noise` ((G, G) or (B, G, G)), or the library's own keyed by each
        seed -- and the colours are the classes' copper colours shaded by the heights.  Without it, nothing changes: the classes
        are `t_classes` (default all zero) and the colours zero.

        `draws="host"` replays every instance's draws on torch's CPU generator (replay_draws); `draws="device"` makes the same draws
        in one kernel launch ahead of the generation, with no per-instance host work: the result's `draws` then carry the crater
        tables without the profile coordinates and without the phases (device_draws() fetches everything)."""
        if draws not in ("host", "device"):
            raise ValueError(f'draws must be "host" or "device", got {draws!r}')
        if start_pos is not None or goal_pos is not None:
            raise NotImplementedError("start_pos / goal_pos crater avoidance is not mirrored (DatasetGenerator passes neither)")
        seeds = [int(s) for s in seeds]
        B, G = self.batch, self.grid_size
        if len(seeds) != B:
            raise ValueError(f"expected {B} seeds, got {len(seeds)}")
        if occupancy is None and noise is not None:
            raise ValueError("noise= is the colouring step's input: pass occupancy= as well")
        if occupancy is not None and t_classes is not None:
            raise ValueError("t_classes= and occupancy= are two sources for one class map: pass one")
        coloring = None if occupancy is None else (lower_threshold, upper_threshold)
        if draws == "device":
            return self._generate_device(seeds, is_fractal, (is_crater, num_craters, crater_margin, min_angle, max_angle, min_radius,
                                                             max_radius), coloring, t_classes, slip_models, occupancy, noise,
                                         feature_size, ambient_intensity)
        draws = [replay_draws(s, G, self.resolution, is_fractal, is_crater, num_craters, crater_margin, min_angle, max_angle,
                              min_radius, max_radius, coloring=coloring) for s in seeds]
        return self.generate_from_draws(draws, is_fractal, t_classes, slip_models, occupancy=occupancy, noise=noise,
                                        feature_size=feature_size, ambient_intensity=ambient_intensity)

    def generate_from_draws(self, draws: List[Draws], is_fractal: bool = True, t_classes=None, slip_models=None, occupancy=None,
                            noise=None, feature_size: float = 20, ambient_intensity: float = 0.1) -> Terrain:
        """generate() on given draws (one Draws per instance, e.g. from replay_draws): the device half alone.  With `occupancy`
        the draws carry the light vectors (replay_draws(coloring=...)) and, for the library's own noise, the seeds."""
        if len(draws) != self.batch:
            raise ValueError(f"expected {self.batch} draws, got {len(draws)}")
        if occupancy is not None:
            if t_classes is not None:
                raise ValueError("t_classes= and occupancy= are two sources for one class map: pass one")
            return self._generate_colored(draws, is_fractal, slip_models, occupancy, noise, feature_size, ambient_intensity)
        self.upload_draws(draws, is_fractal)
        self._check(self._lib.bn_terrain_set_coloring(self._handle, 0, None, None, 0, None, None, 0.0, 0.0, None, None, 0))
        cls = self._class_maps(t_classes)
        models = _default_slip_models(1) if slip_models is None else slip_models
        tab, nmodels = _as_param_table(models)
        present = np.unique(cls)
        if present.min() < 0 or present.max() >= nmodels:                                        # set_traversability :556-559
            raise ValueError("The number of terrain classes exceeds the number of slip models.")
        cls32 = np.ascontiguousarray(cls, dtype=np.int32)
        self._check(self._lib.bn_terrain_set_slip(self._handle, cls32.ctypes.data, tab.ctypes.data, tab.shape[0]))
        self._check(self._lib.bn_terrain_generate_async(self._handle, stream_ptr(self._dev)))
        out = self.outputs()
        with torch.cuda.device(self._dev):
            colors = torch.zeros((self.batch, 3, self.grid_size, self.grid_size), device=self._dev)
        self._last = Terrain(*out, t_classes=torch.from_numpy(cls.astype(np.int64)), craters=self._crater_tables(draws), draws=draws,
                             colors=colors)
        return self._last

    @staticmethod
    def _crater_tables(draws):
        return [np.array([[c.center[0], c.center[1], c.radius, c.angle] for c in d.craters], np.float64).reshape(-1, 4) for d in draws]

    def _occupancy_rows(self, occupancy) -> torch.Tensor:
        """(B, C) float32 rows, each normalised as set_terrain_class_coloring does (:384-388, torch float32) with its warning."""
        occ = torch.as_tensor(occupancy).detach().cpu().to(torch.float32).clone()
        if occ.dim() == 1:
            occ = occ.unsqueeze(0).repeat(self.batch, 1)
        if occ.dim() != 2 or occ.shape[0] != self.batch or occ.shape[1] < 1:
            raise ValueError(f"occupancy must be (C,) or ({self.batch}, C), got {tuple(torch.as_tensor(occupancy).shape)}")
        if occ.shape[1] > MAX_COLOR_CLASSES:
            raise ValueError(f"colouring supports 1 to {MAX_COLOR_CLASSES} terrain classes, got {occ.shape[1]}")
        if not bool(torch.isfinite(occ).all()) or bool((occ < 0).any()):
            raise ValueError("occupancy ratios must be finite and >= 0")
        if not bool((occ > 0).any(dim=1).all()):
            raise ValueError("every occupancy row needs a class with a ratio > 0")
        warned = False
        for row in occ:
            if row.sum() > 1:
                row /= row.sum()
                if not warned:
                    warnings.warn("Sum of occupancy vector exceeds one! The vector has been normalized.")
                    warned = True
        return occ

    def _noise_fields(self, noise) -> np.ndarray:
        B, G = self.batch, self.grid_size
        n = noise.detach().cpu().numpy() if isinstance(noise, torch.Tensor) else np.asarray(noise)
        if n.shape == (G, G):
            n = np.broadcast_to(n, (B, G, G))
        if n.shape != (B, G, G):
            raise ValueError(f"noise must be ({G}, {G}) or ({B}, {G}, {G}), got {n.shape}")
        return np.ascontiguousarray(n, dtype=np.float32)

    def _set_colored(self, draws, seeds, is_fractal, slip_models, occupancy, noise, feature_size, ambient_intensity) -> np.ndarray:
        """Validate and set the colouring step's inputs and the slip table; with `draws` (host draws) they are uploaded too and
        carry the light vectors, without, the light is left to the device draws of `seeds`.  Returns the (B, 3) light set."""
        B, G = self.batch, self.grid_size
        occ = self._occupancy_rows(occupancy)
        C_ = occ.shape[1]
        if draws is None:
            light = np.zeros((B, 3), np.float32)
        else:
            if any(d.light is None for d in draws):
                raise ValueError("colouring needs the light vectors: make the draws with replay_draws(..., coloring=True)")
            light = np.ascontiguousarray(np.stack([d.light for d in draws]), dtype=np.float32)
        thr = np.ascontiguousarray((torch.cumsum(occ, dim=1) * 100).numpy(), dtype=np.float32)          # :428, per row
        start = np.array([int((row > 0).nonzero().min().item()) for row in occ], np.int32)             # :431
        table = np.ascontiguousarray(_copper_table(C_))
        field_ = None
        if noise is not None:
            field_, seeds = self._noise_fields(noise), None
        elif draws is not None:
            if any(d.seed is None for d in draws):
                raise ValueError("the library's own noise is keyed by the instance seeds: draws without a seed need noise=")
            seeds = np.array([d.seed % (1 << 64) for d in draws], np.uint64)
        models = _default_slip_models(1) if slip_models is None else slip_models
        tab, nmodels = _as_param_table(models)
        if draws is not None:
            self.upload_draws(draws, is_fractal)
        self._check(self._lib.bn_terrain_set_coloring(
            self._handle, 1, thr.ctypes.data, start.ctypes.data, C_, table.ctypes.data, light.ctypes.data, float(ambient_intensity),
            float(feature_size), None if field_ is None else field_.ctypes.data, None if seeds is None else seeds.ctypes.data, nmodels))
        self._check(self._lib.bn_terrain_set_slip(self._handle, None, tab.ctypes.data, tab.shape[0]))
        return light

    def _check_class_counts(self) -> None:
        B = self.batch
        unassigned, beyond = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._check(self._lib.bn_terrain_class_counts(self._handle, unassigned.ctypes.data, beyond.ctypes.data))
        if unassigned.any():
            warnings.warn("Some grid cells have not been assigned a terrain class.")                    # :440-441
        if unassigned.any() or beyond.any():                                                            # set_traversability :554-557
            raise ValueError("The number of terrain classes exceeds the number of slip models.")

    def _generate_colored(self, draws, is_fractal, slip_models, occupancy, noise, feature_size, ambient_intensity) -> Terrain:
        light = self._set_colored(draws, None, is_fractal, slip_models, occupancy, noise, feature_size, ambient_intensity)
        self._check(self._lib.bn_terrain_generate_async(self._handle, stream_ptr(self._dev)))
        self._check_class_counts()
        out = self.outputs()
        cls, colors, nz = self._color_outputs()
        self._last = Terrain(*out, t_classes=cls.cpu().to(torch.int64), craters=self._crater_tables(draws), draws=draws,
                             colors=colors, noise=nz, light=light, classes_device=cls)
        return self._last

    def _generate_device(self, seeds, is_fractal, geometry, coloring, t_classes, slip_models, occupancy, noise, feature_size,
                         ambient_intensity) -> Terrain:
        """generate() with the draws made on the device: parameters, one draws launch, the generation, one small read-back."""
        B, G = self.batch, self.grid_size
        is_crater, num_craters, crater_margin, min_angle, max_angle, min_radius, max_radius = geometry
        lo, hi = (0.8, 1.0) if coloring is None else coloring
        keys = np.array([s % (1 << 64) for s in seeds], np.uint64)
        stream = stream_ptr(self._dev)
        self._check(self._lib.bn_terrain_set_geometry(self._handle, self.resolution, self.roughness_exponent, self.amplitude_gain,
                                                      int(bool(is_fractal))))
        self._check(self._lib.bn_terrain_set_draw_params(self._handle, int(bool(is_crater)), int(num_craters), float(crater_margin),
                                                         float(min_angle), float(max_angle), float(min_radius), float(max_radius),
                                                         int(coloring is not None), float(lo), float(hi)))
        if coloring is not None:
            self._set_colored(None, keys, is_fractal, slip_models, occupancy, noise, feature_size, ambient_intensity)
        else:
            self._check(self._lib.bn_terrain_set_coloring(self._handle, 0, None, None, 0, None, None, 0.0, 0.0, None, None, 0))
            cls = self._class_maps(t_classes)
            models = _default_slip_models(1) if slip_models is None else slip_models
            tab, nmodels = _as_param_table(models)
            present = np.unique(cls)
            if present.min() < 0 or present.max() >= nmodels:                                    # set_traversability :556-559
                raise ValueError("The number of terrain classes exceeds the number of slip models.")
            cls32 = np.ascontiguousarray(cls, dtype=np.int32)
            self._check(self._lib.bn_terrain_set_slip(self._handle, cls32.ctypes.data, tab.ctypes.data, tab.shape[0]))
        self._check(self._lib.bn_terrain_draw_async(self._handle, keys.ctypes.data, stream))
        slots, stride = C.c_int32(), C.c_int32()                  # the sizes of the tables the read-back copies
        self._check(self._lib.bn_terrain_draw_layout(self._handle, C.byref(slots), C.byref(stride)))
        self._device = {"seeds": [int(s) for s in seeds], "light": coloring is not None, "fractal": bool(is_fractal),
                        "slots": slots.value, "stride": stride.value}
        self._check(self._lib.bn_terrain_generate_async(self._handle, stream))
        drawn = self._read_draws(full=False)
        if coloring is not None:
            self._check_class_counts()
        out = self.outputs()
        if coloring is not None:
            cls_t, colors, nz = self._color_outputs()
            self._last = Terrain(*out, t_classes=cls_t.cpu().to(torch.int64), craters=self._crater_tables(drawn), draws=drawn,
                                 colors=colors, noise=nz, light=np.stack([d.light for d in drawn]), classes_device=cls_t)
        else:
            with torch.cuda.device(self._dev):
                colors = torch.zeros((B, 3, G, G), device=self._dev)
            self._last = Terrain(*out, t_classes=torch.from_numpy(cls.astype(np.int64)), craters=self._crater_tables(drawn),
                                 draws=drawn, colors=colors)
        return self._last

    def _read_draws(self, full: bool) -> List[Draws]:
        """The draws the device made last, one Draws per instance: the records and crater tables and, with `full`, each crater's
        profile coordinates and the phases.  Raises what replay_draws raises (check_draw_records)."""
        B, G = self.batch, self.grid_size
        dev = getattr(self, "_device", None)
        if dev is None:
            raise RuntimeError('generate(..., draws="device") has not run')
        slots, stride = dev["slots"], dev["stride"]
        rec = np.zeros((B, 4), np.int32)
        centers, angles = np.zeros((B, slots, 2), np.float32), np.zeros((B, slots), np.float64)
        ints, vals = np.zeros((B, slots, 8), np.int32), np.zeros((B, slots, 2), np.float32)
        light_u, light = np.zeros((B, 2), np.float32), np.zeros((B, 3), np.float32)
        lin = np.zeros((B, slots, stride), np.float32) if full else None
        ph = np.zeros((B, num_phases(G)), np.float32) if full and dev["fractal"] else None
        self._check(self._lib.bn_terrain_read_draws(
            self._handle, rec.ctypes.data, centers.ctypes.data, angles.ctypes.data, light_u.ctypes.data,
            light.ctypes.data if dev["light"] else None, ints.ctypes.data, vals.ctypes.data,
            None if lin is None else lin.ctypes.data, None if ph is None else ph.ctypes.data))
        check_draw_records(rec, vals[:, :, 0], G)
        out = []
        for b in range(B):
            craters = []
            for j in range(int(rec[b, 3])):
                n = int(ints[b, j, 6])
                craters.append(Crater(centers[b, j].copy(), float(vals[b, j, 0]), float(angles[b, j]), n, tuple(int(v) for v in ints[b, j, :6]),
                                      lin[b, j, :n].copy() if full else np.zeros(0, np.float32), float(vals[b, j, 1])))
            d = Draws(craters, int(rec[b, 0]), bool(rec[b, 1]), ph[b].copy() if ph is not None else np.zeros(0, np.float32),
                      seed=dev["seeds"][b])
            if dev["light"]:
                d.light_uniforms, d.light = light_u[b].copy(), light[b].copy()
            out.append(d)
        return out

    def device_draws(self) -> List[Draws]:
        """The draws of the last generate(..., draws="device") as full Draws objects (profile coordinates and phases included), as
        replay_draws would return them: generate_from_draws() takes them."""
        return self._read_draws(full=True)

    def _color_outputs(self):
        """(classes int32 (B, G, G), colours (B, 3, G, G), noise (B, G, G)) device tensors (copies)."""
        ptrs = [C.c_void_p() for _ in range(3)]
        self._check(self._lib.bn_terrain_color_buffers(self._handle, *[C.byref(p) for p in ptrs]))
        B, G = self.batch, self.grid_size
        with torch.cuda.device(self._dev):
            cls = self.view(ptrs[0].value, (B, G, G), "<i4").clone()
            colors = self.view(ptrs[1].value, (B, 3, G, G)).clone()
            nz = self.view(ptrs[2].value, (B, G, G)).clone()
        return cls, colors, nz

    def colorize(self, heights, t_classes, num_classes: int, light, ambient_intensity: float = 0.1) -> torch.Tensor:
        """(B, 3, G, G) device colours of create_color_map + create_shading (terrain_properties.py:462-523) for given (B, G, G)
        heights and classes and (B, 3) light vectors (light_source() makes one the reference's way); `num_classes` sizes the
        copper table.  Also how an instance stored without colours gets them."""
        B, G = self.batch, self.grid_size
        h = heights.detach().cpu().numpy() if isinstance(heights, torch.Tensor) else np.asarray(heights)
        if h.shape == (G, G):
            h = h[None]
        if h.shape != (B, G, G):
            raise ValueError(f"heights must be ({B}, {G}, {G}), got {h.shape}")
        h = np.ascontiguousarray(h, dtype=np.float32)
        cls = np.ascontiguousarray(self._class_maps(t_classes), dtype=np.int32)
        L = np.asarray(light.detach().cpu().numpy() if isinstance(light, torch.Tensor) else light, dtype=np.float32)
        if L.shape == (3,):
            L = np.broadcast_to(L, (B, 3))
        if L.shape != (B, 3):
            raise ValueError(f"light must be (3,) or ({B}, 3), got {L.shape}")
        L = np.ascontiguousarray(L)
        table = np.ascontiguousarray(_copper_table(num_classes))
        self._check(self._lib.bn_terrain_colorize(self._handle, h.ctypes.data, cls.ctypes.data, table.ctypes.data, int(num_classes),
                                                  L.ctypes.data, float(ambient_intensity), stream_ptr(self._dev)))
        return self._color_outputs()[1]

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
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self._lib.bn_terrain_buffers(self._handle, *[C.byref(p) for p in ptrs]))
        shape = (self.batch, self.grid_size, self.grid_size)
        with torch.cuda.device(self._dev):
            return tuple(self.view(p.value, shape).clone() for p in ptrs)

    def spectrum(self, instance: int = 0) -> np.ndarray:
        """Test hook: the scaled fBm spectrum of `instance` that the inverse DFT reads, (G+2, G+2) complex64."""
        N = self.grid_size + 2
        buf = np.empty((N, N, 2), np.float32)
        self._check(self._lib.bn_terrain_spectrum(self._handle, instance, buf.ctypes.data))
        return buf[..., 0] + 1j * buf[..., 1]

    def to_instances(self):
        """The last generate() as io.MapInstance objects (CPU tensors, the reference's on-disk layout; colours are zero unless
        the generation coloured them)."""
        from .io import MapInstance
        t = self._last
        if t is None:
            raise RuntimeError("generate() has not run")
        G = self.grid_size
        out = []
        for b in range(self.batch):
            tensors = {"heights": t.heights[b].cpu(), "slopes": t.slopes[b].cpu(), "t_classes": t.t_classes[b].clone(),
                       "colors": torch.zeros(3, G, G) if t.colors is None else t.colors[b].cpu()}
            out.append(MapInstance(grid_size=G, tensors=tensors, latent_mean=t.latent_mean[b].cpu(),
                                   latent_std=t.latent_std[b].cpu(), extra={"craters": t.craters[b]}))
        return out
