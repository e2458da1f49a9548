"""The dataset stage on the GPU: splits of map instances, their slip observations and the three dataset views.

Mirror of the reference's `DatasetGenerator.generate_dataset` (src/data/dataset_generator.py:92-190) and of the three `Dataset`
classes of src/data/terrain_dataset.py, the objects `ClassifierTrainer` and `SlipRegressorTrainer` are constructed with:

    models = slip_models(10)
    train = DatasetGenerator(models, None, "train", 64, 0.5, environment_count=10, instance_count=8, batch=16).generate_dataset()
    valid = DatasetGenerator(models, None, "valid", 64, 0.5, 10, 2, batch=16, seed_information=train.seed_information).generate_dataset()
    ClassifierTrainer(state_dict, model_dir, params, TerrainClassificationDataset(train), TerrainClassificationDataset(valid)).train()
    SlipRegressorTrainer(dev, model_dir, data_dir, 10, params, SlipRegressionDataset(train)).train_all_models()

A split lives on the device (`TerrainDataset`): the maps are generated `batch` per launch by `TerrainGenerator(draws="device")`
and copied into (M, ...) tensors; with a `data_directory` the reference's files are written as well (`io.save_instance`, one
`{e:03d}_{i:03d}.pt` per map and `seed_information.pt`), and `TerrainDataset.from_directory` reads such a directory back.  The
seed chain across the splits is the reference's `set_seed`; without a directory it is passed in memory (`seed_information=`).
The planning half -- seeds, occupancy rows, file names (`plan_split`, `DatasetGenerator.plan`) -- needs no device.

The slip observations of `SlipRegressionDataset` (the reference draws `latent_models.sample()` per item from torch's global
generator) are a keyed Philox stream of (observation_seed, map index, epoch): an item is the same whenever it is asked for, and
`set_epoch` moves every map to fresh draws.  `gather_observations` is `RegressorTrainer.load_data`'s
per-class, capped, order-preserving concatenation as three kernel launches over the whole split (csrc/dataset_kernels.hip).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._device import check, resolve_device, stream_ptr

SPLITS = ("train", "valid", "test")
MAX_CLASSES = 64                          # csrc/dataset_kernels.hip keeps the per-class tables in LDS
MAX_MAPS = 1 << 32                        # the map index is one 32-bit counter word of the observation stream


@dataclass
class ParamsTerrainGeometry:
    """The fields of the reference's ParamsTerrainGeometry (src/data/utils.py) with set_terrain_geometry's defaults."""
    is_fractal: bool = True
    is_crater: bool = True
    num_craters: int = 3
    crater_margin: float = 5
    min_angle: float = 10
    max_angle: float = 20
    min_radius: float = 5
    max_radius: float = 10


@dataclass
class ParamsTerrainColoring:
    """The fields of the reference's ParamsTerrainColoring that generate_map_instance reads, with their defaults."""
    lower_threshold: float = 0.8
    upper_threshold: float = 1.0
    ambient_intensity: float = 0.1


# ---- the planning half: no device ------------------------------------------------------------------------------------------
def _check_split(data_split, subset_index, what: str) -> None:
    if data_split not in SPLITS:
        raise ValueError("data_split must be one of 'train', 'valid', 'test'")
    if data_split == "test" and subset_index is None:
        raise ValueError(what)


def split_directory(data_split: str, subset_index: Optional[int] = None) -> str:
    """A split's directory relative to the data directory: `train`, `valid`, `test/subsetNN`."""
    return os.path.join("test", f"subset{subset_index:02d}") if data_split == "test" else data_split


def previous_split(data_split: str, subset_index: Optional[int] = None) -> Optional[str]:
    """The relative directory whose seed_information.pt the split continues from (set_seed, :154-190): none for train, train for
    valid, valid for test subset 1, subset k - 1 for test subset k."""
    if data_split == "train":
        return None
    if data_split == "valid":
        return "train"
    return "valid" if subset_index == 1 else split_directory("test", subset_index - 1)


@dataclass
class SplitPlan:
    """What generate_dataset decides before any map exists.  Map m = e * instance_count + i has seeds[m], occupancy row
    environments[m] = e and the file file_names[m] (relative to the data directory)."""
    environment_seed: int
    base_instance_seed: int
    last_instance_seed: int
    seeds: List[int]
    environments: List[int]
    file_names: List[str]
    occupancy: torch.Tensor                # (environment_count, num_total_terrain_classes) float32
    directory: str                         # the split's relative directory

    @property
    def seed_information(self) -> Dict[str, int]:
        return {"environment_seed": self.environment_seed, "last_instance_seed": self.last_instance_seed}


def plan_split(data_split: str, subset_index: Optional[int], environment_count: int, instance_count: int, environment_seed: int,
               base_instance_seed: int, num_total_terrain_classes: int = 10, num_selected_terrain_classes: int = 4) -> SplitPlan:
    """generate_dataset's bookkeeping (:99-152, :278-308): environment e's group starts at base + e * instance_count and counts up
    by one per instance; the occupancy table is generate_occupancy_distribution(environment_seed)."""
    from .terrain import occupancies
    E, N = int(environment_count), int(instance_count)
    rel = split_directory(data_split, subset_index)
    seeds, envs, names = [], [], []
    for e in range(E):
        for i in range(N):
            seeds.append(int(base_instance_seed) + e * N + i)
            envs.append(e)
            names.append(os.path.join(rel, f"{e:03d}_{i:03d}.pt"))
    occ = occupancies(E, num_total_terrain_classes, num_selected_terrain_classes, seed=int(environment_seed))
    return SplitPlan(int(environment_seed), int(base_instance_seed), int(base_instance_seed) + E * N, seeds, envs, names, occ, rel)


def _load_seed_information(path: str) -> Dict[str, int]:
    info = torch.load(path, map_location="cpu", weights_only=True)
    return {"environment_seed": int(info["environment_seed"]), "last_instance_seed": int(info["last_instance_seed"])}


# ---- the two device operations -----------------------------------------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _maps(t, dev: torch.device, dtype, name: str, shape=None) -> torch.Tensor:
    t = torch.as_tensor(t)
    if t.dim() < 2:
        raise ValueError(f"{name} must be (M, ...) maps, got shape {tuple(t.shape)}")
    t = t.detach().to(dev, dtype).reshape(t.shape[0], -1).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must hold {shape[0]} maps of {shape[1]} cells, got {tuple(t.shape)}")
    return t


def _raise(lib, code: int) -> None:
    if code == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_dataset_last_error().decode("utf-8", "replace"))
    check(lib, "dataset", code)


def sample_slips(mean, std, seed: int = 0, epoch: int = 0, first_map: int = 0, z=None, device=None) -> torch.Tensor:
    """Slip observations of maps first_map, first_map + 1, ...: mean and std (M, ...) -> slips of mean's shape on the device, on
    torch's current stream.  `z` of the same shape replaces the stream's normals (slips = z * std + mean bit for bit)."""
    dev = resolve_device(device if device is not None else (mean.device if isinstance(mean, torch.Tensor) and mean.is_cuda else None), "dataset")
    lib = _capi.load()
    shape = tuple(torch.as_tensor(mean).shape)
    with torch.cuda.device(dev):
        m = _maps(mean, dev, torch.float32, "mean")
        s = _maps(std, dev, torch.float32, "std", m.shape)
        zz = None if z is None else _maps(z, dev, torch.float32, "z", m.shape)
        out = torch.empty_like(m)
        _raise(lib, lib.bn_dataset_sample_slips_async(dev.index, stream_ptr(dev), _ptr(m), _ptr(s), _ptr(zz), m.shape[0], m.shape[1], int(first_map),
                                                      int(seed) % (1 << 64), int(epoch) % (1 << 32), _ptr(out)))
    return out.reshape(shape)


def _order_tensor(order, M: int, dev: torch.device) -> Optional[torch.Tensor]:
    if order is None:
        return None
    o = torch.as_tensor(order).detach().cpu().to(torch.int64).reshape(-1)
    if o.numel() != M or not torch.equal(torch.sort(o).values, torch.arange(M)):
        raise ValueError(f"order must be a permutation of the {M} maps")
    return o.to(dev)


def gather(slopes, classes, num_classes: int, cap: int, slips=None, mean=None, std=None, order=None, seed: int = 0, epoch: int = 0,
           x: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, device=None):
    """bn_dataset_gather_async on torch's current stream: (x, y, counts, totals) with x, y (num_classes, cap) float32, counts
    (num_classes) int32 and totals (num_classes) int64 on the device.  Row k of x / y holds the slopes / slips of class k's cells,
    map after map in `order` (a permutation of the maps; None: 0, 1, ...), row-major inside a map, cut at cap; what lies beyond
    counts[k] keeps what the given x and y held (zeros when they are allocated here).  Without `slips` the kept cells' observations
    are drawn from mean and std with (seed, epoch)."""
    src = slopes if isinstance(slopes, torch.Tensor) and slopes.is_cuda else None
    dev = resolve_device(device if device is not None else (src.device if src is not None else None), "dataset")
    lib = _capi.load()
    Cn, cap = int(num_classes), int(cap)
    with torch.cuda.device(dev):
        sl = _maps(slopes, dev, torch.float32, "slopes")
        M, cells = sl.shape
        cl = _maps(classes, dev, torch.int32, "classes", sl.shape)
        sp = None if slips is None else _maps(slips, dev, torch.float32, "slips", sl.shape)
        mu = None if mean is None else _maps(mean, dev, torch.float32, "mean", sl.shape)
        sd = None if std is None else _maps(std, dev, torch.float32, "std", sl.shape)
        od = _order_tensor(order, M, dev)
        if Cn < 1 or Cn > MAX_CLASSES:
            raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}]")
        if cap < 1:
            raise ValueError("cap must be >= 1")
        for name, t in (("x", x), ("y", y)):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (Cn, cap) or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous ({Cn}, {cap}) float32 device tensor")
        x = torch.zeros(Cn, cap, device=dev) if x is None else x
        y = torch.zeros(Cn, cap, device=dev) if y is None else y
        counts = torch.zeros(Cn, device=dev, dtype=torch.int32)
        totals = torch.zeros(Cn, device=dev, dtype=torch.int64)
        nbytes = lib.bn_dataset_gather_workspace_bytes(M, Cn)
        if nbytes == 0:
            raise ValueError(f"{M} maps with {Cn} classes are out of the library's range")
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)          # torch's allocator keeps it alive for the stream
        _raise(lib, lib.bn_dataset_gather_async(dev.index, stream_ptr(dev), _ptr(sl), _ptr(sp), _ptr(mu), _ptr(sd), _ptr(cl), _ptr(od), M, cells, Cn, cap,
                                                int(seed) % (1 << 64), int(epoch) % (1 << 32), _ptr(x), _ptr(y), _ptr(counts), _ptr(totals), _ptr(work),
                                                nbytes))
    return x, y, counts, totals


# ---- the split on the device ---------------------------------------------------------------------------------------------------
class TerrainDataset:
    """One split on the device: heights, slopes, latent_mean, latent_std (M, G, G) float32, colors (M, 3, G, G) float32,
    t_classes (M, G, G) int32 (the generator's device class buffer; items come out as int64, as the reference stores them) and
    seeds (M) int64 on the host.  `names` are the maps' file names relative to the data directory, `seed_information` the two
    values the next split continues from.  observation_seed and epoch key the slip observations (set_epoch)."""

    def __init__(self, heights, slopes, latent_mean, latent_std, colors, t_classes, seeds, names: Optional[Sequence[str]] = None,
                 seed_information: Optional[Dict[str, int]] = None, observation_seed: int = 0, epoch: int = 0) -> None:
        self.heights, self.slopes, self.latent_mean, self.latent_std = heights, slopes, latent_mean, latent_std
        self.colors, self.t_classes = colors, t_classes
        self.seeds = torch.as_tensor(seeds, dtype=torch.int64).reshape(-1)
        M = heights.shape[0]
        if M >= MAX_MAPS:
            raise ValueError("a split holds fewer than 2^32 maps")
        self.names = list(names) if names is not None else [f"{m:06d}.pt" for m in range(M)]
        self.seed_information = seed_information
        self.observation_seed, self.epoch = int(observation_seed), int(epoch)

    def __len__(self) -> int:
        return int(self.heights.shape[0])

    @property
    def device(self) -> torch.device:
        return self.heights.device

    @property
    def grid_size(self) -> int:
        return int(self.heights.shape[-1])

    def set_epoch(self, epoch: int) -> None:
        """Every map's slip observations move to the draws of `epoch`; nothing else changes."""
        self.epoch = int(epoch)

    def index(self, index) -> int:
        M, m = len(self), int(index)
        if m < -M or m >= M:
            raise IndexError(f"index {m} is out of range for a split of {M} maps")
        return m % M

    def classes(self, m: int) -> torch.Tensor:
        return self.t_classes[m].to(torch.int64)

    def slips(self, m: int) -> torch.Tensor:
        """(G, G) slip observations of map m at the current epoch."""
        return sample_slips(self.latent_mean[m:m + 1], self.latent_std[m:m + 1], self.observation_seed, self.epoch, first_map=m)[0]

    @classmethod
    def from_directory(cls, data_directory: str, data_split: str, subset_index: Optional[int] = None, device=None) -> "TerrainDataset":
        """Load the reference's files of one split with io.load_instance.  The maps come in the SORTED order of their file
        names (environment, then instance: generate_dataset's order); the reference's BaseDataset keeps os.listdir's order,
        which is arbitrary, so an index there and here need not name the same map."""
        from .io import load_instance
        _check_split(data_split, subset_index, "subset index must be specified for the test split")
        dev = resolve_device(device, "dataset", lenient=True)
        rel = split_directory(data_split, subset_index)
        folder = os.path.join(data_directory, rel)
        files = sorted(f for f in os.listdir(folder) if f != "seed_information.pt")
        if not files:
            raise ValueError(f"{folder} holds no map instance")
        insts = [load_instance(os.path.join(folder, f)) for f in files]
        info_path = os.path.join(folder, "seed_information.pt")
        info = _load_seed_information(info_path) if os.path.exists(info_path) else None
        M = len(insts)
        seeds = list(range(info["last_instance_seed"] - M, info["last_instance_seed"])) if info is not None else [-1] * M

        def stack(get, dtype):
            return torch.stack([get(i).to(dtype) for i in insts]).to(dev).contiguous()
        return cls(stack(lambda i: i.tensors["heights"], torch.float32), stack(lambda i: i.tensors["slopes"], torch.float32),
                   stack(lambda i: i.latent_mean, torch.float32), stack(lambda i: i.latent_std, torch.float32),
                   stack(lambda i: i.tensors["colors"], torch.float32), stack(lambda i: i.tensors["t_classes"], torch.int32), seeds,
                   names=[os.path.join(rel, f) for f in files], seed_information=info)

    def to_instances(self):
        """The maps as io.MapInstance objects (CPU tensors, the reference's on-disk layout: t_classes int64)."""
        from .io import MapInstance
        h, s, c, t = self.heights.cpu(), self.slopes.cpu(), self.colors.cpu(), self.t_classes.cpu().to(torch.int64)
        mu, sd = self.latent_mean.cpu(), self.latent_std.cpu()
        return [MapInstance(grid_size=self.grid_size, tensors={"heights": h[m].clone(), "slopes": s[m].clone(), "t_classes": t[m].clone(),
                                                               "colors": c[m].clone()},
                            latent_mean=mu[m].clone(), latent_std=sd[m].clone(), extra={"seed": int(self.seeds[m])}) for m in range(len(self))]

    def save(self, data_directory: str) -> None:
        """Write every map to <data_directory>/<its name> (io.save_instance) and, if known, the split's seed_information.pt."""
        from .io import save_instance
        for inst, name in zip(self.to_instances(), self.names):
            path = os.path.join(data_directory, name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            save_instance(path, inst)
        if self.seed_information is not None and self.names:
            torch.save(dict(self.seed_information), os.path.join(data_directory, os.path.dirname(self.names[0]), "seed_information.pt"))


class _View(torch.utils.data.Dataset):
    """A dataset view: constructed on a TerrainDataset, or with the reference's (data_directory, data_split, subset_index,
    device) on a directory of its files."""

    def __init__(self, data, data_split: Optional[str] = None, subset_index: Optional[int] = None, device=None) -> None:
        if not isinstance(data, TerrainDataset):
            data = TerrainDataset.from_directory(data, data_split, subset_index, device)
        self.data = data
        self.device = data.device

    def __len__(self) -> int:
        return len(self.data)

    def set_epoch(self, epoch: int) -> None:
        self.data.set_epoch(epoch)


class TerrainClassificationDataset(_View):
    """Items (colors (3, G, G) float32, t_classes (G, G) int64), device tensors."""

    def __getitem__(self, index) -> Tuple[torch.Tensor, torch.Tensor]:
        m = self.data.index(index)
        return self.data.colors[m], self.data.classes(m)


class SlipRegressionDataset(_View):
    """Items (slopes, slips, t_classes), (G, G) device tensors; slips are the observation stream's draws for (observation_seed,
    map index, epoch) where the reference samples the latent model from torch's global generator."""

    def __getitem__(self, index) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        m = self.data.index(index)
        return self.data.slopes[m], self.data.slips(m), self.data.classes(m)

    def gather_observations(self, num_classes: int, num_samples: int = 9999, order=None):
        """RegressorTrainer.load_data over the whole split on the device: (phis, slips, counts, totals).  phis[k] and slips[k] are
        the slopes and slip observations of class k's cells, map after map in `order` (a permutation of the maps; None: 0, 1, ...),
        row-major inside a map, cut at num_samples -- device tensors of counts[k] elements; counts and totals are (num_classes)
        int64 host tensors, totals the number of cells of each class in the split.  The observations are the items' (the same
        stream), drawn only for the cells that are kept."""
        d = self.data
        x, y, counts, totals = gather(d.slopes, d.t_classes, num_classes, num_samples, mean=d.latent_mean, std=d.latent_std, order=order,
                                      seed=d.observation_seed, epoch=d.epoch)
        counts, totals = counts.cpu().to(torch.int64), totals.cpu()
        phis = {k: x[k, :int(counts[k])] for k in range(int(num_classes))}
        slips = {k: y[k, :int(counts[k])] for k in range(int(num_classes))}
        return phis, slips, counts, totals


class TraversabilityPredictionDataset(_View):
    """Items (colors (3, G, G), slopes, latent mean, latent stddev (G, G)), device tensors."""

    def __getitem__(self, index) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        m = self.data.index(index)
        return self.data.colors[m], self.data.slopes[m], self.data.latent_mean[m], self.data.latent_std[m]


# ---- the generator ---------------------------------------------------------------------------------------------------------------
class DatasetGenerator:
    """The reference's DatasetGenerator (dataset_generator.py:25-190) around TerrainGenerator: same constructor, same seed
    chain, same files.  Additions: batch= (maps per launch), noise= (None: the library's own seeded noise, not OpenSimplex; a
    callable (seed, G) -> (G, G) field lets a caller with the real opensimplex supply the reference's), seed_information= (the
    previous split's {"environment_seed", "last_instance_seed"} when data_directory is None).
    data_directory=None keeps the split in memory only.  Nothing here touches the device before generate_dataset()."""

    def __init__(self, slip_models, data_directory: Optional[str], data_split: str, grid_size: int, resolution: float, environment_count: int,
                 instance_count: int, num_total_terrain_classes: int = 10, num_selected_terrain_classes: int = 4,
                 params_terrain_geometry=None, params_terrain_coloring=None, subset_index: Optional[int] = None, device=None, *,
                 batch: int = 16, noise: Optional[Callable] = None, seed_information: Optional[Dict[str, int]] = None) -> None:
        self.slip_models = slip_models
        _check_split(data_split, subset_index, "subset_index must be specified for generating test data.")
        self.data_directory, self.data_split = data_directory, data_split
        self.subset_index = subset_index if data_split == "test" else None
        self.grid_size, self.resolution = int(grid_size), float(resolution)
        self.environment_count, self.instance_count = int(environment_count), int(instance_count)
        self.num_total_terrain_classes, self.num_selected_terrain_classes = int(num_total_terrain_classes), int(num_selected_terrain_classes)
        self.params_terrain_geometry = params_terrain_geometry if params_terrain_geometry is not None else ParamsTerrainGeometry()
        self.params_terrain_coloring = params_terrain_coloring if params_terrain_coloring is not None else ParamsTerrainColoring()
        self.device = device
        if int(batch) < 1:
            raise ValueError("batch must be >= 1")
        self.batch, self.noise = int(batch), noise
        self.seed_information = seed_information

    def set_seed(self) -> Tuple[int, int]:
        """(environment_seed, base_instance_seed): (0, 0) for train, else the previous split's seed information -- read from its
        seed_information.pt, or with data_directory=None the `seed_information` given to the constructor."""
        prev = previous_split(self.data_split, self.subset_index)
        if prev is None:
            return 0, 0
        if self.data_directory is None:
            if self.seed_information is None:
                raise ValueError(f"without a data directory the {self.data_split} split needs seed_information= of the {prev} split")
            info = self.seed_information
        else:
            info = _load_seed_information(os.path.join(self.data_directory, prev, "seed_information.pt"))
        return int(info["environment_seed"]), int(info["last_instance_seed"])

    def generate_occupancy_distribution(self, seed: int) -> torch.Tensor:
        from .terrain import occupancies
        return occupancies(self.environment_count, self.num_total_terrain_classes, self.num_selected_terrain_classes, seed=int(seed))

    def plan(self) -> SplitPlan:
        """The split's seeds, occupancy rows and file names: everything generate_dataset decides before it generates."""
        environment_seed, base_instance_seed = self.set_seed()
        return plan_split(self.data_split, self.subset_index, self.environment_count, self.instance_count, environment_seed, base_instance_seed,
                          self.num_total_terrain_classes, self.num_selected_terrain_classes)

    def generate_dataset(self, processes: int = 4) -> TerrainDataset:
        """Generate the split, `batch` maps per launch (the last launch holds the rest; a launch may span environments), and
        return it on the device.  With a data directory the reference's files are written too.  `processes` is accepted and
        ignored: there is no worker pool."""
        from .terrain import TerrainGenerator
        plan = self.plan()
        dev = resolve_device(self.device, "dataset", lenient=True)
        M, G = len(plan.seeds), self.grid_size
        if M < 1:
            raise ValueError("environment_count and instance_count must be >= 1")
        g, c = self.params_terrain_geometry, self.params_terrain_coloring
        with torch.cuda.device(dev):
            maps = {k: torch.empty(M, G, G, device=dev) for k in ("heights", "slopes", "latent_mean", "latent_std")}
            colors = torch.empty(M, 3, G, G, device=dev)
            classes = torch.empty(M, G, G, device=dev, dtype=torch.int32)
        generators: Dict[int, TerrainGenerator] = {}
        try:
            for s in range(0, M, self.batch):
                n = min(self.batch, M - s)
                if n not in generators:
                    generators[n] = TerrainGenerator(G, self.resolution, batch=n, device_id=dev.index)
                seeds = plan.seeds[s:s + n]
                field = None if self.noise is None else np.stack([np.asarray(self.noise(seed, G), np.float32).reshape(G, G) for seed in seeds])
                t = generators[n].generate(seeds, is_fractal=g.is_fractal, is_crater=g.is_crater, num_craters=g.num_craters,
                                           crater_margin=g.crater_margin, min_angle=g.min_angle, max_angle=g.max_angle, min_radius=g.min_radius,
                                           max_radius=g.max_radius, slip_models=self.slip_models, occupancy=plan.occupancy[plan.environments[s:s + n]],
                                           noise=field, lower_threshold=c.lower_threshold, upper_threshold=c.upper_threshold,
                                           ambient_intensity=c.ambient_intensity, draws="device")
                for k in maps:
                    maps[k][s:s + n] = getattr(t, k)
                colors[s:s + n] = t.colors
                classes[s:s + n] = t.classes_device
        finally:
            for gen in generators.values():
                gen.close()
        data = TerrainDataset(maps["heights"], maps["slopes"], maps["latent_mean"], maps["latent_std"], colors, classes, plan.seeds,
                              names=plan.file_names, seed_information=plan.seed_information)
        if self.data_directory is not None:
            data.save(self.data_directory)
        return data
