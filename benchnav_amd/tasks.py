"""The task stage on the device: which start/goal pairs of a map can be solved at all, and how long their best path is
(DESIGN.md 4.16).

    tasks = TaskSet.sample(test_split, trials=4, seed=0, min_separation=10.0)
    report = Benchmark(test_split, predictor, trials=4, tasks=tasks).run("mppi", ["expected_value", "cvar@0.9"])
    print(report.table())                  # ... with an `spl` column

Three steps on arrays that already sit on the device (csrc/task_kernels.hip): `passable_mask` marks the truly passable ground of B
maps (the environment step's stuck rule on the latent slip), `label_components` labels its 4- or 8-connected regions -- a cell's
label is the smallest linear index of its region, so the result is unique --, and `sample_pairs` draws start/goal pairs that lie in
one region, far enough apart (Philox, keyed by seed, map, pair and attempt: a pair is a function of those alone).
`optimal_lengths` gives every pair the length L* of the shortest 8-connected grid path over the passable cells, D[start] of the
existing A* field on flat ground.  Positions are CELL CENTRES: `ix * resolution`, the reference's rule, maps back to cell ix - 1
under the float32 lookup floor((p - x0) / res) for some ix at 0.3 m per cell; centres map back for every resolution and size tried.

SPL (success weighted by path length) of a setting is the mean over its valid episodes of [outcome == GOAL] * L* / max(L, L*).
Two biases are stated, not corrected: L* is the GRID optimum with A*'s edges (a diagonal step between two passable cells, whatever
its corner cells hold), at most 1.0824 times the any-angle optimum, so a good planner's L may undercut it; and an episode ends
within the goal radius, which shortens a real path further.  The max() absorbs both: such an episode counts 1.

`TaskSet`'s arithmetic and JSON need no device."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi
from ._device import _DevArray, check, resolve_device, stream_ptr

MAX_ATTEMPTS, MAX_PAIRS, STATS = _capi.BN_TASK_MAX_ATTEMPTS, _capi.BN_TASK_MAX_PAIRS, _capi.BN_TASK_STATS
STAT_NAMES = ("passable", "components", "largest", "largest_label", "errors")
GOAL, INVALID = _capi.BN_OUTCOME_GOAL, _capi.BN_OUTCOME_INVALID

_p = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def _raise(lib, code: int) -> None:
    if code == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_task_last_error().decode("utf-8", "replace"))
    check(lib, "task", code)


def _device_of(device, *tensors) -> torch.device:
    src = next((t for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), None)
    return resolve_device(device if device is not None else (src.device if src is not None else None), "tasks")


def _shape3(t, name: str) -> Tuple[int, int, int]:
    shape = tuple(torch.as_tensor(t).shape)
    if len(shape) != 3:
        raise ValueError(f"{name} must be (M, H, W), got shape {shape}")
    return shape


def _maps3(t, dev: torch.device, dtype, name: str) -> torch.Tensor:
    _shape3(t, name)
    return torch.as_tensor(t).detach().to(dev, dtype).contiguous()


# ---- the three device steps ------------------------------------------------------------------------------------------------------
def passable_mask(mean, std, kappa: float = 0.0, stuck_threshold: float = 0.1, device=None) -> torch.Tensor:
    """(M, H, W) uint8 on the device, one launch on torch's current stream (bn_task_mask_async): 1 where mean and std are finite
    and 1 - clamp(mean + kappa * std, 0, 1) > stuck_threshold in float32 -- evaluate.py's stuck(v) rule at the latent slip
    mean + kappa std; kappa = 0 reads the mean."""
    if not math.isfinite(float(kappa)) or not math.isfinite(float(stuck_threshold)):
        raise ValueError("kappa and stuck_threshold must be finite")
    if _shape3(std, "std") != _shape3(mean, "mean"):
        raise ValueError(f"std must have mean's shape {_shape3(mean, 'mean')}, got {_shape3(std, 'std')}")
    dev = _device_of(device, mean, std)
    lib = _capi.load()
    with torch.cuda.device(dev):
        mu = _maps3(mean, dev, torch.float32, "mean")
        sd = _maps3(std, dev, torch.float32, "std")
        M, H, W = mu.shape
        mask = torch.empty(M, H, W, device=dev, dtype=torch.uint8)
        _raise(lib, lib.bn_task_mask_async(dev.index, stream_ptr(dev), _p(mu), _p(sd), M, H * W, float(kappa), float(stuck_threshold), _p(mask)))
    return mask


def label_components(mask, connectivity: int = 4, device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(labels (M, H, W) int32, sizes (M, H * W) int32, stats (M, 8) int32) on the device (bn_task_label_async; the header
    defines every entry).  mask: (M, H, W), non-zero = passable.  Reads the statistics back once and raises where a map's error
    flag is set (a loop of the labelling reached its bound: its labels are not to be used)."""
    if int(connectivity) not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    _shape3(mask, "mask")
    dev = _device_of(device, mask)
    lib = _capi.load()
    with torch.cuda.device(dev):
        mk = _maps3(torch.as_tensor(mask) != 0, dev, torch.uint8, "mask")
        M, H, W = mk.shape
        nbytes = lib.bn_task_workspace_bytes(M, H, W)
        if nbytes == 0:
            raise ValueError(f"{M} maps of {H} x {W} cells are out of the library's range")
        labels = torch.empty(M, H, W, device=dev, dtype=torch.int32)
        sizes = torch.empty(M, H * W, device=dev, dtype=torch.int32)
        stats = torch.empty(M, STATS, device=dev, dtype=torch.int32)
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)              # torch's allocator keeps it alive for the stream
        _raise(lib, lib.bn_task_label_async(dev.index, stream_ptr(dev), _p(mk), M, H, W, int(connectivity), _p(labels), _p(sizes), _p(stats),
                                            _p(work), nbytes))
        flags = stats[:, 4].cpu().numpy()
    if flags.any():
        m = int(np.nonzero(flags)[0][0])
        raise RuntimeError(f"labelling map {m} reached a loop bound (error flags {int(flags[m])}); {int((flags != 0).sum())} such maps")
    return labels, sizes, stats


def sample_pairs(labels, sizes, pairs: int, seed: int, first_map: int = 0, border: int = 2, min_separation_sq: int = 0,
                 min_component_cells: int = 1, max_attempts: int = 256, origin=(0.0, 0.0), resolution: float = 0.5,
                 device=None) -> Dict[str, torch.Tensor]:
    """{"cells": (M, pairs, 4) int32 (sx, sy, gx, gy), "attempt": (M, pairs) int32, "positions": (M, pairs, 4) float32 cell
    centres} on the device, one launch (bn_task_sample_async; the header states the draw and the acceptance rule).  A pair
    without an accepted attempt below max_attempts is -1 / -1 / NaN.  Pairs are independent draws: two of a map may coincide."""
    M, H, W = _shape3(labels, "labels")
    if torch.as_tensor(sizes).numel() != M * H * W:
        raise ValueError(f"sizes must be ({M}, {H * W}), got {tuple(torch.as_tensor(sizes).shape)}")
    P = int(pairs)
    if P < 1 or P > MAX_PAIRS:
        raise ValueError(f"pairs must be in [1, {MAX_PAIRS}]")
    dev = _device_of(device, labels, sizes)
    lib = _capi.load()
    with torch.cuda.device(dev):
        lb = _maps3(labels, dev, torch.int32, "labels")
        sz = torch.as_tensor(sizes).detach().to(dev, torch.int32).reshape(M, -1).contiguous()
        out = {"cells": torch.empty(M, P, 4, device=dev, dtype=torch.int32), "attempt": torch.empty(M, P, device=dev, dtype=torch.int32),
               "positions": torch.empty(M, P, 4, device=dev, dtype=torch.float32)}
        _raise(lib, lib.bn_task_sample_async(dev.index, stream_ptr(dev), _p(lb), _p(sz), M, H, W, P, int(seed) & ((1 << 64) - 1), int(first_map),
                                             int(border), int(min_separation_sq), int(min_component_cells), int(max_attempts), float(origin[0]),
                                             float(origin[1]), float(resolution), _p(out["cells"]), _p(out["attempt"]), _p(out["positions"])))
    return out


def optimal_lengths(mask, cells, resolution: float, chunk: int = 64, device=None) -> torch.Tensor:
    """(M, P) float32 on the device: the shortest 8-connected grid path length in metres from each pair's start cell to its goal
    cell over the passable cells -- D[start] of the A* field (bn_astar) on zero heights with the mask as the risk and a threshold of
    0.5, one instance per pair, `chunk` pairs per solve.  +inf where the field does not reach the start (another component, or a
    blocked start or goal), NaN for a pair without cells (-1).  mask: (M, H, W); cells: (M, P, 4) int32 (sx, sy, gx, gy)."""
    dev = _device_of(device, mask, cells)
    lib = _capi.load()
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")

    def ok(code):
        if code:
            check(lib, "astar", code)

    with torch.cuda.device(dev):
        risk = _maps3(torch.as_tensor(mask) != 0, dev, torch.float32, "mask")
        M, H, W = risk.shape
        cl = torch.as_tensor(cells).detach().to(dev, torch.int32)
        if cl.dim() != 3 or cl.shape[0] != M or cl.shape[2] != 4:
            raise ValueError(f"cells must be ({M}, P, 4), got {tuple(cl.shape)}")
        P = int(cl.shape[1])
        flat = cl.reshape(M * P, 4).contiguous()
        host = flat.cpu().numpy()
        inside = ((host >= 0).all(axis=1) & (host[:, [0, 2]] < W).all(axis=1) & (host[:, [1, 3]] < H).all(axis=1))
        heights = torch.zeros(H, W, device=dev, dtype=torch.float32)
        out = torch.full((M * P,), float("nan"), device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev)
        handles: Dict[int, C.c_void_p] = {}
        try:
            for n0 in range(0, M * P, chunk):
                B = min(chunk, M * P - n0)
                if B not in handles:
                    h = C.c_void_p()
                    ok(lib.bn_astar_create(dev.index, H, W, B, C.byref(h)))
                    handles[B] = h
                h = handles[B]
                for b in range(B):
                    n = n0 + b
                    ok(lib.bn_astar_set_map(h, b, _p(heights), _p(risk[n // P]), _capi.BN_MEM_DEVICE, 0.5, float(resolution)))
                    gx, gy = (int(host[n, 2]), int(host[n, 3])) if inside[n] else (-1, -1)
                    ok(lib.bn_astar_set_goal(h, b, gx, gy))
                ok(lib.bn_astar_solve_async(h, C.c_void_p(stream.cuda_stream)))
                d, nx = C.c_void_p(), C.c_void_p()
                ok(lib.bn_astar_buffers(h, 0, C.byref(d), C.byref(nx)))
                D = torch.as_tensor(_DevArray(d.value, (B, H * W)), device=dev)
                sel = flat[n0:n0 + B]
                at = (sel[:, 1].clamp(0, H - 1).to(torch.int64) * W + sel[:, 0].clamp(0, W - 1).to(torch.int64)).unsqueeze(1)
                out[n0:n0 + B] = D.gather(1, at)[:, 0]                        # on the solve's stream, behind it
                ok(lib.bn_astar_sync(h))                                      # ... and a failed field solve is an error
                stream.synchronize()                                          # the gather has read D: the next chunk may overwrite it
        finally:
            for h in handles.values():
                lib.bn_astar_destroy(h)
        out = torch.where(torch.as_tensor(inside, device=dev), out, torch.full_like(out, float("nan")))
    return out.reshape(M, P)


# ---- SPL ---------------------------------------------------------------------------------------------------------------------------
def spl_figures(outcome, path_length, optimal_length) -> Tuple[Optional[float], Optional[float]]:
    """(spl, path_ratio_mean) of one setting's episodes.  spl: the mean over the episodes that are not INVALID of
    [outcome == GOAL] * L* / max(L, L*) (1 where both are 0); path_ratio_mean: the mean of L / L* over the GOAL episodes with
    L* > 0.  A mean over nothing is None.  See the module docstring for the two biases of L*."""
    oc = np.asarray(outcome).ravel()
    L, Ls = np.asarray(path_length, np.float64).ravel(), np.asarray(optimal_length, np.float64).ravel()
    valid, goal = oc != INVALID, oc == GOAL
    top = np.maximum(L, Ls)
    with np.errstate(all="ignore"):
        term = np.where(goal, np.where(top > 0.0, Ls / top, 1.0), 0.0)
        ratio = L / Ls
    rated = goal & (Ls > 0.0)
    return (float(np.mean(term[valid])) if valid.any() else None, float(np.mean(ratio[rated])) if rated.any() else None)


# ---- the task set ------------------------------------------------------------------------------------------------------------------
def _listed(a: np.ndarray):
    """Nested lists with None for NaN and "inf" for +inf: strict JSON."""
    def one(v):
        if isinstance(v, list):
            return [one(x) for x in v]
        if isinstance(v, float) and v != v:
            return None
        if isinstance(v, float) and math.isinf(v):
            return "inf" if v > 0 else "-inf"
        return v
    return one(np.asarray(a).tolist())


def _floats(v, dtype) -> np.ndarray:
    def one(x):
        if isinstance(x, list):
            return [one(y) for y in x]
        return float("nan") if x is None else float(x)
    return np.asarray(one(v), dtype)


class TaskSet:
    """Start/goal pairs for every map of a split, `trials` per map, with what they were a function of.

    start, goal (M, trials, 2) float32 positions (cell centres; NaN without a pair); cells (M, trials, 4) int32 (sx, sy, gx, gy),
    -1 without; attempt (M, trials) int32, the accepted draw, -1 without (and for fixed positions); valid (M, trials) bool;
    optimal_length (M, trials) float32, L* in metres (+inf across components, NaN without cells); params: a dict."""

    def __init__(self, start, goal, cells, attempt, valid, optimal_length, params: dict) -> None:
        self.start, self.goal = np.ascontiguousarray(start, np.float32), np.ascontiguousarray(goal, np.float32)
        self.cells, self.attempt = np.ascontiguousarray(cells, np.int32), np.ascontiguousarray(attempt, np.int32)
        self.valid, self.optimal_length = np.ascontiguousarray(valid, bool), np.ascontiguousarray(optimal_length, np.float32)
        self.params = dict(params)
        M, T = self.valid.shape
        for name, shape in (("start", (M, T, 2)), ("goal", (M, T, 2)), ("cells", (M, T, 4)), ("attempt", (M, T)), ("optimal_length", (M, T))):
            if getattr(self, name).shape != shape:
                raise ValueError(f"{name} must be {shape}, got {getattr(self, name).shape}")

    maps = property(lambda self: self.valid.shape[0])
    trials = property(lambda self: self.valid.shape[1])

    # -- JSON --
    def to_dict(self) -> dict:
        return {"params": self.params, "maps": self.maps, "trials": self.trials, "start": _listed(self.start), "goal": _listed(self.goal),
                "cells": self.cells.tolist(), "attempt": self.attempt.tolist(), "valid": self.valid.tolist(),
                "optimal_length": _listed(self.optimal_length)}

    @classmethod
    def from_dict(cls, doc: dict) -> "TaskSet":
        M, T = int(doc["maps"]), int(doc["trials"])
        return cls(_floats(doc["start"], np.float32).reshape(M, T, 2), _floats(doc["goal"], np.float32).reshape(M, T, 2),
                   np.asarray(doc["cells"], np.int32).reshape(M, T, 4), np.asarray(doc["attempt"], np.int32).reshape(M, T),
                   np.asarray(doc["valid"], bool).reshape(M, T), _floats(doc["optimal_length"], np.float32).reshape(M, T), doc["params"])

    def to_json(self, path: str) -> None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=1, allow_nan=False)
            f.write("\n")

    @classmethod
    def from_json(cls, path: str) -> "TaskSet":
        with open(path) as f:
            return cls.from_dict(json.load(f))

    # -- the two ways to make one --
    @staticmethod
    def _mask(dataset, kappa: float, stuck_threshold: float, dev: torch.device) -> torch.Tensor:
        return passable_mask(dataset.latent_mean.to(dev, torch.float32), dataset.latent_std.to(dev, torch.float32), kappa, stuck_threshold,
                             device=dev)

    @classmethod
    def sample(cls, dataset, trials: int, seed: int, min_separation: float = 10.0, connectivity: int = 4, kappa: float = 0.0, border: int = 2,
               min_component_cells: int = 64, max_attempts: int = 256, resolution: float = 0.5, stuck_threshold: float = 0.1,
               chunk: int = 64, mask=None) -> "TaskSet":
        """`trials` pairs per map of `dataset` (a dataset.TerrainDataset), drawn in one connected region of the latent model's
        passable ground: map m of the split is map `first_map` = m of the draw, so a pair is a function of (seed, m, trial) and of
        the map.  min_separation: metres between the two cell centres at least (ceil((min_separation / resolution)^2) in squared
        cells).  mask: a (M, G, G) mask of the caller's own instead of the latent model's.  A pair without an accepted attempt is
        not valid (and INVALID in a campaign)."""
        dev = resolve_device(dataset.device if dataset.device.type == "cuda" else None, "tasks")
        sep_sq = int(math.ceil((float(min_separation) / float(resolution)) ** 2))
        with torch.cuda.device(dev):
            mk = cls._mask(dataset, kappa, stuck_threshold, dev) if mask is None else _maps3(torch.as_tensor(mask) != 0, dev, torch.uint8, "mask")
            labels, sizes, _ = label_components(mk, connectivity, device=dev)
            got = sample_pairs(labels, sizes, int(trials), seed, 0, border, sep_sq, min_component_cells, max_attempts, (0.0, 0.0), resolution,
                               device=dev)
            best = optimal_lengths(mk, got["cells"], resolution, chunk, device=dev)
            cells, attempt, pos, best = (t.cpu().numpy() for t in (got["cells"], got["attempt"], got["positions"], best))
        params = {"kind": "sampled", "seed": int(seed), "trials": int(trials), "min_separation": float(min_separation), "min_separation_sq": sep_sq,
                  "connectivity": int(connectivity), "kappa": float(kappa), "border": int(border), "min_component_cells": int(min_component_cells),
                  "max_attempts": int(max_attempts), "resolution": float(resolution), "stuck_threshold": float(stuck_threshold)}
        return cls(pos[..., :2], pos[..., 2:], cells, attempt, (attempt >= 0) & np.isfinite(best), best, params)

    @classmethod
    def from_positions(cls, dataset, start_pos, goal_pos, trials: int, kappa: float = 0.0, resolution: float = 0.5, stuck_threshold: float = 0.1,
                       chunk: int = 64, mask=None) -> "TaskSet":
        """The same object from fixed positions: start_pos, goal_pos (2,), (M, 2) or (M, trials, 2), kept as given.  Their cells
        are floor(p / resolution) in float32; `valid` is "both cells are on the map, passable and in one 8-connected component"."""
        dev = resolve_device(dataset.device if dataset.device.type == "cuda" else None, "tasks")
        M, T = len(dataset), int(trials)

        def spread(a):
            a = np.asarray(a, np.float32)
            return np.ascontiguousarray(np.broadcast_to(a[:, None, :] if a.ndim == 2 else a, (M, T, 2)))

        start, goal = spread(start_pos), spread(goal_pos)
        res = np.float32(resolution)
        with np.errstate(all="ignore"):
            cells = np.concatenate([np.floor(start / res), np.floor(goal / res)], axis=-1)
        with torch.cuda.device(dev):
            mk = cls._mask(dataset, kappa, stuck_threshold, dev) if mask is None else _maps3(torch.as_tensor(mask) != 0, dev, torch.uint8, "mask")
            H, W = int(mk.shape[1]), int(mk.shape[2])
            inside = (np.isfinite(cells).all(axis=-1) & (cells >= 0).all(axis=-1) & (cells[..., [0, 2]] < W).all(axis=-1)
                      & (cells[..., [1, 3]] < H).all(axis=-1))
            cells = np.where(inside[..., None], np.nan_to_num(cells, nan=-1.0, posinf=-1.0, neginf=-1.0), -1.0).astype(np.int32)
            labels, _, _ = label_components(mk, 8, device=dev)
            lab = labels.cpu().numpy()
            best = optimal_lengths(mk, torch.from_numpy(cells), resolution, chunk, device=dev).cpu().numpy()
        mi = np.arange(M)[:, None]
        safe = np.maximum(cells, 0)
        ls, lg = lab[mi, safe[..., 1], safe[..., 0]], lab[mi, safe[..., 3], safe[..., 2]]
        params = {"kind": "positions", "trials": T, "kappa": float(kappa), "resolution": float(resolution), "stuck_threshold": float(stuck_threshold)}
        return cls(start, goal, cells, np.full((M, T), -1, np.int32), inside & (ls >= 0) & (ls == lg), best, params)
