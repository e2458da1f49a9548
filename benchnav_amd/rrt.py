"""MI355X-native RRT global planner with the reference's Python interface.

Mirror of `RRT(nn.Module)` and `Tree` in the reference's src/planners/global_planners/sampling_based/{rrt,tree}.py: the base
class its closed-loop RRT inherits -- sampling, nearest neighbour, tree storage, goal test, path reconstruction.  The tree is
grown on the device (csrc/rrt_kernels.hip, one workgroup per planner) and equals the reference's CPU run bit for bit: nodes,
edges, costs and the returned path (DESIGN.md 4.6 states the arithmetic and the one rule the reference leaves open, which of
several equal-cost near-goal nodes ends the path: here the lowest index).

The reference seeds torch's GLOBAL generator in its constructor (set_randomness) and draws from it in forward().  This class
does NOT touch torch's, NumPy's or Python's global generators: every planner owns its MT19937 stream on the device, seeded
like the reference's (the low 32 bits of `seed`) and continued across forward() calls as the reference's is.  Code that relied
on RRT(...) reseeding the global generators as a side effect has to call its own seeding.

    planner = RRT(grid_map, goal_pos, max_iterations=1000, seed=42)
    path = planner(state)                      # (L, 2) or None, as the reference
    paths, lengths, found = planner.plan_batch(states, goals, seeds)     # B planners per launch
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _capi
from ._device import _DevArray, _PlannerHandle, _TreePlanner, _check_seed, check, resolve_device, seed_array, tree_capacity  # noqa: F401


class Tree:
    """The reference Tree's public state after forward(): `nodes` (capacity, 2) float32 (zeros where unset), `nodes_count`,
    `edges` (capacity,) int64 (-1 where unset, and at the root), `costs` (capacity,) float32 (inf where unset).  The capacity
    is the reference's: 1000, doubled while the tree does not fit."""

    def __init__(self, nodes: torch.Tensor, edges: torch.Tensor, costs: torch.Tensor):
        n = int(nodes.shape[0])
        cap = tree_capacity(n)
        dev = nodes.device
        self.nodes = torch.zeros((cap, 2), dtype=torch.float32, device=dev)
        self.edges = -torch.ones(cap, dtype=torch.int64, device=dev)
        self.costs = torch.full((cap,), torch.inf, dtype=torch.float32, device=dev)
        self.nodes[:n] = nodes
        self.edges[:n] = edges.to(torch.int64)
        self.costs[:n] = costs
        self.nodes_count = n


class _Handle(_PlannerHandle):
    """One bn_rrt handle: B instances of one parameter set."""
    family = "rrt"

    def __init__(self, lib, dev: torch.device, B: int, owner: "RRT"):
        cfg = _capi.RRTConfig()
        lib.bn_rrt_config_init(C.byref(cfg))
        cfg.device_id, cfg.num_instances, cfg.max_iterations, cfg.flags = dev.index, B, owner._max_iterations, owner._flags
        cfg.x_limits[0], cfg.x_limits[1] = float(owner.x_limits[0]), float(owner.x_limits[1])
        cfg.y_limits[0], cfg.y_limits[1] = float(owner.y_limits[0]), float(owner.y_limits[1])
        cfg.delta_distance, cfg.goal_sample_rate = float(owner._delta_distance), float(owner._goal_sample_rate)
        cfg.seed = owner._seed
        self.iters = owner._max_iterations
        super().__init__(lib, dev, B, cfg)


def _check(lib, code: int):
    check(lib, "rrt", code)


class RRT(_TreePlanner, nn.Module):
    _handle_type = _Handle

    def __init__(self, grid_map, goal_pos: torch.Tensor, max_iterations: int = 1000, delta_distance: float = 5,
                 goal_sample_rate: float = 0.1, dim_state: int = 2, device: Optional[str] = None, seed: int = 42,
                 node_storage: Optional[str] = None, workgroup: Optional[int] = None) -> None:
        """The reference's constructor (rrt.py:30-79).  `node_storage="global"` keeps the nodes in global memory at any size
        (the path taken above 8191 iterations); `workgroup` = 64 or 256 picks the growth kernel's width (default: the
        library's)."""
        super().__init__()
        # the reference's plain RRT does not run with dim_state == 3 (its 3-vector sample meets 2-vector nodes)
        assert dim_state == 2, "RRT plans in (x, y): dim_state must be 2"
        self._seed = _check_seed(seed)
        self.resolution = grid_map.resolution
        self.x_limits = grid_map.x_limits
        self.y_limits = grid_map.y_limits
        self.device = device if device is not None else "cuda" if torch.cuda.is_available() else "cpu"
        self._max_iterations = int(max_iterations)
        if self._max_iterations < 1:
            raise ValueError("max_iterations must be >= 1")
        self._delta_distance = delta_distance
        self._goal_sample_rate = goal_sample_rate
        self._dim_state = dim_state
        self.tree = None
        self._planner_name = "rrt"
        if node_storage not in (None, "lds", "global") or workgroup not in (None, 64, 256):
            raise ValueError("node_storage is None, 'lds' or 'global'; workgroup is None, 64 or 256")
        self._flags = (_capi.BN_RRT_FLAG_GLOBAL_NODES if node_storage == "global" else 0) | \
            {None: 0, 64: _capi.BN_RRT_FLAG_ONE_WAVE, 256: _capi.BN_RRT_FLAG_FOUR_WAVES}[workgroup]
        self._goal_host = goal_pos.detach().to("cpu", torch.float32)[:2].contiguous()
        self._dev = resolve_device(self.device, "RRT", lenient=True)
        self._goal_node = self._goal_host.to(self.device)
        self._lib = _capi.load()
        self._handles = {}                   # B -> _Handle: forward() is the B = 1 handle, whose stream continues across calls
        self._goal_node_indices = []
        self.last_batch = None

    # ---- the reference's interface ---------------------------------------------------------------------------------------
    def forward(self, state: torch.Tensor) -> Optional[torch.Tensor]:
        start = state[:2] if state.shape[0] == 3 else state
        start = start.detach().to("cpu", torch.float32)
        if not self._is_within_bounds(start) or not self._is_within_bounds(self._goal_host):        # rrt.py:94-97, before any launch
            raise ValueError("Start or goal position is out of bounds.")
        h = self._handle(1)
        self._launch(h, start.numpy()[None], self._goal_host.numpy()[None], None if h.used else np.array([self._seed], np.uint64))
        res = h.buffer(_capi.BN_RRT_BUF_RESULTS, (1, 4), "<i4").cpu().numpy()[0]
        self.tree = self._tree(h, 0)
        self._near_goal_count = int(res[3])
        self._goal_node_indices = [int(res[1])] if res[0] else []     # the pick only: the reference sorts every near-goal node here
        if not res[0]:
            return None
        path = h.buffer(_capi.BN_RRT_BUF_PATHS, (1, h.iters + 1, 2))[0, :int(res[2])].clone()
        return path.to(self.device)

    # ---- B planners per launch -------------------------------------------------------------------------------------------
    def plan_batch(self, states, goals=None, seeds=None):
        """forward() of B planners that share this one's limits and parameters, in one launch.  states: (B, 2) or (B, 3);
        goals: (B, 2), default this planner's goal for all; seeds: B integers in 0 ... 2^32 - 1, each reseeding its planner's
        stream as constructing it does.  seeds=None continues the B streams of the last plan_batch of this batch size (the
        first such call starts them all from the constructor's seed).  Returns (paths, lengths, found) on the device: paths
        (B, Lmax, 2) float32 with NaN beyond a path, lengths (B,) int32 (0 where no path), found (B,) bool.  The trees are
        `batch_tree(b)`, and `last_batch` holds the near-goal counts and the picked node indices."""
        states = torch.as_tensor(states).detach().to("cpu", torch.float32)
        if states.dim() != 2 or states.shape[1] not in (2, 3):
            raise ValueError(f"states must be (B, 2) or (B, 3), got {tuple(states.shape)}")
        B = int(states.shape[0])
        starts = states[:, :2].contiguous()
        g = self._goal_host[None].expand(B, 2) if goals is None else torch.as_tensor(goals).detach().to("cpu", torch.float32)[:, :2]
        g = g.contiguous()
        if tuple(g.shape) != (B, 2):
            raise ValueError(f"goals must be (B, 2), got {tuple(g.shape)}")
        for b in range(B):
            if not self._is_within_bounds(starts[b]) or not self._is_within_bounds(g[b]):
                raise ValueError("Start or goal position is out of bounds.")
        sd = None if seeds is None else seed_array(seeds, B)
        h = self._handle(B)
        self._launch(h, starts.numpy(), g.numpy(), sd)
        return self._batch_result(h)

    def grow_from_samples(self, states, samples, goals=None):
        """plan_batch on the caller's samples in place of the stream's: samples (B, max_iterations, 2) float32, host or
        device; iteration i of instance b steers towards samples[b, i].  The planners' streams are left where they are."""
        states = torch.as_tensor(states).detach().to("cpu", torch.float32)
        B = int(states.shape[0])
        starts = states[:, :2].contiguous()
        g = (self._goal_host[None].expand(B, 2) if goals is None else torch.as_tensor(goals).detach().to("cpu", torch.float32)[:, :2]).contiguous()
        for b in range(B):
            if not self._is_within_bounds(starts[b]) or not self._is_within_bounds(g[b]):
                raise ValueError("Start or goal position is out of bounds.")
        samples = torch.as_tensor(samples).detach().to(torch.float32).contiguous()
        if tuple(samples.shape) != (B, self._max_iterations, 2):
            raise ValueError(f"samples must be ({B}, {self._max_iterations}, 2), got {tuple(samples.shape)}")
        h = self._handle(B)
        self._grow(h, starts.numpy(), g.numpy(), samples)
        return self._batch_result(h)

    def batch_tree(self, b: int) -> Tree:
        """Instance b's tree of the last plan_batch / grow_from_samples."""
        if self._last_handle is None:
            raise RuntimeError("no batch has been planned")
        return self._tree(self._last_handle, int(b))

    def sample_table(self):
        """The samples of the last plan (forward or plan_batch): (xy (B, max_iterations, 2) float32, is_goal (B,
        max_iterations) bool), device tensors."""
        h = self._last_handle
        xy = h.buffer(_capi.BN_RRT_BUF_SAMPLES, (h.B, h.iters, 2)).clone()
        fl = h.buffer(_capi.BN_RRT_BUF_SAMPLE_FLAGS, (h.B, h.iters), "<i4").clone()
        return xy, fl != 0

    def node_storage(self, B: int = 1) -> str:
        return {0: "global", 1: "lds", 2: "lds+costs"}[int(self._lib.bn_rrt_node_storage(self._handle(B).h))]

    # ---- plumbing --------------------------------------------------------------------------------------------------------
    def _tree(self, h: _Handle, b: int) -> Tree:
        n = h.iters + 1
        return Tree(h.buffer(_capi.BN_RRT_BUF_NODES, (h.B, n, 2))[b], h.buffer(_capi.BN_RRT_BUF_EDGES, (h.B, n), "<i4")[b],
                    h.buffer(_capi.BN_RRT_BUF_COSTS, (h.B, n))[b])

    def _batch_result(self, h: _Handle):
        self._last_handle = h
        res = h.buffer(_capi.BN_RRT_BUF_RESULTS, (h.B, 4), "<i4").clone()
        lengths, found = res[:, 2].contiguous(), res[:, 0] != 0
        lmax = max(int(lengths.max().item()), 1)
        paths = h.buffer(_capi.BN_RRT_BUF_PATHS, (h.B, h.iters + 1, 2))[:, :lmax].clone()
        self.last_batch = {"near_goal_counts": res[:, 3].clone(), "picks": res[:, 1].clone()}
        return paths, lengths, found
