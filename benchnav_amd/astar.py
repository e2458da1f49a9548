"""MI355X-native A* global planner with the reference's Python interface.

Mirror of `AStar(nn.Module)` in the reference's src/planners/global_planners/search_based/astar.py (constructor :33-71,
forward :73-122).  The reference searches from the new start on every forward() call; the goal and the maps are fixed at
construction and the edge weight is symmetric, so here the constructor enqueues ONE goal-rooted shortest-path solve on the
GPU (csrc/astar_kernels.hip: the cost-to-go field and a one-byte next-hop map, copied to pinned host memory), and forward()
walks the next-hop map on the host from the start cell: O(path length), no GPU round trip.  build_jump_tables() adds
pointer-doubling tables over that map on the device: hop_counts() (reachability and path length of every cell) and paths()
(forward() for many starts at once, the result staying on the device).

It returns A shortest path (first minimiser in the reference's direction order among equal-cost hops); the reference returns
one too where its search is exact, and otherwise a costlier one ("AStar").
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _capi
from ._device import Handle, _DevArray, resolve_device, stream_ptr  # noqa: F401  (tests import _DevArray from here)


class AStar(Handle, nn.Module):
    family = "astar"

    def __init__(self, grid_map, goal_pos: torch.Tensor, dynamics, stuck_threshold: float, device: Optional[str] = None) -> None:
        super().__init__()
        heights = grid_map.tensors["heights"].detach()                            # astar.py:53-58
        risks = dynamics._traversability_model._risks.detach()
        self.resolution = grid_map.resolution
        self.x_limits = grid_map.x_limits
        self.y_limits = grid_map.y_limits
        self._stuck_threshold = stuck_threshold
        self.device = device if device is not None else "cuda" if torch.cuda.is_available() else "cpu"
        assert risks.shape == heights.shape, "Traversability and height maps must have the same shape."
        self._h, self._w = heights.shape
        self._goal_node = self._pos_to_index(goal_pos)                             # astar.py:71
        self.dev = self._dev = resolve_device(self.device, "AStar", lenient=True)
        heights = heights.to(torch.float32).contiguous()
        risks = risks.to(torch.float32).contiguous()
        # the goal checks of forward() (astar.py:88-94), decided once: the goal never changes
        gx, gy = self._goal_node
        self._goal_in_bounds = self._is_within_bounds(self._goal_node)
        self._goal_collision = self._goal_in_bounds and bool(risks[gy, gx].item() <= np.float32(stuck_threshold))
        self._lib = _capi.load()
        h = C.c_void_p()
        self._check(self._lib.bn_astar_create(self._dev.index, self._h, self._w, 1, C.byref(h)))
        self._handle = h
        on_dev = heights.is_cuda and risks.is_cuda and heights.device == self._dev and risks.device == self._dev
        if on_dev:
            where, hp, rp = _capi.BN_MEM_DEVICE, heights.data_ptr(), risks.data_ptr()
        else:
            hn, rn = heights.cpu().numpy(), risks.cpu().numpy()      # alive until set_map returns (it copies synchronously)
            where, hp, rp = _capi.BN_MEM_HOST, hn.ctypes.data, rn.ctypes.data
        self._check(self._lib.bn_astar_set_map(self._handle, 0, hp, rp, where, float(stuck_threshold), float(self.resolution)))
        self._check(self._lib.bn_astar_set_goal(self._handle, 0, gx, gy))
        self._check(self._lib.bn_astar_solve_async(self._handle, stream_ptr(self._dev)))
        self._buf = np.empty((self._h * self._w, 2), np.int32)
        self._jump_built = False                                                   # the tables come with the first use

    def forward(self, state: torch.Tensor) -> Optional[torch.Tensor]:
        state = state[:2] if state.shape[0] == 3 else state                        # astar.py:84
        if state.is_cuda:
            state = state.detach().cpu()                                           # one read; the index arithmetic below is IEEE f32
        start_node = self._pos_to_index(state)
        if not self._is_within_bounds(start_node) or not self._goal_in_bounds:     # astar.py:88-92
            raise ValueError("Start or goal position is out of bounds.")
        if self._goal_collision:                                                   # astar.py:93-94
            raise ValueError("Goal position is not traversable.")
        n = self._lib.bn_astar_path(self._handle, 0, start_node[0], start_node[1],
                                    self._buf.ctypes.data_as(C.POINTER(C.c_int32)), self._buf.shape[0])
        if n < 0:
            self._check(n)
        if n == 0:
            return None                                                            # astar.py:122
        nodes = torch.from_numpy(self._buf[:n].astype(np.int64))
        return nodes.to(self.device) * self.resolution                             # _reconstruct_path, astar.py:213

    def field(self):
        """(D, next) of the solve as device tensors: D (H, W) float32, +inf where the goal is not reached and on collision
        cells; next (H, W) uint8, a direction index of astar.py:154-163, 8 at the goal, 255 where the goal is unreachable."""
        self._check(self._lib.bn_astar_sync(self._handle))
        d, nx = C.c_void_p(), C.c_void_p()
        self._check(self._lib.bn_astar_buffers(self._handle, 0, C.byref(d), C.byref(nx)))
        D = self.view(d.value, (self._h, self._w)).clone()
        n = self.view(nx.value, (self._h, self._w), "|u1").clone()
        return D, n

    # ---- jump tables (csrc/astar_kernels.hip): hop counts and batched paths that stay on the device --------------------------
    def _stream(self):
        return stream_ptr(self._dev)

    def build_jump_tables(self) -> None:
        """Build the pointer-doubling tables behind the solve (bn_astar_jump_build_async) on the current stream: hops to the
        goal for every cell and the cell 2^k hops on, max(1, ceil(log2(H W))) levels.  hop_counts() and paths()
        call it on first use."""
        self._check(self._lib.bn_astar_jump_build_async(self._handle, self._stream()))
        self._jump_built = True

    def _tables(self):
        if not self._jump_built:
            self.build_jump_tables()

    def hop_counts(self) -> torch.Tensor:
        """(H, W) int32 device tensor: hops from every cell to the goal along the next-hop map, 0 at the goal, -1 where the goal
        is unreachable (everywhere for a goal out of bounds or in collision).  The path from a cell has hops + 1 nodes."""
        self._tables()
        self._check(self._lib.bn_astar_sync(self._handle))
        hp, jp, lv, eb = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        self._check(self._lib.bn_astar_jump_buffers(self._handle, 0, C.byref(hp), C.byref(jp), C.byref(lv), C.byref(eb)))
        return self.view(hp.value, (self._h, self._w), "<i4").clone()

    def paths(self, states: torch.Tensor, max_len: Optional[int] = None):
        """forward() for N starts at once, on the device.  states: (N, 2) or (N, 3) positions, host or device.  Returns
        (points, lengths): points (N, max_len, 2), points[i, :lengths[i]] == forward(states[i]) (the same node * resolution
        arithmetic and dtype), NaN beyond; lengths (N,) int32, 0 where forward() returns None.  A path longer than max_len is
        truncated and lengths keeps the full count; max_len=None sizes the output from the largest length (one small read-back).
        Raises as forward() does for the goal, and for a start out of bounds (naming the first such row)."""
        states = torch.as_tensor(states)
        if states.dim() != 2 or states.shape[1] not in (2, 3):
            raise ValueError(f"states must be (N, 2) or (N, 3), got {tuple(states.shape)}")
        n = int(states.shape[0])
        pos = states.detach()[:, :2]
        # _pos_to_index (astar.py:215-228) per row, in the caller's dtype as forward() does it: the quotient, truncated toward zero
        qx = ((pos[:, 0] - self.x_limits[0]) / self.resolution).trunc()
        qy = ((pos[:, 1] - self.y_limits[0]) / self.resolution).trunc()
        inb = (qx >= 0) & (qx < self._w) & (qy >= 0) & (qy < self._h)
        if not self._goal_in_bounds or not bool(inb.all()):                        # astar.py:88-92
            row = "" if bool(inb.all()) else f" (states[{int(torch.nonzero(~inb)[0, 0])}])"
            raise ValueError("Start or goal position is out of bounds." + row)
        if self._goal_collision:                                                   # astar.py:93-94
            raise ValueError("Goal position is not traversable.")
        self._tables()
        starts = torch.stack([qx, qy], dim=1).to(torch.int32).to(self._dev).contiguous()
        lengths = torch.empty(n, dtype=torch.int32, device=self._dev)

        def run(cap, out):
            self._check(self._lib.bn_astar_paths_async(self._handle, 0, C.c_void_p(starts.data_ptr()), _capi.BN_MEM_DEVICE, n, cap,
                                                       C.c_void_p(None if out is None else out.data_ptr()),
                                                       C.c_void_p(lengths.data_ptr()), self._stream()))
        if max_len is None:
            run(0, None)
            max_len = int(lengths.max()) if n else 0
        cap = int(max_len)
        if cap < 0:
            raise ValueError("max_len must be >= 0")
        nodes = torch.empty((n, cap, 2), dtype=torch.int32, device=self._dev)
        run(cap, nodes)
        points = nodes.to(torch.int64).to(self.device) * self.resolution           # _reconstruct_path, astar.py:213
        return torch.where(nodes.to(self.device) < 0, float("nan"), points), lengths

    def _pos_to_index(self, pos: torch.Tensor) -> tuple[int, int]:               # astar.py:215-228
        return (
            int((pos[0] - self.x_limits[0]) / self.resolution),
            int((pos[1] - self.y_limits[0]) / self.resolution),
        )

    def _is_within_bounds(self, node: tuple[int, int]) -> bool:                   # astar.py:169-180
        return 0 <= node[0] < self._w and 0 <= node[1] < self._h

