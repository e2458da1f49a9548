"""MI355X-native closed-loop RRT global planner with the reference's Python interface.

Mirror of `CLRRT(RRT)` in the reference's src/planners/global_planners/sampling_based/cl_rrt.py: every iteration samples a pose,
finds the nearest node, lays a Dubins path to the sample (src/planners/local_planners/dubins.py), follows it in closed loop with
pure pursuit and two PID controllers (pure_pursuit.py) on the unicycle dynamics, and appends the last state as a node where the
follower came within 1 m of the path's end.  The tree is grown on the device (csrc/clrrt_kernels.hip, one wave per planner);
DESIGN.md 4.7 states the arithmetic and the rules taken over from the reference, among them: the goal node's heading is the FIRST
forward()'s for the life of the planner, and a steer from a node other than the root updates that node's stored integrals in
place, feasible or not.

Like `RRT`, this class does not touch torch's, NumPy's or Python's global generators: every planner owns its MT19937 stream on
the device, seeded like the reference's and continued across forward() calls.

    planner = CLRRT(3, 2, dynamics, objectives, grid_map, delta_t=0.1, max_iterations=500, seed=42)
    action_seq, state_seq = planner(state)               # (L, 2), (1, L + 1, 3) or (None, None), as the reference
    actions, states, lengths, found = planner.plan_batch(states, goals, seeds)       # B planners per launch
    ... = planner.plan_batch(states, goals, seeds, risk_maps=maps)                   # ... each on its own (G, G) risk map
    planner = CLRRT.from_parameters(64, 0.5, delta_t=0.1, stuck_threshold=0.1)       # without reference-shaped objects
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _capi
from ._device import _PlannerHandle, _TreePlanner, _check_seed, check, resolve_device, seed_array, stream_ptr, tree_capacity

WORDS = ("LSL", "RSR", "RSL", "LSR", "RLR", "LRL")
_POINTS = 64


class Tree:
    """The reference Tree's public state after forward() (planner_name="cl_rrt"): `nodes` (capacity, 3), `nodes_count`, `edges`
    (capacity,) int64, `costs`, `action_seqs` (capacity, max_seqs, 2), `state_seqs` (capacity, max_seqs + 1, 3), `seq_lengths`
    (capacity,) int64 and `controllers_states` (capacity, 4); zeros (-1, inf) where unset.  The capacity is the reference's: 1000,
    doubled while the tree does not fit."""

    def __init__(self, n: int, nodes, edges, costs, action_seqs, state_seqs, seq_lengths, controllers_states):
        cap = tree_capacity(n)
        dev, S = nodes.device, int(action_seqs.shape[1])
        self.nodes = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
        self.edges = -torch.ones(cap, dtype=torch.int64, device=dev)
        self.costs = torch.full((cap,), torch.inf, dtype=torch.float32, device=dev)
        self.action_seqs = torch.zeros((cap, S, 2), dtype=torch.float32, device=dev)
        self.state_seqs = torch.zeros((cap, S + 1, 3), dtype=torch.float32, device=dev)
        self.seq_lengths = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.controllers_states = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
        self.nodes[:n] = nodes[:n]
        self.edges[:n] = edges[:n].to(torch.int64)
        self.costs[:n] = costs[:n]
        self.action_seqs[:n] = action_seqs[:n]
        self.state_seqs[:n] = state_seqs[:n]
        self.seq_lengths[:n] = seq_lengths[:n].to(torch.int64)
        self.controllers_states[:n] = controllers_states[:n]
        self.nodes_count = n


def _check(lib, code: int):
    check(lib, "clrrt", code)


class _Handle(_PlannerHandle):
    """One bn_clrrt handle: B instances of one parameter set, on the owner's map or (set_maps) on one map each."""
    family = "clrrt"

    def __init__(self, lib, dev: torch.device, B: int, owner: "CLRRT"):
        cfg = _capi.CLRRTConfig()
        lib.bn_clrrt_config_init(C.byref(cfg))
        cfg.device_id, cfg.num_instances, cfg.max_iterations, cfg.max_seqs = dev.index, B, owner._max_iterations, owner._max_seqs
        cfg.path_cap = owner._path_cap
        cfg.grid_size, cfg.resolution = owner._grid_size, owner.resolution
        cfg.x_limits[0], cfg.x_limits[1] = float(owner.x_limits[0]), float(owner.x_limits[1])
        cfg.y_limits[0], cfg.y_limits[1] = float(owner.y_limits[0]), float(owner.y_limits[1])
        cfg.delta_distance, cfg.goal_sample_rate = float(owner._delta_distance), float(owner._goal_sample_rate)
        cfg.goal_threshold, cfg.delta_t = float(owner._goal_threshold), float(owner._delta_t)
        for i in range(2):
            cfg.u_min[i], cfg.u_max[i] = float(owner._u_min[i]), float(owner._u_max[i])
        cfg.seed = owner._seed
        self.iters, self.S = owner._max_iterations, owner._max_seqs
        super().__init__(lib, dev, B, cfg)
        self.path_cap = int(lib.bn_clrrt_path_cap(self.h))
        self.G, self.per_instance = owner._grid_size, False
        self._shared = (owner._risk, np.ascontiguousarray(owner._goal_host.numpy()[:2], np.float32), float(owner._stuck_threshold))
        self._set_shared()

    def _set_shared(self):
        risk, goal, thr = self._shared
        self._check(self._lib.bn_clrrt_set_map(self.h, risk.ctypes.data, goal.ctypes.data, thr))
        self.per_instance = False

    def set_maps(self, risk_maps=None):
        """risk_maps (B, G, G) float32 -- a torch tensor on the host or the device (copied device to device on torch's current
        stream), or a NumPy array -- become the instances' own maps; None returns the handle to the owner's shared map."""
        if risk_maps is None:
            if self.per_instance:
                self._set_shared()
            return
        if isinstance(risk_maps, torch.Tensor) and risk_maps.is_cuda:
            keep = risk_maps.detach().to(self.dev, torch.float32).contiguous()
            where, ptr = _capi.BN_MEM_DEVICE, keep.data_ptr()
        else:
            host = risk_maps.detach().numpy() if isinstance(risk_maps, torch.Tensor) else risk_maps
            keep = np.ascontiguousarray(host, np.float32)
            where, ptr = _capi.BN_MEM_HOST, keep.ctypes.data
        if tuple(keep.shape) != (self.B, self.G, self.G):
            raise ValueError(f"risk_maps must be ({self.B}, {self.G}, {self.G}), got {tuple(keep.shape)}")
        self._check(self._lib.bn_clrrt_set_instance_maps(self.h, stream_ptr(self.dev), C.c_void_p(ptr), where, self._shared[2]))
        self.per_instance = True


class CLRRT(_TreePlanner, nn.Module):
    _handle_type = _Handle

    def __init__(self, dim_state: int, dim_control: int, dynamics, objectives, grid_map, delta_t: float, max_iterations: int = 500,
                 delta_distance: float = 5, goal_sample_rate: float = 0.25, max_seqs: int = 250, goal_threshold: float = 1.0,
                 device: Optional[str] = None, dtype: torch.dtype = torch.float32, seed: int = 42, path_cap: Optional[int] = None) -> None:
        """The reference's constructor (cl_rrt.py:26-136).  `dynamics` and `objectives` are read like MPPI's and DWA's here: the
        risk map, the grid's geometry, the action bounds, the goal and the stuck threshold.  path_cap: the longest action sequence
        forward() can return (default min(max_iterations * max_seqs, 65536)); a longer path raises."""
        super().__init__()
        from .mppi import _planner_inputs
        if dim_state != 3 or dim_control != 2:
            raise ValueError("CLRRT plans for the unicycle model: dim_state=3, dim_control=2")
        if dtype != torch.float32:
            raise ValueError(f"CLRRT runs the float32 dynamics of the device (dtype={dtype}); the reference's default is float32 too")
        assert dynamics.min_action.shape == (dim_control,), "minimum actions must be a tensor of shape (dim_control,)"
        assert dynamics.max_action.shape == (dim_control,), "maximum actions must be a tensor of shape (dim_control,)"
        try:
            inp = _planner_inputs(dynamics, objectives)
        except TypeError as e:
            raise TypeError("CLRRT needs dynamics in 'inference' mode: the device transit reads the predicted risk map, and the "
                            "reference's own CLRRT fails on observation mode's (state, traversability) tuple") from e
        self._dim_state, self._dim_control, self._dtype = dim_state, dim_control, dtype
        self._configure(inp["grid_size"], float(grid_map.resolution), grid_map.x_limits, grid_map.y_limits,
                        dynamics.min_action.detach().to("cpu", torch.float32).tolist(), dynamics.max_action.detach().to("cpu", torch.float32).tolist(),
                        inp["stuck_threshold"], inp["risks"], inp["goal"], delta_t, max_iterations, delta_distance, goal_sample_rate, max_seqs,
                        goal_threshold, device, seed, path_cap)

    @classmethod
    def from_parameters(cls, grid_size: int, resolution: float, x_limits=None, y_limits=None, u_min=(0.0, -1.0), u_max=(1.0, 1.0),
                        stuck_threshold: float = 0.1, delta_t: float = 0.1, max_iterations: int = 500, delta_distance: float = 5,
                        goal_sample_rate: float = 0.25, max_seqs: int = 250, goal_threshold: float = 1.0, risk_map=None, goal=None,
                        device: Optional[str] = None, seed: int = 42, path_cap: Optional[int] = None) -> "CLRRT":
        """A planner from the numbers the constructor reads off `dynamics`, `objectives` and `grid_map`: the grid (x_limits and
        y_limits default to (0, grid_size * resolution)), the action bounds, the stuck threshold and the planner's parameters.
        risk_map: the shared (G, G) map (default zeros: a caller that plans on per-instance maps gives them to plan_batch or
        CLRRTLoop); goal: (2,) the default goal of forward and plan_batch and the goal steer_batch's costs run against (default
        the limits' lower corner)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        G = int(grid_size)
        x_limits = (0.0, G * float(resolution)) if x_limits is None else x_limits
        y_limits = x_limits if y_limits is None else y_limits
        self._dim_state, self._dim_control, self._dtype = 3, 2, torch.float32
        self._configure(G, float(resolution), torch.as_tensor(x_limits, dtype=torch.float32), torch.as_tensor(y_limits, dtype=torch.float32),
                        [float(v) for v in u_min], [float(v) for v in u_max], float(stuck_threshold),
                        torch.zeros(G, G) if risk_map is None else torch.as_tensor(risk_map),
                        torch.tensor([float(x_limits[0]), float(y_limits[0])]) if goal is None else goal, delta_t, max_iterations,
                        delta_distance, goal_sample_rate, max_seqs, goal_threshold, device, seed, path_cap)
        return self

    def _configure(self, grid_size, resolution, x_limits, y_limits, u_min, u_max, stuck_threshold, risks, goal, delta_t, max_iterations,
                   delta_distance, goal_sample_rate, max_seqs, goal_threshold, device, seed, path_cap) -> None:
        self._seed = _check_seed(seed)
        self.resolution = resolution
        self.x_limits, self.y_limits = x_limits, y_limits
        self.device = device if device is not None else "cuda" if torch.cuda.is_available() else "cpu"
        self._max_iterations, self._max_seqs = int(max_iterations), int(max_seqs)
        if self._max_iterations < 1 or self._max_seqs < 1:
            raise ValueError("max_iterations and max_seqs must be >= 1")
        self._delta_distance, self._goal_sample_rate, self._goal_threshold = delta_distance, goal_sample_rate, goal_threshold
        self._delta_t = float(delta_t)
        self._path_cap = 0 if path_cap is None else int(path_cap)
        self._grid_size = grid_size
        self._stuck_threshold = stuck_threshold
        self._risk = np.ascontiguousarray(torch.as_tensor(risks).detach().to("cpu", torch.float32).numpy())
        if self._risk.shape != (self._grid_size, self._grid_size):
            raise ValueError(f"the risk map must be ({self._grid_size}, {self._grid_size}), got {self._risk.shape}")
        self._u_min, self._u_max = u_min, u_max
        self._goal_host = torch.as_tensor(goal).detach().to("cpu", torch.float32)[:2].contiguous()
        self.tree = None
        self._planner_name = "cl_rrt"
        self._start_node = None
        self._dev = resolve_device(self.device, "CLRRT", lenient=True)
        self._goal_node = self._goal_host.clone()                 # grows by one heading per forward(), as the reference's does
        self._lib = _capi.load()
        self._handles = {}
        self._goal_node_indices = []
        self.last_batch = None
        self._last_handle = None

    # ---- the reference's interface ---------------------------------------------------------------------------------------
    def forward(self, state: torch.Tensor):
        start = torch.as_tensor(state).detach().to("cpu", torch.float32)
        if tuple(start.shape) != (3,):
            raise ValueError(f"state must be (3,), got {tuple(start.shape)}")
        self._start_node = start
        theta = torch.atan2(self._goal_node[1] - start[1], self._goal_node[0] - start[0])             # cl_rrt.py:150-154
        self._goal_node = torch.cat((self._goal_node, theta.unsqueeze(0)), dim=0)                   # index 2 stays the first call's
        if not self._is_within_bounds(start) or not self._is_within_bounds(self._goal_node):        # before any launch
            raise ValueError("Start or goal position is out of bounds.")
        h = self._handle(1)
        h.set_maps(None)
        seeds = None if h.used else np.array([self._seed], np.uint64)
        self._launch(h, start.numpy()[None], self._goal_node[:3].numpy()[None], seeds)
        res = h.buffer(_capi.BN_CLRRT_BUF_RESULTS, (1, 6), "<i4").cpu().numpy()[0]
        self.tree = self._tree(h, 0, int(res[5]))
        self._near_goal_count = int(res[3])
        self._goal_node_indices = [int(res[1])] if res[0] else []     # the pick only: the reference sorts every near-goal node here
        if not res[0]:
            return None, None
        self._raise_unless_path(res)
        L = int(res[2])
        actions = h.buffer(_capi.BN_CLRRT_BUF_PATH_ACTIONS, (1, h.path_cap, 2))[0, :L].clone()
        states = h.buffer(_capi.BN_CLRRT_BUF_PATH_STATES, (1, h.path_cap + 1, 3))[:, :L + 1].clone()
        return actions.to(self.device), states.to(self.device)

    @staticmethod
    def _raise_unless_path(res):
        if res[4] != 0:
            raise RuntimeError(f"the path has {int(res[2])} actions and does not fit the path buffer: construct CLRRT with a larger path_cap")
        if res[1] == 0:
            # the reference fails here too (torch.cat of an empty list): the start lies within the goal threshold
            raise RuntimeError("the start node is the cheapest node within the goal threshold: there is no sequence to return")

    # ---- B planners per launch -------------------------------------------------------------------------------------------
    def _batch_inputs(self, states, goals):
        states = torch.as_tensor(states).detach().to("cpu", torch.float32)
        if states.dim() != 2 or states.shape[1] != 3:
            raise ValueError(f"states must be (B, 3), got {tuple(states.shape)}")
        B = int(states.shape[0])
        g = self._goal_host[None].expand(B, 2) if goals is None else torch.as_tensor(goals).detach().to("cpu", torch.float32)
        if g.dim() != 2 or g.shape[0] != B or g.shape[1] not in (2, 3):
            raise ValueError(f"goals must be (B, 2) or (B, 3), got {tuple(g.shape)}")
        if g.shape[1] == 2:                    # a fresh planner's first forward(): the heading from the start to the goal
            g = torch.cat((g, torch.atan2(g[:, 1] - states[:, 1], g[:, 0] - states[:, 0])[:, None]), dim=1)
        for b in range(B):
            if not self._is_within_bounds(states[b]) or not self._is_within_bounds(g[b]):
                raise ValueError("Start or goal position is out of bounds.")
        return B, np.ascontiguousarray(states.numpy()), np.ascontiguousarray(g.numpy())

    def plan_batch(self, states, goals=None, seeds=None, risk_maps=None):
        """forward() of B planners that share this one's map and parameters, in one launch.  states: (B, 3); goals: (B, 2) -- the
        goal heading is then each instance's own atan2(goal - start), a fresh planner's -- or (B, 3) goal nodes, default this
        planner's goal; seeds: B integers in 0 ... 2^32 - 1, each reseeding its planner's stream as constructing it does; None
        continues the B streams of the last plan_batch of this batch size.  The costs of instance b run against ITS goal.
        risk_maps: (B, G, G) float32, a torch tensor on the host or the device or a NumPy array: instance b plans on map b, as a
        planner constructed on that map does; None plans on this planner's map, also after a call with maps.
        Returns (actions (B, Lmax, 2), states (B, Lmax + 1, 3), lengths (B,) int32, found (B,) bool) on the device, NaN beyond a
        path; `batch_tree(b)` and `last_batch` hold the rest."""
        B, sn, gn = self._batch_inputs(states, goals)
        sd = None if seeds is None else seed_array(seeds, B)
        h = self._handle(B)
        h.set_maps(risk_maps)
        if sd is None and not h.used:
            sd = np.full(B, self._seed, np.uint64)
        self._launch(h, sn, gn, sd)
        return self._batch_result(h)

    def grow_from_samples(self, states, samples, goals=None, risk_maps=None):
        """plan_batch on the caller's samples in place of the stream's: samples (B, max_iterations, 3) float32, host or device."""
        B, sn, gn = self._batch_inputs(states, goals)
        samples = torch.as_tensor(samples).detach().to(torch.float32).contiguous()
        if tuple(samples.shape) != (B, self._max_iterations, 3):
            raise ValueError(f"samples must be ({B}, {self._max_iterations}, 3), got {tuple(samples.shape)}")
        h = self._handle(B)
        h.set_maps(risk_maps)
        self._grow(h, sn, gn, samples)
        return self._batch_result(h)

    def steer_batch(self, from_states, controller_states, targets, risk_maps=None):
        """One _steer per instance with no tree: from_states (B, 3), controller_states (B, 4) (previous error and integral of the
        linear, then the angular controller), targets (B, 3).  The costs run against this planner's goal; risk_maps as plan_batch's.  Returns a dict of
        device tensors: `path` (B, 64, 2) float64 truncated reference paths (NaN beyond), `points` (B,), `word` (B,) index into
        WORDS, `targets` (B, max_seqs) target index per step, `actions` (B, max_seqs, 2), `states` (B, max_seqs + 1, 3),
        `feasible`, `length`, `cost`, `controllers` (B, 4) float64."""
        f = np.ascontiguousarray(torch.as_tensor(from_states).detach().to("cpu", torch.float32).numpy())
        c = np.ascontiguousarray(torch.as_tensor(controller_states).detach().to("cpu", torch.float32).numpy())
        t = np.ascontiguousarray(torch.as_tensor(targets).detach().to("cpu", torch.float32).numpy())
        B = f.shape[0]
        if f.shape != (B, 3) or c.shape != (B, 4) or t.shape != (B, 3):
            raise ValueError("from_states (B, 3), controller_states (B, 4), targets (B, 3)")
        h = self._handle(B)
        h.set_maps(risk_maps)
        _check(self._lib, self._lib.bn_clrrt_steer_async(h.h, self._stream(), f.ctypes.data, c.ctypes.data, t.ctypes.data))
        torch.cuda.current_stream(self._dev).synchronize()
        res = h.buffer(_capi.BN_CLRRT_BUF_STEER_RESULTS, (B, 4), "<i4").clone()
        return {"path": h.buffer(_capi.BN_CLRRT_BUF_STEER_PATHS, (B, _POINTS, 2), "<f8").clone(), "points": res[:, 3], "word": res[:, 2],
                "targets": h.buffer(_capi.BN_CLRRT_BUF_STEER_TARGETS, (B, h.S), "<i4").clone(),
                "actions": h.buffer(_capi.BN_CLRRT_BUF_STEER_ACTIONS, (B, h.S, 2)).clone(),
                "states": h.buffer(_capi.BN_CLRRT_BUF_STEER_STATES, (B, h.S + 1, 3)).clone(), "feasible": res[:, 0] != 0, "length": res[:, 1],
                "cost": h.buffer(_capi.BN_CLRRT_BUF_STEER_COSTS, (B,)).clone(),
                "controllers": h.buffer(_capi.BN_CLRRT_BUF_STEER_CONTROLLERS, (B, 4), "<f8").clone()}

    def batch_tree(self, b: int) -> Tree:
        """Instance b's tree of the last plan_batch / grow_from_samples."""
        if self._last_handle is None:
            raise RuntimeError("no batch has been planned")
        h = self._last_handle
        n = int(h.buffer(_capi.BN_CLRRT_BUF_COUNTS, (h.B,), "<i4")[int(b)].item())
        return self._tree(h, int(b), n)

    def sample_table(self):
        """The samples of the last plan: (samples (B, max_iterations, 3) float32, is_goal (B, max_iterations) bool)."""
        h = self._last_handle
        xy = h.buffer(_capi.BN_CLRRT_BUF_SAMPLES, (h.B, h.iters, 3)).clone()
        fl = h.buffer(_capi.BN_CLRRT_BUF_SAMPLE_FLAGS, (h.B, h.iters), "<i4").clone()
        return xy, fl != 0

    def iteration_log(self):
        """What every iteration of the last plan did: (nearest (B, max_iterations) int32 node indices, feasible (B, max_iterations)
        bool), device tensors."""
        h = self._last_handle
        return (h.buffer(_capi.BN_CLRRT_BUF_NEAREST, (h.B, h.iters), "<i4").clone(),
                h.buffer(_capi.BN_CLRRT_BUF_FEASIBLE, (h.B, h.iters), "<i4").clone() != 0)

    # ---- plumbing --------------------------------------------------------------------------------------------------------
    def _tree(self, h: _Handle, b: int, n: int) -> Tree:
        c = h.iters + 1
        return Tree(n, h.buffer(_capi.BN_CLRRT_BUF_NODES, (h.B, c, 3))[b], h.buffer(_capi.BN_CLRRT_BUF_EDGES, (h.B, c), "<i4")[b],
                    h.buffer(_capi.BN_CLRRT_BUF_COSTS, (h.B, c))[b], h.buffer(_capi.BN_CLRRT_BUF_ACTION_SEQS, (h.B, c, h.S, 2))[b],
                    h.buffer(_capi.BN_CLRRT_BUF_STATE_SEQS, (h.B, c, h.S + 1, 3))[b],
                    h.buffer(_capi.BN_CLRRT_BUF_SEQ_LENGTHS, (h.B, c), "<i4")[b], h.buffer(_capi.BN_CLRRT_BUF_CONTROLLERS, (h.B, c, 4))[b])

    def _batch_result(self, h: _Handle):
        self._last_handle = h
        res = h.buffer(_capi.BN_CLRRT_BUF_RESULTS, (h.B, 6), "<i4").clone()
        host = res.cpu().numpy()
        for b in range(h.B):
            if host[b, 0] and host[b, 4] != 0:
                self._raise_unless_path(host[b])
        found = (res[:, 0] != 0) & (res[:, 1] > 0)
        lengths = torch.where(found, res[:, 2], torch.zeros_like(res[:, 2])).contiguous()
        lmax = max(int(lengths.max().item()), 1)
        actions = h.buffer(_capi.BN_CLRRT_BUF_PATH_ACTIONS, (h.B, h.path_cap, 2))[:, :lmax].clone()
        states = h.buffer(_capi.BN_CLRRT_BUF_PATH_STATES, (h.B, h.path_cap + 1, 3))[:, :lmax + 1].clone()
        self.last_batch = {"near_goal_counts": res[:, 3].clone(), "picks": res[:, 1].clone(), "node_counts": res[:, 5].clone(),
                           "nearest": h.buffer(_capi.BN_CLRRT_BUF_NEAREST, (h.B, h.iters), "<i4").clone(),
                           "feasible": h.buffer(_capi.BN_CLRRT_BUF_FEASIBLE, (h.B, h.iters), "<i4").clone() != 0}
        return actions, states, lengths, found
