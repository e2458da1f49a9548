"""The reference's A* + DWA driver loop (test/test_astar_dwa.py:179-211) on the device, for the B environments of a
`BatchedPlanetaryEnv`.

Every control step of every instance runs inside one kernel (csrc/astar_dwa.hip, bn_astar_dwa_episode_async): the A* path from
the rover's current cell -- a walk of the goal-rooted next-hop map that ONE A* solve per (map, goal) produced (AStar.forward,
astar.py:73-122) -- DWA.forward (dwa.py:116-153) and PlanetaryEnv.step (planetary_env.py:189-219).  Nothing returns to the host
between steps.

    env = BatchedPlanetaryEnv(planner, latent_mean, latent_std, start_pos, goal_pos)
    loop = AStarDWALoop(env, heights, risks, stuck_threshold=env.stuck_threshold, a_lim=(0.5, 0.5), delta_t=0.1)
    env.reset(seed=0)                                  # also resets the loop
    states, rewards, actions, sub_goals, done_step, status = loop.run(1000)
    loop.raise_for_status()                            # the reference's ValueError, for the first instance that raised

Semantics the reference loop fixes ("A* + DWA loop"):
- the start cell is int((x - x_limits[0]) / res) in float32, truncated; a start at x = x_limits[1] (where the environment clamps)
  indexes to G and is out of bounds: the instance stops there with status BN_AD_OUT_OF_BOUNDS, as the reference raises;
- an unreachable start is the reference's None and DWA keeps its previous path; without one the stage cost runs against the goal.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _capi
from ._device import Handle, stream_ptr
from ._episodes import EpisodeLoop

_MESSAGES = {
    _capi.BN_AD_OUT_OF_BOUNDS: "Start or goal position is out of bounds.",       # astar.py:88-92
    _capi.BN_AD_GOAL_COLLISION: "Goal position is not traversable.",             # astar.py:93-94
}


def _per_instance(a, B: int, G: int, what: str) -> np.ndarray:
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float32)
    if a.shape == (G, G):
        a = np.broadcast_to(a, (B, G, G))
    if a.shape != (B, G, G):
        raise ValueError(f"{what} must be (G, G) or (B, G, G) = {(B, G, G)}, got {a.shape}")
    return np.ascontiguousarray(a)


class AStarDWALoop(Handle, EpisodeLoop):       # (Handle first: its close() and `with` are the loop's)
    family = "astar"                         # the handle the loop owns; the planner's (`_h`) is the environment's
    _astar = property(lambda self: self._handle)
    _noun, _buffers_fn = "steps", "bn_astar_dwa_episode_buffers"

    def __init__(self, env, heights, risks, stuck_threshold: float, a_lim, delta_t: float, num_lin_vel: int = 10,
                 num_ang_vel: int = 10, lookahead_distance: float = 1.0, walk: str = "serial"):
        """env: a BatchedPlanetaryEnv; its planner (NativeMPPI, horizon = DWA's horizon) rolls out the candidates on `risks` and
        its goals are the A* goals.  heights, risks: (G, G) or (B, G, G).  a_lim: DWA's acceleration limits (2,); delta_t: DWA's
        time step for the window (dwa.py:168-199).  walk: how the kernel reads the A* path -- "serial": one lane walks the next-hop
        map node by node; "jump": every lane fetches its own node through the A* handle's jump tables (built here, after the
        solve).  The outputs are bit-identical."""
        if walk not in ("serial", "jump"):
            raise ValueError(f"walk must be 'serial' or 'jump', got {walk!r}")
        self.walk = walk
        EpisodeLoop.__init__(self, env)
        planner = env.planner
        self.dev = self._dev
        B, G = self.B, self.G = planner.B, planner.G
        self._heights = _per_instance(heights, B, G, "heights")
        self._risks = _per_instance(risks, B, G, "risks")
        if planner._shared_map and B > 1 and not all(np.array_equal(self._risks[0], r) for r in self._risks[1:]):
            raise ValueError("per-instance risk maps need a planner without shared_map")
        self.stuck_threshold = float(stuck_threshold)
        a_lim = np.asarray(a_lim.detach().cpu() if torch.is_tensor(a_lim) else a_lim, np.float32).reshape(2)
        self._a_lim = (C.c_float * 2)(float(a_lim[0]), float(a_lim[1]))
        self.delta_t, self.lookahead_distance = float(delta_t), float(lookahead_distance)
        self.num_lin_vel, self.num_ang_vel = int(num_lin_vel), int(num_ang_vel)
        if self.num_lin_vel < 1 or self.num_ang_vel < 1 or self.num_lin_vel * self.num_ang_vel > 1024:
            raise ValueError("num_lin_vel * num_ang_vel must be in [1, 1024]")
        env._check_stream()
        # the DWA rolls its candidates out on the risk map (the dynamics' traversability, dwa.py:224-227)
        if planner._shared_map:
            planner.set_map(self._risks[0], -1)
        else:
            for b in range(B):
                planner.set_map(self._risks[b], b)
        # the A* planner of every instance: one goal-rooted solve, goal = the environment's goal (astar.py:71)
        self.resolution = planner.resolution
        self._x0, self._y0 = planner.x_limits[0], planner.y_limits[0]
        self._handle = C.c_void_p()
        self._check(self._lib.bn_astar_create(planner.device_id, G, G, B, C.byref(self._handle)))
        goals = env._goal_pos.detach().cpu().numpy().astype(np.float32)
        for b in range(B):
            self._check(self._lib.bn_astar_set_map(self._astar, b, C.c_void_p(self._heights[b].ctypes.data),
                                                         C.c_void_p(self._risks[b].ctypes.data), _capi.BN_MEM_HOST,
                                                         self.stuck_threshold, self.resolution))
            gx, gy = self.pos_to_index(goals[b])
            self._check(self._lib.bn_astar_set_goal(self._astar, b, gx, gy))
        self._check(self._lib.bn_astar_solve_async(self._astar, stream_ptr(self._dev)))
        if walk == "jump":
            self._check(self._lib.bn_astar_jump_build_async(self._astar, stream_ptr(self._dev)))
        self._prev = torch.zeros(B, 2, device=self._dev)          # the window centre: DWA's _previous_action_seq[0] (zeros, dwa.py:59)
        self.status = np.zeros(B, np.int32)
        self.status_step = np.full(B, -1, np.int32)
        _capi.check(self._lib.bn_astar_dwa_reset(self._h))
        self._register()

    def pos_to_index(self, pos):
        """AStar._pos_to_index (astar.py:215-228): float32 arithmetic, int() truncates toward zero."""
        p = np.asarray(pos, np.float32)
        return (int((p[0] - np.float32(self._x0)) / np.float32(self.resolution)),
                int((p[1] - np.float32(self._y0)) / np.float32(self.resolution)))

    def reset(self):
        """A new episode: forget the root cells, the statuses and the step count, and re-centre the window on zero.  env.reset()
        calls it."""
        self.env._check_stream()
        _capi.check(self._lib.bn_astar_dwa_reset(self._h))
        self._prev.zero_()
        self._rows = 0
        self.status = np.zeros(self.B, np.int32)
        self.status_step = np.full(self.B, -1, np.int32)

    def run(self, n_steps: int, z: Optional[torch.Tensor] = None, log: bool = True):
        """n_steps control steps from the environment's current states.  z: (n_steps, B) injected slip draws; None draws them
        like env.step does (Philox keyed by the env seed and the step index).  Returns numpy arrays (states (n+1, B, 3),
        rewards (n, B), actions (n, B, 2), sub_goals (n, B, 2), done_step (B), status (B)); a frozen instance's rows hold its
        state and NaN elsewhere.  done_step and status steps count from the last reset.  log=False only enqueues and
        returns None: the log, done_step and status stay on the device (episode_buffers()), `status` / `status_step` here are
        not refreshed and the walks' error word is not read."""
        n = self._guard(n_steps)
        zp = self._slip_draws(z, n)
        state = self.env._robot_state.contiguous()
        _capi.check(self._lib.bn_astar_dwa_set_walk(self._h, 1 if self.walk == "jump" else 0))   # (the planner handle may serve other loops)
        _capi.check(self._lib.bn_astar_dwa_episode_async(
            self._h, self._astar, n, C.c_void_p(state.data_ptr()), _capi.BN_MEM_DEVICE, C.c_void_p(self._prev.data_ptr()),
            self._a_lim, self.delta_t, self.num_lin_vel, self.num_ang_vel, self.lookahead_distance,
            C.c_void_p(None if zp is None else zp.data_ptr())))
        self._keep = (state, zp)
        B = self.B
        if not log:
            ptr = self.episode_buffers()[0]
            self._advance(n, self.view(ptr, (n + 1, B, 3))[-1].clone())
            return None
        states = np.empty((n + 1, B, 3), np.float32)
        rewards = np.empty((n, B), np.float32)
        actions = np.empty((n, B, 2), np.float32)
        sub_goals = np.empty((n, B, 2), np.float32)
        done = np.empty(B, np.int32)
        status = np.empty(B, np.int32)
        status_step = np.empty(B, np.int32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        rc = self._lib.bn_astar_dwa_episode_log(self._h, ptr(states), ptr(rewards), ptr(actions), ptr(sub_goals), ptr(done),
                                                ptr(status), ptr(status_step))
        if rc == _capi.BN_OK or rc == _capi.BN_ERR_STATE:      # the steps ran (a broken walk only froze its rover): keep in step
            self._advance(n, torch.as_tensor(states[-1], device=self._dev).contiguous())
            self.status, self.status_step = status, status_step
        _capi.check(rc)
        return states, rewards, actions, sub_goals, done, status

    def set_root(self, instance: int, cell):
        """Instance `instance`'s root cell (ix, iy), or None to forget it: the start of the previous path DWA keeps where the
        current cell has none.  For teacher-forced steps from recorded states."""
        ix, iy = (-1, -1) if cell is None else (int(cell[0]), int(cell[1]))
        _capi.check(self._lib.bn_astar_dwa_set_root(self._h, int(instance), ix, iy))

    def raise_for_status(self):
        """Raise what the reference loop raised for the first instance that stopped (ValueError with AStar.forward's text)."""
        for b in range(self.B):
            s = int(self.status[b])
            if s == _capi.BN_AD_OK:
                continue
            if s in _MESSAGES:
                raise ValueError(_MESSAGES[s])
            raise RuntimeError(f"instance {b}: the A* field solve failed (status {s})")
