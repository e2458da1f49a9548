"""The reference's CL-RRT driver loop (test/test_cl_rrt.py:167-200) on the device, for the B environments of a
`BatchedPlanetaryEnv`: plan, replay the planned ACTION sequence open loop through the environment's step, measure at every control
step how far the rover has drifted from the planned STATE sequence, replan from the current state when the drift exceeds 1 m.

The follow half is one kernel (csrc/clrrt_loop.hip, bn_clrrt_loop_run): every rover runs its iterations on the device until the
call's end or until it needs a plan.  The planning half is the `CLRRT`'s own kernels under a mask: only the rovers that asked
replan, the others keep every byte.  The host looks at one counter per ROUND of replans and at nothing per control step.

    env = BatchedPlanetaryEnv(mppi, latent_mean, latent_std, start_pos, goal_pos, time_limit=100.0)
    planner = CLRRT(3, 2, dynamics, objectives, grid_map, delta_t=0.1)
    loop = CLRRTLoop(env, planner)                      # all rovers plan on the planner's one risk map, each to ITS goal
    loop = CLRRTLoop(env, planner, risk_maps=maps)      # ... or rover b on maps[b]; loop.set_risk_maps(maps) between episodes
    env.reset(seed=0)                                   # also resets the loop
    log = loop.run(1000)                                # dict of numpy arrays, rows by loop iteration
    loop.raise_for_status()                             # what the reference raised, for the first rover that stopped

Rules the reference's loop fixes (INTEGRATION.md "CL-RRT loop"): `t` counts loop ITERATIONS, and a flagged replan
consumes one without a step; the slip draw of iteration t is z row t, or Philox keyed by (env seed, t); the goal node's heading is
the rover's first plan's for the whole episode; where the reference raises or fails, the rover alone stops with a status.
Teacher forcing: with `samples` (P, B, max_iterations, 3), rover b's p-th plan since the reset grows from table p instead of its
MT19937 stream, and a rover that needs a plan beyond P stops with NO_PLAN; `set_plans` installs plans without the planner.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _capi
from .clrrt import _Handle
from ._device import _check_seed
from ._episodes import EpisodeLoop

STATUS_NAMES = ("RUNNING", "GOAL", "TIME_LIMIT", "NO_PLAN", "NO_SEQUENCE", "PLAN_EXHAUSTED", "PATH_OVERFLOW", "OUT_OF_BOUNDS")
EVENT_NAMES = ("STEP", "REPLAN", "FROZEN")


class CLRRTLoop(EpisodeLoop):
    _noun, _buffers_fn, _row_draws = "iterations", "bn_clrrt_loop_episode_buffers", True
    _iters = property(lambda self: self._rows)
    # episode_buffers(): done_step is done_iter where the rover reached its goal, else -1; stopped the status where it is neither
    # RUNNING, GOAL nor TIME_LIMIT, else 0 (benchmark.clrrt_outcome_words states the rule on NumPy)

    def __init__(self, env, planner, seeds=None, risk_maps=None):
        """env: a BatchedPlanetaryEnv (its goals are the rovers' goals, its time limit the loop's); planner: a CLRRT on the same
        grid (its risk map, limits, action bounds and parameters serve every rover); seeds: B integers in 0 ... 2^32 - 1 for the
        rovers' planner streams, reseeded at every reset (default: the planner's seed for each); risk_maps: (B, G, G), rover b
        plans on map b (set_risk_maps)."""
        super().__init__(env)
        self.planner = planner
        if planner._dev != self._dev:
            raise ValueError(f"the planner is on {planner._dev}, the environment on {self._dev}")
        env._check_stream()
        sd = [planner._seed] * self.B if seeds is None else list(seeds)
        if len(sd) != self.B:
            raise ValueError("one seed per rover")
        self._seeds = np.array([_check_seed(s) for s in sd], np.uint64)
        self._handle = _Handle(self._lib, self._dev, self.B, planner)       # the loop's own: plan_batch and forward keep theirs
        if risk_maps is not None:
            self._handle.set_maps(risk_maps)
        self._zero()
        self.reset()
        self._register()

    def _zero(self):
        self.status = np.zeros(self.B, np.int32)
        self.done_iter = np.full(self.B, -1, np.int32)
        self.plans = np.zeros(self.B, np.int32)
        self.steps = np.zeros(self.B, np.int32)
        self.follow_ms = 0.0

    @property
    def elapsed(self) -> np.ndarray:
        """(B,) each rover's own elapsed time: its environment steps times delta_t, accumulated in float64 like the reference's."""
        m = int(self.steps.max()) if self.B else 0
        acc = np.concatenate(([0.0], np.cumsum(np.full(m, self.env._delta_t, np.float64))))      # elapsed += delta_t, step by step
        return acc[self.steps]

    def reset(self):
        """A new episode: iteration 0, no plans, statuses cleared, the planner streams reseeded.  The goal nodes are computed
        here, once: (x, y, atan2(goal - state)) from the environment's current states, as the rover's first forward() would.
        env.reset() calls it."""
        env = self.env
        if self._handle is None:                            # closed: env.reset() still finds it registered
            return
        env._check_stream()
        states = env._robot_state.detach().to("cpu", torch.float32)
        goals = env._goal_pos.detach().to("cpu", torch.float32)
        nodes = torch.cat((goals, torch.atan2(goals[:, 1] - states[:, 1], goals[:, 0] - states[:, 0])[:, None]), dim=1)
        self._goal_nodes = np.ascontiguousarray(nodes.numpy(), np.float32)
        _capi.check(self._lib.bn_clrrt_loop_reset(self._h, self._handle.h, self._goal_nodes.ctypes.data, self._seeds.ctypes.data,
                                                  float(env._delta_t), float(env._time_limit)))
        self._rows = 0
        self._zero()

    def set_risk_maps(self, risk_maps):
        """The rovers' own risk maps from the next plan on: (B, G, G) float32, a torch tensor on the host or the device (copied
        device to device on torch's current stream) or a NumPy array; None returns every rover to the planner's map.  Between
        episodes: the rovers' current plans stay as they were grown."""
        self.env._check_stream()
        self._handle.set_maps(risk_maps)

    def run(self, n_iterations: int, z: Optional[torch.Tensor] = None, samples: Optional[torch.Tensor] = None, stage_in_lds: bool = True,
            log: bool = True):
        """n loop iterations from the environment's current states; calling it again continues the episode.  z: (n, B) injected
        slip draws (row t: iteration t of this call); None draws them like env.step (Philox keyed by the env seed and the episode's
        iteration index).  samples: (P, B, max_iterations, 3) sample tables (teacher forcing).  stage_in_lds=False is a test knob:
        the follow kernel reads every plan from global memory; the logs are bit-identical.
        Returns a dict of numpy arrays, rows by iteration of this call: states (n+1, B, 3), rewards (n, B), actions (n, B, 2),
        deviations (n, B), plan_index (n, B), events (n, B); and per rover done_iter, status, plans, steps (since the reset).  A
        row without a step holds the rover's state and NaN elsewhere (a flagged replan keeps its deviation).
        log=False downloads nothing and returns None: the log and the rovers' words stay on the device (episode_buffers(),
        rover_buffers()); `status`, `done_iter`, `plans`, `steps` and `elapsed` here are not refreshed."""
        env, B = self.env, self.B
        n = self._guard(n_iterations)
        zp = self._slip_draws(z, n)
        sp, P = None, 0
        if samples is not None:
            sp = torch.as_tensor(samples).to(self._dev, torch.float32).contiguous()
            if sp.dim() != 4 or tuple(sp.shape[1:]) != (B, self._handle.iters, 3):
                raise ValueError(f"samples must be (P, {B}, {self._handle.iters}, 3), got {tuple(sp.shape)}")
            P = int(sp.shape[0])
            if P == 0:                                      # no table at all: every plan needed is beyond P (a non-null pointer says "injected")
                sp = torch.zeros(1, device=self._dev)
        state = env._robot_state.to(self._dev, torch.float32).contiguous().clone()
        ms = C.c_float(0.0)
        rc = self._lib.bn_clrrt_loop_run(self._h, self._handle.h, n, C.c_void_p(state.data_ptr()), C.c_void_p(None if zp is None else zp.data_ptr()),
                                         C.c_void_p(None if sp is None else sp.data_ptr()), P, 0 if stage_in_lds else 1, C.byref(ms))
        _capi.check(rc)
        self.follow_ms = float(ms.value)
        self._keep = (zp, sp)
        if not log:
            self._advance(n, state, elapsed=env._elapsed_time)
            return None
        out = {"states": np.empty((n + 1, B, 3), np.float32), "rewards": np.empty((n, B), np.float32), "actions": np.empty((n, B, 2), np.float32),
               "deviations": np.empty((n, B), np.float32), "plan_index": np.empty((n, B), np.int32), "events": np.empty((n, B), np.int32),
               "done_iter": np.empty(B, np.int32), "status": np.empty(B, np.int32), "plans": np.empty(B, np.int32), "steps": np.empty(B, np.int32)}
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        _capi.check(self._lib.bn_clrrt_loop_log(self._h, ptr(out["states"]), ptr(out["rewards"]), ptr(out["actions"]), ptr(out["deviations"]),
                                                ptr(out["plan_index"]), ptr(out["events"]), ptr(out["done_iter"]), ptr(out["status"]),
                                                ptr(out["plans"]), ptr(out["steps"])))
        self.status, self.done_iter, self.plans, self.steps = out["status"], out["done_iter"], out["plans"], out["steps"]
        self._advance(n, state, elapsed=float(self.elapsed.max()))
        return out

    def rover_buffers(self):
        """(status (B,), plans (B,)) int32 device tensors: views of the words the latest run left, valid until the next run."""
        st, pl = C.c_void_p(), C.c_void_p()
        _capi.check(self._lib.bn_clrrt_loop_rover_buffers(self._h, C.byref(st), C.byref(pl)))
        return self._handle.view(st.value, (self.B,), "<i4"), self._handle.view(pl.value, (self.B,), "<i4")

    def set_plans(self, actions, states, lengths=None, iteration: Optional[int] = None):
        """Teacher forcing: actions (B, L, 2), states (B, L + 1, 3) and lengths (B,) (default L for every rover) become the rovers'
        current plans, action_index 0, no replan pending.  iteration: also set the episode's iteration counter (the rovers', the
        loop's and the environment's step count), to continue a recorded episode from that iteration."""
        a = np.ascontiguousarray(torch.as_tensor(actions).detach().to("cpu", torch.float32).numpy())
        s = np.ascontiguousarray(torch.as_tensor(states).detach().to("cpu", torch.float32).numpy())
        B = self.B
        if a.ndim != 3 or a.shape[0] != B or a.shape[2] != 2 or s.shape != (B, a.shape[1] + 1, 3):
            raise ValueError(f"actions must be ({B}, L, 2) and states ({B}, L + 1, 3), got {a.shape} and {s.shape}")
        L = int(a.shape[1])
        ln = np.full(B, L, np.int32) if lengths is None else np.ascontiguousarray(np.asarray(lengths, np.int32).reshape(B))
        self.env._check_stream()
        it = -1 if iteration is None else int(iteration)
        _capi.check(self._lib.bn_clrrt_loop_set_plans(self._h, self._handle.h, a.ctypes.data, s.ctypes.data, ln.ctypes.data, L, it))
        if it >= 0:
            self._rows = it
            self.env._steps = self.env._draws = it          # run() advances the two together

    def buffer(self, which: int, shape, typestr="<f4") -> torch.Tensor:
        """A view of one of the loop's CL-RRT handle's device buffers (bn_clrrt_buffer_id): trees, paths, results, streams."""
        return self._handle.buffer(which, shape, typestr)

    def raise_for_status(self):
        """Raise what the reference's loop raised for the first rover that stopped on an error (GOAL and TIME_LIMIT are its two
        regular ends)."""
        for b in range(self.B):
            s, t = int(self.status[b]), int(self.done_iter[b])
            if s in (_capi.BN_CL_RUNNING, _capi.BN_CL_GOAL, _capi.BN_CL_TIME_LIMIT):
                continue
            if s == _capi.BN_CL_NO_PLAN:
                raise TypeError(f"rover {b}, iteration {t}: forward() returned (None, None): 'NoneType' object is not subscriptable")
            if s == _capi.BN_CL_PLAN_EXHAUSTED:
                raise IndexError(f"rover {b}, iteration {t}: action_index is out of bounds for the planned action sequence")
            if s == _capi.BN_CL_OUT_OF_BOUNDS:
                raise ValueError("Start or goal position is out of bounds.")
            if s == _capi.BN_CL_PATH_OVERFLOW:
                raise RuntimeError(f"rover {b}, iteration {t}: the path does not fit the path buffer: construct CLRRT with a larger path_cap")
            raise RuntimeError(f"rover {b}, iteration {t}: the start node is the cheapest node within the goal threshold: there is no sequence to return")
