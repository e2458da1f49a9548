"""The CL-RRT plan-follow-replan loop (the reference's test/test_cl_rrt.py:167-200) restated in NumPy, given the
plans and the slip draws: the specification csrc/clrrt_loop.hip implements, held to the reference's recorded episodes
(tests/golden/clrrt_loop.npz) in test_clrrt_loop_oracle.py.  The environment step is the existing oracle's
(oracle.env_step_sampled, the one tests/test_gpu_env.py holds the step kernel to); the deviation is rrt_spec.norm, the fused
float32 norm of DESIGN.md 4.6 item 4.  Written from the rules; imports neither the reference nor the library."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from rrt_spec import norm

RUNNING, GOAL, TIME_LIMIT, NO_PLAN, NO_SEQUENCE, PLAN_EXHAUSTED, PATH_OVERFLOW, OUT_OF_BOUNDS = range(8)
STEP, REPLAN, FROZEN = 0, 1, 2


def limit_steps(delta_t: float, time_limit: float) -> int:
    """The first step count at which PlanetaryEnv's float64 `elapsed += delta_t` exceeds the time limit."""
    elapsed, k = 0.0, 0
    while not elapsed > time_limit:
        elapsed += delta_t
        k += 1
    return k


def deviation(plan_states, state) -> np.float32:
    """min over ALL planned states of the float32 norm of (plan_xy - state_xy)."""
    ps = np.asarray(plan_states, np.float32)
    s = np.asarray(state, np.float32)
    return np.float32(norm(ps[:, 0] - s[0], ps[:, 1] - s[1]).min())


class Rover:
    """One rover.  plans: a callable (index, state) -> (actions (L, 2), states (L + 1, 3)), or None where forward() returns
    (None, None), or a status code where it raises; index counts the plans since the reset."""

    def __init__(self, p_env, MU, SG, goal_thr, state, plans, delta_t=0.1, time_limit=100.0):
        self.p, self.MU, self.SG, self.goal_thr = p_env, MU, SG, goal_thr
        self.state = np.asarray(state, np.float32).copy()
        self.plans = plans
        self.limit = limit_steps(float(delta_t), time_limit)       # the Python float the reference accumulates, not p_env.dt (float32)
        self.t, self.status, self.done_iter = 0, RUNNING, -1
        self.need, self.aidx, self.n_plans, self.steps = True, 0, 0, 0
        self.actions = self.plan_states = None

    def set_plan(self, actions, states):
        self.actions, self.plan_states = np.asarray(actions, np.float32), np.asarray(states, np.float32)
        self.aidx, self.need = 0, False

    def iterate(self, z):
        """One loop iteration with slip draw z.  Returns (event, reward, action (2,), deviation, plan index); the state is
        self.state afterwards."""
        nan, nan2 = np.float32(np.nan), np.full(2, np.nan, np.float32)
        t = self.t
        self.t += 1
        if self.status == RUNNING and self.need:
            got = self.plans(self.n_plans, self.state.copy())
            self.n_plans += 1
            if got is None:
                self.status, self.done_iter = NO_PLAN, t
            elif isinstance(got, int):
                self.status, self.done_iter = got, t
            else:
                self.set_plan(*got)
        if self.status != RUNNING:
            return FROZEN, nan, nan2, nan, self.n_plans - 1
        dev = nan
        if t > 0:
            dev = deviation(self.plan_states, self.state)
            if dev > np.float32(1.0):
                self.need = True
                return REPLAN, nan, nan2, dev, self.n_plans - 1
        if self.aidx >= len(self.actions):
            self.status, self.done_iter = PLAN_EXHAUSTED, t
            return FROZEN, nan, nan2, dev, self.n_plans - 1
        u = self.actions[self.aidx]
        self.aidx += 1
        ns, rw, term = O.env_step_sampled(self.p, self.MU, self.SG, float(z), self.goal_thr, self.state, u)
        self.state = ns
        self.steps += 1
        if term:
            self.status, self.done_iter = GOAL, t
        elif self.steps >= self.limit:
            self.status, self.done_iter = TIME_LIMIT, t
        return STEP, rw, u.copy(), dev, self.n_plans - 1

    def run(self, n, z):
        """n iterations; z (n,) slip draws (NaN where the reference took no step).  Returns the logs as the device loop lays them
        out: states (n + 1, 3), rewards, actions (n, 2), deviations, plan_index, events."""
        out = {"states": np.empty((n + 1, 3), np.float32), "rewards": np.empty(n, np.float32), "actions": np.empty((n, 2), np.float32),
               "deviations": np.empty(n, np.float32), "plan_index": np.empty(n, np.int32), "events": np.empty(n, np.int32)}
        out["states"][0] = self.state
        for i in range(n):
            ev, rw, u, dev, k = self.iterate(z[i])
            out["states"][i + 1] = self.state
            out["rewards"][i], out["actions"][i], out["deviations"][i], out["plan_index"][i], out["events"][i] = rw, u, dev, k, ev
        return out


def fixture_episode(fx, name):
    """Episode `name` of tests/golden/clrrt_loop.npz: (environment parameters, latent mean, latent std, plans list)."""
    G, res = int(fx["G"]), float(fx["res"])
    MU = np.clip(fx["mean"] * np.float32(float(fx[f"{name}__scale"])), 0.0, 0.7).astype(np.float32)
    SG = np.full_like(MU, float(fx["std"]))
    p = O.make_params(1, 1, G, res, fx["goal"], thr=float(fx["thr"]), dt=float(fx["delta_t"]))
    plans = []
    for k in range(int(fx[f"{name}__n_plans"])):
        plans.append((fx[f"{name}__p{k}__actions"], fx[f"{name}__p{k}__states"]) if bool(fx[f"{name}__p{k}__found"]) else None)
    return p, MU, SG, plans
