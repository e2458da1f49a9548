"""CPU statement of the A* + DWA closed loop (the reference's test_astar_dwa.py:179-211), composed from the existing oracle
parts: astar_oracle.solve / walk (the goal-rooted field and its next-hop walk), oracle.dwa_sub_goal and oracle.dwa (DWA.forward),
oracle.env_step_sampled (PlanetaryEnv.step with an explicit slip draw).  The rules the device loop (csrc/astar_dwa.hip) follows:
the start cell truncates, an out-of-bounds start or goal stops the episode, an unreachable start keeps the previous path."""
import numpy as np

import astar_oracle as A
from oracle import oracle as O

OK, OUT_OF_BOUNDS, GOAL_COLLISION = 0, 1, 2


def start_cell(pos, x0, y0, res):
    """AStar._pos_to_index: int() of the float32 quotient, truncating toward zero (not floor)."""
    f = np.float32
    qx = (f(pos[0]) - f(x0)) / f(res)
    qy = (f(pos[1]) - f(y0)) / f(res)
    return int(qx), int(qy)


def window(prev, a_lim, dt, nv, nw, u_min=(0.0, -1.0), u_max=(1.0, 1.0)):
    """DWA._generate_actions (dwa.py:168-199) with ATen's scalar linspace, in float32: (nv * nw, 2), v major."""
    f = np.float32
    lo = [max(f(u_min[i]), f(prev[i]) - f(a_lim[i]) * f(dt)) for i in range(2)]
    hi = [min(f(u_max[i]), f(prev[i]) + f(a_lim[i]) * f(dt)) for i in range(2)]

    def lin(a, b, n):
        if n == 1:
            return np.array([a], np.float32)
        step = (b - a) / f(n - 1)
        return np.array([a + step * f(i) if i < n // 2 else b - step * f(n - 1 - i) for i in range(n)], np.float32)
    vs, ws = lin(lo[0], hi[0], nv), lin(lo[1], hi[1], nw)
    return np.stack([np.repeat(vs, nw), np.tile(ws, nv)], 1).astype(np.float32)


def path_points(nodes, res):
    """_reconstruct_path (astar.py:213): f32(ix) * f32(res), x_limits[0] ignored."""
    return np.asarray(nodes, np.int64).astype(np.float32) * np.float32(res)


class Loop:
    """One rover: step() = AStar.forward -> DWA.update_reference_path -> DWA.forward -> env.step."""

    def __init__(self, heights, risk, thr, res, goal_pos, T, MU, SG, goal_thr=1.0, a_lim=(0.5, 0.5), dwa_dt=0.1, nv=10, nw=10,
                 lookahead=1.0, env_dt=0.1, u_min=(0.0, -1.0), u_max=(1.0, 1.0)):
        self.G = risk.shape[0]
        self.res, self.thr, self.risk = res, thr, np.asarray(risk, np.float32)
        self.goal_pos = np.asarray(goal_pos, np.float32)
        self.goal = start_cell(self.goal_pos, 0.0, 0.0, res)
        gx, gy = self.goal
        self.goal_in = 0 <= gx < self.G and 0 <= gy < self.G
        self.goal_col = self.goal_in and bool(self.risk[gy, gx] <= np.float32(thr))
        self.nxt = A.solve(heights, risk, thr, res, self.goal)[1] if self.goal_in else None
        self.u_min, self.u_max = u_min, u_max
        self.p = O.make_params(64, T, self.G, res, self.goal_pos, thr=thr, u_min=u_min, u_max=u_max)
        self.pe = O.make_params(64, T, self.G, res, self.goal_pos, thr=thr, dt=env_dt, u_min=u_min, u_max=u_max)
        self.MU, self.SG, self.goal_thr = MU, SG, goal_thr
        self.a_lim, self.dwa_dt, self.nv, self.nw, self.look = a_lim, dwa_dt, nv, nw, lookahead
        self.prev = np.zeros(2, np.float32)
        self.path = None                      # DWA.reference_path: kept when AStar.forward returns None
        self.status, self.status_step = OK, -1

    def astar(self, state):
        """AStar.forward: (status, path points or None)."""
        ix, iy = start_cell(state, 0.0, 0.0, self.res)
        if not (0 <= ix < self.G and 0 <= iy < self.G) or not self.goal_in:
            return OUT_OF_BOUNDS, None
        if self.goal_col:
            return GOAL_COLLISION, None
        nodes = A.walk(self.nxt, (ix, iy))
        return OK, None if nodes is None else path_points(nodes, self.res)

    def sub_goal(self, state, actions):
        if self.path is None:
            return np.asarray(self.goal_pos, np.float32)                 # dwa.py:243-247
        return O.dwa_sub_goal(self.p, self.risk, state, actions[0], self.path, self.look)[0]

    def step(self, j, state, z, teacher=None):
        """One control step from `state` with slip draw z; returns (next state, reward, terminated, sub_goal, action) or None
        when AStar.forward raised (self.status / status_step say what).  teacher: (window centre, previous path or None) to
        start from -- the fixture's teacher forcing."""
        if teacher is not None:
            self.prev, self.path = teacher
        status, path = self.astar(state)
        if status != OK:
            self.status, self.status_step = status, j
            return None
        if path is not None:
            self.path = path                                                # update_reference_path(None) keeps the old one
        actions = window(self.prev, self.a_lim, self.dwa_dt, self.nv, self.nw, self.u_min, self.u_max)
        sg = self.sub_goal(state, actions)
        best = O.dwa(self.p, self.risk, state, actions, sg)["best"]
        self.prev = actions[best]
        ns, rw, term = O.env_step_sampled(self.pe, self.MU, self.SG, z, self.goal_thr, state, self.prev)
        return ns, rw, term, sg, self.prev.copy()


def root_path(loop, root):
    """The path DWA keeps for a root cell (the latest start whose walk reached the goal), or None before one."""
    return None if root[0] < 0 else path_points(A.walk(loop.nxt, (int(root[0]), int(root[1]))), loop.res)


def fixture_loop(fx, name):
    """A Loop on episode `name` of tests/golden/astar_dwa_loop.npz (risk = the expected-value map = the latent mean)."""
    mean = fx[f"{name}__mean"]
    steer = bool(fx[f"{name}__steer"])
    bounds = {} if steer else dict(u_min=(0.5, 0.0), u_max=(1.0, 0.0))
    return Loop(fx[f"{name}__heights"], mean, float(fx["thr"]), float(fx["res"]), fx[f"{name}__goal"], int(fx["T"]), mean,
                np.full_like(mean, float(fx["std"])), goal_thr=float(fx["goal_threshold"]), a_lim=tuple(fx["a_lim"]),
                dwa_dt=float(fx["delta_t"]), nv=int(fx["nv"]), nw=int(fx["nw"]), lookahead=float(fx["lookahead"]), **bounds)
