"""CPU statement of the A* + DWA closed loop (the reference's test_astar_dwa.py:179-211), composed from the existing oracle
parts: astar_oracle.solve / walk (the goal-rooted field and its next-hop walk), oracle.dwa_sub_goal and oracle.dwa (DWA.forward),
oracle.env_step_sampled (PlanetaryEnv.step with an explicit slip draw).  The rules the device loop (csrc/astar_dwa.hip) follows:
the start cell truncates, an out-of-bounds start or goal stops the episode, an unreachable start keeps the previous path."""
import numpy as np

import astar_oracle as A
from oracle import oracle as O

OK, OUT_OF_BOUNDS, GOAL_COLLISION = 0, 1, 2

# The sub-goal rule tests |atan2f(dy, dx) - th| < pi/2 in float32, and the device's atan2f and the host libm's need not round alike:
# a path point whose bearing lies within DELTA of the boundary may be "ahead" on one side only.  Derived, not tuned (DESIGN.md,
# "Arithmetic spec"): DELTA = (max(E_dev, E_host) + 1) * 2^-22 with the two measured maximum errors in ulps of the result
#   E_dev  = 2.44 ulp  (MI355X, bn_device_math_eval fn 6 against float64 arctan2, tests/test_gpu_device_math.py)
#   E_host = 1.42 ulp  (glibc through oracle_atan2f, tests/test_astar_dwa_oracle.py)
# |atan2| < 4, so one ulp of it is at most 2^-22; the + 1 covers the rounding of the subtraction of th (|ang| is near pi/2 < 2
# there: half an ulp of it is 2^-24) and the rule's float32 threshold PI_F / 2, which lies 4.4e-8 = 0.18 * 2^-22 above pi/2.
ATAN2_E_DEV, ATAN2_E_HOST = 2.44, 1.42
DELTA = (max(ATAN2_E_DEV, ATAN2_E_HOST) + 1) * 2.0 ** -22


def atan2_pairs():
    """(dy, dx) float32 inputs on which the two atan2f are measured, away from the axes: the offsets (i, j) * res - frac of grid
    points from a rover for |i|, |j| <= 64 at res 0.3 and 0.5 (8 seeded fractions each), 2^20 random pairs, and tiny and huge ratios."""
    rng = np.random.default_rng(0)
    ys, xs = [], []
    i = np.arange(-64, 65, dtype=np.float32)
    for res in (0.3, 0.5):
        for frac in rng.random((8, 2)).astype(np.float32):
            dx, dy = np.meshgrid(i * np.float32(res) - frac[0], i * np.float32(res) - frac[1])
            ys.append(dy.ravel()); xs.append(dx.ravel())
    r = (rng.standard_normal((2, 1 << 20)) * 30.0).astype(np.float32)
    ys.append(r[0]); xs.append(r[1])
    big = np.float32([1e-45, 1e-40, 1e-38, 1e-30, 1e-10, 1.0, 1e10, 1e30, 3e38])
    b, a = np.meshgrid(big, big)
    for sy in (1, -1):
        for sx in (1, -1):
            ys.append((sy * b).ravel().astype(np.float32)); xs.append((sx * a).ravel().astype(np.float32))
    dy, dx = np.concatenate(ys).astype(np.float32), np.concatenate(xs).astype(np.float32)
    keep = (dy != 0) & (dx != 0)
    return dy[keep], dx[keep]


def atan2_ulp_error(got, dy, dx):
    """Largest |got - arctan2(dy, dx)| (float64 of the same float32 inputs) in ulps of the float32 result."""
    want = np.arctan2(dy.astype(np.float64), dx.astype(np.float64))
    ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
    return float((np.abs(np.asarray(got, np.float32).astype(np.float64) - want) / ulp).max())


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
                 lookahead=1.0, env_dt=0.1, u_min=(0.0, -1.0), u_max=(1.0, 1.0), x_limits=None, y_limits=None):
        """x_limits / y_limits: the grid's limits (None: [0, G * res], and y like x: make_params' defaults).  The cells of the
        start and the goal subtract the lower limit (_pos_to_index); the path's points do not (_reconstruct_path)."""
        self.G = risk.shape[0]
        self.res, self.thr, self.risk = res, thr, np.asarray(risk, np.float32)
        self.goal_pos = np.asarray(goal_pos, np.float32)
        if y_limits is None:
            y_limits = x_limits
        self.x0 = 0.0 if x_limits is None else x_limits[0]
        self.y0 = 0.0 if y_limits is None else y_limits[0]
        self.goal = start_cell(self.goal_pos, self.x0, self.y0, res)
        gx, gy = self.goal
        self.goal_in = 0 <= gx < self.G and 0 <= gy < self.G
        self.goal_col = self.goal_in and bool(self.risk[gy, gx] <= np.float32(thr))
        self.nxt = A.solve(heights, risk, thr, res, self.goal)[1] if self.goal_in else None
        self.u_min, self.u_max = u_min, u_max
        lim = dict(x_limits=x_limits, y_limits=y_limits)
        self.p = O.make_params(64, T, self.G, res, self.goal_pos, thr=thr, u_min=u_min, u_max=u_max, **lim)
        self.pe = O.make_params(64, T, self.G, res, self.goal_pos, thr=thr, dt=env_dt, u_min=u_min, u_max=u_max, **lim)
        self.MU, self.SG, self.goal_thr = MU, SG, goal_thr
        self.a_lim, self.dwa_dt, self.nv, self.nw, self.look = a_lim, dwa_dt, nv, nw, lookahead
        self.prev = np.zeros(2, np.float32)
        self.path = None                      # DWA.reference_path: kept when AStar.forward returns None
        self.status, self.status_step = OK, -1

    def astar(self, state):
        """AStar.forward: (status, path points or None)."""
        ix, iy = start_cell(state, self.x0, self.y0, self.res)
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

    def preview(self, state):
        """What the step from `state` (window centre self.prev) will pick, from one walk and without stepping: (bearing margin,
        index of the pick in the path the step uses -- None where the goal is the stage goal --, whether that path is the kept one).
        The margin says how far the pick is from hanging on the last bits of atan2f: the smallest | |ang64| - pi/2 | over the
        points with dist > lookahead of the path the step will use (the fresh one, else the kept one), seen from the slot-0 state
        oracle.dwa_sub_goal reports; ang64 = atan2(dy, dx) - th in float64 from the float32 dx, dy, th.  inf without such a
        point, without a path, or where AStar.forward raises."""
        status, fresh = self.astar(state)
        path = self.path if fresh is None else fresh
        if status != OK or path is None:
            return np.inf, None, False
        a0 = window(self.prev, self.a_lim, self.dwa_dt, self.nv, self.nw, self.u_min, self.u_max)[0]
        sg, sel, idx = O.dwa_sub_goal(self.p, self.risk, state, a0, path, self.look)
        return bearing_margin(path, sel, self.look), idx, fresh is None

    def bearing_margin(self, state):
        """The bearing margin of the step from `state`: preview(state)[0]."""
        return self.preview(state)[0]

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


def bearing_margin(path, sel, lookahead):
    """Loop.bearing_margin's rule on a float path (P, 2) seen from the slot-0 state sel (3,)."""
    path = np.asarray(path, np.float32).reshape(-1, 2)
    sel = np.asarray(sel, np.float32)
    dx, dy = path[:, 0] - sel[0], path[:, 1] - sel[1]                   # float32, as the rule computes them
    far = np.sqrt(dx * dx + dy * dy) > np.float32(lookahead)
    if not far.any():
        return np.inf
    ang = np.arctan2(dy[far].astype(np.float64), dx[far].astype(np.float64)) - np.float64(sel[2])
    return float(np.abs(np.abs(ang) - np.pi / 2).min())


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
