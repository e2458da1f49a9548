"""The closed-loop RRT planner restated in NumPy: the specification csrc/clrrt_kernels.hip implements, held to the
reference's recorded iterations (tests/golden/clrrt.npz) in test_clrrt_oracle.py.  Written from the rules; imports neither the
reference nor the library.

Number formats, as the reference runs under NumPy >= 2 (a float32 scalar combined with a Python number stays float32):
  * the six Dubins words, their angles, lengths and the turning centres are float32 (NumPy's own float32 cos / sin / arctan2 /
    arccos / arcsin / remainder: `M32` below, so that another implementation of them can be put in their place);
  * the path points are float64: the arc length x = 0.25 i is float64 (np.arange), and it enters every point formula;
  * truncation, pure pursuit and the PID run in float64 on those points; the action is cast to float32;
  * the integral is a float32 number updated as f32(f64(integral) + e dt);
  * transit and the costs are float32, with the library's sincos (csrc/bn_device_math.h) restated here.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional

import numpy as np

from terrain_draws_spec import Stream

f32, f64 = np.float32, np.float64
PI32, TWO_PI32, HALF_PI32 = f32(np.pi), f32(2 * np.pi), f32(np.pi / 2)
PI, TWO_PI = float(np.pi), float(2 * np.pi)
RADIUS, SPACING, LOOKAHEAD2 = 1.0, 0.25, 0.25
WORDS = ("LSL", "RSR", "RSL", "LSR", "RLR", "LRL")
TRANSIT_DT = f32(0.1)               # UnicycleModel.transit's default delta_t: CLRRT does not pass its own
# Largest device-versus-fixture difference of a path point, in metres, rounded up (measured on an MI355X: 1.82e-6):
# a steer whose discrete decisions change when the points move by this much is "marginal" and may be left out of a comparison.
EPS_POINT = 2.0e-6

# mid_height: h = sqrt(4 - (inter / 2)^2) of the middle circle, which the reference writes with the scalars' own power operator
M32 = SimpleNamespace(cos=np.cos, sin=np.sin, arctan2=np.arctan2, arccos=np.arccos, arcsin=np.arcsin, sqrt=np.sqrt,
                      mid_height=lambda inter: f32((f32(4) - (inter / f32(2)) ** 2) ** 0.5))


def _rounded(fn):
    """The float64 function (Python's math) rounded once to float32: what the device takes a float32 transcendental to be."""
    return lambda *a: f32(fn(*(float(v) for v in a)))


def _mid_height_sqrt(inter):
    hi = f32(f32(inter) * f32(0.5))
    return f32(np.sqrt(f32(f32(4) - f32(hi * hi))))


# The device's own float32 math (csrc/clrrt_kernels.hip sincos32, atan2_32, acos, asin): with it the float32 half of a steer has no
# freedom left.  sqrt is IEEE on both sides; the middle circle's height is a float32 sqrt in the kernel.
M64R = SimpleNamespace(cos=_rounded(math.cos), sin=_rounded(math.sin), arctan2=_rounded(math.atan2), arccos=_rounded(math.acos),
                       arcsin=_rounded(math.asin), sqrt=np.sqrt, mid_height=_mid_height_sqrt)
DOUBLE_ROUNDING_BAND = 2.0 ** -44


def rounding_margin(r: float) -> float:
    """Relative distance of the float64 r from the nearest float32 rounding boundary (the midpoint of two neighbouring float32
    values); inf where r is 0 or not finite."""
    r = float(r)
    if r == 0.0 or not math.isfinite(r):
        return math.inf
    v = f32(r)
    lo, hi = float(np.nextafter(v, f32(-np.inf))), float(np.nextafter(v, f32(np.inf)))
    return min(abs(r - (float(v) + lo) / 2), abs(r - (float(v) + hi) / 2)) / abs(r)


def instrumented_m64r():
    """(namespace, margins): M64R whose every transcendental call appends rounding_margin of its float64 result to `margins`.  A
    steer "sits in the double-rounding band" if one of them is below DOUBLE_ROUNDING_BAND: there a 1-ulp difference between two
    float64 libraries could flip the float32 value."""
    margins = []

    def wrap(fn):
        def call(*a):
            r = fn(*(float(v) for v in a))
            margins.append(rounding_margin(r))
            return f32(r)
        return call
    ns = SimpleNamespace(cos=wrap(math.cos), sin=wrap(math.sin), arctan2=wrap(math.atan2), arccos=wrap(math.acos), arcsin=wrap(math.asin),
                         sqrt=np.sqrt, mid_height=_mid_height_sqrt)
    return ns, margins


def pymod(a, b):
    """Python's float modulo (np.remainder, torch.remainder): fmod, then the divisor is added where the signs differ.  The result
    has the sign of the divisor; the addition rounds in the format of the operands."""
    t = type(a) if isinstance(a, np.floating) else float
    m = t(math.fmod(a, b)) if t is float else t(np.fmod(a, t(b)))
    if m != 0 and ((m < 0) != (b < 0)):
        m = t(m + t(b))
    return m


def norm2_32(dx, dy):
    """np.linalg.norm of a float32 2-vector: sqrt of the dot product."""
    v = np.array([dx, dy], np.float32)
    return f32(np.sqrt(v.dot(v)))


# ---- samples ---------------------------------------------------------------------------------------------------------------------
def goal_heading(start, goal):
    """atan2(goal - start) in float32: torch.atan2 of the float32 differences, taken as the float64 function rounded to float32
    (NumPy's own float32 arctan2 is an ulp off on some arguments, (16, 16) among them)."""
    s, g = np.asarray(start, np.float32), np.asarray(goal, np.float32)
    return f32(np.arctan2(f64(f32(g[1] - s[1])), f64(f32(g[0] - s[0]))))


def parse_samples(stream: Stream, iters: int, x_limits, y_limits, goal_node, rate: float):
    """(samples (iters, 3) float32, is_goal (iters,) bool): one uniform per iteration, three more where it is not below f32(rate):
    x, y as DESIGN.md 4.6 item 3 and theta = f32(f32(u 2) f32(pi))."""
    xs, x0 = f32(x_limits[1] - x_limits[0]), f32(x_limits[0])
    ys, y0 = f32(y_limits[1] - y_limits[0]), f32(y_limits[0])
    g = np.asarray(goal_node, np.float32)[:3]
    out, flag = np.empty((iters, 3), np.float32), np.zeros(iters, bool)
    for i in range(iters):
        if stream.uniform() < f32(rate):
            out[i], flag[i] = g, True
        else:
            out[i, 0] = f32(f32(stream.uniform() * xs) + x0)
            out[i, 1] = f32(f32(stream.uniform() * ys) + y0)
            out[i, 2] = f32(f32(stream.uniform() * f32(2)) * PI32)
    return out, flag


# ---- Dubins ----------------------------------------------------------------------------------------------------------------------
def find_center(p, left: bool, m=M32):
    a = f32(p[2] + (HALF_PI32 if left else -HALF_PI32))
    return np.array([f32(p[0] + f32(m.cos(a))), f32(p[1] + f32(m.sin(a)))], np.float32)


def all_options(start, end, m=M32):
    """The six words in the reference's order: (total length, (beta0, beta2, third), straight).  float32 throughout."""
    s, e = np.asarray(start, np.float32), np.asarray(end, np.float32)
    ls, rs, le, re = find_center(s, True, m), find_center(s, False, m), find_center(e, True, m), find_center(e, False, m)
    inf = (float("inf"), np.zeros(3, np.float32))
    mod = lambda v: pymod(f32(v), TWO_PI32)
    out = []
    # LSL, RSR
    for (c0, c2, sign) in ((ls, le, 1), (rs, re, -1)):
        sd = norm2_32(c0[0] - c2[0], c0[1] - c2[1])
        al = f32(m.arctan2(f32(c2[1] - c0[1]), f32(c2[0] - c0[0])))
        if sign > 0:
            b2, b0 = mod(e[2] - al), mod(al - s[2])
        else:
            b2, b0 = mod(-e[2] + al), mod(-al + s[2])
        out.append((f32(f32(b2 + b0) + sd), np.array([sign * b0, sign * b2, sd], np.float32), True))
    # RSL, LSR
    for (c0, c2, rsl) in ((rs, le, True), (ls, re, False)):
        med = (c2 - c0) / f32(2)
        psia = f32(m.arctan2(med[1], med[0]))
        half = norm2_32(med[0], med[1])
        if half < RADIUS:
            out.append(inf + (True,))
            continue
        al = f32(m.arccos(f32(1) / half))
        if rsl:
            b0 = mod(-f32(f32(f32(psia + al) - s[2]) - HALF_PI32))
            b2 = mod(f32(f32(f32(PI32 + e[2]) - HALF_PI32) - al) - psia)
        else:
            b0 = mod(f32(f32(psia - al) - s[2]) + HALF_PI32)
            b2 = mod(f32(f32(f32(0.5 * np.pi) - e[2]) - al) + psia)
        sd = f32(f32(2) * f32(m.sqrt(f32(f32(half * half) - f32(1)))))
        out.append((f32(f32(b0 + b2) + sd), np.array([-b0, b2, sd] if rsl else [b0, -b2, sd], np.float32), True))
    # RLR, LRL
    for (c0, c2, rlr) in ((rs, re, True), (ls, le, False)):
        d = norm2_32(c0[0] - c2[0], c0[1] - c2[1])
        if d > 4 * RADIUS or d < 2 * RADIUS:
            out.append(inf + (False,))
            continue
        gam = f32(f32(2) * f32(m.arcsin(d / f32(4))))
        at = f32(m.arctan2(f32(c2[1] - c0[1]), f32(c2[0] - c0[0])))
        tail = f32(f32(PI32 - gam) / f32(2))
        if rlr:
            b0 = mod(f32(f32(-at + s[2]) + HALF_PI32) + tail)
            b2 = mod(f32(f32(at - e[2]) + HALF_PI32) + tail)
        else:
            b0 = mod(f32(f32(at - s[2]) + HALF_PI32) + tail)
            b2 = mod(f32(f32(-at + e[2]) + HALF_PI32) + tail)
        third = f32(TWO_PI32 - gam)
        total = f32(f32(third + abs(b0)) + abs(b2))
        out.append((total, np.array([-b0, -b2, third] if rlr else [b0, b2, third], np.float32), False))
    return out


def choose_word(options) -> int:
    """min() over the lengths: the first of equal lengths."""
    best = 0
    for k in range(1, 6):
        if options[k][0] < options[best][0]:
            best = k
    return best


def _arc(ref, beta, center, x):
    a = f64(ref[2]) + (x / RADIUS - PI / 2) * f64(np.sign(beta))
    return np.array([f64(center[0]) + RADIUS * np.cos(a), f64(center[1]) + RADIUS * np.sin(a)])


def dubins_points(start, end, m=M32, limit: Optional[int] = None):
    """(points (N, 2) float64, word index): a point per 0.25 of arc length from 0 up to (not including) the total, then the end
    point.  limit: stop after that many points (the truncation needs the first few only)."""
    s, e = np.asarray(start, np.float32), np.asarray(end, np.float32)
    opts = all_options(s, e, m)
    w = choose_word(opts)
    path, straight = opts[w][1], opts[w][2]
    a0, a1 = f32(abs(path[0])), f32(abs(path[1]))
    c0 = find_center(s, bool(path[0] > 0), m)
    c2 = find_center(e, bool(path[1] > 0), m)
    if straight:
        total = f32(f32(a1 + a0) + path[2])
        if a0 > 0:
            ang = f32(s[2] + f32(f32(a0 - HALF_PI32) * np.sign(path[0])))
            ini = np.array([f32(c0[0] + f32(m.cos(ang))), f32(c0[1] + f32(m.sin(ang)))], np.float32)
        else:
            ini = s[:2].copy()
        if a1 > 0:
            ang = f32(e[2] + f32(f32(-a1 - HALF_PI32) * np.sign(path[1])))
            fin = np.array([f32(c2[0] + f32(m.cos(ang))), f32(c2[1] + f32(m.sin(ang)))], np.float32)
        else:
            fin = e[:2].copy()
        dist = norm2_32(ini[0] - fin[0], ini[1] - fin[1])
    else:
        total = f32(f32(a1 + a0) + f32(abs(path[2])))
        inter = norm2_32(c0[0] - c2[0], c0[1] - c2[1])
        u = (c2 - c0) / inter
        orth = np.array([-u[1], u[0]], np.float32)
        h = m.mid_height(inter)
        c1 = ((c0 + c2) / f32(2) + (np.sign(path[0]) * orth) * h).astype(np.float32)
        psi0 = f32(f32(m.arctan2(f32(c1[1] - c0[1]), f32(c1[0] - c0[0]))) - PI32)
    count = int(math.ceil(float(total) / SPACING))               # len(np.arange(0, total, 0.25)), computed in float64
    n = count if limit is None else min(count, limit)
    lim0, lim1 = f64(a0) * RADIUS, f64(f32(total - a1))
    pts = []
    for i in range(n):
        x = f64(i * SPACING)
        if x < lim0:
            pts.append(_arc(s, path[0], c0, x))
        elif x > lim1:
            pts.append(_arc(e, path[1], c2, x - f64(total)))
        elif straight:
            c = (x - f64(a0)) / f64(dist)
            pts.append(c * fin.astype(np.float64) + (1 - c) * ini.astype(np.float64))
        else:
            a = f64(psi0) - f64(np.sign(path[0])) * (x / RADIUS - f64(a0))
            pts.append(np.array([f64(c1[0]) + RADIUS * np.cos(a), f64(c1[1]) + RADIUS * np.sin(a)]))
    if limit is None or count < limit:
        pts.append(e[:2].astype(np.float64))
    return np.array(pts, np.float64).reshape(-1, 2), w


def truncate(points, delta: float):
    """The path up to the first index whose float64 cumulative length (a sequential sum) exceeds delta."""
    d = points[1:] - points[:-1]
    seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    acc = 0.0
    for i, v in enumerate(seg):
        acc = acc + float(v)
        if acc > delta:
            return points[:i + 1]
    return points


def reference_path(start, end, delta: float, m=M32):
    """The truncated path of one steer.  Only the first points are generated: every segment is at most 0.25 (+ rounding) long,
    so the limit index lies within ceil(delta / 0.2) + 2 points."""
    limit = int(math.ceil(delta / 0.2)) + 2
    pts, w = dubins_points(start, end, m, limit)
    out = truncate(pts, delta)
    assert len(out) < limit or len(pts) < limit
    return out, w


# ---- float32 transit and costs ---------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return f32(f64(a) * f64(b) + f64(c))


def sincos_spec(x):
    """csrc/bn_device_math.h sincos_spec: (sin, cos) of a float32 angle."""
    x = f32(x)
    t = _fma32(x, f32(0.318309886183790672), f32(12582912.0))
    fn = f32(t - f32(12582912.0))
    r = _fma32(-fn, f32(3.140625), x)
    r = _fma32(-fn, f32(9.67502593994140625e-4), r)
    r = _fma32(-fn, f32(1.509957990978376432e-7), r)
    s = f32(r * r)
    p = f32(2.599125082269893e-06)
    q = _fma32(f32(-2.6072027026202704e-07), s, f32(2.476157715136651e-05))
    for cp, cq in ((-0.0001980613305931911, -0.001388839678838849), (0.008333009667694569, 0.04166664183139801), (-0.16666656732559204, -0.5)):
        p, q = _fma32(p, s, f32(cp)), _fma32(q, s, f32(cq))
    S = _fma32(f32(p * s), r, r)
    C = _fma32(q, s, f32(1))
    if int(np.array(t, np.float32).view(np.uint32)) & 1:
        S, C = f32(-S), f32(-C)
    return S, C


def wrap32(th):
    return f32(pymod(f32(f32(th) + PI32), TWO_PI32) - PI32)


@dataclass
class Config:
    mean: np.ndarray                 # (G, G) float32 risk
    res: float
    thr: float
    goal: np.ndarray                 # (2,) float32: the stage and terminal costs' goal
    delta_t: float = 0.1             # the PID's step
    max_seqs: int = 250
    delta: float = 5.0
    x0: float = 0.0
    y0: float = 0.0
    u_min: tuple = (0.0, -1.0)
    u_max: tuple = (1.0, 1.0)
    G: int = field(init=False)

    def __post_init__(self):
        self.G = int(self.mean.shape[0])
        self.mean = np.asarray(self.mean, np.float32)
        self.goal = np.asarray(self.goal, np.float32)


def cell(cfg: Config, x, y):
    ix = int(np.floor(f32(f32(f32(x) - f32(cfg.x0)) / f32(cfg.res))))
    iy = int(np.floor(f32(f32(f32(y) - f32(cfg.y0)) / f32(cfg.res))))
    return min(max(ix, 0), cfg.G - 1), min(max(iy, 0), cfg.G - 1)


def trav(cfg: Config, x, y):
    ix, iy = cell(cfg, x, y)
    return f32(f32(1) - np.clip(cfg.mean[iy, ix], f32(0), f32(1))), (ix, iy)


def point_cost(cfg: Config, x, y):
    """Objectives.stage_cost at a position: the float32 distance to the goal + 1e4 where the traversability is at or below the
    stuck threshold."""
    dx, dy = f32(f32(x) - cfg.goal[0]), f32(f32(y) - cfg.goal[1])
    tv, c = trav(cfg, x, y)
    return f32(f32(np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))) + (f32(1.0e4) if tv <= f32(cfg.thr) else f32(0))), c


# ---- one steer -------------------------------------------------------------------------------------------------------------------
@dataclass
class Steer:
    path: np.ndarray                 # truncated reference path (N, 2) float64
    word: int
    targets: np.ndarray              # (L,) target index per step
    actions: np.ndarray              # (L, 2) float32, as stored (not clamped)
    states: np.ndarray               # (L + 1, 3) float32: slots 0 .. L-1 hold the un-clamped, un-wrapped next state, slot L the last state
    cells: list                      # the cells the costs read
    cost: np.float32
    feasible: bool
    length: int
    ctrl: np.ndarray                 # (4,) float64: previous error and integral of the linear, then the angular controller
    integrals: np.ndarray            # (2,) float32: the integrals, what the parent's stored row receives
    wrap_arg: float = 0.0            # the last step's (bearing - heading) + pi, the largest intermediate of its angular error


def follow(cfg: Config, from_state, ctrl, path, word=-1, nudge=None) -> Steer:
    """_simulate_path_following on a given (truncated) path.  nudge=(a, b): the linear error is multiplied by 1 + a and b is added
    to every bearing atan2(dy, dx), the lanes' validity test and the target's errors alike, before anything is cast or compared:
    the freedom another float64 atan2 / sqrt / fmod has once the points are given.  None leaves the arithmetic as it is."""
    x, y, th = (f32(v) for v in np.asarray(from_state, np.float32))
    lin_i, ang_i = f32(ctrl[1]), f32(ctrl[3])
    e_lin, e_ang = f64(ctrl[0]), f64(ctrl[2])
    px, py = path[:, 0], path[:, 1]
    dt = float(cfg.delta_t)
    targets, actions, states, cells = [], [], [], []
    cost, feasible, wrap_arg = f32(0), False, 0.0
    umin, umax = np.float32(cfg.u_min), np.float32(cfg.u_max)
    for t in range(cfg.max_seqs):
        # pure pursuit in float64
        dx, dy = px - f64(x), py - f64(y)
        ang = np.arctan2(dy, dx) - f64(th) if nudge is None else (np.arctan2(dy, dx) + f64(nudge[1])) - f64(th)
        valid = (np.abs(ang) < PI / 2) & ((dx * dx + dy * dy) > LOOKAHEAD2)
        k = int(np.argmax(valid)) if valid.any() else len(px) - 1
        tx, ty = float(dx[k]), float(dy[k])
        e_lin = f64(math.sqrt(tx * tx + ty * ty))
        bearing = math.atan2(ty, tx)
        if nudge is not None:
            e_lin, bearing = f64(e_lin * (1.0 + nudge[0])), bearing + nudge[1]
        wrap_arg = float(bearing - float(th)) + PI
        e_ang = f64(pymod(wrap_arg, TWO_PI) - PI)
        lin_i = f32(f64(lin_i) + e_lin * dt)
        ang_i = f32(f64(ang_i) + e_ang * dt)
        v, om = f32(e_lin), f32(e_ang)
        targets.append(k)
        actions.append((v, om))
        # transit in float32 (robot_model.py:75-94), slot t left un-clamped and un-wrapped
        tv, c0 = trav(cfg, x, y)
        vc, oc = min(max(v, umin[0]), umax[0]), min(max(om, umin[1]), umax[1])
        sn, cs = sincos_spec(th)
        g = f32(tv * vc)
        xn = f32(x + f32(f32(g * cs) * TRANSIT_DT))
        yn = f32(y + f32(f32(g * sn) * TRANSIT_DT))
        tn = f32(th + f32(f32(tv * oc) * TRANSIT_DT))
        states.append((xn, yn, tn))
        x = min(max(xn, f32(cfg.x0)), f32(cfg.x0 + cfg.G * cfg.res))
        y = min(max(yn, f32(cfg.y0)), f32(cfg.y0 + cfg.G * cfg.res))
        th = wrap32(tn)
        sc, c1 = point_cost(cfg, xn, yn)
        cost = f32(cost + sc)
        cells += [c0, c1]
        ex, ey = float(px[-1]) - float(x), float(py[-1]) - float(y)
        if math.sqrt(ex * ex + ey * ey) < 1:
            feasible = True
            break
    tc, c2 = point_cost(cfg, x, y)
    cost = f32(cost + tc)
    cells.append(c2)
    states.append((x, y, th))
    return Steer(path, word, np.asarray(targets, np.int32), np.asarray(actions, np.float32).reshape(-1, 2), np.asarray(states, np.float32),
                 cells, cost, feasible, len(actions), np.array([e_lin, lin_i, e_ang, ang_i], np.float64), np.array([lin_i, ang_i], np.float32), wrap_arg)


def steer(cfg: Config, from_state, ctrl, target, m=M32) -> Steer:
    path, w = reference_path(from_state, target, cfg.delta, m)
    return follow(cfg, from_state, ctrl, path, w)


def steer_is_marginal(cfg: Config, from_state, ctrl, target, eps: float = EPS_POINT, m=M32) -> bool:
    """A discrete decision of this steer hangs on less than the device's measured point difference: the two shortest words are
    within 8 float32 ulps of each other, the point count hangs on the last bits of the total, or the follow loop on the points
    moved by +-eps changes a target index, the termination step, feasibility or a traversability cell."""
    opts = all_options(from_state, target, m)
    lens = sorted(float(o[0]) for o in opts)
    if lens[1] - lens[0] <= 8 * float(np.spacing(f32(lens[0]))):
        return True
    path, w = reference_path(from_state, target, cfg.delta, m)
    q = lens[0] / SPACING
    if len(path) - 1 >= math.floor(q) and min(q - math.floor(q), math.ceil(q) - q) < 1e-5:
        return True
    base = follow(cfg, from_state, ctrl, path, w)
    for sx, sy in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        alt = follow(cfg, from_state, ctrl, path + np.array([sx * eps, sy * eps]), w)
        if alt.length != base.length or alt.feasible != base.feasible or not np.array_equal(alt.targets, base.targets) or alt.cells != base.cells:
            return True
    return False


# ---- the tree --------------------------------------------------------------------------------------------------------------------
@dataclass
class SpecTree:
    nodes: np.ndarray                # (n, 3) float32
    edges: np.ndarray                # (n,) int32
    costs: np.ndarray                # (n,) float32
    seq_lengths: np.ndarray          # (n,) int32
    controllers_states: np.ndarray   # (n, 4) float32
    action_seqs: list                # per node (L, 2)
    state_seqs: list                 # per node (L + 1, 3)
    near: np.ndarray                 # (iters,) nearest index per iteration
    feasible: np.ndarray             # (iters,) bool
    steers: list
    pick: int = -1
    actions: Optional[np.ndarray] = None
    states: Optional[np.ndarray] = None


def nearest(nodes, sx, sy):
    """rule 5 of DESIGN.md 4.6 on nodes[:, :2]: the fused norm, the lowest index among equal distances."""
    from rrt_spec import norm
    return int(np.argmin(norm(nodes[:, 0] - f32(sx), nodes[:, 1] - f32(sy))))


def grow(cfg: Config, start, samples) -> SpecTree:
    nodes, edges, costs = [np.asarray(start, np.float32)], [-1], [f32(0)]
    lens, ctrls, aseq, sseq = [0], [np.zeros(4, np.float32)], [np.zeros((0, 2), np.float32)], [np.zeros((0, 3), np.float32)]
    near, feas, steers = [], [], []
    for smp in np.asarray(samples, np.float32):
        arr = np.asarray(nodes, np.float32)
        p = nearest(arr, smp[0], smp[1])
        st = steer(cfg, arr[p], ctrls[p], smp)
        if p != 0:
            ctrls[p][1], ctrls[p][3] = st.integrals               # the aliased integrals, feasible or not
        near.append(p); feas.append(st.feasible); steers.append(st)
        if not st.feasible:
            continue
        nodes.append(st.states[-1]); edges.append(p); costs.append(f32(costs[p] + st.cost)); lens.append(st.length)
        ctrls.append(st.ctrl.astype(np.float32)); aseq.append(st.actions); sseq.append(st.states)
    return SpecTree(np.asarray(nodes, np.float32), np.asarray(edges, np.int32), np.asarray(costs, np.float32), np.asarray(lens, np.int32),
                    np.asarray(ctrls, np.float32), aseq, sseq, np.asarray(near, np.int32), np.asarray(feas, bool), steers)


def pick_and_path(tree: SpecTree, goal, threshold: float = 1.0) -> SpecTree:
    """rule 8 of DESIGN.md 4.6 (lowest cost, then lowest index among the nodes within the threshold of the goal), then the
    segments from the root, each later one without its first state."""
    from rrt_spec import norm
    g = np.asarray(goal, np.float32)
    near = np.nonzero(norm(tree.nodes[:, 0] - g[0], tree.nodes[:, 1] - g[1]) < f32(threshold))[0]
    if near.size == 0:
        return tree
    tree.pick = int(near[np.argmin(tree.costs[near])])
    idx = [tree.pick]
    while idx[-1] != 0:
        idx.append(int(tree.edges[idx[-1]]))
    chain = idx[::-1][1:]
    if not chain:
        # the reference's torch.cat of nothing raises here (the start within the threshold of the goal and no cheaper node)
        tree.actions, tree.states = np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32)
        return tree
    tree.actions = np.concatenate([tree.action_seqs[i] for i in chain])
    # the walk starts at the picked node, whose segment is taken whole; every segment before it loses its first state
    tree.states = np.concatenate([tree.state_seqs[i][1:] for i in chain[:-1]] + [tree.state_seqs[chain[-1]]])
    return tree
