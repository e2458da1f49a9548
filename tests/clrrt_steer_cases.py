"""The steer table of test_clrrt_steer_table.py (CPU) and test_gpu_clrrt_steer.py (GPU): about 600 seeded, deterministic steers that
hold `clrrt_steer` (csrc/clrrt_kernels.hip) to tests/clrrt_spec.py evaluated with the device's own float32 math (`M64R`), plus the
comparison functions both files share.  A group is one planner configuration; it is run as one steer_batch per 64 cases (the
boundaries groups hold 70).

Maps (G = 64, resolution 0.5, stuck threshold 0.2, goal (24, 24)): A = plan 0's `mean` of tests/golden/clrrt.npz; B = synthetic:
uniform risk in [0, 0.6], a four-row stripe at 0.95 (y in [20, 22): +1e4 per step, the rover creeps), a block at 1.0 and above
(x in [20, 24), y in [4, 8): traversability 0, the rover does not move) and a few cells below 0 and above 1 for the clamp.

Groups:
  random_0 .. random_3   4 x 64, map A, delta 5, max_seqs 250: start uniform in [1, 31]^2, heading in [-pi, pi]; target at a distance
                         from {0.3, 1, 2, 3, 4, 6, 18} in a random direction, clipped to the map, heading in [0, 2 pi); integrals
                         random and non-zero.  All six words, most steers feasible (asserted in the CPU test).
  boundaries_d5 / _d12   placed, map A: the cases of `_boundary_base`, each at orientation 0 and rotated by 0.7 rad about the map's
                         centre (a tie on the axes stays a tie only where the arithmetic is symmetric).  Expected words and point
                         counts stand as literals in BOUNDARY_EXPECT, produced once by the spec.
  long_d12               delta 12, the largest the handle accepts: 16 steers whose shortest word is RLR / LRL (all-arc paths, run to
                         their end; in 20000 draws of the recipe no CCC word was the shortest beyond 9.2 m) and 16 with totals
                         >= 16 m from the straight words, where the point count hits the 64 cap.
  short_d02 / _d025 / _d05   delta 0.2 (the truncated path is the start point alone), 0.25 and 0.5.
  maxseqs_*              eight random feasible steers of spec lengths L0 .. L7, all eight at max_seqs = Li (steer i feasible on the
                         last permitted step) and Li - 1 (not feasible), and at max_seqs = 1.
  edges_B                map B: starts within one step of each limit heading outward (the clean state clamps, slot t keeps the
                         un-clamped one), starts on the stripe, starts inside the traversability-0 block (max_seqs steps, infeasible,
                         every state equal), targets beyond the stripe, starts on the cells outside [0, 1], and random ones.

Straight-ahead cases start at x = f32(7.9) rather than on a dyadic coordinate: with a dyadic start the float32 total is an exact
multiple of 0.25 and the cumulative length lands on delta itself, which the table test counts as truncation-marginal for all of them
(more than the cap); from f32(7.9) every x + d is rounded and none is.  The y coordinate stays dyadic, so LSL and RSR still tie.  The
one truncation-marginal case of each boundaries group is the same pose at heading 0, whose total is 0 (0 / 0.25 is an integer).
No case of the table sits in the double-rounding band; none had to be replaced.

Two things the placed cases brought out, both the reference's own behaviour and equal on the device: "RLR centre distance 4" picks
RSL with a straight part of length 0 between its arcs, and the one point that falls on it is 0 / 0 (the comparisons match the NaN
masks); and a straight path ahead of the rover makes the angular error cancel to (nearly) nothing, where the +-2^-48 nudge of the
bearing is visible in the float32 action by construction (`aligned`): 14 of the 70 boundary cases are cast-sensitive for that reason
and no other case of the table is.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

import clrrt_cases as Cs
import clrrt_spec as S

f32 = np.float32
G, RES, THR, GOAL = 64, 0.5, 0.2, (24.0, 24.0)
PI32, HALF_PI32, TWO_PI32 = S.PI32, S.HALF_PI32, S.TWO_PI32
DISTANCES = (0.3, 1.0, 2.0, 3.0, 4.0, 6.0, 18.0)
ORIENTATION = 0.7                    # the non-axis-aligned orientation of the boundary cases, radians about the map's centre
CAP = 0.02                           # share of a group that may be left out (the cap tests/test_gpu_clrrt.py uses)
POINT_BOUND_ULPS = 4                 # see test_gpu_clrrt_steer.py: 4 x the measured 1 ulp
NUDGES = tuple((a * 2.0 ** -48, b * 2.0 ** -48) for a in (1, -1) for b in (1, -1))


@dataclass
class Group:
    name: str
    map: str                         # "A" or "B"
    delta: float
    max_seqs: int
    from_states: np.ndarray          # (n, 3) float32
    ctrls: np.ndarray                # (n, 4) float32: previous error and integral, linear then angular
    targets: np.ndarray              # (n, 3) float32
    expect: Optional[list] = None    # per case (word, points), literals

    def __len__(self):
        return len(self.from_states)


# ---- maps ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def risk_map(which):
    if which == "A":
        return Cs.fixture()["p0_mean"].astype(np.float32)
    rng = np.random.default_rng(20240607)
    m = rng.uniform(0.0, 0.6, (G, G)).astype(np.float32)
    m[40:44, :] = 0.95                                           # rows iy 40 .. 43: y in [20, 22)
    m[8:16, 40:48] = 1.0                                         # iy 8 .. 15, ix 40 .. 47: x in [20, 24), y in [4, 8)
    m[10:12, 42:46] = 1.3
    m[52:56, 8:12] = np.float32([[-0.2, -0.05, 1.05, 1.5]] * 4)  # x in [4, 6), y in [26, 28): clamped to 0 and 1
    return m


def config(g: Group) -> S.Config:
    return S.Config(mean=risk_map(g.map), res=RES, thr=THR, goal=f32(GOAL), delta_t=0.1, max_seqs=g.max_seqs, delta=g.delta)


def planner(g: Group, **kw):
    """benchnav_amd.CLRRT with the group's configuration on reference-shaped stand-ins."""
    import torch
    from benchnav_amd import CLRRT
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    gm = FakeGridMap(G, RES)
    args = dict(delta_t=0.1, max_iterations=1, delta_distance=g.delta, max_seqs=g.max_seqs)
    args.update(kw)
    return CLRRT(3, 2, FakeDynamics(risk_map(g.map), gm), FakeObjectives(torch.tensor(GOAL), THR), gm, **args)


# ---- the recipes -----------------------------------------------------------------------------------------------------------------
def _random(rng, n, distances=DISTANCES):
    fs, ct, tg = np.empty((n, 3), f32), np.empty((n, 4), f32), np.empty((n, 3), f32)
    for i in range(n):
        x, y, th = rng.uniform(1, 31), rng.uniform(1, 31), rng.uniform(-math.pi, math.pi)
        d, a = distances[int(rng.integers(len(distances)))], rng.uniform(0, 2 * math.pi)
        fs[i] = (x, y, th)
        tg[i] = (min(max(x + d * math.cos(a), 0.25), 31.75), min(max(y + d * math.sin(a), 0.25), 31.75), rng.uniform(0, 2 * math.pi))
        sg = rng.choice([-1.0, 1.0], 2)
        ct[i] = (rng.uniform(0, 5), sg[0] * rng.uniform(0.1, 20), rng.uniform(-math.pi, math.pi), sg[1] * rng.uniform(0.1, 5))
    return fs, ct, tg


def _filtered(rng, n, keep, distances):
    """The first n draws of the random recipe that `keep(spec word, float32 total)` accepts."""
    fs, ct, tg = [], [], []
    while len(fs) < n:
        f, c, t = _random(rng, 1, distances)
        opts = S.all_options(f[0], t[0], S.M64R)
        w = S.choose_word(opts)
        if keep(w, float(opts[w][0])):
            fs.append(f[0]); ct.append(c[0]); tg.append(t[0])
    return np.array(fs, f32), np.array(ct, f32), np.array(tg, f32)


STRAIGHT_X = f32(7.9)                # an odd last bit just below 8: x + d is rounded for every d below (module docstring)
STRAIGHT_D = (0.25, 0.5, 1.0, 2.0, 5.0, 20.0)


def _boundary_base():
    """(name, start, target) at orientation 0."""
    two, four, twopi = f32(2), f32(4), TWO_PI32
    down, up = (lambda v: np.nextafter(f32(v), f32(-np.inf))), (lambda v: np.nextafter(f32(v), f32(np.inf)))
    P = (12.0, 14.0)
    out = [("same pose", (*P, 0.5), (*P, 0.5)),                               # LSL: a full circle of length 2 pi, atan2(0, 0)
           ("same pose, heading 0", (*P, 0.0), (*P, 0.0)),                    # ... and of length 0: the end point alone
           ("same position, heading + pi", (*P, 0.0), (*P, PI32))]
    out += [(f"straight ahead {d}", (STRAIGHT_X, 14.0, 0.0), (f32(STRAIGHT_X + f32(d)), 14.0, 0.0)) for d in STRAIGHT_D]
    # heading 0 both: the right start centre (12, 13) and the left end centre (ex, 13): half their distance is (ex - 12) / 2
    out += [(f"RSL half distance {n}", (*P, 0.0), (ex, 12.0, 0.0)) for n, ex in (("below 1", down(14)), ("1", f32(14)), ("above 1", up(14)))]
    out += [(f"LSR half distance {n}", (*P, 0.0), (ex, 16.0, 0.0)) for n, ex in (("below 1", down(14)), ("1", f32(14)), ("above 1", up(14)))]
    # LRL: start (1, 14) heading pi / 2, left centre (0, 14); target heading 3 pi / 2 at x = d - 1, left centre (d, 14): the centre
    # distance is d itself, representable one ulp either side of 2 and of 4.  RLR: the mirror image, headings -pi / 2 and pi / 2
    for word, hs, he in (("LRL", HALF_PI32, f32(1.5 * math.pi)), ("RLR", -HALF_PI32, HALF_PI32)):
        for n, d in (("below 2", down(two)), ("2", two), ("above 2", up(two)), ("below 4", down(four)), ("4", four), ("above 4", up(four))):
            out.append((f"{word} centre distance {n}", (1.0, 14.0, hs), (f32(d - f32(1)), 14.0, he)))
    out.append(("collinear behind", (*P, 0.0), (9.0, 14.0, 0.0)))
    out += [(f"target heading {n}", (*P, 0.0), (15.0, 16.0, h)) for n, h in (("0", 0.0), ("pi/2", HALF_PI32), ("pi", PI32),
                                                                              ("3pi/2", f32(1.5 * math.pi)), ("below 2pi", down(twopi)))]
    out += [("start heading pi", (*P, PI32), (15.0, 16.0, 1.0)), ("start heading -pi", (*P, -PI32), (15.0, 16.0, 1.0))]
    return out


def _rotated(pose, phi):
    if phi == 0.0:
        return f32(pose)
    x, y, th = (float(v) for v in pose)
    c, s = math.cos(phi), math.sin(phi)
    return f32([16 + c * (x - 16) - s * (y - 16), 16 + s * (x - 16) + c * (y - 16), th + phi])


def boundary_names():
    return [f"{n} @ {phi}" for phi in (0.0, ORIENTATION) for n, _, _ in _boundary_base()]


# (word, points of the truncated path) per case of boundary_names(), by clrrt_spec with M64R; test_clrrt_steer_table.py holds the
# spec to them.  Straight ahead gives LSL -- but at 2 m, where RSL comes to 1.9999999 against LSL's 2.0 (checked there as well).
BOUNDARY_EXPECT = {
    "boundaries_d5": [(0, 21), (0, 1), (4, 21), (0, 2), (0, 3), (0, 5), (0, 9), (0, 21), (0, 21), (0, 21), (2, 14), (2, 14),
        (0, 21), (3, 14), (3, 14), (4, 21), (4, 21), (5, 21), (5, 14), (2, 14), (1, 14), (5, 21), (4, 21), (4, 21), (4, 14),
        (2, 14), (0, 14), (0, 21), (3, 16), (0, 17), (2, 21), (3, 21), (3, 16), (2, 21), (2, 21), (0, 21), (0, 21), (0, 21),
        (3, 2), (3, 3), (3, 5), (3, 9), (3, 21), (3, 21), (0, 21), (0, 21), (2, 14), (0, 21), (3, 14), (3, 14), (0, 21), (0,
        21), (5, 21), (5, 14), (1, 14), (1, 14), (0, 21), (0, 21), (0, 21), (0, 14), (0, 14), (0, 14), (0, 21), (3, 16), (0,
        17), (0, 21), (3, 21), (3, 16), (2, 21), (2, 21)],
    "boundaries_d12": [(0, 27), (0, 1), (4, 31), (0, 2), (0, 3), (0, 5), (0, 9), (0, 21), (0, 49), (0, 38), (2, 14), (2,
        14), (0, 38), (3, 14), (3, 14), (4, 31), (4, 31), (5, 31), (5, 14), (2, 14), (1, 14), (5, 31), (4, 31), (4, 31), (4,
        14), (2, 14), (0, 14), (0, 39), (3, 16), (0, 17), (2, 26), (3, 24), (3, 16), (2, 27), (2, 27), (0, 27), (0, 27), (0,
        47), (3, 2), (3, 3), (3, 5), (3, 9), (3, 21), (3, 48), (0, 38), (0, 38), (2, 14), (0, 38), (3, 14), (3, 14), (0,
        47), (0, 47), (5, 31), (5, 14), (1, 14), (1, 14), (0, 47), (0, 47), (0, 47), (0, 14), (0, 14), (0, 14), (0, 39), (3,
        16), (0, 17), (0, 26), (3, 24), (3, 16), (2, 27), (2, 27)],
}


def _boundaries(delta):
    base = _boundary_base()
    fs = np.array([_rotated(s, phi) for phi in (0.0, ORIENTATION) for _, s, _ in base], f32)
    tg = np.array([_rotated(t, phi) for phi in (0.0, ORIENTATION) for _, _, t in base], f32)
    ct = np.zeros((len(fs), 4), f32)
    ct[::3] = f32([0.4, 12.5, -0.1, 3.25])
    name = f"boundaries_d{delta}"
    return Group(name, "A", float(delta), 250, fs, ct, tg, BOUNDARY_EXPECT[name])


def _edges():
    fs, tg = [], []
    for s in ((31.99, 10.0, 0.0), (0.01, 10.0, PI32), (10.0, 31.99, HALF_PI32), (10.0, 0.01, -HALF_PI32)):          # one step from a limit
        for t in ((16.0, 14.0, 2.0), (14.0, 20.0, 4.0)):
            fs.append(s); tg.append(t)
    for s, t in (((5.0, 21.0, 0.0), (9.0, 21.5, 0.3)), ((15.0, 20.5, 1.0), (15.5, 24.0, 1.5)), ((25.0, 21.5, -2.0), (23.0, 18.0, 4.0)),
                 ((12.0, 21.9, -1.5), (12.0, 18.5, 4.7))):                                                          # on the stripe
        fs.append(s); tg.append(t)
    for t in ((26.0, 7.0, 0.0), (25.0, 3.0, 1.0), (18.0, 2.0, 3.5)):                                                # inside the block
        fs.append((22.0, 6.0, 0.0)); tg.append(t)
    for s, t in (((10.3, 17.0, 1.5), (10.3, 25.1, HALF_PI32)), ((20.0, 18.5, 1.0), (22.0, 24.0, 1.2)), ((6.0, 24.0, -1.6), (6.5, 18.0, 4.7)),
                 ((28.0, 19.0, 2.0), (26.0, 23.5, 2.2))):                                                           # beyond the stripe
        fs.append(s); tg.append(t)
    for s, t in (((4.2, 26.5, 0.0), (5.9, 27.5, 0.5)), ((5.9, 27.9, PI32), (3.0, 26.2, 3.0)), ((5.2, 25.5, 1.5), (5.3, 28.5, 1.6))):   # the clamped cells
        fs.append(s); tg.append(t)
    fs, tg = np.array(fs, f32), np.array(tg, f32)
    ct = np.zeros((len(fs), 4), f32)
    ct[1::2] = f32([0.2, -3.5, 0.3, 0.75])
    r = _random(np.random.default_rng(77), 10)
    return Group("edges_B", "B", 5.0, 250, np.concatenate([fs, r[0]]), np.concatenate([ct, r[1]]), np.concatenate([tg, r[2]]))


@functools.lru_cache(maxsize=None)
def groups():
    out = []
    rng = np.random.default_rng(8)
    for k in range(4):
        out.append(Group(f"random_{k}", "A", 5.0, 250, *_random(rng, 64)))
    out += [_boundaries(5), _boundaries(12)]
    rng = np.random.default_rng(12)
    ccc = _filtered(rng, 16, lambda w, total: w >= 4, (1.0, 2.0, 3.0))
    far = _filtered(rng, 16, lambda w, total: total >= 16.0, (16.0, 18.0, 22.0))
    out.append(Group("long_d12", "A", 12.0, 250, *(np.concatenate([a, b]) for a, b in zip(ccc, far))))
    for name, delta, seed in (("short_d02", 0.2, 2), ("short_d025", 0.25, 25), ("short_d05", 0.5, 50)):
        out.append(Group(name, "A", delta, 250, *_random(np.random.default_rng(seed), 16)))
    # eight feasible steers of at least two steps, and their spec lengths
    cfg = S.Config(mean=risk_map("A"), res=RES, thr=THR, goal=f32(GOAL))
    rng = np.random.default_rng(88)
    fs, ct, tg, lens = [], [], [], []
    while len(fs) < 8:
        f, c, t = _random(rng, 1)
        st = S.steer(cfg, f[0], c[0], t[0], S.M64R)
        if st.feasible and st.length >= 2 and st.length not in lens:
            fs.append(f[0]); ct.append(c[0]); tg.append(t[0]); lens.append(st.length)
    fs, ct, tg = np.array(fs, f32), np.array(ct, f32), np.array(tg, f32)
    for i, L in enumerate(lens):
        out.append(Group(f"maxseqs_{i}_at_{L}", "A", 5.0, L, fs, ct, tg))
        out.append(Group(f"maxseqs_{i}_below_{L}", "A", 5.0, L - 1, fs, ct, tg))
    out.append(Group("maxseqs_1", "A", 5.0, 1, fs, ct, tg))
    out.append(_edges())
    return {g.name: g for g in out}


def group_names():
    return list(groups())


# ---- the spec's results ----------------------------------------------------------------------------------------------------------
@dataclass
class SpecCase:
    steer: S.Steer                   # the whole steer under M64R
    total: float                     # the chosen word's float32 total
    band: bool                       # a transcendental's float64 result lies within 2^-44 of a float32 rounding boundary
    truncation_marginal: bool


def _truncation_marginal(path, pts, whole, total, delta):
    """The cumulative length comes within 1e-12 of delta at or before the cut, or the path runs to its end (the point count then
    is ceil(total / 0.25) + 1) and total / 0.25 lies within 1e-9 of an integer."""
    d = pts[1:] - pts[:-1]
    seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    acc = 0.0
    for v in seg[:len(path)]:                                   # up to and including the segment that made the cut
        acc = acc + float(v)
        if abs(acc - delta) <= 1e-12:
            return True
    if whole and len(path) == len(pts):
        q = total / S.SPACING
        return abs(q - round(q)) < 1e-9
    return False


def _spec_case(g, cfg, f, c, t):
    m, margins = S.instrumented_m64r()
    limit = int(math.ceil(g.delta / 0.2)) + 2
    pts, w = S.dubins_points(f, t, m, limit)
    path = S.truncate(pts, g.delta)
    assert len(path) < limit or len(pts) < limit
    opt = S.all_options(f, t, S.M64R)[w][1]
    total = float(f32(f32(abs(opt[1]) + abs(opt[0])) + abs(opt[2])))
    whole = int(math.ceil(total / S.SPACING)) < limit                # the end point was generated
    st = S.follow(cfg, f, c, path, w)
    return SpecCase(st, total, min(margins) < S.DOUBLE_ROUNDING_BAND, _truncation_marginal(path, pts, whole, total, g.delta))


@functools.lru_cache(maxsize=None)
def spec(name):
    """Per case of the group: SpecCase."""
    g = groups()[name]
    cfg = config(g)
    out = []
    for f, c, t in zip(g.from_states, g.ctrls, g.targets):
        with np.errstate(invalid="ignore"):                          # "RLR centre distance 4": see point_difference
            out.append(_spec_case(g, cfg, f, c, t))
    return out


def steers_differ(a: S.Steer, b: S.Steer) -> bool:
    """A target index, the length, feasibility, a cell, or any bit of actions, states, cost or integrals."""
    return (a.length != b.length or a.feasible != b.feasible or not np.array_equal(a.targets, b.targets) or a.cells != b.cells
            or a.actions.tobytes() != b.actions.tobytes() or a.states.tobytes() != b.states.tobytes()
            or f32(a.cost).tobytes() != f32(b.cost).tobytes() or a.integrals.tobytes() != b.integrals.tobytes())


@functools.lru_cache(maxsize=None)
def cast_sensitive(name, i):
    """A follow on the case's own spec path with the bearing and the linear error nudged by +-2^-48 changes something."""
    g = groups()[name]
    cfg, base = config(g), spec(name)[i].steer
    return any(steers_differ(base, S.follow(cfg, g.from_states[i], g.ctrls[i], base.path, base.word, nudge=n)) for n in NUDGES)


ALIGNED = 2.0 ** -20


@functools.lru_cache(maxsize=None)
def aligned(name, i):
    """0: every angular error of the spec's follow is at least 2^-20 in magnitude.  Below that the bearing of the target cancels
    against the heading (a straight path ahead of the rover), and a 2^-48 nudge of the bearing moves the float32 cast of the
    error with a probability of 1 / 16 per step and more: such a case is cast-sensitive by construction, not by accident.
    2: every error below 2^-20 is an exact zero (the bearing is atan2(0, positive)): no float64 library has a freedom there.
    1: the others."""
    om = np.abs(spec(name)[i].steer.actions[:, 1].astype(np.float64))
    small = om[om < ALIGNED]
    return 0 if small.size == 0 else (2 if not small.any() else 1)


# ---- what steer_batch returns, and the comparisons ---------------------------------------------------------------------------------
def as_device(steers, max_seqs):
    """The spec's steers laid out as CLRRT.steer_batch lays out the device's (NumPy arrays): NaN beyond a path, rows beyond a
    length left at zero here (the device leaves them as they were)."""
    n = len(steers)
    out = dict(path=np.full((n, 64, 2), np.nan), points=np.zeros(n, np.int32), word=np.zeros(n, np.int32), targets=np.zeros((n, max_seqs), np.int32),
               actions=np.zeros((n, max_seqs, 2), f32), states=np.zeros((n, max_seqs + 1, 3), f32), feasible=np.zeros(n, bool),
               length=np.zeros(n, np.int32), cost=np.zeros(n, f32), controllers=np.zeros((n, 4)))
    for i, st in enumerate(steers):
        L = st.length
        out["path"][i, :len(st.path)] = st.path
        out["points"][i], out["word"][i], out["length"][i], out["feasible"][i], out["cost"][i] = len(st.path), st.word, L, st.feasible, st.cost
        out["targets"][i, :L], out["actions"][i, :L], out["states"][i, :L + 1], out["controllers"][i] = st.targets, st.actions, st.states, st.ctrl
    return out


def point_difference(dev, i, want: S.Steer):
    """(ulps, metres) of the device's path of case i against the spec's, point counts being equal."""
    n = len(want.path)
    got, fin = dev["path"][i, :n], np.isfinite(want.path)
    assert np.array_equal(np.isfinite(got), fin), i          # a zero-length straight between two arcs makes its one point 0 / 0, on both sides
    return Cs.ulps64(got[fin], want.path[fin]), float(np.abs(got[fin] - want.path[fin]).max(initial=0.0))


def check_dubins(dev, i, case: SpecCase, bound_ulps=POINT_BOUND_ULPS):
    """(a) of test_gpu_clrrt_steer.py for one case; returns point_difference, or None where the counts differ on a
    truncation-marginal case."""
    want, n = case.steer, int(dev["points"][i])
    if not case.truncation_marginal:
        assert int(dev["word"][i]) == want.word, (i, int(dev["word"][i]), want.word)
        assert n == len(want.path), (i, n, len(want.path))
    assert 1 <= n <= 64 and np.isnan(dev["path"][i, n:]).all(), i
    if n != len(want.path):
        return None
    ulps, metres = point_difference(dev, i, want)
    assert ulps <= bound_ulps, (i, ulps, metres)
    return ulps, metres


def follow_on_device_points(cfg, g: Group, dev, i) -> S.Steer:
    n = int(dev["points"][i])
    return S.follow(cfg, g.from_states[i], g.ctrls[i], dev["path"][i, :n].copy(), int(dev["word"][i]))


def controller_error_ulps(ctrl, want: S.Steer) -> float:
    """The float64 errors of the last step against the spec's, each in its own rounding unit: the linear error sqrt(d2) in ulps
    of itself; the angular error ((bearing - heading) + pi) mod 2 pi - pi in ulps of its largest intermediate, the argument of the
    modulo, which reaches 3 pi -- one ulp of a bearing near pi becomes one ulp of a number in [8, 16) there, four times as large,
    whatever the error that is left after the wrap."""
    lin = abs(float(ctrl[0]) - float(want.ctrl[0])) / float(np.spacing(abs(float(want.ctrl[0]))))
    ang = abs(float(ctrl[2]) - float(want.ctrl[2])) / float(np.spacing(max(abs(want.wrap_arg), abs(float(want.ctrl[2])))))
    return max(lin, ang)


def follow_mismatch(dev, i, want: S.Steer):
    """(b) of test_gpu_clrrt_steer.py for one case: None where the device's follow half equals `want` (the spec's follow on the
    device's own points) -- target indices, length, feasibility; actions, states, cost and the float32 integrals bit for bit; the
    float64 errors within 4 ulps (controller_error_ulps) -- else the first differing quantity and step."""
    L = int(dev["length"][i])
    if L != want.length or bool(dev["feasible"][i]) != want.feasible:
        return f"length / feasible {L} {bool(dev['feasible'][i])} against {want.length} {want.feasible}"
    for name, got, ref in (("target", dev["targets"][i, :L], want.targets), ("action", dev["actions"][i, :L].view(np.uint32), want.actions.view(np.uint32)),
                           ("state", dev["states"][i, :L + 1].view(np.uint32), want.states.view(np.uint32))):
        if not np.array_equal(got, ref):
            t = int(np.nonzero((got != ref).reshape(len(ref), -1).any(1))[0][0])
            return f"{name} at step {t}: {got[t].tolist()} against {ref[t].tolist()}"
    if f32(dev["cost"][i]).tobytes() != f32(want.cost).tobytes():
        return f"cost {dev['cost'][i]!r} against {want.cost!r}"
    ctrl = dev["controllers"][i]
    if f32(ctrl[[1, 3]]).tobytes() != want.integrals.tobytes() or not np.array_equal(ctrl[[1, 3]], want.integrals.astype(np.float64)):
        return f"integrals {ctrl[[1, 3]].tolist()} against {want.integrals.tolist()}"
    err = controller_error_ulps(ctrl, want)
    if err > 4:
        return f"controller errors {err} ulps"
    return None


def loose_follow_ok(dev, i, want: S.Steer, cost_rel=1e-6):
    """The bounds of tests/test_gpu_clrrt.py (TOL_TRAJ, COST_REL) on the follow half: what a cast-sensitive case still has to meet."""
    L = int(dev["length"][i])
    if L != want.length or bool(dev["feasible"][i]) != want.feasible or not np.array_equal(dev["targets"][i, :L], want.targets):
        return False
    return (np.abs(dev["actions"][i, :L] - want.actions).max(initial=0) <= Cs.TOL_TRAJ and np.abs(dev["states"][i, :L + 1] - want.states).max() <= Cs.TOL_TRAJ
            and abs(float(dev["cost"][i]) - float(want.cost)) <= cost_rel * max(abs(float(want.cost)), 1.0))
