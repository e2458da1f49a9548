"""Inputs of tests/test_gpu_dwa_subgoal.py (DWA.forward's window and sub-goal pick on synthetic float paths, against the oracle),
built without a device so that tests/test_astar_dwa_oracle.py can check on the CPU that none of them hangs on the last bits of
atan2f (astar_dwa_oracle.DELTA) and how many fuzz seeds are redrawn.

A configuration is a dict: geo (G, res, x_limits or None), lds (the planner's LDS map window), bounds (u_min, u_max), nv, nw,
states (B, 3), prev (B, 2), path (P, 2) or None, look; `expect`, where present, is the index the pick must have."""
import numpy as np

import astar_dwa_oracle as L
from oracle import oracle as O

T, THR = 20, 0.2
A_LIM, DWA_DT = (0.5, 0.5), 0.1
GEOS = ((64, 0.5, None), (64, 0.5, (-8.0, 24.0)), (50, 0.3, None))
WIDE, NARROW = ((0.0, -1.0), (1.0, 1.0)), ((0.3, -0.02), (0.36, 0.02))      # NARROW cuts the window on both sides of both axes
LENGTHS = (1, 2, 255, 256, 257, 513, 2000)
SHAPES = ((1, 1), (1, 9), (9, 1), (7, 13), (32, 32))
FUZZ_SEEDS = tuple(range(500, 524))
REDRAW = 1000                                                               # a flagged seed s is redrawn from s + REDRAW


def risk_map(G):
    return (0.1 + 0.85 * np.random.default_rng(G).random((G, G))).astype(np.float32)


def goal_of(geo):
    G, res, xl = geo
    x0 = 0.0 if xl is None else xl[0]
    return np.float32([x0 + 0.8 * G * res, x0 + 0.7 * G * res])


def params(cfg):
    G, res, xl = cfg["geo"]
    return O.make_params(64, T, G, res, goal_of(cfg["geo"]), thr=THR, u_min=cfg["bounds"][0], u_max=cfg["bounds"][1], x_limits=xl,
                         y_limits=xl)


def config(states, prev, path, geo=GEOS[0], lds=True, bounds=WIDE, nv=10, nw=10, look=1.0, **extra):
    states = np.asarray(states, np.float32).reshape(-1, 3)
    prev = np.ascontiguousarray(np.broadcast_to(np.asarray(prev, np.float32), (len(states), 2)))
    path = None if path is None else np.ascontiguousarray(np.asarray(path, np.float32).reshape(-1, 2))
    return dict(geo=geo, lds=lds, bounds=bounds, nv=nv, nw=nw, states=states, prev=prev, path=path, look=look, **extra)


def slot0(cfg, b):
    """The state the sub-goal rule sees for instance b (candidate 0's aliased slot 0), by the oracle."""
    a0 = L.window(cfg["prev"][b], A_LIM, DWA_DT, cfg["nv"], cfg["nw"], *cfg["bounds"])[0]
    return O.dwa_sub_goal(params(cfg), risk_map(cfg["geo"][0]), cfg["states"][b], a0, cfg["path"], cfg["look"])[1]


def margin(cfg):
    """The smallest bearing margin over the configuration's instances (inf without a path)."""
    if cfg["path"] is None:
        return np.inf
    return min(L.bearing_margin(cfg["path"], slot0(cfg, b), cfg["look"]) for b in range(len(cfg["states"])))


# ---- paths and states -----------------------------------------------------------------------------------------------------------
def float_path(rng, P, centre, step=0.35):
    """A smooth random walk of P float points from near `centre`."""
    head = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.normal(0, 0.25, P))
    pts = np.float32(centre) + rng.uniform(-1, 1, 2) + np.cumsum(np.stack([np.cos(head), np.sin(head)], 1) * step, 0)
    return pts.astype(np.float32)


def cell_path(rng, P, centre, res):
    """8-connected cell centres times the resolution, as _reconstruct_path makes them: many exactly equal distances."""
    moves = np.array([(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)])
    d = (rng.integers(0, 8) + np.cumsum(rng.choice([-1, 0, 0, 0, 1], P))) % 8
    cells = np.round(np.float64(centre) / res).astype(np.int64) + np.cumsum(moves[d], 0)
    return (cells.astype(np.float32) * np.float32(res)).astype(np.float32)


def states_in(rng, geo, B):
    G, res, xl = geo
    x0 = 0.0 if xl is None else xl[0]
    xy = x0 + rng.uniform(0.15, 0.85, (B, 2)) * G * res
    return np.concatenate([xy, rng.uniform(-np.pi, np.pi, (B, 1))], 1).astype(np.float32)


# ---- the hand-made cases ------------------------------------------------------------------------------------------------------------
REST = np.float32([8.0, 8.0, 0.25])        # dyadic; with prev = (0, w) candidate 0 has v = 0 and the slot-0 position is (8, 8) exactly


def _far_fill(rng, P):
    """P points no nearer than 3 to (8, 8): never the nearest once a point at distance < 3 is ahead."""
    ang, rad = rng.uniform(-np.pi, np.pi, P), rng.uniform(3.0, 9.0, P)
    return (np.float32([8.0, 8.0]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)).astype(np.float32)


def length_case(P):
    rng = np.random.default_rng(10_000 + P)
    st = states_in(rng, GEOS[0], 2)
    return config(st, [[0.4, 0.1], [0.0, -0.3]], float_path(rng, P, st[0, :2]))


def tie_cases():
    """(name, cfg): pairs of points mirrored about the rover's x and a duplicate -- float32 distances equal to the bit -- at
    (i, j): different lanes, i in a HIGHER lane than j mod 256, and the same lane a stride apart; both orders of the pair."""
    a, am = np.float32([9.25, 8.5]), np.float32([9.25, 7.5])               # dx = 1.25, dy = +-0.5: both ahead of heading ~0.25
    out = []
    for i, j in ((3, 200), (45, 300), (10, 266)):
        for first, second in ((a, am), (am, a)):
            path = _far_fill(np.random.default_rng(i), 600)
            path[i], path[j], path[j + 40] = first, second, first           # the mirror image later, and a duplicate after that
            out.append((f"{i}_{j}_{'a' if first is a else 'm'}", config(REST, (0.0, 0.3), path, expect=i)))
    return out


def lookahead_cases():
    far = np.float32([[12.0, 8.5]])
    one = np.float32(1.0)
    mk = lambda pts, look, expect: config(REST, (0.0, 0.3), np.concatenate([np.float32(pts).reshape(-1, 2), far]), look=look, expect=expect)
    return [("equal_is_not_ahead", mk([9.0, 8.0], 1.0, 1)),                                    # dist == lookahead
            ("one_ulp_further_is", mk([np.nextafter(np.float32(9.0), np.float32(10.0)), 8.0], 1.0, 0)),
            ("equal_3_4_5", mk([9.5, 10.0], 2.5, 1)),                                        # 1.5^2 + 2^2 = 2.5^2 exactly
            ("one_ulp_further_3_4_5", mk([9.5, np.nextafter(np.float32(10.0), np.float32(11.0))], 2.5, 0)),
            ("lookahead_one_ulp_less", mk([9.0, 8.0], np.nextafter(one, np.float32(0.0)), 0))]


def nothing_ahead_cases():
    rng = np.random.default_rng(7)
    behind = (np.float32([8.0, 8.0]) + np.stack([-rng.uniform(0.5, 6.0, 300), rng.uniform(-1.0, 1.0, 300)], 1)).astype(np.float32)
    within = (np.float32([8.0, 8.0]) + rng.uniform(-0.6, 0.6, (300, 2))).astype(np.float32)
    return [("all_behind", config(REST, (0.0, 0.3), behind, expect=299)), ("all_within", config(REST, (0.0, 0.3), within, expect=299)),
            ("one_point", config(REST, (0.0, 0.3), behind[:1], expect=0))]


def unwrapped_cases():
    """Headings near +-pi: points straight ahead geometrically whose atan2 has the other sign are 2 pi away in the unwrapped
    difference and do not count; the far point whose atan2 has the heading's sign does."""
    out = []
    for th in (3.0, -3.0):
        ray = lambda ang, r: np.float32([8.0, 8.0]) + np.float32(r) * np.float32([np.cos(ang), np.sin(ang)])
        path = np.stack([ray(-th, 1.5), ray(-th * 0.99, 2.0), ray(th * 0.98, 4.0), ray(0.0, 3.0)]).astype(np.float32)
        out.append((f"th{th:+.0f}", config([8.0, 8.0, th], (0.0, 0.0), path, expect=2)))
    return out


def shape_case(nv, nw, kind):
    rng = np.random.default_rng(20_000 + 100 * nv + nw)
    st = states_in(rng, GEOS[0], 2)
    prev, bounds = {"inside": ([0.5, 0.1], WIDE), "one_side": ([0.02, 0.98], WIDE), "both_sides": ([0.33, 0.0], NARROW),
                    "outside": ([1.5, -2.0], WIDE)}[kind]
    return config(st, prev, cell_path(rng, 400, st[1, :2], 0.5), bounds=bounds, nv=nv, nw=nw)


def batch_case():
    rng = np.random.default_rng(31)
    st = states_in(rng, GEOS[0], 5)
    st[:, :2] = st[0, :2] + rng.uniform(-3, 3, (5, 2)).astype(np.float32)
    return config(st, rng.uniform([0, -1], [1, 1], (5, 2)), float_path(rng, 700, st[0, :2]))


def geometry_case(geo, lds):
    rng = np.random.default_rng(40_000 + GEOS.index(geo))
    st = states_in(rng, geo, 2)
    return config(st, [[0.6, -0.2], [0.1, 0.4]], cell_path(rng, 300, st[0, :2], geo[1]), geo=geo, lds=lds)


def fuzz_draw(seed):
    rng = np.random.default_rng(seed)
    geo = GEOS[rng.integers(len(GEOS))]
    B = int(rng.choice([1, 2, 5]))
    nv, nw = SHAPES[rng.integers(len(SHAPES))] if rng.random() < 0.5 else (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
    st = states_in(rng, geo, B)
    P = int(rng.choice(LENGTHS + (64, 700)))
    kind = rng.integers(3)
    path = None if rng.random() < 0.1 else (float_path(rng, P, st[0, :2]) if kind == 0 else cell_path(rng, P, st[0, :2], geo[1]))
    bounds = NARROW if rng.random() < 0.25 else WIDE
    prev = rng.uniform([-0.2, -1.3], [1.2, 1.3], (B, 2))
    if rng.random() < 0.3:
        prev[:, 0] = 0.0                                                    # v = 0: the slot-0 position is the start itself
    return config(st, prev, path, geo=geo, lds=bool(rng.random() < 0.5), bounds=bounds, nv=nv, nw=nw, look=float(rng.choice([0.5, 1.0, 2.0])))


def fuzz_case(seed):
    """(configuration, redrawn): a draw whose bearing margin is within DELTA is redrawn once, from seed + REDRAW -- decided by
    the oracle alone."""
    cfg = fuzz_draw(seed)
    if margin(cfg) > L.DELTA:
        return cfg, False
    return fuzz_draw(seed + REDRAW), True


def all_fixed():
    """Every hand-made configuration, named."""
    out = [(f"length{P}", length_case(P)) for P in LENGTHS]
    out += [("tie" + n, c) for n, c in tie_cases()] + [("look_" + n, c) for n, c in lookahead_cases()]
    out += [("none_" + n, c) for n, c in nothing_ahead_cases()] + [("unwrapped_" + n, c) for n, c in unwrapped_cases()]
    out += [(f"shape{nv}x{nw}_{k}", shape_case(nv, nw, k)) for nv, nw in SHAPES for k in ("inside", "one_side", "both_sides", "outside")]
    out += [("batch", batch_case())] + [(f"geo{GEOS.index(g)}_{int(l)}", geometry_case(g, l)) for g in GEOS for l in (True, False)]
    return out
