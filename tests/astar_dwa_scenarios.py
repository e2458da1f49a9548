"""Scenarios of the A* + DWA closed loop shared by the CPU oracle tests (tests/test_astar_dwa_oracle.py: the free-running cap on
ambiguous steps) and the GPU tests (tests/test_gpu_astar_dwa.py, tests/test_gpu_astar_dwa_oracle.py: the device loop replayed
against the oracle).  Deterministic and seeded; nothing stored.  `case(name)` is the 64 x 64 problem of test_astar_dwa.py in six
variants; `scenario(name)` wraps those and the shapes that reach the fused kernel's other code paths into one description."""
import numpy as np

import astar_maps as M

G, RES, THR, T = 64, 0.5, 0.2, 50
A_LIM, DWA_DT, NV, NW, LOOK = (0.5, 0.5), 0.1, 10, 10, 1.0
CASES = ("smooth", "maze", "low_risk_patch", "disconnected", "edge", "goal_collision")
STRAIGHT = dict(u_min=(0.5, 0.0), u_max=(1.0, 0.0))


def smooth_risk(seed, lo=0.3, hi=0.95, g=G):
    from benchnav_amd import synth
    r = synth.smooth_risk_map(g, seed).numpy()
    return (lo + (hi - lo) * (r - r.min()) / (r.max() - r.min())).astype(np.float32)


def latent(g=G):
    """The environment's latent slip model (mean, std) on a g x g grid."""
    mean = (np.float32(0.2) + np.float32(0.1) * smooth_risk(99, 0.0, 1.0, g)).astype(np.float32)
    return mean, np.full((g, g), 0.05, np.float32)


def case(name):
    """(heights, risk, start (x, y), goal (x, y), planner kwargs) of one scenario on the test_astar_dwa.py problem."""
    h = M.smooth_heights(G, G, 5)
    kw = {}
    if name == "smooth":
        return h, smooth_risk(1), (5.0, 6.0), (26.0, 25.0), kw
    if name == "maze":                         # the serpentine corridor of astar_maps.spiral: paths of ~2000 nodes
        h, risk, thr, res, goal = M.spiral(G)
        return h, risk.astype(np.float32), (0.3, 0.3), ((goal[0] + 0.5) * RES, (goal[1] + 0.5) * RES), kw
    if name == "low_risk_patch":               # risk <= THR is a collision for A*: the patch interior has no path (None).  Driven
        risk = smooth_risk(2)                  # straight at the goal, the rover crosses the patch the path leads round
        yy, xx = np.mgrid[0:G, 0:G]
        risk[(xx - 30) ** 2 + (yy - 30) ** 2 <= 36] = 0.05
        return h, risk, (8.0, 8.0), (26.0, 26.0), dict(STRAIGHT)
    if name == "disconnected":                 # the start's region is walled off from the goal: no path, the goal is the stage goal
        risk = smooth_risk(3)
        risk[:, 20] = 0.05
        risk[:, 21] = 0.05
        return h, risk, (4.0, 16.0), (26.0, 16.0), kw
    if name == "edge":                         # forced straight ahead through the goal into the x = G * res edge: out of bounds
        return h, smooth_risk(4, 0.3, 0.5), (27.0, 16.0), (30.25, 16.25), dict(STRAIGHT)
    if name == "goal_collision":
        risk = smooth_risk(5)
        risk[50, 50] = 0.1
        return h, risk, (5.0, 5.0), (25.25, 25.25), kw
    raise KeyError(name)


# ---- the scenarios of the device-against-oracle replay ------------------------------------------------------------------------
SCENARIOS = tuple(f"case_{c}" for c in CASES) + ("general33", "last_byte_a", "last_byte_b", "origin", "big416", "spiral_1x1",
                                                  "spiral_3x5", "spiral_32x32", "late_fallback")


def _one(heights, risk, start, goal, n, **kw):
    g = risk.shape[-1]
    out = dict(G=g, res=RES, x_limits=None, heights=heights, risks=risk, starts=np.float32([start]), goals=np.float32([goal]),
               n=n, nv=NV, nw=NW, planner={}, latent=latent(g))
    out.update(kw)
    return out


def scenario(name):
    """dict(G, res, x_limits (None: [0, G * res]; y like x), heights, risks ((G, G), or (B, G, G) for B different maps),
    starts (B, 2), goals (B, 2), n steps, nv, nw, planner (NativeMPPI keywords: control bounds), latent (mean, std))."""
    if name.startswith("case_"):
        h, risk, start, goal, kw = case(name[5:])
        return _one(h, risk, start, goal, 300, planner=kw)
    if name == "general33":
        # res 0.3 is the general geometry; 33 * 33 cells are odd, so `next` is staged byte-wise and the slices of instances 1, 2
        # start unaligned.  Path points ignore the origin (-2, -2), as the reference's do: the rovers chase a path displaced by
        # (+2, +2); the third ends clamped in the corner of the map, still in bounds (cell 32 of 33), so all three keep running.
        g, lim = 33, (-2.0, 7.9)
        H = np.stack([M.smooth_heights(g, g, 40 + b) for b in range(3)])
        R = np.stack([smooth_risk(41 + b, g=g) for b in range(3)])
        yy, xx = np.mgrid[0:g, 0:g]
        R[1][(xx - 14) ** 2 + (yy - 21) ** 2 <= 4] = 0.05                  # instance 1 meets a patch without a path
        starts = np.float32([[-1.0, -0.5], [-1.2, 0.7], [6.2, 6.6]])
        goals = np.float32([[1.0, 1.5], [5.5, 4.5], [7.3, 7.5]])
        return dict(G=g, res=0.3, x_limits=lim, heights=H, risks=R, starts=starts, goals=goals, n=150, nv=NV, nw=NW, planner={},
                    latent=latent(g))
    if name.startswith("last_byte_"):
        # What the byte-wise staging of `next` copies LAST: rovers 1 and 2 stand still (one candidate: v = 0) in the last cell
        # (32, 32) of their slices, so every step's walk starts on the last byte of an unaligned slice.  For one of them that
        # cell's only hop is to (32, 31) -- its two other neighbours are collisions -- and the stage goal is a point of the
        # fresh path.  For the other all three neighbours are collisions: the cell has no next hop (255), there is no path and
        # none kept, and the stage goal is the goal.  _a and _b swap the two and run one after the other: whatever a stale byte
        # of LDS holds, it is not right for both.  Rover 0 drives an ordinary map.
        g = 33
        H = np.stack([M.smooth_heights(g, g, 70 + b) for b in range(3)])
        R = np.stack([smooth_risk(71 + b, g=g) for b in range(3)])
        hop, none = (1, 2) if name == "last_byte_a" else (2, 1)
        R[hop][32, 31] = R[hop][31, 31] = 0.05                               # risk[iy, ix]: (31, 32) and (31, 31) are collisions
        R[none][32, 31] = R[none][31, 31] = R[none][31, 32] = 0.05            # ... and (32, 31) too: walled in
        starts = np.float32([[2.0, 3.0], [9.7, 9.75], [9.7, 9.75]])
        goals = np.float32([[7.0, 6.5], [3.0, 4.0], [4.5, 2.5]])
        return dict(G=g, res=0.3, x_limits=None, heights=H, risks=R, starts=starts, goals=goals, n=24, nv=1, nw=1, planner={},
                    latent=latent(g))
    if name == "origin":                       # a power-of-two resolution at a non-zero origin
        h, risk, start, goal, kw = case("smooth")
        return _one(h, risk, (-3.0, -2.0), (10.0, 9.0), 150, x_limits=(-8.0, 24.0))
    if name == "big416":                       # 416 * 416 bytes of `next` do not fit the 160 KiB of LDS: the walk reads global memory
        g = 416
        return _one(M.smooth_heights(g, g, 50), smooth_risk(51, g=g), (20.0, 30.0), (180.0, 150.0), 40)
    if name.startswith("spiral_"):             # ~2000 nodes a walk: 32 segments of 64 lanes, 2 of 1024
        nv, nw = (int(v) for v in name[7:].split("x"))
        h, risk, start, goal, kw = case("maze")
        # (one candidate is (lo_v, lo_w): with the default bounds the rover would only turn on the spot, so 1 x 1 gets a minimum
        # speed and a narrow turn rate, and cuts across the corridor walls: walks from many cells)
        kw = dict(planner=dict(u_min=(0.4, -0.1), u_max=(1.0, 0.1))) if nv * nw == 1 else {}
        return _one(h, risk, start, goal, 100 if nv * nw > 64 else 200, nv=nv, nw=nw, **kw)
    if name == "late_fallback":
        # A band of low risk -- a collision for A*, fast ground for the rover -- 110 cells long.  Driven straight, the rover enters
        # it at its west end and stays in it: no cell in it has a path, so DWA keeps the path of the last cell before it (the
        # root), which runs along the band.  The pick moves along that kept path with the rover, past its 64th node: with
        # 7 x 1 candidates a segment has 64 lanes and pass 2 finds the pick in the second one.
        g, res = 128, 0.25
        risk = smooth_risk(61, g=g)
        risk[60:69, 10:121] = 0.05
        return _one(M.smooth_heights(g, g, 60), risk, (1.1, 16.1), (31.2, 16.1), 320, res=res, nv=7, nw=1,
                    planner=dict(u_min=(1.0, 0.0), u_max=(1.0, 0.0)))        # full speed: 0.3 cells a step
    raise KeyError(name)


def oracle_loop(sc, b):
    """The CPU oracle (astar_dwa_oracle.Loop) of instance b of a scenario."""
    import astar_dwa_oracle as L
    pick = lambda a: a[b] if a.ndim == 3 else a
    kw = dict(sc["planner"])
    return L.Loop(pick(sc["heights"]), pick(sc["risks"]), THR, sc["res"], sc["goals"][b], T, sc["latent"][0], sc["latent"][1],
                  goal_thr=1.0, a_lim=A_LIM, dwa_dt=DWA_DT, nv=sc["nv"], nw=sc["nw"], lookahead=LOOK, x_limits=sc["x_limits"], **kw)


def initial_state(sc, b):
    """(x, y, heading towards the goal): PlanetaryEnv's initial robot state (planetary_env.py:128-141), float32."""
    d = sc["goals"][b] - sc["starts"][b]
    return np.float32([sc["starts"][b][0], sc["starts"][b][1], np.arctan2(d[1], d[0])])


def draws(sc, seed=11):
    """The injected slip draws z (n, B) of a scenario."""
    return np.random.default_rng(seed).standard_normal((sc["n"], len(sc["starts"]))).astype(np.float32)


def free_run(sc, b):
    """The oracle alone, free-running, on instance b: (steps run before AStar.forward raised or n, steps with bearing_margin <=
    DELTA, the loop, the picks' path indices -- None where the goal was the stage goal -- and whether the path was a kept one)."""
    import astar_dwa_oracle as L
    lp = oracle_loop(sc, b)
    st, z = initial_state(sc, b), draws(sc)
    flagged, idx, kept = 0, [], []
    for j in range(sc["n"]):
        margin, i, k = lp.preview(st)
        flagged += margin <= L.DELTA
        idx.append(i)
        kept.append(k)
        out = lp.step(j, st, z[j, b])
        if out is None:
            return j, flagged, lp, idx[:-1], kept[:-1]
        st = out[0]
    return sc["n"], flagged, lp, idx, kept


def lds_bytes(sc, window_cells):
    """astar_dwa_lds_bytes (csrc/astar_dwa.hip) with `next` staged: 4 * (window + 32 reduction words + 2 per candidate + one per
    lane + 4) + the H * W bytes of `next` rounded up to 4; window_cells = 0 is a lower bound (the map window is optional)."""
    na = sc["nv"] * sc["nw"]
    lanes = (na + 63) // 64 * 64
    return 4 * (window_cells + 32 + 2 * na + lanes + 4) + ((sc["G"] ** 2 + 3) & ~3)
