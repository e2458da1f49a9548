"""Adversarial maps for the A* field solve (csrc/astar_kernels.hip): deterministic, seeded, no stored fixtures.

Every generator returns cases (heights, risk, thr, res, goal): float32 (H, W) maps, the stuck threshold (collision = risk <= thr),
the resolution and the goal cell (ix, iy).  The kernel cuts a map into 32 x 32 tiles, each relaxed with a 1-cell halo; these
maps aim at its tile boundaries and corners, partial tiles, long hop counts, wide weight ranges and the threshold's edges.
`CASES` names every case; `batch_instance(k)` makes the instances of a heterogeneous batch.
"""
from __future__ import annotations

import numpy as np

TILE = 32
THR = 0.2
FREE, BLOCKED = np.float32(0.9), np.float32(0.0)


def smooth_heights(H, W, seed, amplitude=2.0):
    """A sum of three seeded sinusoid products, float32 in [0, amplitude]: smooth at any shape, 1 x 1 included."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    h = np.zeros((H, W))
    for _ in range(3):
        fx, fy = rng.uniform(0.02, 0.15, 2)
        px, py = rng.uniform(0, 2 * np.pi, 2)
        h += np.sin(fx * x + px) * np.cos(fy * y + py)
    return ((h + 3.0) * (amplitude / 6.0)).astype(np.float32)


def iid_risk(H, W, seed, blocked):
    """Uniform risk in [0, 1) shifted so that a fraction `blocked` of the cells is at or below THR."""
    u = np.random.default_rng(seed).random((H, W))
    return (u - blocked + THR).astype(np.float32)


def _free_goal(risk, goal, thr=THR):
    risk[goal[1], goal[0]] = max(np.float32(thr) + np.float32(0.5), FREE)
    return goal


# ---- shapes: partial tiles and goals on tile edges ------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 2), (1, 97), (97, 1), (2, 33), (31, 31), (32, 32), (33, 33), (32, 65), (65, 32), (63, 95), (100, 7))


def shape_goals(H, W):
    """The 4 corners, cells on x = 31 / 32 and y = 31 / 32 where they exist, and the centre of the last partial tile."""
    g = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    g += [(x, H // 2) for x in (31, 32) if x < W] + [(W // 2, y) for y in (31, 32) if y < H]
    g.append(((W - 1) // TILE * TILE + (W - 1) % TILE // 2, (H - 1) // TILE * TILE + (H - 1) % TILE // 2))
    return list(dict.fromkeys(g))


def shapes(H, W, seed=0):
    """One smooth map with ~20 % i.i.d. blocked cells; every goal of shape_goals made free.  Returns (heights, risk, goals)."""
    risk = iid_risk(H, W, seed + H * 131 + W, 0.2)
    goals = [_free_goal(risk, g) for g in shape_goals(H, W)]
    return smooth_heights(H, W, seed + 7), risk, THR, 0.5, goals


# ---- maps connected across tiles only diagonally ------------------------------------------------------------------------
def zipper(transpose=False):
    """128 x 64: only (31, y) for even y and (32, y) for odd y are free, so every hop is a diagonal across the x = 31 | 32 tile
    boundary (and the walk crosses y = 31 | 32 and 63 | 64 at tile corners).  The goal is the top end."""
    H, W = 128, 64
    risk = np.full((H, W), BLOCKED)
    ys = np.arange(H)
    risk[ys, np.where(ys % 2 == 0, 31, 32)] = FREE
    h = smooth_heights(H, W, 11)
    goal = (31, 0)
    if transpose:
        return np.ascontiguousarray(h.T), np.ascontiguousarray(risk.T), THR, 0.5, goal[::-1]
    return h, risk, THR, 0.5, goal


def corner_gate(n=160, goal=(5, 5), seed=12):
    """n x n: every cell with x % 32 or y % 32 in {0, 31} is a wall, and at each interior tile corner one diagonal pair is open
    -- (32i - 1, 32j - 1) and (32i, 32j) for i + j even, else (32i - 1, 32j) and (32i, 32j - 1).  Tiles meet only at corners:
    a solve that does not re-flag the diagonal tile leaves the rest of the map at +inf."""
    y, x = np.mgrid[0:n, 0:n]
    wall = np.isin(x % TILE, (0, TILE - 1)) | np.isin(y % TILE, (0, TILE - 1))
    risk = np.where(wall, BLOCKED, FREE).astype(np.float32)
    for i in range(1, (n - 1) // TILE + 1):
        for j in range(1, (n - 1) // TILE + 1):
            a, b = TILE * i, TILE * j
            pair = ((a - 1, b - 1), (a, b)) if (i + j) % 2 == 0 else ((a - 1, b), (a, b - 1))
            for cx, cy in pair:
                risk[cy, cx] = FREE
    return smooth_heights(n, n, seed), risk, THR, 0.5, goal


def spiral(n=192, seed=13):
    """n x n square spiral: a 1-cell corridor wound inward between 1-cell walls, from (0, 0) to the goal at its centre end.
    The only route is the corridor, so hop counts reach about n^2 / 2."""
    risk = np.full((n, n), BLOCKED)
    x = y = 0
    risk[0, 0] = FREE
    moves = [(n - 1, (1, 0)), (n - 1, (0, 1)), (n - 1, (-1, 0))]
    L, d = n - 3, 0
    while L > 0:
        moves += [(L, ((0, -1), (1, 0), (0, 1), (-1, 0))[d % 4]), (L, ((0, -1), (1, 0), (0, 1), (-1, 0))[(d + 1) % 4])]
        L, d = L - 2, d + 2
    for length, (dx, dy) in moves:
        for _ in range(length):
            x, y = x + dx, y + dy
            risk[y, x] = FREE
    return smooth_heights(n, n, seed), risk, THR, 0.5, (x, y)


def percolation(n=256, seed=0, blocked=0.55):
    """n x n i.i.d. risk with ~55 % blocked (8-connected site percolation needs ~59 %): many components, tortuous paths.
    The goal is the free cell nearest the centre in the largest 8-connected component."""
    from scipy import ndimage
    risk = iid_risk(n, n, 1000 + seed, blocked)
    free = ~(risk <= np.float32(THR))
    lab, _ = ndimage.label(free, structure=np.ones((3, 3)))
    big = np.bincount(lab.ravel())[1:].argmax() + 1
    ys, xs = np.nonzero(lab == big)
    j = np.argmin((ys - n // 2) ** 2 + (xs - n // 2) ** 2)
    return smooth_heights(n, n, 2000 + seed), risk, THR, 0.5, (int(xs[j]), int(ys[j]))


# ---- weights ------------------------------------------------------------------------------------------------------------
def wide_weights(H=128, W=160, seed=14):
    """i.i.d. heights in [0, 50) at res 0.05: edge weights from 0.05 to 50, so cells are improved many times."""
    rng = np.random.default_rng(seed)
    h = (rng.random((H, W)) * 50.0).astype(np.float32)
    risk = iid_risk(H, W, seed, 0.1)
    return h, risk, THR, 0.05, _free_goal(risk, (W // 3, H // 2))


def cliffs(H=144, W=112, seed=15):
    """Smooth heights plus 10 m terraces (the side of 3 random lines) and 10 m single-cell spikes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    h = smooth_heights(H, W, seed).astype(np.float64)
    for _ in range(3):
        a, b = rng.uniform(-1, 1, 2)
        c = a * rng.uniform(0, W) + b * rng.uniform(0, H)
        h += 10.0 * (a * x + b * y > c)
    h += 10.0 * (rng.random((H, W)) < 0.03)
    risk = iid_risk(H, W, seed, 0.15)
    return h.astype(np.float32), risk, THR, 0.3, _free_goal(risk, (W - 5, 4))


# ---- the threshold, non-finite heights, resolutions ---------------------------------------------------------------------
def thr_nan(H=96, W=80, seed=16, thr=0.37):
    """20 % of cells with risk exactly == thr (a collision) and 20 % with NaN risk (free), the rest above thr."""
    rng = np.random.default_rng(seed)
    u = rng.random((H, W))
    risk = (np.float32(thr) + np.float32(0.01) + rng.random((H, W)).astype(np.float32)).astype(np.float32)
    risk[u < 0.2] = np.float32(thr)
    risk[(u >= 0.2) & (u < 0.4)] = np.nan
    goal = (W // 2, H // 2)
    risk[goal[1], goal[0]] = np.nan
    return smooth_heights(H, W, seed), risk, thr, 0.5, goal


def nonfinite_heights(H=64, W=70, seed=17):
    """A few NaN and +inf heights: every edge at such a cell has a NaN or +inf weight, i.e. no edge (scipy is not a reference)."""
    rng = np.random.default_rng(seed)
    h = smooth_heights(H, W, seed)
    for v in (np.nan, np.inf):
        h.ravel()[rng.choice(H * W, 40, replace=False)] = v
    risk = iid_risk(H, W, seed, 0.1)
    goal = (3, H - 4)
    h[goal[1], goal[0]] = 1.0
    return h, risk, THR, 0.5, _free_goal(risk, goal)


RESOLUTIONS = (0.05, 0.3, 0.7, 1.0, 2.0)


def resolution(res, H=48, W=80, seed=18):
    risk = iid_risk(H, W, seed, 0.2)
    return smooth_heights(H, W, seed), risk, THR, res, _free_goal(risk, (W - 1 - 9, 10))


def plateau():
    """8 x 16, resolution 1, a 4e7 m cliff at x = 8, the goal beyond it.  Every low cell costs ~4e7, where the f32 spacing is 4
    and an edge weight of 1 or sqrt(2) is absorbed (fl32(w + D) == D): low cells point at each other and no walk ends."""
    h = np.zeros((8, 16), np.float32)
    h[:, 8:] = np.float32(4e7)
    return h, np.full((8, 16), FREE), THR, 1.0, (12, 4)


def batch_instance(k, n=256):
    """Instance k of a heterogeneous batch of n x n maps at resolution 0.5 (one handle shares one resolution): generator
    k % 8, seed k, a threshold of its own (the risk shifted with it) and its own goal; k = 62 has its goal off the map and
    k = 63 in collision."""
    thr = float(np.float32(0.1 + 0.005 * k))
    kind = k % 8
    if kind == 0:
        h, r, g = smooth_heights(n, n, k), iid_risk(n, n, k, 0.1 + 0.03 * (k % 5)), (k * 37 % n, k * 11 % n)
        _free_goal(r, g)
    elif kind == 1:
        h, r, _, _, g = percolation(n, seed=k)
    elif kind == 2:
        h, r, _, _, g = corner_gate(n, goal=(1 + k % 29, 2 + k % 23), seed=k)
    elif kind == 3:
        h, r, _, _, g = spiral(n, seed=k)
    elif kind == 4:
        h, r, _, _, g = wide_weights(n, n, seed=k)
    elif kind == 5:
        h, r, _, _, g = cliffs(n, n, seed=k)
    elif kind == 6:
        h, r, _, _, g = thr_nan(n, n, seed=k, thr=thr)
    else:
        h, r, g = smooth_heights(n, n, k, amplitude=8.0), iid_risk(n, n, k, 0.35), (n - 1 - k % 7, n - 1 - k % 5)
        _free_goal(r, g)
    if kind != 6:
        r = (r + np.float32(thr - THR)).astype(np.float32)
    if k == 62:
        g = (n + 3, 1)
    elif k == 63:
        ys, xs = np.nonzero(r <= np.float32(thr))
        g = (int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))
    return h, r, thr, 0.5, g


def _cases():
    out = {}
    for H, W in SHAPES:
        h, r, thr, res, goals = shapes(H, W)
        for g in goals:
            out[f"shape{H}x{W}_g{g[0]}_{g[1]}"] = (h, r, thr, res, g)
    out["zipper"] = zipper()
    out["zipper_T"] = zipper(transpose=True)
    out["corner_gate"] = corner_gate()
    out["spiral"] = spiral()
    for s in range(3):
        out[f"percolation{s}"] = percolation(seed=s)
    out["wide_weights"] = wide_weights()
    out["cliffs"] = cliffs()
    out["thr_nan"] = thr_nan()
    out["nonfinite_heights"] = nonfinite_heights()
    for res in RESOLUTIONS:
        out[f"res{res}"] = resolution(res)
    out["plateau"] = plateau()
    return out


CASES = _cases()
NO_F64 = ("nonfinite_heights", "plateau")          # no float64 reference (non-finite weights; absorption)


def size(name):
    return CASES[name][0].size
