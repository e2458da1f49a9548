"""CPU restatement of the A* planner's goal-rooted field (benchnav_amd/csrc/astar_kernels.hip) in numpy float32.

Graph of the reference (src/planners/global_planners/search_based/astar.py): cells (ix, iy), arrays indexed [iy, ix]; an edge
a -> b for every in-bounds neighbour b of the 8 (in the order `DIRS`) that is not a collision, collision = risk <= threshold
(NaN risk is free); weight w = sqrt_f32(f32(dx^2 + dy^2) + dz * dz), dx, dy = |d index| * resolution in double, dz = |h_a - h_b|
in f32.  The field: D[goal] = 0, D[n] = min over edges n -> m of fl32(w + D[m]); next[n] = first minimiser of fl32(w + D[m])
over the directions (every cell), NEXT_GOAL at the goal, NEXT_NONE where no candidate is finite.

Two solvers reach the same fixpoint (fl32(w + d) is monotone in d and w > 0): `field_dijkstra` (a heapq Dijkstra, exact
fl32 per relaxation; fast on any map) and `field_relax` (vectorised Jacobi relaxation to the fixpoint; the number of sweeps is
the longest hop count, so it is the cross-check on small maps).  Test infrastructure: the product never imports this.
"""
from __future__ import annotations

import heapq
import struct

import numpy as np

DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))   # astar.py:154-163, as (dx, dy)
NEXT_GOAL, NEXT_NONE = 8, 255
_F = struct.Struct("f")


def _f32(x: float) -> float:
    return _F.unpack(_F.pack(x))[0]


def planar_terms(resolution: float):
    """f32(dx^2 + dy^2) for an axis and a diagonal step, the double sum rounded once (astar.py:134-140 under NumPy 2)."""
    r = float(resolution)
    return np.float32(r * r + 0.0), np.float32(r * r + r * r)


def free_mask(risk, threshold) -> np.ndarray:
    return ~(np.asarray(risk, np.float32) <= np.float32(threshold))


def weights(heights, resolution):
    """(8, H, W) float32: w[d, iy, ix] = weight of the step from (ix, iy) in direction d; +inf off the map."""
    h = np.asarray(heights, np.float32)
    H, W = h.shape
    pa, pd = planar_terms(resolution)
    out = np.full((8, H, W), np.inf, np.float32)
    for d, (dx, dy) in enumerate(DIRS):
        ys, yd = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
        xs, xd = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
        dz = np.abs(h[ys, xs] - h[yd, xd])
        out[d, ys, xs] = np.sqrt((pa if d < 4 else pd) + dz * dz)
    return out


def _neighbour_values(D, d):
    """D at the neighbour in direction d of every cell (+inf off the map)."""
    dx, dy = DIRS[d]
    H, W = D.shape
    out = np.full_like(D, np.inf)
    out[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = D[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    return out


def _goal_ok(free, goal):
    gx, gy = goal
    H, W = free.shape
    return 0 <= gx < W and 0 <= gy < H and bool(free[gy, gx])


def field_dijkstra(heights, risk, threshold, resolution, goal) -> np.ndarray:
    """D (H, W) float32, +inf where not reached and on collision cells."""
    free = free_mask(risk, threshold)
    H, W = free.shape
    D = np.full(H * W, np.inf)
    if not _goal_ok(free, goal):
        return D.reshape(H, W).astype(np.float32)
    w = weights(heights, resolution)
    wl = [w[d].ravel().tolist() for d in range(8)]
    fl = free.ravel().tolist()
    offs = [dy * W + dx for dx, dy in DIRS]
    g = goal[1] * W + goal[0]
    D[g] = 0.0
    Dl = D.tolist()
    done = bytearray(H * W)
    heap = [(0.0, g)]
    while heap:
        dm, m = heapq.heappop(heap)
        if done[m]:
            continue
        done[m] = 1
        for d in range(8):
            wd = wl[d][m]                           # w(m, n) == w(n, m) bit for bit
            if wd == np.inf:
                continue
            n = m + offs[d]
            if not fl[n] or done[n]:
                continue
            c = _f32(wd + dm)                       # the double sum of two f32 is exact: one rounding, as fl32
            if c < Dl[n]:
                Dl[n] = c
                heapq.heappush(heap, (c, n))
    return np.asarray(Dl, np.float32).reshape(H, W)


def field_relax(heights, risk, threshold, resolution, goal, max_sweeps=100000) -> np.ndarray:
    """The same field by vectorised Jacobi relaxation of D[n] = min_m fl32(w + D[m]) from +inf to the fixpoint."""
    free = free_mask(risk, threshold)
    H, W = free.shape
    D = np.full((H, W), np.inf, np.float32)
    if not _goal_ok(free, goal):
        return D
    w = weights(heights, resolution)
    D[goal[1], goal[0]] = 0.0
    for _ in range(max_sweeps):
        best = D.copy()
        for d in range(8):
            c = w[d] + _neighbour_values(D, d)
            best = np.where(free & (c < best), c, best)
        if np.array_equal(best, D):
            return D
        D = best
    raise RuntimeError("relaxation did not converge")


def next_hops(heights, D, goal, resolution, risk=None, threshold=None) -> np.ndarray:
    """(H, W) uint8: first minimiser of fl32(w + D[m]) in DIRS order; D is +inf on collision cells, so they never win."""
    w = weights(heights, resolution)
    best = np.full(D.shape, np.inf, np.float32)
    arg = np.full(D.shape, NEXT_NONE, np.uint8)
    for d in range(8):
        c = w[d] + _neighbour_values(D, d)
        take = c < best
        best = np.where(take, c, best)
        arg[take] = d
    gx, gy = goal
    H, W = D.shape
    if 0 <= gx < W and 0 <= gy < H and D[gy, gx] == 0.0:
        arg[gy, gx] = NEXT_GOAL
    return arg


def solve(heights, risk, threshold, resolution, goal, method="dijkstra"):
    """(D, next) of one (map, goal)."""
    f = field_dijkstra if method == "dijkstra" else field_relax
    D = f(heights, risk, threshold, resolution, goal)
    return D, next_hops(heights, D, goal, resolution)


def walk(nxt, start):
    """Nodes [(ix, iy), ...] from `start` to the goal along `nxt`, or None when the goal is unreachable."""
    H, W = nxt.shape
    ix, iy = start
    path = []
    for _ in range(H * W):
        path.append((ix, iy))
        c = int(nxt[iy, ix])
        if c == NEXT_GOAL:
            return path
        if c == NEXT_NONE:
            return None
        ix, iy = ix + DIRS[c][0], iy + DIRS[c][1]
    raise RuntimeError("walk exceeded H*W nodes")


def path_cost64(heights, path, resolution) -> float:
    """The path's cost re-evaluated in float64 (sum of sqrt(dx^2 + dy^2 + dz^2))."""
    h = np.asarray(heights, np.float64)
    c = 0.0
    for (ax, ay), (bx, by) in zip(path[:-1], path[1:]):
        dx, dy = abs(ax - bx) * resolution, abs(ay - by) * resolution
        c += (dx * dx + dy * dy + (h[ay, ax] - h[by, bx]) ** 2) ** 0.5
    return c


def check_path(path, start, goal, free) -> str:
    """'' if `path` is 8-connected, starts at `start`, ends at `goal` and every node after the start is free."""
    if tuple(path[0]) != tuple(start) or tuple(path[-1]) != tuple(goal):
        return f"endpoints {path[0]} -> {path[-1]}, expected {start} -> {goal}"
    for (ax, ay), (bx, by) in zip(path[:-1], path[1:]):
        if max(abs(ax - bx), abs(ay - by)) != 1:
            return f"step {(ax, ay)} -> {(bx, by)} is not an 8-neighbour step"
        if not free[by, bx]:
            return f"node {(bx, by)} is a collision cell"
    return ""


# ---- independent checks: a float64 shortest path, an oracle-free fixpoint certificate, hop counts ------------------------
def field_f64(heights, risk, threshold, resolution, goal) -> np.ndarray:
    """D (H, W) float64 by scipy's Dijkstra over the same graph, built afresh in float64 (no code shared with `weights`):
    an edge n -> m between 8-neighbours that are both in bounds and free (risk > threshold, NaN free), of weight
    sqrt((dx res)^2 + (dy res)^2 + (h_n - h_m)^2) from the float32 heights.  +inf where the goal is not reached, on collision
    cells, and everywhere when the goal is out of bounds or in collision.  Finite heights only."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    h = np.asarray(heights, np.float32).astype(np.float64)
    r = np.asarray(risk, np.float32)
    free = ~(r <= np.float32(threshold))
    H, W = h.shape
    out = np.full((H, W), np.inf)
    gx, gy = goal
    if not (0 <= gx < W and 0 <= gy < H and free[gy, gx]):
        return out
    iy, ix = np.mgrid[0:H, 0:W]
    rows, cols, vals = [], [], []
    for ddx in (-1, 0, 1):
        for ddy in (-1, 0, 1):
            if ddx == 0 and ddy == 0:
                continue
            jx, jy = ix + ddx, iy + ddy
            ok = (jx >= 0) & (jx < W) & (jy >= 0) & (jy < H)
            ok[ok] &= free[iy[ok], ix[ok]] & free[jy[ok], jx[ok]]
            a, b = iy[ok] * W + ix[ok], jy[ok] * W + jx[ok]
            dz = h.ravel()[a] - h.ravel()[b]
            rows.append(a)
            cols.append(b)
            vals.append(np.sqrt((ddx * float(resolution)) ** 2 + (ddy * float(resolution)) ** 2 + dz * dz))
    g = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W)).tocsr()
    # the graph is symmetric, so the distances from the goal are the costs to it
    return dijkstra(g, directed=True, indices=gy * W + gx).reshape(H, W)


def certify_field(heights, risk, threshold, resolution, goal, D) -> str:
    """'' when D is THE float32 field of (map, goal), else what is wrong.  Oracle-free: one vectorised pass computes
    best[n] = min over in-bounds m of fl32(w(n, m) + D[m]) (D read as +inf on collision cells; `c < best` selects, so a NaN
    weight is no edge), then +inf on collision cells and 0 at an in-bounds free goal, and requires best == D bit for bit.

    Why a fixpoint is the field: let D* be the Dijkstra field, the least realised f32 path cost from every cell.  (a) D <= D*:
    along D*'s shortest-path tree in increasing D*, D[n] <= fl32(w + D[m]) <= fl32(w + D*[m]) = D*[n], since fl32(w + d) is
    monotone in d.  (b) D >= D*: when w > 0 is never absorbed (fl32(w + d) > d for every finite d used), D strictly falls
    along the minimising neighbour, so from a finite D[n] that chain cannot repeat a cell and ends at the goal, and D[n] is
    the realised cost of that path, hence >= D*[n].  So the fixpoint is unique and equals D*.  With absorption (costs near
    2^24 x an edge weight, `plateau` in astar_maps.py) step (b) fails and a fixpoint lower than D* could pass."""
    D = np.asarray(D, np.float32)
    free = free_mask(risk, threshold)
    H, W = free.shape
    if D.shape != (H, W):
        return f"shape {D.shape}, expected {(H, W)}"
    Dm = np.where(free, D, np.float32(np.inf))
    h = np.asarray(heights, np.float32)
    r = float(resolution)
    best = np.full((H, W), np.inf, np.float32)
    for dx, dy in DIRS:
        p = np.float32(r * r + 0.0) if dx == 0 or dy == 0 else np.float32(r * r + r * r)
        ys, yd = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
        xs, xd = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
        with np.errstate(invalid="ignore"):
            dz = np.abs(h[ys, xs] - h[yd, xd])
            c = np.sqrt(p + dz * dz) + Dm[yd, xd]
            sub = best[ys, xs]
            best[ys, xs] = np.where(c < sub, c, sub)
    best[~free] = np.inf
    gx, gy = goal
    if 0 <= gx < W and 0 <= gy < H and free[gy, gx]:
        best[gy, gx] = 0.0
    else:
        best[:] = np.inf
    bad = best.view(np.uint32) != D.view(np.uint32)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        return f"{int(bad.sum())} cells are not the fixpoint, first ({x}, {y}): D {D[y, x]!r}, min over neighbours {best[y, x]!r}"
    return ""


def hop_counts(nxt) -> np.ndarray:
    """(H, W) int64: the number of hops along `nxt` from every cell to NEXT_GOAL (0 at the goal), -1 where the walk ends at
    NEXT_NONE.  Pointer doubling, ceil(log2(H W)) + 1 rounds.  Raises on a cycle, a hop off the map or an unknown code."""
    nxt = np.asarray(nxt, np.uint8)
    H, W = nxt.shape
    n = H * W
    code = nxt.ravel().astype(np.int64)
    if ((code > NEXT_GOAL) & (code != NEXT_NONE)).any():
        raise ValueError(f"unknown next-hop code {sorted(set(code[(code > NEXT_GOAL) & (code != NEXT_NONE)].tolist()))}")
    idx = np.arange(n)
    step = code < 8
    ddx = np.array([d[0] for d in DIRS] + [0], np.int64)[np.minimum(code, 8)]
    ddy = np.array([d[1] for d in DIRS] + [0], np.int64)[np.minimum(code, 8)]
    x, y = idx % W + ddx, idx // W + ddy
    off = step & ((x < 0) | (x >= W) | (y < 0) | (y >= H))
    if off.any():
        raise ValueError(f"next of cell {int(idx[off][0] % W), int(idx[off][0] // W)} points off the map")
    jump = np.where(step, y * W + x, idx)
    hops = step.astype(np.int64)
    for _ in range(int(np.ceil(np.log2(max(n, 1)))) + 1):
        hops = hops + hops[jump]
        jump = jump[jump]
    if step[jump].any():
        c = int(idx[step[jump]][0])
        raise RuntimeError(f"next-hop cycle reached from cell {(c % W, c // W)}")
    return np.where(code[jump] == NEXT_GOAL, hops, -1).reshape(H, W)


def check_f64(heights, risk, threshold, resolution, goal, D, nxt) -> str:
    """'' when the float32 field D (and its next-hop map) agrees with field_f64: the same finite cells, every free cell's walk
    ends at the goal exactly where D is finite, and |D - D64| <= (hops + 1) 2^-22 D64 per cell, hops counted along `nxt`
    (each hop rounds its weight and its sum in float32: a few 2^-24 relative)."""
    D = np.asarray(D, np.float32)
    D64 = field_f64(heights, risk, threshold, resolution, goal)
    fin = np.isfinite(D)
    if not np.array_equal(fin, np.isfinite(D64)):
        y, x = np.argwhere(fin != np.isfinite(D64))[0]
        return f"finite cells differ, first ({x}, {y}): D {D[y, x]!r}, float64 {D64[y, x]!r}"
    hops = hop_counts(nxt)
    free = free_mask(risk, threshold)           # a collision cell has D = +inf but a next hop: a start may be in collision
    if not np.array_equal((hops >= 0)[free], fin[free]):
        return "the next-hop walks do not end at the goal exactly where D is finite"
    err = np.abs(D[fin].astype(np.float64) - D64[fin])
    tol = (hops[fin] + 1) * 2.0 ** -22 * D64[fin]
    if (err > tol).any():
        j = np.argmax(err - tol)
        return f"{int((err > tol).sum())} cells beyond tolerance, worst {err[j]!r} > {tol[j]!r}"
    return ""


# ---- tests/golden/astar.npz (tests/golden/make_golden_astar.py) ---------------------------------------------------------
def load_fixtures(path):
    """{name: dict(heights, risk, thr, res, x0, y0, goal_pos, starts, status, messages, paths)}; status 0 path, 1 None, 2 ValueError."""
    z = np.load(path)
    out = {}
    for name in z["names"]:
        g = lambda k: z[f"{name}__{k}"]  # noqa: E731
        thr, res, x0, y0 = g("scalars")
        nodes, offs = g("nodes"), g("offsets")
        def m(k):          # float32 map, or uint8 codes (stored as row deltas mod 256) times a float32 scale: make_golden_astar.py _q8
            if f"{name}__{k}" in z.files:
                return g(k)
            codes = np.cumsum(g(f"{k}_q8d"), axis=1, dtype=np.uint8)
            return codes.astype(np.float32) * np.float32(g(f"{k}_scale"))
        out[str(name)] = dict(heights=m("heights"), risk=m("risk"), thr=float(thr), res=float(res), x0=float(x0), y0=float(y0),
                              goal_pos=g("goal_pos"), starts=g("starts"), status=g("status"), messages=g("messages"),
                              paths=[nodes[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)])
    return out


def pos_to_index(pos, x0, y0, res):
    """astar.py:215-228 on a float32 torch position: int() of an f32 quotient, truncating toward zero."""
    import torch
    pos = torch.as_tensor(pos, dtype=torch.float32)
    return int((pos[0] - x0) / res), int((pos[1] - y0) / res)


def forward_like(fx, D_next, start_pos):
    """astar.py:73-122 over a solved field: ('path', nodes) / ('none', None) / ('error', message)."""
    H, W = fx["heights"].shape
    inb = lambda n: 0 <= n[0] < W and 0 <= n[1] < H  # noqa: E731
    s = pos_to_index(start_pos, fx["x0"], fx["y0"], fx["res"])
    g = pos_to_index(fx["goal_pos"], fx["x0"], fx["y0"], fx["res"])
    if not inb(s) or not inb(g):
        return "error", "Start or goal position is out of bounds."
    if not free_mask(fx["risk"], fx["thr"])[g[1], g[0]]:
        return "error", "Goal position is not traversable."
    p = walk(D_next[1], s)
    return ("none", None) if p is None else ("path", p)


def census(fx, got):
    """Compares forward() outcomes `got` (a list of forward_like results, one per fixture start) with the reference's.
    Returns (identical, tied, cheaper, failures).  A path that differs from the reference's is a tie when its float64 cost is
    the reference path's to n_edges * 2^-22 relative, and "cheaper" when it costs less than that: the reference's search does
    not lower the priority of a node already queued (astar.py:116-120, `if neighbor not in open_set`), so it does not always
    return a shortest path.  A path that costs MORE than the reference's is a failure."""
    free = free_mask(fx["risk"], fx["thr"])
    identical = tied = cheaper = 0
    fails = []
    for i, (kind, val) in enumerate(got):
        st = int(fx["status"][i])
        if st == 2:
            if kind != "error" or val != str(fx["messages"][i]):
                fails.append(f"start {i}: reference raised {fx['messages'][i]!r}, got {kind} {val!r}")
            continue
        if st == 1:
            if kind != "none":
                fails.append(f"start {i}: reference returned None, got {kind}")
            continue
        if kind != "path":
            fails.append(f"start {i}: reference returned a path, got {kind} {val!r}")
            continue
        ref = [tuple(int(v) for v in n) for n in fx["paths"][i]]
        mine = [tuple(int(v) for v in n) for n in val]
        why = check_path(mine, ref[0], ref[-1], free)
        if why:
            fails.append(f"start {i}: {why}")
            continue
        if mine == ref:
            identical += 1
            continue
        c_ref, c_mine = path_cost64(fx["heights"], ref, fx["res"]), path_cost64(fx["heights"], mine, fx["res"])
        tol = max(len(ref), len(mine)) * 2.0 ** -22 * c_ref
        if abs(c_mine - c_ref) <= tol:
            tied += 1
        elif c_mine < c_ref:
            cheaper += 1
        else:
            fails.append(f"start {i}: cost {c_mine!r} exceeds the reference's {c_ref!r} (tolerance {tol:.3e})")
    return identical, tied, cheaper, fails
