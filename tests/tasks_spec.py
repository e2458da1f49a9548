"""NumPy restatement of the task stage (benchnav_amd/csrc/task_kernels.hip, benchnav_amd/tasks.py): the passable mask, component
labels by a plain flood fill, sizes, statistics, the start/goal sampler and SPL.  Every result is an integer or a fixed function of
integers, so the GPU tests compare bit for bit.  Philox comes from tests/rng_reference.py.  Test infrastructure: the product never
imports this."""
from __future__ import annotations

import numpy as np

import rng_reference as R

f32 = np.float32
TASK_WORD = 0x5441534B                  # 'TASK'
STATS = 8
GOAL, INVALID = 0, 3                    # benchmark outcome codes


# ---- mask ------------------------------------------------------------------------------------------------------------------------
def passable(mean, std, kappa=0.0, stuck_threshold=0.1) -> np.ndarray:
    """uint8: isfinite(mean) && isfinite(std) && 1 - clamp(fl32(mean + fl32(kappa * std)), 0, 1) > stuck_threshold, in float32."""
    mean, std = np.asarray(mean, f32), np.asarray(std, f32)
    ok = np.isfinite(mean) & np.isfinite(std)
    with np.errstate(all="ignore"):
        prod = (f32(kappa) * np.where(ok, std, f32(0))).astype(f32)
        v = (np.where(ok, mean, f32(0)) + prod).astype(f32)
        trav = (f32(1) - np.minimum(np.maximum(v, f32(0)), f32(1))).astype(f32)
    return (ok & (trav > f32(stuck_threshold))).astype(np.uint8)


# ---- labels ----------------------------------------------------------------------------------------------------------------------
def neighbours(connectivity):
    if connectivity == 4:
        return ((1, 0), (-1, 0), (0, 1), (0, -1))
    if connectivity == 8:
        return ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1))
    raise ValueError("connectivity must be 4 or 8")


def flood_labels(mask, connectivity=4) -> np.ndarray:
    """(H, W) int32 of one map: the smallest linear index iy * W + ix of the cell's component, -1 on a blocked cell.  Cells are
    visited in index order, so the seed of a fill is its component's smallest index."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    free = m.ravel().tolist()
    lab = [-1] * (H * W)
    nb = neighbours(connectivity)
    for seed in range(H * W):
        if not free[seed] or lab[seed] >= 0:
            continue
        lab[seed] = seed
        stack = [seed]
        while stack:
            c = stack.pop()
            y, x = divmod(c, W)
            for dx, dy in nb:
                nx, ny = x + dx, y + dy
                if 0 <= nx < W and 0 <= ny < H:
                    n = ny * W + nx
                    if free[n] and lab[n] < 0:
                        lab[n] = seed
                        stack.append(n)
    return np.asarray(lab, np.int32).reshape(H, W)


def label(masks, connectivity=4):
    """(labels (M, H, W) int32, sizes (M, H * W) int32, stats (M, 8) int32) of a batch of masks."""
    masks = np.asarray(masks)
    labels = np.stack([flood_labels(m, connectivity) for m in masks])
    return labels, sizes(labels), stats(labels)


def sizes(labels) -> np.ndarray:
    labels = np.asarray(labels)
    M, cells = labels.shape[0], labels[0].size
    out = np.zeros((M, cells), np.int32)
    for m in range(M):
        l = labels[m].ravel()
        out[m] = np.bincount(l[l >= 0], minlength=cells).astype(np.int32)
    return out


def stats(labels, error_flags=0) -> np.ndarray:
    """Per map: passable cells, components, the largest size, its label (the smallest label wins a tie; -1 without one), error
    flags, three zeros."""
    sz = sizes(labels)
    out = np.zeros((sz.shape[0], STATS), np.int32)
    for m, s in enumerate(sz):
        big = int(s.max()) if s.size else 0
        out[m, :5] = [int(s.sum()), int((s > 0).sum()), big, int(np.argmax(s)) if big > 0 else -1, error_flags]   # argmax: the first
    return out


# ---- pairs -----------------------------------------------------------------------------------------------------------------------
def cell_centres(i, origin, resolution) -> np.ndarray:
    """fl32(origin + fl32(fl32(i + 0.5) * resolution))"""
    half = (np.asarray(i).astype(f32) + f32(0.5)).astype(f32)
    return (f32(origin) + (half * f32(resolution)).astype(f32)).astype(f32)


def cell_of(position, origin, resolution) -> np.ndarray:
    """The float32 lookup floor((p - origin) / resolution) of the planners and the environment."""
    q = ((np.asarray(position, f32) - f32(origin)).astype(f32) / f32(resolution)).astype(f32)
    return np.floor(q).astype(np.int64)


def draws(seed, first_map, M, P, attempts, H, W, border):
    """(sx, sy, gx, gy), each (M, P, attempts) int64: every attempt's cells."""
    Win, Hin = W - 2 * border, H - 2 * border
    n = np.uint64(Win * Hin)
    a = np.arange(attempts, dtype=np.uint32)[None, None, :]
    p = np.arange(P, dtype=np.uint32)[None, :, None]
    m = R.u32(np.arange(M, dtype=np.int64) + int(first_map))[:, None, None]
    r0, r1, _, _ = R.philox4x32(a, p, m, np.uint32(TASK_WORD), R.lo32(seed), R.hi32(seed), rounds=10)
    s = ((r0.astype(np.uint64) * n) >> np.uint64(32)).astype(np.int64)
    g = ((r1.astype(np.uint64) * n) >> np.uint64(32)).astype(np.int64)
    return s % Win + border, s // Win + border, g % Win + border, g // Win + border


def accepted(labels, sz, seed, first_map, P, attempts, border, min_separation_sq, min_component_cells) -> np.ndarray:
    """(M, P, attempts) bool: the attempts the rules accept, with their cells (sx, sy, gx, gy)."""
    labels = np.asarray(labels)
    M, H, W = labels.shape
    sx, sy, gx, gy = draws(seed, first_map, M, P, attempts, H, W, border)
    mi = np.arange(M)[:, None, None]
    ls, lg = labels[mi, sy, sx], labels[mi, gy, gx]
    big = np.asarray(sz)[mi, np.maximum(ls, 0)] >= min_component_cells
    ok = (ls >= 0) & (lg == ls) & big & ((gx - sx) ** 2 + (gy - sy) ** 2 >= min_separation_sq)
    return ok, (sx, sy, gx, gy)


def sample(labels, sz, pairs, seed, first_map=0, border=2, min_separation_sq=0, min_component_cells=1, max_attempts=256, x0=0.0, y0=0.0,
           resolution=0.5):
    """(cells (M, P, 4) int32, attempt (M, P) int32, positions (M, P, 4) float32): the lowest accepted attempt of every pair,
    -1 / -1 / NaN where none is."""
    ok, (sx, sy, gx, gy) = accepted(labels, sz, seed, first_map, pairs, max_attempts, border, min_separation_sq, min_component_cells)
    found = ok.any(axis=2)
    first = np.argmax(ok, axis=2)
    take = lambda v: np.take_along_axis(v, first[..., None], axis=2)[..., 0]
    cells = np.stack([take(sx), take(sy), take(gx), take(gy)], axis=-1)
    cells = np.where(found[..., None], cells, -1).astype(np.int32)
    attempt = np.where(found, first, -1).astype(np.int32)
    pos = np.stack([cell_centres(cells[..., 0], x0, resolution), cell_centres(cells[..., 1], y0, resolution),
                    cell_centres(cells[..., 2], x0, resolution), cell_centres(cells[..., 3], y0, resolution)], axis=-1)
    positions = np.where(found[..., None], pos, f32(np.nan)).astype(f32)
    return cells, attempt, positions


# ---- the masks the CPU and the GPU tests label ----------------------------------------------------------------------------------------
def iid(H, W, seed, blocked=0.3) -> np.ndarray:
    return (np.random.default_rng(seed).random((H, W)) >= blocked).astype(np.uint8)


def serpentine(n) -> np.ndarray:
    """One corridor one cell wide: the even rows, joined at alternating ends.  One component that crosses every tile border."""
    g = np.zeros((n, n), np.uint8)
    g[0::2] = 1
    g[1::4, n - 1] = 1
    g[3::4, 0] = 1
    return g


def comb(H, W) -> np.ndarray:
    """Two interleaved combs that never touch: a spine on the first row with teeth on the columns 0 mod 4, one on the last row with
    teeth on the columns 2 mod 4."""
    g = np.zeros((H, W), np.uint8)
    g[0], g[H - 1] = 1, 1
    g[0:H - 2, 0::4] = 1
    g[2:H, 2::4] = 1
    return g


def spiral(n) -> np.ndarray:
    """A square spiral corridor one cell wide with walls one cell wide, from a corner inwards."""
    g = np.zeros((n, n), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    g[0, 0] = 1
    free = lambda px, py: 0 <= px < n and 0 <= py < n and bool(g[py, px])
    while True:
        for _ in range(2):
            nx, ny = x + dx, y + dy
            if 0 <= nx < n and 0 <= ny < n and not g[ny, nx] and not free(x + 2 * dx, y + 2 * dy):
                break
            dx, dy = -dy, dx
        else:
            return g
        x, y = nx, ny
        g[y, x] = 1


def two_spirals(n) -> np.ndarray:
    """Two spirals side by side, the second mirrored, a blocked column between them."""
    s = spiral(n)
    return np.concatenate([s, np.zeros((n, 1), np.uint8), s[::-1, ::-1]], axis=1)


def label_cases():
    """{name: masks (M, H, W) uint8}, the cases of the issue."""
    checker = (np.add.outer(np.arange(64), np.arange(64)) % 2 == 0).astype(np.uint8)
    single = np.zeros((64, 64), np.uint8)
    single[37, 45] = 1
    one = lambda g: np.asarray(g, np.uint8)[None]
    return {
        "1x1_passable": one([[1]]), "1x1_blocked": one([[0]]), "2x2": one([[1, 0], [0, 1]]),
        "31x33": one(iid(31, 33, 1)), "32x32": one(iid(32, 32, 2)), "33x33": one(iid(33, 33, 3)), "65x65": one(iid(65, 65, 4)),
        "96x160": one(iid(96, 160, 5)),
        "64_all_passable": one(np.ones((64, 64))), "64_all_blocked": one(np.zeros((64, 64))), "64_checkerboard": one(checker),
        "64_single_cell": one(single), "256_serpentine": one(serpentine(256)), "comb": one(comb(70, 90)), "two_spirals": one(two_spirals(47)),
        "512_iid": one(iid(512, 512, 6)),
        "batch_of_five": np.stack([iid(64, 64, 7), checker, serpentine(64), iid(64, 64, 8, blocked=0.45), comb(64, 64)]),
    }


# ---- SPL -------------------------------------------------------------------------------------------------------------------------
def spl(outcome, path_length, optimal_length):
    """(spl, path_ratio_mean) of one setting's episodes: the mean over the valid (not INVALID) episodes of
    [outcome == GOAL] * L* / max(L, L*) (1 where both are 0), and the mean of L / L* over the GOAL episodes with L* > 0; None over
    nothing."""
    oc = np.asarray(outcome).ravel()
    L, Ls = np.asarray(path_length, np.float64).ravel(), np.asarray(optimal_length, np.float64).ravel()
    terms, ratios = [], []
    for o, l, ls in zip(oc, L, Ls):
        if o == INVALID:
            continue
        if o == GOAL:
            top = max(float(l), float(ls))
            terms.append(float(ls) / top if top > 0.0 else 1.0)
            if ls > 0.0:
                ratios.append(float(l) / float(ls))
        else:
            terms.append(0.0)
    mean = lambda v: float(np.mean(np.asarray(v, np.float64))) if v else None
    return mean(terms), mean(ratios)
