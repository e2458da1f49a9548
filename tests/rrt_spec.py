"""The RRT global planner restated in NumPy float32: the specification csrc/rrt_kernels.hip implements, checked
bit for bit against the reference's recorded trees (tests/golden/rrt.npz) in test_rrt_oracle.py.

The draws are terrain_draws_spec.Stream's (MT19937 of the seed's low 32 bits, one float32 uniform per 32-bit output); every
comparison is float32 against the float32 of the Python number; the norm of (dx, dy) is sqrt(fma(dy, dy, f32(dx dx))).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from terrain_draws_spec import Stream

f32 = np.float32
GOAL_THRESHOLD = 0.1


def check_seed(seed) -> int:
    """np.random.seed's range (set_randomness): 0 ... 2^32 - 1."""
    s = int(seed)
    if s < 0 or s > 0xFFFFFFFF:
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    return s


def norm(dx, dy) -> np.ndarray:
    """sqrt(fma(dy, dy, f32(dx dx))) in float32, elementwise.  The FMA is made in float64 with the sum rounded to odd (the
    products are exact in float64; the error of the float64 sum sets the sticky bit), so that the rounding to float32 is the
    single rounding of the fused operation."""
    dx, dy = np.asarray(dx, np.float32), np.asarray(dy, np.float32)
    a = dy.astype(np.float64) * dy.astype(np.float64)                # exact: 48 bits
    b = (dx * dx).astype(np.float32).astype(np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)                                  # two-sum: s + err == a + b exactly
    bits = np.atleast_1d(s).view(np.int64).copy()
    e = np.atleast_1d(err)
    even = (bits & 1) == 0
    bits = np.where((e > 0) & even, bits | 1, np.where((e < 0) & even, bits - 1, bits))      # s >= 0: the bit pattern is monotone
    r = np.sqrt(bits.view(np.float64).astype(np.float32))
    return r.reshape(np.shape(s)) if np.ndim(s) else r[0]


def parse_samples(stream: Stream, iters: int, x_limits, y_limits, goal, rate: float):
    """The sample of every iteration from the stream: (xy (iters, 2) float32, is_goal (iters,) bool).  One uniform per
    iteration, two more where it is not below f32(rate)."""
    xs, x0 = f32(x_limits[1] - x_limits[0]), f32(x_limits[0])
    ys, y0 = f32(y_limits[1] - y_limits[0]), f32(y_limits[0])
    g = np.asarray(goal, np.float32)
    xy, flag = np.empty((iters, 2), np.float32), np.zeros(iters, bool)
    for i in range(iters):
        if stream.uniform() < f32(rate):
            xy[i], flag[i] = g, True
        else:
            xy[i, 0] = f32(f32(stream.uniform() * xs) + x0)
            xy[i, 1] = f32(f32(stream.uniform() * ys) + y0)
    return xy, flag


@dataclass
class SpecTree:
    nodes: np.ndarray              # (n, 2) float32
    edges: np.ndarray              # (n,) int32, -1 at the root
    costs: np.ndarray              # (n,) float32
    near: np.ndarray               # near-goal node indices, ascending
    pick: int                      # lowest cost, then lowest index among `near`; -1 when there is none
    path: Optional[np.ndarray]     # (L, 2) float32 node rows, root first


def grow(start, samples: np.ndarray, delta: float):
    """The tree of `samples` from `start`: nodes, edges, costs of iters + 1 nodes (_steer always returns feasible)."""
    iters = len(samples)
    nodes, edges, costs = np.zeros((iters + 1, 2), np.float32), np.full(iters + 1, -1, np.int32), np.zeros(iters + 1, np.float32)
    nodes[0] = np.asarray(start, np.float32)[:2]
    dl = f32(delta)
    for i in range(iters):
        n = i + 1
        sx, sy = samples[i]
        p = int(np.argmin(norm(nodes[:n, 0] - sx, nodes[:n, 1] - sy)))       # the first minimum: the lowest index
        fx, fy = nodes[p]
        dx, dy = f32(sx - fx), f32(sy - fy)
        d = norm(dx, dy)
        if d > dl:
            dx, dy, d = f32(f32(dx / d) * dl), f32(f32(dy / d) * dl), dl
        nodes[n] = (f32(fx + dx), f32(fy + dy))
        edges[n] = p
        costs[n] = f32(costs[p] + d)
    return nodes, edges, costs


def goal_pick(nodes, edges, costs, goal, threshold: float = GOAL_THRESHOLD):
    g = np.asarray(goal, np.float32)
    near = np.nonzero(norm(nodes[:, 0] - g[0], nodes[:, 1] - g[1]) < f32(threshold))[0]
    if near.size == 0:
        return near, -1, None
    pick = int(near[np.argmin(costs[near])])                                  # near is ascending: the lowest index among equal costs
    idx = [pick]
    while idx[-1] != 0:
        idx.append(int(edges[idx[-1]]))
    return near, pick, nodes[idx[::-1]].copy()


def plan_from_samples(start, goal, samples, delta) -> SpecTree:
    nodes, edges, costs = grow(start, samples, delta)
    near, pick, path = goal_pick(nodes, edges, costs, goal)
    return SpecTree(nodes, edges, costs, near, pick, path)


def plan(stream: Stream, start, goal, iters, x_limits, y_limits, delta, rate) -> SpecTree:
    """One forward() on `stream` (a second call on the same stream continues it, as the reference does not reseed)."""
    xy, _ = parse_samples(stream, iters, x_limits, y_limits, goal, rate)
    return plan_from_samples(start, goal, xy, delta)
