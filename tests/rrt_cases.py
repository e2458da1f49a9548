"""tests/golden/rrt.npz (made by tests/golden/make_golden_rrt.py from the unmodified reference) as plain objects, and the rules
the RRT tests hold a result to.  Loaded once and shared; nothing here is modified by a test."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass
from typing import List

import numpy as np

from helpers import GOLDEN_DIR


@dataclass(frozen=True)
class RefCall:
    nodes: np.ndarray
    edges: np.ndarray
    costs: np.ndarray
    goal_idx: np.ndarray           # the reference's _goal_node_indices (its argsort of the near-goal costs)
    path: np.ndarray               # (L, 2); (0, 2) when forward() returned None
    found: bool


@dataclass(frozen=True)
class RefCase:
    k: int
    x_limits: tuple
    y_limits: tuple
    start: np.ndarray
    goal: np.ndarray
    delta: float
    rate: float
    iters: int
    seed: int
    calls: List[RefCall]

    @property
    def geometry(self):
        return (self.x_limits, self.y_limits, tuple(self.start), tuple(self.goal), self.delta, self.rate, self.iters)


@functools.lru_cache(maxsize=1)
def load():
    z = np.load(os.path.join(GOLDEN_DIR, "rrt.npz"))
    cases = []
    for k in range(int(z["n_cases"])):
        p = z[f"c{k}_params"]
        calls = [RefCall(z[f"c{k}_{j}_nodes"], z[f"c{k}_{j}_edges"], z[f"c{k}_{j}_costs"], z[f"c{k}_{j}_goal_idx"], z[f"c{k}_{j}_path"],
                         bool(z[f"c{k}_{j}_found"])) for j in range(int(z[f"c{k}_calls"]))]
        cases.append(RefCase(k, (float(p[0]), float(p[1])), (float(p[2]), float(p[3])), p[4:6].astype(np.float32), p[6:8].astype(np.float32),
                             float(p[8]), float(p[9]), int(z[f"c{k}_iters"]), int(z[f"c{k}_seed"]), calls))
    meta = {"torch_version": str(z["torch_version"]), "ref_seconds_per_1000": z["ref_seconds_per_1000"]}
    return cases, meta


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_against_reference(ref: RefCall, nodes, edges, costs, near_count: int, pick: int, path) -> None:
    """A result (the spec's or the device's) against what the reference returned: the tree bit for bit; the near-goal count; the
    pick's cost bit for bit; with 16 or fewer near-goal nodes the reference's sort is stable, so pick and path are the
    reference's; with more the reference ends on an arbitrary node among the equal-cost ones, and its path is this one or this
    one plus one last row repeating its end."""
    assert same(nodes, ref.nodes) and same(costs, ref.costs) and np.array_equal(edges, ref.edges)
    assert near_count == len(ref.goal_idx)
    if not ref.found:
        assert near_count == 0 and pick == -1 and path is None
        return
    assert path is not None and path.dtype == np.float32
    ref_pick = int(ref.goal_idx[0])
    assert same(costs[pick:pick + 1], ref.costs[ref_pick:ref_pick + 1])
    assert pick == int(min(i for i in ref.goal_idx.tolist() if bits(ref.costs)[i] == bits(ref.costs)[ref_pick]))    # lowest index among the ties
    if near_count <= 16:
        assert pick == ref_pick and same(path, ref.path)
    else:
        assert same(path, ref.path) or (len(ref.path) == len(path) + 1 and same(ref.path[:-1], path) and same(ref.path[-1], path[-1]))


# ---- caller-supplied samples (grow_from_samples): exact ties and the clip threshold ----
DELTA = 5.0
START = np.array([0.0, 0.0], np.float32)
GOAL = np.array([20.0, 12.0], np.float32)
ABOVE = np.nextafter(np.float32(DELTA), np.float32(np.inf))
# what the first iterations meet, in order (start (0, 0), delta 5):
PREFIX = np.array([
    [0.0, 0.0],        # the start itself: d = 0, a duplicate node 1 = node 0, cost unchanged
    [0.0, 3.0],        # equally far from nodes 0 and 1 (they coincide): parent 0
    [5.0, 3.0],        # d == np.float32(delta) from node 2 = (0, 3): not clipped, node 3 = (5, 3)
    [2.5, 7.0],        # equally far from (0, 3) and (5, 3) (dx = +-2.5, dy = 4): the lower index, node 2
    [0.0, -ABOVE],     # from node 0: d one ulp above delta, clipped to node 5 = (0, -5)
    [20.0, 12.0],      # the goal, far: clipped steps
], np.float32)


def synthetic_samples(iters, variant, rng):
    """(iters, 2): the prefix, then 0 = uniform samples with the goal mixed in; 1 = a third of that, then the goal for ever (a long
    run of exact duplicates once it is reached); 2 = the start for ever (the whole tree is one point)."""
    s = rng.uniform(0.0, 32.0, (iters, 2)).astype(np.float32)
    s[rng.uniform(size=iters) < 0.15] = GOAL
    if variant == 1:
        s[iters // 3:] = GOAL
    if variant == 2:
        s[:] = START
    m = min(iters, len(PREFIX))
    if variant != 2:
        s[:m] = PREFIX[:m]
    return s
