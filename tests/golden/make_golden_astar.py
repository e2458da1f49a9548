#!/usr/bin/env python3
"""Generate tests/golden/astar.npz by running the reference A* planner (build container only).

Runs the *unmodified* reference `AStar` (src/planners/global_planners/search_based/astar.py) on CPU for a set of maps and
starts, and stores plain arrays: the maps, the goal and start positions, and what each forward() returned (the path as cell
indices, None, or the ValueError's message).  Nothing of the reference itself is stored.  The synthetic maps are generated on an 8-bit grid (`_q8`: uint8 codes times one float32
scale per map), which the fixture stores as
row-wise code deltas (mod 256); the real instance's maps are stored as float32.

    python tests/golden/make_golden_astar.py

Recipe: `/root/reference/src` and `/root/reference` on sys.path and `opensimplex` stubbed, as in make_golden.py.  `pqdict` is not
installed in the build container; `_HeapDict` below stands in for it with the two operations astar.py uses (insert a key that is
not queued, pop the key of least priority).  The stand-in breaks ties between equal priorities in insertion order, where pqdict
breaks them by its heap layout: it changes only WHICH of several equal-cost paths the reference returns, never a path's cost.
AStar reads grid_map.tensors["heights"], .resolution, .x_limits, .y_limits and dynamics._traversability_model._risks only
(astar.py:53-58), so the maps are handed to it in small namespace objects holding exactly those.
"""
from __future__ import annotations

import heapq
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("BENCHNAV_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REF, "src"), REF]
sys.path.append(ROOT)
_stub = types.ModuleType("opensimplex")
_stub.seed = lambda s: None
_stub.noise2 = lambda x, y: 0.0
sys.modules["opensimplex"] = _stub


class _HeapDict:
    """pqdict's subset used by astar.py:97-120: pqdict({key: prio}), truth value, `in`, d[key] = prio for an absent key, pop()."""

    def __init__(self, init):
        self._heap, self._live, self._n = [], {}, 0
        for k, p in init.items():
            self[k] = p

    def __bool__(self):
        return bool(self._live)

    def __contains__(self, k):
        return k in self._live

    def __setitem__(self, k, p):
        assert k not in self._live           # astar.py only inserts absent keys
        self._n += 1
        self._live[k] = self._n
        heapq.heappush(self._heap, (p, self._n, k))

    def pop(self):
        while True:
            p, n, k = heapq.heappop(self._heap)
            if self._live.get(k) == n:
                del self._live[k]
                return k


_pq = types.ModuleType("pqdict")
_pq.pqdict = _HeapDict
sys.modules["pqdict"] = _pq

from src.planners.global_planners.search_based.astar import AStar  # noqa: E402

from benchnav_amd import synth  # noqa: E402


def _ns(heights, risk, res, x0, y0):
    H, W = heights.shape
    gm = types.SimpleNamespace(tensors={"heights": torch.from_numpy(heights)}, resolution=res,
                               x_limits=(x0, x0 + W * res), y_limits=(y0, y0 + H * res))
    dyn = types.SimpleNamespace(_traversability_model=types.SimpleNamespace(_risks=torch.from_numpy(risk)))
    return gm, dyn


def _cell_centre(ix, iy, res, x0, y0):
    return np.array([x0 + (ix + 0.5) * res, y0 + (iy + 0.5) * res], np.float32)


def _q8(a):
    """(uint8 codes, float32 scale) of a map, max -> 255: the synthetic maps are generated on this grid, so the fixture stores the
    codes (a few hundred KB instead of 4 B per cell) and the tests decode exactly what the reference saw (`_decode`)."""
    a = np.asarray(a, np.float32)
    top = float(np.nanmax(a)) if np.isfinite(a).any() else 0.0
    scale = np.float32(top / 255.0 if top > 0 else 1.0)
    return np.clip(np.rint(a / scale), 0, 255).astype(np.uint8), scale


def _decode(codes, scale):
    return codes.astype(np.float32) * np.float32(scale)


def _nearest_free(free, cell):
    fy, fx = np.nonzero(free)
    j = np.argmin((fx - cell[0]) ** 2 + (fy - cell[1]) ** 2)
    return int(fx[j]), int(fy[j])


def run_map(name, heights, risk, thr, res, goal_cell, n_random=16, seed=0, x0=0.0, y0=0.0, extra_starts=(), goal_pos=None,
            snap_goal=True):
    stored = {}
    for key, a in (("heights", heights), ("risk", risk)):
        if isinstance(a, tuple):                                       # _q8 codes: store them, run the decoded map
            stored[f"{key}_q8d"] = np.diff(a[0], axis=1, prepend=np.uint8(0))      # row deltas mod 256: smooth maps compress
            stored[f"{key}_scale"] = np.float32(a[1])
        else:
            stored[key] = np.ascontiguousarray(a, np.float32)
    heights = _decode(*heights) if isinstance(heights, tuple) else np.ascontiguousarray(heights, np.float32)
    risk = _decode(*risk) if isinstance(risk, tuple) else np.ascontiguousarray(risk, np.float32)
    for key, a in (("heights", heights), ("risk", risk)):          # what the tests decode is what the reference ran on
        if f"{key}_q8d" in stored:
            back = np.cumsum(stored[f"{key}_q8d"], axis=1, dtype=np.uint8).astype(np.float32) * stored[f"{key}_scale"]
            assert np.array_equal(back, a), key
    H, W = heights.shape
    if snap_goal and goal_pos is None:
        goal_cell = _nearest_free(~(risk <= np.float32(thr)), goal_cell)
    gm, dyn = _ns(heights, risk, res, x0, y0)
    gpos = _cell_centre(*goal_cell, res, x0, y0) if goal_pos is None else np.asarray(goal_pos, np.float32)
    planner = AStar(gm, torch.from_numpy(gpos), dyn, thr, device="cpu")
    rng = np.random.default_rng(seed)
    free = ~(risk <= np.float32(thr))
    starts = []
    fy, fx = np.nonzero(free)
    for j in rng.choice(len(fx), size=min(n_random, len(fx)), replace=False):
        starts.append(_cell_centre(fx[j], fy[j], res, x0, y0))
    cy, cx = np.nonzero(~free)
    if len(cx):                                                       # a start in collision
        j = rng.integers(len(cx))
        starts.append(_cell_centre(cx[j], cy[j], res, x0, y0))
    starts.append(gpos.copy())                                        # start == goal
    left = _cell_centre(0, H // 2, res, x0, y0)
    left[0] = np.float32(x0 - 0.3 * res)                              # just left of x_limits[0]: int() truncates to index 0
    starts.append(left)
    starts += [np.asarray(s, np.float32) for s in extra_starts]
    starts = np.stack(starts).astype(np.float32)
    status, msgs, nodes, offs = [], [], [], [0]
    for s in starts:
        state = torch.tensor([s[0], s[1], 0.3], dtype=torch.float32)
        try:
            p = planner.forward(state)
        except ValueError as e:
            status.append(2); msgs.append(str(e)); offs.append(offs[-1]); continue
        msgs.append("")
        if p is None:
            status.append(1); offs.append(offs[-1]); continue
        idx = np.rint(p.numpy() / res).astype(np.int32)
        assert np.array_equal(torch.from_numpy(idx).to(torch.int64) * res, p), "path is not index * resolution"
        status.append(0); nodes.append(idx); offs.append(offs[-1] + len(idx))
    nodes = np.concatenate(nodes) if nodes else np.zeros((0, 2), np.int32)
    print(f"{name:14s} {H}x{W}: {len(starts)} starts, {status.count(0)} paths ({len(nodes)} nodes), "
          f"{status.count(1)} None, {status.count(2)} ValueError", flush=True)
    return {f"{name}__{k}": v for k, v in dict(
        **stored, scalars=np.array([thr, res, x0, y0], np.float64), goal_pos=gpos, starts=starts,
        status=np.array(status, np.int8), messages=np.array(msgs), nodes=nodes, offsets=np.array(offs, np.int32)).items()}


def main():
    out, names = {}, []

    def add(name, **kw):
        names.append(name)
        out.update(run_map(name, **kw))

    inst = torch.load(os.path.join(HERE, "instance_000_000.pt"), weights_only=False)
    add("instance", heights=inst["tensors"]["heights"].numpy(), risk=inst["distributions"]["predictions"].mean.numpy(),
        thr=0.15, res=0.5, goal_cell=(6, 5), n_random=20, seed=1)
    add("smooth256", heights=_q8(synth.smooth_height_map(256, 256, 1)), risk=_q8(synth.smooth_risk_map(256, 2)),
        thr=0.25, res=0.5, goal_cell=(200, 190), seed=2)
    add("iid256", heights=_q8(synth.iid_height_map(256, 256, 3)), risk=_q8(synth.iid_risk_map(256, 4)),
        thr=0.1, res=0.5, goal_cell=(30, 220), seed=3)
    add("smooth512", heights=_q8(synth.smooth_height_map(512, 512, 5, coarse=32)), risk=_q8(synth.smooth_risk_map(512, 6, coarse=32)),
        thr=0.25, res=0.5, goal_cell=(400, 100), n_random=10, seed=4)
    add("rect200x300", heights=_q8(synth.smooth_height_map(200, 300, 7)),
        risk=_q8(synth.smooth_risk_map(300, 8)[:200]), thr=0.25, res=0.5, goal_cell=(280, 20), seed=5)
    add("flat", heights=_q8(np.zeros((128, 128))), risk=_q8(np.full((128, 128), 0.9)), thr=0.1, res=0.5,
        goal_cell=(100, 90), seed=6)
    add("maze", heights=_q8(synth.smooth_height_map(128, 96, 9, amplitude=0.3)), risk=_q8(synth.serpentine_risk_map(128, 96, period=4)),
        thr=0.1, res=0.5, goal_cell=(50, 126), n_random=12, seed=7)
    ring = synth.smooth_risk_map(96, 10).numpy() * 0.5 + 0.4             # all free, then a closed wall around the goal
    ring[40:56, 40] = ring[40:56, 55] = ring[40, 40:56] = ring[55, 40:56] = 0.0
    add("unreachable", heights=_q8(synth.smooth_height_map(96, 96, 11)), risk=_q8(ring), thr=0.1, res=0.5, goal_cell=(47, 48), seed=8)
    add("origin_res03", heights=_q8(synth.smooth_height_map(96, 96, 12)), risk=_q8(synth.smooth_risk_map(96, 13)),
        thr=0.25, res=0.3, goal_cell=(70, 20), seed=9, x0=-10.0, y0=5.0)
    # the three ValueErrors of astar.py:88-94: a start out of bounds, a goal out of bounds, a goal in collision
    h = _q8(synth.smooth_height_map(64, 64, 14))
    r = _q8(synth.smooth_risk_map(64, 15))
    add("err_start", heights=h, risk=r, thr=0.1, res=0.5, goal_cell=(10, 10), n_random=2, seed=10,
        extra_starts=[(40.0, 3.0), (3.0, -0.6)])
    add("err_goal_oob", heights=h, risk=r, thr=0.1, res=0.5, goal_cell=(0, 0), goal_pos=(33.0, 5.0), n_random=2, seed=11)
    cy, cx = np.nonzero(_decode(*r) <= np.float32(0.1))
    add("err_goal_coll", heights=h, risk=r, thr=0.1, res=0.5, goal_cell=(int(cx[0]), int(cy[0])), n_random=2, seed=12,
        snap_goal=False)
    out["names"] = np.array(names)
    out["numpy_version"] = np.array(np.__version__)
    path = os.path.join(HERE, "astar.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
