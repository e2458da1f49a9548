#!/usr/bin/env python3
"""Generate tests/golden/clrrt.npz by running the reference closed-loop RRT planner (build container only).

Runs the *unmodified* reference `CLRRT` (src/planners/global_planners/sampling_based/cl_rrt.py, with its Tree, Dubins,
PurePursuit, UnicycleModel in inference mode and Objectives) on CPU and stores plain arrays.  The planner's methods are wrapped
from outside to record what each iteration did; nothing of the reference itself is stored.

    python tests/golden/make_golden_clrrt.py

Recipe of make_golden_rrt.py / make_golden_astar_dwa.py: the reference's src and root on sys.path, `opensimplex` stubbed.

Keys.  `n_plans`, `torch_version`, `numpy_version`, `G`, `res`, `thr`, `std`; per plan k: `p{k}_mean` (G, G) float32 risk mean,
`p{k}_params` float64 (max_iterations, delta_distance, goal_sample_rate, max_seqs, goal_threshold, delta_t, seed, calls),
`p{k}_goal` (2,) float32; per call j of it, prefix `p{k}_{j}_`:
  start (3,)                      the state forward() was given
  sample (I, 3)                   the sample of every iteration (the goal node's first three entries, or the drawn position)
  is_goal (I,)                    the sample was the goal node
  near (I,)                       Tree.nearest_neighbor's index
  from_state (I, 3)               the state the steer started from
  ctrl_before (I, 4)              the controllers' state at reset (the parent's stored row; zeros at the root)
  ctrl_after (I, 4) float64       the controllers' state _simulate_path_following returned
  parent_row (I, 4)               the parent's stored row after the steer (the aliased integrals)
  feasible (I,), length (I,), cost (I,)
  path_off (I + 1,), path (sum N, 2) float64      the truncated reference path of every iteration
  seq_off (I + 1,), actions (sum L, 2), states (sum L + I, 3), target (sum L,)   L actions, L + 1 states and the target index per step
  nodes (n, 3), edges (n,), costs (n,), seq_lengths (n,), controllers_states (n, 4)   the tree after forward()
  goal_idx, ret_actions (L, 2), ret_states (L + 1, 3), found, seconds
"""
from __future__ import annotations

import os
import sys
import time
import types

import numpy as np
import torch

REF = os.environ.get("BENCHNAV_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REF, "src"), REF, os.path.dirname(HERE)]
_stub = types.ModuleType("opensimplex")
_stub.seed = lambda s: None
_stub.noise2 = lambda x, y: 0.0
sys.modules["opensimplex"] = _stub

from torch.distributions import Normal  # noqa: E402
from src.environments.grid_map import GridMap  # noqa: E402
from src.simulator.problem_formulation.utils import ModelConfig  # noqa: E402
from src.simulator.problem_formulation.robot_model import UnicycleModel  # noqa: E402
from src.simulator.problem_formulation.objectives import Objectives  # noqa: E402
from src.planners.global_planners.sampling_based.cl_rrt import CLRRT  # noqa: E402

import clrrt_spec as S  # noqa: E402

G, RES, THR, STD, DT = 64, 0.5, 0.2, 0.05, 0.1


def mean_map(seed, stuck=None):
    """make_golden_astar_dwa.py's smooth sinusoidal mean; `stuck` = (cx, cy, r) cells of risk 0.9 (traversability 0.1 <= THR)."""
    yy, xx = np.mgrid[0:G, 0:G].astype(np.float32)
    m = (0.45 + 0.2 * np.sin(xx / 9.0 + seed) * np.cos(yy / 11.0 - seed)).astype(np.float32)
    if stuck is not None:
        cx, cy, r = stuck
        m[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 0.9
    return m


# (map seed, stuck region, [start of every forward() call], goal, iterations, max_seqs, seed, delta_distance).  Chosen so that the
# spec alone calls at most 2 % of a plan's steers marginal (asserted below); plan 2's short max_seqs leaves most steers infeasible,
# 24 of them from a node other than the root (the aliased integrals of a failed steer).
PLANS = [
    (1, None, [(8.0, 8.0, 0.3)], (24.0, 24.0), 60, 250, 42, 5.0),
    (2, (28, 26, 5), [(6.0, 9.0, -1.2)], (22.0, 20.0), 50, 250, 0, 5.0),
    (3, None, [(8.0, 8.0, 0.3)], (24.0, 24.0), 50, 40, 2 ** 32 - 1, 2.25),
    (4, (40, 20, 4), [(10.0, 6.0, 2.0), (5.0, 20.0, -0.5)], (18.0, 14.0), 50, 250, 11, 5.0),
    (1, None, [(8.0, 8.0, 0.3)], (24.0, 24.0), 3, 250, 42, 5.0),
]


def build(mean, goal, iters, max_seqs, seed, delta):
    mean_t, std_t = torch.from_numpy(mean), torch.full((G, G), STD)
    tens = {"heights": torch.zeros(G, G), "slopes": torch.zeros(G, G), "t_classes": torch.zeros(G, G), "colors": torch.zeros(3, G, G)}
    dist = {"latent_models": Normal(mean_t, std_t), "predictions": Normal(mean_t, std_t)}
    gm = GridMap(grid_size=G, resolution=RES, tensors=tens, distributions=dist, instance_name="synthetic", device="cpu")
    dyn = UnicycleModel(gm, ModelConfig(mode="inference", inference_metric="expected_value"), device="cpu")
    obj = Objectives(dyn, goal_pos=torch.tensor(goal, dtype=torch.float32), stuck_threshold=THR)
    return CLRRT(dim_state=3, dim_control=2, dynamics=dyn, objectives=obj, grid_map=gm, delta_t=DT, max_iterations=iters,
                 delta_distance=delta, max_seqs=max_seqs, device="cpu", seed=seed)


def record_call(planner, start):
    rows = {k: [] for k in ("sample", "is_goal", "near", "from_state", "ctrl_before", "ctrl_after", "parent_row", "feasible", "length",
                            "cost", "path", "actions", "states", "target")}
    real_steer, real_sim, pp = planner._steer, planner._simulate_path_following, planner._pure_pursuit
    real_target = pp._compute_target_points
    cur = {}

    def steer(idx, to_node):
        rows["sample"].append(to_node[:3].numpy().astype(np.float32).copy())
        rows["is_goal"].append(to_node is planner._goal_node)
        rows["near"].append(int(idx))
        return real_steer(idx, to_node)

    def target(state_batch, paths):
        out = real_target(state_batch, paths)
        hit = torch.nonzero((paths[0] == out[0]).all(dim=1))[:, 0]
        cur["t"].append(int(hit[0]))
        return out

    def sim(idx, path):
        tree = planner.tree
        cur["t"] = []
        rows["from_state"].append((planner._start_node if idx == 0 else tree.nodes[idx]).numpy().astype(np.float32).copy())
        rows["ctrl_before"].append(np.zeros(4, np.float32) if idx == 0 else tree.controllers_states[idx].numpy().copy())
        rows["path"].append(path.numpy().astype(np.float64).copy())
        assert path.dtype == torch.float64 and len(np.unique(path.numpy(), axis=0)) == len(path)
        a, s, c, cost, ok = real_sim(idx, path)
        rows["ctrl_after"].append(c[0].numpy().astype(np.float64).copy())
        rows["parent_row"].append(tree.controllers_states[idx].numpy().copy())
        rows["feasible"].append(bool(ok))
        rows["length"].append(int(a.shape[1]))
        rows["cost"].append(float(cost))
        rows["actions"].append(a[0].numpy().astype(np.float32).copy())
        rows["states"].append(s[0].numpy().astype(np.float32).copy())
        rows["target"].append(np.asarray(cur["t"], np.int32))
        assert len(cur["t"]) == a.shape[1]
        return a, s, c, cost, ok

    planner._steer, planner._simulate_path_following, pp._compute_target_points = steer, sim, target
    try:
        t0 = time.perf_counter()
        with torch.no_grad():
            ret_a, ret_s = planner(torch.tensor(start, dtype=torch.float32))
        dt = time.perf_counter() - t0
    finally:
        planner._steer, planner._simulate_path_following, pp._compute_target_points = real_steer, real_sim, real_target
    tree, n = planner.tree, planner.tree.nodes_count
    out = {
        "start": np.float32(start),
        "sample": np.asarray(rows["sample"], np.float32), "is_goal": np.asarray(rows["is_goal"], np.bool_),
        "near": np.asarray(rows["near"], np.int32), "from_state": np.asarray(rows["from_state"], np.float32),
        "ctrl_before": np.asarray(rows["ctrl_before"], np.float32), "ctrl_after": np.asarray(rows["ctrl_after"], np.float64),
        "parent_row": np.asarray(rows["parent_row"], np.float32), "feasible": np.asarray(rows["feasible"], np.bool_),
        "length": np.asarray(rows["length"], np.int32), "cost": np.asarray(rows["cost"], np.float32),
        "path_off": np.cumsum([0] + [len(p) for p in rows["path"]]).astype(np.int32), "path": np.concatenate(rows["path"]),
        "seq_off": np.cumsum([0] + [len(a) for a in rows["actions"]]).astype(np.int32),
        "actions": np.concatenate(rows["actions"]), "states": np.concatenate(rows["states"]), "target": np.concatenate(rows["target"]),
        "nodes": tree.nodes[:n].numpy().astype(np.float32).copy(), "edges": tree.edges[:n].numpy().astype(np.int32),
        "costs": tree.costs[:n].numpy().astype(np.float32).copy(), "seq_lengths": tree.seq_lengths[:n].numpy().astype(np.int32),
        "controllers_states": tree.controllers_states[:n].numpy().astype(np.float32).copy(),
        "goal_idx": np.asarray(planner._goal_node_indices, np.int32),
        "ret_actions": ret_a.numpy().astype(np.float32) if ret_a is not None else np.zeros((0, 2), np.float32),
        "ret_states": ret_s[0].numpy().astype(np.float32) if ret_s is not None else np.zeros((0, 3), np.float32),
        "found": np.bool_(ret_a is not None), "seconds": np.float64(dt),
    }
    return out


def main():
    arrays = {"torch_version": np.array(torch.__version__), "numpy_version": np.array(np.__version__), "G": np.int32(G), "res": np.float64(RES),
              "thr": np.float64(THR), "std": np.float64(STD)}
    shares = []
    for k, (mseed, stuck, starts, goal, iters, max_seqs, seed, delta) in enumerate(PLANS):
        mean = mean_map(mseed, stuck)
        planner = build(mean, goal, iters, max_seqs, seed, delta)
        arrays[f"p{k}_mean"] = mean
        arrays[f"p{k}_params"] = np.array([iters, delta, 0.25, max_seqs, 1.0, DT, seed, len(starts)], np.float64)
        arrays[f"p{k}_goal"] = np.float32(goal)
        for j, start in enumerate(starts):
            r = record_call(planner, start)
            for name, v in r.items():
                arrays[f"p{k}_{j}_{name}"] = v
            # the spec alone: the share of steers with a marginal discrete decision stays under 2 % (tests/test_clrrt_oracle.py asserts it too)
            cfg = S.Config(mean=mean, res=RES, thr=THR, goal=np.float32(goal), delta_t=DT, max_seqs=max_seqs, delta=delta)
            marg = sum(S.steer_is_marginal(cfg, r["from_state"][i], r["ctrl_before"][i], r["sample"][i]) for i in range(iters))
            shares.append((k, j, marg, iters))
            print(f"plan {k} call {j}: seed {seed} iters {iters} max_seqs {max_seqs}: {len(r['nodes'])} nodes, {int(r['feasible'].sum())} feasible, "
                  f"found {bool(r['found'])}, path {len(r['ret_actions'])} steps, marginal {marg}, {r['seconds']:.2f} s")
    arrays["n_plans"] = np.int32(len(PLANS))
    out = os.path.join(HERE, "clrrt.npz")
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) < (1 << 20)
    assert all(m <= 0.02 * n for _, _, m, n in shares), shares


if __name__ == "__main__":
    main()
