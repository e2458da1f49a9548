"""Shared by test_clrrt_oracle.py and test_gpu_clrrt.py: the fixture tests/golden/clrrt.npz, the spec's configuration of a fixture
plan, a planner on reference-shaped stand-ins, and the teacher-forced comparison of the device's steers with the recorded ones."""
import functools
import os

import numpy as np

import clrrt_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
G, RES, THR = 64, 0.5, 0.2
TOL_TRAJ = 1e-4                      # README "Parity": trajectories against the reference


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(HERE, "golden", "clrrt.npz"))


def calls():
    fx = fixture()
    return [(k, j) for k in range(int(fx["n_plans"])) for j in range(int(fx[f"p{k}_params"][7]))]


def params(k):
    P = fixture()[f"p{k}_params"]
    return dict(iters=int(P[0]), delta=float(P[1]), rate=float(P[2]), max_seqs=int(P[3]), goal_threshold=float(P[4]), delta_t=float(P[5]),
                seed=int(P[6]), calls=int(P[7]))


def spec_config(k):
    fx, p = fixture(), params(k)
    return S.Config(mean=fx[f"p{k}_mean"], res=RES, thr=THR, goal=fx[f"p{k}_goal"], delta_t=p["delta_t"], max_seqs=p["max_seqs"], delta=p["delta"])


def rows(k, j):
    """The recorded iterations of call j of plan k: a list of dicts."""
    fx, pre = fixture(), f"p{k}_{j}_"
    po, so = fx[pre + "path_off"], fx[pre + "seq_off"]
    out = []
    for i in range(params(k)["iters"]):
        out.append(dict(sample=fx[pre + "sample"][i], near=int(fx[pre + "near"][i]), from_state=fx[pre + "from_state"][i],
                        ctrl_before=fx[pre + "ctrl_before"][i], ctrl_after=fx[pre + "ctrl_after"][i], parent_row=fx[pre + "parent_row"][i],
                        feasible=bool(fx[pre + "feasible"][i]), length=int(fx[pre + "length"][i]), cost=float(fx[pre + "cost"][i]),
                        path=fx[pre + "path"][po[i]:po[i + 1]], actions=fx[pre + "actions"][so[i]:so[i + 1]],
                        states=fx[pre + "states"][so[i] + i:so[i + 1] + i + 1], target=fx[pre + "target"][so[i]:so[i + 1]]))
    return out


@functools.lru_cache(maxsize=None)
def marginal(k, j):
    """Per recorded iteration: does the spec call one of the steer's discrete decisions marginal (clrrt_spec.steer_is_marginal)?"""
    cfg = spec_config(k)
    return np.array([S.steer_is_marginal(cfg, r["from_state"], r["ctrl_before"], r["sample"]) for r in rows(k, j)])


def planner(k, **kw):
    """benchnav_amd.CLRRT for plan k on reference-shaped stand-ins; keywords replace the plan's constructor arguments (`goal`: the
    objectives' goal)."""
    import torch
    from benchnav_amd import CLRRT
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    fx, p = fixture(), params(k)
    gm = FakeGridMap(G, RES)
    dyn = FakeDynamics(fx[f"p{k}_mean"], gm)
    obj = FakeObjectives(torch.as_tensor(np.float32(kw.pop("goal", fx[f"p{k}_goal"])).copy()), THR)
    args = dict(delta_t=p["delta_t"], max_iterations=p["iters"], delta_distance=p["delta"], goal_sample_rate=p["rate"], max_seqs=p["max_seqs"],
                goal_threshold=p["goal_threshold"], seed=p["seed"])
    args.update(kw)
    return CLRRT(3, 2, dyn, obj, gm, **args)


def ulps64(got, want):
    """Largest |got - want| in ulps of the float64 `want` (at least the ulp of 1: the coordinates are metres)."""
    return float((np.abs(got - want) / np.spacing(np.maximum(np.abs(want), 1.0))).max()) if want.size else 0.0


def steer_differences(pl, k, j):
    """Every recorded iteration of (k, j) through pl.steer_batch: a dict of per-iteration arrays -- `points_equal`, `point_abs`
    (largest point difference in metres), `point_ulps`, `discrete_equal` (target indices, length and feasibility), `traj` (largest action /
    state difference), `cost_rel`, `ctrl` (largest controller-state difference relative to max(|value|, 1))."""
    rs = rows(k, j)
    out = pl.steer_batch(np.stack([r["from_state"] for r in rs]), np.stack([r["ctrl_before"] for r in rs]), np.stack([r["sample"] for r in rs]))
    out = {n: v.cpu().numpy() for n, v in out.items()}
    res = {n: [] for n in ("points_equal", "point_abs", "point_ulps", "discrete_equal", "traj", "cost_rel", "ctrl")}
    for i, r in enumerate(rs):
        n = int(out["points"][i])
        same_n = n == len(r["path"])
        res["points_equal"].append(same_n)
        res["point_abs"].append(float(np.abs(out["path"][i, :n] - r["path"]).max()) if same_n else np.inf)
        res["point_ulps"].append(ulps64(out["path"][i, :n], r["path"]) if same_n else np.inf)
        L = int(out["length"][i])
        disc = same_n and L == r["length"] and bool(out["feasible"][i]) == r["feasible"] and np.array_equal(out["targets"][i, :L], r["target"])
        res["discrete_equal"].append(disc)
        if disc:
            res["traj"].append(max(float(np.abs(out["actions"][i, :L] - r["actions"]).max()), float(np.abs(out["states"][i, :L + 1] - r["states"]).max())))
            res["cost_rel"].append(abs(float(out["cost"][i]) - r["cost"]) / max(abs(r["cost"]), 1.0))
            res["ctrl"].append(float((np.abs(out["controllers"][i] - r["ctrl_after"]) / np.maximum(np.abs(r["ctrl_after"]), 1.0)).max()))
        else:
            res["traj"].append(np.inf); res["cost_rel"].append(np.inf); res["ctrl"].append(np.inf)
    return {n: np.asarray(v) for n, v in res.items()}, out
