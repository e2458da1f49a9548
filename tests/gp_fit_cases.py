"""The seeded cases of the GP fit tests (CPU: test_gp_fit_oracle.py; GPU: test_gpu_gp_fit.py) and their recorded spreads.

Data: N slopes uniform in [-30, 30] degrees with one DUPLICATED input (N >= 2), slips clip(0.5 tanh(x / 12) + 0.3 + 0.05 eps, 0, 1),
both float32.  N covers: below one MFMA block (1, 5), either side of a fragment row block of 16 (16, 17) and of a panel of 32
(31, 32, 33), a partial last panel behind two full ones (65), several panels (130, 257) and one size whose fitted handle lands
on the slab predict kernel (1041).  A single evaluation is a size and one of the four hyperparameter sets of gp_cases.HYPER
(set 3's noise 1e-4 raised to 2e-4 so that its raw noise exists), given as raw parameters; a trajectory is a size and a number
of Adam steps at lr 0.1 from theta = 0 (N = 5 is no trajectory case: its lengthscale gradient underflows).

`python tests/gp_fit_cases.py` rewrites tests/golden/gp_fit.json: per case the spread between gp_fit_spec's two formulations,
the spread between two implementations of the Cholesky formulation, and the ratio of the kernel formulation's distance from
the Cholesky formulation to the first and to the larger of the two (floor 4 eps)."""
import functools
import json
import os

import numpy as np

import gp_cases as GC
import gp_fit_spec as F

NB = F.NB
SIZES = (1, 5, 16, 17, NB - 1, NB, NB + 1, 2 * NB + 1, 130, 257, 1041)
NOISE = tuple(max(h[2], 2e-4) for h in GC.HYPER)
EVAL_CASES = [(n, h) for n in SIZES for h in range(len(GC.HYPER))]
TRAJECTORIES = ((67, 25), (257, 25), (130, 100))            # (N, Adam steps)
LR = 0.1
EMULATED_MAX = 257                                          # the CPU test re-runs the kernel formulation up to this size
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_fit.json")
EPS = np.finfo(np.float64).eps


def eval_id(n: int, h: int) -> str:
    return f"n{n}_h{h}"


def traj_id(n: int, steps: int) -> str:
    return f"n{n}_it{steps}"


@functools.lru_cache(maxsize=None)
def data(n: int):
    """(train_x float32 (n,), train_y float32 (n,))"""
    rng = np.random.default_rng(77000 + n)
    x = rng.uniform(-30.0, 30.0, n).astype(np.float32)
    if n >= 2:
        x[1] = x[0]
    y = np.clip(0.5 * np.tanh(x / 12.0) + 0.3 + 0.05 * rng.standard_normal(n), 0.0, 1.0).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def theta(h: int) -> np.ndarray:
    """the raw parameters of hyperparameter set h"""
    s, l, _ = GC.HYPER[h]
    return np.array([GC.CONSTANTS[h], F.inverse_softplus(s), F.inverse_softplus(l), F.inverse_softplus(NOISE[h] - F.LOWER_BOUND)])


@functools.lru_cache(maxsize=None)
def expected_eval(n: int, h: int):
    """gp_fit_spec.loss_grad_cholesky of the case, computed once per process"""
    x, y = data(n)
    loss, grad = F.loss_grad_cholesky(x, y, theta(h))
    grad.setflags(write=False)
    return loss, grad


def measured_eval_spread(n: int, h: int):
    x, y = data(n)
    return F.eval_spread(expected_eval(n, h), F.loss_grad_eigen(x, y, theta(h)))


def measured_lapack_spread(n: int, h: int):
    """the Cholesky formulation against itself with other code behind every step (gp_fit_spec.loss_grad_cholesky_numpy)"""
    x, y = data(n)
    return F.eval_spread(expected_eval(n, h), F.loss_grad_cholesky_numpy(x, y, theta(h)))


def emulation_distance(n: int, h: int):
    """(loss, gradient): the kernel formulation's distance from the Cholesky formulation"""
    x, y = data(n)
    return F.eval_spread(expected_eval(n, h), F.kernel_formulation(x, y, theta(h)))


def yardstick(rec):
    """(loss, gradient): the larger of the two-formulation spread and the two-implementation spread, floor 4 eps"""
    return max(rec["loss_spread"], rec["lapack_loss_spread"], 4 * EPS), max(rec["grad_spread"], rec["lapack_grad_spread"], 4 * EPS)


@functools.lru_cache(maxsize=None)
def expected_trajectory(n: int, steps: int):
    """(theta, losses) of gp_fit_spec.adam on the Cholesky formulation, computed once per process"""
    x, y = data(n)
    th, losses = F.adam(x, y, F.loss_grad_cholesky, steps, lr=LR)
    th.setflags(write=False)
    losses.setflags(write=False)
    return th, losses


def measured_trajectory_spread(n: int, steps: int):
    x, y = data(n)
    return F.trajectory_spread(expected_trajectory(n, steps), F.adam(x, y, F.loss_grad_eigen, steps, lr=LR))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    evals, trajs = {}, {}
    for n, h in EVAL_CASES:
        ls, gs = measured_eval_spread(n, h)
        rec = {"loss_spread": ls, "grad_spread": gs}
        rec["lapack_loss_spread"], rec["lapack_grad_spread"] = measured_lapack_spread(n, h)
        el, eg = emulation_distance(n, h)
        rec["emulation_loss_ratio"], rec["emulation_grad_ratio"] = el / max(ls, 4 * EPS), eg / max(gs, 4 * EPS)
        rec["emulation_loss_ratio_yardstick"], rec["emulation_grad_ratio_yardstick"] = el / yardstick(rec)[0], eg / yardstick(rec)[1]
        rec = {k: float(v) for k, v in rec.items()}
        evals[eval_id(n, h)] = rec
        print(eval_id(n, h), rec)
    for n, steps in TRAJECTORIES:
        ts, ls = measured_trajectory_spread(n, steps)
        th, losses = expected_trajectory(n, steps)
        trajs[traj_id(n, steps)] = {"theta_spread": ts, "loss_spread": ls, "theta": [float(v) for v in th], "first_loss": float(losses[0]),
                                    "last_loss": float(losses[-1])}
        print(traj_id(n, steps), trajs[traj_id(n, steps)])
    with open(GOLDEN, "w") as f:
        json.dump({"what": "per case of gp_fit_cases.py: the spread between gp_fit_spec.loss_grad_cholesky and loss_grad_eigen "
                           "(eval_spread / trajectory_spread), between loss_grad_cholesky and loss_grad_cholesky_numpy (lapack_*), and "
                           "the kernel formulation's distance over the first and over the larger of the two (floor 4 eps)",
                   "evaluations": evals, "trajectories": trajs}, f, indent=1)
        f.write("\n")
