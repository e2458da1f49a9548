"""CPU: the float64 specification of the GP fit (gp_fit_spec.py) against closed forms, finite differences and itself, the recorded
spreads of tests/golden/gp_fit.json, the NumPy emulation of the kernels' formulation, and the Adam trajectory.

The emulation's bound ("Held to"): the emulation was meant to stay below 4 x the two-formulation spread, a quarter
of the GPU test's margin.  It does on 42 of the 44 cases; on n130_h0 (loss 5.0 x a spread of 9.1e-16, i.e. 20 eps) and n257_h3 (loss
7.8 x a spread of 3.6e-14) it does not, and neither does a second implementation of the SAME Cholesky formulation
(gp_fit_spec.loss_grad_cholesky_numpy: 3.7 x and 8.7 x there), so on those cases the two-formulation spread is a lucky draw and
not the size of a correct evaluation's error.  The emulation is therefore held to 4 x the larger of the two spreads (it lands at
up to 1.4 x in the loss and 1.9 x in the gradient); the GPU test's bound of 16 x the two-formulation spread stays as it was set."""
import numpy as np
import pytest

import gp_fit_cases as FC
import gp_fit_spec as F

EPS = np.finfo(np.float64).eps
FLOOR = 64 * EPS


def test_spec_closed_form_one_training_point():
    """N = 1: K = s + noise, loss = [ r^2 / K + log K + log 2 pi ] / 2, dloss/dc = -r / K, dloss/dK = (1 / K - r^2 / K^2) / 2."""
    x, y = np.float32([3.5]), np.float32([0.7])
    th = np.array([0.1, -0.3, 1.2, -2.0])
    c, s, l, noise = F.hyper(th)
    K, r = s + noise, float(y[0]) - c
    loss = (r * r / K + np.log(K) + F.LOG2PI) / 2.0
    gK = (1.0 / K - r * r / (K * K)) / 2.0
    grad = np.array([-r / K, gK * F.sigmoid(th[1]), 0.0, gK * F.sigmoid(th[3])])
    for f in (F.loss_grad_cholesky, F.loss_grad_eigen, F.loss_grad_cholesky_numpy, F.kernel_formulation):
        got_loss, got_grad = f(x, y, th)
        assert abs(got_loss - loss) <= 8 * EPS * abs(loss), f.__name__
        np.testing.assert_allclose(got_grad, grad, rtol=0, atol=16 * EPS * np.max(np.abs(grad)), err_msg=f.__name__)


def test_spec_gradient_matches_central_differences():
    x, y = FC.data(33)
    th = FC.theta(0)
    _, grad = F.loss_grad_eigen(x, y, th)
    for p in range(4):
        step = np.zeros(4)
        step[p] = 1e-5
        fd = (F.loss_grad_eigen(x, y, th + step)[0] - F.loss_grad_eigen(x, y, th - step)[0]) / 2e-5
        assert abs(fd - grad[p]) <= 1e-7 * max(1.0, np.max(np.abs(grad))), (p, fd, grad[p])


@pytest.mark.parametrize("n,h", FC.EVAL_CASES, ids=[FC.eval_id(n, h) for n, h in FC.EVAL_CASES])
def test_two_formulations_agree_and_the_spread_is_recorded(n, h):
    """Cholesky + autograd and the eigendecomposition closed form agree to 1e-10 (cond(K) <= (s N + noise) / noise <= 1.6e6 here),
    and the golden file holds spreads of the same order as the ones measured here (within 50x, floor 64 eps: BLAS builds differ
    in summation order)."""
    rec = FC.golden()["evaluations"][FC.eval_id(n, h)]
    ls, gs = FC.measured_eval_spread(n, h)
    lls, lgs = FC.measured_lapack_spread(n, h)
    print(FC.eval_id(n, h), "loss spread", ls, "gradient spread", gs, "two implementations", lls, lgs)
    assert max(ls, gs, lls, lgs) <= 1e-10
    assert max(rec["loss_spread"], rec["grad_spread"], rec["lapack_loss_spread"], rec["lapack_grad_spread"]) <= 1e-10
    assert ls <= 50 * max(rec["loss_spread"], FLOOR) and gs <= 50 * max(rec["grad_spread"], FLOOR)
    assert lls <= 50 * max(rec["lapack_loss_spread"], FLOOR) and lgs <= 50 * max(rec["lapack_grad_spread"], FLOOR)


def test_recorded_emulation_ratios_stay_below_four_times_the_yardstick():
    """every case of the golden file, the ones too large to re-run here included"""
    worst = [0.0, 0.0]
    for key, rec in FC.golden()["evaluations"].items():
        assert rec["emulation_loss_ratio_yardstick"] < 4.0 and rec["emulation_grad_ratio_yardstick"] < 4.0, key
        worst = [max(worst[0], rec["emulation_loss_ratio_yardstick"]), max(worst[1], rec["emulation_grad_ratio_yardstick"])]
    print("worst recorded emulation ratios: loss", worst[0], "gradient", worst[1])
    assert sorted(FC.golden()["evaluations"]) == sorted(FC.eval_id(n, h) for n, h in FC.EVAL_CASES)


@pytest.mark.parametrize("n,h", [c for c in FC.EVAL_CASES if c[0] <= FC.EMULATED_MAX], ids=[FC.eval_id(n, h) for n, h in FC.EVAL_CASES if n <= FC.EMULATED_MAX])
def test_kernel_formulation_stays_below_four_times_the_yardstick(n, h):
    """explicit L^-1, K^-1 = L^-T L^-1 tile by tile and the fixed reduction orders, against the Cholesky formulation: below 4 x
    the larger of the recorded two-formulation and two-implementation spreads, floor 64 eps / 4 (a quarter of the GPU bound)"""
    rec = FC.golden()["evaluations"][FC.eval_id(n, h)]
    el, eg = FC.emulation_distance(n, h)
    yl, yg = FC.yardstick(rec)
    print(FC.eval_id(n, h), "emulation / yardstick:", el / yl, eg / yg, "; / two-formulation spread:", el / max(rec["loss_spread"], 4 * EPS),
          eg / max(rec["grad_spread"], 4 * EPS))
    assert el <= max(4 * yl, FLOOR / 4) and eg <= max(4 * yg, FLOOR / 4)


@pytest.mark.parametrize("n,steps", FC.TRAJECTORIES, ids=[FC.traj_id(n, s) for n, s in FC.TRAJECTORIES])
def test_adam_trajectories_agree_between_formulations_and_with_torch(n, steps):
    """100 (or 25) Adam steps at lr 0.1 from theta = 0 stay positive definite without jitter; the two gradient formulations and
    torch.optim.Adam give the same trajectory to 1e-11, the recorded spread is of the measured order, and the fit works: the loss
    falls from about 1 by more than 1 (100 steps: to about -1.7)."""
    rec = FC.golden()["trajectories"][FC.traj_id(n, steps)]
    x, y = FC.data(n)
    th, losses = FC.expected_trajectory(n, steps)
    ts, ls = FC.measured_trajectory_spread(n, steps)
    tts, tls = F.trajectory_spread((th, losses), F.adam_torch(x, y, steps, lr=FC.LR))
    print(FC.traj_id(n, steps), "theta", th, "loss", losses[0], "->", losses[-1], "spread", ts, ls, "against torch.optim.Adam", tts, tls)
    assert np.isfinite(th).all() and np.isfinite(losses).all()
    assert max(ts, ls, tts, tls) <= 1e-11
    assert ts <= 50 * max(rec["theta_spread"], FLOOR) and ls <= 50 * max(rec["loss_spread"], FLOOR)
    assert 0.9 < losses[0] < 1.1 and losses[-1] < losses[0] - 1.0
    np.testing.assert_allclose(th, rec["theta"], rtol=0, atol=1e-9)
    if steps == 100:
        assert losses[-1] < -1.6 and th[2] > 6.0 and th[3] < -6.0
