"""GPU: fitting the GP slip regressors on the device (benchnav_amd/gp.py, csrc/gp_fit_kernels.hip) against the
float64 specification (tests/gp_fit_spec.py on the cases of tests/gp_fit_cases.py): the single evaluation of loss and gradient,
the Adam trajectory, the handle a fit and a device factorisation hand to the predict kernels, the failure path and the
trainer's round trip through the reference's file layout.

Bounds: loss, gradient, theta and loss history within 16 x the case's recorded two-formulation spread (tests/golden/gp_fit.json),
floor 64 eps, in gp_fit_spec's measures (eval_spread, trajectory_spread); predictions of a fitted handle within the bounds of
tests/test_gpu_gp.py against gp_spec.posterior_cholesky at the hyperparameters read back from the handle: float32 outputs within
1 ulp of the rounded spec, float64 outputs within 16 x the spread of the two posterior formulations at those hyperparameters."""
import types

import numpy as np
import pytest
import torch

import gp_cases as GC
import gp_fit_cases as FC
import gp_fit_spec as F
import gp_spec as S

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G0 = 16


def _fit(n, lower_bound=F.LOWER_BOUND):
    from benchnav_amd import _capi, gp
    x, y = FC.data(n)
    return gp._Fit(_capi.load(), torch.device("cuda", torch.cuda.current_device()), F.widen(x), F.widen(y), lower_bound)


def _ulps(dev: np.ndarray, want: np.ndarray) -> np.ndarray:
    d = np.abs(dev.astype(np.float64) - want.astype(np.float64))
    return d / np.spacing(np.maximum(np.abs(dev), np.abs(want)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("n,h", FC.EVAL_CASES, ids=[FC.eval_id(n, h) for n, h in FC.EVAL_CASES])
def test_single_evaluation_matches_the_float64_spec(n, h):
    rec = FC.golden()["evaluations"][FC.eval_id(n, h)]
    want = FC.expected_eval(n, h)
    with _fit(n) as fit:
        fit.set_raw(FC.theta(h))
        fit.evaluate()
        raw, grad, loss, status, failed = fit.read()
        assert fit.history().size == 0                                  # an evaluation is no iteration
    assert status == 0 and failed == -1 and np.array_equal(raw, FC.theta(h))
    ls, gs = F.eval_spread(want, (loss, grad))
    print(f"{FC.eval_id(n, h)}: loss {loss:.17g} spread {ls:.3g} gradient spread {gs:.3g} = "
          f"{ls / max(rec['loss_spread'], 4 * EPS):.3g} x / {gs / max(rec['grad_spread'], 4 * EPS):.3g} x the recorded spread")
    assert ls <= max(16 * rec["loss_spread"], 64 * EPS)
    assert gs <= max(16 * rec["grad_spread"], 64 * EPS)


@pytest.mark.parametrize("n,steps", FC.TRAJECTORIES, ids=[FC.traj_id(n, s) for n, s in FC.TRAJECTORIES])
def test_adam_trajectory_matches_the_float64_spec_and_repeats_bit_for_bit(n, steps):
    from benchnav_amd.gp import GPSlipRegressor
    rec = FC.golden()["trajectories"][FC.traj_id(n, steps)]
    want = FC.expected_trajectory(n, steps)
    x, y = FC.data(n)
    a = GPSlipRegressor.fit(x, y, learning_rate=FC.LR, num_iterations=steps)
    b = GPSlipRegressor.fit(x, y, learning_rate=FC.LR, num_iterations=steps)
    assert a.loss_history.dtype == np.float64 and a.loss_history.shape == (steps,) and a.raw_parameters.shape == (4,)
    ts, ls = F.trajectory_spread(want, (a.raw_parameters, a.loss_history))
    print(f"{FC.traj_id(n, steps)}: theta {a.raw_parameters} loss {a.loss_history[0]:.6g} -> {a.loss_history[-1]:.6g}; theta spread {ts:.3g} "
          f"loss spread {ls:.3g} = {ts / max(rec['theta_spread'], 4 * EPS):.3g} x / {ls / max(rec['loss_spread'], 4 * EPS):.3g} x the recorded spread")
    phi = torch.from_numpy(GC.case(n, 0)[6].copy()).cuda().reshape(G0, G0)
    pa, pb = a.predict_tensors(phi, dtype=torch.float64), b.predict_tensors(phi, dtype=torch.float64)
    same = (np.array_equal(a.raw_parameters.view(np.uint64), b.raw_parameters.view(np.uint64))
            and np.array_equal(a.loss_history.view(np.uint64), b.loss_history.view(np.uint64))
            and torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]))
    hyp = F.hyper(a.raw_parameters)
    got = (a.constant, a.outputscale, a.lengthscale, a.noise)
    a.close()
    b.close()
    assert same, "two fits of the same data differ in their bits"
    assert np.allclose(got, hyp, rtol=8 * EPS, atol=0)
    assert ts <= max(16 * rec["theta_spread"], 64 * EPS)
    assert ls <= max(16 * rec["loss_spread"], 64 * EPS)


def _check_predictions(reg, x, y, phi, label):
    """reg against gp_spec.posterior_cholesky at the hyperparameters read back from it"""
    c, s, l, noise = reg.constant, reg.outputscale, reg.lengthscale, reg.noise
    want = S.posterior_cholesky(x, y, c, s, l, noise, phi)
    sm, ss = S.spread(want, S.posterior_eigen(x, y, c, s, l, noise, phi))
    t = torch.from_numpy(np.asarray(phi, np.float32).copy()).cuda().reshape(G0, G0)
    m32, s32 = reg.predict_tensors(t)
    m64, s64 = reg.predict_tensors(t, dtype=torch.float64)
    um = _ulps(m32.cpu().numpy().reshape(-1), want[0].astype(np.float32))
    us = _ulps(s32.cpu().numpy().reshape(-1), want[1].astype(np.float32))
    dm, ds = S.spread(want, (m64.cpu().numpy().reshape(-1), s64.cpu().numpy().reshape(-1)))
    print(f"{label}: float32 ulps mean {um.max():.3g} std {us.max():.3g}; float64 spread mean {dm:.3g} std {ds:.3g} = "
          f"{dm / max(sm, 4 * EPS):.3g} x / {ds / max(ss, 4 * EPS):.3g} x the two posterior formulations' spread")
    assert um.max() <= 1.0 and us.max() <= 1.0, label
    assert dm <= max(16 * sm, 64 * EPS) and ds <= max(16 * ss, 64 * EPS), label


@pytest.mark.parametrize("n", FC.SIZES)
def test_fitted_and_device_factorised_handles_predict_within_the_existing_bounds(n):
    from benchnav_amd.gp import GPSlipRegressor
    x, y = FC.data(n)
    phi = GC.case(n, 0)[6]
    fitted = GPSlipRegressor.fit(x, y, learning_rate=FC.LR, num_iterations=3)
    assert fitted.num_points == n and fitted.loss_history.shape == (3,)
    _check_predictions(fitted, x, y, phi, f"n{n} fit")
    fitted.close()
    for h in (0, 3):
        cx, cy, c, s, l, noise, cphi = GC.case(n, h)
        reg = GPSlipRegressor(cx, cy, c, s, l, noise, factorization="device")
        assert (reg.constant, reg.outputscale, reg.lengthscale, reg.noise) == (c, s, l, noise) and reg.raw_parameters is None
        _check_predictions(reg, cx, cy, cphi, f"n{n}_h{h} device")
        reg.close()


def test_a_predictor_serves_host_and_device_factorised_classes_in_one_map():
    from benchnav_amd.gp import GPSlipRegressor, TraversabilityPredictor
    x0, y0, c0, s0, l0, n0, _ = GC.case(67, 0)
    x1, y1, c1, s1, l1, n1, _ = GC.case(130, 1)
    regs = {0: GPSlipRegressor(x0, y0, c0, s0, l0, n0), 1: GPSlipRegressor(x1, y1, c1, s1, l1, n1, factorization="device")}
    rng = np.random.default_rng(21)
    G = 24
    cls = torch.from_numpy(rng.integers(0, 3, (G, G)))              # class 2 has no regressor
    slopes = torch.from_numpy(rng.uniform(-30, 30, (G, G)).astype(np.float32)).cuda()
    pred = TraversabilityPredictor(None, regs)
    for dtype in (torch.float32, torch.float64):
        mean, std = pred.predict_maps(slopes, t_classes=cls, dtype=dtype)
        for k, r in regs.items():
            mask = (cls == k).cuda()
            wm, ws = r.predict_tensors(slopes[mask], dtype=dtype)
            assert mask.any() and torch.equal(mean[mask], wm) and torch.equal(std[mask], ws)
        none = (cls == 2).cuda()
        assert not mean[none].any() and not std[none].any()
    for r in regs.values():
        r.close()


def test_a_zero_pivot_raises_reports_its_status_and_leaves_the_device_usable():
    """Two equal inputs with s = 1, l = 1, noise = 1e-300: K = [[1, 1], [1, 1]] in IEEE arithmetic, the second pivot is exactly 0."""
    from benchnav_amd import _capi, gp
    x = y = np.zeros(2, np.float32)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(np.ones((2, 2)) + 1e-300 * np.eye(2))
    with pytest.raises(ValueError, match=r"iteration 0 \(no jitter is added\)"):
        gp.GPSlipRegressor(x, y, 0.0, 1.0, 1.0, 1e-300, factorization="device")
    lib = _capi.load()
    with gp._Fit(lib, torch.device("cuda", torch.cuda.current_device()), np.zeros(2), np.zeros(2), F.LOWER_BOUND) as fit:
        gp._check_fit(lib, lib.bn_gp_fit_set_hyperparameters(fit.handle, 0.0, 1.0, 1.0, 1e-300))
        fit.evaluate()
        raw, grad, loss, status, failed = fit.read()
        assert status == 1 and failed == 0
        assert loss == 0.0 and not grad.any()                       # the kernels behind the failing one wrote nothing
        fit.run(2, 0.1)                                             # enqueued behind the failure: every launch returns at once
        assert fit.read()[3:] == (1, 0) and fit.history().size == 0
        with pytest.raises(ValueError, match="no jitter is added"):
            fit.finish()
        fit.set_raw(np.zeros(4))                                    # a new start on the same handle
        fit.run(2, 0.1)
        assert fit.read()[3:] == (0, -1) and fit.history().size == 2
    with pytest.raises(ValueError, match=r"iteration 1 \(no jitter is added\)"):
        # theta = 0 is positive definite; Adam's first step is -lr sign(gradient), and the gradients of the raw outputscale and
        # the raw noise are positive here (alpha = 0), so a step of 1e3 takes both to -1000: softplus underflows to 0, K = 0
        gp.GPSlipRegressor.fit(x, y, learning_rate=1e3, num_iterations=3, noise_lower_bound=0.0)
    x5, y5 = FC.data(33)
    ok = gp.GPSlipRegressor.fit(x5, y5, num_iterations=2)
    assert np.isfinite(ok.loss_history).all() and ok.loss_history.shape == (2,)
    ok.close()


class _Params:
    batch_size, learning_rate, num_iterations = 2, 0.1, 5


def test_trainer_round_trip_through_the_reference_layout(tmp_path):
    from benchnav_amd import gp
    rng = np.random.default_rng(9)
    M, G = 4, 16
    slopes = torch.from_numpy(rng.uniform(-30, 30, (M, G, G)).astype(np.float32))
    classes = torch.from_numpy(rng.integers(0, 2, (M, G, G)))
    gain = torch.where(classes == 0, 0.3, 0.6)
    slips = torch.clamp(gain * torch.tanh(slopes / 12.0) + 0.3 + 0.05 * torch.from_numpy(rng.standard_normal((M, G, G)).astype(np.float32)), 0.0, 1.0)
    ds = torch.utils.data.TensorDataset(slopes, slips, classes)
    torch.manual_seed(3)
    trainer = gp.SlipRegressorTrainer(None, str(tmp_path / "models"), str(tmp_path / "data"), 2, _Params, ds)
    trainer.train_all_models()
    assert trainer.model_directory.endswith("lr1e-01_iters005")
    regs = gp.load_slip_regressors(2, trainer.model_directory, str(tmp_path / "data"))
    phi = GC.case(130, 0)[6]
    for k in range(2):
        data = torch.load(tmp_path / "data" / "slip_observations" / f"{k:02d}_class.pth", weights_only=True)
        state = torch.load(tmp_path / "models" / "lr1e-01_iters005" / "models" / f"{k:02d}_class.pth", weights_only=True)
        assert data["train_x"].numel() == int((classes == k).sum()) and all(v.dtype == torch.float32 for v in state.values())
        hyp = gp.hyperparameters_from_state_dict(state)
        assert (regs[k].constant, regs[k].outputscale, regs[k].lengthscale, regs[k].noise) == tuple(hyp[n] for n in ("constant", "outputscale", "lengthscale", "noise"))
        want_raw = np.float32(trainer.regressors[k].raw_parameters)
        got_raw = np.float32([float(state[key].reshape(())) for key in ("mean_module.raw_constant", "covar_module.raw_outputscale",
                                                                        "covar_module.base_kernel.raw_lengthscale", "likelihood.noise_covar.raw_noise")])
        assert np.array_equal(want_raw, got_raw)
        _check_predictions(regs[k], data["train_x"].numpy(), data["train_y"].numpy(), phi, f"trainer class {k}")
    for r in list(regs.values()) + list(trainer.regressors.values()):
        r.close()
