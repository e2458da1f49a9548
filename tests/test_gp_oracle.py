"""CPU: the float64 specification of the GP slip regressor (gp_spec.py) against closed forms and against itself, the recorded
spreads of tests/golden/gp_slip.json, the host factorisation of benchnav_amd.gp, the state-dict parser and the input checks."""
import os

import numpy as np
import pytest
import torch

import gp_cases as GC
import gp_spec as S
from benchnav_amd import gp

EPS = np.finfo(np.float64).eps


def test_spec_closed_form_one_training_point():
    """N = 1: K = s + noise, so mean = c + k (y - c) / (s + noise) and var = s - k^2 / (s + noise) + noise."""
    x, y, c, s, l, noise = np.float32(3.5), np.float32(0.7), 0.1, 0.5, 5.0, 0.0025
    phi = np.array([3.5, -2.0, 0.0, 40.0])
    k = s * np.exp(-(phi - float(x)) ** 2 / (2 * l * l))
    mean = c + k * (float(y) - c) / (s + noise)
    std = np.sqrt(s - k * k / (s + noise) + noise)
    for f in (S.posterior_cholesky, S.posterior_eigen):
        m, sd = f([x], [y], c, s, l, noise, phi)
        np.testing.assert_allclose(m, mean, rtol=8 * EPS, atol=0)
        np.testing.assert_allclose(sd, std, rtol=64 * EPS, atol=0)    # s - k^2 / (s + noise) cancels two digits at phi = x


@pytest.mark.parametrize("n,h", [(5, 0), (67, 3), (130, 2)])
def test_spec_far_from_the_data_returns_the_prior(n, h):
    """A test point far from every training input: k(phi, x) underflows to 0, so mean = c and std = sqrt(s + noise) exactly."""
    x, y, c, s, l, noise, _ = GC.case(n, h)
    for f in (S.posterior_cholesky, S.posterior_eigen):
        m, sd = f(x, y, c, s, l, noise, [1e4, -1e4])
        assert np.all(m == c) and np.all(sd == np.sqrt(s + noise))


@pytest.mark.parametrize("n,h", GC.CASES, ids=[GC.case_id(n, h) for n, h in GC.CASES])
def test_two_formulations_agree_and_the_spread_is_recorded(n, h):
    """The Cholesky and the eigendecomposition evaluation agree to 1e-10 relative (cond(K) <= (s N + noise) / noise <= 3.1e6 here:
    a backward-stable solve loses at most cond * eps = 7e-10 and in practice far less), and the golden file holds a spread for
    the case of the same order as the one measured here (within 50x: BLAS builds differ in summation order)."""
    ms, ss = GC.measured_spread(n, h)
    print(GC.case_id(n, h), "mean spread", ms, "std spread", ss)
    assert ms <= 1e-10 and ss <= 1e-10
    rec = GC.golden()["cases"][GC.case_id(n, h)]
    assert rec["mean_spread"] <= 1e-10 and rec["std_spread"] <= 1e-10
    floor = 64 * EPS
    assert ms <= 50 * max(rec["mean_spread"], floor) and ss <= 50 * max(rec["std_spread"], floor)


def _kernel_formulation(n, h):
    """The device's formulation in NumPy: explicit L^-1 from gp.factorize, v = L^-1 k, |v|^2 summed in reversed order."""
    x, y, c, s, l, noise, phi = GC.case(n, h)
    xs, alpha, linv = gp.factorize(x, y, c, s, l, noise)
    d = phi.astype(np.float64)[None, :] - xs[:, None]
    ks = s * np.exp((d * d) * (-1.0 / (2.0 * l * l)))
    v = linv @ ks
    mean = c + (ks[::-1] * alpha[::-1, None]).sum(axis=0)
    var = np.maximum(s - (v[::-1] ** 2).sum(axis=0), 0.0) + noise
    return mean, np.sqrt(var)


@pytest.mark.parametrize("n,h", GC.CASES, ids=[GC.case_id(n, h) for n, h in GC.CASES])
def test_host_factorisation_and_the_kernel_formulation(n, h):
    """gp.factorize: L^-1 K L^-T = I to 1e-9, alpha = K^-1 (y - c), L^-1 lower triangular; and the device's formulation evaluated
    with it in NumPy stays within the GPU test's float64 bound (16 x the recorded spread, floor 64 eps) of the spec."""
    x, y, c, s, l, noise, _ = GC.case(n, h)
    xs, alpha, linv = gp.factorize(x, y, c, s, l, noise)
    assert xs.dtype == alpha.dtype == linv.dtype == np.float64 and linv.shape == (n, n) and linv.flags.c_contiguous
    assert np.array_equal(xs, x.astype(np.float64)) and np.all(np.triu(linv, 1) == 0)
    K = S.kernel(xs, xs, s, l) + noise * np.eye(n)
    assert np.max(np.abs(linv @ K @ linv.T - np.eye(n))) <= 1e-9
    resid = K @ alpha - (y.astype(np.float64) - c)
    assert np.max(np.abs(resid)) <= 1e-9 * max(1.0, np.max(np.abs(y)))
    rec = GC.golden()["cases"][GC.case_id(n, h)]
    ms, ss = S.spread(GC.expected(n, h), _kernel_formulation(n, h))
    print(GC.case_id(n, h), "kernel formulation / recorded spread:", ms / max(rec["mean_spread"], 4 * EPS), ss / max(rec["std_spread"], 4 * EPS))
    assert ms <= max(16 * rec["mean_spread"], 64 * EPS) and ss <= max(16 * rec["std_spread"], 64 * EPS)


def test_state_dict_parser_reproduces_hand_set_hyperparameters():
    """A hand-built dictionary with gpytorch's documented key names: raw = inverse softplus of the wanted value (noise: of the
    value minus the lower bound)."""
    def raw(v):
        return float(np.log(np.expm1(v)))
    want = {"constant": -0.125, "outputscale": 0.37, "lengthscale": 4.5, "noise": 0.0125}
    sd = {"likelihood.noise_covar.raw_noise": torch.tensor([raw(want["noise"] - 1e-4)], dtype=torch.float64),
          "likelihood.noise_covar.raw_noise_constraint.lower_bound": torch.tensor(1e-4, dtype=torch.float64),
          "likelihood.noise_covar.raw_noise_constraint.upper_bound": torch.tensor(float("inf")),
          "mean_module.raw_constant": torch.tensor(want["constant"], dtype=torch.float64),
          "covar_module.raw_outputscale": torch.tensor(raw(want["outputscale"]), dtype=torch.float64),
          "covar_module.base_kernel.raw_lengthscale": torch.tensor([[raw(want["lengthscale"])]], dtype=torch.float64),
          "covar_module.base_kernel.raw_lengthscale_constraint.lower_bound": torch.tensor(0.0),
          "covar_module.raw_outputscale_constraint.lower_bound": torch.tensor(0.0)}
    got = gp.hyperparameters_from_state_dict(sd)
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, got[k], v)
    # the older ConstantMean key, no stored bound (default 1e-4), float32 storage
    old = {"likelihood.noise_covar.raw_noise": torch.tensor([0.0]), "mean_module.constant": torch.tensor([0.25]),
           "covar_module.raw_outputscale": torch.tensor(0.0), "covar_module.base_kernel.raw_lengthscale": torch.tensor([[0.0]])}
    got = gp.hyperparameters_from_state_dict(old)
    assert got["constant"] == 0.25 and abs(got["outputscale"] - np.log(2.0)) < 1e-15 and abs(got["lengthscale"] - np.log(2.0)) < 1e-15
    assert abs(got["noise"] - (np.log(2.0) + 1e-4)) < 1e-15
    assert abs(gp.hyperparameters_from_state_dict(old, noise_lower_bound=0.0)["noise"] - np.log(2.0)) < 1e-15
    with pytest.raises(ValueError, match="raw_outputscale"):
        gp.hyperparameters_from_state_dict({k: v for k, v in old.items() if k != "covar_module.raw_outputscale"})


def test_invalid_inputs_raise():
    x, y = np.linspace(-5, 5, 8, dtype=np.float32), np.zeros(8, np.float32)
    ok = dict(constant=0.0, outputscale=0.5, lengthscale=5.0, noise=0.01)
    gp.factorize(x, y, **ok)
    for bad in (dict(outputscale=0.0), dict(lengthscale=-1.0), dict(noise=0.0), dict(noise=float("nan")), dict(constant=float("inf"))):
        with pytest.raises(ValueError):
            gp.factorize(x, y, **{**ok, **bad})
    with pytest.raises(ValueError, match="differ in length"):
        gp.factorize(x, y[:5], **ok)
    with pytest.raises(ValueError, match="finite"):
        gp.factorize(np.float32([0.0, np.nan]), y[:2], **ok)
    with pytest.raises(ValueError, match=str(gp.MAX_POINTS)):
        gp.factorize(np.zeros(gp.MAX_POINTS + 1, np.float32), np.zeros(gp.MAX_POINTS + 1, np.float32), **ok)
    with pytest.raises(ValueError, match=str(gp.MAX_POINTS)):
        gp.factorize(np.zeros(0, np.float32), np.zeros(0, np.float32), **ok)
    with pytest.raises(ValueError, match="one-dimensional"):
        gp.factorize(np.zeros((4, 2), np.float32), np.zeros(4, np.float32), **ok)
    # no jitter: duplicated inputs under a noise far below eps * s make k(x, x) + noise I numerically singular
    with pytest.raises(ValueError, match="positive definite"):
        gp.factorize(np.zeros(6, np.float32), np.zeros(6, np.float32), constant=0.0, outputscale=1.0, lengthscale=1.0, noise=1e-300)
    # the constructor checks its inputs before it looks for a device
    with pytest.raises(ValueError):
        gp.GPSlipRegressor(x, y, 0.0, 0.5, 5.0, -1.0)


def test_load_slip_regressors_reads_the_reference_layout_with_weights_only(tmp_path, monkeypatch):
    """trainers/utils.py:65-108: <train>/slip_observations/<i:02d>_class.pth and <models>/models/<i:02d>_class.pth; the loader
    hands the parsed hyperparameters and the float32 data to the regressor (constructed here without a device)."""
    made = []

    class Fake:
        def __init__(self, train_x, train_y, device=None, **hyper):
            made.append((np.asarray(train_x), np.asarray(train_y), hyper))
    monkeypatch.setattr(gp.GPSlipRegressor, "from_gpytorch_state_dict",
                        classmethod(lambda cls, sd, tx, ty, device=None: Fake(tx, ty, device=device, **gp.hyperparameters_from_state_dict(sd))))
    os.makedirs(tmp_path / "data" / "slip_observations")
    os.makedirs(tmp_path / "learned" / "models")
    for i in range(2):
        torch.save({"train_x": torch.arange(4.0) + i, "train_y": torch.ones(4) * i}, tmp_path / "data" / "slip_observations" / f"{i:02d}_class.pth")
        torch.save({"likelihood.noise_covar.raw_noise": torch.tensor([0.0]), "mean_module.raw_constant": torch.tensor(0.5 * i),
                    "covar_module.raw_outputscale": torch.tensor(0.0), "covar_module.base_kernel.raw_lengthscale": torch.tensor([[1.0]])},
                   tmp_path / "learned" / "models" / f"{i:02d}_class.pth")
    out = gp.load_slip_regressors(2, str(tmp_path / "learned"), str(tmp_path / "data"))
    assert sorted(out) == [0, 1] and len(made) == 2
    assert np.array_equal(made[1][0], np.arange(4.0) + 1) and made[1][2]["constant"] == 0.5
    assert abs(made[0][2]["lengthscale"] - np.log1p(np.e)) < 1e-12
