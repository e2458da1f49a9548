"""Risk-map precompute ("next" row N1): TraversabilityModel._infer_risk_map (traversability_model.py:28-51).
CPU: the NumPy oracle against the reference fixture.  GPU: the HIP kernel against the oracle and the fixture."""
import os

import numpy as np
import pytest

from helpers import GOLDEN_DIR
from oracle import risk_oracle as RO


def _fx():
    z = np.load(os.path.join(GOLDEN_DIR, "riskmap.npz"))
    return {k: z[k] for k in z.files}


def _keys(fx):
    return [(k, k[2:].split("_")[0], float(k[2:].split("_")[1])) for k in fx if k.startswith("R_")]


def test_oracle_matches_reference_risk_maps():
    fx = _fx()
    for key, metric, q in _keys(fx):
        got = RO.infer_risk_map(fx["mean"], fx["std"], metric, q, fx["z"])
        if metric == "var":
            assert np.array_equal(got, fx[key]), key                 # selection + torch's fused lerp (test_risk_oracle_torch.py)
        else:
            assert np.abs(got - fx[key]).max() <= 5e-7, key          # tail mean: summation order only
    assert np.array_equal(RO.infer_risk_map(fx["mean"], fx["std"], "expected_value"), fx["mean"])


@pytest.mark.gpu
def test_kernel_matches_oracle_and_reference_with_the_reference_draw():
    import torch
    from benchnav_amd.risk import infer_risk_map
    fx = _fx()
    mean, std, z = torch.from_numpy(fx["mean"]), torch.from_numpy(fx["std"]), torch.from_numpy(fx["z"])
    for key, metric, q in _keys(fx):
        got = infer_risk_map(mean, std, metric, q, num_samples=int(fx["n"]), z=z).cpu().numpy()
        orc = RO.infer_risk_map(fx["mean"], fx["std"], metric, q, fx["z"])
        if metric == "var":
            assert np.array_equal(got, orc) and np.array_equal(got, fx[key]), key
        else:
            assert np.abs(got - orc).max() <= 5e-7 and np.abs(got - fx[key]).max() <= 5e-7, key
    ev = infer_risk_map(mean, std, "expected_value")
    assert torch.equal(ev.cpu(), mean)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 1500, 3000])
def test_kernel_sampling_mode_matches_the_gaussian_closed_form(n):
    """In-kernel Philox draws: VaR_q -> mean + std * Phi^-1(q), CVaR_q -> mean + std * phi(Phi^-1(q)) / (1 - q),
    within sampling error of n draws per cell (averaged over a 64x64 map the bias must vanish)."""
    import torch
    from scipy.stats import norm
    from benchnav_amd.risk import infer_risk_map
    G, q = 64, 0.9
    mean = torch.full((G, G), 0.4)
    std = torch.full((G, G), 0.1)
    zq = norm.ppf(q)
    var = infer_risk_map(mean, std, "var", q, num_samples=n, seed=3).cpu().numpy()
    cvar = infer_risk_map(mean, std, "cvar", q, num_samples=n, seed=3).cpu().numpy()
    assert abs(var.mean() - (0.4 + 0.1 * zq)) < 1.5e-3 and var.std() < 0.1 * 2.0 / np.sqrt(n) * 1.5
    assert abs(cvar.mean() - (0.4 + 0.1 * norm.pdf(zq) / (1 - q))) < 2e-3
    assert (cvar > var).all()
    other = infer_risk_map(mean, std, "var", q, num_samples=n, seed=4).cpu().numpy()
    assert not np.array_equal(var, other)


@pytest.mark.gpu
def test_risk_map_feeds_the_planner_like_the_reference_constructor():
    """cvar map -> MPPI: the constructor path of test_mppi.py:146-169 (UnicycleModel.__init__ runs _infer_risk_map)."""
    import torch
    from benchnav_amd.risk import infer_risk_map
    from benchnav_amd import NativeMPPI, synth
    G = 64
    mean = synth.smooth_risk_map(G, 4) * 0.7
    std = synth.slip_std_map(G, 4)
    R = infer_risk_map(mean, std, "cvar", 0.9, num_samples=1000, seed=1)
    assert R.shape == (G, G) and torch.isfinite(R).all() and (R > mean.cuda()).all()
    with NativeMPPI(horizon=20, num_samples=256, grid_size=G, resolution=0.5) as pl:
        pl.set_map(R.cpu().numpy()); pl.set_goal([24.0, 24.0])
        us, xs = pl.solve([8.0, 8.0, 0.7])
        assert np.isfinite(us).all() and np.isfinite(xs).all()


def test_metric_and_confidence_are_validated_like_model_config():
    import torch
    from benchnav_amd.risk import infer_risk_map
    m = torch.zeros(4, 4)
    with pytest.raises(AssertionError):
        infer_risk_map(m, m, "median")
    with pytest.raises(AssertionError):
        infer_risk_map(m, m, "var", None)
    with pytest.raises(AssertionError):
        infer_risk_map(m, m, "cvar", 1.5)
