"""CPU: the GP slip regressor above 1024 training points (tests/gp_large_cases.py): benchnav_amd.gp.factorize takes the sizes, a
NumPy emulation of gp_slab_kernel's formulation (slabs of 32 row blocks, ascending k per row block, the kernel's fold order) stays
within the GPU test's float64 bound of the spec, and load_slip_regressors hands small and large classes to the regressor."""
import os

import numpy as np
import pytest
import torch

import gp_large_cases as LC
import gp_spec as S
from benchnav_amd import gp

EPS = np.finfo(np.float64).eps


def test_golden_file_holds_every_case_and_the_emulation_left_the_margin():
    """The recorded two-formulation spreads are of the order cond(K) eps allows (<= 1e-10, as at the small sizes), and the
    emulation was recorded below 4 x the spread: the 16 x of DESIGN.md 4.9 keeps its room for the device's exp and MFMA order."""
    rec = LC.golden()["cases"]
    assert sorted(rec) == sorted(LC.case_id(n, h) for n, h in LC.CASES)
    for k, v in rec.items():
        assert 0 < v["mean_spread"] <= 1e-10 and 0 < v["std_spread"] <= 1e-10, k
        assert v["emulation_mean_multiple"] <= 4.0 and v["emulation_std_multiple"] <= 4.0, (k, v)


@pytest.mark.parametrize("n,h", LC.CASES, ids=[LC.case_id(n, h) for n, h in LC.CASES])
def test_factorize_takes_the_size_and_the_slab_formulation_stays_within_the_spec(n, h):
    x, y, c, s, l, noise, _ = LC.case(n, h)
    xs, alpha, linv = gp.factorize(x, y, c, s, l, noise)
    assert xs.dtype == alpha.dtype == linv.dtype == np.float64 and linv.shape == (n, n) and linv.flags.c_contiguous
    assert np.array_equal(xs, x.astype(np.float64)) and np.all(np.triu(linv, 1) == 0)
    K = S.kernel(xs, xs, s, l) + noise * np.eye(n)
    assert np.max(np.abs(linv @ K @ linv.T - np.eye(n))) <= 1e-9
    resid = K @ alpha - (y.astype(np.float64) - c)
    assert np.max(np.abs(resid)) <= 1e-9 * max(1.0, np.max(np.abs(y)))
    rec = LC.golden()["cases"][LC.case_id(n, h)]
    ms, ss = S.spread(LC.expected(n, h), LC.slab_formulation(n, h))
    print(LC.case_id(n, h), "slab formulation / recorded spread:", ms / max(rec["mean_spread"], 4 * EPS), ss / max(rec["std_spread"], 4 * EPS))
    assert ms <= max(16 * rec["mean_spread"], 64 * EPS) and ss <= max(16 * rec["std_spread"], 64 * EPS)


def test_factorize_small_sizes_keep_their_numpy_path():
    """N <= 1024 goes through np.linalg.solve(L, I) as before: the same L^-1 bits as the formula written out here."""
    x, y, c, s, l, noise, _ = LC.case(130, 3)
    _, _, linv = gp.factorize(x, y, c, s, l, noise)
    xs = x.astype(np.float64)
    d = xs[:, None] - xs[None, :]
    L = np.linalg.cholesky(s * np.exp(-(d * d) / (2.0 * l * l)) + noise * np.eye(130))
    assert np.array_equal(linv, np.tril(np.linalg.solve(L, np.eye(130))))


def test_factorize_rejects_out_of_range_sizes_before_it_builds_k(monkeypatch):
    def no_k(*a, **k):
        raise AssertionError("K was built")
    monkeypatch.setattr(np.linalg, "cholesky", no_k)
    monkeypatch.setattr(np, "exp", no_k)
    ok = dict(constant=0.0, outputscale=0.5, lengthscale=5.0, noise=0.01)
    for n in (0, gp.MAX_POINTS + 1):
        with pytest.raises(ValueError, match="takes 1 to 10240 training points"):
            gp.factorize(np.zeros(n, np.float32), np.zeros(n, np.float32), **ok)


def test_load_slip_regressors_hands_over_small_and_large_classes(tmp_path, monkeypatch):
    """Class 0 with 130 observations and class 1 with 2000 in the reference's file layout: both reach the regressor whole."""
    made = []

    class Fake:
        def __init__(self, train_x, train_y, device=None, **hyper):
            made.append((np.asarray(train_x), np.asarray(train_y), hyper))
    monkeypatch.setattr(gp.GPSlipRegressor, "from_gpytorch_state_dict",
                        classmethod(lambda cls, sd, tx, ty, device=None: Fake(tx, ty, device=device, **gp.hyperparameters_from_state_dict(sd))))
    os.makedirs(tmp_path / "data" / "slip_observations")
    os.makedirs(tmp_path / "learned" / "models")
    sizes = (130, 2000)
    for i, n in enumerate(sizes):
        torch.save({"train_x": torch.linspace(-30.0, 30.0, n) + i, "train_y": torch.full((n,), 0.25 * i)},
                   tmp_path / "data" / "slip_observations" / f"{i:02d}_class.pth")
        torch.save({"likelihood.noise_covar.raw_noise": torch.tensor([0.0]), "mean_module.raw_constant": torch.tensor(0.5 * i),
                    "covar_module.raw_outputscale": torch.tensor(0.0), "covar_module.base_kernel.raw_lengthscale": torch.tensor([[1.0]])},
                   tmp_path / "learned" / "models" / f"{i:02d}_class.pth")
    out = gp.load_slip_regressors(2, str(tmp_path / "learned"), str(tmp_path / "data"))
    assert sorted(out) == [0, 1] and [m[0].shape[0] for m in made] == list(sizes)
    assert np.array_equal(made[1][0], (torch.linspace(-30.0, 30.0, 2000) + 1).numpy()) and made[1][2]["constant"] == 0.5
    # and the host side of the real constructor takes both sizes
    for tx, ty, hyper in made:
        xs, alpha, linv = gp.factorize(tx, ty, **hyper)
        assert linv.shape == (tx.shape[0],) * 2 and np.isfinite(alpha).all()
