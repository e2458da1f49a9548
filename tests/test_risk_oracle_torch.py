"""CPU: oracle/risk_oracle.py against the reference's own three lines, restated with torch calls on CPU float32 tensors:

    var  = torch.quantile(samples, q, dim=0)
    cvar = torch.nanmean(torch.where(samples > var, samples, nan), dim=0)

over every case of tests/risk_cases.py.  VaR is compared by value (the sign of a zero picked among tied +-0 is not defined by
either sort), CVaR by its NaN pattern and by the derived summation bound against a float64 tail mean.  The GPU kernel is held to
the oracle in test_gpu_risk_edges.py; this file is what ties the oracle to torch."""
import numpy as np
import pytest
import torch

import risk_cases as RC
from oracle import risk_oracle as RO

f32 = np.float32


def _torch_reference(smp, q):
    s = torch.from_numpy(np.ascontiguousarray(smp))
    var = torch.quantile(s, q, dim=0)
    cvar = torch.nanmean(torch.where(s > var, s, torch.tensor(float("nan"))), dim=0)
    return var.numpy(), cvar.numpy()


def _same_value(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def test_fma32_rounds_once():
    """4097 * 16773121 = 2^36 + 1 exactly.  Added to 2^60 (float32 spacing 2^37) the sum lies just above the midpoint 2^60 + 2^36:
    one rounding goes up to 2^60 + 2^37.  A float64 add drops the 1 (spacing 2^8), lands on the midpoint and rounds to even, 2^60."""
    assert 4097 * 16773121 == 2 ** 36 + 1
    assert RO.fma32(4097.0, 16773121.0, 2.0 ** 60) == f32(2.0 ** 60 + 2.0 ** 37)
    assert RO.fma32(4097.0, -16773121.0, -2.0 ** 60) == f32(-(2.0 ** 60 + 2.0 ** 37))
    assert RO.fma32(4097.0, 16773120.0, 2.0 ** 60) == f32(2.0 ** 60)                   # 2^36 - 4096: below the midpoint
    assert f32(np.float64(4097.0 * 16773121.0) + 2.0 ** 60) == f32(2.0 ** 60)          # the double rounding this avoids
    # exact rational arithmetic on random operands, cancellation included
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(f32)
    b = (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(f32)
    c = np.where(rng.random(4000) < 0.5, -(a * b).astype(f32), rng.standard_normal(4000).astype(f32)).astype(f32)
    got = RO.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        assert abs(Fraction(float(g)) - exact) <= Fraction(float(np.spacing(np.abs(g)))) / 2, (x, y, z, g)
    assert np.isnan(RO.fma32(0.5, np.inf - np.inf, np.inf)) and RO.fma32(0.0, 1.0, -0.0) == 0


@pytest.mark.parametrize("variant", RC.VARIANTS)
@pytest.mark.parametrize("n", RC.NS)
def test_oracle_equals_torch_quantile_and_nanmean(n, variant):
    mean, std = RC.maps()
    z = RC.draws(n, variant)
    smp = RC.samples(n, variant)
    worst = 0.0
    for q in RC.QS:
        tv, tc = _torch_reference(smp, q)
        var = RO.infer_risk_map(mean, std, "var", q, z)
        bad = ~_same_value(var, tv)
        assert not bad.any(), f"n={n} q={q} {variant}: VaR differs from torch.quantile in cells {np.argwhere(bad).tolist()}"
        cvar = RO.infer_risk_map(mean, std, "cvar", q, z)
        assert np.array_equal(np.isnan(cvar), np.isnan(tc)), f"n={n} q={q} {variant}: CVaR NaN pattern"
        ref64, scale = RC.tail_mean64(smp, tv)
        fin = ~np.isnan(tc)
        assert np.array_equal(fin, ~np.isnan(ref64))
        if fin.any():
            err = np.abs(cvar.astype(np.float64) - ref64)[fin]
            bound = RC.cvar_bound(n, scale)[fin]
            assert (err <= bound).all(), f"n={n} q={q} {variant}: CVaR {err.max():.3g} over its bound"
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    print(f"\noracle vs torch n={n} {variant}: VaR equal in all cells, CVaR error / bound max {worst:.3f}")


def test_the_cases_reach_what_they_are_for():
    """Both lerp branches, w = 0, first and last rank, tied ranks lo / hi, mixed signed zeros, all-negative and mixed-sign keys."""
    ws = {(n, q): RC.rank(q, n) for n in RC.NS for q in RC.QS}
    assert any(0 < w < 0.5 for _, _, w in ws.values()) and any(w >= 0.5 and w != 0.5 for _, _, w in ws.values())
    assert any(w == 0.5 for _, _, w in ws.values())
    for n in RC.NS:
        assert ws[(n, 0.0)] == (0, 0, 0) and ws[(n, 1.0)] == (n - 1, n - 1, 0)
        assert RC.capacity(n) * 64 >= n
    smp = RC.samples(1000, "halves").reshape(1000, -1)
    srt = np.sort(smp, axis=0)
    lo, hi, _ = RC.rank(0.9, 1000)
    row = slice(RC.HALVES_ROW * RC.G, (RC.HALVES_ROW + 1) * RC.G)
    assert hi == lo + 1 and (srt[lo, row] == srt[hi, row]).all()
    zc = smp[:, RC.NAMED["signed_zeros"][0]]
    assert (zc == 0).all() and np.signbit(zc).any() and not np.signbit(zc).all()
    assert (smp[:, RC.NAMED["all_negative"][0]] < 0).all()
    mc = smp[:, RC.NAMED["mixed_sign"][0]]
    assert (mc < 0).any() and (mc > 0).any()
    tc = np.unique(smp[:, RC.NAMED["rounded_ties"][0]])
    assert 1 < tc.size < 40
    assert np.unique(smp[:, RC.NAMED["std0"][0]]).size == 1


@pytest.mark.parametrize("n", [200, 1000])
def test_non_finite_cells_are_nan_like_torch(n):
    """A NaN mean or std, and a mean of +-inf (inf - inf in the lerp), give NaN for both metrics, in torch and in the oracle."""
    mean, std = (a.copy() for a in RC.maps())
    mean[0, 1], std[1, 0], mean[2, 2], mean[6, 4] = np.nan, np.nan, np.inf, -np.inf
    bad = np.zeros((RC.G, RC.G), bool)
    bad[0, 1] = bad[1, 0] = bad[2, 2] = bad[6, 4] = True
    z = RC.draws(n)
    smp = RC.samples(n, "plain", mean, std)
    for q in (0.1, 0.5, 0.9, 1.0):
        tv, tc = _torch_reference(smp, q)
        var = RO.infer_risk_map(mean, std, "var", q, z)
        cvar = RO.infer_risk_map(mean, std, "cvar", q, z)
        assert np.isnan(tv[bad]).all() and np.isnan(tc[bad]).all()
        assert np.isnan(var[bad]).all() and np.isnan(cvar[bad]).all()
        assert _same_value(var, tv).all() and np.array_equal(np.isnan(cvar), np.isnan(tc))
        assert np.isfinite(var[~bad]).all()


def test_one_nan_sample_makes_the_column_nan():
    """np.sort puts a NaN last and would return a number for every q < 1; torch.quantile returns NaN."""
    mean, std = RC.maps()
    z = RC.draws(65).copy()
    z[7, 3, 3] = np.nan
    smp = ((z * std[None]).astype(f32) + mean[None]).astype(f32)
    for q in (0.0, 0.5, 1.0):
        tv, tc = _torch_reference(smp, q)
        var = RO.infer_risk_map(mean, std, "var", q, z)
        cvar = RO.infer_risk_map(mean, std, "cvar", q, z)
        assert np.isnan(tv[3, 3]) and np.isnan(var[3, 3]) and np.isnan(cvar[3, 3]) and np.isnan(tc[3, 3])
        assert _same_value(var, tv).all()
