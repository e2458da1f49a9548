"""GPU: risk.infer_risk_maps (bn_risk_maps_infer, risk_maps_kernel of csrc/risk_kernels.hip) -- M maps under C settings in one launch.

The contract: out[c, m] is bit for bit infer_risk_map(mean[m], std[m], *settings[c], num_samples, seed=seeds[m]) -- or z=z[m] with
injected draws -- for every c and m.  The inputs are tests/risk_cases.py's: M = 3 maps of 7 x 7 (maps() and two shifted copies;
147 cells are no multiple of the four waves of a workgroup, so workgroups straddle maps and the last one is part-filled), C = 5
settings (the expected value, VaR at both ends of the confidence range's lerp branches, CVaR at an interior and a last-rank
confidence) and sample counts on both sides of every instantiation edge (R = 16 / 32 / 64).  On injected draws the batched output
is also held to torch.quantile on the CPU by value and to the float64 tail mean within risk_cases.cvar_bound, so the chain
single call -> batched call cannot drift together.  One batched output per n is computed once and shared."""
import functools

import numpy as np
import pytest

import risk_cases as RC

f32 = np.float32
pytestmark = pytest.mark.gpu

SETTINGS = [("expected_value", None), ("var", 0.0), ("var", 0.9), ("cvar", 0.5), ("cvar", 0.999)]
NS = [2, 64, 65, 1000, 1025, 2049]
SEEDS = [0xBD22BBCCCC2, 7, (1 << 64) - 1]          # both halves non-zero, a small one, the largest
M = 3


@functools.lru_cache(maxsize=None)
def _maps():
    """(mean, std) (3, 7, 7): risk_cases.maps() and two copies shifted by one and by ten cells (and in level)."""
    mean, std = RC.maps()
    means = np.stack([mean, np.roll(mean.ravel(), 1).reshape(RC.G, RC.G) + f32(0.125), np.roll(mean.ravel(), 10).reshape(RC.G, RC.G) - f32(0.25)])
    stds = np.stack([std, np.roll(std.ravel(), 1).reshape(RC.G, RC.G), np.roll(std.ravel(), 10).reshape(RC.G, RC.G) * f32(0.5)])
    return means.astype(f32), stds.astype(f32)


@functools.lru_cache(maxsize=None)
def _draws(n):
    """z (3, n, 7, 7): the plain draws, the variant with a row of ties, and the plain draws in reverse sample order."""
    z = np.stack([RC.draws(n, "plain"), RC.draws(n, "halves"), RC.draws(n, "plain")[::-1]])
    z.setflags(write=False)
    return z


def _samples(z, mean, std):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((z * std[None]).astype(f32) + mean[None]).astype(f32)


def _batched(n, z=None, means=None, stds=None, settings=SETTINGS, seeds=SEEDS):
    import torch
    from benchnav_amd.risk import infer_risk_maps
    if means is None:
        means, stds = _maps()
    zt = None if z is None else torch.from_numpy(np.array(z, f32))
    return infer_risk_maps(torch.from_numpy(means), torch.from_numpy(stds), settings, num_samples=n, seeds=seeds, z=zt).cpu().numpy()


def _single(m, c, n, z=None, means=None, stds=None):
    import torch
    from benchnav_amd.risk import infer_risk_map
    if means is None:
        means, stds = _maps()
    metric, q = SETTINGS[c]
    zt = None if z is None else torch.from_numpy(np.array(z[m], f32))
    return infer_risk_map(torch.from_numpy(means[m]), torch.from_numpy(stds[m]), metric, q, num_samples=n, z=zt, seed=SEEDS[m]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _outputs(n):
    """(Philox output, injected-draw output), each (5, 3, 7, 7): computed once per n and shared."""
    a, b = _batched(n), _batched(n, _draws(n))
    a.setflags(write=False); b.setflags(write=False)
    return a, b


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("n", NS)
def test_every_setting_and_map_is_the_single_call_bit_for_bit(n):
    philox, injected = _outputs(n)
    assert philox.shape == injected.shape == (len(SETTINGS), M, RC.G, RC.G)
    for c in range(len(SETTINGS)):
        for m in range(M):
            for what, got, z in (("philox", philox, None), ("injected", injected, _draws(n))):
                want = _single(m, c, n, z)
                bad = _bits(got[c, m]) != _bits(want)
                assert not bad.any(), f"n={n} {what} setting {SETTINGS[c]} map {m}: cells {np.argwhere(bad).tolist()} differ"
    means, _ = _maps()
    assert np.array_equal(_bits(philox[0]), _bits(means))                  # an expected_value row is the mean itself


@pytest.mark.parametrize("n", NS)
def test_injected_draws_against_torch_quantile_and_the_float64_tail_mean(n):
    import torch
    _, got = _outputs(n)
    means, stds = _maps()
    z = _draws(n)
    worst = 0.0
    for m in range(M):
        smp = _samples(z[m], means[m], stds[m])
        for c, (metric, q) in enumerate(SETTINGS):
            if metric == "expected_value":
                continue
            var = torch.quantile(torch.from_numpy(smp), q, dim=0).numpy()     # the CPU's value is the reference's
            if metric == "var":
                same = (got[c, m] == var) | (np.isnan(got[c, m]) & np.isnan(var))
                assert same.all(), f"n={n} map {m} VaR@{q}: cells {np.argwhere(~same).tolist()}: {got[c, m][~same]} vs {var[~same]}"
                continue
            ref64, scale = RC.tail_mean64(smp, var)
            assert np.array_equal(np.isnan(got[c, m]), np.isnan(ref64)), f"n={n} map {m} CVaR@{q}: NaN pattern"
            fin = ~np.isnan(ref64)
            err, bound = np.abs(got[c, m].astype(np.float64) - ref64)[fin], RC.cvar_bound(n, scale)[fin]
            assert (err <= bound).all(), f"n={n} map {m} CVaR@{q}: error {err.max():.3g} over its bound"
            nz = bound > 0
            worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
    print(f"\nn={n}: VaR equals torch.quantile in all cells of all maps; CVaR error / bound max {worst:.3f}")


def test_a_nan_cell_in_one_map_leaves_the_other_maps_alone():
    n = 1000
    means, stds = (a.copy() for a in _maps())
    means[1, 3, 3] = np.nan                                                   # map 1, cell 24: its workgroup also holds cells of map 1 only
    stds[1, 0, 0] = np.nan                                                    # map 1, cell 0: shares a workgroup with map 0's last cell
    base_p, base_z = _outputs(n)
    for base, z in ((base_p, None), (base_z, _draws(n))):
        got = _batched(n, z, means, stds)
        assert np.isnan(got[:, 1, 3, 3]).all() and np.isnan(got[1:, 1, 0, 0]).all()
        for m in (0, 2):
            assert np.array_equal(_bits(got[:, m]), _bits(base[:, m])), f"map {m} changed"
        keep = np.ones((RC.G, RC.G), bool)
        keep[3, 3] = keep[0, 0] = False
        assert np.array_equal(_bits(got[:, 1][:, keep]), _bits(base[:, 1][:, keep])), "map 1's other cells changed"


def test_two_calls_and_a_side_stream_give_the_same_bits():
    import torch
    n = 1000
    base, _ = _outputs(n)
    assert np.array_equal(_bits(_batched(n)), _bits(base))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _batched(n)                                                     # (.cpu() inside waits for the side stream)
    assert np.array_equal(_bits(got), _bits(base))


def test_map_and_setting_counts_do_not_matter():
    """A sub-batch in another order with other settings around it returns the same rows."""
    n = 65
    base, _ = _outputs(n)
    means, stds = _maps()
    order = [2, 0]
    settings = [SETTINGS[3], SETTINGS[0], SETTINGS[2], SETTINGS[2]]
    got = _batched(n, None, means[order], stds[order], settings, [SEEDS[m] for m in order])
    for i, c in enumerate((3, 0, 2, 2)):
        for k, m in enumerate(order):
            assert np.array_equal(_bits(got[i, k]), _bits(base[c, m])), (i, k)


def test_refusals():
    import torch
    from benchnav_amd.risk import infer_risk_maps
    means, stds = (torch.from_numpy(a) for a in _maps())
    var = ("var", 0.9)
    with pytest.raises(ValueError, match="settings"):
        infer_risk_maps(means, stds, [], num_samples=100)
    with pytest.raises(ValueError, match="settings"):
        infer_risk_maps(means, stds, [var] * 17, num_samples=100)
    assert infer_risk_maps(means, stds, [var] * 16, num_samples=100).shape == (16, M, RC.G, RC.G)
    for bad in (1, 4097):
        with pytest.raises(ValueError, match="num_samples"):
            infer_risk_maps(means, stds, [var], num_samples=bad)
    for q in (-0.1, 1.5, None):
        with pytest.raises(AssertionError, match="confidence_value"):
            infer_risk_maps(means, stds, [("expected_value", None), ("cvar", q)], num_samples=100)
    with pytest.raises(AssertionError, match="inference_metric"):
        infer_risk_maps(means, stds, [("mean", None)], num_samples=100)
    with pytest.raises(ValueError, match="seeds"):
        infer_risk_maps(means, stds, [var], num_samples=100, seeds=[1, 2])
    with pytest.raises(ValueError, match="z must be"):
        infer_risk_maps(means, stds, [var], num_samples=100, z=torch.zeros(M, 99, RC.G, RC.G))
