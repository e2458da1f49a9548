"""CPU: the host half of the colouring step (benchnav_amd.terrain) and its oracles (tests/colouring_oracle.py) against the
reference's own results (tests/golden/colouring.npz, made by tests/golden/make_golden_colouring.py).

The colour tolerance is not a constant: it is 1.5 x the distance the reference itself keeps from the float64 restatement on
the same inputs (colouring_oracle.colour_bound), DESIGN.md 4.5's convention."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import colouring_oracle as CO
import terrain_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, SHARED = CO.load_cases()
OCC_SETS = [(10, 10, 4), (100, 10, 4), (25, 10, 3)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_mirror_gives_the_reference_classes_exactly(name):
    fx = CASES[name]
    t = CO.classes_f32(fx["noise"], fx["occupancy"])
    assert np.array_equal(t, fx["t_classes"].astype(np.int64))
    assert int((t == -1).sum()) == int(fx["unassigned"])
    if name == "g64_unassigned":
        assert int(fx["unassigned"]) > 0 and bool(fx["raised"])
    else:
        assert int(fx["unassigned"]) == 0 and not bool(fx["raised"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_mirror_colours_within_the_reference_spread(name):
    from benchnav_amd.terrain import _copper_table
    fx = CASES[name]
    table = _copper_table(fx["occupancy"].size)
    bound = CO.colour_bound(fx, table)
    orc = CO.colours_f64(fx["heights"], fx["t_classes"], table, fx["light"], float(fx["ambient"]))
    got = CO.colours_f32(fx["heights"], fx["t_classes"], table, fx["light"], float(fx["ambient"]))
    err = float(np.abs(got.astype(np.float64) - orc).max())
    differing = float(np.mean(got != fx["colors"]))
    print(f"{name}: reference spread {bound / 1.5:.3e}, mirror error {err:.3e}, values differing from the reference {differing:.4f}")
    assert got.shape == fx["colors"].shape == (3, int(fx["G"]), int(fx["G"]))
    assert err <= bound
    assert float(np.abs(got.astype(np.float64) - fx["colors"]).max()) <= bound + bound / 1.5       # both within their own distance
    if name == "g64_one":
        assert bound == 0.0 and not got.any() and not fx["colors"].any()


def test_copper_table_equals_matplotlib_rows_without_importing_matplotlib():
    from benchnav_amd.terrain import _copper_table
    for C in range(1, 17):
        assert np.array_equal(_copper_table(C), SHARED[f"copper/{C}"]), C
        assert _copper_table(C).dtype == np.float32
    assert not _copper_table(1).any()
    with pytest.raises(ValueError):
        _copper_table(65)
    code = ("import sys, benchnav_amd, benchnav_amd.terrain as t; t._copper_table(10); t.occupancies(4); "
            "assert not any(m.split('.')[0] == 'matplotlib' for m in sys.modules), 'matplotlib imported'")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("shape", OCC_SETS)
@pytest.mark.parametrize("seed", [0, 1])
def test_occupancies_equal_the_reference_tables_bit_for_bit(shape, seed):
    from benchnav_amd.terrain import occupancies
    E, T, S = shape
    got = occupancies(E, T, S, seed=seed).numpy()
    ref = SHARED[f"occ/{E}_{T}_{S}_{seed}"]
    assert got.dtype == np.float32 and np.array_equal(got, ref)


def test_occupancies_where_the_reference_raises():
    from benchnav_amd.terrain import occupancies
    a, b = occupancies(7, 10, 4, seed=0).numpy(), occupancies(7, 10, 4, seed=0).numpy()
    assert np.array_equal(a, b) and a.shape == (7, 10)
    for row in a:
        assert int((row == np.float32(1 / 4)).sum()) == 4 and int((row == 0).sum()) == 6


@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_reproduces_the_light_draws_and_the_light_vector(name):
    from benchnav_amd.terrain import replay_draws
    fx = CASES[name]
    lo, hi = (float(v) for v in fx["thresholds"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = replay_draws(int(fx["seed"]), int(fx["G"]), float(fx["res"]), coloring=(lo, hi), **O.geometry(fx))
        plain = replay_draws(int(fx["seed"]), int(fx["G"]), float(fx["res"]), **O.geometry(fx))
    assert np.array_equal(d.light_uniforms, fx["light_uniforms"])
    # the vector goes through torch's sqrt, cos and sin, whose last bit depends on the CPU (as linspace's does for the craters):
    # z is exact everywhere, x and y are the fixture's on the CPU that made it and within two float32 steps of it elsewhere
    assert d.light.dtype == np.float32 and d.light[2] == fx["light"][2]
    assert np.all(np.abs(d.light - fx["light"]) <= 2 * np.spacing(np.abs(fx["light"])))
    print(f"{name}: light vector bit for bit: {np.array_equal(d.light, fx['light'])}")
    assert plain.light is None and plain.light_uniforms is None and np.array_equal(plain.phases, d.phases)
    assert abs(float(np.linalg.norm(d.light.astype(np.float64))) - 1.0) < 1e-6 and lo <= d.light[2] <= hi


def test_light_source_is_the_first_two_draws_of_a_seed():
    import torch
    from benchnav_amd.terrain import light_source
    a, b = light_source(5), light_source(torch.Generator().manual_seed(5))
    assert a.shape == (3,) and a.dtype == np.float32 and np.array_equal(a, b)
    assert not np.array_equal(a, light_source(6))
    assert 0.2 <= light_source(5, 0.2, 0.3)[2] <= 0.3


def test_noise_mirror_lattice_seeds_and_class_coverage():
    fs = 20.0
    n0 = CO.noise_f32(0, 64, fs)
    assert n0.dtype == np.float32 and n0.shape == (64, 64) and np.isfinite(n0).all()
    assert np.all(n0[::20, ::20] == 0)                                     # lattice points: x and y multiples of the feature size
    assert np.array_equal(n0, CO.noise_f32(0, 64, fs)) and not np.array_equal(n0, CO.noise_f32(1, 64, fs))
    assert not np.array_equal(CO.noise_f32(1, 64, fs), CO.noise_f32(1 + (1 << 32), 64, fs))      # the key's high word counts
    assert np.array_equal(CO.noise_f32(3, 64, fs), CO.noise_f32(3, 128, fs)[:64, :64])           # a field, not a tile
    rows = SHARED["occ/10_10_4_0"]
    for seed in range(64):
        n = CO.noise_f32(seed, 64, fs)
        assert n.max() > n.min(), seed
        for r, occ in enumerate(rows):
            t = CO.classes_f32(n, occ)
            want = set(np.flatnonzero(occ > 0).tolist())
            assert set(np.unique(t).tolist()) == want, (seed, r, np.unique(t), want)
