"""CPU: the host half of benchnav_amd.terrain against the reference's own terrain fixtures (tests/golden/terrain*.npz) -- the
replayed draws bit for bit, the torch.rand stream identity they rest on, the float64 oracle (tests/terrain_oracle.py) and the
float32 crater mirror."""
import warnings

import numpy as np
import pytest
import torch

import terrain_oracle as O

CASES = O.load_cases()


def test_rand_n_equals_n_single_draws():
    # the fBm phases are drawn as ONE torch.rand(n); the reference draws them one torch.rand(1) at a time
    for n in (5, 141, 2201, 4358, 33282):
        a = torch.Generator().manual_seed(n)
        b = torch.Generator().manual_seed(n)
        whole = torch.rand(n, generator=a)
        single = torch.cat([torch.rand(1, generator=b) for _ in range(n)])
        assert torch.equal(whole, single), n


@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_reproduces_crater_tables_and_phases(name):
    fx = CASES[name]
    d = O.draws_for(fx)
    tab = np.array([[c.center[0], c.center[1], c.radius, c.angle] for c in d.craters], np.float64).reshape(-1, 4)
    assert np.array_equal(tab, fx["craters"])
    assert d.gave_up == bool(fx["gave_up"])
    u = fx["uniforms"]
    if O.geometry(fx)["is_fractal"]:
        from benchnav_amd.terrain import num_phases
        assert d.phases.size == num_phases(int(fx["G"]))
        assert np.array_equal(d.phases, u[u.size - d.phases.size:])
    else:
        assert d.phases.size == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_profile_inputs_are_the_references_on_this_cpu(name):
    """The replay computes each crater's linspace and -tan with the reference's own torch calls: on a CPU of the kind that made
    the fixtures they are the recorded values bit for bit (torch's CPU linspace depends on the vector width)."""
    fx = CASES[name]
    d, r = O.draws_for(fx), O.reference_draws(fx)
    for a, b in zip(d.craters, r.craters):
        assert a.neg_tan == b.neg_tan
        assert np.abs(a.lin.astype(np.float64) - b.lin).max() <= np.spacing(np.float32(a.radius))
        if torch.backends.cpu.get_cpu_capability() == "AVX512":
            assert np.array_equal(a.lin, b.lin)


def test_fixture_covers_the_issue_cases():
    assert CASES["giveup"]["gave_up"] and len(CASES["giveup"]["craters"]) < O.geometry(CASES["giveup"])["num_craters"]
    b = O.draws_for(CASES["border"])
    N = int(CASES["border"]["G"]) + 2
    assert any(c.bounds[0] == 0 or c.bounds[1] == 0 for c in b.craters) and any(c.bounds[2] == N or c.bounds[3] == N for c in b.craters)
    assert {int(CASES[k]["G"]) % 2 for k in ("odd33", "odd50")} == {1, 0} and int(CASES["odd33"]["G"]) == 33
    assert len(np.unique(CASES["classes3"]["t_classes"])) == 3 and CASES["classes3"]["models"].shape[0] == 3


def test_giveup_warns_after_1000_attempts():
    from benchnav_amd.terrain import replay_draws
    fx = CASES["giveup"]
    with pytest.warns(UserWarning, match="1000 attempts"):
        d = replay_draws(int(fx["seed"]), int(fx["G"]), float(fx["res"]), **O.geometry(fx))
    assert d.attempts == 1001


def test_slip_models_mirror_the_generator():
    from benchnav_amd.terrain import slip_models
    fx = CASES["classes3"]
    got = np.array([[m.slip_sensitivity, m.slip_nonlinearity, m.slip_offset, m.base_noise_scale, m.slope_noise_scale]
                    for m in slip_models(3)])
    assert np.array_equal(got, fx["models"])
    with pytest.raises(ValueError):
        slip_models(2, (1.0, 1.0))


def test_oracle_spectrum_matches_the_reference():
    fx = CASES["small"]
    s = O.spectrum(int(fx["G"]), float(fx["res"]), O.draws_for(fx).phases)
    ref = fx["spectrum"].astype(np.complex128)
    assert np.array_equal(ref == 0, s == 0)                            # the cells no loop writes, and the origin
    # complex64 rounding of rad * e^{i phi} and of the scaling: a few float32 ulps of the largest entry
    assert np.abs(ref - s).max() <= 8 * np.finfo(np.float32).eps * np.abs(s).max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_the_reference(name):
    fx = CASES[name]
    orc = O.oracle_for(fx)
    for key in ("heights", "slopes", "mean", "std"):
        # the reference is float32: its distance to the float64 restatement is float32 rounding of the field, a few ulps of
        # the largest height grown by sqrt(G') over the FFT's sums (slopes: height errors over 8 res)
        scale = {"heights": np.abs(orc["heights"]).max(), "slopes": np.abs(orc["heights"]).max() / (8 * float(fx["res"])),
                 "mean": 1.0, "std": 1.0}[key]
        bound = 64 * np.finfo(np.float32).eps * scale * (int(fx["G"]) + 2) ** 0.5
        assert O.spread(fx, orc, key) <= bound, (key, O.spread(fx, orc, key), bound)


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if not O.geometry(CASES[n])["is_fractal"]])
def test_crater_float32_mirror_is_the_reference_with_its_distances(name):
    fx = CASES[name]
    d = O.reference_draws(fx)
    G = int(fx["G"])
    ref_d, ieee_d = O.reference_dists(fx, d), O.ieee_dists(d)
    # the mirror's operation order is the reference's: with the reference's own distances it is the reference bit for bit
    assert np.array_equal(O.craters_f32(G, d, ref_d)[1:-1, 1:-1], fx["heights"])
    # the recorded distances are float32 sqrt within one ulp of the correctly rounded one
    for r, i in zip(ref_d, ieee_d):
        assert np.all(np.abs(r.view(np.int32).astype(np.int64) - i.view(np.int32).astype(np.int64)) <= 1)
    # with IEEE sqrt (the device's) the heights stay within an ulp-level distance of the reference
    ieee = O.craters_f32(G, d)[1:-1, 1:-1]
    assert np.abs(ieee - fx["heights"]).max() <= 4 * np.finfo(np.float32).eps * np.abs(fx["heights"]).max()


def test_start_and_goal_are_refused():
    from benchnav_amd.terrain import TerrainGenerator
    gen = TerrainGenerator.__new__(TerrainGenerator)
    with pytest.raises(NotImplementedError):
        TerrainGenerator.generate(gen, [0], start_pos=torch.zeros(2), goal_pos=torch.ones(2))
