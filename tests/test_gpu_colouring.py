"""GPU: the colouring step of benchnav_amd.TerrainGenerator (csrc/terrain_kernels.hip: terrain_noise / classes / color kernels)
against the reference's own results (tests/golden/colouring.npz) and the oracles of tests/colouring_oracle.py.

Classes are held exactly.  Colours are held to 1.5 x the distance the reference itself keeps from the float64 restatement on
the fixture's inputs (colouring_oracle.colour_bound); heights, slopes and the slip maps as tests/test_gpu_terrain.py holds them."""
import warnings

import numpy as np
import pytest
import torch

import colouring_oracle as CO
import terrain_oracle as O

pytestmark = pytest.mark.gpu
CASES, SHARED = CO.load_cases()
GOOD = sorted(n for n in CASES if not bool(CASES[n]["raised"]))
KEYS = ("heights", "slopes", "mean", "std")


def _fx64(fx):
    """The case with its classes as terrain_oracle expects them (int64)."""
    return dict(fx, t_classes=fx["t_classes"].astype(np.int64))


def _generate(fx, gen=None, **over):
    from benchnav_amd.terrain import TerrainGenerator
    G, res = int(fx["G"]), float(fx["res"])
    lo, hi = (float(v) for v in fx["thresholds"])
    kw = dict(occupancy=fx["occupancy"], noise=fx["noise"], slip_models=O.models_for(fx), lower_threshold=lo, upper_threshold=hi,
              ambient_intensity=float(fx["ambient"]), **O.geometry(fx))
    kw.update(over)
    own = gen is None
    gen = TerrainGenerator(G, res, batch=1) if own else gen
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = gen.generate([int(fx["seed"])], **kw)
        torch.cuda.synchronize()
        return t
    finally:
        if own:
            gen.close()


@pytest.mark.parametrize("name", GOOD)
def test_end_to_end_from_a_seed_with_the_fixture_noise(name):
    from benchnav_amd.terrain import _copper_table
    fx = _fx64(CASES[name])
    t = _generate(fx)
    # classes: exactly the reference's
    assert t.t_classes.dtype == torch.int64 and np.array_equal(t.t_classes[0].numpy(), fx["t_classes"])
    assert np.array_equal(t.noise[0].cpu().numpy(), fx["noise"])
    # the light vector comes from the host's torch sqrt / cos / sin, which round differently on different CPUs (as linspace does
    # for the craters): z is exact, x and y within two float32 steps of what the reference built where the fixture was made
    light = t.light[0]
    assert light[2] == fx["light"][2] and np.all(np.abs(light - fx["light"]) <= 2 * np.spacing(np.abs(fx["light"])))
    # geometry and slip maps: as test_gpu_terrain holds its classes3 case
    orc = O.oracle_for(fx)
    got = {"heights": t.heights, "slopes": t.slopes, "mean": t.latent_mean, "std": t.latent_std}
    for key in KEYS:
        g = got[key][0].cpu().numpy()
        assert g.shape == fx[key].shape and np.isfinite(g).all(), key
        err = float(np.abs(g.astype(np.float64) - orc[key]).max())
        print(f"{name} {key}: error {err:.3e}, reference spread {O.spread(fx, orc, key):.3e}")
        assert err <= O.tolerance(fx, orc, key), (key, err, O.spread(fx, orc, key))
    # colours: the float64 restatement on the heights the device itself produced (and the light it was given), within the
    # reference's own spread
    table = _copper_table(fx["occupancy"].size)
    bound = CO.colour_bound(fx, table)
    h = t.heights[0].cpu().numpy()
    c = t.colors[0].cpu().numpy()
    err = float(np.abs(c.astype(np.float64) - CO.colours_f64(h, fx["t_classes"], table, light, float(fx["ambient"]))).max())
    print(f"{name} colours: error {err:.3e}, bound {bound:.3e}")
    assert c.shape == (3, int(fx["G"]), int(fx["G"])) and c.dtype == np.float32 and err <= bound


def test_unassigned_cells_and_missing_slip_models_raise_what_the_reference_raises():
    from benchnav_amd.terrain import TerrainGenerator
    fx = CASES["g64_unassigned"]
    with TerrainGenerator(64, 0.5, batch=1) as gen:
        with pytest.warns(UserWarning, match="have not been assigned a terrain class"):
            with pytest.raises(ValueError, match="exceeds the number of slip models"):
                gen.generate([int(fx["seed"])], occupancy=fx["occupancy"], noise=fx["noise"], slip_models=O.models_for(fx))
        counts = [np.zeros(1, np.int32), np.zeros(1, np.int32)]
        gen._check(gen._lib.bn_terrain_class_counts(gen._handle, counts[0].ctypes.data, counts[1].ctypes.data))
        assert int(counts[0][0]) == int(fx["unassigned"]) and int(counts[1][0]) == 0
        cls = gen._color_outputs()[0][0].cpu().numpy()
        assert np.array_equal(cls, fx["t_classes"].astype(np.int32))            # the class map itself is the reference's, -1 included
        # a class beyond the slip models: four classes in the map, two models
        ramp = CASES["g64_ramp"]
        with pytest.raises(ValueError, match="exceeds the number of slip models"):
            gen.generate([0], occupancy=ramp["occupancy"], noise=ramp["noise"], slip_models=O.models_for(ramp)[:2])
        gen._check(gen._lib.bn_terrain_class_counts(gen._handle, counts[0].ctypes.data, counts[1].ctypes.data))
        assert int(counts[0][0]) == 0 and int(counts[1][0]) == int((ramp["t_classes"] >= 2).sum())
        with pytest.raises(ValueError, match="two sources"):
            gen.generate([0], occupancy=ramp["occupancy"], t_classes=np.zeros((64, 64), np.int64))
        with pytest.raises(ValueError):
            gen.generate([0], occupancy=np.full(65, 1 / 65), slip_models=O.models_for(ramp))
        with pytest.warns(UserWarning, match="has been normalized"):
            t = gen.generate([0], occupancy=ramp["occupancy"] * 2, noise=ramp["noise"], slip_models=O.models_for(ramp))
        assert np.array_equal(t.t_classes[0].numpy(), CO.classes_f32(ramp["noise"], ramp["occupancy"] * 2))


@pytest.mark.parametrize("name", sorted(CASES))
def test_colorize_on_the_fixture_heights(name):
    from benchnav_amd.terrain import TerrainGenerator, _copper_table
    fx = CASES[name]
    C_ = fx["occupancy"].size
    table = _copper_table(C_)
    bound = CO.colour_bound(fx, table)
    with TerrainGenerator(int(fx["G"]), float(fx["res"]), batch=1) as gen:
        c = gen.colorize(fx["heights"][None], fx["t_classes"][None], C_, fx["light"][None], float(fx["ambient"]))
        torch.cuda.synchronize()
        c = c[0].cpu().numpy()
    orc = CO.colours_f64(fx["heights"], fx["t_classes"], table, fx["light"], float(fx["ambient"]))
    err = float(np.abs(c.astype(np.float64) - orc).max())
    print(f"{name}: device error {err:.3e}, bound {bound:.3e}, differing from the float32 mirror "
          f"{float(np.mean(c != CO.colours_f32(fx['heights'], fx['t_classes'], table, fx['light'], float(fx['ambient'])))):.4f}")
    assert c.dtype == np.float32 and c.shape == fx["colors"].shape
    assert err <= bound
    assert float(np.abs(c.astype(np.float64) - fx["colors"]).max()) <= bound + bound / 1.5
    if name == "g64_one":
        assert not c.any()


@pytest.mark.parametrize("G", [33, 64, 256])
def test_own_noise_equals_the_numpy_mirror_bit_for_bit(G):
    from benchnav_amd.terrain import TerrainGenerator, slip_models
    seeds = [0, 5, (1 << 40) + 3]
    occ = SHARED["occ/10_10_4_0"][:3]
    with TerrainGenerator(G, 0.5, batch=3) as gen:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = gen.generate(seeds, occupancy=occ, slip_models=slip_models(10), num_craters=1, min_radius=2, max_radius=3)
        torch.cuda.synchronize()
    for b, s in enumerate(seeds):
        mirror = CO.noise_f32(s, G, 20.0)
        dev = t.noise[b].cpu().numpy()
        assert np.array_equal(dev.view(np.uint32), mirror.view(np.uint32)), (G, s)          # bit for bit, the sign of a zero included
        assert np.array_equal(t.t_classes[b].numpy(), CO.classes_f32(mirror, occ[b])), (G, s)


def test_batch_equals_singles_run_to_run_and_uncoloured_is_untouched():
    from benchnav_amd.terrain import TerrainGenerator, slip_models
    G, seeds, occ, models = 64, [0, 1, 7, 3], SHARED["occ/10_10_4_0"][:4], slip_models(10)

    def fields(t):
        return {"classes": t.t_classes.numpy(), "colors": t.colors.cpu().numpy(), "noise": t.noise.cpu().numpy(),
                "heights": t.heights.cpu().numpy(), "mean": t.latent_mean.cpu().numpy(), "std": t.latent_std.cpu().numpy()}
    with TerrainGenerator(G, 0.5, batch=4) as gen:
        plain = gen.generate(seeds, slip_models=models)
        before = {k: getattr(plain, k).cpu().numpy() for k in ("heights", "slopes", "latent_mean", "latent_std", "colors")}
        assert not before["colors"].any() and not plain.t_classes.any() and plain.noise is None
        batch = fields(gen.generate(seeds, occupancy=occ, slip_models=models))
        again = fields(gen.generate(seeds, occupancy=occ, slip_models=models))
        plain2 = gen.generate(seeds, slip_models=models)
        after = {k: getattr(plain2, k).cpu().numpy() for k in before}
    for k in batch:
        assert np.array_equal(batch[k], again[k]), k
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert not plain2.t_classes.any()
    assert batch["colors"].any() and len(np.unique(batch["classes"])) > 1
    with TerrainGenerator(G, 0.5, batch=1) as one:
        for i, s in enumerate(seeds):
            single = fields(one.generate([s], occupancy=occ[i], slip_models=models))
            for k in batch:
                assert np.array_equal(batch[k][i], single[k][0]), (k, s)


def test_to_instances_round_trips_colours_and_classes(tmp_path):
    from benchnav_amd.io import load_instance, save_instance
    from benchnav_amd.terrain import TerrainGenerator, slip_models
    G = 64
    with TerrainGenerator(G, 0.5, batch=2) as gen:
        t = gen.generate([4, 5], occupancy=SHARED["occ/10_10_4_0"][:2], slip_models=slip_models(10))
        insts = gen.to_instances()
    for b, inst in enumerate(insts):
        path = str(tmp_path / f"000_{b:03d}.pt")
        save_instance(path, inst)
        back = load_instance(path)
        col, cls = back.tensors["colors"], back.tensors["t_classes"]
        assert col.dtype == torch.float32 and tuple(col.shape) == (3, G, G) and cls.dtype == torch.int64 and tuple(cls.shape) == (G, G)
        assert torch.equal(col, t.colors[b].cpu()) and torch.equal(cls, t.t_classes[b])
        assert col.any() and len(cls.unique()) == 4
        assert torch.equal(back.latent_mean, t.latent_mean[b].cpu()) and torch.isfinite(back.latent_mean).all()
