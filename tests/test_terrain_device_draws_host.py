"""CPU: the NumPy restatement of the draws' specification (tests/terrain_draws_spec.py: MT19937, float32 uniforms, the crater
loop, the crater table, the phases, the light source) against benchnav_amd.terrain.replay_draws on torch's CPU generator, and
the host side of the device draw path (the read-back's warning and error)."""
import warnings

import numpy as np
import pytest

import terrain_draws_spec as S


def _replay(seed, G, **kw):
    from benchnav_amd.terrain import replay_draws
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return replay_draws(seed, G, S.RES, **kw)


def _assert_equal(spec, ref, what):
    assert spec.attempts == ref.attempts and spec.gave_up == ref.gave_up, what
    assert len(spec.craters) == len(ref.craters), what
    for a, b in zip(spec.craters, ref.craters):
        assert np.array_equal(a.center.view(np.uint32), b.center.view(np.uint32)), what
        assert np.float32(a.radius) == np.float32(b.radius) and a.angle == b.angle, what
        assert a.n == b.n and tuple(a.bounds) == tuple(b.bounds) and a.fits, what
        # torch's vectorised linspace and float32 tan against the scalar formulas: the CPU-to-CPU spread
        assert np.abs(a.lin.astype(np.float64) - b.lin).max() <= np.spacing(np.float32(b.radius)), what
        assert abs(float(a.neg_tan) - b.neg_tan) <= np.spacing(np.float32(abs(b.neg_tan))), what
    assert np.array_equal(spec.phases.view(np.uint32), ref.phases.view(np.uint32)), what


@pytest.mark.parametrize("name", sorted(S.SEED_SETS))
def test_restatement_equals_the_replay(name):
    G, seeds, kw = S.SEED_SETS[name]
    margins = []
    for seed in seeds:
        spec, ref = S.draws(seed, G, S.RES, **kw), _replay(seed, G, **kw)
        _assert_equal(spec, ref, (name, seed))
        margins += spec.margins
        if name == "g33_giveup":
            assert spec.attempts == 1001 and spec.gave_up
        if name == "six_craters":
            assert spec.gave_up and len(spec.craters) <= 5
    # no accept / reject decision hangs on a rounding: every overlap distance stays 16 float32 ulps clear of its threshold
    assert min(margins) > 16, (name, min(margins))


def test_restatement_equals_the_replay_with_flags_and_light():
    for seed in (0, 3, 11):
        for kw in ({"is_crater": False}, {"is_fractal": False}, {"is_crater": False, "is_fractal": False}, {}):
            for col in (True, (0.5, 0.9)):
                spec, ref = S.draws(seed, 20, S.RES, coloring=col, **kw), _replay(seed, 20, coloring=col, **kw)
                _assert_equal(spec, ref, (seed, kw))
                assert np.array_equal(spec.light_uniforms.view(np.uint32), ref.light_uniforms.view(np.uint32))
                ulp = np.spacing(np.abs(ref.light).astype(np.float32)).astype(np.float64)
                assert np.all(np.abs(spec.light.astype(np.float64) - ref.light) <= 2 * ulp), (seed, kw, col)


def test_crater_slices_always_fit():
    """psx - sx = n // 2 - cx whichever side of the border the crater lies on, so psx + (ex - sx) = n // 2 - cx + min(cx + n // 2, N)
    <= 2 (n // 2) <= n: the host's "does not fit" ValueError cannot be reached from a draw.  Checked here by brute force over the
    centre cells, sizes and radii of small maps; the read-back's handling of the status word is covered by the unit call below."""
    for G in (2, 3, 8, 20):
        for n in range(1, 3 * G):
            for c in range(G):
                N = G + 2
                s, e, p = max(c - n // 2, 0), min(c + n // 2, N), max(n // 2 - c, 0)
                assert p + (e - s) <= n
    for seed in range(2000):                        # one crater per seed (no rejection), larger than the map or near its size
        d = S.draws(seed, 6 + seed % 3, 0.25, is_fractal=False, num_craters=1, min_radius=0.2, max_radius=3)
        assert len(d.craters) == 1 and d.craters[0].fits


def test_read_back_raises_what_the_host_path_raises():
    from benchnav_amd.terrain import check_draw_records
    rec = np.zeros((3, 4), np.int32)
    rec[:, 0] = (2, 1001, 5)
    rec[:, 3] = (3, 2, 3)
    radii = np.full((3, 3), 7.5, np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        check_draw_records(rec, radii, 64)
    rec[1, 1] = 1
    with pytest.warns(UserWarning, match="Failed to place all craters after 1000 attempts"):
        check_draw_records(rec, radii, 64)
    rec[2, 2] = 2                                   # the status word: 1 + the first crater whose slices disagree
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="crater of radius 7.5 does not fit a 64x64 map"):
            check_draw_records(rec, radii, 64)


def test_device_draws_are_refused_by_name_only():
    from benchnav_amd.terrain import TerrainGenerator
    gen = TerrainGenerator.__new__(TerrainGenerator)
    gen.batch, gen.grid_size = 1, 16
    with pytest.raises(ValueError, match="draws"):
        TerrainGenerator.generate(gen, [0], draws="gpu")


def test_draws_kernel_is_built_without_scratch():
    import os
    from test_build_artifacts import LLVM, _kernel_metadata
    if not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("ROCm LLVM tools not installed")
    import tempfile
    from benchnav_amd import _capi
    from benchnav_amd import build as b
    _capi.load()
    with tempfile.TemporaryDirectory() as tmp:
        meta = _kernel_metadata(b.LIB_PATH, tmp)
    hits = {k: v for k, v in meta.items() if "terrain_draws_kernel" in k}
    assert len(hits) == 1, sorted(meta)
    assert not any(v["private"] or v["vgpr_spills"] for v in hits.values()), hits
