"""CPU: the library builds with the GP fit kernels, exports and binds their entry points and rejects bad arguments before it
touches a device; the MFMA kernels' code objects have no private segment and no spill (metadata read as tests/test_gp_build.py
does); GPSlipRegressor.state_dict round-trips through hyperparameters_from_state_dict; SlipRegressorTrainer.load_data equals a
restatement of the reference's loop (trainers/regressor_trainer.py:90-126) under the same seed."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from benchnav_amd import _capi, build, gp
from test_gp_build import LLVM, _gp_kernel_metadata

FIT_SYMBOLS = ("bn_gp_fit_workspace_bytes", "bn_gp_fit_create", "bn_gp_fit_destroy", "bn_gp_fit_set_raw", "bn_gp_fit_set_hyperparameters",
               "bn_gp_fit_evaluate_async", "bn_gp_fit_run_async", "bn_gp_fit_read", "bn_gp_fit_hyperparameters", "bn_gp_fit_history",
               "bn_gp_fit_finish", "bn_gp_fit_last_error")
MFMA_KERNELS = ("gp_fit_trsm_kernel", "gp_fit_syrk_kernel", "gp_fit_inverse_kernel", "gp_fit_grad_kernel")
OTHER_KERNELS = ("gp_fit_build_kernel", "gp_fit_potrf_kernel", "gp_fit_z_kernel", "gp_fit_alpha_kernel", "gp_fit_loss_kernel",
                 "gp_fit_adam_kernel", "gp_fit_pack_kernel")


def test_library_builds_and_exports_the_gp_fit_symbols():
    assert "gp_fit_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gp_fit_kernels.hip"))
    assert "gp_handle.h" in build.HEADERS
    lib = _capi.load()
    header = open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "benchnav_mppi.h")).read()
    for name in FIT_SYMBOLS:
        assert name in _capi.SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"\b{name}\s*\(", header), name
    import benchnav_amd
    assert benchnav_amd.SlipRegressorTrainer is gp.SlipRegressorTrainer and callable(benchnav_amd.GPSlipRegressor.fit)


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")), reason="ROCm LLVM tools not installed")
def test_gp_fit_kernels_have_no_private_segment_and_no_spill(tmp_path):
    """Every kernel of the file once; the four MFMA kernels (16 to 64 accumulator registers) within 128 VGPRs, which keeps the
    1024-thread inverse kernel launchable and four waves per SIMD resident for the others."""
    _capi.load()
    meta = _gp_kernel_metadata(build.LIB_PATH, str(tmp_path))
    for name in MFMA_KERNELS + OTHER_KERNELS:
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == 1, (name, sorted(meta))
        v = next(iter(found.values()))
        assert v["private"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (name, v)
        if name in MFMA_KERNELS:
            assert v["vgpr"] <= 128, (name, v)
    # the predict kernels' names stay unique for tests/test_gp_build.py and tests/test_gp_large_build.py
    for name in ("gp_predict_kernel", "gp_bucket_kernel", "gp_slab_kernel"):
        assert sum(name in k for k in meta) == 1, name


def test_c_abi_rejects_bad_arguments_before_touching_the_device():
    lib = _capi.load()
    n = 4
    x, y = np.arange(n, dtype=np.float64), np.ones(n)
    h = C.c_void_p()

    def create(n_=n, x_=x, y_=y, lb=1e-4):
        return lib.bn_gp_fit_create(0, n_, x_.ctypes.data, y_.ctypes.data, lb, C.byref(h))
    bad_x, bad_y = x.copy(), y.copy()
    bad_x[2], bad_y[1] = np.inf, np.nan
    big = np.zeros(gp.MAX_POINTS + 1)
    for kw, word in ((dict(n_=0), b"10240"), (dict(n_=gp.MAX_POINTS + 1, x_=big, y_=big), b"10240"), (dict(x_=bad_x), b"finite"),
                     (dict(y_=bad_y), b"finite"), (dict(lb=-1.0), b">= 0"), (dict(lb=float("nan")), b"finite")):
        assert create(**kw) == _capi.BN_ERR_INVALID, kw
        assert word in lib.bn_gp_fit_last_error(), (kw, lib.bn_gp_fit_last_error())
        assert not h.value
    assert lib.bn_gp_fit_create(0, n, None, y.ctypes.data, 1e-4, C.byref(h)) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_fit_create(0, n, x.ctypes.data, None, 1e-4, C.byref(h)) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_fit_create(0, n, x.ctypes.data, y.ctypes.data, 1e-4, None) == _capi.BN_ERR_INVALID
    ok = (0.1, 0.9, 0.999, 1e-8)
    for args, word in (((-1,) + ok, b"iterations"), ((1, 0.0) + ok[1:], b"lr"), ((1, -0.1) + ok[1:], b"lr"), ((1, float("nan")) + ok[1:], b"lr"),
                       ((1, 0.1, 1.0, 0.999, 1e-8), b"beta"), ((1, 0.1, 0.9, 0.999, -1.0), b"eps"), ((1,) + ok, b"null")):
        assert lib.bn_gp_fit_run_async(None, None, *args) == _capi.BN_ERR_INVALID, args
        assert word in lib.bn_gp_fit_last_error(), (args, lib.bn_gp_fit_last_error())
    raw = np.zeros(4)
    assert lib.bn_gp_fit_set_raw(None, raw.ctypes.data) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_fit_set_hyperparameters(None, 0.0, 1.0, 1.0, 0.1) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_fit_evaluate_async(None, None) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_fit_read(None, None, None, None, None, None) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_fit_history(None, None, 0) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_fit_finish(None, None, C.byref(h)) == _capi.BN_ERR_INVALID
    lib.bn_gp_fit_destroy(None)
    # two N x N float64 buffers, the diagonal tiles' inverses, four vectors, three partials per tile, the history, the state
    assert lib.bn_gp_fit_workspace_bytes(0) == 0 and lib.bn_gp_fit_workspace_bytes(gp.MAX_POINTS + 1) == 0
    base = lib.bn_gp_fit_workspace_bytes(1)
    assert lib.bn_gp_fit_workspace_bytes(32) == base
    np_, T = 10240, 320
    assert lib.bn_gp_fit_workspace_bytes(10240) - base == (2 * np_ * np_ * 8 + 8192 * T + 32 * np_ + 12 * T * (T + 1)) - (2 * 32 * 32 * 8 + 8192 + 32 * 32 + 24)
    if not torch.cuda.is_available():
        assert create() == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_gp_fit_last_error()
        xs, ys = np.float32([0.0, 1.0, 2.0]), np.float32([0.0, 0.5, 1.0])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gp.GPSlipRegressor.fit(xs, ys, num_iterations=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gp.GPSlipRegressor(xs, ys, 0.0, 0.5, 5.0, 0.01, factorization="device")


def test_python_checks_its_arguments_before_it_looks_for_a_device():
    xs, ys = np.float32([0.0, 1.0, 2.0]), np.float32([0.0, 0.5, 1.0])
    with pytest.raises(ValueError, match="factorization"):
        gp.GPSlipRegressor(xs, ys, 0.0, 0.5, 5.0, 0.01, factorization="gpu")
    with pytest.raises(ValueError, match="> 0"):
        gp.GPSlipRegressor(xs, ys, 0.0, 0.5, 5.0, 0.0, factorization="device")
    with pytest.raises(ValueError, match="differ in length"):
        gp.GPSlipRegressor.fit(xs, ys[:2])
    with pytest.raises(ValueError, match="num_iterations"):
        gp.GPSlipRegressor.fit(xs, ys, num_iterations=-1)
    with pytest.raises(ValueError, match="learning_rate"):
        gp.GPSlipRegressor.fit(xs, ys, learning_rate=0.0)
    with pytest.raises(ValueError, match="initial_raw"):
        gp.GPSlipRegressor.fit(xs, ys, initial_raw=[0.0, 0.0, np.nan, 0.0])
    with pytest.raises(ValueError, match=str(gp.MAX_POINTS)):
        gp.GPSlipRegressor.fit(np.zeros(gp.MAX_POINTS + 1, np.float32), np.zeros(gp.MAX_POINTS + 1, np.float32))


def test_state_dict_round_trips_the_float32_rounded_raw_parameters():
    reg = gp.GPSlipRegressor.__new__(gp.GPSlipRegressor)          # what fit() fills in, without a device
    reg._handle = None
    reg.raw_parameters = np.array([0.3826389773950206, -2.85648781937315, 7.978460502014347, -6.760458973418911])
    sd = reg.state_dict()
    assert sd["likelihood.noise_covar.raw_noise"].shape == (1,) and sd["covar_module.base_kernel.raw_lengthscale"].shape == (1, 1)
    assert sd["mean_module.raw_constant"].shape == () and sd["covar_module.raw_outputscale"].shape == ()
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert float(sd["likelihood.noise_covar.raw_noise_constraint.lower_bound"]) == float(np.float32(1e-4))
    assert float(sd["likelihood.noise_covar.raw_noise_constraint.upper_bound"]) == float("inf")
    r32 = reg.raw_parameters.astype(np.float32).astype(np.float64)
    got = gp.hyperparameters_from_state_dict(sd)
    want = {"constant": r32[0], "outputscale": np.logaddexp(0.0, r32[1]), "lengthscale": np.logaddexp(0.0, r32[2]),
            "noise": np.logaddexp(0.0, r32[3]) + float(np.float32(1e-4))}
    assert got == {k: float(v) for k, v in want.items()}
    plain = gp.GPSlipRegressor.__new__(gp.GPSlipRegressor)
    plain._handle = None
    with pytest.raises(ValueError, match="no raw parameters"):
        plain.state_dict()


def _reference_load_data(loader, num_classes, num_samples):
    """regressor_trainer.py:90-126 restated: per batch and class the masked slopes and slips, concatenated and cut"""
    xs, ys = {k: [] for k in range(num_classes)}, {k: [] for k in range(num_classes)}
    for slopes, slips, t_classes in loader:
        for k in range(num_classes):
            mask = t_classes == k
            if torch.any(mask):
                xs[k].append(slopes[mask])
                ys[k].append(slips[mask])
    return ({k: torch.cat(xs[k], dim=0)[:num_samples] for k in range(num_classes)},
            {k: torch.cat(ys[k], dim=0)[:num_samples] for k in range(num_classes)})


def test_trainer_load_data_equals_the_reference_loop_under_the_same_seed(tmp_path):
    rng = np.random.default_rng(4)
    M, G = 5, 16
    slopes = torch.from_numpy(rng.uniform(-30, 30, (M, G, G)).astype(np.float32))
    slips = torch.from_numpy(rng.uniform(0, 1, (M, G, G)).astype(np.float32))
    classes = torch.from_numpy(rng.integers(0, 3, (M, G, G)))
    ds = torch.utils.data.TensorDataset(slopes, slips, classes)
    params = types.SimpleNamespace(batch_size=2, learning_rate=0.1, num_iterations=100)
    trainer = gp.SlipRegressorTrainer("cuda", str(tmp_path / "m"), str(tmp_path / "d"), 3, params, ds)
    assert trainer.model_directory == os.path.join(str(tmp_path / "m"), "lr1e-01_iters100")
    assert os.path.isdir(os.path.join(trainer.model_directory, "models")) and os.path.isdir(str(tmp_path / "d" / "slip_observations"))
    for num_samples in (9999, 100):
        torch.manual_seed(11)
        got_x, got_y = trainer.load_data(num_samples) if num_samples != 9999 else trainer.load_data()
        torch.manual_seed(11)
        want_x, want_y = _reference_load_data(torch.utils.data.DataLoader(ds, batch_size=2, shuffle=True), 3, num_samples)
        for k in range(3):
            assert torch.equal(got_x[k], want_x[k]) and torch.equal(got_y[k], want_y[k])
            assert got_x[k].numel() == min(num_samples, int((classes == k).sum()))
    # the files a regressor is saved to, written here from a device-less stand-in
    reg = gp.GPSlipRegressor.__new__(gp.GPSlipRegressor)
    reg._handle = None
    reg.raw_parameters = np.array([0.25, -1.0, 2.0, -3.0])
    trainer.save(got_x[1], got_y[1], reg, 1)
    data = torch.load(tmp_path / "d" / "slip_observations" / "01_class.pth", weights_only=True)
    state = torch.load(os.path.join(trainer.model_directory, "models", "01_class.pth"), weights_only=True)
    assert torch.equal(data["train_x"], got_x[1]) and torch.equal(data["train_y"], got_y[1])
    assert gp.hyperparameters_from_state_dict(state)["constant"] == 0.25
