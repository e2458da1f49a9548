"""CPU: the library builds with the GP kernels, exports their entry points and rejects bad arguments before it touches a device;
the predict kernel's code object has no private segment and no spill (metadata read as tests/test_build_artifacts.py does)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from benchnav_amd import _capi, build, gp

LLVM = "/opt/rocm/lib/llvm/bin"
GP_SYMBOLS = ("bn_gp_max_points", "bn_gp_create", "bn_gp_destroy", "bn_gp_workspace_bytes", "bn_gp_predict_async", "bn_gp_last_error")


def test_library_builds_and_exports_the_gp_symbols():
    assert "gp_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gp_kernels.hip"))
    lib = _capi.load()
    for name in GP_SYMBOLS:
        assert name in _capi.SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "benchnav_mppi.h")).read()
    for name in GP_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
    import benchnav_amd
    assert benchnav_amd.TraversabilityPredictor is gp.TraversabilityPredictor and benchnav_amd.GPSlipRegressor is gp.GPSlipRegressor
    assert benchnav_amd.load_slip_regressors is gp.load_slip_regressors


def _gp_kernel_metadata(so_path, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", so_path, os.devnull])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
    out = {}
    for i, s in enumerate(starts):
        blob = os.path.join(tmp, f"bundle{i}.bin")
        with open(blob, "wb") as f:
            f.write(data[s:(starts[i + 1] if i + 1 < len(starts) else len(data))])
        co = os.path.join(tmp, f"co{i}.o")
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={blob}", f"--output={co}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True, text=True)
        if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)\s+\.sgpr_count:\s+\d+\s+\.sgpr_spill_count:\s+(\d+)\s+\.symbol:\s+(\S+)\.kd"
                             r"[\s\S]*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)", notes):
            if "gp_" in m.group(3):
                out[m.group(3)] = {"private": int(m.group(1)), "sgpr_spills": int(m.group(2)), "vgpr": int(m.group(4)), "vgpr_spills": int(m.group(5))}
    return out


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")), reason="ROCm LLVM tools not installed")
def test_gp_kernels_have_no_private_segment_and_no_spill(tmp_path):
    """The predict kernel lives at one or two workgroups of 8 waves per CU (its k tile fills the LDS): a scratch segment or a spill
    in its MFMA loop would show at once.  128 VGPRs keep two workgroups (4 waves per SIMD) resident where the LDS allows it."""
    _capi.load()
    meta = _gp_kernel_metadata(build.LIB_PATH, str(tmp_path))
    predict = {k: v for k, v in meta.items() if "gp_predict_kernel" in k}
    bucket = {k: v for k, v in meta.items() if "gp_bucket_kernel" in k}
    assert len(predict) == 1 and len(bucket) == 1, sorted(meta)
    for v in list(predict.values()) + list(bucket.values()):
        assert v["private"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, meta
    assert next(iter(predict.values()))["vgpr"] <= 128, predict


def _gpu_present():
    return torch.cuda.is_available()


def test_c_abi_rejects_bad_arguments_before_touching_the_device():
    from benchnav_amd import _capi
    lib = _capi.load()
    assert lib.bn_gp_max_points() == gp.MAX_POINTS
    n = 4
    x, a, li = np.arange(n, dtype=np.float64), np.ones(n), np.eye(n)
    h = C.c_void_p()

    def create(n_=n, x_=x, a_=a, li_=li, c=0.0, s=1.0, l=1.0, nz=0.1):
        return lib.bn_gp_create(0, n_, x_.ctypes.data, a_.ctypes.data, li_.ctypes.data, c, s, l, nz, C.byref(h))
    bad_x, bad_li, up = x.copy(), li.copy(), li.copy()
    bad_x[2] = np.inf
    bad_li[3, 1] = np.nan
    up[0, 3] = np.nan                                    # above the diagonal: not read
    for kw, word in ((dict(n_=0), b"1024"), (dict(n_=gp.MAX_POINTS + 1), b"1024"), (dict(s=0.0), b"> 0"), (dict(l=-2.0), b"> 0"),
                     (dict(nz=0.0), b"> 0"), (dict(c=float("nan")), b"finite"), (dict(x_=bad_x), b"finite"), (dict(li_=bad_li), b"finite")):
        assert create(**kw) == _capi.BN_ERR_INVALID, kw
        assert word in lib.bn_gp_last_error(), (kw, lib.bn_gp_last_error())
    assert lib.bn_gp_create(0, n, None, a.ctypes.data, li.ctypes.data, 0.0, 1.0, 1.0, 0.1, C.byref(h)) == _capi.BN_ERR_INVALID
    assert lib.bn_gp_workspace_bytes(1, 256, 0) == 0 and lib.bn_gp_workspace_bytes(1, 256, 33) == 0
    assert lib.bn_gp_workspace_bytes(64, 65536, 4) == 64 * 65536 * 4 + 3328       # 4 B cells + 4 B (3 C + 1) rounded up to 256
    lib.bn_gp_destroy(None)
    if not _gpu_present():
        assert create(li_=up) == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_gp_last_error()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gp.GPSlipRegressor(np.float32([0.0, 1.0]), np.float32([0.0, 1.0]), 0.0, 0.5, 5.0, 0.01)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gp.TraversabilityPredictor(None, {})
