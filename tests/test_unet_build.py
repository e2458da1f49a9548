"""CPU: the library builds with the U-Net kernels, the header, the binding and the exports agree, the kernels' code objects have no
private segment and no spill, and the C ABI rejects bad arguments before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from benchnav_amd import _capi, build, unet
from test_gp_build import LLVM

UNET_SYMBOLS = ("bn_unet_param_count", "bn_unet_create", "bn_unet_destroy", "bn_unet_workspace_bytes", "bn_unet_forward_async",
                "bn_unet_feature_layout", "bn_unet_conv2d_workspace_bytes", "bn_unet_conv2d_async", "bn_unet_maxpool_async", "bn_unet_last_error")
UNET_KERNELS = ("unet_conv_kernelILi1E", "unet_conv_kernelILi3E", "unet_conv_kernelILi7E", "unet_relayout_kernel", "unet_maxpool_kernel",
                "unet_head_kernel")


def test_library_builds_and_exports_the_unet_symbols():
    for src in ("unet_kernels.hip", "unet_host.cpp"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src))
    assert "unet_handle.h" in build.HEADERS
    lib = _capi.load()
    header = open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "benchnav_mppi.h")).read()
    declared = set(re.findall(r"\b(bn_unet_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(UNET_SYMBOLS) == {n for n in _capi.SYMBOLS if n.startswith("bn_unet_")}
    for name in UNET_SYMBOLS:
        assert getattr(lib, name) is not None
    import benchnav_amd
    assert benchnav_amd.TerrainClassifier is unet.TerrainClassifier and benchnav_amd.fold_state_dict is unet.fold_state_dict
    assert benchnav_amd.load_terrain_classifier is unet.load_terrain_classifier


def _unet_kernel_metadata(so_path, tmp):
    """tests/test_gp_build.py's _gp_kernel_metadata for the kernels named unet_* (that function keeps the gp_* kernels only): the
    register and scratch counts of the code objects' notes, nothing of their instructions."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", so_path, os.devnull])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
    out = []
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
            if "unet_" in m.group(3):
                out.append((m.group(3), {"private": int(m.group(1)), "sgpr_spills": int(m.group(2)), "vgpr": int(m.group(4)),
                                         "vgpr_spills": int(m.group(5))}))
    return out


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")), reason="ROCm LLVM tools not installed")
def test_unet_kernels_appear_once_without_private_segment_or_spill(tmp_path):
    """The convolution keeps 32 accumulator registers and 32 staging registers per lane.  vgpr_count is the unified count (VGPRs
    + AGPRs) out of 512 per SIMD lane: up to 168 keep three waves per SIMD, three workgroups per CU (its 40 KB of LDS allow four)."""
    _capi.load()
    meta = _unet_kernel_metadata(build.LIB_PATH, str(tmp_path))
    names = [n for n, _ in meta]
    assert len(names) == len(UNET_KERNELS), names
    for want in UNET_KERNELS:
        assert sum(want in n for n in names) == 1, (want, names)
    for n, v in meta:
        assert v["private"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (n, v)
        assert v["vgpr"] <= 168, (n, v)


def test_c_abi_rejects_bad_arguments_before_touching_the_device():
    lib = _capi.load()
    n = lib.bn_unet_param_count(10)
    assert n == unet.param_count(10) == 14323722 and lib.bn_unet_param_count(0) == 0 and lib.bn_unet_param_count(33) == 0
    assert lib.bn_unet_param_count(32) == unet.param_count(32)
    params = np.zeros(n, np.float32)
    h = C.c_void_p()

    def create(classes=10, p=params, count=None):
        return lib.bn_unet_create(0, classes, p.ctypes.data if p is not None else None, p.size if count is None else count, C.byref(h))
    bad = params.copy()
    bad[n // 2] = np.nan
    for kw, word in ((dict(classes=0), b"[1, 32]"), (dict(classes=33), b"[1, 32]"), (dict(count=n - 1), b"count"), (dict(p=bad), b"finite"),
                     (dict(p=None, count=n), b"null")):
        assert create(**kw) == _capi.BN_ERR_INVALID, kw
        assert word in lib.bn_unet_last_error(), (kw, lib.bn_unet_last_error())
    assert lib.bn_unet_create(0, 10, params.ctypes.data, n, None) == _capi.BN_ERR_INVALID
    # the workspace: 0 out of range
    assert lib.bn_unet_workspace_bytes(1, 64, 64) > 0 and lib.bn_unet_workspace_bytes(64, 256, 256) > 0
    for args in ((1, 48, 64), (1, 64, 48), (0, 64, 64), (1, 0, 64), (1, 64, 2080), (4097, 32, 32), (65, 512, 512), (1, -32, 32)):
        assert lib.bn_unet_workspace_bytes(*args) == 0, args
    # the forward and the single layers check their pointers and shapes first (the handle is never dereferenced here)
    fake = C.c_void_p(256)
    assert lib.bn_unet_forward_async(None, None, 1, 64, 64, fake, None, None, None, fake, 1 << 30) == _capi.BN_ERR_INVALID
    assert lib.bn_unet_forward_async(fake, None, 1, 64, 64, None, None, None, None, fake, 1 << 30) == _capi.BN_ERR_INVALID
    assert lib.bn_unet_forward_async(fake, None, 1, 48, 64, fake, None, None, None, fake, 1 << 30) == _capi.BN_ERR_INVALID
    assert b"multiples of 32" in lib.bn_unet_last_error()
    assert lib.bn_unet_forward_async(fake, None, 1, 64, 64, fake, None, None, None, fake, 16) == _capi.BN_ERR_INVALID
    assert b"workspace" in lib.bn_unet_last_error()

    def conv(a=fake, ca=3, skip=None, cb=0, up=0, maps=1, hin=8, win=8, w=fake, cout=4, k=3, stride=1, pad=1, out=fake, ws=fake, nbytes=1 << 20):
        return lib.bn_unet_conv2d_async(0, None, a, ca, skip, cb, up, maps, hin, win, w, None, cout, k, stride, pad, None, 0, out, ws, nbytes)
    for kw in (dict(a=None), dict(w=None), dict(out=None), dict(ws=None), dict(cb=2), dict(k=5), dict(stride=3), dict(pad=4), dict(ca=0),
               dict(cout=0), dict(cout=4097), dict(nbytes=16), dict(up=1, hin=7), dict(hin=0), dict(k=7, pad=0, hin=4), dict(maps=0)):
        assert conv(**kw) == _capi.BN_ERR_INVALID, kw
    assert lib.bn_unet_conv2d_workspace_bytes(3, 4, 3) == (32 * 64 + 64) * 4 and lib.bn_unet_conv2d_workspace_bytes(3, 4, 5) == 0
    assert lib.bn_unet_maxpool_async(0, None, None, 1, 4, 4, fake) == _capi.BN_ERR_INVALID
    assert lib.bn_unet_maxpool_async(0, None, fake, 0, 4, 4, fake) == _capi.BN_ERR_INVALID
    off, ch, fh, fw = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.bn_unet_feature_layout(1, 48, 64, 0, C.byref(off), C.byref(ch), C.byref(fh), C.byref(fw)) == _capi.BN_ERR_INVALID
    assert lib.bn_unet_feature_layout(1, 64, 64, 10, C.byref(off), C.byref(ch), C.byref(fh), C.byref(fw)) == _capi.BN_ERR_INVALID
    assert lib.bn_unet_feature_layout(2, 64, 96, 4, C.byref(off), C.byref(ch), C.byref(fh), C.byref(fw)) == _capi.BN_OK
    assert (ch.value, fh.value, fw.value) == (512, 2, 3) and off.value % 256 == 0 and off.value < lib.bn_unet_workspace_bytes(2, 64, 96)
    lib.bn_unet_destroy(None)
    if not torch.cuda.is_available():
        assert create() == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_unet_last_error()
        assert conv() == _capi.BN_ERR_NO_DEVICE
