"""CPU: the library builds with the U-Net training kernels, the header, the binding and the exports agree on the bn_segtrain_*
symbols, and the segtrain_* kernels' code objects have no private segment and no spill."""
import os
import re
import subprocess

import pytest

from benchnav_amd import _capi, build
from test_gp_build import LLVM

SEGTRAIN_SYMBOLS = ("bn_segtrain_param_count", "bn_segtrain_create", "bn_segtrain_destroy", "bn_segtrain_workspace_bytes", "bn_segtrain_grad_async",
                    "bn_segtrain_step_async", "bn_segtrain_read", "bn_segtrain_steps", "bn_segtrain_conv2d_backward_workspace_bytes",
                    "bn_segtrain_conv2d_backward_async", "bn_segtrain_batchnorm_forward_async", "bn_segtrain_batchnorm_backward_async",
                    "bn_segtrain_maxpool_backward_async", "bn_segtrain_cross_entropy_async", "bn_segtrain_adam_async", "bn_segtrain_last_error")
SEGTRAIN_KERNELS = ("segtrain_wgrad_kernelILi1E", "segtrain_wgrad_kernelILi3E", "segtrain_wgrad_kernelILi7E", "segtrain_wgrad_reduce_kernel",
                    "segtrain_dgrad_kernelILi1E", "segtrain_dgrad_kernelILi3E", "segtrain_dgrad_kernelILi7E", "segtrain_flip_kernel",
                    "segtrain_split_kernel", "segtrain_bias_grad_kernel", "segtrain_bn_stats_kernel", "segtrain_bn_apply_kernel",
                    "segtrain_bn_bwd_sums_kernel", "segtrain_bn_bwd_dx_kernel", "segtrain_maxpool_bwd_kernel", "segtrain_ce_kernel",
                    "segtrain_mean_kernel", "segtrain_adam_kernel")


def test_library_builds_and_exports_the_segtrain_symbols():
    for src in ("segtrain_kernels.hip", "segtrain_host.cpp"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src))
    assert "segtrain_handle.h" in build.HEADERS
    lib = _capi.load()
    header = open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "benchnav_mppi.h")).read()
    declared = set(re.findall(r"\b(bn_segtrain_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(SEGTRAIN_SYMBOLS) == {n for n in _capi.SYMBOLS if n.startswith("bn_segtrain_")}
    for name in SEGTRAIN_SYMBOLS:
        assert getattr(lib, name) is not None
    import benchnav_amd
    from benchnav_amd import unet_train
    for name in ("TrainableTerrainClassifier", "ClassifierTrainer", "init_state_dict", "pack_state_dict", "unpack_params"):
        assert getattr(benchnav_amd, name) is getattr(unet_train, name)


def _segtrain_kernel_metadata(so_path, tmp):
    """tests/test_unet_build.py's _unet_kernel_metadata for the kernels named segtrain_*: the register and scratch counts of the
    code objects' notes, nothing of their instructions."""
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
            if "segtrain_" in m.group(3):
                out.append((m.group(3), {"private": int(m.group(1)), "sgpr_spills": int(m.group(2)), "vgpr": int(m.group(4)),
                                         "vgpr_spills": int(m.group(5))}))
    return out


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")), reason="ROCm LLVM tools not installed")
def test_segtrain_kernels_appear_once_without_private_segment_or_spill(tmp_path):
    """The two GEMM kernels keep 32 accumulator and 32 staging registers per lane like the forward convolution: up to 168 unified
    registers keep three waves per SIMD.  No kernel name may hold `unet_` or `gp_` (the filters of the other build tests)."""
    _capi.load()
    meta = _segtrain_kernel_metadata(build.LIB_PATH, str(tmp_path))
    names = [n for n, _ in meta]
    assert len(names) == len(SEGTRAIN_KERNELS), names
    for want in SEGTRAIN_KERNELS:
        assert sum(want in n for n in names) == 1, (want, names)
    for n, v in meta:
        assert "unet_" not in n and "gp_" not in n, n
        assert v["private"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (n, v)
        assert v["vgpr"] <= 168, (n, v)
