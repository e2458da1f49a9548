"""CPU: the raised limit of the GP slip regressor (10240 training points) at the C ABI, the workspace that does not grow with
it, and gp_slab_kernel's code object: no private segment, no spill, and a register count that lets its 8 waves be resident
(metadata read with tests/test_gp_build.py's reader)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from benchnav_amd import _capi, build, gp
from test_gp_build import LLVM, _gp_kernel_metadata


def test_one_limit():
    lib = _capi.load()
    assert gp.MAX_POINTS == 10240 == lib.bn_gp_max_points()


def test_create_checks_the_new_limit_before_touching_the_device():
    lib = _capi.load()
    h = C.c_void_p()
    n = gp.MAX_POINTS + 1
    x, a = np.zeros(n), np.zeros(n)
    li = np.zeros(1)                                     # never read: n is checked first
    assert lib.bn_gp_create(0, n, x.ctypes.data, a.ctypes.data, li.ctypes.data, 0.0, 1.0, 1.0, 0.1, C.byref(h)) == _capi.BN_ERR_INVALID
    assert b"n must be in [1, 10240] training points" in lib.bn_gp_last_error()
    n = 1025
    x, a, li = np.linspace(-30.0, 30.0, n), np.ones(n), np.ascontiguousarray(np.tril(np.full((n, n), 1e-3)) + np.eye(n))
    rc = lib.bn_gp_create(0, n, x.ctypes.data, a.ctypes.data, li.ctypes.data, 0.0, 1.0, 1.0, 0.1, C.byref(h))
    if torch.cuda.is_available():
        assert rc == _capi.BN_OK and h.value
        lib.bn_gp_destroy(h)
    else:                                                # valid arguments: the device is the first thing missing
        assert rc == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_gp_last_error()
    bad = li.copy()
    bad[n - 1, 3] = np.inf                               # the checks reach the last row of a large matrix
    assert lib.bn_gp_create(0, n, x.ctypes.data, a.ctypes.data, bad.ctypes.data, 0.0, 1.0, 1.0, 0.1, C.byref(h)) == _capi.BN_ERR_INVALID
    assert b"finite" in lib.bn_gp_last_error()


def test_workspace_does_not_grow_with_the_limit():
    lib = _capi.load()
    assert lib.bn_gp_workspace_bytes(64, 65536, 4) == 64 * 65536 * 4 + 3328
    assert lib.bn_gp_workspace_bytes(1, 256, 1) == 1024 + 256
    assert lib.bn_gp_workspace_bytes(1, 256, 0) == 0 and lib.bn_gp_workspace_bytes(1, 256, 33) == 0


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")), reason="ROCm LLVM tools not installed")
def test_slab_kernel_has_no_private_segment_no_spill_and_fits_eight_waves(tmp_path):
    """gp_slab_kernel holds 16 accumulators of 4 doubles (128 registers) and one set of L^-1 fragments (32) per lane and runs one
    workgroup of 8 waves per CU (its two k chunks take 128 KB of LDS): 2 waves per SIMD, so at most 256 of the 512 registers of a
    lane each.  A spill in the MFMA loop would go to scratch memory."""
    _capi.load()
    meta = _gp_kernel_metadata(build.LIB_PATH, str(tmp_path))
    slab = {k: v for k, v in meta.items() if "gp_slab_kernel" in k}
    assert len(slab) == 1, sorted(meta)
    v = next(iter(slab.values()))
    assert v["private"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, slab
    assert 128 + 32 <= v["vgpr"] <= 256, slab
