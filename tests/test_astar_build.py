"""CPU: the A* kernels (csrc/astar_kernels.hip) are in the built library without a scratch segment or VGPR spills."""
import os

import pytest

from test_build_artifacts import LLVM, _kernel_metadata


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")), reason="ROCm LLVM tools not installed")
def test_astar_kernels_have_no_scratch_and_no_spills(tmp_path):
    from benchnav_amd import _capi
    from benchnav_amd import build as b
    _capi.load()
    meta = _kernel_metadata(b.LIB_PATH, str(tmp_path))
    hits = {k: v for k, v in meta.items() if "astar_" in k}
    assert {"init", "field", "next"} <= {k.split("astar_")[1].split("_kernel")[0] for k in hits}, sorted(hits)
    bad = {k: v for k, v in hits.items() if v["private"] or v["vgpr_spills"]}
    assert not bad, bad
