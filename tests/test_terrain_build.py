"""CPU: the terrain kernels (csrc/terrain_kernels.hip) are in the built library without a scratch segment or VGPR spills."""
import os

import pytest

from test_build_artifacts import LLVM, _kernel_metadata


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/clang-offload-bundler")), reason="ROCm LLVM tools not installed")
def test_terrain_kernels_have_no_scratch_and_no_spills(tmp_path):
    from benchnav_amd import _capi
    from benchnav_amd import build as b
    _capi.load()
    meta = _kernel_metadata(b.LIB_PATH, str(tmp_path))
    hits = {k: v for k, v in meta.items() if "terrain_" in k}
    names = {k.split("terrain_")[1].split("_kernel")[0] for k in hits}
    assert {"crater", "minshift", "spectrum", "dft_rows", "dft_cols", "surface"} <= names, sorted(hits)
    bad = {k: v for k, v in hits.items() if v["private"] or v["vgpr_spills"]}
    assert not bad, bad
