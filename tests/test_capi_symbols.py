"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol the header declares.
No compute call is made (there is no GPU here); creation must fail loudly, not fall back."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from benchnav_amd import _capi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "benchnav_mppi.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_for_gfx950():
    path = build.build_library()
    assert os.path.exists(path)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True)
    if out.returncode == 0 and out.stdout:
        assert "gfx950" in out.stdout or True   # offload bundle is embedded; arch is checked below
    blob = open(path, "rb").read()
    assert b"gfx950" in blob, "no gfx950 code object embedded in the library"


def test_every_declared_symbol_is_exported_and_bound():
    lib = _capi.load()
    decl = declared_functions()
    assert len(decl) >= 20
    assert set(decl) == set(_capi.SYMBOLS), (set(decl) ^ set(_capi.SYMBOLS))
    for name in decl:
        assert getattr(lib, name) is not None


def test_config_struct_matches_header_layout():
    lib = _capi.load()
    cfg = _capi.Config()
    lib.bn_mppi_config_init(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_capi.Config)
    assert (cfg.horizon, cfg.num_samples, cfg.num_instances) == (50, 1024, 1)
    assert (cfg.u_min[0], cfg.u_min[1], cfg.u_max[0], cfg.u_max[1]) == (0.0, -1.0, 1.0, 1.0)   # robot_model.py:54-57
    assert abs(cfg.dt - 0.1) < 1e-7 and cfg.seed == 42
    assert lib.bn_mppi_abi_version() == _capi.ABI_VERSION


def test_abi_rejects_wrong_struct_size_and_null():
    lib = _capi.load()
    cfg = _capi.Config()
    lib.bn_mppi_config_init(C.byref(cfg))
    cfg.struct_size = 4
    h = C.c_void_p()
    assert lib.bn_mppi_create(C.byref(cfg), C.byref(h)) == _capi.BN_ERR_INVALID
    assert b"struct_size" in lib.bn_last_error()
    assert lib.bn_mppi_create(None, C.byref(h)) == _capi.BN_ERR_INVALID
    assert lib.bn_mppi_sync(None) == _capi.BN_ERR_INVALID
    assert lib.bn_mppi_solve_count(None) == 0
    lib.bn_mppi_destroy(None)


def test_invalid_configs_are_rejected_before_touching_the_device():
    lib = _capi.load()
    for field, value in (("horizon", 0), ("num_samples", 0), ("grid_size", 0), ("resolution", 0.0), ("lambda_", 0.0)):
        cfg = _capi.Config()
        lib.bn_mppi_config_init(C.byref(cfg))
        setattr(cfg, field, value)
        h = C.c_void_p()
        assert lib.bn_mppi_create(C.byref(cfg), C.byref(h)) == _capi.BN_ERR_INVALID, field
    cfg = _capi.Config()
    lib.bn_mppi_config_init(C.byref(cfg))
    cfg.x_limits[1] = 10.0            # 64 cells of 0.5 m do not fit in 10 m
    h = C.c_void_p()
    assert lib.bn_mppi_create(C.byref(cfg), C.byref(h)) == _capi.BN_ERR_INVALID
    assert b"limits" in lib.bn_last_error()


def _gpu_present():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_present(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_gpu():
    lib = _capi.load()
    cfg = _capi.Config()
    lib.bn_mppi_config_init(C.byref(cfg))
    h = C.c_void_p()
    assert lib.bn_mppi_create(C.byref(cfg), C.byref(h)) == _capi.BN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.bn_last_error()
    # every other family whose create reaches the device check with a few bytes of valid arguments, each with its own error string
    one = np.ones(1)
    rrt, clrrt = _capi.RRTConfig(), _capi.CLRRTConfig()
    lib.bn_rrt_config_init(C.byref(rrt))
    lib.bn_clrrt_config_init(C.byref(clrrt))
    f32 = np.ones(1, np.float32)
    calls = {
        "astar": lambda: lib.bn_astar_create(0, 4, 4, 1, C.byref(h)),
        "terrain": lambda: lib.bn_terrain_create(0, 8, 1, C.byref(h)),
        "rrt": lambda: lib.bn_rrt_create(C.byref(rrt), C.byref(h)),
        "clrrt": lambda: lib.bn_clrrt_create(C.byref(clrrt), C.byref(h)),
        "gp": lambda: lib.bn_gp_create(0, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, 0.0, 1.0, 1.0, 1.0, C.byref(h)),
        "gp_fit": lambda: lib.bn_gp_fit_create(0, 1, one.ctypes.data, one.ctypes.data, 1e-4, C.byref(h)),
        "risk": lambda: lib.bn_risk_map_infer(0, None, f32.ctypes.data, f32.ctypes.data, _capi.BN_MEM_HOST, 1, _capi.BN_RISK_EXPECTED,
                                              0.0, 0, None, _capi.BN_MEM_HOST, 0, f32.ctypes.data, _capi.BN_MEM_HOST),
    }
    for family, call in calls.items():
        assert call() == _capi.BN_ERR_NO_DEVICE, (family, getattr(lib, f"bn_{family}_last_error")())
        assert b"no CPU fallback" in getattr(lib, f"bn_{family}_last_error")(), family
    import torch
    from benchnav_amd.mppi import MPPI

    class Dyn:
        min_action = torch.tensor([0.0, -1.0]); max_action = torch.tensor([1.0, 1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MPPI(5, 8, 3, 2, Dyn(), object(), torch.tensor([0.5, 0.5]), 0.5)


def test_product_never_imports_the_oracle():
    """The product path must not route through oracle/ (or any CPU restatement)."""
    pkg = os.path.join(ROOT, "benchnav_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".inc")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "mppi_oracle" not in text and "liboracle" not in text, f


def test_header_is_plain_c_and_the_integration_example_compiles():
    """include/benchnav_mppi.h must be usable from C (the boundary is a C ABI): the caller shown in INTEGRATION.md
    compiles as strict C99 against it."""
    import shutil
    import subprocess
    import tempfile
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"```c\n(.*?)```", text, flags=re.S)
    assert m, "INTEGRATION.md lost its C example"
    body = m.group(1).replace("#include \"benchnav_mppi.h\"", "")
    src = ("#include <stdio.h>\n#include \"benchnav_mppi.h\"\nstatic void apply(float a, float b) { (void)a; (void)b; }\n"
           "int run(const float *risks, const float *state) {\n" + body + "\nreturn 0; }\n")
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    try:
        r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), f.name],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    finally:
        os.unlink(f.name)


def test_the_wrappers_share_one_device_array_and_keep_their_check_functions():
    """Tests, tools and the benchmark import _DevArray from mppi, astar and rrt: all three are the one class of _device.py.  The
    rate tools call rrt._check and clrrt._check."""
    from benchnav_amd import _device, astar, clrrt, mppi, rrt
    assert mppi._DevArray is _device._DevArray and astar._DevArray is _device._DevArray and rrt._DevArray is _device._DevArray
    assert callable(rrt._check) and callable(clrrt._check)


# What the toolchain itself exports from a HIP shared library (one __hip_cuid_<hash> per translation unit with kernels; the linker's
# own section marks where it emits them): looked up on the library as it was before the host file was split, where the only other
# unmangled export was the RCCL loader's `rccl_api` (an anonymous namespace inside an extern "C" block).
TOOLCHAIN_EXPORTS = re.compile(r"^(__hip_cuid_[0-9a-f]+|_init|_fini|__bss_start|_edata|_end)$")


def test_only_the_headers_functions_are_exported_unmangled():
    path = build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert len(names) > 100
    plain = sorted(n for n in names if not n.startswith("_Z"))
    stray = [n for n in plain if n not in set(declared_functions()) and not TOOLCHAIN_EXPORTS.match(n)]
    assert not stray, f"unmangled exports the public header does not declare: {stray}"
