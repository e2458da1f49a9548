"""CPU: the Python side of a bn_mppi_t -- the one function that fills bn_mppi_config, and the handle base's lifetime, error
check and buffer view against stub libraries.  The expected config fields are written out by hand from the two constructors
this function replaced (NativeMPPI: every switch, float32 1/(s*s); MPPI: seven switches, the inverted covariance, never the
private-stream flag)."""
import ctypes as C

import pytest

from benchnav_amd import _capi
from benchnav_amd._device import Handle
from benchnav_amd._mppi_handle import MPPIHandle, mppi_config

F = _capi
BASE = dict(horizon=50, num_samples=1024, num_instances=1, grid_size=64, resolution=0.5, x_limits=(0.0, 32.0), y_limits=(0.0, 32.0),
            sigma=(0.5, 0.5), inv_var=(4.0, 4.0), lambda_=0.5, u_min=(0.0, -1.0), u_max=(1.0, 1.0), dt=0.1, stuck_threshold=0.3,
            seed=42, device_id=0, stream=None)
# every switch as NativeMPPI's defaults pass it: no flag but the one of stream=None
NATIVE_DEFAULTS = dict(store_controls=False, shared_map=False, lds_window=True, profile=False, pipeline=True, sampled_slip=False,
                       lean=False, overlap=True, reference_order=False, host_paced=False, unordered_outputs=False, kernel="auto")


def _case(flags, stream=None, fields=None, **switches):
    args = dict(BASE, stream=stream, **(fields or {}))
    args.update(switches)
    return args, flags


CASES = [
    # NativeMPPI(...) with its defaults: a private stream, nothing else
    _case(F.BN_FLAG_PRIVATE_STREAM, **NATIVE_DEFAULTS),
    # ... on the null stream (torch's default): an int 0 is a stream, not "none"
    _case(0, stream=0, **NATIVE_DEFAULTS),
    # every positive switch, the wave kernel, a caller's stream
    _case(F.BN_FLAG_STORE_CONTROLS + F.BN_FLAG_SHARED_MAP + F.BN_FLAG_PROFILE + F.BN_FLAG_SAMPLED_SLIP + F.BN_FLAG_LEAN
          + F.BN_FLAG_REFERENCE_ORDER + F.BN_FLAG_HOST_PACED + F.BN_FLAG_UNORDERED_OUTPUTS + F.BN_FLAG_WAVE_KERNEL, stream=0x7F00DEAD0010,
          **dict(NATIVE_DEFAULTS, store_controls=True, shared_map=True, profile=True, sampled_slip=True, lean=True, reference_order=True,
                 host_paced=True, unordered_outputs=True, kernel="wave")),
    # every negative switch turned off, the role kernel, private stream
    _case(F.BN_FLAG_NO_LDS_WINDOW + F.BN_FLAG_NO_PIPELINE + F.BN_FLAG_NO_OVERLAP + F.BN_FLAG_ROLE_KERNEL + F.BN_FLAG_PRIVATE_STREAM,
          **dict(NATIVE_DEFAULTS, lds_window=False, pipeline=False, overlap=False, kernel="role")),
    # the latency kernel, host-paced, B = 3 on device 2, limits that are neither symmetric nor equal, another geometry
    _case(F.BN_FLAG_LAT_KERNEL + F.BN_FLAG_HOST_PACED, stream=0,
          fields=dict(horizon=4, num_samples=64, num_instances=3, grid_size=16, resolution=0.25, x_limits=(-3.0, 1.0), y_limits=(2.5, 6.5),
                      sigma=(0.25, 0.75), inv_var=(16.0, 1.7777777910232544), lambda_=0.125, u_min=(-0.5, -2.0), u_max=(1.5, 2.0), dt=0.05,
                      stuck_threshold=0.1, seed=2 ** 40 + 7, device_id=2),
          **dict(NATIVE_DEFAULTS, host_paced=True, kernel="lat")),
    # single switches, one at a time
    _case(F.BN_FLAG_SHARED_MAP + F.BN_FLAG_PRIVATE_STREAM, **dict(NATIVE_DEFAULTS, shared_map=True)),
    _case(F.BN_FLAG_NO_LDS_WINDOW, stream=0, **dict(NATIVE_DEFAULTS, lds_window=False)),
    _case(F.BN_FLAG_NO_PIPELINE, stream=0, **dict(NATIVE_DEFAULTS, pipeline=False)),
    _case(F.BN_FLAG_NO_OVERLAP, stream=0, **dict(NATIVE_DEFAULTS, overlap=False)),
    # MPPI(...) as the drop-in class calls it: its seven switches only, always a stream; defaults -> STORE_CONTROLS
    _case(F.BN_FLAG_STORE_CONTROLS, stream=0, store_controls=True, profile=False, sampled_slip=False, lean=False, reference_order=False,
          host_paced=False, unordered_outputs=False),
    # MPPI(noise="philox", host_loop="actions", lean=True, store_controls=False, profile=True): host_loop arrives as a truthy string
    _case(F.BN_FLAG_PROFILE + F.BN_FLAG_LEAN + F.BN_FLAG_HOST_PACED + F.BN_FLAG_UNORDERED_OUTPUTS, stream=0x55AA0000, store_controls=False,
          profile=True, sampled_slip=False, lean=True, reference_order=False, host_paced="actions", unordered_outputs=True),
    # MPPI(sampled_slip=True, reference_order=True)
    _case(F.BN_FLAG_STORE_CONTROLS + F.BN_FLAG_SAMPLED_SLIP + F.BN_FLAG_REFERENCE_ORDER, stream=0, store_controls=True, profile=False,
          sampled_slip=True, lean=False, reference_order=True, host_paced=False, unordered_outputs=False),
]


def _f32(v):
    return C.c_float(v).value


@pytest.mark.parametrize("args, flags", CASES)
def test_mppi_config_fills_every_field(args, flags):
    lib = _capi.load()
    cfg = mppi_config(lib, **args)
    assert cfg.struct_size == C.sizeof(_capi.Config)
    assert cfg.flags == flags
    assert cfg.stream == (args["stream"] or None)                 # c_void_p reads NULL back as None, for stream=0 and stream=None alike
    for name in ("device_id", "horizon", "num_samples", "num_instances", "grid_size", "seed"):
        assert getattr(cfg, name) == args[name], name
    for name in ("resolution", "lambda_", "dt", "stuck_threshold"):
        assert getattr(cfg, name) == _f32(args[name]), name
    for name in ("x_limits", "y_limits", "sigma", "inv_var", "u_min", "u_max"):
        assert list(getattr(cfg, name)) == [_f32(v) for v in args[name]], name


def test_the_cases_toggle_every_switch_and_every_kernel():
    from benchnav_amd._mppi_handle import _KERNELS, _SWITCHES
    for name in _SWITCHES:
        assert {bool(a[name]) for a, _ in CASES if name in a} == {False, True}, name
    assert {a.get("kernel", "auto") for a, _ in CASES} == set(_KERNELS) == {"auto", "wave", "role", "lat"}
    every = 0
    for _, flags in CASES:
        every |= flags
    assert every == 2 ** 15 - 1                                     # BN_FLAG_STORE_CONTROLS ... BN_FLAG_UNORDERED_OUTPUTS, all fifteen


def test_mppi_config_refuses_a_switch_it_does_not_know():
    with pytest.raises(KeyError, match="store_control"):
        mppi_config(_capi.load(), **dict(BASE, store_control=True))
    with pytest.raises(KeyError, match="fast"):
        mppi_config(_capi.load(), **dict(BASE, kernel="fast"))


# ---- lifetime, error check and buffer view, on stub libraries --------------------------------------------------------------
class _Stub:
    """A library of one family: bn_<family>_destroy counts, <error call> answers, bn_<family>_device_buffer reports 40 bytes."""

    def __init__(self, family, error_call):
        self.destroyed = []
        setattr(self, f"bn_{family}_destroy", lambda h: self.destroyed.append(h.value))
        setattr(self, error_call, lambda: f"{family} went wrong".encode())
        setattr(self, f"bn_{family}_device_buffer", self._device_buffer)

    @staticmethod
    def _device_buffer(h, which, ptr, nbytes):
        ptr._obj.value, nbytes._obj.value = 0x1000, 40
        return 0


class _Other(Handle):
    family = "terrain"


def _owner(cls, family, error_call):
    o = cls.__new__(cls)
    o._lib, o._handle = _Stub(family, error_call), C.c_void_p(0xBEEF)
    return o


@pytest.mark.parametrize("cls, family, error_call", [(MPPIHandle, "mppi", "bn_last_error"), (_Other, "terrain", "bn_terrain_last_error")])
def test_handle_is_destroyed_once_and_checks_with_its_familys_error(cls, family, error_call):
    o = _owner(cls, family, error_call)
    lib, alias = o._lib, o._handle
    o._check(0)                                                   # BN_OK does not raise
    with pytest.raises(_capi.BenchnavError, match=f"-4: {family} went wrong") as e:
        o._check(_capi.BN_ERR_STATE)
    assert e.value.code == _capi.BN_ERR_STATE
    with o as same:
        assert same is o and bool(o._handle)
        o.close()
        assert lib.destroyed == [0xBEEF] and not o._handle and not alias      # an alias bound before close() reads as closed too
        o.close()                                                 # a second close() ...
    assert lib.destroyed == [0xBEEF]                              # ... and leaving the block after it destroy nothing more
    o.__del__()
    assert lib.destroyed == [0xBEEF]
    with _owner(cls, family, error_call) as p:                    # leaving the block is what closes
        plib = p._lib
    assert plib.destroyed == [0xBEEF] and not p._handle


def test_a_positive_code_is_an_error_for_mppi_and_a_count_elsewhere():
    with pytest.raises(_capi.BenchnavError, match="mppi went wrong"):
        _owner(MPPIHandle, "mppi", "bn_last_error")._check(3)
    _owner(_Other, "terrain", "bn_terrain_last_error")._check(3)


def test_del_swallows_what_a_half_built_or_shut_down_owner_raises():
    o = MPPIHandle.__new__(MPPIHandle)                            # the constructor raised before create: nothing to destroy
    o.__del__()
    o = _owner(MPPIHandle, "mppi", "bn_last_error")
    o._lib = None                                                 # interpreter shutdown: the library object is gone
    o.__del__()


@pytest.mark.parametrize("cls, family, error_call", [(MPPIHandle, "mppi", "bn_last_error"), (_Other, "terrain", "bn_terrain_last_error")])
def test_buffer_asserts_that_the_shape_accounts_for_every_byte(cls, family, error_call):
    o = _owner(cls, family, error_call)
    assert o.device_buffer(0) == (0x1000, 40)
    for shape, typestr in (((9,), "<f4"), ((2, 5), "<f8"), ((40,), "<i4"), ((41,), "|u1")):
        with pytest.raises(AssertionError):
            o.buffer(0, shape, typestr)
