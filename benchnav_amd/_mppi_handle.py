"""The Python side of one bn_mppi_t: `mppi_config` fills bn_mppi_config, `MPPIHandle` owns the handle.  NativeMPPI (native.py) and
MPPI (mppi.py) derive from the one and call the other; nothing else writes a `_capi.Config` field or creates a bn_mppi_t
(`self._create(lib, mppi_config(lib, ...))`: the base's bn_<family>_create)."""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._device import Handle

# switch -> (its BN_FLAG_*, the value of the switch that sets the flag); a switch that is not passed leaves its flag clear
_SWITCHES = {
    "store_controls": (_capi.BN_FLAG_STORE_CONTROLS, True), "shared_map": (_capi.BN_FLAG_SHARED_MAP, True), "profile": (_capi.BN_FLAG_PROFILE, True),
    "sampled_slip": (_capi.BN_FLAG_SAMPLED_SLIP, True), "lean": (_capi.BN_FLAG_LEAN, True), "reference_order": (_capi.BN_FLAG_REFERENCE_ORDER, True),
    "host_paced": (_capi.BN_FLAG_HOST_PACED, True), "unordered_outputs": (_capi.BN_FLAG_UNORDERED_OUTPUTS, True),
    "lds_window": (_capi.BN_FLAG_NO_LDS_WINDOW, False), "pipeline": (_capi.BN_FLAG_NO_PIPELINE, False), "overlap": (_capi.BN_FLAG_NO_OVERLAP, False),
}
_KERNELS = {"auto": 0, "wave": _capi.BN_FLAG_WAVE_KERNEL, "role": _capi.BN_FLAG_ROLE_KERNEL, "lat": _capi.BN_FLAG_LAT_KERNEL}


def mppi_config(lib, *, horizon, num_samples, num_instances, grid_size, resolution, x_limits, y_limits, sigma, inv_var, lambda_,
                u_min, u_max, dt, stuck_threshold, seed, device_id, stream, kernel="auto", **switches) -> _capi.Config:
    """bn_mppi_config_init and every field of the struct; needs no GPU.  `inv_var` is the caller's own: MPPI inverts the covariance
    as the reference does, NativeMPPI takes float32 1/(s*s).  stream: an int hipStream_t (0 is the null stream, torch's default)
    or None for a stream of the handle's own (BN_FLAG_PRIVATE_STREAM).  switches: booleans named in _SWITCHES (else KeyError)."""
    cfg = _capi.Config()
    lib.bn_mppi_config_init(C.byref(cfg))
    cfg.horizon, cfg.num_samples, cfg.num_instances = horizon, num_samples, num_instances
    cfg.device_id, cfg.grid_size, cfg.resolution = device_id, grid_size, resolution
    for i in range(2):
        cfg.x_limits[i], cfg.y_limits[i] = x_limits[i], y_limits[i]
        cfg.sigma[i], cfg.inv_var[i] = sigma[i], inv_var[i]
        cfg.u_min[i], cfg.u_max[i] = u_min[i], u_max[i]
    cfg.lambda_, cfg.dt, cfg.stuck_threshold, cfg.seed, cfg.stream = lambda_, dt, stuck_threshold, seed, stream
    cfg.flags = _KERNELS[kernel] | (_capi.BN_FLAG_PRIVATE_STREAM if stream is None else 0)
    for name, value in switches.items():
        flag, sets = _SWITCHES[name]
        if bool(value) == sets:
            cfg.flags |= flag
    return cfg


class MPPIHandle(Handle):
    """The owner of one bn_mppi_t.  The MPPI family predates the per-family error strings: its text is the library's
    `bn_last_error`, and its entry points return BN_OK or an error, so every nonzero code raises (the few that return a count
    -- bn_mppi_solve_count, bn_mppi_row_pitch ... -- are read unchecked)."""
    family, last_error, nonzero_is_error = "mppi", "bn_last_error", True

    def arithmetic(self) -> str:
        """'spec' (default: carried heading vector, fused transit) or 'reference_order' (robot_model.py:86-88 as written)."""
        return "reference_order" if self._lib.bn_mppi_arithmetic(self._handle) == 1 else "spec"

    def kernel_ms(self):
        r, f, n = C.c_float(), C.c_float(), C.c_int32()
        self._check(self._lib.bn_mppi_kernel_ms(self._handle, C.byref(r), C.byref(f), C.byref(n)))
        return r.value, f.value, n.value

    def algorithmic_bytes(self, injected_noise: bool = True, window: bool = False) -> int:
        """SURVEY 8d's algorithmic bytes of one solve; window=True counts the reachable LDS window instead of the whole map."""
        kind = _capi.BN_NOISE_DEVICE_KT2 if injected_noise else _capi.BN_NOISE_PHILOX
        fn = self._lib.bn_mppi_algorithmic_bytes_window if window else self._lib.bn_mppi_algorithmic_bytes
        return int(fn(self._handle, kind))
