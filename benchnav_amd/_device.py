"""What the wrappers share on the Python side: the view of library-owned device memory, torch's current stream as the library
takes it, the device a `device` argument names, the error check, the base of every class that owns a library handle, the seed
checks, the reference Tree's capacity rule, and the plumbing of the two tree planners (rrt.py, clrrt.py)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _capi


class _DevArray:
    """Library-owned device memory exposed to torch through __cuda_array_interface__."""

    def __init__(self, ptr: int, shape, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def stream_ptr(dev) -> C.c_void_p:
    """torch's current stream on `dev`, as the `void *stream` of the library's *_async entry points."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_seed(seed) -> int:
    s = int(seed)
    if s < 0 or s > 0xFFFFFFFF:              # np.random.seed's range (set_randomness)
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    return s


def seed_array(seeds, B: int) -> np.ndarray:
    if len(seeds) != B:
        raise ValueError("one seed per instance")
    return np.array([_check_seed(s) for s in seeds], np.uint64)


def tree_capacity(n: int) -> int:
    """The reference Tree's capacity for n nodes: 1000 (tree.py:17), doubled while the tree does not fit."""
    cap = 1000
    while cap < n:
        cap *= 2
    return cap


def check(lib, family: str, code: int, last_error: Optional[str] = None, nonzero: bool = False):
    """Raise the family's last error (`last_error`, default bn_<family>_last_error) for a negative code -- some entry points
    return a count -- or, with `nonzero`, for any code but 0."""
    if code < 0 or (nonzero and code):
        raise _capi.BenchnavError(code, getattr(lib, last_error or f"bn_{family}_last_error")().decode("utf-8", "replace"))


def resolve_device(device, who: str, lenient: bool = False) -> torch.device:
    """The CUDA device, with its index, that `device` names for benchnav_amd.<who>.  None or an index-less CUDA device is the
    current device.  Any other kind of device is an error, or with `lenient` (the planners that receive the reference's
    `device` argument) the current device too.  Without a GPU nothing resolves: there is no CPU fallback."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"benchnav_amd.{who} needs an MI355X (gfx950) device; there is no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        if not lenient:
            raise RuntimeError(f"benchnav_amd.{who} runs on the GPU only (device={device!r})")
        dev = torch.device("cuda")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


class Handle:
    """One handle of the library's `family` (bn_<family>_destroy / _last_error / _device_buffer).  The owner sets `_lib` and, from
    the family's create call, `_handle` (a c_void_p); it is destroyed once -- by close(), by leaving a `with` block, or when the
    object goes (also during interpreter shutdown, with module globals gone: __del__ swallows what that raises).  `last_error`
    names the call that holds the family's error text if not bn_<family>_last_error; `nonzero_is_error`: not only negative codes raise."""
    family, last_error, nonzero_is_error = "", None, False
    _lib = _handle = dev = None              # dev: the torch device of the handle's memory, what buffer() and view() wrap for

    def _create(self, lib, cfg) -> None:
        """bn_<family>_create(&cfg, &handle), for a family created from a config struct: sets `_lib`, `_handle` and `dev`."""
        self._lib, self.dev = lib, torch.device("cuda", cfg.device_id)
        h = C.c_void_p()
        self._check(getattr(lib, f"bn_{self.family}_create")(C.byref(cfg), C.byref(h)))
        self._handle = h

    def _check(self, code: int) -> None:
        if code:
            check(self._lib, self.family, code, self.last_error, self.nonzero_is_error)

    def close(self) -> None:
        h = self._handle
        if h:
            getattr(self._lib, f"bn_{self.family}_destroy")(h)
            h.value = None                   # an alias the owner bound once (NativeMPPI._h) reads as closed too
        self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_buffer(self, which: int):
        """(device pointer, bytes) of the family's buffer `which`."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._check(getattr(self._lib, f"bn_{self.family}_device_buffer")(self._handle, which, C.byref(ptr), C.byref(nbytes)))
        return ptr.value, nbytes.value

    def view(self, ptr: int, shape, typestr="<f4") -> torch.Tensor:
        """Library memory on `dev` as a tensor: for a pointer the library hands back without a buffer id."""
        return torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.dev)

    def buffer(self, which: int, shape, typestr="<f4") -> torch.Tensor:
        """The family's buffer `which` as a tensor of `shape`, which must account for every byte of it."""
        ptr, nbytes = self.device_buffer(which)
        assert math.prod(shape) * int(typestr[2:]) == nbytes, (which, tuple(shape), typestr, nbytes)
        return self.view(ptr, shape, typestr)


class _PlannerHandle(Handle):
    """One handle of a tree planner's `family` ("rrt", "clrrt": bn_<family>_create / _device_buffer): B instances of one
    parameter set.  A subclass fills the family's config struct."""
    h = property(lambda self: self._handle)

    def __init__(self, lib, dev: torch.device, B: int, cfg):
        self._create(lib, cfg)
        self.B, self.used = B, False         # used: a plan has run, its streams are seeded


class _TreePlanner:
    """The plumbing RRT and CLRRT share.  The planner class names its handle type (`_handle_type`, constructed as
    (lib, dev, B, owner)) and carries `_lib`, `_dev`, `_handles`, `x_limits` and `y_limits`."""
    _handle_type = None
    _last_handle = None

    def _is_within_bounds(self, node: torch.Tensor) -> bool:
        x, y = node[:2]
        return self.x_limits[0] <= x.item() <= self.x_limits[1] and self.y_limits[0] <= y.item() <= self.y_limits[1]

    def _stream(self):
        return stream_ptr(self._dev)

    def _handle(self, B: int):
        if B not in self._handles:
            self._handles[B] = self._handle_type(self._lib, self._dev, B, self)
        return self._handles[B]

    def _launch(self, h, starts: np.ndarray, goals: np.ndarray, seeds: Optional[np.ndarray]) -> None:
        starts, goals = np.ascontiguousarray(starts, np.float32), np.ascontiguousarray(goals, np.float32)
        sp = seeds.ctypes.data if seeds is not None else None
        plan = getattr(self._lib, f"bn_{h.family}_plan_async")
        check(self._lib, h.family, plan(h.h, self._stream(), starts.ctypes.data, goals.ctypes.data, sp))
        h.used = True
        self._last_handle = h
        torch.cuda.current_stream(self._dev).synchronize()

    def _grow(self, h, starts: np.ndarray, goals: np.ndarray, samples: torch.Tensor) -> None:
        """bn_<family>_grow_from_samples_async on a contiguous float32 sample table, host or device, and the wait for it."""
        if samples.is_cuda:
            samples = samples.to(self._dev)
            where, ptr = _capi.BN_MEM_DEVICE, samples.data_ptr()
        else:
            keep = samples.numpy()
            where, ptr = _capi.BN_MEM_HOST, keep.ctypes.data
        grow = getattr(self._lib, f"bn_{h.family}_grow_from_samples_async")
        check(self._lib, h.family, grow(h.h, self._stream(), starts.ctypes.data, goals.ctypes.data, ptr, where))
        torch.cuda.current_stream(self._dev).synchronize()
