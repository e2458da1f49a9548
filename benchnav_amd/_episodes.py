"""What the closed loops on a `BatchedPlanetaryEnv` share (AStarDWALoop, CLRRTLoop): the registration with env.reset(), the guard
that an episode has ONE driver, injected slip draws, the device log's pointers and the one place the environment's counters move."""
from __future__ import annotations

import ctypes as C
import weakref

import torch

from . import _capi
from ._device import Handle


class EpisodeLoop:
    """A loop names the rows of its log (`_noun`: "steps", "iterations"), the entry point that hands out its device log
    (`_buffers_fn`) and whether a row takes one of the environment's draws (`_row_draws`), and has a reset().  `_h` is the
    environment planner's handle, not the loop's; `_handle` is what the loop owns and close() closes (AStarDWALoop, a `Handle`, owns
    a library handle and takes close() and `with` from there)."""
    _noun = _buffers_fn = ""
    _row_draws = False
    _handle = None

    def __init__(self, env):
        self.env, self.B = env, env.B
        self._lib, self._h, self._dev = env.planner._lib, env.planner._h, env._dev
        self._rows = 0                                      # rows run since the last reset

    def _register(self):                                    # the end of a constructor: from here on env.reset() resets the loop too
        self.env._on_reset.append(weakref.WeakMethod(self.reset))

    def _guard(self, n) -> int:
        """Before a run of n rows: the stream, one driver per episode, n >= 1.  Returns int(n)."""
        env = self.env
        env._check_stream()
        if env._steps != self._rows:                        # (the environment counts steps: only another noun is spelled out)
            mine = f"{self._rows}" if self._noun == "steps" else f"{self._rows} {self._noun}"
            raise RuntimeError(f"the environment has taken {env._steps} steps since its reset, this loop {mine}: "
                               "drive an episode either with env.step or with run()")
        if int(n) < 1:
            raise ValueError(f"n_{self._noun} must be >= 1")
        return int(n)

    def _slip_draws(self, z, n: int):
        """z (n, B), injected slip draws, as a contiguous float32 device tensor; None stays None."""
        if z is None:
            return None
        zp = torch.as_tensor(z).to(self._dev, torch.float32).contiguous()
        if tuple(zp.shape) != (n, self.B):
            raise ValueError(f"z must be (n_{self._noun}, B) = {(n, self.B)}, got {tuple(zp.shape)}")
        return zp

    def episode_buffers(self):
        """Device pointers (states (cap + 1, B, 3), rewards (cap, B), done_step (B), stopped (B), both int32) of the latest run's
        log, its n and the row capacity `cap` the log is laid out for: what bn_episode_score reads.  Nothing is copied."""
        s, r, d, st, n, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        _capi.check(getattr(self._lib, self._buffers_fn)(self._h, C.byref(s), C.byref(r), C.byref(d), C.byref(st), C.byref(n), C.byref(cap)))
        return s.value, r.value, d.value, st.value, n.value, cap.value

    def _advance(self, n: int, state: torch.Tensor, elapsed=None) -> None:
        """The environment and the loop after a run of n rows.  env._robot_state becomes `state`: the log's last row
        (AStarDWALoop, as after env.run; with log=False a clone of the device row) or the tensor the kernel advanced (CLRRTLoop).
        env._steps += n for every driver.  env._draws += n where a row takes a draw (CLRRTLoop; not AStarDWALoop, not env.run).
        env._elapsed_time becomes `elapsed`; None is env.run's rule, += n * delta_t (AStarDWALoop).  A CLRRTLoop row need not be
        a step: with the log it passes the largest of its rovers' own times, without it the value the environment has."""
        env = self.env
        env._robot_state = state
        env._steps += n
        if self._row_draws:
            env._draws += n
        env._elapsed_time = env._elapsed_time + n * env._delta_t if elapsed is None else elapsed
        self._rows += n

    def close(self) -> None:
        """Close what the loop owns, once; env.reset() still finds the loop registered, so its reset() returns at once then."""
        h, self._handle = self._handle, None
        if h is not None:
            h.close()

    __enter__, __exit__ = Handle.__enter__, Handle.__exit__   # `with` as every handle owner has it
