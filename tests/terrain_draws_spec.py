"""The terrain generator's random draws restated in NumPy integers and float32 ("The draws on the device"): the
specification csrc/terrain_kernels.hip's terrain_draws_kernel implements, independent of torch's generator.

MT19937 seeded with the low 32 bits of the seed; one float32 uniform per 32-bit output; the crater rejection loop, the crater
table, the fBm phases and the light source in the order benchnav_amd.terrain.replay_draws makes them on torch's CPU generator.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

MAX_ATTEMPTS = 1000
f32 = np.float32


def mt_seed(seed: int) -> np.ndarray:
    """init_genrand(seed & 0xffffffff): mt[i] = 1812433253 (mt[i-1] ^ (mt[i-1] >> 30)) + i."""
    mt = np.empty(624, np.uint32)
    x = int(seed) & 0xFFFFFFFF
    mt[0] = x
    for i in range(1, 624):
        x = (1812433253 * (x ^ (x >> 30)) + i) & 0xFFFFFFFF
        mt[i] = x
    return mt


def _mix(a, b):
    y = (a & np.uint32(0x80000000)) | (b & np.uint32(0x7FFFFFFF))
    return (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908B0DF), np.uint32(0))


def mt_twist(mt: np.ndarray) -> np.ndarray:
    """The next block of 624 state words, in the four dependent segments i < 227, 227 <= i < 454, 454 <= i < 623, i = 623."""
    nx = np.empty_like(mt)
    nx[:227] = mt[397:624] ^ _mix(mt[:227], mt[1:228])
    nx[227:454] = nx[:227] ^ _mix(mt[227:454], mt[228:455])
    nx[454:623] = nx[227:396] ^ _mix(mt[454:623], mt[455:624])
    nx[623] = nx[396] ^ _mix(mt[623:624], nx[0:1])[0]
    return nx


def temper(y: np.ndarray) -> np.ndarray:
    y = y ^ (y >> np.uint32(11))
    y = y ^ ((y << np.uint32(7)) & np.uint32(0x9D2C5680))
    y = y ^ ((y << np.uint32(15)) & np.uint32(0xEFC60000))
    return y ^ (y >> np.uint32(18))


class Stream:
    """The float32 uniforms of one seed: f32(r & 0xFFFFFF) * 2^-24 for each 32-bit output r, in order."""

    def __init__(self, seed: int) -> None:
        self.mt, self.out, self.pos, self.drawn = mt_seed(seed), None, 624, 0

    def _refill(self):
        self.mt = mt_twist(self.mt)
        self.out = ((temper(self.mt) & np.uint32(0xFFFFFF)).astype(np.float32) * f32(2.0 ** -24)).astype(np.float32)
        self.pos = 0

    def uniform(self) -> np.float32:
        if self.pos == 624:
            self._refill()
        self.pos += 1
        self.drawn += 1
        return self.out[self.pos - 1]

    def uniforms(self, n: int) -> np.ndarray:
        got = np.empty(n, np.float32)
        k = 0
        while k < n:
            if self.pos == 624:
                self._refill()
            m = min(n - k, 624 - self.pos)
            got[k:k + m] = self.out[self.pos:self.pos + m]
            self.pos += m
            k += m
        self.drawn += n
        return got


@dataclass
class SpecCrater:
    center: np.ndarray            # (2,) float32
    radius: np.float32
    angle: float                  # double
    n: int
    bounds: tuple                 # sx, sy, ex, ey, psx, psy
    fits: bool
    lin: np.ndarray               # (n,) float32, torch's scalar linspace
    neg_tan: np.float32


@dataclass
class SpecDraws:
    craters: List[SpecCrater]
    attempts: int
    gave_up: bool
    phases: np.ndarray
    light_uniforms: Optional[np.ndarray] = None
    light: Optional[np.ndarray] = None
    margins: List[float] = field(default_factory=list)    # per attempt, the least |overlap distance - threshold| / ulp(threshold)


def num_phases(G: int) -> int:
    h = (G + 2) // 2
    return (h + 1) ** 2 + (h - 1) ** 2


def crater_table(G: int, res: float, center: np.ndarray, radius: np.float32, angle: float) -> SpecCrater:
    N = G + 2
    x0 = G * res / 2 - G / 2 * res
    two_r = f32(2.0 * float(radius))
    n = int(np.ceil(two_r / f32(res)))
    cell = np.floor((center - f32(x0)).astype(np.float32) / f32(res)).astype(np.int64)
    cx, cy = (int(min(max(c, 0), G - 1)) for c in cell)
    sx, sy = max(cx - n // 2, 0), max(cy - n // 2, 0)
    ex, ey = min(cx + n // 2, N), min(cy + n // 2, N)
    psx, psy = max(n // 2 - cx, 0), max(n // 2 - cy, 0)
    fits = not (psx + (ex - sx) > n or psy + (ey - sy) > n)
    if n > 1:
        step = f32(two_r / f32(n - 1))
    else:
        step = f32(0)
    i = np.arange(n)
    lo = (-radius + (step * i.astype(np.float32)).astype(np.float32)).astype(np.float32)
    hi = (radius - (step * (n - 1 - i).astype(np.float32)).astype(np.float32)).astype(np.float32)
    lin = np.where(i < n // 2, lo, hi).astype(np.float32)
    rad = f32(f32(angle) * f32(np.pi / 180.0))                       # deg2rad in float32
    neg_tan = f32(-np.tan(np.float64(rad)))                          # the tangent in float64, rounded once
    return SpecCrater(center.astype(np.float32), f32(radius), float(angle), n, (sx, sy, ex, ey, psx, psy), fits, lin, neg_tan)


def light_vector(u_angle: np.float32, u_z: np.float32, lower: float, upper: float) -> np.ndarray:
    ang = f32(u_angle * f32(2 * np.pi))
    z = f32(f32(u_z * f32(upper - lower)) + f32(lower))
    rad = np.sqrt(f32(f32(1) - f32(z * z)))
    return np.array([f32(rad * f32(np.cos(np.float64(ang)))), f32(rad * f32(np.sin(np.float64(ang)))), z], np.float32)


def draws(seed: int, G: int, res: float, is_fractal: bool = True, is_crater: bool = True, num_craters: int = 3,
          crater_margin: float = 5, min_angle: float = 10, max_angle: float = 20, min_radius: float = 5, max_radius: float = 10,
          coloring=None) -> SpecDraws:
    s = Stream(seed)
    N = G + 2
    x0 = G * res / 2 - G / 2 * res
    span, org = f32((N - 1) * res - x0), f32(x0)
    rspan, rmin, margin = f32(max_radius - min_radius), f32(min_radius), f32(crater_margin)
    craters, count, gave_up, margins = [], 0, False, []
    if is_crater:
        while len(craters) < num_craters:
            cx = f32(f32(s.uniform() * span) + org)
            cy = f32(f32(s.uniform() * span) + org)
            r = f32(f32(s.uniform() * rspan) + rmin)
            overlap = False
            if craters:                                              # every earlier crater is compared (torch's any())
                dx, dy = (pxs - cx).astype(np.float32), (pys - cy).astype(np.float32)
                dist = np.sqrt(((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32))
                thr = ((prs + r).astype(np.float32) + margin).astype(np.float32)
                margins.append(float((np.abs(dist.astype(np.float64) - thr) / np.spacing(thr)).min()))
                overlap = bool((dist < thr).any())
            if not overlap:
                angle = float(s.uniform()) * (max_angle - min_angle) + min_angle
                craters.append(crater_table(G, res, np.array([cx, cy], np.float32), r, angle))
                pxs, pys, prs = (np.array([getattr(c, k) if k == "radius" else c.center[k] for c in craters], np.float32)
                                 for k in (0, 1, "radius"))
            count += 1
            if count > MAX_ATTEMPTS:
                gave_up = True
                break
    phases = s.uniforms(num_phases(G)) if is_fractal else np.zeros(0, np.float32)
    d = SpecDraws(craters, count, gave_up, phases, margins=margins)
    if coloring is not None and coloring is not False:
        lo, hi = (0.8, 1.0) if coloring is True else coloring
        ua, uz = s.uniform(), s.uniform()
        d.light_uniforms = np.array([ua, uz], np.float32)
        d.light = light_vector(ua, uz, float(lo), float(hi))
    return d


# the seed sets the device draws are checked on: (G, seeds, extra geometry)
SEED_SETS = {
    "g64": (64, list(range(256)), {}),
    "g33_giveup": (33, list(range(64)), {}),
    "g34_block_boundary": (34, list(range(32)), {}),
    "g256": (256, list(range(16)), {}),
    "big_seeds": (64, [2 ** 32 + 5, 2 ** 40 + 7, 2 ** 63 - 1], {}),
    "six_craters": (64, list(range(16)), {"num_craters": 6}),
}
RES = 0.5
