"""Restatements of the colouring step (the reference's TerrainColoring.set_terrain_class_coloring, terrain_properties.py:364-523)
for the tests of benchnav_amd.terrain's colouring and csrc/terrain_kernels.hip's terrain_noise / classes / color kernels:

  * classes_f32: generate_multi_terrain's float32 arithmetic in its order (min-max normalisation, thresholds, class chain)
  * colours_f32: create_shading's float32 arithmetic in its order on a (C, 3) colour table
  * colours_f64: the same formulas in float64 from the same float32 inputs: the reference's own float32 error shows as its
    distance to this, and that distance is the tests' yardstick (colour_bound)
  * noise_f32:   the library's own gradient noise, float32 operation by operation, Philox from rng_reference
  * copper_reference: the copper rows as matplotlib itself gives them (fixture making only; the tests read the stored rows)
"""
from __future__ import annotations

import os

import numpy as np
import torch

import rng_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
NOISE_WORD = 0x544E4F49                                       # 'TNOI'
_D = F32(0.70710677)
GRAD = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [_D, _D], [-_D, _D], [_D, -_D], [-_D, -_D]], F32)


def load_cases():
    """({name: dict of arrays} for every colouring case, {key: array} for the shared entries) of tests/golden/colouring.npz."""
    f = np.load(os.path.join(HERE, "golden", "colouring.npz"))
    cases = {}
    for name in f["cases"]:
        pre = f"{name}/"
        cases[str(name)] = {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
    shared = {k: f[k] for k in f.files if k.split("/")[0] not in cases}           # copper/C, occ/E_T_S_seed, cases
    return cases, shared


def normalised(occupancy):
    """The occupancy as set_terrain_class_coloring leaves it (:384-388): divided by its sum when that exceeds one, torch float32."""
    occ = torch.as_tensor(np.asarray(occupancy, F32)).clone()
    if occ.sum() > 1:
        occ /= occ.sum()
    return occ


def thresholds(occupancy):
    """(thr (C,) float32, start): torch's float32 cumsum * 100 and the first class with occupancy > 0 (:428-431)."""
    occ = normalised(occupancy)
    return (torch.cumsum(occ, dim=0) * 100).numpy().astype(F32), int((occ > 0).nonzero().min().item())


def classes_f32(noise, occupancy):
    """t_classes (G, G) int64 from a float32 noise field: nd = (n - min) / (max - min) * 100, then the reference's chain of masks."""
    n = np.asarray(noise, F32)
    thr, start = thresholds(occupancy)
    with np.errstate(invalid="ignore", divide="ignore"):
        nd = ((n - n.min()) / (n.max() - n.min()) * F32(100)).astype(F32)
    t = np.full(n.shape, -1, np.int64)
    for i in range(start, thr.size):
        mask = nd <= thr[i] if i == start else (nd > thr[i - 1]) & (nd <= thr[i])
        t[mask] = i
    return t


def _normals(h):
    """(nx, ny) of create_shading :494-506 in h's dtype: one-sided at the borders, the two differences halved in the interior."""
    dx = h[:, :-1] - h[:, 1:]
    dy = h[:-1, :] - h[1:, :]
    nx, ny = np.zeros_like(h), np.zeros_like(h)
    nx[:, :-1] += dx
    nx[:, 1:] += dx
    nx[:, 1:-1] /= 2
    ny[:-1, :] += dy
    ny[1:, :] += dy
    ny[1:-1, :] /= 2
    return nx, ny


def _shaded(h, t_classes, table, light, ambient, dt):
    h, table, L = np.asarray(h, F32).astype(dt), np.asarray(table, F32).astype(dt), np.asarray(light, F32).astype(dt)
    amb = dt(F32(ambient))                                    # the reference multiplies a float32 tensor by the Python float
    nx, ny = _normals(h)
    ln = np.sqrt((nx * nx + ny * ny) + dt(1))
    ux, uy, uz = nx / ln, ny / ln, dt(1) / ln
    shade = (L[0] * ux + L[1] * uy) + L[2] * uz
    c = table[np.clip(np.asarray(t_classes), 0, table.shape[0] - 1)]          # (G, G, 3); under / over take the end rows
    c = np.moveaxis(c, -1, 0)
    return np.clip(shade[None] * c + amb * c, 0, 1).astype(dt)


def colours_f32(h, t_classes, table, light, ambient=0.1):
    """(3, G, G) float32: every operation rounded to float32, in the reference's order."""
    return _shaded(h, t_classes, table, light, ambient, F32)


def colours_f64(h, t_classes, table, light, ambient=0.1):
    """(3, G, G) float64 from the same float32 inputs."""
    return _shaded(h, t_classes, table, light, ambient, np.float64)


def colour_bound(fx, table):
    """1.5 x the reference's own distance from the float64 restatement on the fixture's inputs."""
    orc = colours_f64(fx["heights"], fx["t_classes"], table, fx["light"], float(fx["ambient"]))
    return 1.5 * float(np.abs(fx["colors"].astype(np.float64) - orc).max())


def _fade(t):
    a = t * F32(6) - F32(15)
    b = t * a + F32(10)
    return ((t * t) * t) * b


def _corner(seed, a, b, p, q):
    w = R.philox4x32(a, b, NOISE_WORD, 0, R.lo32(seed), R.hi32(seed), rounds=10)[0]
    g = GRAD[(w & np.uint32(7)).astype(np.int64)]
    return g[..., 0] * p + g[..., 1] * q


def noise_f32(seed, G, feature_size=20.0):
    """The library's own noise field (G, G) float32 for one instance seed: float32 NumPy operations are the device's
    (each rounded once, no FMA), in the kernel's order."""
    seed = int(seed) % (1 << 64)
    f = F32(feature_size)
    x = np.arange(G, dtype=F32)
    u, v = np.broadcast_arrays((x / f)[None, :], (x / f)[:, None])
    fi, fj = np.floor(u), np.floor(v)
    ci, cj = fi.astype(np.int64), fj.astype(np.int64)
    p, q = u - fi, v - fj
    p1, q1 = p - F32(1), q - F32(1)
    d00, d10 = _corner(seed, ci, cj, p, q), _corner(seed, ci + 1, cj, p1, q)
    d01, d11 = _corner(seed, ci, cj + 1, p, q1), _corner(seed, ci + 1, cj + 1, p1, q1)
    wp, wq = _fade(p), _fade(q)
    l0 = d00 + wp * (d10 - d00)
    l1 = d01 + wp * (d11 - d01)
    out = l0 + wq * (l1 - l0)
    assert out.dtype == F32
    return out


def copper_reference(C):
    """(C, 3) float32 copper rows from matplotlib itself, as create_color_map :462-470 calls it."""
    import matplotlib
    import matplotlib.pyplot as plt
    norm = matplotlib.colors.Normalize(vmin=0, vmax=C - 1)
    return plt.cm.copper(norm(np.arange(C, dtype=np.int64)))[:, :3].astype(F32)
