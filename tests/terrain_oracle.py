"""Float64 restatement of the reference's terrain generation (terrain_properties.py set_terrain_geometry / set_traversability,
slip_model.py), on the draws benchnav_amd.terrain.replay_draws makes, plus a float32 mirror of the crater carving in the order the
device kernel (csrc/terrain_kernels.hip) and the reference use.

The discrete structure -- crater slice bounds, profile sizes -- comes from the draws as the reference computes it in float32;
the arithmetic on it is float64 here, so the reference's own float32 error shows as its distance to this oracle.
"""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GEOM_KEYS = ("is_fractal", "is_crater", "num_craters", "crater_margin", "min_angle", "max_angle", "min_radius", "max_radius")


def load_cases():
    """{name: dict of arrays} for every case of tests/golden/terrain*.npz."""
    out = {}
    f = np.load(os.path.join(HERE, "golden", "terrain.npz"))
    for name in f["cases"]:
        pre = f"{name}/"
        out[str(name)] = {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
    for big in ("terrain_256_fbm", "terrain_256_both"):
        g = np.load(os.path.join(HERE, "golden", big + ".npz"))
        out[big] = {k: g[k] for k in g.files}
    return out


def geometry(fx):
    v = dict(zip(GEOM_KEYS, fx["geom"]))
    return {k: (bool(x) if k.startswith("is_") else int(x) if k == "num_craters" else float(x)) for k, x in v.items()}


def draws_for(fx):
    from benchnav_amd.terrain import replay_draws
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return replay_draws(int(fx["seed"]), int(fx["G"]), float(fx["res"]), **geometry(fx))


def models_for(fx):
    from benchnav_amd.terrain import SlipParams
    return [SlipParams(*row) for row in fx["models"]]


def t_classes_for(fx):
    G = int(fx["G"])
    return fx["t_classes"] if "t_classes" in fx else np.zeros((G, G), np.int64)


def min_shift(h):
    return h - h.min()


def carve_f64(h, c):
    sx, sy, ex, ey, psx, psy = c.bounds
    lin = np.linspace(-float(c.radius), float(c.radius), c.n)
    d = np.sqrt(lin[:, None] ** 2 + lin[None, :] ** 2)
    prof = np.where(d <= c.radius, -np.tan(np.deg2rad(float(np.float32(c.angle)))) * (c.radius - d), 0.0)
    sl = prof[psy:psy + (ey - sy), psx:psx + (ex - sx)]
    h[sy:ey, sx:ex] = np.where(sl != 0, h[sy:ey, sx:ex] + sl, h[sy:ey, sx:ex])
    return min_shift(h)


def carve_f32(h, c, d=None):
    """The kernel's float32 operations: d = sqrt(x*x + y*y), p = (-tan) * (r - d) where d <= r, h + p where p != 0.  d defaults
    to IEEE (correctly rounded) sqrt as on the device; pass the reference's recorded distances (n, n) to replay the reference."""
    sx, sy, ex, ey, psx, psy = c.bounds
    lin = c.lin.astype(np.float32)
    r, nt = np.float32(c.radius), np.float32(c.neg_tan)
    if d is None:
        d = np.sqrt(lin[:, None] * lin[:, None] + lin[None, :] * lin[None, :])
    prof = np.where(d <= r, nt * (r - d), np.float32(0)).astype(np.float32)
    sl = prof[psy:psy + (ey - sy), psx:psx + (ex - sx)]
    h[sy:ey, sx:ex] = np.where(sl != 0, h[sy:ey, sx:ex] + sl, h[sy:ey, sx:ex])
    return (h - h.min()).astype(np.float32)


def ieee_dists(draws):
    """Each crater's (n, n) profile distances with IEEE float32 sqrt, as the device computes them."""
    return [np.sqrt(c.lin[:, None] * c.lin[:, None] + c.lin[None, :] * c.lin[None, :]) for c in draws.craters]


def reference_dists(fx, draws):
    """Each crater's (n, n) profile distances as the reference's torch.sqrt returned them when the fixture was made.  torch's
    vectorised CPU sqrt is not correctly rounded on every CPU, so these are data of the fixture, not recomputed here."""
    flat, out, off = fx["crater_dist"], [], 0
    for c in draws.craters:
        out.append(flat[off:off + c.n * c.n].reshape(c.n, c.n))
        off += c.n * c.n
    assert off == flat.size
    return out


def reference_draws(fx):
    """draws_for(fx) with each crater's linspace and -tan replaced by the values the reference's torch calls returned when the
    fixture was made (torch's CPU linspace depends on the CPU's vector width): the inputs the reference itself carved with."""
    import dataclasses
    d = draws_for(fx)
    lin, nt, off, craters = fx["crater_lin"], fx["crater_negtan"], 0, []
    for j, c in enumerate(d.craters):
        craters.append(dataclasses.replace(c, lin=lin[off:off + c.n].copy(), neg_tan=float(nt[j])))
        off += c.n
    assert off == lin.size and len(craters) == nt.size
    return dataclasses.replace(d, craters=craters)


def craters_f32(G, draws, dists=None):
    """Padded float32 heights after every crater.  With dists=reference_dists(...) this is the reference bit for bit; without,
    it is what the device computes (IEEE sqrt).  The two differ only where the reference's sqrt rounded differently."""
    h = np.zeros((G + 2, G + 2), np.float32)
    for i, c in enumerate(draws.craters):
        h = carve_f32(h, c, None if dists is None else dists[i])
    return h


def spectrum(G, res, phases, H=0.75, gain=10.0):
    """The final scaled state of generate_fractal_surface's grid (:254-295), float64 from the float32 phases."""
    N = G + 2
    h = N // 2
    grid = np.zeros((N, N), np.complex128)
    phi = (np.float32(2 * np.pi) * phases.astype(np.float32)).astype(np.float64)
    expo = -((H + 1) / 2)
    k = 0
    for y in range(h + 1):
        for x in range(h + 1):
            rad = float(x * x + y * y) ** expo if (x or y) else 0.0
            grid[y, x] = rad * np.exp(1j * phi[k])
            k += 1
            if x > 0 and y > 0:
                grid[-y, -x] = np.conj(grid[y, x])
    for y, x in ((h, 0), (0, h), (h, h)):
        grid[y, x] = grid[y, x].real
    for y in range(1, h):
        for x in range(1, h):
            rad = float(x * x + y * y) ** expo
            grid[y, N - x] = rad * np.exp(1j * phi[k])
            grid[N - y, x] = np.conj(grid[y, N - x])
            k += 1
    assert k == phases.size
    return grid * (abs(gain) * (N * res * 1e3) ** (H + 1 + 0.5))


def fbm_surface(G, res, phases, H=0.75, gain=10.0):
    return np.fft.ifft2(spectrum(G, res, phases, H, gain)).real / (res * 1e3) ** 2 * 1e-3


def slopes_f64(hp, res):
    gx = ((hp[:-2, 2:] - hp[:-2, :-2]) + 2 * (hp[1:-1, 2:] - hp[1:-1, :-2]) + (hp[2:, 2:] - hp[2:, :-2])) / (8 * res)
    gy = ((hp[2:, :-2] - hp[:-2, :-2]) + 2 * (hp[2:, 1:-1] - hp[:-2, 1:-1]) + (hp[2:, 2:] - hp[:-2, 2:])) / (8 * res)
    return np.rad2deg(np.arctan(np.sqrt(gx ** 2 + gy ** 2)))


def slip_f64(slopes, t_classes, models):
    mean = np.full(slopes.shape, np.inf)
    std = np.full(slopes.shape, np.inf)
    for c, m in enumerate(models):
        mask = t_classes == c
        phi = slopes[mask]
        base = m.slip_sensitivity * 1e-3 * np.abs(phi) ** m.slip_nonlinearity
        mean[mask] = np.clip(np.where(phi >= 0, base + m.slip_offset, -base + m.slip_offset), 0, 1)
        std[mask] = m.base_noise_scale + m.slope_noise_scale * np.abs(phi)
    return mean, std


def generate(G, res, draws, is_fractal, t_classes, models, H=0.75, gain=10.0):
    """heights, slopes, latent mean, latent std (G, G) float64 for one instance."""
    hp = np.zeros((G + 2, G + 2))
    for c in draws.craters:
        hp = carve_f64(hp, c)
    if is_fractal:
        hp = min_shift(hp + fbm_surface(G, res, draws.phases, H, gain))
    slopes = slopes_f64(hp, res)
    mean, std = slip_f64(slopes, t_classes, models)
    return {"heights": hp[1:-1, 1:-1], "slopes": slopes, "mean": mean, "std": std}


def oracle_for(fx):
    d = draws_for(fx)
    return generate(int(fx["G"]), float(fx["res"]), d, geometry(fx)["is_fractal"], t_classes_for(fx), models_for(fx))


def spread(fx, orc, key):
    """The reference's own float32 distance to the float64 restatement on one field."""
    return float(np.abs(fx[key].astype(np.float64) - orc[key]).max())


def tolerance(fx, orc, key):
    """1.5 x the reference's spread, floored at 4 float32 ulps of the field's largest magnitude (a field the reference
    happens to hit exactly still has a representable neighbourhood)."""
    return max(1.5 * spread(fx, orc, key), 4 * float(np.finfo(np.float32).eps) * float(np.abs(orc[key]).max()))
