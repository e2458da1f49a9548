"""Shared inputs of the risk-map edge tests (test_risk_oracle_torch.py on the CPU, test_gpu_risk_edges.py on the GPU).

Seeded inputs only: nothing here is a recorded result.  One 7 x 7 map (49 cells: the kernel's last workgroup holds one cell of
its four), sample counts on both sides of every lane-capacity (64 R) and instantiation (R = 16 / 32 / 64) edge, confidences
that reach both lerp branches, w = 0 and the first and last ranks, and named cells for the key orders a radix select can get
wrong.  Everything is computed once per process and handed out read-only."""
import functools

import numpy as np

import rng_reference as R

f32 = np.float32
G = 7
CELLS = G * G
NS = [2, 3, 63, 64, 65, 200, 1000, 1024, 1025, 2048, 2049, 4096]
QS = [0.0, 1e-4, 0.1, 1 / 3, 0.5, 0.75, 0.9, 0.975, 0.999, 1.0]
MAP_SEED = 20240611
Z_SEED = (9 << 32) | 0x7A                     # rng_reference.risk seed of the injected draws
HALVES_ROW = 3                                # cells 21..27: ordinary cells whose draws the "halves" variant quantises
VARIANTS = ("plain", "halves")

# flat cell index -> (mean, std).  Spread over several workgroups (cells 4 k .. 4 k + 3 share one); 48 is alone in the last.
NAMED = {
    "std0": (0, None, 0.0),                   # std = 0: every sample equals the (ordinary) mean
    "signed_zeros": (5, -0.0, 0.0),           # z * 0 + (-0.0): +0 where z > 0, -0 where z < 0
    "mixed_sign": (10, 0.0, 1.0),
    "all_negative": (47, -3.0, 1e-3),
    "rounded_ties": (48, 0.5, 1e-7),          # ulp(0.5) = 6e-8: the draws collapse onto a few values
}
DEGENERATE = ("std0", "signed_zeros", "rounded_ties")      # not part of the Philox cases (std = 0 / 1e-7)


def capacity(n):
    """Draws per lane of the instantiation that n selects."""
    return 16 if n <= 1024 else 32 if n <= 2048 else 64


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def maps(philox=False):
    """(mean, std) float32 (7, 7).  philox=True keeps the ordinary draw in the DEGENERATE cells."""
    rng = np.random.default_rng(MAP_SEED)
    mean = rng.uniform(-0.5, 0.7, CELLS).astype(f32)
    std = rng.uniform(0.0, 0.2, CELLS).astype(f32)
    for name, (cell, m, s) in NAMED.items():
        if philox and name in DEGENERATE:
            continue
        if m is not None:
            mean[cell] = f32(m)
        std[cell] = f32(s)
    return _ro(mean.reshape(G, G)), _ro(std.reshape(G, G))


@functools.lru_cache(maxsize=None)
def draws(n, variant="plain"):
    """z (n, 7, 7) float32: rng_reference.risk(Z_SEED, 49, n).  "halves": row HALVES_ROW rounded to multiples of 0.5, which ties
    whole runs of ranks (ranks lo and hi among them)."""
    assert variant in VARIANTS
    z = np.ascontiguousarray(R.risk(Z_SEED, CELLS, n).astype(f32).T).reshape(n, G, G)
    if variant == "halves":
        z[:, HALVES_ROW] = np.round(z[:, HALVES_ROW] * f32(2)) / f32(2)
    return _ro(z)


def samples(n, variant="plain", mean=None, std=None):
    """Normal.sample: normal_().mul_(std).add_(mean), each step rounded to float32."""
    if mean is None:
        mean, std = maps()
    with np.errstate(invalid="ignore", over="ignore"):
        return ((draws(n, variant) * std[None]).astype(f32) + mean[None]).astype(f32)


def rank(q, n):
    """torch.quantile's float32 rank arithmetic: (lo, hi, w)."""
    pos = f32(f32(q) * f32(n - 1))
    lo_f = np.floor(pos)
    return int(lo_f), int(np.ceil(pos)), f32(pos - lo_f)


def tail_mean64(smp, var):
    """float64 mean of the float32 samples strictly above var, and the scale sum|x| / c of the CVaR bound; NaN where no sample is."""
    mask = smp > var[None]
    c = mask.sum(axis=0)
    x = np.where(mask, smp, f32(0)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x.sum(axis=0) / c, np.abs(x).sum(axis=0) / c


def cvar_bound(n, scale):
    """|float32 tail mean - float64 tail mean| <= (R + 8) 2^-24 (sum|x| / c), derived, not measured.  Every float32 operation
    adds a relative 2^-24 of a partial sum that never exceeds sum|x|: R - 1 sequential adds per lane, six butterfly levels, the
    division and the final rounding make R + 7; one more covers the second-order terms.  The count c <= 4096 is exact."""
    return (capacity(n) + 8) * 2.0 ** -24 * scale
