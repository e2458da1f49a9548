"""NumPy restatement of TraversabilityModel._infer_risk_map (TEST INFRASTRUCTURE ONLY).

Follows reference traversability_model.py:28-51 with the sampling, quantile and tail mean spelled out:
  samples = z * std + mean                      Normal.sample == normal_().mul_(std).add_(mean)  
  var     = torch.quantile(samples, q, dim=0)   'linear': rank = fp32(q) * (n-1); lerp(below, above, frac)   (:35)
  cvar    = nanmean(where(samples > var, samples, nan), dim=0)                                    (:38-42)

The lerp is at::lerp as torch evaluates it, which is FUSED (its CPU vector path and the GPU compilers alike):
  |w| < 0.5:  fma(w, above - below, below)          else:  fma(w - 1, above - below, above)
one rounding of product plus addend.  Rounding the product first (what this file did before) differs from torch.quantile by
up to 0.5 ulp in a few cells of most maps; tests/test_risk_oracle_torch.py holds this file to torch.quantile by value.  The
float32 fma is emulated exactly (fma32).  A column that holds a NaN yields NaN, as torch.quantile does (np.sort alone would
put the NaN last and return a number); an all-inf column yields NaN through inf - inf in the lerp, again as torch.
Also pinned by tests/golden/riskmap.npz (outputs of the imported reference on the same z).
"""
import numpy as np

f32 = np.float32


def fma32(a, b, c):
    """float32 fma(a, b, c) = round32(a * b + c) with ONE rounding, elementwise.

    The float64 product of two float32 values is exact (48 significant bits).  The float64 sum p + c is not, and rounding it
    to float64 and then to float32 rounds twice.  So: two-sum gives the exact error e of the float64 sum s; where e != 0, s is
    moved to its odd-mantissa neighbour on e's side (round to odd).  Rounding that to float32 (53 >= 24 + 2 bits) equals
    rounding the exact value once."""
    a, b, c = (np.asarray(v, f32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def infer_risk_map(mean, std, metric, confidence=None, z=None):
    mean = np.asarray(mean, f32); std = np.asarray(std, f32)
    if metric == "expected_value":
        return mean.copy()
    z = np.asarray(z, f32)
    n = z.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        samples = ((z * std[None]).astype(f32) + mean[None]).astype(f32)
        srt = np.sort(samples, axis=0)
        pos = f32(f32(confidence) * f32(n - 1))
        lo_f = np.floor(pos); lo = int(lo_f); hi = int(np.ceil(pos)); w = f32(pos - lo_f)
        below, above = srt[lo], srt[hi]
        d = (above - below).astype(f32)               # inf - inf = NaN: an all-inf column
        if abs(w) < 0.5:                              # at::lerp, fused
            var = fma32(w, d, below)
        else:
            var = fma32(f32(w - f32(1)), d, above)
        var = np.where(np.isnan(samples).any(axis=0), f32(np.nan), var).astype(f32)
    if metric == "var":
        return var
    mask = samples > var[None]
    s = np.where(mask, samples, f32(0)).astype(np.float64).sum(axis=0)
    c = mask.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s / c).astype(f32)
