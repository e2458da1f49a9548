#!/usr/bin/env python3
"""Maps per second and float64 FLOP/s of the exact-GP slip prediction (benchnav_amd/gp.py, csrc/gp_kernels.hip): the device time
of one TraversabilityPredictor.predict_maps call (events around bn_gp_predict_async, median of --reps after a warm-up) at
G = 256, four terrain classes with one regressor each, N = 256 / 1000 training points, B = 1 / 64 maps -- or the sizes and
batches of --sizes / --batches (the slab kernel's record, profiles/gp_large_rates.json: --sizes 2048 4096 9999 --batches 1 8).

FLOPs count the triangular work: per cell N (N + 1) for v = L^-1 k over the lower triangle (one multiply and one add per entry),
2 N for |v|^2, 2 N for k . alpha; the kernel evaluations (an exp each) are not counted.  `executed` counts what the MFMAs issue:
the row blocks padded to 16 (256 nb (nb + 1) per cell, nb = ceil(N / 16)).

Beside it at B = 1: the same prediction composed from PyTorch float64 operations on the same device (class by class: the
k(x, phi) matrix materialised, one matmul with L^-1), and NumPy float64 on the host.

Above 1024 points a row also holds the host's time and peak memory for factorize + bn_gp_create (the four classes, one after the
other) and, for the 16 x 16 corner of the first map, the float32 ulp distance to tests/gp_spec.posterior_cholesky; the NumPy
composition on the host is left out there.

    python tools/gp_rate.py [--reps 5] [--sizes 256 1000] [--batches 1 64] [--out profiles/gp_rates.json]
"""
from __future__ import annotations

import argparse
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

G, CLASSES = 256, 4
SIZES, BATCHES = (256, 1000), (1, 64)
SMALL_MAX = 1024            # the sizes of gp_predict_kernel; above, gp_slab_kernel
HYPER = [(0.5, 5.0, 0.0025), (0.05, 3.0, 0.01), (1.0, 10.0, 0.04), (0.3, 2.0, 0.01)]


def training_sets(n):
    out = []
    for k in range(CLASSES):
        rng = np.random.default_rng(100 + k)
        x = rng.uniform(-30, 30, n).astype(np.float32)
        y = (0.5 * np.tanh(x / (10.0 + k)) + 0.05 * rng.standard_normal(n)).astype(np.float32)
        out.append((x, y, 0.05 * k, *HYPER[k]))
    return out


def device_time(fn, stream, reps):
    fn()
    fn()
    stream.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), [round(t, 4) for t in times]


def torch_composed(sets, facts, slopes, classes):
    """one map, float64 torch ops on the device"""
    mean = torch.zeros_like(slopes, dtype=torch.float64)
    std = torch.zeros_like(mean)
    phi_all = slopes.to(torch.float64)
    for k, ((_, _, c, s, l, noise), (x, alpha, linv)) in enumerate(zip(sets, facts)):
        mask = classes == k
        phi = phi_all[mask]
        d = x[:, None] - phi[None, :]
        ks = s * torch.exp(-(d * d) / (2.0 * l * l))
        v = linv @ ks
        mean[mask] = c + alpha @ ks
        std[mask] = torch.sqrt(torch.clamp(s - (v * v).sum(0), min=0.0) + noise)
    return mean, std


def numpy_composed(sets, facts, slopes, classes):
    mean = np.zeros(slopes.shape, np.float64)
    std = np.zeros(slopes.shape, np.float64)
    for k, ((_, _, c, s, l, noise), (x, alpha, linv)) in enumerate(zip(sets, facts)):
        mask = classes == k
        phi = slopes[mask].astype(np.float64)
        d = x[:, None] - phi[None, :]
        ks = s * np.exp(-(d * d) / (2.0 * l * l))
        v = linv @ ks
        mean[mask] = c + alpha @ ks
        std[mask] = np.sqrt(np.maximum(s - (v * v).sum(0), 0.0) + noise)
    return mean, std


def ulp_sample(sets, pred, slopes, classes):
    """float32 ulp distance of the 16 x 16 corner of map 0 to tests/gp_spec.posterior_cholesky (rounded to float32)"""
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import gp_spec
    sl, cl = slopes[0, :16, :16].contiguous(), classes[0, :16, :16].contiguous()
    m, s = pred.predict_maps(sl, t_classes=cl)
    m, s, hs, hc = m.cpu().numpy(), s.cpu().numpy(), sl.cpu().numpy(), cl.cpu().numpy()
    worst = {"mean": 0.0, "std": 0.0}
    for k, (x, y, c, sc, l, noise) in enumerate(sets):
        mask = hc == k
        if not mask.any():
            continue
        wm, ws = gp_spec.posterior_cholesky(x, y, c, sc, l, noise, hs[mask])
        for name, dev, want in (("mean", m[mask], wm.astype(np.float32)), ("std", s[mask], ws.astype(np.float32))):
            d = np.abs(dev.astype(np.float64) - want.astype(np.float64))
            ulp = np.spacing(np.maximum(np.abs(dev), np.abs(want)).astype(np.float32)).astype(np.float64)
            worst[name] = max(worst[name], float((d / ulp).max()))
    out = {"sample_cells": 256, "sample_max_ulp_f32_mean_vs_posterior_cholesky": worst["mean"],
           "sample_max_ulp_f32_std_vs_posterior_cholesky": worst["std"]}
    print(json.dumps(out), flush=True)
    return out


def create_large(n):
    """The four regressors of a size above SMALL_MAX, made once for all batches: the host's time per class for factorize +
    bn_gp_create, the process's peak memory after the first class, and the factors (caught on their way into the constructor) for
    the PyTorch composition."""
    from benchnav_amd import gp
    sets, facts, times = training_sets(n), [], []
    inner = gp.factorize

    def catching(*a):
        facts.append(inner(*a))
        return facts[-1]
    gp.factorize = catching
    try:
        regs, peak = {}, 0
        for k, t in enumerate(sets):
            t0 = time.perf_counter()
            regs[k] = gp.GPSlipRegressor(*t)
            times.append(round(time.perf_counter() - t0, 2))
            peak = peak or resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
            print(json.dumps({"N": n, "class": k, "factorize_and_create_s": times[-1]}), flush=True)
    finally:
        gp.factorize = inner
    return {"regs": regs, "facts": facts, "host": {"factorize_and_create_s_per_class": times, "host_peak_rss_bytes_first_class": int(peak),
                                                   "torch_threads": torch.get_num_threads()}}


def measure(n, B, reps, facts_cache, large=None):
    from benchnav_amd.gp import GPSlipRegressor, TraversabilityPredictor, factorize
    sets = training_sets(n)
    regs = large["regs"] if large else {k: GPSlipRegressor(*t) for k, t in enumerate(sets)}
    pred = TraversabilityPredictor(None, regs)
    gen = torch.Generator().manual_seed(B * 10000 + n)
    slopes = (torch.rand(B, G, G, generator=gen) * 60.0 - 30.0).cuda()
    classes = torch.randint(0, CLASSES, (B, G, G), generator=gen).to(torch.int32).cuda()
    stream = torch.cuda.current_stream()
    ms, all_ms = device_time(lambda: pred.predict_maps(slopes, t_classes=classes), stream, reps)
    cells = B * G * G
    nb = (n + 15) // 16
    useful = cells * (n * (n + 1) + 4 * n)
    executed = cells * 256 * nb * (nb + 1)
    row = {"N": n, "B": B, "G": G, "classes": CLASSES, "launch_pair_ms": round(ms, 4), "launch_pair_ms_all": all_ms,
           "ms_per_map": round(ms / B, 4), "maps_per_s": round(1e3 * B / ms, 2), "f64_tflops_triangular": round(useful / ms * 1e-9, 3),
           "f64_tflops_executed_mfma": round(executed / ms * 1e-9, 3),
           "workspace_bytes": int(pred._lib.bn_gp_workspace_bytes(B, G * G, CLASSES))}
    if large:
        row.update(large["host"])
        if B == 1:
            row.update(ulp_sample(sets, pred, slopes, classes))
    if B == 1:
        if large:
            facts_cache[n] = large["facts"]
        if n not in facts_cache:
            facts_cache[n] = [factorize(*t) for t in sets]
        facts = facts_cache[n]
        dfacts = [tuple(torch.from_numpy(a).cuda() for a in f) for f in facts]
        tms, tall = device_time(lambda: torch_composed(sets, dfacts, slopes[0], classes[0]), stream, reps)
        m, s = pred.predict_maps(slopes[0], t_classes=classes[0], dtype=torch.float64)
        tm, ts = torch_composed(sets, dfacts, slopes[0], classes[0])
        row.update({"torch_f64_composed_ms": round(tms, 4), "torch_f64_composed_ms_all": tall,
                    "torch_f64_peak_k_matrix_bytes": int(n * int((classes[0] == 0).sum().item()) * 8),
                    "max_rel_std_diff_vs_torch_f64": float(((s - ts).abs() / ts).max().item())})
        if n <= SMALL_MAX:
            hs, hc = slopes[0].cpu().numpy(), classes[0].cpu().numpy()
            t0 = time.perf_counter()
            nm, ns = numpy_composed(sets, facts, hs, hc)
            host_s = time.perf_counter() - t0
            row.update({"numpy_host_ms": round(host_s * 1e3, 1),
                        "max_rel_std_diff_vs_numpy": float(np.max(np.abs(s.cpu().numpy() - ns) / ns)),
                        "max_abs_mean_diff_vs_numpy": float(np.max(np.abs(m.cpu().numpy() - nm)))})
        del dfacts
        if large:
            facts_cache.pop(n)
    if not large:
        for r in regs.values():
            r.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES), help="training points per class")
    ap.add_argument("--batches", type=int, nargs="+", default=list(BATCHES), help="maps per call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_rates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gp_rate.py needs an MI355X (gfx950) device")
    rows, cache = [], {}
    for n in args.sizes:
        large = create_large(n) if n > SMALL_MAX else None
        for B in args.batches:
            rows.append(measure(n, B, args.reps, cache, large))
            print(json.dumps(rows[-1]), flush=True)
        if large:
            for r in large["regs"].values():
                r.close()
            del large
    out = {"what": "benchnav_amd.TraversabilityPredictor.predict_maps: device time of one call (bucketing + predict kernels, events on "
                   f"the stream, median of {args.reps} after a warm-up) on one MI355X; FLOPs count the triangular work",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
