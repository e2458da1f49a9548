#!/usr/bin/env python3
"""Maps per second of the U-Net terrain classifier (benchnav_amd/unet.py, csrc/unet_kernels.hip): the device time of one forward
per map at 64^2, 128^2 and 256^2 for B = 1, 8 and 64 maps, measured twice -- the class maps alone
(TerrainClassifier.predict_classes) and colours -> slip mean / std through TraversabilityPredictor.predict_maps (ten classes, one
regressor of 256 points each).

The baseline is the specification module (tests/unet_spec.py: plain torch.nn with BatchNorm, float32) moved to the same device
and run under torch.no_grad() -- PyTorch's own convolutions, never this package in another mode; for the second measurement its
argmax feeds the same predict_maps(t_classes=...).  Weights and colours are the tests' seeded recipe (tests/unet_cases.py).

Method: every shape is warmed up on both sides (code objects, the library's algorithm search), then the two sides alternate;
a sample is `inner` back-to-back calls between two events on the stream (inner sized so that a sample lasts >= 20 ms), the
figure is the median of --reps samples per side.  At B = 1 the time stands beside the floor the weight traffic sets: the
57.3 MB of folded float32 parameters read once at the device's peak bandwidth.

    python tools/unet_rate.py [--reps 7] [--sizes 64 128 256] [--batches 1 8 64] [--out profiles/unet_rates.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES, BATCHES = (64, 128, 256), (1, 8, 64)
PEAK_HBM_BYTES_PER_S = 8.0e12            # MI355X HBM3E peak


def sample(fn, stream, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(inner):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(ours, base, stream, reps):
    """medians (ms per call) of the two sides, alternating, after a warm-up of both"""
    for fn in (ours, base, ours, base):
        fn()
    stream.synchronize()
    inner = [max(1, min(50, int(np.ceil(20.0 / max(sample(fn, stream, 1), 1e-3))))) for fn in (ours, base)]
    t = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((ours, base)):
            t[i].append(sample(fn, stream, inner[i]))
    return [float(np.median(v)) for v in t], [[round(x, 4) for x in v] for v in t], inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--batches", type=int, nargs="+", default=list(BATCHES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_rates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/unet_rate.py needs an MI355X (gfx950) device")
    import unet_cases as UC
    import unet_spec
    from benchnav_amd.gp import GPSlipRegressor, TraversabilityPredictor
    from benchnav_amd.unet import TerrainClassifier, param_count

    sd = UC.state_dict()
    clf = TerrainClassifier(sd, classes=UC.CLASSES)
    base = unet_spec.Unet(UC.CLASSES)
    base.load_state_dict(sd)
    base = base.float().eval().cuda()
    rng = np.random.default_rng(5)
    regs = {}
    for k in range(UC.CLASSES):
        x = rng.uniform(-30, 30, 256).astype(np.float32)
        y = (0.4 * np.tanh(x / (8.0 + k)) + 0.05 * rng.standard_normal(x.size)).astype(np.float32)
        regs[k] = GPSlipRegressor(x, y, 0.05 * k, 0.5, 5.0 + k, 0.0025)
    pred = TraversabilityPredictor(clf, regs)
    stream = torch.cuda.current_stream()
    weight_bytes = 4 * param_count(UC.CLASSES)
    floor_ms = weight_bytes / PEAK_HBM_BYTES_PER_S * 1e3
    rows = []
    with torch.no_grad():
        for G in args.sizes:
            for B in args.batches:
                colors = UC.draw_colors(1000 + G + B, B, G, G).cuda()
                slopes = (torch.rand(B, G, G, generator=torch.Generator().manual_seed(G + B)) * 60.0 - 30.0).cuda()
                agree = float((clf.predict_classes(colors).long() == base.predict(colors)).double().mean())
                (c_ms, cb_ms), c_all, c_inner = alternate(lambda: clf.predict_classes(colors), lambda: base.predict(colors), stream, args.reps)
                (p_ms, pb_ms), p_all, p_inner = alternate(lambda: pred.predict_maps(slopes, colors=colors),
                                                          lambda: pred.predict_maps(slopes, t_classes=base.predict(colors)), stream, args.reps)
                row = {"G": G, "B": B, "classes_ms": round(c_ms, 4), "classes_ms_per_map": round(c_ms / B, 4), "classes_maps_per_s": round(1e3 * B / c_ms, 1),
                       "torch_f32_classes_ms": round(cb_ms, 4), "torch_over_ours_classes": round(cb_ms / c_ms, 3),
                       "slip_ms": round(p_ms, 4), "slip_maps_per_s": round(1e3 * B / p_ms, 1), "torch_f32_classifier_slip_ms": round(pb_ms, 4),
                       "torch_over_ours_slip": round(pb_ms / p_ms, 3), "class_map_agreement_with_torch_f32": agree,
                       "samples_ms": {"classes": c_all[0], "torch_classes": c_all[1], "slip": p_all[0], "torch_slip": p_all[1]},
                       "calls_per_sample": {"classes": c_inner, "slip": p_inner},
                       "workspace_bytes": int(clf._lib.bn_unet_workspace_bytes(B, G, G))}
                if B == 1:
                    row["weight_traffic_floor_ms"] = round(floor_ms, 5)
                    row["classes_ms_over_floor"] = round(c_ms / floor_ms, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"what": "benchnav_amd.TerrainClassifier.predict_classes (classes_*) and TraversabilityPredictor.predict_maps(colors=...) (slip_*): "
                   f"device time of one call on one MI355X, events on the stream, median of {args.reps} samples alternating with the baseline "
                   "after a warm-up; baseline torch_*: tests/unet_spec.Unet in float32 on the same device (PyTorch's own ops)",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__,
           "folded_parameter_bytes": weight_bytes, "peak_hbm_bytes_per_s_assumed": PEAK_HBM_BYTES_PER_S, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    clf.close()


if __name__ == "__main__":
    main()
