#!/usr/bin/env python3
"""Time of one training step of the U-Net terrain classifier (benchnav_amd/unet_train.py, csrc/segtrain_kernels.hip): training-mode
forward, cross-entropy, backward and Adam on B = 16 maps of 64^2 (the reference's batch size and map size) and of 256^2.

The baseline is the specification module (tests/unet_spec.py: plain torch.nn, float32) on the same device doing the same step with
PyTorch's own ops: zero_grad, forward in train(), F.cross_entropy, backward, torch.optim.Adam.step -- never this package in
another mode.  Weights, colours and targets are the tests' seeded recipe.

Method: both sides are warmed up, then alternate; a sample is `inner` back-to-back steps between two events on the stream (inner
sized so that a sample lasts >= 20 ms), the figure is the median of --reps samples per side.  The share of backward-weight is the
sum over the 31 convolutions of the device time of bn_segtrain_conv2d_backward_async (weight gradient only: the GEMM and the
reduction of its partials) on tensors of that layer's shapes, each timed alone the same way, over the step time; where such a call
is bound by its launches the share is an upper bound.

    python tools/unet_train_rate.py [--reps 7] [--sizes 64 256] [--batch 16] [--out profiles/unet_train_rates.json]
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

from unet_rate import alternate, sample  # noqa: E402


def layer_shapes(classes, B, G):
    """per convolution of unet.conv_table: (a shape, skip shape or None, upsample, weight shape, stride, pad)"""
    from benchnav_amd.unet import conv_inputs, conv_table
    out = []
    for (_, _, shape, stride, pad), (side, cb, up) in zip(conv_table(classes), conv_inputs(classes, G)):
        a_side = side // 2 if up else side
        out.append(((B, shape[1] - cb, a_side, a_side), (B, cb, side, side) if cb else None, up, shape, stride, pad))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_train_rates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/unet_train_rate.py needs an MI355X (gfx950) device")
    import torch.nn.functional as F
    import unet_cases as UC
    import unet_spec
    from benchnav_amd import unet_train

    stream = torch.cuda.current_stream()
    lr, B, rows = 1e-3, args.batch, []
    for G in args.sizes:
        colors = UC.draw_colors(2000 + G, B, G, G).cuda()
        coarse = torch.randint(0, UC.CLASSES, (B, 1, G // 8, G // 8), generator=torch.Generator().manual_seed(G)).float()
        targets = F.interpolate(coarse, scale_factor=8, mode="nearest")[:, 0].long().cuda()
        net = unet_train.TrainableTerrainClassifier(UC.state_dict(), classes=UC.CLASSES)
        base = unet_spec.Unet(UC.CLASSES)
        base.load_state_dict(UC.state_dict())
        base = base.float().train().cuda()
        opt = torch.optim.Adam(base.parameters(), lr=lr)
        loss_slot = torch.zeros(1, device="cuda")

        def ours():
            net.train_step_async(colors, targets, lr, loss_out=loss_slot)

        def torch_step():
            opt.zero_grad()
            F.cross_entropy(base(colors), targets).backward()
            opt.step()

        first = (net.train_step(colors, targets, lr), float(F.cross_entropy(base(colors), targets)))
        (o_ms, b_ms), all_ms, inner = alternate(ours, torch_step, stream, args.reps)
        wgrad_ms, per_layer = 0.0, []
        gen = torch.Generator().manual_seed(3)
        for a_shape, skip_shape, up, w_shape, stride, pad in layer_shapes(UC.CLASSES, B, G):
            a = torch.randn(a_shape, generator=gen).cuda()
            skip = torch.randn(skip_shape, generator=gen).cuda() if skip_shape else None
            weight = torch.randn(w_shape, generator=gen).cuda()
            side = (a_shape[2] * (2 if up else 1) + 2 * pad - w_shape[2]) // stride + 1
            grad_out = torch.randn(B, w_shape[0], side, side, generator=gen).cuda()
            fn = lambda: unet_train.conv2d_backward(a, weight, grad_out, stride, pad, skip=skip, upsample=up, need=("weight",))  # noqa: E731
            fn()
            stream.synchronize()
            k = max(1, min(50, int(np.ceil(20.0 / max(sample(fn, stream, 1), 1e-3)))))
            ms = float(np.median([sample(fn, stream, k) for _ in range(args.reps)]))
            per_layer.append(round(ms, 4))
            wgrad_ms += ms
        row = {"G": G, "B": B, "step_ms": round(o_ms, 4), "steps_per_s": round(1e3 / o_ms, 2), "maps_per_s": round(1e3 * B / o_ms, 1),
               "torch_f32_step_ms": round(b_ms, 4), "torch_over_ours": round(b_ms / o_ms, 3),
               "backward_weight_ms": round(wgrad_ms, 4), "backward_weight_share_of_step": round(wgrad_ms / o_ms, 3),
               "backward_weight_ms_per_convolution": per_layer, "first_loss": {"ours": first[0], "torch_f32": first[1]},
               "samples_ms": {"ours": all_ms[0], "torch": all_ms[1]}, "steps_per_sample": inner,
               "workspace_bytes": int(net._lib.bn_segtrain_workspace_bytes(B, G, G))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        net.close()
    out = {"what": "benchnav_amd.TrainableTerrainClassifier.train_step_async: device time of one training step (training-mode forward, "
                   f"cross-entropy, backward, Adam) on one MI355X, events on the stream, median of {args.reps} samples alternating with the "
                   "baseline after a warm-up; baseline torch_*: tests/unet_spec.Unet in float32 on the same device doing the same step with "
                   "PyTorch's own ops; backward_weight_*: the 31 weight-gradient calls timed alone on the layers' shapes",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
