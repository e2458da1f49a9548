"""Writes tests/golden/unet_train.json: the float32 CPU specification's own distance from float64 on the cases of
tests/unet_train_cases.py -- the yardstick the device's training kernels are held to (unet_cases.BOUND_FACTOR times each figure).
CPU only; run from the repository root:  python tests/golden/make_golden_unet_train.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import unet_train_cases as TC  # noqa: E402


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    out = {"what": "float32 CPU spec against the float64 spec (tests/unet_spec.Unet in training mode, F.cross_entropy, torch.optim.Adam) on the "
                   "cases of tests/unet_train_cases.py; conv: max |error| of torch's float32 CPU convolution gradients over max |float64 gradient|",
           "torch": torch.__version__, "conv": {}, "network": {}, "trajectory": {}}
    for name in TC.REAL_CASES:
        a, skip, w, go = TC.conv_inputs(name, integers=False)
        want = TC.conv_reference(name, a, skip, w, go, torch.float64)
        got = TC.conv_reference(name, a, skip, w, go, torch.float32)
        out["conv"][name] = {k: TC.relative_error(g, r) for k, g, r in zip(("weight", "a", "skip"), got, want) if r is not None}
    for name in TC.CASES:
        out["network"][name] = TC.float32_figures(name)
    t64, t32 = TC.reference_trajectory(), TC.spec_trajectory(torch.float32)
    out["trajectory"] = {"case": TC.TRAJECTORY_CASE, "lr": TC.TRAJECTORY_LR, "loss_float64": t64,
                         "loss_relative_error": [abs(a - b) / abs(b) for a, b in zip(t32, t64)]}
    with open(TC.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
