"""The seeded cases the U-Net tests share.  The 57 MB of weights are not a fixture: they are drawn from a seed on the machine
that runs the test, and every reference (the float64 spec, its float32 twin) is computed once per process and left unchanged.
Not a test module."""
import functools
import json
import os

import torch

import unet_spec

CLASSES = 10
WEIGHT_SEED = 1
# name -> (input seed, B, H, W): a 1 x 1 bottleneck (padding everywhere), a batch with a 2 x 2 bottleneck, a non-square map
CASES = {"b1_32x32": (1, 1, 32, 32), "b3_64x64": (2, 3, 64, 64), "b2_32x96": (4, 2, 32, 96)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet.json")
BOUND_FACTOR = 8.0          # device error <= 8 x the float32 CPU spec's own (k-ordered chains vs blocked sums, one-rounding BN fold)
MIN_CLASS_SHARE, MIN_CLASSES, MAX_EXCLUDED_SHARE = 0.02, 3, 0.002


def draw_state_dict(seed=WEIGHT_SEED, classes=CLASSES):
    """seed -> the float32 state dict of unet_spec.Unet: kaiming-normal convolutions, head bias N(0, 0.5), BatchNorm weight and
    running variance U(0.5, 1.5), bias and running mean N(0, 0.2)."""
    torch.manual_seed(seed)
    net = unet_spec.Unet(classes)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                if m.bias is not None:
                    m.bias.normal_(0.0, 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.2)
                m.running_mean.normal_(0.0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return {k: v.clone() for k, v in net.state_dict().items()}


def draw_colors(seed, B, H, W):
    """A coarse random image upsampled 8x nearest, mixed 0.8 / 0.2 with per-pixel uniform noise: float32 in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 3, H // 8, W // 8, generator=g)
    fine = torch.rand(B, 3, H, W, generator=g)
    return (0.8 * torch.nn.functional.interpolate(coarse, scale_factor=8, mode="nearest") + 0.2 * fine).contiguous()


@functools.lru_cache(maxsize=None)
def state_dict():
    return draw_state_dict()


@functools.lru_cache(maxsize=None)
def spec(dtype=torch.float64):
    net = unet_spec.Unet(CLASSES)
    net.load_state_dict(state_dict())
    return net.to(dtype).eval()


@functools.lru_cache(maxsize=None)
def colors(name):
    return draw_colors(*CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 logits, float64 encoder features, float64 decoder outputs) of the case."""
    with torch.no_grad():
        enc, dec = spec().features(colors(name).double())
        return spec().segmentation_head(dec[-1]), enc, dec


@functools.lru_cache(maxsize=None)
def float32_error(name):
    """The float32 CPU spec's largest |logit - float64 logit| relative to the largest |float64 logit|."""
    ref = reference(name)[0]
    with torch.no_grad():
        lo = spec(torch.float32)(colors(name))
    return float((lo.double() - ref).abs().max() / ref.abs().max())


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def logit_bound(name):
    """The relative bound on the device's logits (and features): BOUND_FACTOR x the recorded float32-CPU figure."""
    return BOUND_FACTOR * golden()[name]["float32_cpu_relative_error"]


def margin_mask(name):
    """Cells whose float64 top-two margin exceeds 2 x the absolute logit bound: where the class map must equal the float64 argmax."""
    ref = reference(name)[0]
    top = ref.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > 2.0 * logit_bound(name) * float(ref.abs().max())
