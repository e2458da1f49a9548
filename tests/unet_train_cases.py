"""The seeded cases the U-Net training tests share (benchnav_amd/unet_train.py): the layer shapes, the network
cases, and the float64 specification (tests/unet_spec.Unet in training mode with F.cross_entropy and torch.optim.Adam), computed
once per process and left unchanged.  `python tests/golden/make_golden_unet_train.py` records the float32 CPU spec's own distance
from float64 in tests/golden/unet_train.json; the device is held to unet_cases.BOUND_FACTOR times that.  Not a test module."""
import functools
import json
import os

import torch
import torch.nn.functional as F

import unet_cases as UC
import unet_spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_train.json")
EPS32 = 2.0 ** -23

# name: (B, Ca, h, w of a, Cout, k, stride, pad, Cb, upsample, wanted gradients); the smallest shapes that take each path
CONV_CASES = {
    "stem_7x7_s2_cin3_32x32": (1, 3, 32, 32, 16, 7, 2, 3, 0, False, ("weight",)),
    "3x3_s1_out1x1": (1, 5, 1, 1, 16, 3, 1, 1, 0, False, ("weight", "a")),
    "3x3_s1_out1x3_b3": (3, 64, 1, 3, 48, 3, 1, 1, 0, False, ("weight", "a")),
    "3x3_s1_out5x4_b3": (3, 5, 5, 4, 16, 3, 1, 1, 0, False, ("weight", "a")),
    "3x3_s1_out5x4_b1": (1, 5, 5, 4, 16, 3, 1, 1, 0, False, ("weight", "a")),
    "3x3_s2_in2x2": (1, 5, 2, 2, 10, 3, 2, 1, 0, False, ("weight", "a")),
    "3x3_s2_in4x4": (1, 64, 4, 4, 16, 3, 2, 1, 0, False, ("weight", "a")),
    "3x3_s2_in2x6_b3": (3, 5, 2, 6, 48, 3, 2, 1, 0, False, ("weight", "a")),
    "3x3_s2_odd_input_9x7": (1, 5, 9, 7, 10, 3, 2, 1, 0, False, ("weight", "a")),
    "1x1_s2_cin64_6x5": (3, 64, 6, 5, 48, 1, 2, 0, 0, False, ("weight", "a")),
    "3x3_cin768_2x2_k_slabs": (1, 768, 2, 2, 16, 3, 1, 1, 0, False, ("weight", "a")),
    "3x3_s1_9x9_b3_cout80": (3, 5, 9, 9, 80, 3, 1, 1, 0, False, ("weight", "a")),
    "3x3_s1_40x40_b3_split_pixels": (3, 5, 40, 40, 16, 3, 1, 1, 0, False, ("weight", "a")),
    "head_like_cout10_b3": (3, 16, 5, 4, 10, 3, 1, 1, 0, False, ("weight", "a")),
    "upsample_concat_a2x2x8_skip4x4x4": (1, 8, 2, 2, 16, 3, 1, 1, 4, True, ("weight", "a", "skip")),
    "upsample_concat_b3": (3, 8, 2, 2, 10, 3, 1, 1, 4, True, ("weight", "a", "skip")),
    "upsample_no_skip": (1, 8, 2, 2, 16, 3, 1, 1, 0, True, ("weight", "a")),
}
# the cases whose data gradient is also added into a non-zero destination
ACCUMULATE_CASES = ("3x3_s1_out5x4_b3", "3x3_s2_odd_input_9x7", "upsample_concat_b3")
# real-valued (N(0, 1)) gradients against float64: the split pixel axis, a strided one, the K slabs, the upsample-concat gather
REAL_CASES = ("3x3_s1_40x40_b3_split_pixels", "3x3_s2_odd_input_9x7", "3x3_cin768_2x2_k_slabs", "upsample_concat_b3")


def conv_inputs(name, integers=True):
    """(a, skip or None, weight, grad_out) of the case as float32, small integers or N(0, 1)."""
    B, ca, h, w, cout, k, stride, pad, cb, up, _ = CONV_CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + (0 if integers else 1000))
    draw = (lambda *s: torch.randint(-3, 4, s, generator=gen).to(torch.float32)) if integers else (lambda *s: torch.randn(*s, generator=gen))
    hin, win = (2 * h, 2 * w) if up else (h, w)
    a = draw(B, ca, h, w)
    skip = draw(B, cb, hin, win) if cb else None
    weight = draw(cout, ca + cb, k, k)
    ho, wo = (hin + 2 * pad - k) // stride + 1, (win + 2 * pad - k) // stride + 1
    return a, skip, weight, draw(B, cout, ho, wo)


def conv_reference(name, a, skip, weight, grad_out, dtype=torch.float64):
    """(grad_weight, grad_a, grad_skip or None) by torch.autograd.grad of F.conv2d in `dtype` on the CPU."""
    _, _, _, _, _, _, stride, pad, _, up, _ = CONV_CASES[name]
    a, weight = a.to(dtype).requires_grad_(), weight.to(dtype).requires_grad_()
    skip = None if skip is None else skip.to(dtype).requires_grad_()
    x = F.interpolate(a, scale_factor=2, mode="nearest") if up else a
    if skip is not None:
        x = torch.cat([x, skip], dim=1)
    y = F.conv2d(x, weight, None, stride, pad)
    leaves = [weight, a] + ([skip] if skip is not None else [])
    g = torch.autograd.grad(y, leaves, grad_out.to(dtype))
    return g[0], g[1], (g[2] if skip is not None else None)


def relative_error(got, want):
    """max |got - want| over max |want|, in float64"""
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


# ---- the network cases: name -> (input seed, B, H, W); 12, 6 and 4 values per channel at the bottleneck ----
CASES = {"b3_64x64": (2, 3, 64, 64), "b2_32x96": (4, 2, 32, 96), "b4_32x32": (6, 4, 32, 32)}
TRAJECTORY_CASE, TRAJECTORY_STEPS, TRAJECTORY_LR = "b3_64x64", 6, 1e-3


@functools.lru_cache(maxsize=None)
def colors(name):
    return UC.draw_colors(*CASES[name])


@functools.lru_cache(maxsize=None)
def targets(name):
    """A seeded coarse class image upsampled 8x nearest: (B, H, W) int64 in [0, CLASSES)."""
    seed, B, H, W = CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    coarse = torch.randint(0, UC.CLASSES, (B, 1, H // 8, W // 8), generator=g).float()
    return F.interpolate(coarse, scale_factor=8, mode="nearest")[:, 0].long().contiguous()


def spec_net(dtype):
    net = unet_spec.Unet(UC.CLASSES)
    net.load_state_dict(UC.state_dict())
    return net.to(dtype).train()


def spec_gradients(name, dtype):
    """(loss, {key: gradient}, state dict after the forward: the running statistics have taken one update) of the training-mode
    spec in `dtype`."""
    net = spec_net(dtype)
    loss = F.cross_entropy(net(colors(name).to(dtype)), targets(name))
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().clone() for k, p in net.named_parameters()}, {k: v.detach().clone() for k, v in net.state_dict().items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    return spec_gradients(name, torch.float64)


def spec_trajectory(dtype, weight_decay=0.0):
    """The losses of TRAJECTORY_STEPS steps of torch.optim.Adam(lr = TRAJECTORY_LR) on TRAJECTORY_CASE's one batch."""
    net = spec_net(dtype)
    opt = torch.optim.Adam(net.parameters(), lr=TRAJECTORY_LR, weight_decay=weight_decay)
    x, t, out = colors(TRAJECTORY_CASE).to(dtype), targets(TRAJECTORY_CASE), []
    for _ in range(TRAJECTORY_STEPS):
        opt.zero_grad()
        loss = F.cross_entropy(net(x), t)
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return out


@functools.lru_cache(maxsize=None)
def reference_trajectory():
    return spec_trajectory(torch.float64)


def relative_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def stats_keys(state):
    return [k for k in state if k.endswith("running_mean") or k.endswith("running_var")]


def stats_error(got_state, want_state):
    """The running statistics' largest |difference| over the largest |value| of the tensor, over all of them."""
    return max(relative_error(got_state[k], want_state[k]) for k in stats_keys(want_state))


def float32_figures(name):
    """What the golden file records per network case: the float32 CPU spec's distance from float64."""
    l64, g64, s64 = reference(name)
    l32, g32, s32 = spec_gradients(name, torch.float32)
    per = {k: relative_l2(g32[k], g64[k]) for k in g64}
    num = sum(float((g32[k].double() - g64[k]).norm()) ** 2 for k in g64) ** 0.5
    den = sum(float(g64[k].norm()) ** 2 for k in g64) ** 0.5
    return {"loss_float64": l64, "loss_relative_error": abs(l32 - l64) / abs(l64), "gradient_global_relative_l2": num / den,
            "gradient_worst_tensor_relative_l2": max(per.values()), "gradient_worst_tensor": max(per, key=per.get),
            "running_statistics_relative_error": stats_error(s32, s64)}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def loss_bound(figure):
    """BOUND_FACTOR x the recorded float32 CPU figure, floor 4 eps (relative)"""
    return UC.BOUND_FACTOR * max(figure, 4 * EPS32)
