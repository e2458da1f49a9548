"""GPU: the U-Net training step held to its own layers at the network's shapes (DESIGN.md 4.12 "Checks").  tests/unet_train_walk.py
recomposes forward, loss and backward from the device's single-layer functions -- they call the helpers csrc/segtrain_host.cpp's
seg_run calls -- in the documented order; tests/test_unet_train_walk.py holds that walk to the float64 spec on the CPU.  Here:

a. composition: TrainableTerrainClassifier.gradients() equals the device walk bit for bit (the head's bias gradient, which has no
   single-layer entry point, within one float32 ulp of the walk's float64 sum);
b. three train_steps with weight decay equal the walk plus the single-layer Adam bit for bit: parameters, exp_avg, exp_avg_sq,
   running statistics, loss, step counts;
c. every primitive call of that walk, which sees real activations at the real shapes, against TorchBackend(float64) of the same call
   on the device's own float32 inputs.  Errors do not propagate from layer to layer, so the bounds are the layer tests'.

Every bound comes from the CPU reference or the project's constants, never from the device."""
import functools

import numpy as np
import pytest
import torch

import unet_cases as UC
import unet_train_cases as TC
from test_gpu_unet_train_layers import _ulp_of_max, _within_one_ulp
from unet_train_walk import DeviceBackend, TorchBackend, walk

pytestmark = pytest.mark.gpu

CASES = sorted(TC.CASES)


def _net():
    from benchnav_amd import unet_train
    return unet_train.TrainableTerrainClassifier(UC.state_dict(), classes=UC.CLASSES)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _first_difference(got, want, order):
    """The first key, in `order`, whose tensors differ in a bit, with the count of differing elements and the largest difference."""
    for k in order:
        if not _same_bits(got[k], want[k]):
            g, w = got[k].cpu(), want[k].cpu()
            return k, int((_bits(g) != _bits(w)).sum()), float((g.double() - w.double()).abs().max())
    return None


@functools.lru_cache(maxsize=None)
def _device_walk(name):
    """(loss, gradients, running statistics, every primitive call) of the device walk from the seeded state: once per module."""
    calls = []
    loss, grads, stats = walk(DeviceBackend(), UC.state_dict(), TC.colors(name), TC.targets(name), observe=lambda *call: calls.append(call))
    return loss, grads, stats, calls


# ---- a. composition ----
@pytest.mark.parametrize("name", CASES)
def test_gradients_equal_the_walk_over_single_layers_bit_for_bit(name):
    want_loss, want, _, calls = _device_walk(name)
    with _net() as net:
        loss, got = net.gradients(TC.colors(name), TC.targets(name))
    bias = "segmentation_head.0.bias"
    assert set(got) == set(want) and list(want)[1] == bias
    assert loss == want_loss, (loss, want_loss)
    order = [k for k in want if k != bias]                  # the walk's insertion order is the backward's
    assert len(order) == 91
    assert _first_difference(got, want, order) is None, ("first differing gradient in backward order", _first_difference(got, want, order))
    (float64_sum,) = [out for kind, _, _, out in calls if kind == "bias_grad"]
    _within_one_ulp(got[bias], float64_sum.cpu(), bias)


# ---- b. three steps ----
def test_three_train_steps_equal_the_walk_and_the_single_layer_adam_bit_for_bit():
    from benchnav_amd import unet_train
    name, lr, weight_decay, betas, eps = "b4_32x32", 1e-3, 1e-2, (0.9, 0.999), 1e-8
    x, t = TC.colors(name), TC.targets(name)
    be, ref = DeviceBackend(), TorchBackend(torch.float64)
    worst = 0.0
    with _net() as net:
        for step in (1, 2, 3):
            state, (m, v) = net.state_dict(), net.adam_state()
            want_loss, grads, stats = walk(be, state, x, t)
            assert set(grads) == set(m) == set(v)
            want_p, want_m, want_v = {}, {}, {}
            for k, g in grads.items():
                want_p[k], want_m[k], want_v[k] = be.adam(state[k], g, m[k], v[k], step, lr, weight_decay, betas, eps)
                for what, got, spec in zip("pmv", (want_p[k], want_m[k], want_v[k]), ref.adam(state[k], g, m[k], v[k], step, lr, weight_decay, betas, eps)):
                    worst = max(worst, float((got.cpu().double() - spec).abs().max()) / _ulp_of_max(spec))
                    _within_one_ulp(got, spec, ("the single-layer Adam against the float64 formula", k, what, step))
            loss = net.train_step(x, t, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
            after, (m, v) = net.state_dict(), net.adam_state()
            step_grads = unet_train.unpack_params(net._read(unet_train.READ_GRADIENTS), UC.CLASSES, trainable_only=True)
            assert loss == want_loss, (step, loss, want_loss)
            assert net.steps == step
            tracked = [k for k in after if k.endswith("num_batches_tracked")]
            assert len(tracked) == 30 and all(after[k].dtype == torch.int64 and int(after[k]) == step for k in tracked)
            order = [k for k in grads if k != "segmentation_head.0.bias"] + ["segmentation_head.0.bias"]
            for what, got, want in (("gradient", step_grads, grads), ("parameter", after, want_p), ("exp_avg", m, want_m), ("exp_avg_sq", v, want_v),
                                    ("running statistic", after, stats)):
                assert _first_difference(got, want, order if want is not stats else sorted(stats)) is None, (
                    step, what, "first difference in backward order", _first_difference(got, want, order if want is not stats else sorted(stats)))
            assert len(stats) == 60 and set(after) == set(want_p) | set(stats) | set(tracked)
    print(f"\nAdam, 92 tensors x 3 steps x (p, m, v): worst error {worst:.3f} ulp of the tensor's largest magnitude (bound 1)")


# ---- c. teacher-forced float64 per layer ----
def _relative(got, ref64, ref32):
    """(the device's error over its bound, that bound): error relative to the tensor's largest |value|, bound BOUND_FACTOR x max(the
    float32 CPU figure of the same call on the same inputs, 4 eps)."""
    bound = TC.loss_bound(TC.relative_error(ref32, ref64))
    return TC.relative_error(got.cpu(), ref64) / bound, bound


def _ulps(got, ref64):
    return float((got.cpu().double() - ref64.double()).abs().max()) / _ulp_of_max(ref64)


def _check_call(kind, inputs, out, ref64, ref32):
    """[(what, the device's figure over its bound, passed)] for one recorded primitive call."""
    want = getattr(ref64, kind)(**inputs)
    res = []
    if kind == "conv":
        ratio, _ = _relative(out, want, ref32.conv(**inputs))
        res.append(("forward convolution", ratio, out.dtype == torch.float32 and out.shape == want.shape and ratio <= 1.0))
    elif kind == "conv_backward":
        want32 = ref32.conv_backward(**inputs)
        for what, g, w, w32 in zip(("grad_weight", "grad_a", "grad_skip"), out, want, want32):
            if w is None:
                res.append((what, 0.0, g is None))
                continue
            ratio, _ = _relative(g, w, w32)
            res.append((what, ratio, g.dtype == torch.float32 and g.shape == w.shape and ratio <= 1.0))
    elif kind == "batchnorm":
        (y, stats, rm, rv), (wy, wstats, wrm, wrv) = out, want
        for what, g, w in (("batchnorm y", y, wy), ("running_mean", rm, wrm), ("running_var", rv, wrv)):
            res.append((what, _ulps(g, w), g.dtype == torch.float32 and g.shape == w.shape and _ulps(g, w) <= 1.0))
        s = stats.cpu()
        s = s if s.shape == wstats.shape else torch.full_like(wstats, float("nan"))
        rel = float(((s - wstats).abs() / (1e-12 * wstats.abs())).max())       # mean and 1 / sqrt(var + eps) in float64: rtol 1e-12, no atol
        res.append(("batchnorm stats", rel, s.dtype == torch.float64 and rel <= 1.0))
    elif kind == "batchnorm_backward":
        (gx, gres, gg, gb), (wx, wres, wg, wb) = out, want
        for what, g, w in (("batchnorm grad_x", gx, wx), ("grad_gamma", gg, wg), ("grad_beta", gb, wb)):
            res.append((what, _ulps(g, w), g.dtype == torch.float32 and g.shape == w.shape and _ulps(g, w) <= 1.0))
        if inputs["residual"]:
            same = _same_bits(gres, ref32.batchnorm_backward(**inputs)[1])          # grad_out under the mask: exact in float32
            res.append(("grad_residual", 0.0 if same else float("inf"), same))
        else:
            res.append(("grad_residual", 0.0, gres is None and wres is None))
    elif kind == "maxpool":
        same = _same_bits(out, ref32.maxpool(**inputs))
        res.append(("max-pool forward", 0.0 if same else float("inf"), same))
    elif kind == "maxpool_backward":
        into = inputs["into"]
        S = ref64.maxpool_backward(inputs["x"], inputs["grad_out"].abs(), None if into is None else into.abs())
        bound = 2.5 * np.spacing(S.to(torch.float32).numpy()).astype(np.float64)
        ratio = float(((out.cpu().double() - want).abs().numpy() / bound).max())
        res.append(("max-pool backward", ratio, out.dtype == torch.float32 and out.shape == want.shape and ratio <= 1.0))
    elif kind == "cross_entropy":
        (loss, grad), (wloss, wgrad) = out, want
        res.append(("loss", _ulps(loss.reshape(()), wloss), loss.dtype == torch.float32 and _ulps(loss.reshape(()), wloss) <= 1.0))
        res.append(("grad_logits", _ulps(grad, wgrad), grad.dtype == torch.float32 and grad.shape == wgrad.shape and _ulps(grad, wgrad) <= 1.0))
    else:
        raise AssertionError(f"a primitive call of an unknown kind: {kind}")
    return res


@pytest.mark.parametrize("name", CASES)
def test_every_layer_call_of_the_walk_against_float64_on_the_devices_own_inputs(name):
    """Bounds (device figure / bound must be <= 1):
    convolution forward, grad_weight, grad_a (+ into, added in float64), grad_skip: error over the tensor's largest |value| <=
      unet_cases.BOUND_FACTOR x max(TorchBackend(float32)'s own error on the same call, 4 x 2^-23);
    BatchNorm y, running statistics, grad_x, grad_gamma, grad_beta, the loss and grad_logits: one float32 ulp of the tensor's largest
      magnitude from the float64 rule (the backward's mask from the device's saved y); stats rtol 1e-12; grad_residual and the
      max-pool's forward equal in bits;
    max-pool backward: per cell 2.5 x spacing(float32(S)), S = the float64 backward of |grad_out| plus |into|: at most five float32
      roundings of partial sums no larger than S."""
    calls = _device_walk(name)[3]
    ref64, ref32 = TorchBackend(torch.float64), TorchBackend(torch.float32)
    counts, worst, failed = {}, {}, []
    for kind, key, inputs, out in calls:
        counts[kind] = counts.get(kind, 0) + 1
        if kind == "bias_grad":                             # the walk's own float64 sum, held in (a)
            continue
        for what, ratio, ok in _check_call(kind, inputs, out, ref64, ref32):
            if not ratio <= worst.get(what, (-1.0, None))[0]:
                worst[what] = (ratio, key)
            if not ok:
                failed.append((what, key, ratio))
    print(f"\n{name}: worst device figure over its bound, per kind of call\n" + "\n".join(f"  {what:20s} {r:9.3f}  {key}" for what, (r, key) in worst.items()))
    assert counts == {"conv": 31, "batchnorm": 30, "maxpool": 1, "cross_entropy": 1, "bias_grad": 1, "batchnorm_backward": 30, "conv_backward": 31,
                      "maxpool_backward": 1}, counts
    assert not failed, failed
