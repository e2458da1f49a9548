"""One training step of the U-Net terrain classifier recomposed from single layers ("Checks"): the training-mode
forward, the mean cross-entropy and the backward of tests/unet_spec.Unet as a walk over primitive calls of a backend, written
against that module tree and smp's state-dict keys.  It is the independent statement of the graph -- nothing here is derived from
csrc/unet_graph.h or benchnav_amd.unet.conv_table.

    loss, grads, stats = walk(backend, state_dict, colors, targets, observe=None)

grads: {state-dict key: gradient} of every parameter, inserted in the backward's order (per node: BatchNorm's weight and bias, then
the convolution's weight; the head's weight, then its bias), so the first differing key names the node.  stats: {key: updated
running mean / variance}.  observe(kind, key, inputs, outputs) sees every primitive call: `kind` is the backend method's name,
`key` the layer's weight key ("encoder.maxpool", "loss" where there is none), `inputs` the keyword arguments, `outputs` what the
call returned -- getattr(other_backend, kind)(**inputs) replays the call elsewhere.

The backward is the forward's order reversed, with a layer's downsample standing BEFORE block 0's conv1 in the forward.  A gradient
slot's first writer stores, later writers add through into_a / into_skip / into.  So an encoder feature's gradient receives the
decoder's skip gradient first, then block 0's conv1, then the downsample; the stem's output the decoder's skip, then the pool.

Two backends: TorchBackend(dtype) on the CPU, and DeviceBackend -- unet.conv2d, unet.maxpool and unet_train's single-layer
functions on device tensors, without a tensor leaving the device inside the walk.  Not a test module."""
import math

import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
ENCODER_WIDTHS = (64, 128, 256, 512)


class _Slot:
    """An activation of the graph and the gradient that accumulates for it (None until its first writer)."""

    def __init__(self, value, is_input=False):
        self.value, self.grad, self.is_input = value, None, is_input


def walk(backend, state_dict, colors, targets, observe=None):
    be = backend
    P = {k: be.tensor(v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
    targets = be.tensor(targets)
    tape, grads, stats = [], {}, {}

    def call(kind, key, **inputs):
        out = getattr(be, kind)(**inputs)
        if observe is not None:
            observe(kind, key, inputs, out)
        return out

    # ---- forward: every node goes on the tape ----
    def conv(conv, bn, a, stride, pad, relu, skip=None, upsample=False, residual=None):
        """relu?(bn(conv(up2x?(a) ++ skip)) + residual); the head (bn None) is the convolution with its bias."""
        wkey = conv + ".weight"
        c = call("conv", wkey, a=a.value, w=P[wkey], bias=None if bn else P[conv + ".bias"], stride=stride, pad=pad,
                 skip=None if skip is None else skip.value, upsample=upsample)
        node = dict(kind="conv", conv=conv, bn=bn, a=a, skip=skip, upsample=upsample, residual=residual, relu=relu, stride=stride, pad=pad, c=c)
        if bn is None:
            node["out"] = _Slot(c)
        else:
            y, node["stats"], rm, rv = call("batchnorm", bn + ".weight", x=c, gamma=P[bn + ".weight"], beta=P[bn + ".bias"],
                                            residual=None if residual is None else residual.value, relu=relu,
                                            running_mean=P[bn + ".running_mean"], running_var=P[bn + ".running_var"])
            stats[bn + ".running_mean"], stats[bn + ".running_var"] = rm, rv
            node["out"] = _Slot(y)
        tape.append(node)
        return node["out"]

    x = _Slot(be.tensor(colors), is_input=True)                # the colours need no gradient
    f1 = conv("encoder.conv1", "encoder.bn1", x, 2, 3, True)
    y = _Slot(call("maxpool", "encoder.maxpool", x=f1.value))
    tape.append(dict(kind="maxpool", a=f1, out=y))
    features, cin = [f1], 64
    for l, width in enumerate(ENCODER_WIDTHS):
        for b in range(2):
            p = f"encoder.layer{l + 1}.{b}"
            stride = 2 if (b == 0 and l > 0) else 1
            identity = y
            if b == 0 and (stride != 1 or cin != width):        # unet_spec.BasicBlock's condition; it stands before conv1
                identity = conv(p + ".downsample.0", p + ".downsample.1", y, stride, 0, False)
            t = conv(p + ".conv1", p + ".bn1", y, stride, 1, True)
            y = conv(p + ".conv2", p + ".bn2", t, 1, 1, True, residual=identity)
            cin = width
        features.append(y)
    for b, skip in enumerate((features[3], features[2], features[1], features[0], None)):
        p = f"decoder.blocks.{b}"
        y = conv(p + ".conv1.0", p + ".conv1.1", y, 1, 1, True, skip=skip, upsample=True)
        y = conv(p + ".conv2.0", p + ".conv2.1", y, 1, 1, True)
    logits = conv("segmentation_head.0", None, y, 1, 1, False)
    loss, logits.grad = call("cross_entropy", "loss", logits=logits.value, targets=targets)

    # ---- backward: the tape reversed ----
    for node in reversed(tape):
        out = node["out"]
        assert out.grad is not None, "a node's output has no gradient when the backward reaches it"
        if node["kind"] == "maxpool":
            a = node["a"]
            a.grad = call("maxpool_backward", "encoder.maxpool", x=a.value, grad_out=out.grad, into=a.grad)
            continue
        conv_key, bn, a, skip, residual = node["conv"], node["bn"], node["a"], node["skip"], node["residual"]
        g = out.grad
        if bn is not None:
            g, gres, grads[bn + ".weight"], grads[bn + ".bias"] = call(
                "batchnorm_backward", bn + ".weight", grad_out=g, y=out.value, x=node["c"], stats=node["stats"], gamma=P[bn + ".weight"],
                relu=node["relu"], residual=residual is not None)
            if residual is not None:
                assert residual.grad is None, f"{bn}: BatchNorm's residual gradient must be its slot's first writer"
                residual.grad = gres
        need = ("weight",) + (() if a.is_input else ("a",)) + (("skip",) if skip is not None else ())
        if skip is not None:                                    # the split writes both halves one way: both stored or both added
            assert (a.grad is None) == (skip.grad is None), f"{conv_key}: a one-sided `into` would add +0 to the other half"
        gw, ga, gs = call("conv_backward", conv_key + ".weight", a=a.value, w=P[conv_key + ".weight"], grad_out=g, stride=node["stride"], pad=node["pad"],
                          skip=None if skip is None else skip.value, upsample=node["upsample"], need=need, into_a=a.grad,
                          into_skip=None if skip is None else skip.grad)
        grads[conv_key + ".weight"] = gw
        if "a" in need:
            a.grad = ga
        if skip is not None:
            skip.grad = gs
        if bn is None:
            # the head's bias has no single-layer entry point: the per-channel sum in float64, rounded once
            total = g.double().sum(dim=(0, 2, 3))
            if observe is not None:
                observe("bias_grad", conv_key + ".bias", dict(grad_out=g), total)
            grads[conv_key + ".bias"] = total.to(g.dtype)
    return float(loss), grads, stats


class TorchBackend:
    """Every primitive by plain torch on the CPU in `dtype`.  Tensor arguments may come from anywhere (the device's float32, a
    float64 stats pair): each call takes them to the CPU and to `dtype` first, so a recorded device call replays as it is."""

    def __init__(self, dtype=torch.float64):
        self.dtype = dtype

    def tensor(self, t):
        if t is None:
            return None
        t = torch.as_tensor(t).detach().cpu()
        return t.to(self.dtype) if t.is_floating_point() else t

    def conv(self, a, w, bias, stride, pad, skip, upsample):
        a, w, bias, skip = map(self.tensor, (a, w, bias, skip))
        x = F.interpolate(a, scale_factor=2, mode="nearest") if upsample else a
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        return F.conv2d(x, w, bias, stride, pad)

    def conv_backward(self, a, w, grad_out, stride, pad, skip, upsample, need, into_a, into_skip):
        """torch.autograd.grad of this one F.conv2d (behind its upsample and concatenation), `into` added behind it."""
        a, w, grad_out, skip, into_a, into_skip = map(self.tensor, (a, w, grad_out, skip, into_a, into_skip))
        leaves = {"weight": w.requires_grad_()}
        if "a" in need:
            leaves["a"] = a.requires_grad_()
        if "skip" in need and skip is not None:
            leaves["skip"] = skip.requires_grad_()
        x = F.interpolate(a, scale_factor=2, mode="nearest") if upsample else a
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        got = dict(zip(leaves, torch.autograd.grad(F.conv2d(x, w, None, stride, pad), list(leaves.values()), grad_out)))
        ga, gs = got.get("a"), got.get("skip")
        if ga is not None and into_a is not None:
            ga = ga + into_a
        if gs is not None and into_skip is not None:
            gs = gs + into_skip
        return (got["weight"] if "weight" in need else None), ga, gs

    def batchnorm(self, x, gamma, beta, residual, relu, running_mean, running_var):
        """(y, stats = (mean, 1 / sqrt(biased variance + eps)), running mean, running variance: momentum 0.1, unbiased variance)"""
        x, gamma, beta, residual, running_mean, running_var = map(self.tensor, (x, gamma, beta, residual, running_mean, running_var))
        n = x.numel() // x.shape[1]
        mean, var = x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + BN_EPS)
        y = (x - mean.view(1, -1, 1, 1)) * (invstd * gamma).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        if residual is not None:
            y = y + residual
        if relu:
            y = y.clamp_min(0.0)
        rm = None if running_mean is None else (1.0 - BN_MOMENTUM) * running_mean + BN_MOMENTUM * mean
        rv = None if running_var is None else (1.0 - BN_MOMENTUM) * running_var + BN_MOMENTUM * var * n / (n - 1)
        return y, torch.stack([mean, invstd]), rm, rv

    def batchnorm_backward(self, grad_out, y, x, stats, gamma, relu, residual):
        """The closed formula; the ReLU's mask comes from the given y (y > 0).  (grad_x, grad_residual or None, grad_gamma, grad_beta)"""
        grad_out, y, x, stats, gamma = map(self.tensor, (grad_out, y, x, stats, gamma))
        n = x.numel() // x.shape[1]
        g = torch.where(y > 0, grad_out, torch.zeros_like(grad_out)) if relu else grad_out
        mean, invstd = stats[0].view(1, -1, 1, 1), stats[1].view(1, -1, 1, 1)
        xhat = (x - mean) * invstd
        sum_g, sum_gx = g.sum(dim=(0, 2, 3)), (g * xhat).sum(dim=(0, 2, 3))
        gx = gamma.view(1, -1, 1, 1) * invstd * (g - sum_g.view(1, -1, 1, 1) / n - xhat * (sum_gx.view(1, -1, 1, 1) / n))
        return gx, (g if residual else None), sum_gx, sum_g

    def maxpool(self, x):
        return F.max_pool2d(self.tensor(x), 3, 2, 1)

    def maxpool_backward(self, x, grad_out, into):
        x, grad_out, into = self.tensor(x).requires_grad_(), self.tensor(grad_out), self.tensor(into)
        g, = torch.autograd.grad(F.max_pool2d(x, 3, 2, 1), x, grad_out)
        return g if into is None else g + into

    def cross_entropy(self, logits, targets):
        logits = self.tensor(logits).requires_grad_()
        loss = F.cross_entropy(logits, self.tensor(targets))
        grad, = torch.autograd.grad(loss, logits)
        return loss.detach(), grad

    def adam(self, p, g, m, v, step, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
        """torch.optim.Adam's step number `step` (from 1): (p, m, v) after it."""
        p, g, m, v = map(self.tensor, (p, g, m, v))
        b1, b2 = betas
        g = g + weight_decay * p
        m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        return p - (lr / (1 - b1 ** step)) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps), m, v


class DeviceBackend:
    """Every primitive by the device's own single-layer functions: they call the helpers the training step calls."""

    dtype = torch.float32

    def __init__(self, device=None):
        from benchnav_amd import unet, unet_train
        from benchnav_amd._device import resolve_device
        self.unet, self.train, self.device = unet, unet_train, resolve_device(device, "unet_train")

    def tensor(self, t):
        if t is None:
            return None
        t = torch.as_tensor(t).detach()
        return t.to(self.device, torch.float32 if t.is_floating_point() else t.dtype).contiguous()

    def conv(self, a, w, bias, stride, pad, skip, upsample):
        return self.unet.conv2d(a, w, bias, stride, pad, skip=skip, upsample=upsample, device=self.device)

    def conv_backward(self, a, w, grad_out, stride, pad, skip, upsample, need, into_a, into_skip):
        return self.train.conv2d_backward(a, w, grad_out, stride, pad, skip=skip, upsample=upsample, need=need, into_a=into_a, into_skip=into_skip,
                                          device=self.device)

    def batchnorm(self, x, gamma, beta, residual, relu, running_mean, running_var):
        return self.train.batchnorm_forward(x, gamma, beta, residual, relu, running_mean, running_var, device=self.device)

    def batchnorm_backward(self, grad_out, y, x, stats, gamma, relu, residual):
        return self.train.batchnorm_backward(grad_out, y, x, stats, gamma, relu, residual=residual, device=self.device)

    def maxpool(self, x):
        return self.unet.maxpool(x, device=self.device)

    def maxpool_backward(self, x, grad_out, into):
        return self.train.maxpool_backward(x, grad_out, into=into, device=self.device)

    def cross_entropy(self, logits, targets):
        return self.train.cross_entropy(logits, targets, device=self.device)

    def adam(self, p, g, m, v, step, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
        return self.train.adam(p, g, m, v, step, lr, weight_decay, betas, eps, device=self.device)
