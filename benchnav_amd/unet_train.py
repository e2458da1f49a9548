"""Training the U-Net terrain classifier on the GPU: the reference's trainers/classifier_trainer.py:ClassifierTrainer (Adam on the
cross-entropy of Unet(resnet18, classes) in training mode, a validation pass per epoch, best_model.pth when the validation loss
improves).  DESIGN.md 4.12, csrc/segtrain_kernels.hip.  Hand-written HIP throughout: no autograd and no torch convolution.

    sd = init_state_dict(classes=10, seed=0)                   # or a state dict of your own (smp's keys)
    net = TrainableTerrainClassifier(sd, classes=10)
    loss = net.train_step(colors, targets, lr=1e-3)            # (B, 3, H, W) colours, (B, H, W) integer class maps
    trainer = ClassifierTrainer(net, directory, params, train_dataset, valid_dataset)
    trainer.train()                                            # writes <directory>/bs..._lr..._wd..._epochs.../models/best_model.pth
    clf = load_terrain_classifier(".../best_model.pth")       # unet.py reads it back
"""
from __future__ import annotations

import ctypes as C
import json
import os
from datetime import datetime
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _capi
from ._device import Handle, check, resolve_device, stream_ptr
from .unet import TerrainClassifier, _check_classes, _ptr, conv_table

BN_KEYS = ("weight", "bias", "running_mean", "running_var")
READ_PARAMETERS, READ_GRADIENTS, READ_M, READ_V = 0, 1, 2, 3


def param_layout(classes: int) -> List[Tuple[str, Tuple[int, ...], bool]]:
    """The packed unfolded parameters (include/benchnav_mppi.h) as (state-dict key, shape, trainable) in order: per convolution
    of unet.conv_table its weight, then its BatchNorm's weight, bias, running_mean, running_var; the head has its bias."""
    out = []
    for wkey, bn, shape, _, _ in conv_table(classes):
        out.append((wkey, tuple(shape), True))
        if bn is None:
            out.append((wkey[:-len("weight")] + "bias", (shape[0],), True))
        else:
            out.extend((f"{bn}.{k}", (shape[0],), k in ("weight", "bias")) for k in BN_KEYS)
    return out


def param_count(classes: int) -> int:
    """bn_segtrain_param_count(classes) without the library."""
    return sum(int(np.prod(shape)) for _, shape, _ in param_layout(classes))


def pack_state_dict(state_dict, classes: int = 10) -> np.ndarray:
    """The packed float32 parameters of bn_segtrain_create from a Unet(resnet18, classes).state_dict().  Strict like
    unet.fold_state_dict: a missing key, an unexpected key (other than BatchNorm's num_batches_tracked), a wrong shape or a value
    that is not finite raises ValueError and names the key.  Pure host code; float32 values pass through bit for bit."""
    classes = _check_classes(classes)
    parts, used = [], set()
    for key, shape, _ in param_layout(classes):
        if key not in state_dict:
            raise ValueError(f"the state dict has no key {key!r}")
        v = state_dict[key]
        v = v.detach().cpu().to(torch.float32).numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float32)
        if tuple(v.shape) != shape:
            raise ValueError(f"{key!r} has shape {tuple(v.shape)}, expected {shape}")
        if not np.isfinite(v).all():
            raise ValueError(f"{key!r} holds a value that is not finite")
        used.add(key)
        parts.append(v.reshape(-1))
    for key in state_dict:
        if key not in used and not key.endswith("num_batches_tracked"):
            raise ValueError(f"the state dict has an unexpected key {key!r}")
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def unpack_params(packed, classes: int = 10, num_batches_tracked: int = 0, trainable_only: bool = False) -> Dict[str, torch.Tensor]:
    """pack_state_dict's inverse: smp's state dict (float32 CPU tensors, every BatchNorm's num_batches_tracked as int64) from the
    packed parameters.  trainable_only leaves the running statistics and num_batches_tracked out (the layout of a gradient)."""
    classes = _check_classes(classes)
    packed = np.asarray(packed, dtype=np.float32).reshape(-1)
    if packed.size != param_count(classes):
        raise ValueError(f"expected {param_count(classes)} packed parameters for {classes} classes, got {packed.size}")
    out, at = {}, 0
    for key, shape, trainable in param_layout(classes):
        n = int(np.prod(shape))
        if trainable or not trainable_only:
            out[key] = torch.from_numpy(packed[at:at + n].reshape(shape).copy())
        if key.endswith("running_var") and not trainable_only:
            out[key[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(int(num_batches_tracked), dtype=torch.int64)
        at += n
    return out


def init_state_dict(classes: int = 10, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A start without a checkpoint: torch's default initialisations per shape (Conv2d: kaiming-uniform with a = sqrt(5), i.e.
    U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias; BatchNorm: weight 1, bias 0, running mean 0, running variance 1) drawn
    from a generator seeded with `seed`.  It is NOT segmentation_models_pytorch's start: the reference begins from the ImageNet
    encoder weights, which are not shipped here -- pass your own state dict if you have them."""
    classes = _check_classes(classes)
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for wkey, bn, shape, _, _ in conv_table(classes):
        bound = 1.0 / float(np.sqrt(shape[1] * shape[2] * shape[3]))
        out[wkey] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound
        if bn is None:
            out[wkey[:-len("weight")] + "bias"] = (torch.rand(shape[0], generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound
        else:
            out[f"{bn}.weight"], out[f"{bn}.bias"] = torch.ones(shape[0]), torch.zeros(shape[0])
            out[f"{bn}.running_mean"], out[f"{bn}.running_var"] = torch.zeros(shape[0]), torch.ones(shape[0])
            out[f"{bn}.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return out


def _raise(lib, code: int) -> None:
    if code == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_segtrain_last_error().decode("utf-8", "replace"))
    check(lib, "segtrain", code)


def _check_targets(targets, shape, classes: int, dev) -> torch.Tensor:
    """(B, H, W) integers in [0, classes) as int64 on the device.  Checked before any launch: on the host for a host tensor; a
    device tensor costs one synchronisation."""
    t = torch.as_tensor(targets)
    if t.is_floating_point() or t.dtype == torch.bool or tuple(t.shape) != tuple(shape):
        raise ValueError(f"targets must be integers of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= classes):
        raise ValueError(f"every target must be in [0, {classes})")
    return t.detach().to(dev, torch.int64).contiguous()


class TrainableTerrainClassifier(Handle):
    """smp.Unet(encoder_name="resnet18", classes=C) in training mode on the device with its gradients and Adam's state.
    state_dict: the model's state dict (tensors or arrays, smp's keys).  Colours are (B, 3, H, W) in [0, 1] with H and W multiples
    of 32 and B (H / 32) (W / 32) > 1 (BatchNorm needs more than one value per channel); targets are (B, H, W) integers in
    [0, classes).  Calls are enqueued on torch's current stream.  ValueError for invalid inputs, RuntimeError without a GPU."""

    family = "segtrain"

    def __init__(self, state_dict, classes: int = 10, device=None) -> None:
        self._handle = None
        self.classes = _check_classes(classes)
        params = pack_state_dict(state_dict, self.classes)
        tracked = [int(v) for k, v in state_dict.items() if k.endswith("num_batches_tracked")]
        self._tracked0 = tracked[0] if tracked else 0
        self._dev = resolve_device(device, "unet_train")
        self._lib = _capi.load()
        self._count = params.size
        h = C.c_void_p()
        _raise(self._lib, self._lib.bn_segtrain_create(self._dev.index, self.classes, params.ctypes.data, params.size, C.byref(h)))
        self._handle = h

    def _inputs(self, colors, targets) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._handle is None:
            raise RuntimeError("the classifier is closed")
        x = torch.as_tensor(colors)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected colours of shape (B, 3, H, W), got {tuple(x.shape)}")
        B, _, H, W = x.shape
        if H % 32 or W % 32:
            raise ValueError(f"height and width must be multiples of 32 (five 2x stages), got {H} x {W}")
        if B >= 1 and B * (H // 32) * (W // 32) <= 1:
            raise ValueError("training needs more than 1 value per channel at the bottleneck: B (H / 32) (W / 32) > 1")
        if B < 1 or self._lib.bn_segtrain_workspace_bytes(B, H, W) == 0:
            raise ValueError(f"{B} maps of {H} x {W} are out of the library's range")
        t = _check_targets(targets, (B, H, W), self.classes, self._dev)
        return x.detach().to(self._dev, torch.float32).contiguous(), t

    def _read(self, what: int) -> np.ndarray:
        if self._handle is None:
            raise RuntimeError("the classifier is closed")
        out = np.empty(self._count, np.float32)
        _raise(self._lib, self._lib.bn_segtrain_read(self._handle, what, out.ctypes.data, out.size))
        return out

    @property
    def steps(self) -> int:
        return int(self._lib.bn_segtrain_steps(self._handle)) if self._handle else 0

    def gradients(self, colors, targets) -> Tuple[float, Dict[str, torch.Tensor]]:
        """(loss, {state-dict key: gradient}) of the mean cross-entropy in training mode; nothing in the handle's state changes."""
        x, t = self._inputs(colors, targets)
        B, _, H, W = x.shape
        with torch.cuda.device(self._dev):
            loss = torch.empty(1, device=self._dev, dtype=torch.float32)
            nbytes = self._lib.bn_segtrain_workspace_bytes(B, H, W)
            work = torch.empty(nbytes, device=self._dev, dtype=torch.uint8)
            _raise(self._lib, self._lib.bn_segtrain_grad_async(self._handle, stream_ptr(self._dev), B, H, W, _ptr(x), _ptr(t), _ptr(loss), _ptr(work), nbytes))
            torch.cuda.current_stream(self._dev).synchronize()
        return float(loss.item()), unpack_params(self._read(READ_GRADIENTS), self.classes, trainable_only=True)

    def train_step_async(self, colors, targets, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                         loss_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One Adam step enqueued on the current stream; the loss lands in loss_out (a one-element float32 device view) without
        a host round trip."""
        x, t = self._inputs(colors, targets)
        B, _, H, W = x.shape
        with torch.cuda.device(self._dev):
            if loss_out is None:
                loss_out = torch.empty(1, device=self._dev, dtype=torch.float32)
            nbytes = self._lib.bn_segtrain_workspace_bytes(B, H, W)
            work = torch.empty(nbytes, device=self._dev, dtype=torch.uint8)
            _raise(self._lib, self._lib.bn_segtrain_step_async(self._handle, stream_ptr(self._dev), B, H, W, _ptr(x), _ptr(t), float(lr), float(betas[0]),
                                                               float(betas[1]), float(eps), float(weight_decay), _ptr(loss_out), _ptr(work), nbytes))
        return loss_out

    def train_step(self, colors, targets, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8) -> float:
        """One step of torch.optim.Adam(lr, betas, eps, weight_decay) on this batch; returns the loss before the step."""
        return float(self.train_step_async(colors, targets, lr, weight_decay, betas, eps).item())

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """smp's state dict of the current parameters: float32 CPU tensors, num_batches_tracked as int64."""
        return unpack_params(self._read(READ_PARAMETERS), self.classes, self._tracked0 + self.steps)

    def adam_state(self) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        """Adam's (exp_avg, exp_avg_sq) by state-dict key."""
        return (unpack_params(self._read(READ_M), self.classes, trainable_only=True), unpack_params(self._read(READ_V), self.classes, trainable_only=True))

    def classifier(self) -> TerrainClassifier:
        """The eval-mode TerrainClassifier of the current state (BatchNorm folded with the running statistics)."""
        return TerrainClassifier(self.state_dict(), classes=self.classes, device=self._dev)


# ---- single layers, for the layer-level tests ----
def _f32(t, dev):
    return None if t is None else torch.as_tensor(t).detach().to(dev, torch.float32).contiguous()


def conv2d_backward(a, weight, grad_out, stride: int = 1, padding: int = 0, skip=None, upsample: bool = False, need=("weight", "a", "skip"),
                    into_a=None, into_skip=None, device=None):
    """bn_segtrain_conv2d_backward_async: the gradients of unet.conv2d(a, weight, None, stride, padding, skip, upsample) given
    grad_out, as (grad_weight, grad_a, grad_skip) with None for what `need` leaves out.  into_a / into_skip: tensors the data
    gradients are ADDED to (copies are returned)."""
    dev = resolve_device(device, "unet_train")
    lib = _capi.load()
    a, weight, grad_out, skip = _f32(a, dev), _f32(weight, dev), _f32(grad_out, dev), _f32(skip, dev)
    if a.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3] or grad_out.dim() != 4:
        raise ValueError("a and grad_out must be (B, C, h, w) and weight (Cout, Cin, k, k)")
    B, ca, h, w = a.shape
    hin, win = (2 * h, 2 * w) if upsample else (h, w)
    cb = 0 if skip is None else skip.shape[1]
    if skip is not None and tuple(skip.shape) != (B, cb, hin, win):
        raise ValueError(f"skip must be {(B, cb, hin, win)}, got {tuple(skip.shape)}")
    cout, cin, k, _ = weight.shape
    if cin != ca + cb:
        raise ValueError(f"weight takes {cin} input channels, the input has {ca + cb}")
    if hin + 2 * padding < k or win + 2 * padding < k:
        raise ValueError("the kernel does not fit the padded input")
    ho, wo = (hin + 2 * padding - k) // stride + 1, (win + 2 * padding - k) // stride + 1
    if tuple(grad_out.shape) != (B, cout, ho, wo):
        raise ValueError(f"grad_out must be {(B, cout, ho, wo)}, got {tuple(grad_out.shape)}")
    nbytes = lib.bn_segtrain_conv2d_backward_workspace_bytes(B, cin, hin, win, cout, k, int(stride), int(padding))
    if nbytes == 0:
        raise ValueError("shape out of the library's range (channels in [1, 4096], kernel 1, 3 or 7, stride 1 or 2, pad <= min(3, k - 1))")
    accumulate = into_a is not None or into_skip is not None
    with torch.cuda.device(dev):
        gw = torch.empty_like(weight) if "weight" in need else None
        ga = gs = None
        if "a" in need:
            ga = _f32(into_a, dev).clone() if into_a is not None else (torch.zeros_like(a) if accumulate else torch.empty_like(a))
        if "skip" in need and skip is not None:
            gs = _f32(into_skip, dev).clone() if into_skip is not None else (torch.zeros_like(skip) if accumulate else torch.empty_like(skip))
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        _raise(lib, lib.bn_segtrain_conv2d_backward_async(dev.index, stream_ptr(dev), _ptr(a), ca, _ptr(skip), cb, int(bool(upsample)), B, hin, win,
                                                          _ptr(weight), cout, k, int(stride), int(padding), _ptr(grad_out), _ptr(gw), _ptr(ga), _ptr(gs),
                                                          int(accumulate), _ptr(work), nbytes))
    return gw, ga, gs


def batchnorm_forward(x, gamma, beta, residual=None, relu: bool = False, running_mean=None, running_var=None, device=None):
    """bn_segtrain_batchnorm_forward_async on (B, C, h, w): (y, stats, running_mean, running_var); stats is the float64 (2, C) of batch
    mean and 1 / sqrt(var + eps) the backward takes; the running statistics are updated copies (None if not given)."""
    dev = resolve_device(device, "unet_train")
    lib = _capi.load()
    x, gamma, beta, residual = _f32(x, dev), _f32(gamma, dev), _f32(beta, dev), _f32(residual, dev)
    if x.dim() != 4 or tuple(gamma.shape) != (x.shape[1],) or tuple(beta.shape) != (x.shape[1],):
        raise ValueError("x must be (B, C, h, w), gamma and beta (C,)")
    if residual is not None and residual.shape != x.shape:
        raise ValueError("residual must have x's shape")
    B, ch, h, w = x.shape
    rm = _f32(running_mean, dev).clone() if running_mean is not None else None
    rv = _f32(running_var, dev).clone() if running_var is not None else None
    with torch.cuda.device(dev):
        y = torch.empty_like(x)
        stats = torch.empty(2, ch, device=dev, dtype=torch.float64)
        _raise(lib, lib.bn_segtrain_batchnorm_forward_async(dev.index, stream_ptr(dev), _ptr(x), B, ch, h * w, _ptr(gamma), _ptr(beta), _ptr(residual),
                                                            int(bool(relu)), _ptr(rm), _ptr(rv), _ptr(y), _ptr(stats)))
    return y, stats, rm, rv


def batchnorm_backward(grad_out, y, x, stats, gamma, relu: bool = False, residual: bool = False, device=None):
    """bn_segtrain_batchnorm_backward_async: (grad_x, grad_residual or None, grad_gamma, grad_beta) from batchnorm_forward's x, y, stats."""
    dev = resolve_device(device, "unet_train")
    lib = _capi.load()
    grad_out, y, x, gamma = _f32(grad_out, dev), _f32(y, dev), _f32(x, dev), _f32(gamma, dev)
    stats = torch.as_tensor(stats).detach().to(dev, torch.float64).contiguous()
    if x.dim() != 4 or grad_out.shape != x.shape or y.shape != x.shape or tuple(stats.shape) != (2, x.shape[1]) or tuple(gamma.shape) != (x.shape[1],):
        raise ValueError("grad_out, y and x must be one (B, C, h, w), stats (2, C), gamma (C,)")
    B, ch, h, w = x.shape
    with torch.cuda.device(dev):
        gx = torch.empty_like(x)
        gr = torch.empty_like(x) if residual else None
        gg, gb = torch.empty_like(gamma), torch.empty_like(gamma)
        sums = torch.empty(2, ch, device=dev, dtype=torch.float64)
        _raise(lib, lib.bn_segtrain_batchnorm_backward_async(dev.index, stream_ptr(dev), _ptr(grad_out), _ptr(y), _ptr(x), _ptr(stats), _ptr(gamma),
                                                             int(bool(relu)), B, ch, h * w, _ptr(gx), _ptr(gr), _ptr(gg), _ptr(gb), _ptr(sums)))
    return gx, gr, gg, gb


def maxpool_backward(x, grad_out, into=None, device=None) -> torch.Tensor:
    """bn_segtrain_maxpool_backward_async: the gradient of unet.maxpool(x) given grad_out; added to `into` (a copy) if given."""
    dev = resolve_device(device, "unet_train")
    lib = _capi.load()
    x, grad_out = _f32(x, dev), _f32(grad_out, dev)
    if x.dim() != 4 or x.numel() == 0 or tuple(grad_out.shape) != (x.shape[0], x.shape[1], (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1):
        raise ValueError("x must be a non-empty (B, C, h, w) and grad_out the pooled shape")
    B, ch, h, w = x.shape
    with torch.cuda.device(dev):
        gx = _f32(into, dev).clone() if into is not None else torch.empty_like(x)
        _raise(lib, lib.bn_segtrain_maxpool_backward_async(dev.index, stream_ptr(dev), _ptr(x), _ptr(grad_out), B * ch, h, w, _ptr(gx), int(into is not None)))
    return gx


def cross_entropy(logits, targets, need_grad: bool = True, loss_out: Optional[torch.Tensor] = None, device=None):
    """bn_segtrain_cross_entropy_async: (loss as a one-element device tensor, grad_logits or None) of F.cross_entropy(logits (B, C, H, W),
    targets (B, H, W))."""
    dev = resolve_device(device, "unet_train")
    lib = _capi.load()
    logits = _f32(logits, dev)
    if logits.dim() != 4 or logits.numel() == 0:
        raise ValueError("logits must be a non-empty (B, C, H, W)")
    B, nc, H, W = logits.shape
    t = _check_targets(targets, (B, H, W), nc, dev)
    with torch.cuda.device(dev):
        loss = loss_out if loss_out is not None else torch.empty(1, device=dev, dtype=torch.float32)
        grad = torch.empty_like(logits) if need_grad else None
        work = torch.empty(B * H * W, device=dev, dtype=torch.float64)
        _raise(lib, lib.bn_segtrain_cross_entropy_async(dev.index, stream_ptr(dev), _ptr(logits), _ptr(t), B, nc, H * W, _ptr(loss), _ptr(grad), _ptr(work),
                                                        work.numel() * 8))
    return loss, grad


def adam(p, g, m, v, step: int, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, device=None):
    """bn_segtrain_adam_async on copies: (p, m, v) after step number `step` (from 1) of torch.optim.Adam."""
    dev = resolve_device(device, "unet_train")
    lib = _capi.load()
    p, g, m, v = _f32(p, dev).clone(), _f32(g, dev), _f32(m, dev).clone(), _f32(v, dev).clone()
    if not (p.shape == g.shape == m.shape == v.shape) or p.numel() == 0:
        raise ValueError("p, g, m and v must share one non-empty shape")
    with torch.cuda.device(dev):
        _raise(lib, lib.bn_segtrain_adam_async(dev.index, stream_ptr(dev), _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), int(step), float(lr), float(betas[0]),
                                               float(betas[1]), float(eps), float(weight_decay)))
    return p, m, v


class ClassifierTrainer:
    """The reference's ClassifierTrainer (trainers/classifier_trainer.py:22-165) around TrainableTerrainClassifier.  model: a
    TrainableTerrainClassifier or a state dict; params_model_training: any object with .batch_size, .learning_rate,
    .weight_decay and .num_epochs (and optionally .device, .classes); the datasets yield (colours (3, H, W), class map (H, W)).
    Batches come from torch.utils.data.DataLoader (shuffle=True for training), so the order under torch.manual_seed is the
    reference's.  best_model.pth (torch.save of the state dict) goes to <model_directory>/bs{bs:03d}_lr{lr:.0e}_wd{wd:.0e}_
    epochs{n:03d}/models/ when the epoch's mean validation loss improves -- every epoch without a validation set.  The
    validation loss is the eval-mode classifier's forward and the cross-entropy kernel.  The losses stay on the device during an
    epoch and are read once at its end; `history` keeps them and logs/<time>/history.json holds a copy (tensorboard is not
    used)."""

    def __init__(self, model, model_directory: str, params_model_training, train_dataset, valid_dataset=None) -> None:
        from torch.utils.data import DataLoader
        p = params_model_training
        if not isinstance(model, TrainableTerrainClassifier):
            model = TrainableTerrainClassifier(model, classes=getattr(p, "classes", 10), device=getattr(p, "device", None))
        self.model = model
        self.params_model_training = p
        self.train_dataset, self.valid_dataset = train_dataset, valid_dataset
        self.train_loader = DataLoader(train_dataset, batch_size=p.batch_size, shuffle=True)
        self.valid_loader = DataLoader(valid_dataset, batch_size=p.batch_size, shuffle=False) if valid_dataset is not None else None
        self.model_directory = os.path.join(model_directory, f"bs{p.batch_size:03d}_lr{p.learning_rate:.0e}_wd{p.weight_decay:.0e}_epochs{p.num_epochs:03d}")
        self.model_saving_path = os.path.join(self.model_directory, "models")
        self.log_saving_path = os.path.join(self.model_directory, "logs", datetime.now().strftime("%Y%m%d%H%M%S"))
        os.makedirs(self.model_saving_path, exist_ok=True)
        os.makedirs(self.log_saving_path, exist_ok=True)
        self.history = {"train_iteration": [], "train_epoch": [], "valid_epoch": []}

    def train(self) -> None:
        p, dev = self.params_model_training, self.model._dev
        best = float("inf")
        for epoch in range(p.num_epochs):
            losses = torch.zeros(len(self.train_loader), device=dev, dtype=torch.float32)
            for i, (x, y) in enumerate(self.train_loader):
                self.model.train_step_async(x, y, p.learning_rate, p.weight_decay, loss_out=losses[i:i + 1])
            valid = None
            if self.valid_loader is not None:
                clf = self.model.classifier()
                valid = torch.zeros(len(self.valid_loader), device=dev, dtype=torch.float32)
                for i, (x, y) in enumerate(self.valid_loader):
                    cross_entropy(clf.forward(x), y, need_grad=False, loss_out=valid[i:i + 1], device=dev)
                clf.close()
            train_losses = losses.cpu().tolist()                 # the epoch's one read
            self.history["train_iteration"].extend(train_losses)
            self.history["train_epoch"].append(sum(train_losses) / len(train_losses))
            if valid is not None:
                mean_valid = sum(valid.cpu().tolist()) / len(self.valid_loader)
                self.history["valid_epoch"].append(mean_valid)
                print(f"Epoch {epoch + 1}/{p.num_epochs}, Train Loss: {self.history['train_epoch'][-1]:.4f}, Valid Loss: {mean_valid:.4f}")
                if mean_valid < best:
                    best = mean_valid
                    self.save_model()
            else:
                print(f"Epoch {epoch + 1}/{p.num_epochs}, Train Loss: {self.history['train_epoch'][-1]:.4f}")
                self.save_model()
            with open(os.path.join(self.log_saving_path, "history.json"), "w") as f:
                json.dump(self.history, f)

    def save_model(self) -> None:
        torch.save(self.model.state_dict(), os.path.join(self.model_saving_path, "best_model.pth"))
        print(f"Model saved at {self.model_saving_path}")
