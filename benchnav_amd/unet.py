"""The U-Net terrain classifier on the GPU: the first half of TraversabilityPredictor.predict (reference
src/prediction_models/terrain_classifiers/unet.py: segmentation_models_pytorch's Unet(encoder_name="resnet18", classes=C) on raw
colours in [0, 1]; classifier_and_regressor.py:42-72 calls its `.predict`).  DESIGN.md 4.11, csrc/unet_kernels.hip.

Neither segmentation_models_pytorch nor torchvision is imported: the module tree (a ResNet-18 encoder without fc, five decoder
blocks of 2x nearest upsample + skip concatenation + two conv-BN-ReLU, a 3x3 head) is restated by hand, with smp's state-dict key
names as documented -- they have not been checked against a real checkpoint.  The network runs in eval mode only: every BatchNorm
is folded into its convolution on the host in float64 (`fold_state_dict`), the device sees 31 convolutions with a bias each.

    clf = TerrainClassifier(state_dict, classes=10)         # or load_terrain_classifier(path)
    classes = clf.predict(colors)                             # (B, 3, H, W) -> (B, H, W) int64, H and W multiples of 32
    predictor = TraversabilityPredictor(clf, regressors)      # colours + slopes -> slip mean / std without a host round trip
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _capi
from ._device import Handle, check, resolve_device, stream_ptr

MAX_CLASSES = 32
BN_EPS = 1e-5
_WIDTHS = (64, 128, 256, 512)
_DEC_IN, _DEC_SKIP, _DEC_OUT = (512, 256, 128, 64, 32), (256, 128, 64, 64, 0), (256, 128, 64, 32, 16)


def conv_table(classes: int) -> List[Tuple[str, Optional[str], Tuple[int, int, int, int], int, int]]:
    """The network's 31 convolutions in the order of the packed parameters (include/benchnav_mppi.h): (key of the conv weight,
    prefix of its BatchNorm's keys or None for the head, weight shape (cout, cin, k, k), stride, pad)."""
    t = [("encoder.conv1.weight", "encoder.bn1", (64, 3, 7, 7), 2, 3)]
    cin = 64
    for l, w in enumerate(_WIDTHS):
        p, s = f"encoder.layer{l + 1}", (2 if l else 1)
        t.append((f"{p}.0.conv1.weight", f"{p}.0.bn1", (w, cin, 3, 3), s, 1))
        t.append((f"{p}.0.conv2.weight", f"{p}.0.bn2", (w, w, 3, 3), 1, 1))
        if l:
            t.append((f"{p}.0.downsample.0.weight", f"{p}.0.downsample.1", (w, cin, 1, 1), 2, 0))
        t.append((f"{p}.1.conv1.weight", f"{p}.1.bn1", (w, w, 3, 3), 1, 1))
        t.append((f"{p}.1.conv2.weight", f"{p}.1.bn2", (w, w, 3, 3), 1, 1))
        cin = w
    for b in range(5):
        p = f"decoder.blocks.{b}"
        t.append((f"{p}.conv1.0.weight", f"{p}.conv1.1", (_DEC_OUT[b], _DEC_IN[b] + _DEC_SKIP[b], 3, 3), 1, 1))
        t.append((f"{p}.conv2.0.weight", f"{p}.conv2.1", (_DEC_OUT[b], _DEC_OUT[b], 3, 3), 1, 1))
    t.append(("segmentation_head.0.weight", None, (int(classes), 16, 3, 3), 1, 1))
    return t


def conv_inputs(classes: int, side: int) -> List[Tuple[int, int, bool]]:
    """Per convolution of conv_table, for maps of side x side: (side of its input, channels of the skip tensor concatenated behind
    it or 0, whether the input's first tensor is 2x-upsampled to that side) -- the graph of csrc/unet_graph.h seen from Python."""
    out, cur, block_in = [], int(side), int(side)
    for i, (key, _, shape, stride, pad) in enumerate(conv_table(classes)):
        first, up = key.endswith(".0.conv1.weight") and key.startswith("encoder.layer"), key.startswith("decoder") and ".conv1." in key
        if first:
            block_in = cur
        src = block_in if ".downsample." in key else 2 * cur if up else cur
        out.append((src, _DEC_SKIP[int(key.split(".")[2])] if up else 0, up))
        if ".downsample." not in key:
            cur = (src + 2 * pad - shape[2]) // stride + 1
        if i == 0:
            cur = (cur - 1) // 2 + 1                    # the max-pool behind the stem
    return out


def param_count(classes: int) -> int:
    """Floats of folded parameters: bn_unet_param_count(classes) without the library."""
    return sum(int(np.prod(shape)) + shape[0] for _, _, shape, _, _ in conv_table(classes))


def _check_classes(classes) -> int:
    c = int(classes)
    if c < 1 or c > MAX_CLASSES:
        raise ValueError(f"classes must be in [1, {MAX_CLASSES}], got {c}")
    return c


def fold_state_dict(state_dict, classes: int = 10, dtype=np.float32) -> np.ndarray:
    """The packed float32 parameters of bn_unet_create from a Unet(resnet18, classes).state_dict(): per convolution
    w * gamma / sqrt(var + eps) and beta - mean * gamma / sqrt(var + eps), evaluated in float64 and rounded once.

    Strict: a missing key, an unexpected key (other than BatchNorm's num_batches_tracked) or a wrong shape raises ValueError and
    names the key.  Pure host code.  dtype=np.float64 returns the fold before its rounding (the tests hold it to the BatchNorm
    form at float64's precision)."""
    classes = _check_classes(classes)
    used, parts = set(), []

    def get(key, shape):
        if key not in state_dict:
            raise ValueError(f"the state dict has no key {key!r}")
        v = state_dict[key]
        v = v.detach().cpu().to(torch.float64).numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)
        if tuple(v.shape) != tuple(shape):
            raise ValueError(f"{key!r} has shape {tuple(v.shape)}, expected {tuple(shape)}")
        if not np.isfinite(v).all():
            raise ValueError(f"{key!r} holds a value that is not finite")
        used.add(key)
        return v

    for wkey, bn, shape, _, _ in conv_table(classes):
        w = get(wkey, shape)
        cout = shape[0]
        if bn is None:
            b = get(wkey[:-len("weight")] + "bias", (cout,))
        else:
            gamma, beta = get(f"{bn}.weight", (cout,)), get(f"{bn}.bias", (cout,))
            mean, var = get(f"{bn}.running_mean", (cout,)), get(f"{bn}.running_var", (cout,))
            if (var + BN_EPS <= 0.0).any():
                raise ValueError(f"{bn}.running_var + eps must be > 0")
            scale = gamma / np.sqrt(var + BN_EPS)
            w = w * scale[:, None, None, None]
            b = beta - mean * scale
        parts.append(w.reshape(-1))
        parts.append(b)
    for key in state_dict:
        if key not in used and not key.endswith("num_batches_tracked"):
            raise ValueError(f"the state dict has an unexpected key {key!r}")
    with np.errstate(over="ignore"):
        out = np.concatenate(parts).astype(dtype)
    if not np.isfinite(out).all():
        raise ValueError("a folded parameter overflows float32")
    return np.ascontiguousarray(out)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class TerrainClassifier(Handle):
    """smp.Unet(encoder_name="resnet18", classes=C) in eval mode on the device.  state_dict: the model's state dict (tensors or
    arrays).  Inputs are (B, 3, H, W) colours in [0, 1] with H and W multiples of 32, on the host or the device; every call is
    enqueued on torch's current stream of the device without a synchronisation.  Raises ValueError for invalid inputs and
    RuntimeError without a GPU (no CPU fallback)."""

    family = "unet"
    batched = True                       # predict_classes takes a whole batch: TraversabilityPredictor classifies it in one call
    training = False

    def __init__(self, state_dict, classes: int = 10, device=None) -> None:
        self._handle = None
        self.classes = _check_classes(classes)
        params = fold_state_dict(state_dict, self.classes)
        self._dev = resolve_device(device, "unet")
        self._lib = _capi.load()
        h = C.c_void_p()
        self._check(self._lib.bn_unet_create(self._dev.index, self.classes, params.ctypes.data, params.size, C.byref(h)))
        self._handle = h

    # ---- the nn.Module surface the reference touches ----
    def to(self, device) -> "TerrainClassifier":
        if torch.device(device).type == "cuda" and torch.device(device).index in (None, self._dev.index):
            return self
        raise ValueError(f"this classifier lives on {self._dev}; create another one for {device}")

    def eval(self) -> "TerrainClassifier":
        return self

    # ---- the forward ----
    def _input(self, x) -> torch.Tensor:
        if self._handle is None:
            raise RuntimeError("the classifier is closed")
        x = torch.as_tensor(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected colours of shape (B, 3, H, W), got {tuple(x.shape)}")
        B, _, H, W = x.shape
        if H % 32 or W % 32:
            raise ValueError(f"height and width must be multiples of 32 (five 2x stages), got {H} x {W}")
        if B < 1 or self._lib.bn_unet_workspace_bytes(B, H, W) == 0:
            raise ValueError(f"{B} maps of {H} x {W} are out of the library's range")
        return x.detach().to(self._dev, torch.float32).contiguous()

    def _run(self, x, logits: bool, probabilities: bool, classes: bool):
        x = self._input(x)
        B, _, H, W = x.shape
        with torch.cuda.device(self._dev):
            lo = torch.empty(B, self.classes, H, W, device=self._dev, dtype=torch.float32) if logits else None
            pr = torch.empty(B, self.classes, H, W, device=self._dev, dtype=torch.float32) if probabilities else None
            cl = torch.empty(B, H, W, device=self._dev, dtype=torch.int32) if classes else None
            nbytes = self._lib.bn_unet_workspace_bytes(B, H, W)
            work = torch.empty(nbytes, device=self._dev, dtype=torch.uint8)       # torch's allocator keeps it alive for the stream
            self._check(self._lib.bn_unet_forward_async(self._handle, stream_ptr(self._dev), B, H, W, _ptr(x), _ptr(lo), _ptr(pr),
                                                              _ptr(cl), _ptr(work), nbytes))
        return lo, pr, cl, work

    def forward(self, x) -> torch.Tensor:
        """(B, C, H, W) float32 logits on the device."""
        return self._run(x, True, False, False)[0]

    __call__ = forward

    def predict_classes(self, x) -> torch.Tensor:
        """(B, H, W) int32 class maps on the device: the argmax of the logits, the lowest index on a tie."""
        return self._run(x, False, False, True)[2]

    def predict(self, x, return_probabilities: bool = False) -> torch.Tensor:
        """The reference's predict: softmax(logits, 1).argmax(1) as (B, H, W) int64, or the (B, C, H, W) float32 probabilities."""
        if return_probabilities:
            return self._run(x, False, True, False)[1]
        return self.predict_classes(x).to(torch.int64)

    def features(self, x) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        """(the five encoder features: after conv1 + bn1 + ReLU, layer1 ... layer4; the five decoder block outputs), copied out of
        one forward's workspace -- for localising a mismatch."""
        x = self._input(x)
        B, _, H, W = x.shape
        work = self._run(x, False, False, True)[3]
        out = []
        for i in range(10):
            off, ch, fh, fw = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32()
            self._check(self._lib.bn_unet_feature_layout(B, H, W, i, C.byref(off), C.byref(ch), C.byref(fh), C.byref(fw)))
            n = B * ch.value * fh.value * fw.value
            out.append(work[off.value:off.value + 4 * n].view(torch.float32).reshape(B, ch.value, fh.value, fw.value).clone())
        return out[:5], out[5:]

    # ---- single layers, for the layer-level tests ----
    def conv2d(self, a, weight, bias=None, stride: int = 1, padding: int = 0, skip=None, upsample: bool = False, residual=None,
               relu: bool = False) -> torch.Tensor:
        """The network's one fused convolution on caller tensors: relu?(conv2d(up2x?(a) ++ skip, weight) + bias + residual?)."""
        return conv2d(a, weight, bias, stride, padding, skip, upsample, residual, relu, device=self._dev)

    def maxpool(self, x) -> torch.Tensor:
        return maxpool(x, device=self._dev)


def conv2d(a, weight, bias=None, stride: int = 1, padding: int = 0, skip=None, upsample: bool = False, residual=None, relu: bool = False,
           device=None) -> torch.Tensor:
    """bn_unet_conv2d_async on torch's current stream: a (B, Ca, h, w) (half-size with upsample=True), skip (B, Cb, H, W) or None,
    weight (Cout, Ca + Cb, k, k) with k in {1, 3, 7}, bias (Cout) or None, residual of the output's shape or None."""
    dev = resolve_device(device, "unet")
    lib = _capi.load()
    f = lambda t: None if t is None else torch.as_tensor(t).detach().to(dev, torch.float32).contiguous()
    a, weight, bias, skip, residual = f(a), f(weight), f(bias), f(skip), f(residual)
    if a.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError("a must be (B, C, h, w) and weight (Cout, Cin, k, k)")
    B, ca, h, w = a.shape
    hin, win = (2 * h, 2 * w) if upsample else (h, w)
    cb = 0 if skip is None else skip.shape[1]
    if skip is not None and tuple(skip.shape) != (B, cb, hin, win):
        raise ValueError(f"skip must be {(B, cb, hin, win)}, got {tuple(skip.shape)}")
    cout, cin, k, _ = weight.shape
    if cin != ca + cb:
        raise ValueError(f"weight takes {cin} input channels, the input has {ca + cb}")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError("bias must be (Cout,)")
    if hin + 2 * padding < k or win + 2 * padding < k:
        raise ValueError("the kernel does not fit the padded input")
    ho, wo = (hin + 2 * padding - k) // stride + 1, (win + 2 * padding - k) // stride + 1
    if residual is not None and tuple(residual.shape) != (B, cout, ho, wo):
        raise ValueError(f"residual must be {(B, cout, ho, wo)}, got {tuple(residual.shape)}")
    nbytes = lib.bn_unet_conv2d_workspace_bytes(cin, cout, k)
    if nbytes == 0:
        raise ValueError("channels must be in [1, 4096] and the kernel 1, 3 or 7 wide")
    with torch.cuda.device(dev):
        out = torch.empty(B, cout, ho, wo, device=dev, dtype=torch.float32)
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        code = lib.bn_unet_conv2d_async(dev.index, stream_ptr(dev), _ptr(a), ca, _ptr(skip), cb, int(bool(upsample)), B, hin, win, _ptr(weight),
                                        _ptr(bias), cout, k, int(stride), int(padding), _ptr(residual), int(bool(relu)), _ptr(out),
                                        _ptr(work), nbytes)
    if code == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_unet_last_error().decode("utf-8", "replace"))
    check(lib, "unet", code)
    return out


def maxpool(x, device=None) -> torch.Tensor:
    """bn_unet_maxpool_async: the network's 3x3 stride-2 pad-1 max-pool of (B, C, h, w), padding counting as -inf."""
    dev = resolve_device(device, "unet")
    lib = _capi.load()
    x = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("x must be a non-empty (B, C, h, w)")
    B, ch, h, w = x.shape
    with torch.cuda.device(dev):
        out = torch.empty(B, ch, (h - 1) // 2 + 1, (w - 1) // 2 + 1, device=dev, dtype=torch.float32)
        code = lib.bn_unet_maxpool_async(dev.index, stream_ptr(dev), _ptr(x), B * ch, h, w, _ptr(out))
    if code == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_unet_last_error().decode("utf-8", "replace"))
    check(lib, "unet", code)
    return out


def load_terrain_classifier(path: str, classes: int = 10, device=None) -> TerrainClassifier:
    """A TerrainClassifier from the file the reference's ClassifierTrainer.save_model writes (torch.save(model.state_dict())),
    read with weights_only=True."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    return TerrainClassifier(state, classes=classes, device=device)
