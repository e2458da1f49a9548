"""The specification the U-Net tests hold the device to: segmentation_models_pytorch's Unet(encoder_name="resnet18", classes=C)
restated in plain torch.nn, with smp's state-dict key names (as documented; not checked against a real checkpoint).  Runs on
the CPU in float64 or float32, and on any device as the rate tool's baseline.  Not a test module."""
import torch
from torch import nn
import torch.nn.functional as F


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(out)) + identity)


class Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, w in enumerate((64, 128, 256, 512)):
            setattr(self, f"layer{i + 1}", nn.Sequential(BasicBlock(cin, w, 2 if i else 1), BasicBlock(w, w, 1)))
            cin = w

    def forward(self, x):
        f1 = F.relu(self.bn1(self.conv1(x)))
        f2 = self.layer1(F.max_pool2d(f1, 3, 2, 1))
        f3 = self.layer2(f2)
        f4 = self.layer3(f3)
        f5 = self.layer4(f4)
        return [f1, f2, f3, f4, f5]


class DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(cin + cskip, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())
        self.conv2 = nn.Sequential(nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())

    def forward(self, x, skip):
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        return self.conv2(self.conv1(x))


class Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = nn.ModuleList(DecoderBlock(i, s, o) for i, s, o in zip((512, 256, 128, 64, 32), (256, 128, 64, 64, 0), (256, 128, 64, 32, 16)))


class Unet(nn.Module):
    """forward(x) -> logits (B, C, H, W); features(x) -> (five encoder features, five decoder block outputs)."""

    def __init__(self, classes=10):
        super().__init__()
        self.encoder = Encoder()
        self.decoder = Decoder()
        self.segmentation_head = nn.Sequential(nn.Conv2d(16, classes, 3, 1, 1))

    def features(self, x):
        if x.shape[-2] % 32 or x.shape[-1] % 32:
            raise ValueError(f"height and width must be multiples of 32, got {tuple(x.shape[-2:])}")
        enc = self.encoder(x)
        skips = [enc[3], enc[2], enc[1], enc[0], None]
        dec, y = [], enc[4]
        for block, skip in zip(self.decoder.blocks, skips):
            y = block(y, skip)
            dec.append(y)
        return enc, dec

    def forward(self, x):
        return self.segmentation_head(self.features(x)[1][-1])

    def predict(self, x, return_probabilities=False):
        p = torch.softmax(self.forward(x), dim=1)
        return p if return_probabilities else p.argmax(dim=1)


class FoldedUnet(nn.Module):
    """The same network from the packed folded parameters of benchnav_amd.unet.fold_state_dict: convolution + bias only."""

    def __init__(self, params, classes=10, dtype=torch.float64):
        super().__init__()
        from benchnav_amd.unet import conv_table
        self.convs = []
        at = 0
        p = torch.as_tensor(params).to(dtype)
        for _, _, shape, stride, pad in conv_table(classes):
            n = shape[0] * shape[1] * shape[2] * shape[3]
            self.convs.append((p[at:at + n].reshape(shape), p[at + n:at + n + shape[0]], stride, pad))
            at += n + shape[0]
        assert at == p.numel()

    def _c(self, i, x):
        w, b, s, pad = self.convs[i]
        return F.conv2d(x, w, b, s, pad)

    def forward(self, x):
        f = [F.relu(self._c(0, x))]
        y, i = F.max_pool2d(f[0], 3, 2, 1), 1
        for l in range(4):
            t = F.relu(self._c(i, y))
            identity = self._c(i + 2, y) if l else y
            y = F.relu(self._c(i + 1, t) + identity)
            i += 3 if l else 2
            y = F.relu(self._c(i + 1, F.relu(self._c(i, y))) + y)
            i += 2
            f.append(y)
        for b, skip in enumerate((f[3], f[2], f[1], f[0], None)):
            y = F.interpolate(y, scale_factor=2, mode="nearest")
            if skip is not None:
                y = torch.cat([y, skip], dim=1)
            y = F.relu(self._c(i + 1, F.relu(self._c(i, y))))
            i += 2
        return self._c(i, y)
