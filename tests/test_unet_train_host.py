"""CPU: the host side of training the U-Net terrain classifier (benchnav_amd/unet_train.py, csrc/segtrain_host.cpp): every entry
point rejects bad arguments before it touches a device, the packed layout round-trips bit for bit and strictly, init_state_dict is
a function of its seed, and the packed state folds to what the classifier folds from the state dict itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import unet_cases as UC
import unet_spec
from benchnav_amd import _capi, unet, unet_train


def test_c_abi_rejects_bad_arguments_before_touching_the_device():
    lib = _capi.load()
    n = lib.bn_segtrain_param_count(10)
    assert n == unet_train.param_count(10) and lib.bn_segtrain_param_count(0) == 0 and lib.bn_segtrain_param_count(33) == 0
    # folded: weight + bias per convolution; unfolded: weight + four BatchNorm vectors (the head: weight + bias)
    assert n == unet.param_count(10) + 3 * sum(s[0] for _, bn, s, _, _ in unet.conv_table(10) if bn is not None)
    params = np.zeros(n, np.float32)
    h = C.c_void_p()

    def create(classes=10, p=params, count=None):
        return lib.bn_segtrain_create(0, classes, p.ctypes.data if p is not None else None, p.size if count is None else count, C.byref(h))
    bad = params.copy()
    bad[n // 2] = np.inf
    for kw, word in ((dict(classes=0), b"[1, 32]"), (dict(classes=33), b"[1, 32]"), (dict(count=n - 1), b"count"), (dict(p=bad), b"finite"),
                     (dict(p=None, count=n), b"null")):
        assert create(**kw) == _capi.BN_ERR_INVALID, kw
        assert word in lib.bn_segtrain_last_error(), (kw, lib.bn_segtrain_last_error())
    assert lib.bn_segtrain_create(0, 10, params.ctypes.data, n, None) == _capi.BN_ERR_INVALID
    # the workspace: bn_unet_workspace_bytes' range, and more than one value per channel at the bottleneck
    assert lib.bn_segtrain_workspace_bytes(2, 32, 32) > 0 and lib.bn_segtrain_workspace_bytes(1, 32, 64) > 0
    assert lib.bn_segtrain_workspace_bytes(3, 64, 64) > lib.bn_unet_workspace_bytes(3, 64, 64)
    for args in ((1, 32, 32), (1, 48, 64), (2, 64, 48), (0, 64, 64), (2, 0, 64), (2, 64, 2080), (4097, 32, 32), (65, 512, 512), (2, -32, 32)):
        assert lib.bn_segtrain_workspace_bytes(*args) == 0, args
    fake = C.c_void_p(256)

    def grad(hh=fake, B=2, H=32, W=32, x=fake, t=fake, loss=fake, ws=fake, nbytes=1 << 40):
        return lib.bn_segtrain_grad_async(hh, None, B, H, W, x, t, loss, ws, nbytes)

    def step(hh=fake, B=2, H=32, W=32, x=fake, t=fake, loss=fake, ws=fake, nbytes=1 << 40, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
        return lib.bn_segtrain_step_async(hh, None, B, H, W, x, t, lr, b1, b2, eps, wd, loss, ws, nbytes)
    for call in (grad, step):
        for kw in (dict(hh=None), dict(x=None), dict(t=None), dict(loss=None), dict(ws=None), dict(H=48), dict(B=0), dict(B=1)):
            assert call(**kw) == _capi.BN_ERR_INVALID, (call.__name__, kw)
        assert call(B=1) == _capi.BN_ERR_INVALID and b"more than 1 value per channel" in lib.bn_segtrain_last_error()
    assert lib.bn_segtrain_read(None, 0, fake, n) == _capi.BN_ERR_INVALID and lib.bn_segtrain_read(fake, 0, None, n) == _capi.BN_ERR_INVALID
    assert lib.bn_segtrain_steps(None) == -1
    lib.bn_segtrain_destroy(None)

    def conv(a=fake, ca=3, skip=None, cb=0, up=0, maps=1, hin=8, win=8, w=fake, cout=4, k=3, stride=1, pad=1, go=fake, gw=fake, ga=fake, gs=None,
             ws=fake, nbytes=1 << 30):
        return lib.bn_segtrain_conv2d_backward_async(0, None, a, ca, skip, cb, up, maps, hin, win, w, cout, k, stride, pad, go, gw, ga, gs, 0, ws, nbytes)
    for kw in (dict(a=None), dict(w=None), dict(go=None), dict(ws=None), dict(cb=2), dict(gs=fake), dict(k=5), dict(stride=3), dict(pad=4),
               dict(k=1, pad=1), dict(ca=0), dict(cout=0), dict(cout=4097), dict(nbytes=16), dict(up=1, hin=7), dict(hin=0), dict(k=7, pad=0, hin=4),
               dict(maps=0)):
        assert conv(**kw) == _capi.BN_ERR_INVALID, kw
    assert lib.bn_segtrain_conv2d_backward_workspace_bytes(1, 3, 8, 8, 4, 3, 1, 1) > 0
    assert lib.bn_segtrain_conv2d_backward_workspace_bytes(1, 3, 8, 8, 4, 5, 1, 1) == 0

    def bn_fwd(x=fake, maps=2, ch=4, cells=6, g=fake, b=fake, y=fake, st=fake):
        return lib.bn_segtrain_batchnorm_forward_async(0, None, x, maps, ch, cells, g, b, None, 1, None, None, y, st)
    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(y=None), dict(st=None), dict(maps=0), dict(ch=0), dict(ch=4097), dict(cells=0),
               dict(maps=1, cells=1)):
        assert bn_fwd(**kw) == _capi.BN_ERR_INVALID, kw

    def bn_bwd(dy=fake, y=fake, x=fake, st=fake, g=fake, maps=2, ch=4, cells=6, dx=fake, dg=fake, db=fake, sums=fake):
        return lib.bn_segtrain_batchnorm_backward_async(0, None, dy, y, x, st, g, 1, maps, ch, cells, dx, None, dg, db, sums)
    for kw in (dict(dy=None), dict(y=None), dict(x=None), dict(st=None), dict(g=None), dict(dx=None), dict(dg=None), dict(db=None), dict(sums=None),
               dict(maps=1, cells=1), dict(ch=0)):
        assert bn_bwd(**kw) == _capi.BN_ERR_INVALID, kw
    assert lib.bn_segtrain_maxpool_backward_async(0, None, None, fake, 1, 4, 4, fake, 0) == _capi.BN_ERR_INVALID
    assert lib.bn_segtrain_maxpool_backward_async(0, None, fake, fake, 0, 4, 4, fake, 0) == _capi.BN_ERR_INVALID
    assert lib.bn_segtrain_cross_entropy_async(0, None, None, fake, 1, 3, 4, fake, None, fake, 32) == _capi.BN_ERR_INVALID
    assert lib.bn_segtrain_cross_entropy_async(0, None, fake, fake, 1, 33, 4, fake, None, fake, 32) == _capi.BN_ERR_INVALID
    assert lib.bn_segtrain_cross_entropy_async(0, None, fake, fake, 1, 3, 4, fake, None, fake, 31) == _capi.BN_ERR_INVALID
    assert b"workspace" in lib.bn_segtrain_last_error()
    assert lib.bn_segtrain_adam_async(0, None, None, fake, fake, fake, 4, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0) == _capi.BN_ERR_INVALID
    assert lib.bn_segtrain_adam_async(0, None, fake, fake, fake, fake, 4, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0) == _capi.BN_ERR_INVALID
    assert lib.bn_segtrain_adam_async(0, None, fake, fake, fake, fake, 4, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0) == _capi.BN_ERR_INVALID
    if not torch.cuda.is_available():
        assert create() == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_segtrain_last_error()
        for call in (conv, bn_fwd, bn_bwd):
            assert call() == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_segtrain_last_error(), call.__name__
        assert lib.bn_segtrain_maxpool_backward_async(0, None, fake, fake, 1, 4, 4, fake, 0) == _capi.BN_ERR_NO_DEVICE
        assert lib.bn_segtrain_cross_entropy_async(0, None, fake, fake, 1, 3, 4, fake, None, fake, 32) == _capi.BN_ERR_NO_DEVICE
        assert lib.bn_segtrain_adam_async(0, None, fake, fake, fake, fake, 4, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0) == _capi.BN_ERR_NO_DEVICE
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            unet_train.TrainableTerrainClassifier(UC.state_dict())


def test_pack_and_unpack_round_trip_bit_for_bit_and_strictly():
    sd = UC.state_dict()
    packed = unet_train.pack_state_dict(sd, UC.CLASSES)
    assert packed.dtype == np.float32 and packed.size == unet_train.param_count(UC.CLASSES)
    back = unet_train.unpack_params(packed, UC.CLASSES, num_batches_tracked=7)
    assert set(back) == set(sd)
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert back[k].dtype == torch.int64 and int(back[k]) == 7
        else:
            assert back[k].dtype == torch.float32 and np.array_equal(back[k].numpy().view(np.uint32), v.numpy().view(np.uint32)), k
    assert np.array_equal(unet_train.pack_state_dict(back, UC.CLASSES).view(np.uint32), packed.view(np.uint32))
    unet_spec.Unet(UC.CLASSES).load_state_dict(back, strict=True)
    # the layout: the first convolution's weight, then its BatchNorm's four vectors
    assert np.array_equal(packed[:64 * 147], sd["encoder.conv1.weight"].numpy().reshape(-1))
    assert np.array_equal(packed[64 * 147 + 128:64 * 147 + 192], sd["encoder.bn1.running_mean"].numpy())
    trainable = unet_train.unpack_params(packed, UC.CLASSES, trainable_only=True)
    assert set(trainable) == {k for k, _ in unet_spec.Unet(UC.CLASSES).named_parameters()}
    # strict
    for mutate, word in ((lambda d: d.pop("decoder.blocks.2.conv1.1.running_var"), "decoder.blocks.2.conv1.1.running_var"),
                         (lambda d: d.update(extra=torch.zeros(1)), "extra"),
                         (lambda d: d.update({"encoder.layer2.0.downsample.0.weight": torch.zeros(128, 64, 3, 3)}), "encoder.layer2.0.downsample.0.weight"),
                         (lambda d: d.update({"segmentation_head.0.bias": torch.full((UC.CLASSES,), float("nan"))}), "segmentation_head.0.bias")):
        d = dict(sd)
        mutate(d)
        with pytest.raises(ValueError, match=word):
            unet_train.pack_state_dict(d, UC.CLASSES)
    with pytest.raises(ValueError):
        unet_train.unpack_params(packed[:-1], UC.CLASSES)
    with pytest.raises(ValueError):
        unet_train.pack_state_dict(sd, 0)


def test_init_state_dict_is_a_function_of_its_seed():
    a, b, c = unet_train.init_state_dict(10, seed=3), unet_train.init_state_dict(10, seed=3), unet_train.init_state_dict(10, seed=4)
    assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(c)
    assert not torch.equal(a["encoder.conv1.weight"], c["encoder.conv1.weight"])
    unet_spec.Unet(10).load_state_dict(a, strict=True)
    w = a["encoder.layer1.0.conv1.weight"]
    assert float(w.abs().max()) <= 1.0 / np.sqrt(64 * 9) and float(w.std()) > 0.4 / np.sqrt(64 * 9)
    assert torch.equal(a["encoder.bn1.weight"], torch.ones(64)) and torch.equal(a["encoder.bn1.running_var"], torch.ones(64))
    assert a["encoder.bn1.num_batches_tracked"].dtype == torch.int64
    assert unet_train.init_state_dict(3, seed=0)["segmentation_head.0.weight"].shape == (3, 16, 3, 3)


def test_the_packed_state_folds_to_what_the_state_dict_folds_to():
    sd = UC.state_dict()
    direct = unet.fold_state_dict(sd, UC.CLASSES)
    via = unet.fold_state_dict(unet_train.unpack_params(unet_train.pack_state_dict(sd, UC.CLASSES), UC.CLASSES), UC.CLASSES)
    assert np.array_equal(direct.view(np.uint32), via.view(np.uint32))


def test_wrappers_reject_bad_targets_without_a_device():
    with pytest.raises(ValueError, match="targets"):
        unet_train._check_targets(torch.zeros(2, 32, 31, dtype=torch.int64), (2, 32, 32), 10, "cpu")
    with pytest.raises(ValueError, match="targets"):
        unet_train._check_targets(torch.zeros(2, 32, 32), (2, 32, 32), 10, "cpu")
    for bad in (-1, 10):
        t = torch.zeros(2, 32, 32, dtype=torch.int64)
        t[1, 3, 4] = bad
        with pytest.raises(ValueError, match=r"\[0, 10\)"):
            unet_train._check_targets(t, (2, 32, 32), 10, "cpu")
    assert unet_train._check_targets(torch.full((1, 2, 2), 9, dtype=torch.int32), (1, 2, 2), 10, "cpu").dtype == torch.int64
