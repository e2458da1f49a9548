"""GPU: the single layers that train the U-Net terrain classifier (benchnav_amd/unet_train.py, csrc/segtrain_kernels.hip, DESIGN.md
4.12).  Convolution gradients and the max-pool's backward on small-integer data, where every float32 sum is exact whatever its
order: the device must equal float64 autograd on the CPU bit for bit.  The float64-rule primitives (BatchNorm, cross-entropy, Adam)
on random float32 data within one float32 ulp of the tensor's largest magnitude from the float64 formula.  Real-valued convolution
gradients under unet_cases.BOUND_FACTOR times the float32 CPU figure (tests/golden/unet_train.json)."""
import math

import pytest
import torch
import torch.nn.functional as F

import unet_cases as UC
import unet_train_cases as TC

pytestmark = pytest.mark.gpu


def _ulp_of_max(t: torch.Tensor) -> float:
    m = float(t.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 2.0 ** -149


def _within_one_ulp(got: torch.Tensor, want: torch.Tensor, what) -> None:
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
    err, ulp = float((got.cpu().double() - want.double()).abs().max()), _ulp_of_max(want)
    assert err <= ulp, (what, err, ulp)


@pytest.mark.parametrize("name", sorted(TC.CONV_CASES))
def test_convolution_gradients_on_small_integers_are_exact(name):
    """Weights, inputs and output gradients in {-3 ... 3}: every sum stays an integer below 2^24 (at most 9 x 4800 in backward-weight,
    9 x 9 x 80 in backward-data), so float32 holds it exactly in any order.  The weights are random, hence asymmetric: a transposed
    tile, a wrong flip or a permuted k cannot pass."""
    from benchnav_amd import unet_train
    _, _, _, _, _, _, stride, pad, _, up, need = TC.CONV_CASES[name]
    a, skip, weight, grad_out = TC.conv_inputs(name)
    want = TC.conv_reference(name, a, skip, weight, grad_out)
    got = unet_train.conv2d_backward(a, weight, grad_out, stride, pad, skip=skip, upsample=up, need=need)
    for key, g, w in zip(("weight", "a", "skip"), got, want):
        if key not in need:
            assert g is None
            continue
        assert g.dtype == torch.float32 and w.abs().max() > 0 and torch.equal(g.cpu().double(), w), (name, key)


@pytest.mark.parametrize("name", TC.ACCUMULATE_CASES)
def test_data_gradients_accumulate_into_a_nonzero_destination(name):
    """How the encoder features' two consumers and the BasicBlock identity add their gradients: through the convolution's residual
    port (and the split kernel), never an atomic."""
    from benchnav_amd import unet_train
    _, _, _, _, _, _, stride, pad, _, up, need = TC.CONV_CASES[name]
    a, skip, weight, grad_out = TC.conv_inputs(name)
    gen = torch.Generator().manual_seed(99)
    into_a = torch.randint(-3, 4, a.shape, generator=gen).float()
    into_skip = None if skip is None else torch.randint(-3, 4, skip.shape, generator=gen).float()
    _, want_a, want_skip = TC.conv_reference(name, a, skip, weight, grad_out)
    _, got_a, got_skip = unet_train.conv2d_backward(a, weight, grad_out, stride, pad, skip=skip, upsample=up, need=("a", "skip"), into_a=into_a,
                                                    into_skip=into_skip)
    assert torch.equal(got_a.cpu().double(), want_a + into_a.double()), name
    if skip is not None:
        assert torch.equal(got_skip.cpu().double(), want_skip + into_skip.double()), name


@pytest.mark.parametrize("name", TC.REAL_CASES)
def test_real_valued_convolution_gradients_stay_within_the_float32_cpu_bound(name):
    from benchnav_amd import unet_train
    _, _, _, _, _, _, stride, pad, _, up, need = TC.CONV_CASES[name]
    a, skip, weight, grad_out = TC.conv_inputs(name, integers=False)
    want = TC.conv_reference(name, a, skip, weight, grad_out)
    got = unet_train.conv2d_backward(a, weight, grad_out, stride, pad, skip=skip, upsample=up, need=need)
    recorded = TC.golden()["conv"][name]
    errors = {key: TC.relative_error(g.cpu(), w) for key, g, w in zip(("weight", "a", "skip"), got, want) if key in need and w is not None}
    print(f"\n{name}: " + ", ".join(f"grad_{k} {e:.3e} = {e / recorded[k]:.2f} x the float32 CPU figure" for k, e in errors.items()))
    for key, e in errors.items():
        assert e <= UC.BOUND_FACTOR * recorded[key], (name, key, e, recorded[key])


@pytest.mark.parametrize("shape", [(2, 3, 4, 4), (1, 2, 7, 5), (1, 1, 6, 9), (2, 1, 1, 1)])
def test_maxpool_backward_sends_a_tie_to_the_first_maximum(shape):
    """Integer data in {0, 1, 2} (ties in most windows) with one all-zero plane, even and odd sizes, against torch's CPU float64
    backward: the first maximum in row-major order wins (val > maxval)."""
    from benchnav_amd import unet_train
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(0, 3, shape, generator=gen).float()
    x[0, 0] = 0.0
    xd = x.double().requires_grad_()
    y = F.max_pool2d(xd, 3, 2, 1)
    grad_out = torch.randint(-3, 4, y.shape, generator=gen).float()
    grad_out[grad_out == 0] = 1.0
    want, = torch.autograd.grad(y, xd, grad_out.double())
    got = unet_train.maxpool_backward(x, grad_out)
    assert torch.equal(got.cpu().double(), want), shape
    into = torch.randint(-3, 4, shape, generator=gen).float()
    assert torch.equal(unet_train.maxpool_backward(x, grad_out, into=into).cpu().double(), want + into.double())
    if shape == (2, 3, 4, 4):              # the all-zero plane: the four window gradients land on (0,0), (0,1), (1,0), (1,1)
        plane = got[0, 0].cpu()
        assert torch.equal(plane[:2, :2], grad_out[0, 0]) and float(plane.abs().sum()) == float(grad_out[0, 0].abs().sum())


BN_SHAPES = [(2, 5, 1, 1), (3, 5, 2, 2), (4, 5, 25, 41), (2, 64, 1, 1), (3, 64, 2, 2), (4, 64, 25, 41)]     # 2, 12 and 4100 values per channel


def _bn_spec(x, gamma, beta, residual, relu):
    xd = x.double()
    mean, var = xd.mean(dim=(0, 2, 3), keepdim=True), xd.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    y = (xd - mean) * gamma.double().view(1, -1, 1, 1) / torch.sqrt(var + 1e-5) + beta.double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    return (y.clamp_min(0.0) if relu else y), mean.reshape(-1), var.reshape(-1)


@pytest.mark.parametrize("shape", BN_SHAPES)
@pytest.mark.parametrize("relu,with_residual", [(True, True), (False, False)])
def test_batchnorm_training_forward_and_backward_follow_the_float64_rule(shape, relu, with_residual):
    from benchnav_amd import unet_train
    gen = torch.Generator().manual_seed(sum(shape) + 2 * relu)
    B, ch, h, w = shape
    n = B * h * w
    x = torch.randn(shape, generator=gen) * 2.0 + 0.5
    gamma, beta = torch.rand(ch, generator=gen) + 0.5, torch.randn(ch, generator=gen) * 0.2
    residual = torch.randn(shape, generator=gen) if with_residual else None
    rm, rv = torch.randn(ch, generator=gen) * 0.2, torch.rand(ch, generator=gen) + 0.5
    y, stats, rm_new, rv_new = unet_train.batchnorm_forward(x, gamma, beta, residual, relu, rm, rv)
    want_y, mean, var = _bn_spec(x, gamma, beta, residual, relu)
    _within_one_ulp(y, want_y, "y")
    _within_one_ulp(rm_new, 0.9 * rm.double() + 0.1 * mean, "running_mean")
    _within_one_ulp(rv_new, 0.9 * rv.double() + 0.1 * var * n / (n - 1), "running_var (unbiased)")
    assert torch.allclose(stats[0].cpu(), mean, rtol=1e-12, atol=1e-14) and torch.allclose(stats[1].cpu(), 1.0 / torch.sqrt(var + 1e-5), rtol=1e-12)
    # backward: autograd through the same float64 formula
    leaves = [x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()]
    res = None if residual is None else residual.double().requires_grad_()
    out, _, _ = _bn_spec(leaves[0], leaves[1], leaves[2], res, relu)
    grad_out = torch.randn(shape, generator=gen)
    want = torch.autograd.grad(out, leaves + ([res] if res is not None else []), grad_out.double())
    gx, gr, gg, gb = unet_train.batchnorm_backward(grad_out, y, x, stats, gamma, relu, residual=with_residual)
    _within_one_ulp(gx, want[0], "grad_x")
    _within_one_ulp(gg, want[1], "grad_gamma")
    _within_one_ulp(gb, want[2], "grad_beta")
    if with_residual:
        _within_one_ulp(gr, want[3], "grad_residual")
    else:
        assert gr is None


@pytest.mark.parametrize("classes", [10, 3])
@pytest.mark.parametrize("shape", [(1, 1, 2), (3, 2, 2), (4, 25, 41)])
def test_cross_entropy_follows_the_float64_rule(classes, shape):
    from benchnav_amd import unet_train
    gen = torch.Generator().manual_seed(classes + sum(shape))
    B, H, W = shape
    logits = torch.randn(B, classes, H, W, generator=gen) * 3.0
    targets = torch.randint(0, classes, shape, generator=gen)
    ld = logits.double().requires_grad_()
    want = F.cross_entropy(ld, targets)
    want_grad, = torch.autograd.grad(want, ld)
    loss, grad = unet_train.cross_entropy(logits, targets)
    _within_one_ulp(loss.reshape(()), want.detach(), "loss")
    _within_one_ulp(grad, want_grad, "grad_logits")
    loss_only, none = unet_train.cross_entropy(logits, targets, need_grad=False)
    assert none is None and torch.equal(loss_only, loss)
    bad = targets.clone()
    bad[0, 0, 0] = classes
    with pytest.raises(ValueError):
        unet_train.cross_entropy(logits, bad)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_adam_follows_torchs_formula_over_three_steps(weight_decay):
    """Each step from the float32 state the device itself left: float64 arithmetic, p, m and v rounded once."""
    from benchnav_amd import unet_train
    gen = torch.Generator().manual_seed(5)
    n, lr, b1, b2, eps = 4100, 1e-2, 0.9, 0.999, 1e-8
    p, m, v = torch.randn(n, generator=gen), torch.zeros(n), torch.zeros(n)
    for t in (1, 2, 3):
        g = torch.randn(n, generator=gen) * (10.0 ** torch.randint(-4, 1, (n,), generator=gen).float())
        pd, gd = p.double(), g.double() + weight_decay * p.double()
        wm, wv = b1 * m.double() + (1 - b1) * gd, b2 * v.double() + (1 - b2) * gd * gd
        wp = pd - (lr / (1 - b1 ** t)) * wm / (wv.sqrt() / math.sqrt(1 - b2 ** t) + eps)
        gp, gm, gv = unet_train.adam(p, g, m, v, t, lr, weight_decay, (b1, b2), eps)
        _within_one_ulp(gp, wp, ("p", t))
        _within_one_ulp(gm, wm, ("m", t))
        _within_one_ulp(gv, wv, ("v", t))
        p, m, v = gp.cpu(), gm.cpu(), gv.cpu()
    ref = torch.nn.Parameter(torch.ones(3, dtype=torch.float64))
    opt = torch.optim.Adam([ref], lr=lr, weight_decay=weight_decay)
    ref.grad = torch.tensor([0.5, -2.0, 1e-3], dtype=torch.float64)
    opt.step()
    got, _, _ = unet_train.adam(torch.ones(3), ref.grad.float(), torch.zeros(3), torch.zeros(3), 1, lr, weight_decay)
    _within_one_ulp(got, ref.detach(), "torch.optim.Adam's first step")
