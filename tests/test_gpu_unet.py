"""GPU: the U-Net terrain classifier (benchnav_amd/unet.py, csrc/unet_kernels.hip).

Layer level: the fused convolution and the max-pool on small-integer data, where every float32 sum is exact whatever its order, so
the device must equal float64 on the CPU bit for bit.  Network level: seeded cases (tests/unet_cases.py) against the float64 spec
(tests/unet_spec.py) under a bound that comes from the float32 CPU spec's own error (tests/golden/unet.json).  Then the
invariants (repeatability, batch independence, the caller's stream, ties) and the interface up to TraversabilityPredictor."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_cases as UC

pytestmark = pytest.mark.gpu


def _bits(t: torch.Tensor) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _ints(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).to(torch.float32)


# name: (B, Ca, h, w of a, Cout, k, stride, pad, Cb, upsample, bias, residual, relu)
CONV_CASES = {
    "stem_7x7_s2_cin3_32x32": (1, 3, 32, 32, 16, 7, 2, 3, 0, False, True, False, True),
    "3x3_s1_out1x1": (1, 5, 1, 1, 16, 3, 1, 1, 0, False, True, False, False),
    "3x3_s1_out2x2_b3": (3, 3, 2, 2, 10, 3, 1, 1, 0, False, False, False, False),
    "3x3_s1_out1x3": (1, 64, 1, 3, 48, 3, 1, 1, 0, False, True, False, False),
    "3x3_s1_out5x4_b3": (3, 5, 5, 4, 16, 3, 1, 1, 0, False, True, True, True),
    "3x3_s2_out1x1": (1, 5, 2, 2, 10, 3, 2, 1, 0, False, True, False, False),
    "3x3_s2_out2x2": (1, 64, 4, 4, 16, 3, 2, 1, 0, False, False, True, True),
    "3x3_s2_out1x3_b3": (3, 5, 2, 6, 48, 3, 2, 1, 0, False, True, False, False),
    "3x3_s2_out5x4_odd_input": (1, 5, 9, 7, 10, 3, 2, 1, 0, False, True, False, True),
    "1x1_s2_cin64": (3, 64, 6, 5, 48, 1, 2, 0, 0, False, True, False, False),
    "3x3_cin768_k_slabs": (1, 768, 2, 2, 16, 3, 1, 1, 0, False, True, True, True),
    "3x3_s1_9x9_b3_four_pixel_tiles_cout80": (3, 5, 9, 9, 80, 3, 1, 1, 0, False, True, True, False),
    "head_like_cout10_b3": (3, 16, 5, 4, 10, 3, 1, 1, 0, False, True, False, False),
    "upsample_concat_a2x2x8_skip4x4x4": (1, 8, 2, 2, 16, 3, 1, 1, 4, True, True, False, True),
    "upsample_concat_b3": (3, 8, 2, 2, 10, 3, 1, 1, 4, True, True, True, True),
    "upsample_no_skip": (1, 8, 2, 2, 16, 3, 1, 1, 0, True, True, False, True),
}


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_convolution_on_small_integers_is_exact(name):
    """Weights, inputs, bias and residual in {-3 ... 3}: |sum| <= 9 x 6912 + 6 < 2^24, so every partial sum is an integer float32
    holds exactly.  The weights are random, hence asymmetric: a transposed tile or a permuted k cannot pass."""
    from benchnav_amd import unet
    B, ca, h, w, cout, k, stride, pad, cb, up, has_bias, has_res, relu = CONV_CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    a = _ints(gen, B, ca, h, w)
    hin, win = (2 * h, 2 * w) if up else (h, w)
    skip = _ints(gen, B, cb, hin, win) if cb else None
    weight = _ints(gen, cout, ca + cb, k, k)
    bias = _ints(gen, cout) if has_bias else None
    x = F.interpolate(a, scale_factor=2, mode="nearest") if up else a
    if skip is not None:
        x = torch.cat([x, skip], dim=1)
    want = F.conv2d(x.double(), weight.double(), None if bias is None else bias.double(), stride, pad)
    residual = _ints(gen, *want.shape) if has_res else None
    if residual is not None:
        want = want + residual.double()
    if relu:
        want = want.clamp_min(0.0)
    got = unet.conv2d(a, weight, bias, stride, pad, skip=skip, upsample=up, residual=residual, relu=relu)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    assert want.abs().max() > 0 and torch.equal(got.cpu().double(), want), name


def test_maxpool_counts_padding_as_minus_infinity():
    """Directly on negative data (a zero-padded pool would return 0 along the border), on odd and even sizes.  Inside the network
    the pool's input follows a ReLU, so the padding value cannot show through `features`: the next test holds the pool's place in
    the forward instead."""
    from benchnav_amd import unet
    gen = torch.Generator().manual_seed(7)
    for shape in ((2, 3, 6, 8), (1, 2, 7, 5), (1, 1, 1, 1), (1, 1, 2, 2)):
        x = -1.0 - torch.randint(0, 9, shape, generator=gen).to(torch.float32)
        got = unet.maxpool(x)
        want = F.max_pool2d(x, 3, 2, 1)
        assert torch.equal(got.cpu(), want) and (want < 0).all(), shape


@pytest.fixture(scope="module")
def clf():
    from benchnav_amd.unet import TerrainClassifier
    c = TerrainClassifier(UC.state_dict(), classes=UC.CLASSES)
    yield c
    c.close()


def _identity_bn(sd):
    """Every BatchNorm of the state dict made the identity up to eps (folded exactly below by var = 1 - eps)."""
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = torch.full_like(sd[k], 1.0 - 1e-5)
        elif k.endswith("running_mean") or (k.endswith(".bias") and "segmentation_head" not in k):
            sd[k] = torch.zeros_like(sd[k])
        elif k.endswith(".weight") and sd[k].dim() == 1:
            sd[k] = torch.ones_like(sd[k])


def test_maxpool_through_features_on_integer_data():
    """Stem: the centre tap copies colour channel c to channels c, c + 3 (negated) -- after the ReLU the positive and the negative
    part.  layer1: all-zero convolutions, so each block returns relu(0 + identity) = its input.  Then layer1's feature is the
    max-pool of the stem feature, exactly."""
    from benchnav_amd.unet import TerrainClassifier
    sd = {k: v.clone() for k, v in UC.state_dict().items()}
    _identity_bn(sd)
    w = torch.zeros_like(sd["encoder.conv1.weight"])
    for c in range(3):
        w[c, c, 3, 3] = 1.0
        w[c + 3, c, 3, 3] = -1.0
    sd["encoder.conv1.weight"] = w
    for k in sd:
        if k.startswith("encoder.layer1") and "conv" in k:
            sd[k] = torch.zeros_like(sd[k])
    gen = torch.Generator().manual_seed(11)
    x = torch.randint(-3, 4, (2, 3, 32, 64), generator=gen).to(torch.float32)
    net = TerrainClassifier(sd, classes=UC.CLASSES)
    try:
        enc, _ = net.features(x)
    finally:
        net.close()
    # the fold's scale 1 / sqrt(float32(1 - 1e-5) + 1e-5) = 1 + 7e-9 rounds to 1.0f: the folded weights are the integers above
    stem = torch.zeros(2, 64, 16, 32)
    stem[:, 0:3] = x[:, :, ::2, ::2].clamp_min(0.0)
    stem[:, 3:6] = (-x[:, :, ::2, ::2]).clamp_min(0.0)
    assert torch.equal(enc[0].cpu(), stem)
    assert torch.equal(enc[1].cpu(), F.max_pool2d(stem, 3, 2, 1))


@pytest.mark.parametrize("name", sorted(UC.CASES))
def test_network_matches_the_float64_spec(clf, name):
    """Logits and every feature within 8 x the float32 CPU spec's own relative error; the class map equal to the float64 argmax in
    every cell whose top-two margin exceeds twice that bound; probabilities within 4 ulp of the float64 softmax of the device's
    own logits, summing to 1 within 1e-6."""
    x = UC.colors(name)
    ref, renc, rdec = UC.reference(name)
    bound = UC.logit_bound(name)
    logits = clf(x)
    assert logits.dtype == torch.float32 and logits.is_cuda and tuple(logits.shape) == tuple(ref.shape)
    lo = logits.cpu().double()
    rel = float((lo - ref).abs().max() / ref.abs().max())
    print(f"\n{name}: device logits relative error {rel:.3e} = {rel / UC.golden()[name]['float32_cpu_relative_error']:.2f} x the float32 CPU "
          f"figure (bound {UC.BOUND_FACTOR:.0f} x)")
    assert rel <= bound, (name, rel, bound)

    enc, dec = clf.features(x)
    for stage, (got, want) in enumerate(zip(enc + dec, renc + rdec)):
        assert tuple(got.shape) == tuple(want.shape), stage
        r = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print(f"  feature {stage}: relative error {r:.3e}")
        assert r <= bound, (name, stage, r, bound)

    classes = clf.predict_classes(x)
    assert classes.dtype == torch.int32 and classes.is_cuda
    keep = UC.margin_mask(name)
    assert (~keep).double().mean() <= UC.MAX_EXCLUDED_SHARE
    assert torch.equal(classes.cpu().long()[keep], ref.argmax(1)[keep])
    assert torch.equal(classes.cpu().long(), lo.argmax(1))                 # and everywhere the argmax of the device's own logits

    prob = clf.predict(x, return_probabilities=True)
    assert prob.dtype == torch.float32 and tuple(prob.shape) == tuple(ref.shape)
    p = prob.cpu().numpy()
    q = torch.softmax(lo, dim=1).numpy()
    ulps = np.abs(p.astype(np.float64) - q) / np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)
    assert ulps.max() <= 4.0, (name, ulps.max())
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6


def test_repeatability_batch_independence_and_the_callers_stream(clf):
    x = UC.colors("b3_64x64")
    lo, cl = clf(x), clf.predict_classes(x)
    assert np.array_equal(_bits(clf(x)), _bits(lo)) and np.array_equal(_bits(clf.predict_classes(x)), _bits(cl))
    for b in range(x.shape[0]):
        assert np.array_equal(_bits(clf(x[b:b + 1])), _bits(lo[b:b + 1])), b
        assert np.array_equal(_bits(clf.predict_classes(x[b:b + 1])), _bits(cl[b:b + 1])), b
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        doubled = x.cuda(non_blocking=True) * 2.0
        ls = clf(doubled * 0.5)
    side.synchronize()
    assert np.array_equal(_bits(ls), _bits(lo))
    with pytest.raises(ValueError, match="multiples of 32"):
        clf(torch.zeros(1, 3, 48, 64))
    with pytest.raises(ValueError):
        clf(torch.zeros(1, 4, 32, 32))


def test_a_tie_goes_to_the_lowest_index():
    from benchnav_amd.unet import TerrainClassifier
    sd = {k: v.clone() for k, v in UC.state_dict().items()}
    sd["segmentation_head.0.weight"] = torch.zeros_like(sd["segmentation_head.0.weight"])
    sd["segmentation_head.0.bias"] = torch.tensor([0.5, -1.0, 2.0, 0.0, 2.0, 1.0, -3.0, 2.0, 0.0, 1.5])
    net = TerrainClassifier(sd, classes=UC.CLASSES)
    try:
        x = UC.colors("b1_32x32")
        cl, lo = net.predict_classes(x), net(x)
    finally:
        net.close()
    assert torch.equal(lo.cpu(), sd["segmentation_head.0.bias"].reshape(1, -1, 1, 1).expand(1, UC.CLASSES, 32, 32))
    assert (cl == 2).all()


def test_interface_and_checkpoint_round_trip(clf, tmp_path):
    from benchnav_amd import TerrainClassifier, load_terrain_classifier
    x = UC.colors("b2_32x96")
    pred = clf.predict(x)
    assert pred.dtype == torch.int64 and pred.is_cuda and tuple(pred.shape) == (2, 32, 96)
    assert torch.equal(pred, clf.predict_classes(x).long())
    assert torch.equal(clf.predict(x.cuda()), pred)                       # device input
    assert clf.batched is True and clf.training is False and clf.eval() is clf and clf.to("cuda") is clf
    path = str(tmp_path / "unet.pth")
    torch.save(UC.state_dict(), path)
    back = load_terrain_classifier(path, classes=UC.CLASSES)
    try:
        assert isinstance(back, TerrainClassifier) and np.array_equal(_bits(back(x)), _bits(clf(x)))
    finally:
        back.close()


def test_traversability_predictor_from_colours_to_planner_inputs(clf):
    from torch.distributions import Normal
    from benchnav_amd import io
    from benchnav_amd.gp import GPSlipRegressor, TraversabilityPredictor
    from benchnav_amd.risk import infer_risk_map
    from benchnav_amd.terrain import TerrainGenerator, slip_models
    G, B = 32, 3
    with TerrainGenerator(G, 0.5, batch=B) as gen:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = gen.generate([4, 5, 6], occupancy=np.full(4, 0.25), slip_models=slip_models(4), num_craters=1, min_radius=2, max_radius=3)
        insts = gen.to_instances()
    rng = np.random.default_rng(5)
    regs = {}
    for k in range(UC.CLASSES):
        xs = rng.uniform(-30, 30, 24 + 3 * k).astype(np.float32)
        ys = (0.4 * np.tanh(xs / (8.0 + k)) + 0.05 * rng.standard_normal(xs.size)).astype(np.float32)
        regs[k] = GPSlipRegressor(xs, ys, 0.05 * k, 0.5, 5.0 + k, 0.0025)
    colors = UC.draw_colors(9, B, G, G)
    slopes = t.slopes
    pred = TraversabilityPredictor(clf, regs)
    assert pred.terrain_classifier is clf
    # the reference's call: one map
    dist = pred.predict(colors[0], slopes[0])
    assert isinstance(dist, Normal) and dist.mean.shape == (G, G)
    m0, s0 = pred.predict_maps(slopes[0], t_classes=clf.predict_classes(colors[0:1])[0])
    assert np.array_equal(_bits(dist.mean), _bits(m0)) and np.array_equal(_bits(dist.stddev), _bits(s0))
    # a batch in one call equals the single calls
    mean, std = pred.predict_maps(slopes, colors=colors)
    assert mean.shape == (B, G, G) and torch.isfinite(mean).all() and (std > 0).all()
    for b in range(B):
        mb, sb = pred.predict_maps(slopes[b], colors=colors[b])
        assert np.array_equal(_bits(mean[b]), _bits(mb)) and np.array_equal(_bits(std[b]), _bits(sb)), b
        risk = infer_risk_map(mean[b], std[b], "expected_value")
        assert np.array_equal(_bits(risk), _bits(mean[b]))
        inp = io.planner_inputs(insts[b], predictions=(mean[b], std[b]))
        assert inp["risk"].shape == (G, G) and torch.isfinite(inp["risk"]).all()
