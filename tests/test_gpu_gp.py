"""GPU: the exact-GP slip prediction (benchnav_amd/gp.py, csrc/gp_kernels.hip) against the float64 specification
(tests/gp_spec.py on the cases of tests/gp_cases.py), its composition over classes and maps, the permutation of a map's cells,
the reference's interface, and the hand-off to the risk map and the instance files.

Bounds: float32 outputs within 1 float32 ulp of the spec's float64 value rounded to float32 (a float64 evaluation error far below
an ulp can move a value across one rounding boundary at most); float64 outputs within 16 x the case's recorded two-formulation
spread (tests/golden/gp_slip.json), floor 64 eps relative -- gp_spec.spread's measure: the mean relative to the case's largest
|mean|, the std cell by cell."""
import warnings

import numpy as np
import pytest
import torch

import gp_cases as GC
import gp_spec as S

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G0 = 16                                                    # the 256 test slopes of a case as a 16 x 16 map


def _regressor(n, h):
    from benchnav_amd.gp import GPSlipRegressor
    x, y, c, s, l, noise, _ = GC.case(n, h)
    return GPSlipRegressor(x, y, c, s, l, noise)


def _ulps(dev: np.ndarray, want: np.ndarray) -> np.ndarray:
    """|dev - want| in float32 ulps of the larger of the two"""
    d = np.abs(dev.astype(np.float64) - want.astype(np.float64))
    return d / np.spacing(np.maximum(np.abs(dev), np.abs(want)).astype(np.float32)).astype(np.float64)


def _bits(t: torch.Tensor) -> np.ndarray:
    a = t.detach().cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("n,h", GC.CASES, ids=[GC.case_id(n, h) for n, h in GC.CASES])
def test_regressor_matches_the_float64_spec(n, h):
    _, _, c, s, l, noise, phi = GC.case(n, h)
    want_m, want_s = GC.expected(n, h)
    rec = GC.golden()["cases"][GC.case_id(n, h)]
    reg = _regressor(n, h)
    x = torch.from_numpy(phi.copy()).cuda().reshape(G0, G0)
    dist = reg.predict(x)
    m32, s32 = dist.mean, dist.stddev
    m64, s64 = reg.predict_tensors(x, dtype=torch.float64)
    assert m32.shape == s32.shape == m64.shape == (G0, G0) and m32.dtype == torch.float32 and s64.dtype == torch.float64 and m32.is_cuda
    um = _ulps(m32.cpu().numpy().reshape(-1), want_m.astype(np.float32))
    us = _ulps(s32.cpu().numpy().reshape(-1), want_s.astype(np.float32))
    ms, ss = S.spread((want_m, want_s), (m64.cpu().numpy().reshape(-1), s64.cpu().numpy().reshape(-1)))
    print(f"{GC.case_id(n, h)}: float32 ulps mean {um.max():.3g} std {us.max():.3g}; float64 spread mean {ms:.3g} std {ss:.3g} = "
          f"{ms / max(rec['mean_spread'], 4 * EPS):.3g} x / {ss / max(rec['std_spread'], 4 * EPS):.3g} x the recorded spread")
    reg.close()
    assert um.max() <= 1.0 and us.max() <= 1.0
    assert ms <= max(16 * rec["mean_spread"], 64 * EPS)
    assert ss <= max(16 * rec["std_spread"], 64 * EPS)
    # far outside the data (the slopes 1000 and -1e4 of the case): the prior, exactly
    far = np.flatnonzero(np.abs(phi) >= 1000.0)
    assert far.size == 2
    assert np.all(m64.cpu().numpy().reshape(-1)[far] == c) and np.all(s64.cpu().numpy().reshape(-1)[far] == np.sqrt(s + noise))


@pytest.fixture(scope="module")
def regs():
    """regressors of four sizes for classes 0, 1, 3 and 4 (class 2 has none)"""
    r = {0: _regressor(67, 0), 1: _regressor(130, 1), 3: _regressor(5, 2), 4: _regressor(1, 3)}
    yield r
    for v in r.values():
        v.close()


def _layouts(G, rng):
    """three class maps: (a) classes with 1, 16 and 17 cells, the rest unregressed, class 4 absent; (b) random over 0 ... 3;
    (c) class 4 with a few indices outside the table"""
    a = np.full(G * G, 2, np.int64)
    cells = rng.permutation(G * G)
    a[cells[:1]], a[cells[1:17]], a[cells[17:34]] = 0, 1, 3
    b = rng.integers(0, 4, G * G)
    c = np.full(G * G, 4, np.int64)
    c[cells[:5]] = [5, -1, 31, 32, 1000]
    return [v.reshape(G, G) for v in (a, b, c)]


@pytest.mark.parametrize("B", [1, 3])
def test_composition_equals_the_per_class_regressors_bit_for_bit(regs, B):
    from benchnav_amd.gp import TraversabilityPredictor
    G = 24
    rng = np.random.default_rng(7)
    cls = torch.from_numpy(np.stack(_layouts(G, rng)[:B]))
    slopes = torch.from_numpy(rng.uniform(-30, 30, (B, G, G)).astype(np.float32)).cuda()
    pred = TraversabilityPredictor(None, regs)
    for dtype in (torch.float32, torch.float64):
        mean, std = pred.predict_maps(slopes, t_classes=cls, dtype=dtype)
        assert mean.shape == std.shape == (B, G, G) and mean.dtype == dtype
        want_m, want_s = torch.zeros_like(mean), torch.zeros_like(std)
        for k, r in regs.items():
            mask = (cls == k).cuda()
            if mask.any():
                want_m[mask], want_s[mask] = r.predict_tensors(slopes[mask], dtype=dtype)
        assert np.array_equal(_bits(mean), _bits(want_m)) and np.array_equal(_bits(std), _bits(want_s))
        none = ~torch.isin(cls, torch.tensor(list(regs)))
        assert none.any() and not mean.cpu()[none].any() and not std.cpu()[none].any()          # exactly 0 / 0
        assert (std.cpu()[~none] > 0).all()
    single = pred.predict_maps(slopes[0], t_classes=cls[0])
    assert single[0].shape == (G, G) and np.array_equal(_bits(single[0]), _bits(pred.predict_maps(slopes, t_classes=cls)[0][0]))


def test_shuffled_cells_give_the_same_bits_permuted(regs):
    from benchnav_amd.gp import TraversabilityPredictor
    G = 24
    rng = np.random.default_rng(11)
    cls = torch.from_numpy(rng.integers(0, 5, (G, G)))
    slopes = torch.from_numpy(rng.uniform(-30, 30, (G, G)).astype(np.float32))
    slopes.view(-1)[:40] = slopes.view(-1)[0]                      # equal slopes in different tiles
    perm = torch.from_numpy(rng.permutation(G * G))
    pred = TraversabilityPredictor(None, regs)
    for dtype in (torch.float32, torch.float64):
        m, s = pred.predict_maps(slopes.cuda(), t_classes=cls, dtype=dtype)
        mp, sp = pred.predict_maps(slopes.view(-1)[perm].reshape(G, G).cuda(), t_classes=cls.view(-1)[perm].reshape(G, G), dtype=dtype)
        assert np.array_equal(_bits(m).reshape(-1)[perm.numpy()], _bits(mp).reshape(-1))
        assert np.array_equal(_bits(s).reshape(-1)[perm.numpy()], _bits(sp).reshape(-1))
        same = (cls.view(-1)[:40] == cls.view(-1)[0]).numpy()
        assert len(np.unique(_bits(s).reshape(-1)[:40][same])) == 1 and len(np.unique(_bits(m).reshape(-1)[:40][same])) == 1


class _StubClassifier:
    """the classifier's surface: predict((1, 3, G, G) colours) -> (1, G, G) classes; here the class is the red channel"""
    def __init__(self):
        self.calls = 0

    def predict(self, colors):
        self.calls += 1
        assert colors.dim() == 4 and colors.shape[0] == 1 and colors.shape[1] == 3 and colors.is_cuda
        return colors[:, 0].round().to(torch.int64)


def test_reference_interface_stream_and_repeatability(regs):
    from benchnav_amd.gp import TraversabilityPredictor
    from torch.distributions import Normal
    G = 16
    rng = np.random.default_rng(3)
    cls = torch.from_numpy(rng.choice([0, 1, 3, 4], (G, G)))
    colors = torch.stack([cls.to(torch.float32), torch.rand(G, G), torch.rand(G, G)])
    slopes = torch.from_numpy(rng.uniform(-25, 25, (G, G)).astype(np.float32))
    stub = _StubClassifier()
    pred = TraversabilityPredictor(stub, regs)
    dist = pred.predict(colors, slopes)                                   # host tensors, as the reference's predict takes them
    assert isinstance(dist, Normal) and dist.mean.shape == dist.stddev.shape == (G, G) and stub.calls == 1
    assert dist.mean.device == pred.device and dist.mean.dtype == torch.float32
    m, s = pred.predict_maps(slopes, t_classes=cls)
    assert stub.calls == 1                                                # t_classes given: the classifier is not called
    assert np.array_equal(_bits(dist.mean), _bits(m)) and np.array_equal(_bits(dist.stddev), _bits(s))
    m2, s2 = pred.predict_maps(slopes, colors=colors)
    assert stub.calls == 2 and np.array_equal(_bits(m2), _bits(m)) and np.array_equal(_bits(s2), _bits(s))     # a second call: same bits
    # on the caller's stream: the input is produced on a side stream and consumed there without a synchronisation in between
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        doubled = slopes.cuda(non_blocking=True) * 2.0
        ms, ss = pred.predict_maps(doubled * 0.5, t_classes=cls)
    side.synchronize()
    assert ms.device == pred.device and np.array_equal(_bits(ms), _bits(m)) and np.array_equal(_bits(ss), _bits(s))
    # a class without a regressor gives std 0, and Normal refuses it as it does in the reference
    cls[0, 0] = 2
    colors[0, 0, 0] = 2.0
    with pytest.raises(ValueError):
        pred.predict(colors, slopes)
    m3, s3 = pred.predict_maps(slopes, t_classes=cls)
    assert m3[0, 0].item() == 0.0 and s3[0, 0].item() == 0.0
    with pytest.raises(ValueError):
        TraversabilityPredictor(None, regs).predict_maps(slopes)          # neither classes nor a classifier


def test_end_to_end_generator_prediction_risk_map_and_instance_file(tmp_path):
    from benchnav_amd import io
    from benchnav_amd.gp import GPSlipRegressor, TraversabilityPredictor
    from benchnav_amd.risk import infer_risk_map
    from benchnav_amd.terrain import TerrainGenerator, slip_models
    G, B, C_ = 32, 2, 4
    with TerrainGenerator(G, 0.5, batch=B) as gen:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = gen.generate([4, 5], occupancy=np.full(C_, 1.0 / C_), slip_models=slip_models(C_), num_craters=1, min_radius=2, max_radius=3)
        insts = gen.to_instances()
    rng = np.random.default_rng(5)
    regs = {}
    for k in range(C_):
        x = rng.uniform(-30, 30, 40 + 13 * k).astype(np.float32)
        y = (0.4 * np.tanh(x / (8.0 + k)) + 0.05 * rng.standard_normal(x.size)).astype(np.float32)
        regs[k] = GPSlipRegressor(x, y, 0.05 * k, 0.5, 5.0 + k, 0.0025)
    pred = TraversabilityPredictor(None, regs)
    mean, std = pred.predict_maps(t.slopes, t_classes=t.t_classes)
    assert mean.shape == (B, G, G) and torch.isfinite(mean).all() and (std > 0).all()
    for b in range(B):
        risk = infer_risk_map(mean[b], std[b], "expected_value")
        assert np.array_equal(_bits(risk), _bits(mean[b]))
        inp = io.planner_inputs(insts[b], predictions=(mean[b], std[b]))
        assert inp["risk"].shape == (G, G) and torch.isfinite(inp["risk"]).all()
        insts[b].pred_mean, insts[b].pred_std = mean[b].cpu(), std[b].cpu()
        path = str(tmp_path / f"000_{b:03d}.pt")
        io.save_instance(path, insts[b])
        back = io.load_instance(path)
        assert torch.equal(back.pred_mean, mean[b].cpu()) and torch.equal(back.pred_std, std[b].cpu())
