"""CPU: the RRT specification (tests/rrt_spec.py) against the trees the unmodified reference grew
(tests/golden/rrt.npz), its draws against torch's CPU generator, and the host-side checks of benchnav_amd.RRT and the C ABI.
Everything is bit-exact or a stated structural rule; no case is excluded."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import rrt_cases
import rrt_spec as S
from rrt_cases import ABOVE, DELTA, PREFIX, START
from terrain_draws_spec import Stream

CASES, META = rrt_cases.load()
f32 = np.float32


@pytest.fixture(scope="module")
def spec_trees():
    """The spec's tree of every fixture call, computed once."""
    out = {}
    for c in CASES:
        st = Stream(c.seed)
        out[c.k] = [S.plan(st, c.start, c.goal, c.iters, c.x_limits, c.y_limits, c.delta, c.rate) for _ in c.calls]
    return out


def test_fixture_holds_the_cases_the_rules_need():
    assert len(CASES) == 22 and sorted({c.seed for c in CASES[:20]}) == [0, 1, 42, 2 ** 31 - 1, 2 ** 32 - 1]
    assert any(len(c.calls) == 2 for c in CASES) and any(not c.calls[0].found for c in CASES)
    few = [r for c in CASES for r in c.calls if 2 <= len(r.goal_idx) <= 16]
    tied = [r for r in few if len(np.unique(r.costs[r.goal_idx])) < len(r.goal_idx)]
    many = [r for c in CASES for r in c.calls if len(r.goal_idx) > 16]
    assert len(few) >= 6 and len(tied) >= 1 and len(many) >= 1


@pytest.mark.parametrize("k", range(len(CASES)))
def test_spec_equals_the_reference_tree_pick_and_path(spec_trees, k):
    for ref, t in zip(CASES[k].calls, spec_trees[k]):
        rrt_cases.check_against_reference(ref, t.nodes, t.edges, t.costs, len(t.near), t.pick, t.path)
        assert np.array_equal(np.sort(ref.goal_idx), t.near)


@pytest.mark.parametrize("seed", [0, 1, 42, 2 ** 31 - 1, 2 ** 32 - 1])
def test_spec_draws_equal_torch_rand_on_a_seeded_generator(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    want = np.array([torch.rand(1, generator=g).item() for _ in range(1300)], np.float32)      # crosses two block boundaries
    st = Stream(seed)
    got = np.array([st.uniform() for _ in range(1300)], np.float32)
    assert rrt_cases.same(got, want)


def test_sample_parse_takes_one_or_three_draws():
    xy, flag = S.parse_samples(Stream(3), 500, (0.0, 9.9), (1.0, 4.0), (8.7, 3.1), 0.25)
    st = Stream(3)
    for i in range(500):
        u = st.uniform()
        assert flag[i] == (u < np.float32(0.25))
        if flag[i]:
            assert rrt_cases.same(xy[i], np.array([8.7, 3.1], np.float32))
        else:
            x, y = st.uniform() * np.float32(9.9) + np.float32(0.0), st.uniform() * np.float32(3.0) + np.float32(1.0)
            assert rrt_cases.same(xy[i], np.array([x, y], np.float32))
    assert 60 < flag.sum() < 190


def test_norm_is_the_fused_form():
    """sqrt(fma(dy, dy, f32(dx dx))) against exact rational arithmetic on random vectors; the plain sum of squares differs on some."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    v = rng.uniform(-40, 40, (4000, 2)).astype(np.float32)
    got = S.norm(v[:, 0], v[:, 1])
    inner = np.empty(len(v), np.float32)
    for i, (dx, dy) in enumerate(v):
        exact = Fraction(float(dy)) ** 2 + Fraction(float(np.float32(dx * dx)))
        lo = np.float32(float(exact))                                    # float(Fraction) rounds correctly to float64; then to
        inner[i] = lo                                                    # float32: settle the rare double rounding exactly
        for cand in (np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))):
            if abs(Fraction(float(cand)) - exact) < abs(Fraction(float(inner[i])) - exact):
                inner[i] = cand
    assert rrt_cases.same(got, np.sqrt(inner))
    plain = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(np.float32))
    assert int((rrt_cases.bits(plain) != rrt_cases.bits(got)).sum()) > 0


def test_synthetic_prefix_places_the_ties_and_the_clip_threshold():
    """The spec on the prefix alone: what the cases above are there for actually happens (test_gpu_rrt.py runs them on the device)."""
    nodes, edges, costs = S.grow(START, PREFIX, DELTA)
    assert rrt_cases.same(nodes[1], START) and costs[1] == 0 and edges[1] == 0
    assert edges[2] == 0 and edges[3] == 2 and rrt_cases.same(nodes[3], np.array([5.0, 3.0], f32)) and costs[3] == f32(8.0)
    assert S.norm(f32(5.0) - nodes[2][0], f32(3.0) - nodes[2][1]) == f32(DELTA)
    assert S.norm(nodes[2][0] - f32(2.5), nodes[2][1] - f32(7.0)) == S.norm(nodes[3][0] - f32(2.5), nodes[3][1] - f32(7.0)) and edges[4] == 2
    assert S.norm(f32(0.0), -ABOVE) > f32(DELTA) and edges[5] == 0 and costs[5] == f32(DELTA) and rrt_cases.same(nodes[5], np.array([0.0, -5.0], f32))


def test_package_exports_rrt():
    import benchnav_amd
    from benchnav_amd import RRT
    assert RRT is benchnav_amd.rrt.RRT and issubclass(RRT, torch.nn.Module)


def _map():
    return types.SimpleNamespace(resolution=0.5, x_limits=(0.0, 32.0), y_limits=(0.0, 32.0))


def test_constructor_rejects_bad_seed_and_dim_state_on_the_host():
    from benchnav_amd import RRT
    goal = torch.tensor([24.0, 24.0])
    for seed in (2 ** 32, -1, 2 ** 40 + 7):
        with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
            RRT(_map(), goal, seed=seed)
    with pytest.raises(AssertionError, match="dim_state"):
        RRT(_map(), goal, dim_state=3)
    assert S.check_seed(2 ** 32 - 1) == 2 ** 32 - 1
    with pytest.raises(ValueError):
        S.check_seed(2 ** 32)


def test_c_abi_rejects_bad_arguments_before_touching_the_device():
    from benchnav_amd import _capi
    lib = _capi.load()
    cfg = _capi.RRTConfig()
    lib.bn_rrt_config_init(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_capi.RRTConfig)
    assert (cfg.num_instances, cfg.max_iterations, cfg.delta_distance, cfg.goal_sample_rate, cfg.goal_threshold, cfg.seed) == (1, 1000, 5.0, 0.1, 0.1, 42)
    h = C.c_void_p()
    for field, value, word in (("struct_size", 4, b"struct_size"), ("num_instances", 0, b"num_instances"), ("max_iterations", 0, b"max_iterations"),
                               ("max_iterations", 2 ** 20 + 1, b"max_iterations"), ("path_cap", -1, b"path_cap"), ("seed", 2 ** 32, b"Seed"),
                               ("delta_distance", float("nan"), b"finite"), ("flags", _capi.BN_RRT_FLAG_ONE_WAVE | _capi.BN_RRT_FLAG_FOUR_WAVES, b"workgroup")):
        cfg = _capi.RRTConfig()
        lib.bn_rrt_config_init(C.byref(cfg))
        setattr(cfg, field, value)
        assert lib.bn_rrt_create(C.byref(cfg), C.byref(h)) == _capi.BN_ERR_INVALID, field
        assert word in lib.bn_rrt_last_error(), (field, lib.bn_rrt_last_error())
        assert not h.value
    assert lib.bn_rrt_create(None, C.byref(h)) == _capi.BN_ERR_INVALID
    assert lib.bn_rrt_plan_async(None, None, None, None, None) == _capi.BN_ERR_INVALID
    assert lib.bn_rrt_grow_from_samples_async(None, None, None, None, None, 0) == _capi.BN_ERR_INVALID
    assert lib.bn_rrt_sync(None) == _capi.BN_ERR_INVALID and lib.bn_rrt_node_storage(None) == -1
    p, n = C.c_void_p(), C.c_size_t()
    assert lib.bn_rrt_device_buffer(None, 0, C.byref(p), C.byref(n)) == _capi.BN_ERR_INVALID
    lib.bn_rrt_destroy(None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_gpu():
    from benchnav_amd import RRT, _capi
    lib = _capi.load()
    cfg = _capi.RRTConfig()
    lib.bn_rrt_config_init(C.byref(cfg))
    h = C.c_void_p()
    assert lib.bn_rrt_create(C.byref(cfg), C.byref(h)) == _capi.BN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.bn_rrt_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RRT(_map(), torch.tensor([24.0, 24.0]))
