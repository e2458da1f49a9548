"""GPU: benchnav_amd.RRT (csrc/rrt_kernels.hip) against the reference's recorded trees (tests/golden/rrt.npz) and the NumPy
specification (tests/rrt_spec.py, itself held to those trees in test_rrt_oracle.py).  No tolerance anywhere: trees, sample
tables and paths are compared bit for bit, picks by the tie rule of DESIGN.md 4.6."""
import types

import numpy as np
import pytest
import torch

import rrt_cases
import rrt_spec as S
from rrt_cases import DELTA, GOAL, START, synthetic_samples
from terrain_draws_spec import Stream

pytestmark = pytest.mark.gpu

CASES = rrt_cases.load()[0]
SEEDS = [0, 1, 42, 2 ** 31 - 1, 2 ** 32 - 1]
f32 = np.float32


def _map(x_limits=(0.0, 32.0), y_limits=(0.0, 32.0)):
    return types.SimpleNamespace(resolution=0.5, x_limits=x_limits, y_limits=y_limits)


def _planner(c, **kw):
    from benchnav_amd import RRT
    kw.setdefault("seed", c.seed)
    return RRT(_map(c.x_limits, c.y_limits), torch.tensor(c.goal), max_iterations=c.iters, delta_distance=c.delta,
               goal_sample_rate=c.rate, **kw)


def _tree_arrays(tree):
    n = tree.nodes_count
    return tree.nodes[:n].cpu().numpy(), tree.edges[:n].cpu().numpy().astype(np.int32), tree.costs[:n].cpu().numpy()


def _batch_row(pl, b, paths, lengths, found):
    nodes, edges, costs = _tree_arrays(pl.batch_tree(b))
    L = int(lengths[b])
    path = paths[b, :L].cpu().numpy() if bool(found[b]) else None
    assert (L > 0) == bool(found[b])
    if path is not None:
        assert torch.isnan(paths[b, L:]).all()
    return nodes, edges, costs, int(pl.last_batch["near_goal_counts"][b]), int(pl.last_batch["picks"][b]), path


def _same_as_spec(row, t):
    nodes, edges, costs, near, pick, path = row
    assert rrt_cases.same(nodes, t.nodes) and np.array_equal(edges, t.edges) and rrt_cases.same(costs, t.costs)
    assert near == len(t.near) and pick == t.pick
    assert (path is None) == (t.path is None) and (path is None or rrt_cases.same(path, t.path))


# ---- 1. the sample table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.25, 1.0])
def test_sample_table_matches_the_spec(rate):
    """Rate 0 takes 3000 draws per instance (four block boundaries of the stream); rate 1 takes 1000 and every sample is the goal."""
    from benchnav_amd import RRT
    goal = np.array([8.7, 9.1], f32)
    pl = RRT(_map((0.0, 9.9), (0.5, 9.9)), torch.tensor(goal), max_iterations=1000, delta_distance=1.5, goal_sample_rate=rate)
    pl.plan_batch(np.tile(np.array([[1.1, 2.3]], f32), (5, 1)), seeds=SEEDS)
    xy, flag = (v.cpu().numpy() for v in pl.sample_table())
    for b, seed in enumerate(SEEDS):
        want_xy, want_flag = S.parse_samples(Stream(seed), 1000, (0.0, 9.9), (0.5, 9.9), goal, rate)
        assert rrt_cases.same(xy[b], want_xy) and np.array_equal(flag[b], want_flag), (rate, seed)
    assert flag.all() if rate == 1.0 else (not flag.any() if rate == 0.0 else 0 < flag.sum() < flag.size)


# ---- 2. the reference's trees ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single_results():
    """forward() of every single-call fixture case as its own planner: k -> (nodes, edges, costs, near, pick, path)."""
    out = {}
    for c in CASES:
        if len(c.calls) != 1:
            continue
        pl = _planner(c)
        path = pl(torch.tensor(c.start))
        nodes, edges, costs = _tree_arrays(pl.tree)
        pick = pl._goal_node_indices[0] if pl._goal_node_indices else -1
        out[c.k] = (nodes, edges, costs, pl._near_goal_count, pick, None if path is None else path.cpu().numpy())
        assert pl.tree.nodes.shape[0] == (1000 if c.iters < 1000 else 2000) and pl.tree.edges.dtype == torch.int64
        assert torch.isinf(pl.tree.costs[c.iters + 1:]).all() and (pl.tree.edges[c.iters + 1:] == -1).all()
    return out


@pytest.mark.parametrize("k", [c.k for c in CASES if len(c.calls) == 1])
def test_single_instance_matches_the_reference(single_results, k):
    rrt_cases.check_against_reference(CASES[k].calls[0], *single_results[k])


@pytest.mark.parametrize("g", range(4))
def test_batch_of_five_is_bit_identical_to_the_singles(single_results, g):
    cs = CASES[5 * g:5 * g + 5]
    assert len({c.geometry for c in cs}) == 1 and [c.seed for c in cs] == SEEDS
    pl = _planner(cs[0])
    out = pl.plan_batch(np.stack([c.start for c in cs]), seeds=SEEDS)
    for b, c in enumerate(cs):
        row = _batch_row(pl, b, *out)
        rrt_cases.check_against_reference(c.calls[0], *row)
        for got, single in zip(row, single_results[c.k]):
            assert (got is None and single is None) or rrt_cases.same(np.asarray(got), np.asarray(single))


# ---- 3. the stream continues across calls --------------------------------------------------------------------------------
def test_second_forward_continues_the_stream():
    c = next(c for c in CASES if len(c.calls) == 2)
    pl = _planner(c)
    for ref in c.calls:
        path = pl(torch.tensor(c.start))
        nodes, edges, costs = _tree_arrays(pl.tree)
        rrt_cases.check_against_reference(ref, nodes, edges, costs, pl._near_goal_count, pl._goal_node_indices[0], path.cpu().numpy())


def test_plan_batch_twice_without_seeds_continues_every_stream():
    c = CASES[5]                                                                 # 300 iterations
    starts = np.stack([c.start, c.start + f32(0.5), c.start + f32(1.25)])
    pl = _planner(c, seed=11)
    streams = [Stream(11) for _ in range(3)]                                     # no seeds at all: each instance starts from the constructor's
    for _ in range(2):
        out = pl.plan_batch(starts)
        for b in range(3):
            _same_as_spec(_batch_row(pl, b, *out), S.plan(streams[b], starts[b], c.goal, c.iters, c.x_limits, c.y_limits, c.delta, c.rate))
    pl2 = _planner(c, seed=11)
    streams = [Stream(s) for s in (3, 4, 2 ** 32 - 1)]
    for seeds in ([3, 4, 2 ** 32 - 1], None):                                    # seeded, then continued
        out = pl2.plan_batch(starts, seeds=seeds)
        for b in range(3):
            _same_as_spec(_batch_row(pl2, b, *out), S.plan(streams[b], starts[b], c.goal, c.iters, c.x_limits, c.y_limits, c.delta, c.rate))


# ---- 4. caller-supplied samples -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("workgroup", [64, 256])
@pytest.mark.parametrize("iters", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_grow_from_samples_matches_the_spec(iters, workgroup):
    from benchnav_amd import RRT
    rng = np.random.default_rng(iters)
    samples = np.stack([synthetic_samples(iters, v, rng) for v in range(3)])
    pl = RRT(_map(), torch.tensor(GOAL), max_iterations=iters, delta_distance=DELTA, workgroup=workgroup)
    starts = np.tile(START, (3, 1))
    want = [S.plan_from_samples(START, GOAL, samples[b], DELTA) for b in range(3)]
    for where in ("host", "device"):
        out = pl.grow_from_samples(starts, torch.from_numpy(samples).cuda() if where == "device" else samples)
        for b in range(3):
            _same_as_spec(_batch_row(pl, b, *out), want[b])


# ---- 5. where the nodes live ------------------------------------------------------------------------------------------------
def test_global_memory_nodes_equal_lds_nodes_bit_for_bit():
    c = CASES[7]                                                                 # 300 iterations, seed 42
    rows = []
    for storage, workgroup in (("lds", 64), ("global", 64), ("lds", 256), ("global", 256)):
        pl = _planner(c, node_storage=storage, workgroup=workgroup)
        assert pl.node_storage().startswith(storage)
        path = pl(torch.tensor(c.start))
        rows.append(_tree_arrays(pl.tree) + (pl._near_goal_count, pl._goal_node_indices[0], path.cpu().numpy()))
        rrt_cases.check_against_reference(c.calls[0], *rows[-1])
    for r in rows[1:]:
        assert all(rrt_cases.same(np.asarray(a), np.asarray(b)) for a, b in zip(r, rows[0]))


@pytest.fixture(scope="module")
def long_spec():
    """The spec's 8192-iteration plan, grown once: a shorter plan of the same seed is its prefix (the samples do not depend on the tree)."""
    start, goal = np.array([5.0, 5.0], f32), np.array([120.0, 120.0], f32)
    xy, _ = S.parse_samples(Stream(9), 8192, (0.0, 128.0), (0.0, 128.0), goal, 0.1)
    return start, goal, xy, S.grow(start, xy, 5)


@pytest.mark.parametrize("iters,storage,workgroup", [(5460, "lds+costs", None), (5461, "lds", None), (8191, "lds", 64), (8191, "lds", 256),
                                                     (8192, "global", None)])
def test_storage_thresholds_match_the_spec(long_spec, iters, storage, workgroup):
    """Every size at which the growth kernel changes where it keeps the tree: costs leave LDS above 5461 nodes, nodes above 8192
    (8191 iterations, where the 256-thread kernel's LDS is 64 KB and 32 bytes).  One plan each, against the spec."""
    from benchnav_amd import RRT
    start, goal, _, (nodes_, edges_, costs_) = long_spec
    pl = RRT(_map((0.0, 128.0), (0.0, 128.0)), torch.tensor(goal), max_iterations=iters, delta_distance=5, seed=9, workgroup=workgroup)
    assert pl.node_storage() == storage
    path = pl(torch.tensor(start))
    n = iters + 1
    near, pick, want_path = S.goal_pick(nodes_[:n], edges_[:n], costs_[:n], goal)
    t = S.SpecTree(nodes_[:n], edges_[:n], costs_[:n], near, pick, want_path)
    nodes, edges, costs = _tree_arrays(pl.tree)
    _same_as_spec((nodes, edges, costs, pl._near_goal_count, pl._goal_node_indices[0] if pl._goal_node_indices else -1,
                   None if path is None else path.cpu().numpy()), t)
    assert pl.tree.nodes.shape[0] == (8000 if iters < 8000 else 16000)


# ---- 6. errors and results --------------------------------------------------------------------------------------------------
def test_no_path_returns_none():
    c = next(c for c in CASES if not c.calls[0].found)
    pl = _planner(c)
    assert pl(torch.tensor(c.start)) is None and pl._goal_node_indices == [] and pl.tree.nodes_count == c.iters + 1
    paths, lengths, found = pl.plan_batch(np.stack([c.start, c.start]), seeds=[c.seed, c.seed])
    assert not found.any() and (lengths == 0).all() and torch.isnan(paths).all()


def test_out_of_bounds_raises_without_a_launch():
    from benchnav_amd import RRT
    pl = RRT(_map(), torch.tensor([24.0, 24.0]), max_iterations=16)
    for bad in ([-0.1, 8.0], [8.0, 32.5], [float("nan"), 1.0]):
        with pytest.raises(ValueError, match="Start or goal position is out of bounds."):
            pl(torch.tensor(bad))
        with pytest.raises(ValueError, match="out of bounds"):
            pl.plan_batch(np.array([[8.0, 8.0], bad], f32))
    assert pl.tree is None and not pl._handles                                  # nothing was created, let alone launched
    far = RRT(_map(), torch.tensor([40.0, 24.0]), max_iterations=16)
    with pytest.raises(ValueError, match="out of bounds"):
        far(torch.tensor([8.0, 8.0, 0.3]))
    pl(torch.tensor([0.0, 32.0, 1.0]))                                          # the limits themselves are inside (rrt.py:143-145)
    assert pl.tree.nodes_count == 17


def test_c_abi_rejects_out_of_bounds_and_wide_seeds():
    import ctypes as C
    from benchnav_amd import _capi
    lib = _capi.load()
    cfg = _capi.RRTConfig()
    lib.bn_rrt_config_init(C.byref(cfg))
    cfg.max_iterations, cfg.num_instances = 8, 2
    h = C.c_void_p()
    assert lib.bn_rrt_create(C.byref(cfg), C.byref(h)) == _capi.BN_OK
    try:
        ok, bad = np.array([[8, 8], [9, 9]], f32), np.array([[8, 8], [33, 9]], f32)
        seeds, wide = np.array([1, 2], np.uint64), np.array([1, 2 ** 32], np.uint64)
        assert lib.bn_rrt_plan_async(h, None, bad.ctypes.data, ok.ctypes.data, seeds.ctypes.data) == _capi.BN_ERR_INVALID
        assert b"out of bounds" in lib.bn_rrt_last_error()
        assert lib.bn_rrt_plan_async(h, None, ok.ctypes.data, bad.ctypes.data, None) == _capi.BN_ERR_INVALID
        assert lib.bn_rrt_plan_async(h, None, ok.ctypes.data, ok.ctypes.data, wide.ctypes.data) == _capi.BN_ERR_INVALID
        assert b"Seed" in lib.bn_rrt_last_error()
        p, n = C.c_void_p(), C.c_size_t()
        assert lib.bn_rrt_device_buffer(h, 99, C.byref(p), C.byref(n)) == _capi.BN_ERR_INVALID
        assert lib.bn_rrt_plan_async(h, None, ok.ctypes.data, ok.ctypes.data, seeds.ctypes.data) == _capi.BN_OK
        assert lib.bn_rrt_sync(h) == _capi.BN_OK
        assert lib.bn_rrt_device_buffer(h, _capi.BN_RRT_BUF_NODES, C.byref(p), C.byref(n)) == _capi.BN_OK and n.value == 2 * 9 * 8
    finally:
        lib.bn_rrt_destroy(h)


def test_rejected_constructor_arguments():
    from benchnav_amd import RRT
    with pytest.raises(ValueError, match="Seed"):
        RRT(_map(), torch.tensor([24.0, 24.0]), seed=2 ** 32)
    with pytest.raises(AssertionError, match="dim_state"):
        RRT(_map(), torch.tensor([24.0, 24.0]), dim_state=3)
    pl = RRT(_map(), torch.tensor([24.0, 24.0]), max_iterations=16)
    with pytest.raises(ValueError, match="Seed"):
        pl.plan_batch(np.array([[8, 8]], f32), seeds=[2 ** 32])


def test_global_generators_are_left_alone():
    from benchnav_amd import RRT
    torch.manual_seed(123)
    np.random.seed(123)
    want_t, want_n = torch.rand(3), np.random.rand(3)
    torch.manual_seed(123)
    np.random.seed(123)
    RRT(_map(), torch.tensor([24.0, 24.0]), max_iterations=64, seed=5)(torch.tensor([8.0, 8.0]))
    assert torch.equal(torch.rand(3), want_t) and np.array_equal(np.random.rand(3), want_n)


# ---- 7. the path feeds DWA ---------------------------------------------------------------------------------------------------
def test_path_goes_into_dwa_update_reference_path_unchanged():
    from benchnav_amd.dwa import DWA
    c = CASES[15]
    path = _planner(c)(torch.tensor(c.start))
    d = DWA.__new__(DWA)
    torch.nn.Module.__init__(d)
    d._dtype, d._device = torch.float32, path.device
    d.update_reference_path(path)
    assert d.reference_path.shape == (len(c.calls[0].path), 2) and d.reference_path.dtype == torch.float32
    assert rrt_cases.same(d.reference_path.numpy(), c.calls[0].path) and torch.equal(d._path_dev.cpu(), d.reference_path)
