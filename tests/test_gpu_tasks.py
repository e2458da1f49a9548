"""GPU: the task stage (csrc/task_kernels.hip, benchnav_amd/tasks.py) against the NumPy spec of tests/tasks_spec.py, bit for bit:
every result is an integer or a fixed function of integers, so no comparison here has a tolerance.

  labels, sizes and statistics for both connectivities on the cases of tasks_spec.label_cases (a tile is 32 x 32: one tile, a
  one-cell last tile, a corridor that crosses tile borders thousands of times, a batch of different maps);
  the mask on values at the threshold's edge, on NaN and on inf;
  a map's outputs whether it is run alone, first or last in a batch, and over two runs;
  the sampler's cells, attempts and positions;
  the labels and `optimal_lengths` against the existing A* field (the device's, and tests/astar_oracle.py's on the CPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

import astar_oracle as AO
import tasks_spec as S

f32 = np.float32
pytestmark = pytest.mark.gpu

CASES = tuple(S.label_cases())


@functools.lru_cache(maxsize=None)
def _masks():
    cases = S.label_cases()
    for v in cases.values():
        v.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def _spec(name, connectivity):
    return S.label(_masks()[name], connectivity)


def _label(masks, connectivity):
    import torch
    from benchnav_amd import tasks as T
    labels, sizes, stats = T.label_components(torch.from_numpy(np.array(masks)).cuda(), connectivity)
    return labels.cpu().numpy(), sizes.cpu().numpy(), stats.cpu().numpy()


def _same(got, want, ctx):
    for g, w, what in zip(got, want, ("labels", "sizes", "stats")):
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape, (ctx, what, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{ctx}: {what}: {len(bad)} entries differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"


@pytest.mark.parametrize("name", CASES)
def test_labels_sizes_and_statistics_equal_the_spec(name):
    for connectivity in (4, 8):
        got, want = _label(_masks()[name], connectivity), _spec(name, connectivity)
        _same(got, want, (name, connectivity))
        print(f"\n{name} {connectivity}: stats {got[2][:, :5].tolist()}")


def test_checkerboard_is_one_component_or_all_singletons():
    l4, s4, t4 = _label(_masks()["64_checkerboard"], 4)
    l8, s8, t8 = _label(_masks()["64_checkerboard"], 8)
    assert t4[0].tolist() == [2048, 2048, 1, 0, 0, 0, 0, 0] and t8[0].tolist() == [2048, 1, 2048, 0, 0, 0, 0, 0]
    assert (l4[l4 >= 0] == np.nonzero(l4.ravel() >= 0)[0]).all() and set(l8.ravel().tolist()) == {-1, 0}


def test_mask_equals_the_spec_at_the_edges():
    import torch
    from benchnav_amd import tasks as T
    thr = 0.1
    at = f32(1.0) - f32(thr)
    edge = [0.0, 1.0, at, np.nextafter(at, f32(1)), np.nextafter(at, f32(0)), -0.5, 1.5, np.nan, np.inf, -np.inf, 0.5, 0.5, 0.5, 3e38, -3e38, 0.899]
    rng = np.random.default_rng(3)
    mean = np.concatenate([f32(edge), rng.uniform(0.7, 1.0, 33 * 35 * 2 - len(edge)).astype(f32)]).reshape(2, 33, 35)
    std = rng.uniform(0.0, 0.05, mean.shape).astype(f32)
    std[0, 0, 10:15] = [np.nan, np.inf, 0.1, 3e38, 3e38]
    for kappa in (0.0, 1.0, -2.0, 4.5, 3e38):
        got = T.passable_mask(torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda(), kappa, thr).cpu().numpy()
        want = S.passable(mean, std, kappa, thr)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (kappa, np.argwhere(got != want)[:4].tolist())
        assert 0 < want.sum() < want.size or kappa == 3e38
    # a rounded product, then a rounded sum (test_tasks_spec.py shows that a fused multiply-add would answer 0 here)
    k, s, m = f32(1.0 + 2.0 ** -12), f32(1.0 + 2.0 ** -12), f32(-1.0 - 2.0 ** -11)
    got = T.passable_mask(torch.full((1, 1, 1), float(m)).cuda(), torch.full((1, 1, 1), float(s)).cuda(), float(k), float(f32(1) - f32(2.0 ** -24)))
    assert got.cpu().numpy().tolist() == [[[1]]]


def test_a_map_is_labelled_alike_alone_first_and_last_and_twice():
    five = _masks()["batch_of_five"]
    for connectivity in (4, 8):
        want = _spec("batch_of_five", connectivity)
        for m in (0, 2, 4):
            alone = _label(five[m:m + 1], connectivity)
            first = _label(np.concatenate([five[m:m + 1], five[:m], five[m + 1:]]), connectivity)
            last = _label(np.concatenate([five[:m], five[m + 1:], five[m:m + 1]]), connectivity)
            for k in range(3):
                assert np.array_equal(alone[k][0], want[k][m]) and np.array_equal(first[k][0], want[k][m]) and np.array_equal(last[k][-1], want[k][m])
    for name in ("256_serpentine", "512_iid"):
        a, b = _label(_masks()[name], 4), _label(_masks()[name], 4)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name


# ---- the sampler -------------------------------------------------------------------------------------------------------------------
SAMPLER = dict(pairs=64, seed=0x1234567890ABCDEF, first_map=5, border=2, min_separation_sq=21 ** 2, min_component_cells=64, max_attempts=64)


@functools.lru_cache(maxsize=None)
def _sampler_maps():
    masks = np.stack([S.iid(64, 64, 20 + m) for m in range(4)])
    masks.setflags(write=False)
    return masks, S.label(masks, 4)


def _sample(labels, sizes, **kw):
    import torch
    from benchnav_amd import tasks as T
    out = T.sample_pairs(torch.from_numpy(labels).cuda(), torch.from_numpy(sizes).cuda(), **kw)
    return out["cells"].cpu().numpy(), out["attempt"].cpu().numpy(), out["positions"].cpu().numpy()


def test_sampled_pairs_equal_the_spec():
    masks, (labels, sizes, _) = _sampler_maps()
    kw = dict(SAMPLER)
    P = kw.pop("pairs")
    want = S.sample(labels, sizes, P, kw["seed"], kw["first_map"], kw["border"], kw["min_separation_sq"], kw["min_component_cells"],
                    kw["max_attempts"], x0=0.0, y0=0.0, resolution=0.5)
    # a condition on the inputs, not a tolerance: every pair of this case finds an attempt (acceptance is about 0.3 per attempt)
    assert (want[1] >= 0).all() and want[1].max() > 0, want[1].tolist()
    got = _sample(labels, sizes, pairs=P, **kw)
    for g, w, what in zip(got, want, ("cells", "attempt", "positions")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), what
    cells = got[0]
    assert (masks[np.arange(4)[:, None], cells[..., 1], cells[..., 0]] == 1).all() and (cells >= 2).all() and (cells < 62).all()
    assert ((cells[..., 2] - cells[..., 0]) ** 2 + (cells[..., 3] - cells[..., 1]) ** 2 >= 21 ** 2).all()
    # other origin and resolution: the same cells, the centres of the spec; another first_map: other draws
    got2 = _sample(labels, sizes, pairs=P, origin=(-3.0, 1.5), resolution=0.3, **kw)
    want2 = S.sample(labels, sizes, P, kw["seed"], kw["first_map"], kw["border"], kw["min_separation_sq"], kw["min_component_cells"],
                     kw["max_attempts"], x0=-3.0, y0=1.5, resolution=0.3)
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[2].view(np.uint32), want2[2].view(np.uint32))
    shifted = _sample(labels[1:], sizes[1:], pairs=P, **{**kw, "first_map": kw["first_map"] + 1})
    assert np.array_equal(shifted[0], got[0][1:]) and np.array_equal(shifted[1], got[1][1:])       # a map's pairs do not depend on its batch
    more = _sample(labels, sizes, pairs=P, **{**kw, "max_attempts": 256})
    assert np.array_equal(more[0], got[0])


def test_no_pair_where_nothing_qualifies():
    blocked = np.zeros((2, 64, 64), np.uint8)
    small = np.zeros((1, 64, 64), np.uint8)
    small[0, ::3, ::3] = 1                              # singletons
    small[0, 30:37, 30:37] = 1                          # 49 cells (and the singletons it swallows): below 64
    for masks in (blocked, small):
        labels, sizes, stats = _label(masks, 4)
        assert stats[:, 2].max() < 64
        kw = {**SAMPLER, "pairs": 8, "min_separation_sq": 0}
        cells, attempt, pos = _sample(labels, sizes, **kw)
        assert (cells == -1).all() and (attempt == -1).all() and np.isnan(pos).all()
        assert (S.sample(labels, sizes, 8, kw["seed"], kw["first_map"], 2, 0, 64, 64)[1] == -1).all()


# ---- against the A* field ----------------------------------------------------------------------------------------------------------
def _device_field(mask, goal, resolution):
    """D (H, W) float32 of the existing A* solve on zero heights with the mask as the risk, through the C ABI."""
    import torch
    from benchnav_amd import _capi
    from benchnav_amd._device import _DevArray
    lib, h = _capi.load(), C.c_void_p()
    H, W = mask.shape
    heights, risk = np.zeros((H, W), f32), np.ascontiguousarray(mask, f32)
    assert lib.bn_astar_create(0, H, W, 1, C.byref(h)) == 0
    try:
        assert lib.bn_astar_set_map(h, 0, heights.ctypes.data, risk.ctypes.data, _capi.BN_MEM_HOST, 0.5, resolution) == 0
        assert lib.bn_astar_set_goal(h, 0, goal[0], goal[1]) == 0
        assert lib.bn_astar_solve_async(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0 and lib.bn_astar_sync(h) == 0
        d, nx = C.c_void_p(), C.c_void_p()
        assert lib.bn_astar_buffers(h, 0, C.byref(d), C.byref(nx)) == 0
        return torch.as_tensor(_DevArray(d.value, (H, W)), device="cuda").cpu().numpy()
    finally:
        lib.bn_astar_destroy(h)


@pytest.mark.parametrize("name", ["64_iid", "comb"])
def test_labels_and_optimal_lengths_agree_with_the_astar_field(name):
    import torch
    from benchnav_amd import tasks as T
    mask = S.iid(64, 64, 31, blocked=0.5) if name == "64_iid" else _masks()["comb"][0]
    H, W = mask.shape
    res = 0.5
    labels8 = _label(mask[None], 8)[0][0]
    roots, counts = np.unique(labels8[labels8 >= 0], return_counts=True)
    assert len(roots) >= 2
    big, other = roots[np.argsort(-counts, kind="stable")[:2]]
    cells_of = lambda r: np.argwhere(labels8 == r)[:, ::-1]                  # (x, y)
    in_big, in_other = cells_of(big), cells_of(other)
    blocked = np.argwhere(mask == 0)[0, ::-1]
    goal = tuple(int(v) for v in in_big[len(in_big) // 2])
    D = _device_field(mask, goal, res)
    assert np.array_equal(np.isfinite(D), labels8 == labels8[goal[1], goal[0]])
    # pairs: inside the big component (the farthest and a near one), the goal itself, across components, a blocked start, no pair
    far = in_big[np.argmax(((in_big - goal) ** 2).sum(axis=1))]
    pairs = np.array([[*far, *goal], [*in_big[0], *goal], [*goal, *goal], [*in_other[0], *goal], [*blocked, *goal], [-1, -1, -1, -1],
                      [*goal, *far], [*in_other[-1], *in_other[0]]], np.int32)[None]
    got = T.optimal_lengths(torch.from_numpy(mask[None]).cuda(), torch.from_numpy(pairs).cuda(), res, chunk=3).cpu().numpy()
    assert got.dtype == f32 and got.shape == (1, 8)
    zeros, risk = np.zeros((H, W), f32), mask.astype(f32)
    for k, (sx, sy, gx, gy) in enumerate(pairs[0]):
        if sx < 0:
            assert np.isnan(got[0, k])
            continue
        want = AO.field_dijkstra(zeros, risk, 0.5, res, (int(gx), int(gy)))[sy, sx]
        assert got[0, k].view(np.uint32) == want.view(np.uint32), (k, got[0, k], want)
    assert np.isfinite(got[0, [0, 1, 6, 7]]).all() and got[0, 2] == 0.0 and np.isinf(got[0, 3]) and np.isinf(got[0, 4])
    assert got[0, 0] == D[far[1], far[0]] and got[0, 0] >= f32(res) * f32(np.abs(far - goal).max())
    assert abs(float(got[0, 6]) - float(got[0, 0])) <= 2.0 ** -18 * float(got[0, 0])      # the way back: other roundings, the same path set
