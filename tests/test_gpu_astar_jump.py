"""GPU: the A* jump tables (bn_astar_jump_build_async, csrc/astar_kernels.hip) against the numpy doubling over the device's own
next-hop map; batched device paths (bn_astar_paths_async, AStar.paths) against bn_astar_path and astar_oracle.walk; staleness;
and a corrupt map, which the build reports and does not follow."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import astar_jump_oracle as J
import astar_maps as M
import astar_oracle as O

pytestmark = pytest.mark.gpu


def _dev(ptr, shape, typestr):
    """Library-owned device memory as a torch tensor (no copy)."""
    from benchnav_amd.astar import _DevArray
    return torch.as_tensor(_DevArray(ptr, shape, typestr=typestr), device="cuda")


def _planner(case):
    """benchnav_amd.AStar over one (heights, risk, thr, res, goal cell)."""
    from benchnav_amd import AStar
    h, r, thr, res, goal = case
    H, W = h.shape
    gm = types.SimpleNamespace(tensors={"heights": torch.from_numpy(h).cuda()}, resolution=res, x_limits=(0.0, W * res), y_limits=(0.0, H * res))
    dyn = types.SimpleNamespace(_traversability_model=types.SimpleNamespace(_risks=torch.from_numpy(np.asarray(r, np.float32)).cuda()))
    return AStar(gm, torch.tensor([(goal[0] + 0.5) * res, (goal[1] + 0.5) * res]), dyn, thr, device="cuda")


def _handle(lib, cases):
    """A solved C-ABI handle with one instance per case (all of one shape and resolution)."""
    from benchnav_amd import _capi
    H, W = cases[0][0].shape
    a = C.c_void_p()
    assert lib.bn_astar_create(0, H, W, len(cases), C.byref(a)) == 0
    for b, (h, r, thr, res, goal) in enumerate(cases):
        h, r = np.ascontiguousarray(h, np.float32), np.ascontiguousarray(r, np.float32)
        assert lib.bn_astar_set_map(a, b, C.c_void_p(h.ctypes.data), C.c_void_p(r.ctypes.data), _capi.BN_MEM_HOST, thr, res) == 0
        assert lib.bn_astar_set_goal(a, b, goal[0], goal[1]) == 0
    assert lib.bn_astar_solve_async(a, None) == 0
    return a


def _next(lib, a, inst, H, W):
    d, nx = C.c_void_p(), C.c_void_p()
    assert lib.bn_astar_sync(a) == 0, lib.bn_astar_last_error()
    assert lib.bn_astar_buffers(a, inst, C.byref(d), C.byref(nx)) == 0
    return _dev(nx.value, (H, W), "|u1")


def _tables(lib, a, inst, H, W):
    hp, jp, lv, eb = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
    assert lib.bn_astar_sync(a) == 0, lib.bn_astar_last_error()
    assert lib.bn_astar_jump_buffers(a, inst, C.byref(hp), C.byref(jp), C.byref(lv), C.byref(eb)) == 0
    assert eb.value == 4
    return _dev(hp.value, (H, W), "<i4").cpu().numpy(), _dev(jp.value, (lv.value, H * W), "<i4").cpu().numpy()


def _paths(lib, a, inst, starts, max_len, where="device"):
    """(nodes (n, max_len, 2), lengths (n)) of bn_astar_paths_async, as numpy."""
    from benchnav_amd import _capi
    starts = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
    n = len(starts)
    out = torch.full((n, max_len, 2), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    if where == "device":
        sd = torch.from_numpy(starts).cuda()
        rc = lib.bn_astar_paths_async(a, inst, C.c_void_p(sd.data_ptr()), _capi.BN_MEM_DEVICE, n, max_len, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(lens.data_ptr()), None)
    else:
        rc = lib.bn_astar_paths_async(a, inst, C.c_void_p(starts.ctypes.data), _capi.BN_MEM_HOST, n, max_len, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(lens.data_ptr()), None)
    assert rc == 0, lib.bn_astar_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy()


def _host_path(lib, a, inst, ix, iy, cap):
    buf = np.full((cap, 2), -1, np.int32)
    n = lib.bn_astar_path(a, inst, int(ix), int(iy), buf.ctypes.data_as(C.POINTER(C.c_int32)), cap)
    assert n >= 0, lib.bn_astar_last_error()
    return n, buf


def _edge_goal(H, W):
    """A goal of astar_maps.shape_goals on a tile edge (x or y in 31 / 32) where the shape has one, else the last of its goals."""
    goals = M.shape_goals(H, W)
    edge = [g for g in goals if g[0] in (31, 32) or g[1] in (31, 32)]
    return edge[0] if edge else goals[-1]


def _table_cases():
    out = {}
    for H, W in ((1, 1), (1, 97), (2, 33), (33, 33), (63, 95)):
        h, r, thr, res, _ = M.shapes(H, W)
        out[f"shape{H}x{W}"] = (h, r, thr, res, _edge_goal(H, W))
    out["spiral48"] = M.spiral(48)
    out["zipper"] = M.zipper()
    out["walled_off"] = J.walled_off()
    h, r, thr, res, g = M.shapes(33, 33)
    r = r.copy()
    r[20, 9] = M.BLOCKED
    out["goal_collision"] = (h, r, thr, res, (9, 20))
    out["goal_out_of_bounds"] = (h, r, thr, res, (40, 3))
    return out


TABLE_CASES = _table_cases()


# ---- 1. the tables against numpy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_tables_equal_the_numpy_doubling(name):
    case = TABLE_CASES[name]
    H, W = case[0].shape
    pl = _planner(case)
    _, nxt = pl.field()
    nxt = nxt.cpu().numpy()
    pl.build_jump_tables()
    hops, jump = _tables(pl._lib, pl._handle, 0, H, W)
    want_hops, want_jump = J.jump_tables(nxt)
    assert jump.shape == want_jump.shape == (J.num_levels(H * W), H * W)
    assert np.array_equal(hops, want_hops)
    for k in range(len(jump)):
        assert np.array_equal(jump[k], want_jump[k]), (name, k)
    got = pl.hop_counts()
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (H, W) and np.array_equal(got.cpu().numpy(), hops)
    if name == "spiral48":                         # 11 live levels; walks cross 1024 hops
        _, cpu_next = O.solve(*case)
        assert O.hop_counts(cpu_next).max() == 1150 and hops.max() == 1150
    if name == "walled_off":
        assert (hops >= 0).any() and (hops < 0).any()
    if name in ("goal_collision", "goal_out_of_bounds"):
        assert (hops == -1).all()
    pl.close()


# ---- 2. paths ------------------------------------------------------------------------------------------------------------
def _paths_cases():
    h, r, thr, res, _ = M.shapes(33, 33)
    return {"shape33x33": (h, r, thr, res, _edge_goal(33, 33)), "spiral24": M.spiral(24)}


@pytest.mark.parametrize("name", ["shape33x33", "spiral24"])
def test_paths_for_every_cell_equal_the_host_walk(name):
    from benchnav_amd import _capi
    lib = _capi.load()
    case = _paths_cases()[name]
    H, W = case[0].shape
    a = _handle(lib, [case])
    assert lib.bn_astar_jump_build_async(a, None) == 0
    nxt = _next(lib, a, 0, H, W).cpu().numpy()
    starts = np.stack([np.arange(H * W) % W, np.arange(H * W) // W], axis=1).astype(np.int32)
    assert len(starts) == {"shape33x33": 1089, "spiral24": 576}[name]
    ref = [_host_path(lib, a, 0, x, y, H * W) for x, y in starts]
    longest = max(n for n, _ in ref)
    cap = longest + 3
    nodes, lens = _paths(lib, a, 0, starts, cap)
    assert np.array_equal(lens, [n for n, _ in ref])
    for i, (n, buf) in enumerate(ref):
        assert np.array_equal(nodes[i, :n], buf[:n]), i
        assert (nodes[i, n:] == -1).all(), i
        walk = O.walk(nxt, tuple(starts[i]))
        assert (walk is None and n == 0) or np.array_equal(nodes[i, :n], np.asarray(walk)), i
    # truncation: the first 5 nodes, the full count
    short, lens5 = _paths(lib, a, 0, starts, 5)
    assert np.array_equal(lens5, lens) and np.array_equal(short, nodes[:, :5])
    # N = 1, N = 0, starts out of bounds, host starts
    far = int(np.argmax(lens))
    one, len1 = _paths(lib, a, 0, starts[far:far + 1], cap)
    assert len1[0] == longest and np.array_equal(one[0], nodes[far])
    assert lib.bn_astar_paths_async(a, 0, None, _capi.BN_MEM_DEVICE, 0, cap, None, None, None) == 0
    mixed = np.array([[-1, 0], starts[far], [W, 0], [0, H], [0, -3], starts[0]], np.int32)
    got, lenm = _paths(lib, a, 0, mixed, cap)
    assert lenm.tolist() == [-1, longest, -1, -1, -1, int(lens[0])]
    assert (got[[0, 2, 3, 4]] == -1).all() and np.array_equal(got[1], nodes[far]) and np.array_equal(got[5], nodes[0])
    host, lenh = _paths(lib, a, 0, mixed, cap, where="host")
    assert np.array_equal(host, got) and np.array_equal(lenh, lenm)
    lib.bn_astar_destroy(a)


def test_paths_answer_per_instance():
    from benchnav_amd import _capi
    lib = _capi.load()
    cases = []
    for k, goal in enumerate(((31, 16), (2, 30), (16, 0))):
        h, r, thr, res, _ = M.shapes(33, 33, seed=40 + k)
        r = r.copy()
        M._free_goal(r, goal)
        cases.append((h, r, thr, res, goal))
    a = _handle(lib, cases)
    assert lib.bn_astar_jump_build_async(a, None) == 0
    starts = np.stack([np.arange(0, 1089, 7) % 33, np.arange(0, 1089, 7) // 33], axis=1).astype(np.int32)
    seen = []
    for b in range(3):
        nxt = _next(lib, a, b, 33, 33).cpu().numpy()
        hops, jump = _tables(lib, a, b, 33, 33)
        want_hops, want_jump = J.jump_tables(nxt)
        assert np.array_equal(hops, want_hops) and np.array_equal(jump, want_jump), b
        nodes, lens = _paths(lib, a, b, starts, 80)
        for i, (x, y) in enumerate(starts):
            n, buf = _host_path(lib, a, b, x, y, 80)
            assert lens[i] == n and np.array_equal(nodes[i, :min(n, 80)], buf[:min(n, 80)]), (b, i)
            if 0 < n <= 80:
                assert tuple(int(v) for v in nodes[i, n - 1]) == cases[b][4], (b, i)
        seen.append(lens)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    lib.bn_astar_destroy(a)


def test_class_paths_equal_forward():
    case = J.walled_off()
    h, r, thr, res, goal = case
    pl = _planner(case)
    cells = [(3, 3), (50, 35), (14, 17), (9, 11), (19, 23), (8, 10), (20, 24), (goal[0], goal[1]), (55, 0), (0, 39), (30, 20), (12, 12)]
    states = torch.tensor([[(x + 0.25) * res, (y + 0.75) * res, 0.3] for x, y in cells], dtype=torch.float32)
    fwd = [pl.forward(s.cuda()) for s in states]
    assert any(p is None for p in fwd) and any(p is not None for p in fwd)
    for st in (states, states.cuda(), states[:, :2].cuda()):
        points, lengths = pl.paths(st)
        assert points.is_cuda and lengths.is_cuda and lengths.dtype == torch.int32
        assert points.shape == (len(cells), int(lengths.max()), 2)
        for i, p in enumerate(fwd):
            n = int(lengths[i])
            assert n == (0 if p is None else p.shape[0]), i
            if p is not None:
                assert points.dtype == p.dtype and torch.equal(points[i, :n], p), i
            assert torch.isnan(points[i, n:]).all(), i
    points, lengths = pl.paths(states, max_len=4)
    assert points.shape == (len(cells), 4, 2) and int(lengths.max()) > 4
    assert torch.equal(points[0], fwd[0][:4])
    empty, none = pl.paths(torch.zeros(0, 3))
    assert empty.shape == (0, 0, 2) and none.shape == (0,)
    bad = states.clone()
    bad[5, 0] = 56 * res
    with pytest.raises(ValueError, match=r"Start or goal position is out of bounds\..*5"):
        pl.paths(bad)
    with pytest.raises(ValueError, match="Start or goal position is out of bounds."):
        pl.forward(bad[5])
    pl.close()
    blocked = (h, np.where(np.arange(56)[None, :] == goal[0], M.BLOCKED, r).astype(np.float32), thr, res, goal)
    pl = _planner(blocked)
    with pytest.raises(ValueError, match="Goal position is not traversable."):
        pl.paths(states)
    pl.close()


# ---- 3. staleness --------------------------------------------------------------------------------------------------------
def test_stale_tables_are_refused_until_rebuilt():
    from benchnav_amd import _capi
    import test_gpu_astar_dwa as T
    lib = _capi.load()
    heights, risk, start, goal, kw = T._case("smooth")
    z = torch.from_numpy(np.random.default_rng(2).standard_normal((6, 1)).astype(np.float32)).cuda()
    runs = {}
    for walk in ("jump", "serial"):
        pl, env = T._env(1, risk, start, goal)
        loop = T._loop(env, heights, risk, walk=walk)
        env.reset()
        a = loop._astar
        G = T.G
        starts = np.array([[10, 12], [40, 50], [63, 0]], np.int32)
        if walk == "jump":
            before = _paths(lib, a, 0, starts, 200)
        new_goal = (20, 44)
        assert risk[new_goal[1], new_goal[0]] > T.THR
        assert lib.bn_astar_set_goal(a, 0, *new_goal) == 0
        assert lib.bn_astar_solve_async(a, None) == 0
        if walk == "jump":
            out = torch.empty((3, 200, 2), dtype=torch.int32, device="cuda")
            lens = torch.empty(3, dtype=torch.int32, device="cuda")
            sd = torch.from_numpy(starts).cuda()
            rc = lib.bn_astar_paths_async(a, 0, C.c_void_p(sd.data_ptr()), _capi.BN_MEM_DEVICE, 3, 200, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(lens.data_ptr()), None)
            assert rc == _capi.BN_ERR_STATE and b"stale" in lib.bn_astar_last_error()
            with pytest.raises(_capi.BenchnavError) as e:
                loop.run(6, z=z)
            assert e.value.code == _capi.BN_ERR_STATE and "jump tables" in str(e.value)
            assert env._steps == 0                                   # nothing ran
            assert lib.bn_astar_jump_build_async(a, None) == 0
            after = _paths(lib, a, 0, starts, 200)
            for i, (x, y) in enumerate(starts):
                n, buf = _host_path(lib, a, 0, x, y, 200)
                assert after[1][i] == n > 0 and np.array_equal(after[0][i, :n], buf[:n]) and tuple(buf[n - 1]) == new_goal
            assert not np.array_equal(after[0], before[0])
        runs[walk] = loop.run(6, z=z)
    for got, want in zip(runs["jump"], runs["serial"]):
        assert T._eq(got, want)


# ---- 4. a corrupt map is reported and not followed -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cycle", "code"])
def test_corrupt_next_is_reported(kind):
    from benchnav_amd import _capi
    lib = _capi.load()
    h, r, thr, res, _ = M.shapes(33, 33)
    r = np.full_like(r, M.FREE)
    a = _handle(lib, [(h, r, thr, res, (31, 16))])
    nxt = _next(lib, a, 0, 33, 33)
    if kind == "cycle":                            # (5, 7) -> (6, 7) -> (5, 7): direction 1 is +x, direction 0 is -x
        nxt[7, 5] = 1
        nxt[7, 6] = 0
    else:
        nxt[7, 5] = 77
    torch.cuda.synchronize()
    rc = lib.bn_astar_jump_build_async(a, None)
    if rc == 0:
        rc = lib.bn_astar_sync(a)
    assert rc == _capi.BN_ERR_STATE
    msg = lib.bn_astar_last_error()
    assert (b"cycle" if kind == "cycle" else b"unknown code") in msg and b"next-hop map" in msg
    if kind == "code":
        assert b"cell (5, 7)" in msg
    sd = torch.tensor([[5, 7]], dtype=torch.int32, device="cuda")
    out = torch.empty((1, 8, 2), dtype=torch.int32, device="cuda")
    lens = torch.empty(1, dtype=torch.int32, device="cuda")
    assert lib.bn_astar_paths_async(a, 0, C.c_void_p(sd.data_ptr()), _capi.BN_MEM_DEVICE, 1, 8, C.c_void_p(out.data_ptr()),
                                    C.c_void_p(lens.data_ptr()), None) == _capi.BN_ERR_STATE
    hops, _ = _tables_unchecked(lib, a, 33, 33)
    assert hops[7, 5] == -1                        # neither a count nor a walk that never ends
    # a fresh solve and build: the handle works again
    assert lib.bn_astar_solve_async(a, None) == 0
    assert lib.bn_astar_jump_build_async(a, None) == 0
    assert lib.bn_astar_sync(a) == 0, lib.bn_astar_last_error()
    nodes, lens = _paths(lib, a, 0, [[5, 7]], 64)
    n, buf = _host_path(lib, a, 0, 5, 7, 64)
    assert lens[0] == n > 1 and np.array_equal(nodes[0, :n], buf[:n])
    lib.bn_astar_destroy(a)


def _tables_unchecked(lib, a, H, W):
    hp, jp, lv, eb = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
    assert lib.bn_astar_jump_buffers(a, 0, C.byref(hp), C.byref(jp), C.byref(lv), C.byref(eb)) == 0
    torch.cuda.synchronize()
    return _dev(hp.value, (H, W), "<i4").cpu().numpy(), _dev(jp.value, (lv.value, H * W), "<i4").cpu().numpy()
