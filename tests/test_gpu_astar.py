"""GPU: the A* global planner (benchnav_amd.AStar, csrc/astar_kernels.hip) against the CPU oracle (bit for bit) and the
reference's own forward() outcomes (tests/golden/astar.npz)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import astar_oracle as A
from helpers import FakeDynamics, FakeGridMap, FakeObjectives

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = A.load_fixtures(os.path.join(HERE, "golden", "astar.npz"))


def _goal(fx):
    return A.pos_to_index(fx["goal_pos"], fx["x0"], fx["y0"], fx["res"])


def _planner(fx):
    from benchnav_amd import AStar
    H, W = fx["heights"].shape
    gm = FakeGridMap(W, fx["res"], x_limits=(fx["x0"], fx["x0"] + W * fx["res"]), y_limits=(fx["y0"], fx["y0"] + H * fx["res"]))
    gm.tensors = {"heights": torch.from_numpy(fx["heights"]).cuda()}
    dyn = FakeDynamics(torch.from_numpy(fx["risk"]).cuda(), gm)
    return AStar(gm, torch.from_numpy(fx["goal_pos"]), dyn, fx["thr"], device="cuda")


def _forward(planner, s):
    try:
        p = planner.forward(torch.tensor([s[0], s[1], 0.3], dtype=torch.float32, device="cuda"))
    except ValueError as e:
        return "error", str(e)
    if p is None:
        return "none", None
    assert p.dtype == torch.float32 and p.is_cuda and p.shape[1] == 2
    idx = torch.round(p.cpu() / planner.resolution).to(torch.int64)
    assert torch.equal(idx * planner.resolution, p.cpu())
    return "path", [tuple(int(v) for v in n) for n in idx]


_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        fx = FIX[name]
        _ORACLE[name] = A.solve(fx["heights"], fx["risk"], fx["thr"], fx["res"], _goal(fx))
    return _ORACLE[name]


@pytest.mark.parametrize("name", sorted(FIX))
def test_field_and_next_bit_exact_vs_oracle(name):
    pl = _planner(FIX[name])
    D, nxt = pl.field()
    D0, n0 = _oracle(name)
    assert np.array_equal(D.cpu().numpy().view(np.uint32), D0.view(np.uint32)), f"{name}: D differs in {(D.cpu().numpy() != D0).sum()} cells"
    assert np.array_equal(nxt.cpu().numpy(), n0), f"{name}: next differs in {(nxt.cpu().numpy() != n0).sum()} cells"


@pytest.mark.parametrize("name", sorted(FIX))
def test_forward_equals_oracle_walk_and_meets_reference(name):
    fx = FIX[name]
    pl = _planner(fx)
    got = [_forward(pl, s) for s in fx["starts"]]
    want = [A.forward_like(fx, _oracle(name), s) for s in fx["starts"]]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and (g[1] == w[1] if g[0] != "path" else g[1] == [tuple(n) for n in w[1]]), (name, i, g, w)
    identical, tied, cheaper, fails = A.census(fx, got)
    print(f"{name}: {identical} identical to the reference's path, {tied} equal-cost, {cheaper} cheaper than the reference's")
    assert not fails, fails


def _handle(H, W, B):
    from benchnav_amd import _capi
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.bn_astar_create(0, H, W, B, C.byref(h)) == 0, lib.bn_astar_last_error()
    return lib, h


def _read(lib, h, inst, H, W):
    from benchnav_amd.astar import _DevArray
    assert lib.bn_astar_sync(h) == 0, lib.bn_astar_last_error()
    d, n = C.c_void_p(), C.c_void_p()
    assert lib.bn_astar_buffers(h, inst, C.byref(d), C.byref(n)) == 0
    D = torch.as_tensor(_DevArray(d.value, (H, W)), device="cuda").cpu().numpy().copy()
    N = torch.as_tensor(_DevArray(n.value, (H, W), typestr="|u1"), device="cuda").cpu().numpy().copy()
    return D, N


def _set(lib, h, inst, fx, goal):
    hp, rp = np.ascontiguousarray(fx["heights"]), np.ascontiguousarray(fx["risk"])
    assert lib.bn_astar_set_map(h, inst, hp.ctypes.data, rp.ctypes.data, 0, fx["thr"], fx["res"]) == 0, lib.bn_astar_last_error()
    assert lib.bn_astar_set_goal(h, inst, *goal) == 0


def test_two_solves_are_identical():
    fx = FIX["iid256"]
    H, W = fx["heights"].shape
    lib, h = _handle(H, W, 1)
    try:
        _set(lib, h, 0, fx, _goal(fx))
        outs = []
        for _ in range(2):
            assert lib.bn_astar_solve_async(h, None) == 0
            outs.append(_read(lib, h, 0, H, W))
        assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1], outs[1][1])
        buf = (C.c_int32 * 2)()
        assert lib.bn_astar_path(h, 0, W, 0, buf, 1) < 0            # a start out of bounds is an error, not a path
    finally:
        lib.bn_astar_destroy(h)


def test_batch_of_eight_equals_eight_single_solves():
    fx = FIX["smooth256"]
    H, W = fx["heights"].shape
    free = A.free_mask(fx["risk"], fx["thr"])
    rng = np.random.default_rng(3)
    fy, fx_ = np.nonzero(free)
    goals = [(int(fx_[j]), int(fy[j])) for j in rng.choice(len(fx_), 6, replace=False)]
    cy, cx = np.nonzero(~free)
    goals += [(int(cx[0]), int(cy[0])), (W + 3, 1)]                  # a goal in collision, a goal out of bounds
    lib, h = _handle(H, W, 8)
    try:
        for b, g in enumerate(goals):
            _set(lib, h, b, fx, g)
        assert lib.bn_astar_solve_async(h, None) == 0
        batched = [_read(lib, h, b, H, W) for b in range(8)]
    finally:
        lib.bn_astar_destroy(h)
    for b, g in enumerate(goals):
        lib, h = _handle(H, W, 1)
        try:
            _set(lib, h, 0, fx, g)
            assert lib.bn_astar_solve_async(h, None) == 0
            D, N = _read(lib, h, 0, H, W)
        finally:
            lib.bn_astar_destroy(h)
        assert np.array_equal(batched[b][0].view(np.uint32), D.view(np.uint32)) and np.array_equal(batched[b][1], N), b
    assert np.isinf(batched[6][0]).all() and (batched[7][1] == A.NEXT_NONE).all()


def test_collision_is_risk_at_or_below_threshold():
    """astar.py:182-192 reads `risk <= stuck_threshold` as a collision (low risk blocks).  A wall of risk == threshold blocks,
    the one NaN cell in it does not: the path crosses the wall there and only there."""
    risk = np.full((8, 16), 0.9, np.float32)
    risk[:, 8] = np.float32(0.25)
    risk[7, 8] = np.nan
    fx = dict(heights=np.zeros_like(risk), risk=risk, thr=0.25, res=0.5, x0=0.0, y0=0.0,
              goal_pos=np.array([6.75, 0.25], np.float32))
    pl = _planner(fx)
    kind, p = _forward(pl, np.array([1.25, 0.25], np.float32))
    assert kind == "path" and p[0] == (2, 0) and p[-1] == (13, 0)
    assert [n for n in p if n[0] == 8] == [(8, 7)]
    assert p == A.walk(A.solve(fx["heights"], risk, 0.25, 0.5, (13, 0))[1], (2, 0))


def test_astar_dwa_loop_matches_oracle_every_step():
    """test_astar_dwa.py:180-186 with benchnav_amd.AStar + benchnav_amd.DWA: the reference path of every control step is the
    oracle's walk from the step's start cell."""
    from benchnav_amd import DWA
    fx = FIX["smooth256"]
    G, res = fx["heights"].shape[0], fx["res"]
    astar = _planner(fx)
    gm = FakeGridMap(G, res)
    dyn = FakeDynamics(fx["risk"], gm)
    obj = FakeObjectives(torch.from_numpy(fx["goal_pos"]), fx["thr"])
    solver = DWA(horizon=20, dim_state=3, dim_control=2, dynamics=dyn, objectives=obj, a_lim=torch.tensor([0.5, 0.5]),
                 delta_t=0.1, num_lin_vel=10, num_ang_vel=10)
    _, nxt = _oracle("smooth256")
    k = next(i for i, s in enumerate(fx["status"]) if s == 0)
    state = torch.tensor([fx["starts"][k][0], fx["starts"][k][1], 0.0], dtype=torch.float32, device="cuda")
    for step in range(8):
        with torch.no_grad():
            reference_path = astar.forward(state=state)
            want = A.walk(nxt, A.pos_to_index(state[:2].cpu(), fx["x0"], fx["y0"], res))
            got = [tuple(int(v) for v in n) for n in torch.round(reference_path.cpu() / res).to(torch.int64)]
            assert got == want, step
            solver.update_reference_path(reference_path)
            action_seq, state_seq = solver.forward(state=state)
        assert torch.isfinite(state_seq).all()
        state = state_seq[0, 1].detach().clone()
