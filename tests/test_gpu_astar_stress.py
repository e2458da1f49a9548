"""GPU: the A* field solve (csrc/astar_kernels.hip) under stress -- the adversarial maps of tests/astar_maps.py one by one,
heterogeneous and tiny-instance batches, re-solves after the maps and goals change, a large map, the C ABI's edges, the AStar
class's input paths, and the absorption limit.  Checked bit for bit against the oracle where it is affordable, else with the
oracle-free fixpoint certificate (tests/astar_oracle.py certify_field) plus the float64 shortest path."""
import ctypes as C

import numpy as np
import pytest
import torch

import astar_maps as M
import astar_oracle as A
from helpers import FakeDynamics, FakeGridMap
from test_gpu_astar import _handle, _read, _set

pytestmark = pytest.mark.gpu
BN_ERR_INVALID, BN_ERR_STATE = -1, -4


def _fx(case):
    h, r, thr, res, _ = case
    return dict(heights=h, risk=r, thr=thr, res=res)


def _solve_one(case):
    h, r, thr, res, g = case
    H, W = h.shape
    lib, hd = _handle(H, W, 1)
    try:
        _set(lib, hd, 0, _fx(case), g)
        assert lib.bn_astar_solve_async(hd, None) == 0, lib.bn_astar_last_error()
        return _read(lib, hd, 0, H, W)
    finally:
        lib.bn_astar_destroy(hd)


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def _path(lib, hd, inst, start, max_len):
    buf = (C.c_int32 * (2 * max(max_len, 1)))()
    n = lib.bn_astar_path(hd, inst, start[0], start[1], buf, max_len)
    return n, [(buf[2 * i], buf[2 * i + 1]) for i in range(min(max(n, 0), max_len))]


def _certify(case, D, N, f64=True):
    """Certificate, next-hop rule and (optionally) float64 agreement of one solved instance."""
    h, r, thr, res, g = case
    why = A.certify_field(h, r, thr, res, g, D)
    assert why == "", why
    assert np.array_equal(N, A.next_hops(h, D, g, res)), f"next differs in {(N != A.next_hops(h, D, g, res)).sum()} cells"
    if f64:
        why = A.check_f64(h, r, thr, res, g, D, N)
        assert why == "", why
    else:
        A.hop_counts(N)


# ---- every adversarial map through its own handle ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_single_map_bit_exact_and_float64(name):
    case = M.CASES[name]
    h, r, thr, res, g = case
    H, W = h.shape
    lib, hd = _handle(H, W, 1)
    try:
        _set(lib, hd, 0, _fx(case), g)
        assert lib.bn_astar_solve_async(hd, None) == 0
        D, N = _read(lib, hd, 0, H, W)
        D0, N0 = A.solve(h, r, thr, res, g)
        bad = D.view(np.uint32) != D0.view(np.uint32)
        assert not bad.any(), f"{name}: D differs in {bad.sum()} cells, first (iy, ix) {np.argwhere(bad)[0]}"
        assert np.array_equal(N, N0), f"{name}: next differs in {(N != N0).sum()} cells"
        if name == "plateau":
            return                                  # test_plateau_fails_loudly
        if name not in M.NO_F64:
            why = A.check_f64(h, r, thr, res, g, D, N)
            assert why == "", f"{name}: {why}"
        hops = A.hop_counts(N)
        free = A.free_mask(r, thr)
        rng = np.random.default_rng(H * 1000 + W)
        starts = {(g[0], g[1]) if 0 <= g[0] < W and 0 <= g[1] < H else (0, 0), (0, 0), (W - 1, H - 1)}
        far = np.argwhere(hops == hops.max())[0]
        starts.add((int(far[1]), int(far[0])))                          # the longest walk
        for y, x in np.argwhere(free)[rng.choice(int(free.sum()), min(4, int(free.sum())), replace=False)]:
            starts.add((int(x), int(y)))
        if (~free).any():
            y, x = np.argwhere(~free)[0]
            starts.add((int(x), int(y)))                                # a start in collision
        for s in sorted(starts):
            want = A.walk(N0, s)
            n, got = _path(lib, hd, 0, s, H * W)
            assert (n == 0 and want is None) or got == want, (name, s, n)
    finally:
        lib.bn_astar_destroy(hd)


# ---- batches ------------------------------------------------------------------------------------------------------------
def test_heterogeneous_batch_of_64():
    """B = 64 maps of 256^2 (4096 tiles, at most one worker per CU): 8 generators, own seeds, thresholds and goals."""
    n, B = 256, 64
    cases = [M.batch_instance(k, n) for k in range(B)]
    lib, hd = _handle(n, n, B)
    try:
        for b, c in enumerate(cases):
            _set(lib, hd, b, _fx(c), c[4])
        runs = []
        for _ in range(3):
            assert lib.bn_astar_solve_async(hd, None) == 0
            runs.append([_read(lib, hd, b, n, n) for b in range(B)])
    finally:
        lib.bn_astar_destroy(hd)
    for b in range(B):
        assert _same(runs[0][b], runs[1][b]) and _same(runs[0][b], runs[2][b]), f"instance {b} differs between solves"
    for b, c in enumerate(cases):
        D, N = runs[0][b]
        _certify(c, D, N)
        assert np.isinf(D).all() == (b >= 62), b
    for b in (1, 3, 9, 63):                                             # percolation, spiral, percolation, collision goal
        assert _same(runs[0][b], A.solve(*cases[b])), b
    for b in (0, 2, 4, 5, 6, 7, 11, 62):
        assert _same(runs[0][b], _solve_one(cases[b])), b


def test_many_tiny_instances():
    """B = 400 instances of 20 x 17, one partial tile each: more tiles than workers, every instance with its own data."""
    H, W, B = 20, 17, 400
    rng = np.random.default_rng(5)
    cases = []
    for b in range(B):
        thr = float(np.float32(rng.uniform(0.05, 0.4)))
        r = (rng.random((H, W)) * 0.9 + 0.05).astype(np.float32)
        g = (int(rng.integers(W)), int(rng.integers(H)))
        cases.append((M.smooth_heights(H, W, b, amplitude=float(rng.uniform(0.1, 5.0))), r, thr, 0.5, g))
    lib, hd = _handle(H, W, B)
    try:
        for b, c in enumerate(cases):
            _set(lib, hd, b, _fx(c), c[4])
        assert lib.bn_astar_solve_async(hd, None) == 0
        out = [_read(lib, hd, b, H, W) for b in range(B)]
    finally:
        lib.bn_astar_destroy(hd)
    reached = 0
    for b, c in enumerate(cases):
        _certify(c, *out[b], f64=b % 10 == 0)
        reached += np.isfinite(out[b][0]).any()
    assert reached > 300


def test_resolve_after_maps_and_goals_change():
    """Re-solving a handle resets D: heights x4 make instance 3's field RISE, instance 5's goal moves, instance 6's goal goes
    off the map and comes back.  Every instance equals a fresh handle's solve; untouched instances do not change."""
    H, W, B = 96, 96, 8
    cases = [M.batch_instance(k, H) for k in range(B)]
    lib, hd = _handle(H, W, B)

    def solve_all():
        assert lib.bn_astar_solve_async(hd, None) == 0
        got = [_read(lib, hd, b, H, W) for b in range(B)]
        for b in range(B):
            assert _same(got[b], _solve_one(cases[b])), f"instance {b} differs from a fresh handle"
        return got

    try:
        for b, c in enumerate(cases):
            _set(lib, hd, b, _fx(c), c[4])
        first = solve_all()
        h, r, thr, res, g = cases[3]
        cases[3] = (h * np.float32(4.0), r, thr, res, g)
        _set(lib, hd, 3, _fx(cases[3]), g)
        h, r, thr, res, g = cases[5]
        r[H - 2, W - 3] = np.float32(thr + 0.5)
        cases[5] = (h, r, thr, res, (W - 3, H - 2))
        _set(lib, hd, 5, _fx(cases[5]), cases[5][4])
        g6 = cases[6][4]
        cases[6] = cases[6][:4] + ((W, 0),)
        assert lib.bn_astar_set_goal(hd, 6, W, 0) == 0
        second = solve_all()
        assert np.isinf(second[6][0]).all() and (second[6][1] == A.NEXT_NONE).all()
        fin = np.isfinite(first[3][0])
        assert (second[3][0][fin] >= first[3][0][fin]).all() and (second[3][0][fin] > first[3][0][fin]).mean() > 0.9
        assert not _same(second[5], first[5])
        cases[6] = cases[6][:4] + (g6,)
        assert lib.bn_astar_set_goal(hd, 6, *g6) == 0
        third = solve_all()
        assert _same(third[6], first[6])
        for b in (0, 1, 2, 4, 7):
            assert _same(second[b], first[b]) and _same(third[b], first[b]), b
    finally:
        lib.bn_astar_destroy(hd)


LARGE = 1024


def test_large_map_certified():
    """One LARGE^2 smooth map (4 x the cells of the largest map elsewhere), certified and checked against float64."""
    from benchnav_amd import synth
    n = LARGE
    h = synth.smooth_height_map(n, n, 1).numpy()
    r = synth.smooth_risk_map(n, 2).numpy()
    fy, fx = np.nonzero(~(r <= np.float32(0.25)))
    j = int(np.argmax(fy * n + fx))
    case = (h, r, 0.25, 0.5, (int(fx[j]), int(fy[j])))
    D, N = _solve_one(case)
    assert np.isfinite(D).mean() > 0.5
    _certify(case, D, N)


# ---- the C ABI's edges --------------------------------------------------------------------------------------------------
def test_path_abi_edges():
    case = M.CASES["percolation0"]
    h, r, thr, res, g = case
    H, W = h.shape
    D0, N0 = A.solve(h, r, thr, res, g)
    free = A.free_mask(r, thr)
    hops = A.hop_counts(N0)
    lib, hd = _handle(H, W, 1)
    try:
        _set(lib, hd, 0, _fx(case), g)
        assert lib.bn_astar_solve_async(hd, None) == 0
        assert _same(_read(lib, hd, 0, H, W), (D0, N0))                       # the walks below follow a correct map
        far = np.argwhere(hops == hops.max())[0]
        s = (int(far[1]), int(far[0]))
        want = A.walk(N0, s)
        n_full = len(want)
        assert _path(lib, hd, 0, s, n_full)[1] == want
        canary = -12345
        buf = (C.c_int32 * (2 * n_full))(*([canary] * (2 * n_full)))
        k = 7
        assert lib.bn_astar_path(hd, 0, s[0], s[1], buf, k) == n_full            # the full count; only k nodes written
        assert [(buf[2 * i], buf[2 * i + 1]) for i in range(k)] == want[:k]
        assert all(v == canary for v in buf[2 * k:])
        assert lib.bn_astar_path(hd, 0, s[0], s[1], None, 0) == n_full
        assert _path(lib, hd, 0, g, 4) == (1, [g])                             # start == goal
        cy, cx = np.argwhere(~free & (N0 != A.NEXT_NONE))[0]                    # a collision start next to the field
        cs = (int(cx), int(cy))
        assert _path(lib, hd, 0, cs, H * W)[1] == A.walk(N0, cs) and len(A.walk(N0, cs)) > 1
        uy, ux = np.argwhere(free & np.isinf(D0))[0]                           # a free start in another component
        assert _path(lib, hd, 0, (int(ux), int(uy)), H * W)[0] == 0
    finally:
        lib.bn_astar_destroy(hd)


def test_handle_abi_errors():
    lib, hd = _handle(40, 30, 2)
    try:
        assert lib.bn_astar_sync(hd) == BN_ERR_STATE                           # before any solve
        case = M.resolution(0.5, 40, 30)
        _set(lib, hd, 0, _fx(case), case[4])
        assert lib.bn_astar_solve_async(hd, None) == BN_ERR_STATE              # instance 1 has no map
        assert b"no map" in lib.bn_astar_last_error()
        hp, rp = np.ascontiguousarray(case[0]), np.ascontiguousarray(case[1])
        assert lib.bn_astar_set_map(hd, 1, hp.ctypes.data, rp.ctypes.data, 0, case[2], 0.7) == BN_ERR_INVALID
        assert lib.bn_astar_set_map(hd, 1, hp.ctypes.data, rp.ctypes.data, 0, case[2], 0.5) == 0
        assert lib.bn_astar_solve_async(hd, None) == 0 and lib.bn_astar_sync(hd) == 0
    finally:
        lib.bn_astar_destroy(hd)
    from benchnav_amd import _capi
    lib = _capi.load()
    out = C.c_void_p(7)
    assert lib.bn_astar_create(0, 8193, 8192, 1, C.byref(out)) == BN_ERR_INVALID and not out.value   # H W > 2^26


# ---- the AStar class's input paths --------------------------------------------------------------------------------------
def _planner(heights, risk, thr, res, goal):
    from benchnav_amd import AStar
    H, W = heights.shape
    gm = FakeGridMap(W, res, x_limits=(0.0, W * res), y_limits=(0.0, H * res))
    gm.tensors = {"heights": heights}
    goal_pos = torch.tensor([(goal[0] + 0.5) * res, (goal[1] + 0.5) * res], dtype=torch.float32)
    return AStar(gm, goal_pos, FakeDynamics(risk, gm), thr, device="cuda")


def test_astar_class_input_paths_give_one_field():
    h, r, thr, res, g = M.CASES["cliffs"]
    want = A.solve(h, r, thr, res, g)
    ht, rt = torch.from_numpy(h), torch.from_numpy(r)
    variants = {
        "cpu": (ht, rt),
        "cuda": (ht.cuda(), rt.cuda()),
        "float64": (ht.double().cuda(), rt.double()),
        "transposed views": (ht.t().contiguous().cuda().t(), rt.t().contiguous().t()),
    }
    assert not variants["transposed views"][0].is_contiguous() and not variants["transposed views"][1].is_contiguous()
    for what, (hv, rv) in variants.items():
        pl = _planner(hv, rv, thr, res, g)
        D, N = pl.field()
        assert _same((D.cpu().numpy(), N.cpu().numpy()), want), what
        pl.close()
    s = torch.cuda.Stream()
    base = torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        x = torch.rand(2048, 2048, device="cuda")
        for _ in range(20):
            x = x @ x / 2048.0                                              # keep s busy before the map is produced
        rs = base.clone()                                                   # the risk map, produced on s last
        pl = _planner(torch.from_numpy(h).cuda(), rs, thr, res, g)
        D, N = pl.field()
    assert _same((D.cpu().numpy(), N.cpu().numpy()), want)
    pl.close()


# ---- absorption: the documented limit is loud ---------------------------------------------------------------------------
def test_plateau_fails_loudly():
    from benchnav_amd import _capi
    h, r, thr, res, g = M.CASES["plateau"]
    H, W = h.shape
    D0, N0 = A.solve(h, r, thr, res, g)
    lib, hd = _handle(H, W, 1)
    try:
        _set(lib, hd, 0, _fx(M.CASES["plateau"]), g)
        assert lib.bn_astar_solve_async(hd, None) == 0
        assert _same(_read(lib, hd, 0, H, W), (D0, N0))
        buf = (C.c_int32 * (2 * H * W))()
        assert lib.bn_astar_path(hd, 0, 0, 0, buf, H * W) == BN_ERR_STATE
        assert b"exceeded" in lib.bn_astar_last_error()
        assert lib.bn_astar_path(hd, 0, 12, 0, buf, H * W) > 0               # the high side still walks
    finally:
        lib.bn_astar_destroy(hd)
    pl = _planner(torch.from_numpy(h).cuda(), torch.from_numpy(r).cuda(), thr, res, g)
    with pytest.raises(_capi.BenchnavError, match="exceeded"):
        pl.forward(torch.tensor([0.5 * res, 0.5 * res, 0.0], device="cuda"))
    assert pl.forward(torch.tensor([12.5 * res, 0.5 * res, 0.0], device="cuda")) is not None
    pl.close()
