"""GPU: one terrain generator and one A* handle taken through the calls that resize, re-allocate and late-allocate their buffers
(csrc/bn_host.h: the buffer table, its resize and its lazily built groups), against fresh handles that made one call each.  Every
comparison is bit for bit: the same kernels run on the same inputs, whatever the handle held before."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import astar_maps as M

pytestmark = pytest.mark.gpu

G, BATCH, RES, SEEDS = 20, 2, 0.5, (11, 12)
SMALL = dict(draws="device", num_craters=1, min_radius=2, max_radius=3)
LARGE = dict(draws="device", num_craters=2, min_radius=2, max_radius=4)


def _coloring_kwargs():
    """The colouring keywords of test_gpu_terrain_device_draws._coloring_kwargs."""
    from benchnav_amd.terrain import occupancies, slip_models
    return {"occupancy": occupancies(10)[0], "slip_models": slip_models(10), "lower_threshold": 0.8, "upper_threshold": 1.0}


def _draws(draws):
    """Every field of a list of Draws as arrays, in a fixed order."""
    out = []
    for d in draws:
        out += [np.array([d.attempts, int(d.gave_up), len(d.craters)]), d.phases]
        for c in d.craters:
            out += [c.center, np.array([c.radius, c.angle, c.neg_tan]), np.array([c.n, *c.bounds]), c.lin]
        out += [a for a in (d.light_uniforms, d.light) if a is not None]
    return out


def _terrain_step(gen, step, colorize_from=None):
    """Step `step` of the sequence on `gen`: the arrays it produces, as a list."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                      # craters that could not be placed
        if step == "e":
            heights, classes, light = colorize_from
            return [gen.colorize(heights, classes, 10, light).cpu().numpy()]
        if step == "c":
            t = gen.generate(SEEDS, is_crater=False)
        else:
            t = gen.generate(SEEDS, **{"a": SMALL, "b": LARGE, "d": dict(SMALL, **_coloring_kwargs())}[step])
        out = [getattr(t, k).cpu().numpy() for k in ("heights", "slopes", "latent_mean", "latent_std", "t_classes", "colors")]
        if step != "c":
            out += _draws(gen.device_draws())
    if step == "d":
        out.append(t.light)
    return out


@functools.lru_cache(maxsize=None)
def _terrain_reference():
    """What a fresh generator makes of each step alone; (e) colours the heights and classes of (d)."""
    from benchnav_amd.terrain import TerrainGenerator
    ref = {}
    for step in "abcde":
        with TerrainGenerator(G, RES, batch=BATCH) as gen:
            src = (ref["d"][0], ref["d"][4], ref["d"][-1]) if step == "e" else None
            ref[step] = _terrain_step(gen, step, src)
    return ref


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, i)


def test_terrain_buffers_resize_and_allocate_late_without_changing_a_bit():
    from benchnav_amd.terrain import TerrainGenerator
    ref = _terrain_reference()
    assert np.ptp(ref["a"][0]) > 0 and np.ptp(ref["d"][5]) > 0 and np.ptp(ref["e"][0]) > 0     # heights and colours are not blank
    assert ref["b"][0].tobytes() != ref["a"][0].tobytes()                     # and the steps differ
    for run in range(2):                                                     # close(), then once more on a new generator
        gen = TerrainGenerator(G, RES, batch=BATCH)
        last = None
        for step in "abcde":
            got = _terrain_step(gen, step, last and (last[0], last[4], last[-1]))
            _assert_same(got, ref[step], (run, step))
            last = got
        gen.close()


# ---- A* ----------------------------------------------------------------------------------------------------------------------
H, W, B = 33, 34, 2                                                          # two tiles each way with a ragged edge, H != W
GOALS = ((30, 3), (2, 31))
STARTS = np.array([[1, 1], [33, 32], [16, 17]], np.int32)
CAP = H * W


def _maps(seed):
    """B (heights, risk) pairs with ~5 % stuck cells; goals and starts are free."""
    out = []
    for b in range(B):
        risk = M.iid_risk(H, W, seed + b, 0.05)
        for cell in (GOALS[b], *map(tuple, STARTS)):
            M._free_goal(risk, cell)
        out.append((M.smooth_heights(H, W, seed + b), np.ascontiguousarray(risk, np.float32)))
    return out


def _ok(lib, rc):
    assert rc == 0, lib.bn_astar_last_error()


def _set_maps(lib, a, maps):
    from benchnav_amd import _capi
    for b, (h, r) in enumerate(maps):
        _ok(lib, lib.bn_astar_set_map(a, b, C.c_void_p(h.ctypes.data), C.c_void_p(r.ctypes.data), _capi.BN_MEM_HOST, M.THR, RES))
        _ok(lib, lib.bn_astar_set_goal(a, b, *GOALS[b]))


def _paths(lib, a, inst, n, expect=0):
    """bn_astar_paths_async from the first n host starts: (nodes, lengths) as numpy."""
    from benchnav_amd import _capi
    out = torch.full((n, CAP, 2), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    starts = np.ascontiguousarray(STARTS[:n])
    rc = lib.bn_astar_paths_async(a, inst, C.c_void_p(starts.ctypes.data), _capi.BN_MEM_HOST, n, CAP, C.c_void_p(out.data_ptr()),
                                  C.c_void_p(lens.data_ptr()), None)
    assert rc == expect, lib.bn_astar_last_error()
    torch.cuda.synchronize()
    return [out.cpu().numpy(), lens.cpu().numpy()]


def _state(lib, a):
    """D, next, hops, jump tables and the paths of all three starts, for every instance."""
    from benchnav_amd.astar import _DevArray
    view = lambda p, shape, t: torch.as_tensor(_DevArray(p.value, shape, typestr=t), device="cuda").cpu().numpy()
    _ok(lib, lib.bn_astar_sync(a))
    out = []
    for b in range(B):
        d, nx, hp, jp, lv, eb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        _ok(lib, lib.bn_astar_buffers(a, b, C.byref(d), C.byref(nx)))
        _ok(lib, lib.bn_astar_jump_buffers(a, b, C.byref(hp), C.byref(jp), C.byref(lv), C.byref(eb)))
        assert eb.value == 4
        out += [view(d, (H, W), "<f4"), view(nx, (H, W), "|u1"), view(hp, (H, W), "<i4"), view(jp, (lv.value, H * W), "<i4")]
        out += _paths(lib, a, b, 3)
    return out


def test_astar_handle_reused_equals_a_fresh_one():
    from benchnav_amd import _capi
    lib = _capi.load()
    first, final = _maps(100), _maps(200)
    fresh = C.c_void_p()
    _ok(lib, lib.bn_astar_create(0, H, W, B, C.byref(fresh)))
    _set_maps(lib, fresh, final)
    _ok(lib, lib.bn_astar_solve_async(fresh, None))
    _ok(lib, lib.bn_astar_jump_build_async(fresh, None))
    want = _state(lib, fresh)
    lib.bn_astar_destroy(fresh)
    assert want[5].max() > 1 and np.isfinite(want[0]).any()                   # paths were walked over a solved field

    a = C.c_void_p()
    _ok(lib, lib.bn_astar_create(0, H, W, B, C.byref(a)))
    _set_maps(lib, a, first)                                                 # 1
    _ok(lib, lib.bn_astar_solve_async(a, None))                              # 2
    _ok(lib, lib.bn_astar_jump_build_async(a, None))                         # 3: the tables' first allocation
    small = _paths(lib, a, 0, 1)                                             # 4
    grown = _paths(lib, a, 0, 3)                                             # 5: the staging grows
    assert np.array_equal(small[0][0], grown[0][0]) and small[1][0] == grown[1][0]
    _set_maps(lib, a, final)                                                 # 6
    _paths(lib, a, 0, 3, expect=_capi.BN_ERR_STATE)                          # stale tables are refused ...
    assert b"stale" in lib.bn_astar_last_error()
    _ok(lib, lib.bn_astar_solve_async(a, None))                              # 7
    _paths(lib, a, 0, 3, expect=_capi.BN_ERR_STATE)                          # ... until they are rebuilt
    _ok(lib, lib.bn_astar_jump_build_async(a, None))                         # 8
    _assert_same(_state(lib, a), want, "reused handle")                      # 9
    lib.bn_astar_destroy(a)
    for _ in range(2):
        b = C.c_void_p()
        _ok(lib, lib.bn_astar_create(0, H, W, B, C.byref(b)))
        lib.bn_astar_destroy(b)
