"""CPU: the task stage's rules that need no device.

  a. tests/tasks_spec.py, the NumPy spec the GPU tests use as their reference, against independent formulas: scipy.ndimage.label
     canonicalised to smallest indices, a per-attempt Python loop over the sampler's rules, hand-made masks and statistics;
  b. cell centres map back to their cells under the float32 lookup, for six resolutions and four sizes; `ix * resolution` does not;
  c. the new C entry points: declared, exported, bound;
  d. every argument refusal is raised before the device is touched, with its text;
  e. without a GPU a valid call is refused with BN_ERR_NO_DEVICE and "no CPU fallback";
  f. TaskSet's JSON round trip and SPL on hand-made arrays."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import tasks_spec as S
from benchnav_amd import _capi, tasks as T

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a. the spec against independent formulas -------------------------------------------------------------------------------------
def _scipy_labels(mask, connectivity):
    """scipy.ndimage.label, every label replaced by the smallest linear index of its component."""
    from scipy import ndimage
    structure = np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=structure)
    out = np.full(lab.shape, -1, np.int32)
    if n:
        idx = np.arange(lab.size).reshape(lab.shape)
        first = ndimage.minimum(idx, lab, index=np.arange(1, n + 1)).astype(np.int32)
        out[lab > 0] = first[lab[lab > 0] - 1]
    return out


@functools.lru_cache(maxsize=None)
def _cases():
    return S.label_cases()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_flood_fill_labels_equal_scipy(connectivity):
    for name, masks in _cases().items():
        labels, sizes, stats = S.label(masks, connectivity)
        for m, mask in enumerate(masks):
            want = _scipy_labels(mask, connectivity)
            assert np.array_equal(labels[m], want), (name, m, connectivity)
            roots = np.unique(want[want >= 0])
            assert stats[m, 0] == int((mask != 0).sum()) == int(sizes[m].sum()) and stats[m, 1] == roots.size, (name, m)
            assert np.array_equal(np.nonzero(sizes[m])[0], roots), (name, m)
            assert (labels[m].ravel()[roots] == roots).all() and (stats[m, 4:] == 0).all()


def test_statistics_by_hand():
    # three components under 4-connectivity: {0, 1} (size 2), {3, 7} (size 2), {10} (size 1); the tie goes to the smaller label
    mask = np.array([[[1, 1, 0, 1], [0, 0, 0, 1], [0, 0, 1, 0]]], np.uint8)
    labels, sizes, stats = S.label(mask, 4)
    assert labels[0].tolist() == [[0, 0, -1, 3], [-1, -1, -1, 3], [-1, -1, 10, -1]]
    assert sizes[0].tolist() == [2, 0, 0, 2, 0, 0, 0, 0, 0, 0, 1, 0] and stats[0].tolist() == [5, 3, 2, 0, 0, 0, 0, 0]
    labels, sizes, stats = S.label(mask, 8)                    # the diagonal joins {3, 7} and {10}
    assert labels[0, 2, 2] == 3 and stats[0].tolist() == [5, 2, 3, 3, 0, 0, 0, 0]
    assert S.label(np.zeros((1, 2, 2), np.uint8), 4)[2][0].tolist() == [0, 0, 0, -1, 0, 0, 0, 0]
    by_name = _cases()
    assert S.label(by_name["64_checkerboard"], 8)[2][0, :2].tolist() == [2048, 1] and S.label(by_name["64_checkerboard"], 4)[2][0, :3].tolist() == [2048, 2048, 1]
    for name in ("256_serpentine", "two_spirals", "comb"):
        assert S.label(by_name[name], 4)[2][0, 1] == (1 if name == "256_serpentine" else 2), name


def test_mask_at_the_threshold_edge():
    thr = 0.1
    at = f32(1.0) - f32(thr)                                   # 1 - float32(0.9) rounds to 0.100000024 > float32(0.1): passable
    mean = np.array([[0.0, 1.0, at, np.nextafter(at, f32(1)), -0.5, 1.5, np.nan, np.inf, -np.inf, 0.5, 0.5, 0.5]], f32)
    std = np.array([[0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, np.nan, np.inf, 0.1]], f32)
    assert S.passable(mean, std, 0.0, thr).tolist() == [[1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1]]
    assert S.passable(mean, std, 4.5, thr).tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]]      # 0.5 + 0.45 = 0.95: stuck
    # a rounded product, then a rounded sum: a fused multiply-add would keep the product's low bits
    k, s, m = f32(1.0 + 2.0 ** -12), f32(1.0 + 2.0 ** -12), f32(-1.0 - 2.0 ** -11)
    assert f32(k * s) + m == 0.0 and float(k) * float(s) + float(m) > 0.0
    assert S.passable([[m]], [[s]], k, float(f32(1) - f32(2.0 ** -24))).tolist() == [[1]]


# ---- b. cell centres -----------------------------------------------------------------------------------------------------------------
def test_cell_centres_map_back_and_cell_corners_do_not():
    for res in (0.1, 0.25, 0.3, 0.5, 1.0, 2.0):
        for G in (64, 256, 512, 2048):
            i = np.arange(G)
            assert np.array_equal(S.cell_of(S.cell_centres(i, 0.0, res), 0.0, res), i), (res, G)
    corner = lambda G: S.cell_of((np.arange(G).astype(f32) * f32(0.3)).astype(f32), 0.0, 0.3)
    assert int((corner(64) == np.arange(64) - 1).sum()) == 4 and int((corner(2048) == np.arange(2048) - 1).sum()) == 136
    assert int((corner(64) != np.arange(64)).sum()) == 4


# ---- the sampler -------------------------------------------------------------------------------------------------------------------
def test_sampler_accepts_what_the_rules_accept():
    """Every pair against a per-attempt Python loop with the rules as the header states them."""
    import rng_reference as R
    mask = np.stack([S.iid(40, 52, 11), S.iid(40, 52, 12, blocked=0.45)])
    labels, sizes, _ = S.label(mask, 4)
    P, seed, first_map, border, sep_sq, min_cells, attempts = 6, (7 << 32) | 9, 3, 3, 15 ** 2, 30, 128
    cells, attempt, pos = S.sample(labels, sizes, P, seed, first_map, border, sep_sq, min_cells, attempts, x0=-1.0, y0=2.0, resolution=0.3)
    H, W = 40, 52
    Win, Hin = W - 2 * border, H - 2 * border
    found = 0
    for m in range(2):
        for p in range(P):
            want = -1
            for a in range(attempts):
                r = R.philox4x32(a, p, first_map + m, 0x5441534B, 9, 7)
                s, g = (int(r[0]) * Win * Hin) >> 32, (int(r[1]) * Win * Hin) >> 32
                sx, sy, gx, gy = s % Win + border, s // Win + border, g % Win + border, g // Win + border
                ls, lg = labels[m, sy, sx], labels[m, gy, gx]
                if ls >= 0 and ls == lg and sizes[m, ls] >= min_cells and (gx - sx) ** 2 + (gy - sy) ** 2 >= sep_sq:
                    want = a
                    break
            assert attempt[m, p] == want
            if want < 0:
                assert (cells[m, p] == -1).all() and np.isnan(pos[m, p]).all()
                continue
            found += 1
            assert cells[m, p].tolist() == [sx, sy, gx, gy] and border <= sx < W - border and border <= gy < H - border
            assert pos[m, p].tolist() == [f32(-1.0) + f32(f32(sx + 0.5) * f32(0.3)), f32(2.0) + f32(f32(sy + 0.5) * f32(0.3)),
                                          f32(-1.0) + f32(f32(gx + 0.5) * f32(0.3)), f32(2.0) + f32(f32(gy + 0.5) * f32(0.3))]
    assert found >= 6
    none = S.sample(labels, sizes, 2, 1, min_component_cells=10 ** 6, max_attempts=64)
    assert (none[0] == -1).all() and (none[1] == -1).all() and np.isnan(none[2]).all() and none[2].dtype == f32


# ---- c. the C entry points -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("bn_task_workspace_bytes", "bn_task_mask_async", "bn_task_label_async", "bn_task_sample_async", "bn_task_last_error")


def test_new_functions_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "benchnav_mppi.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in _capi.SYMBOLS and getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    for name, value in (("TILE", 32), ("STATS", S.STATS), ("MAX_SIDE", 4096), ("MAX_MAPS", 4096), ("MAX_PAIRS", 65536), ("MAX_ATTEMPTS", 4096),
                        ("ERR_TILE", 1), ("ERR_UNITE", 2), ("ERR_FLATTEN", 4)):
        assert re.search(r"#define\s+BN_TASK_%s\s+%d\b" % (name, value), text) and getattr(_capi, "BN_TASK_" + name) == value
    assert re.search(r"#define\s+BN_TASK_MAX_CELLS\s+\(1 << 24\)", text) and _capi.BN_TASK_MAX_CELLS == 1 << 24
    from benchnav_amd import build
    assert "task_kernels.hip" in build.SOURCES
    import benchnav_amd
    assert benchnav_amd.TaskSet is T.TaskSet and benchnav_amd.label_components is T.label_components


# ---- d. arguments ----------------------------------------------------------------------------------------------------------------
_BUF = np.zeros(64, np.float64)
_P = _BUF.ctypes.data


def _mask_call(lib, M=1, cells=1, kappa=0.0, thr=0.1, mean=_P, std=_P, mask=_P):
    return lib.bn_task_mask_async(0, None, mean, std, M, cells, kappa, thr, mask)


def _label_call(lib, M=1, H=1, W=1, conn=4, mask=_P, labels=_P, sizes=_P, stats=_P, work=_P, nbytes=None):
    need = lib.bn_task_workspace_bytes(M, H, W)
    return lib.bn_task_label_async(0, None, mask, M, H, W, conn, labels, sizes, stats, work, need if nbytes is None else nbytes)


def _sample_call(lib, M=1, H=8, W=8, P=1, seed=0, first_map=0, border=2, sep=0, min_cells=1, attempts=64, x0=0.0, y0=0.0, res=0.5, labels=_P,
                 sizes=_P, cells=_P, attempt=_P, positions=_P):
    return lib.bn_task_sample_async(0, None, labels, sizes, M, H, W, P, seed, first_map, border, sep, min_cells, attempts, x0, y0, res, cells,
                                    attempt, positions)


REFUSALS = [
    (_mask_call, dict(mean=None), b"null argument"), (_mask_call, dict(std=None), b"null argument"), (_mask_call, dict(mask=None), b"null output"),
    (_mask_call, dict(M=0), b"num_maps"), (_mask_call, dict(M=4097), b"num_maps"), (_mask_call, dict(cells=0), b"cells"),
    (_mask_call, dict(cells=2 ** 24 + 1), b"cells"), (_mask_call, dict(kappa=float("nan")), b"kappa"),
    (_mask_call, dict(kappa=float("inf")), b"kappa"), (_mask_call, dict(thr=float("nan")), b"stuck_threshold"),
    (_label_call, dict(mask=None), b"null argument"), (_label_call, dict(labels=None), b"null output"), (_label_call, dict(sizes=None), b"null output"),
    (_label_call, dict(stats=None), b"null output"), (_label_call, dict(M=0), b"num_maps"), (_label_call, dict(M=4097), b"num_maps"),
    (_label_call, dict(H=0), b"H and W"), (_label_call, dict(W=0), b"H and W"), (_label_call, dict(H=4097), b"H and W"),
    (_label_call, dict(W=4097), b"H and W"), (_label_call, dict(H=4096, W=4097), b"H and W"), (_label_call, dict(H=4096, W=4096, M=2, nbytes=0), b"workspace"),
    (_label_call, dict(conn=6), b"connectivity"), (_label_call, dict(conn=0), b"connectivity"), (_label_call, dict(work=None), b"workspace"),
    (_label_call, dict(M=2, H=33, W=65, nbytes=2 * 33 * 65 * 4 - 1), b"workspace"),
    (_sample_call, dict(labels=None), b"null argument"), (_sample_call, dict(sizes=None), b"null argument"),
    (_sample_call, dict(cells=None), b"null output"), (_sample_call, dict(attempt=None), b"null output"), (_sample_call, dict(positions=None), b"null output"),
    (_sample_call, dict(M=0), b"num_maps"), (_sample_call, dict(H=0), b"H and W"), (_sample_call, dict(W=4097), b"H and W"),
    (_sample_call, dict(P=0), b"num_pairs"), (_sample_call, dict(P=65537), b"num_pairs"), (_sample_call, dict(first_map=-1), b"first_map"),
    (_sample_call, dict(first_map=2 ** 32 - 1), b"first_map"), (_sample_call, dict(border=-1), b"border"), (_sample_call, dict(border=4), b"border"),
    (_sample_call, dict(H=9, W=6, border=3), b"border"), (_sample_call, dict(sep=-1), b"min_separation_sq"),
    (_sample_call, dict(min_cells=-1), b"min_component_cells"), (_sample_call, dict(attempts=0), b"max_attempts"),
    (_sample_call, dict(attempts=100), b"max_attempts"), (_sample_call, dict(attempts=4160), b"max_attempts"),
    (_sample_call, dict(res=0.0), b"resolution"), (_sample_call, dict(res=float("nan")), b"resolution"), (_sample_call, dict(x0=float("inf")), b"x0"),
]


def test_arguments_are_refused_before_the_device_is_touched():
    """BN_ERR_INVALID, not BN_ERR_NO_DEVICE and not a HIP error: on a machine without a GPU the argument checks come first."""
    lib = _capi.load()
    for call, kw, text in REFUSALS:
        assert call(lib, **kw) == _capi.BN_ERR_INVALID, (call.__name__, kw)
        assert text in lib.bn_task_last_error(), (call.__name__, kw, lib.bn_task_last_error())
    assert lib.bn_task_workspace_bytes(2, 33, 65) == 2 * 33 * 65 * 4 and lib.bn_task_workspace_bytes(4096, 4096, 4096) == 2 ** 38
    assert lib.bn_task_workspace_bytes(1, 4096, 4096) == 2 ** 26 and lib.bn_task_workspace_bytes(1, 1, 1) == 4
    for bad in ((0, 1, 1), (4097, 1, 1), (1, 0, 1), (1, 1, 0), (1, 4097, 1), (1, 1, 4097), (1, 4096, 4097)):
        assert lib.bn_task_workspace_bytes(*bad) == 0, bad


def test_the_cell_limit_is_two_to_the_24():
    lib = _capi.load()
    # 4096 x 4096 is exactly 2^24 cells: in range; no taller or wider shape fits the side limit, so the product limit shows in the mask call
    assert lib.bn_task_workspace_bytes(1, 4096, 4096) > 0
    assert _mask_call(lib, cells=2 ** 24 + 1) == _capi.BN_ERR_INVALID and b"2^24" in lib.bn_task_last_error()


def test_python_wrappers_check_their_arguments(monkeypatch):
    monkeypatch.setattr(T, "resolve_device", lambda *a, **k: torch.device("cpu"))         # the checks below come before any launch
    one = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="kappa"):
        T.passable_mask(one, one, kappa=float("nan"))
    with pytest.raises(ValueError, match=r"\(M, H, W\)"):
        T.passable_mask(torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="connectivity"):
        T.label_components(one, connectivity=6)
    with pytest.raises(ValueError, match="pairs"):
        T.sample_pairs(one, torch.zeros(1, 16), 0, seed=1)
    with pytest.raises(ValueError, match="sizes"):
        T.sample_pairs(one, torch.zeros(1, 15), 1, seed=1)


# ---- e. no fallback --------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_gpu():
    lib = _capi.load()
    for call in (_mask_call, _label_call, _sample_call):
        assert call(lib) == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_task_last_error(), call.__name__
    one = torch.zeros(1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.passable_mask(one, one)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.label_components(one)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.sample_pairs(one, torch.zeros(1, 64), 1, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.optimal_lengths(one, torch.zeros(1, 1, 4, dtype=torch.int32), 0.5)


# ---- f. the task set and SPL -----------------------------------------------------------------------------------------------------
def _task_set():
    start = np.array([[[1.25, 2.25], [np.nan, np.nan]], [[3.75, 0.25], [0.25, 0.25]]], f32)
    goal = np.array([[[9.25, 2.25], [np.nan, np.nan]], [[3.75, 7.25], [5.25, 5.25]]], f32)
    cells = np.array([[[2, 4, 18, 4], [-1, -1, -1, -1]], [[7, 0, 7, 14], [0, 0, 10, 10]]], np.int32)
    return T.TaskSet(start, goal, cells, [[5, -1], [0, 17]], [[True, False], [True, False]], [[8.0, np.nan], [7.5, np.inf]],
                     {"kind": "sampled", "seed": 3, "trials": 2, "min_separation_sq": 100})


def test_task_set_json_round_trip(tmp_path):
    ts = _task_set()
    path = tmp_path / "sub" / "tasks.json"
    ts.to_json(str(path))
    text = path.read_text()
    assert "NaN" not in text and "Infinity" not in text
    doc = json.loads(text)
    assert doc["optimal_length"] == [[8.0, None], [7.5, "inf"]] and doc["params"]["seed"] == 3
    back = T.TaskSet.from_json(str(path))
    for name in ("start", "goal", "cells", "attempt", "valid", "optimal_length"):
        a, b = getattr(ts, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert back.params == ts.params and (back.maps, back.trials) == (2, 2)
    with pytest.raises(ValueError, match="cells"):
        T.TaskSet(ts.start, ts.goal, ts.cells[:, :1], ts.attempt, ts.valid, ts.optimal_length, {})


def test_spl_on_hand_made_arrays():
    GOAL, LIMIT, STOPPED, INVALID = 0, 1, 2, 3
    outcome = np.array([GOAL, GOAL, LIMIT, INVALID, STOPPED, GOAL])
    L = np.array([10.0, 4.0, 30.0, 0.0, 2.0, 8.0])
    best = np.array([5.0, 5.0, 6.0, 7.0, 3.0, 8.0])
    # 5 / 10, then L < L*: 1, an unreached goal: 0, INVALID: left out, stopped: 0, exactly optimal: 1
    want = (0.5 + 1.0 + 0.0 + 0.0 + 1.0) / 5
    for fn in (S.spl, T.spl_figures):
        spl, ratio = fn(outcome, L, best)
        assert spl == want and ratio == (10.0 / 5.0 + 4.0 / 5.0 + 8.0 / 8.0) / 3, fn
        assert fn(np.array([INVALID]), [1.0], [1.0]) == (None, None) and fn(np.array([LIMIT]), [1.0], [1.0]) == (0.0, None)
        assert fn(np.array([GOAL]), [0.0], [0.0]) == (1.0, None)


def test_report_gains_spl_only_with_a_task_set():
    from benchnav_amd.benchmark import FIELDS, Report
    rng = np.random.default_rng(0)
    arrays = {name: np.zeros((1, 2, 2), np.dtype(str(dt).replace("torch.", ""))) for name, dt in FIELDS}
    arrays["outcome"][0] = [[0, 1], [0, 3]]
    arrays["path_length"][0] = rng.uniform(6.0, 9.0, (2, 2))
    arrays["steps"][0] = 5
    plain = Report("mppi", ["expected_value"], arrays, 0, 4, 2, 20, 0.1, 2.0)
    doc = plain.to_dict()
    assert "tasks" not in doc and "optimal_length" not in doc["episodes"] and "spl" not in doc["summary"][0] and "spl" not in plain.table()
    ts = _task_set()
    rep = Report("mppi", ["expected_value"], arrays, 0, 4, 2, 20, 0.1, 2.0, tasks=ts)
    row, doc = rep.summary()[0], rep.to_dict()
    assert (row["spl"], row["path_ratio_mean"]) == S.spl(arrays["outcome"][0], arrays["path_length"][0], ts.optimal_length)
    assert {k: v for k, v in row.items() if k not in ("spl", "path_ratio_mean")} == plain.summary()[0]
    assert doc["tasks"] == ts.params and doc["episodes"]["optimal_length"] == [[8.0, None], [7.5, "inf"]] and "spl" in rep.table()
    json.dumps(doc, allow_nan=False)
