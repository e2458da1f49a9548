"""CPU: the model-evaluation stage's rules that need no device.

  a. tests/evaluate_spec.py, the NumPy float64 spec the GPU tests use as their reference, against independent formulas: np.bincount,
     torch.distributions (KL, log_prob) in float64, a per-cell Python loop on a hand-made 3 x 3 map;
  b. the new C entry points: declared, exported, bound;
  c. every argument refusal is raised before the device is touched, with its text;
  d. without a GPU a valid call is refused with BN_ERR_NO_DEVICE and "no CPU fallback";
  e. EvaluationReport's arithmetic on hand-made tables, the None rates included."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import evaluate_spec as S
from benchnav_amd import _capi, evaluate as EV

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a. the spec against independent formulas -------------------------------------------------------------------------------------
def test_confusion_is_bincount():
    rng = np.random.default_rng(1)
    M, cells, Cn = 3, 500, 5
    t, p = rng.integers(-1, Cn + 1, (M, cells)).astype(np.int32), rng.integers(-1, Cn + 1, (M, cells)).astype(np.int32)
    table, ignored = S.confusion(t, p, Cn)
    for m in range(M):
        ok = (t[m] >= 0) & (t[m] < Cn) & (p[m] >= 0) & (p[m] < Cn)
        want = np.bincount(t[m][ok] * Cn + p[m][ok], minlength=Cn * Cn).reshape(Cn, Cn)
        assert (table[m] == want).all() and ignored[m] == (~ok).sum() and ignored[m] > 0
    assert table.dtype == np.int64 and table.sum() + ignored.sum() == M * cells


def _slip_data(rng, M, cells, Cn):
    mu, m = rng.uniform(0, 1, (M, cells)).astype(f32), rng.uniform(0, 1, (M, cells)).astype(f32)
    sigma, s = rng.uniform(0.01, 0.3, (M, cells)).astype(f32), rng.uniform(0.01, 0.3, (M, cells)).astype(f32)
    phi = rng.uniform(0, 30, (M, cells)).astype(f32)
    cls = rng.integers(0, Cn, (M, cells)).astype(np.int32)
    y = (m + s * rng.standard_normal((M, cells))).astype(f32)
    return mu, sigma, m, s, phi, cls, y


def test_slip_sums_against_torch_distributions():
    """KL against torch.distributions.kl_divergence and NLL against Normal.log_prob, float64, summed per group with math.fsum.  The
    spec's ordered sum of n terms may differ from the exact sum of the independent terms by its n roundings and by the few ulps per
    term that the two formulas' different operation orders leave: (n + 8) 2^-52 of the sum of the terms' magnitudes."""
    from torch.distributions import Normal, kl_divergence
    rng = np.random.default_rng(2)
    M, cells, Cn, NB = 2, 4096 + 70, 3, 6                  # a slab, a step and a partial step
    mu, sigma, m, s, phi, cls, y = _slip_data(rng, M, cells, Cn)
    got = S.slip(mu, sigma, m, s, phi, cls, Cn, y=y, bins=NB, max_slope=30.0)
    T = lambda a: torch.from_numpy(a.astype(np.float64))
    pred, lat = Normal(T(mu), T(sigma)), Normal(T(m), T(s))
    kl, nll = kl_divergence(lat, pred).numpy(), -pred.log_prob(T(y)).numpy()
    d = mu.astype(np.float64) - m.astype(np.float64)
    z = (y.astype(np.float64) - mu.astype(np.float64)) / sigma.astype(np.float64)
    group = cls.astype(np.int64) * NB + np.minimum((phi.astype(np.float64) // 5.0).astype(np.int64), NB - 1)
    assert got["invalid"].tolist() == [0, 0] and got["counts"][..., 0].sum() == M * cells
    for mm in range(M):
        for g in range(Cn * NB):
            sel = group[mm] == g
            n = int(sel.sum())
            c, j = divmod(g, NB)
            assert got["counts"][mm, c, j, 0] == n and got["counts"][mm, c, j, 1] == int((np.abs(z[mm][sel]) <= 2.0).sum())
            want = [d[mm][sel], np.abs(d[mm][sel]), d[mm][sel] ** 2, sigma[mm][sel].astype(np.float64), s[mm][sel].astype(np.float64), kl[mm][sel],
                    nll[mm][sel], z[mm][sel] ** 2]
            for k, terms in enumerate(want):
                exact, mag = math.fsum(terms), math.fsum(np.abs(terms))
                assert abs(got["sums"][mm, c, j, k] - exact) <= (n + 8) * 2.0 ** -52 * mag + 1e-300, (mm, g, S.SUM_NAMES[k])


def test_slip_bins_and_invalid_cells():
    # slopes on the bin edges: closed on the left, clamped at both ends
    phi = np.array([[0.0, 4.999, 5.0, 29.999, 30.0, 31.0, -1.0, 10.0]], f32)
    assert S.slope_bin(phi, 6, 30.0).tolist() == [[0, 0, 1, 5, 5, 5, 0, 2]]
    assert S.slope_bin(phi, 1, 30.0).tolist() == [[0] * 8]
    n = phi.shape[1]
    full = lambda v: np.full((1, n), v, f32)
    got = S.slip(full(0.5), full(0.1), full(0.5), full(0.1), phi, np.zeros((1, n), np.int32), 1, y=full(0.5), bins=6)
    assert got["counts"][0, 0, :, 0].tolist() == [3, 1, 1, 0, 0, 3] and got["invalid"].tolist() == [0]
    # each way a cell is invalid, one cell each; the last one is valid
    mu = np.array([[np.nan, .5, .5, .5, .5, .5, .5, .5, .5, .5]], f32)
    sg = np.array([[.1, 0.0, -.1, .1, .1, .1, .1, .1, np.inf, .1]], f32)
    s = np.array([[.1, .1, .1, 0.0, .1, .1, .1, .1, .1, .1]], f32)
    ph = np.array([[1, 1, 1, 1, np.nan, 1, 1, 1, 1, 1]], f32)
    y = np.array([[.5, .5, .5, .5, .5, np.inf, -np.inf, .5, .5, .5]], f32)
    cl = np.array([[0, 0, 0, 0, 0, 0, 0, 2, 0, 1]], np.int32)
    got = S.slip(mu, sg, np.full((1, 10), .5, f32), s, ph, cl, 2, y=y, bins=2)
    assert got["invalid"].tolist() == [9] and got["counts"][0, :, :, 0].tolist() == [[0, 0], [1, 0]]
    assert S.slip(mu, sg, np.full((1, 10), .5, f32), s, ph, cl, 2, bins=2)["invalid"].tolist() == [7]          # without y its two cells count
    # y exactly at mu +- 2 sigma is covered; a little beyond is not (-1e-10: far enough from 0 for y - mu to differ from -0.25 in float64)
    mu, sg = full(0.25)[:, :4], full(0.125)[:, :4]
    y = np.array([[0.5, 0.0, np.nextafter(f32(0.5), f32(1)), -1e-10]], f32)
    got = S.slip(mu, sg, mu, sg, full(1.0)[:, :4], np.zeros((1, 4), np.int32), 1, y=y, bins=1)
    assert got["counts"][0, 0, 0].tolist() == [4, 2] and got["sums"][0, 0, 0, 7] > 8.0
    # the latent model as the prediction: d, KL exactly 0
    assert got["sums"][0, 0, 0, :3].tolist() == [0.0, 0.0, 0.0] and got["sums"][0, 0, 0, 5] == 0.0


def test_slip_sum_order_is_the_stated_one():
    """Hand-walk of the order on values whose float64 sum depends on it: one group, 130 cells = two steps and a partial one."""
    rng = np.random.default_rng(3)
    n = 130
    mu = (rng.uniform(0, 1, (1, n)) * 10.0 ** rng.integers(-6, 1, (1, n))).astype(f32)
    z = np.zeros((1, n), f32)
    got = S.slip(mu, np.ones((1, n), f32), z, np.ones((1, n), f32), z, np.zeros((1, n), np.int32), 1, bins=1)["sums"][0, 0, 0, 0]
    x = np.concatenate([mu[0].astype(np.float64), np.zeros(192 - n)])
    total = 0.0
    for st in range(3):
        w = list(x[st * 64:(st + 1) * 64])
        for off in (32, 16, 8, 4, 2, 1):
            w = [w[i] + w[i + off] for i in range(off)]
        total = total + w[0]
    assert got == 0.0 + total
    # ... and it is not a running sum: lanes 1 and 33 meet at the tree's first level, 1 + 1 = 2 survives next to 2^53, 1 alone does not
    mu = np.zeros((1, 64), f32)
    mu[0, [0, 1, 33]] = [2.0 ** 53, 1.0, 1.0]
    got = S.slip(mu, np.ones((1, 64), f32), z[:, :64], np.ones((1, 64), f32), z[:, :64], np.zeros((1, 64), np.int32), 1, bins=1)["sums"][0, 0, 0, 0]
    assert got == 2.0 ** 53 + 2.0 and float(np.cumsum(mu[0].astype(np.float64))[-1]) == 2.0 ** 53
    sums = rng.standard_normal((4, 2, 3, 8))
    want = np.zeros((2, 3, 8))
    for mm in range(4):
        want = want + sums[mm]
    assert (S.slip_total(sums) == want).all()
    assert (S.slip_total(sums[2:], start=S.slip_total(sums[:2])) == want).all()         # maps split over calls: the same bits


def test_metric_bound_is_the_derived_one():
    assert S.metric_bound(3.0, 10) == (2 + 2 + 10) * 2.0 ** -52 * 3.0 and S.metric_bound(0.0, 5) == 0.0
    assert S.U_LOG_DEVICE == 1 and S.LOG_SUMS == (5, 6)


def test_risk_tables_against_a_cell_loop():
    thr = 0.1
    at = f32(1.0) - f32(thr)                               # float32(0.9): 1 - at rounds to 0.100000024 > float32(0.1), one step up is stuck
    y = np.array([[0.0, 1.0, at, np.nextafter(at, f32(1)), 0.5, 0.95, -0.5, 1.5, np.nan]], f32)          # a 3 x 3 map
    r = np.array([[[0.0, 1.0, at, 0.95, 0.5, np.nextafter(at, f32(1)), np.inf, 0.2, 0.3]],
                  [[1.0, 0.0, 0.5, 0.5, 0.5, 0.5, 0.1, 1.2, 0.3]]], f32)
    cls = np.array([[0, 1, 2, 0, 1, 2, 0, 3, 1]], np.int32)
    counts, invalid = S.risk(r, y, cls, 3, thr)
    want, bad = np.zeros((1, 2, 3, 5), np.int64), np.zeros((1, 2), np.int64)
    stuck = lambda v: bool(f32(1.0) - min(max(f32(v), f32(0.0)), f32(1.0)) <= f32(thr))
    for k in range(2):
        for i in range(9):
            yi, ri, c = y[0, i], r[k, 0, i], int(cls[0, i])
            if not (0 <= c < 3) or not np.isfinite(yi) or not np.isfinite(ri):
                bad[0, k] += 1
                continue
            want[0, k, c, 0] += int(yi > ri)
            want[0, k, c, 1 + 2 * int(stuck(ri)) + int(stuck(yi))] += 1
    assert (counts == want).all() and (invalid == bad).all()
    assert bad.tolist() == [[3, 2]] and want[0, :, :, 1:].sum() == 18 - 5
    assert stuck(1.0) and not stuck(at) and stuck(np.nextafter(at, f32(1))) and not stuck(0.0) and stuck(1.5) and not stuck(-0.5)
    assert (S.stuck(np.array([0.875, 0.8749999], f32), 0.125) == [True, False]).all()          # exactly at a threshold float32 holds
    assert want[0, 1, 2, 2] == 1           # believed safe (0.5), actually stuck (0.95)


# ---- b. the C entry points -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("bn_eval_confusion_async", "bn_eval_slip_async", "bn_eval_slip_workspace_bytes", "bn_eval_risk_async", "bn_eval_last_error")


def test_new_functions_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "benchnav_mppi.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in _capi.SYMBOLS and getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    for name, value in (("MAX_CLASSES", 64), ("MAX_BINS", 64), ("MAX_GROUPS", 512), ("SLAB_CELLS", S.SLAB), ("SLIP_SUMS", S.SUMS),
                        ("RISK_COUNTS", S.RISK_COUNTS)):
        assert re.search(r"#define\s+BN_EVAL_%s\s+%d\b" % (name, value), text) and getattr(_capi, "BN_EVAL_" + name) == value
    from benchnav_amd.dataset import MAX_CLASSES
    assert MAX_CLASSES == _capi.BN_EVAL_MAX_CLASSES
    assert EV.SLIP_SUMS == S.SUM_NAMES and len(EV.RISK_COUNTS) == S.RISK_COUNTS
    import benchnav_amd
    assert benchnav_amd.Evaluator is EV.Evaluator and benchnav_amd.confusion_matrix is EV.confusion_matrix


# ---- c. arguments ----------------------------------------------------------------------------------------------------------------
_BUF = np.zeros(64, np.float64)
_P = _BUF.ctypes.data


def _confusion_call(lib, M=1, cells=1, Cn=1, t=_P, p=_P, table=_P, ignored=_P):
    return lib.bn_eval_confusion_async(0, None, t, p, M, cells, Cn, table, ignored)


def _slip_call(lib, M=1, cells=1, Cn=1, NB=1, max_slope=30.0, mean=_P, sums=_P, work=_P, nbytes=None, slips=None):
    need = lib.bn_eval_slip_workspace_bytes(M, cells, Cn, NB)
    return lib.bn_eval_slip_async(0, None, mean, _P, _P, _P, _P, _P, slips, M, cells, Cn, NB, max_slope, sums, _P, _P, None, work,
                                  need if nbytes is None else nbytes)


def _risk_call(lib, S_=1, M=1, cells=1, Cn=1, thr=0.1, risk=_P, counts=_P):
    return lib.bn_eval_risk_async(0, None, risk, _P, _P, S_, M, cells, Cn, thr, counts, _P)


REFUSALS = [
    (_confusion_call, dict(t=None), b"null argument"), (_confusion_call, dict(p=None), b"null argument"),
    (_confusion_call, dict(table=None), b"null output"), (_confusion_call, dict(ignored=None), b"null output"),
    (_confusion_call, dict(M=0), b"num_maps"), (_confusion_call, dict(cells=0), b"cells"),
    (_confusion_call, dict(Cn=0), b"num_classes"), (_confusion_call, dict(Cn=65), b"num_classes"),
    (_confusion_call, dict(M=2 ** 31 - 1, cells=2 ** 40), b"out of range"), (_confusion_call, dict(cells=2 ** 63 - 1), b"out of range"),
    (_slip_call, dict(M=2 ** 31 - 1, Cn=64, NB=8), b"num_maps * num_classes * num_bins"),          # the second launch's grid
    (_slip_call, dict(mean=None), b"null argument"), (_slip_call, dict(sums=None), b"null output"),
    (_slip_call, dict(M=0), b"num_maps"), (_slip_call, dict(cells=0), b"cells"), (_slip_call, dict(Cn=0), b"num_classes"),
    (_slip_call, dict(Cn=65), b"num_classes"), (_slip_call, dict(NB=0), b"num_bins"), (_slip_call, dict(NB=65), b"num_bins"),
    (_slip_call, dict(Cn=64, NB=9), b"num_classes * num_bins"), (_slip_call, dict(max_slope=0.0), b"max_slope"),
    (_slip_call, dict(max_slope=-1.0), b"max_slope"), (_slip_call, dict(max_slope=float("nan")), b"max_slope"),
    (_slip_call, dict(work=None), b"workspace"), (_slip_call, dict(M=2, cells=5000, Cn=4, NB=6, nbytes=2 * 2 * 24 * 64 - 1), b"workspace"),
    (_risk_call, dict(risk=None), b"null argument"), (_risk_call, dict(counts=None), b"null output"),
    (_risk_call, dict(S_=0), b"num_settings"), (_risk_call, dict(S_=17), b"num_settings"), (_risk_call, dict(M=0), b"num_maps"),
    (_risk_call, dict(cells=0), b"cells"), (_risk_call, dict(Cn=65), b"num_classes"), (_risk_call, dict(thr=float("nan")), b"stuck_threshold"),
]


def test_arguments_are_refused_before_the_device_is_touched():
    """BN_ERR_INVALID, not BN_ERR_NO_DEVICE and not a HIP error: on a machine without a GPU the argument checks come first."""
    lib = _capi.load()
    for call, kw, text in REFUSALS:
        assert call(lib, **kw) == _capi.BN_ERR_INVALID, (call.__name__, kw)
        assert text in lib.bn_eval_last_error(), (call.__name__, kw, lib.bn_eval_last_error())
    assert lib.bn_eval_slip_workspace_bytes(2, 5000, 4, 6) == 2 * 2 * 24 * 8 * 8          # maps x slabs x groups x sums x 8 bytes
    assert lib.bn_eval_slip_workspace_bytes(1, 4096, 1, 1) == 64 and lib.bn_eval_slip_workspace_bytes(1, 4097, 1, 1) == 128
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 65, 1), (1, 1, 1, 65), (1, 1, 64, 9)):
        assert lib.bn_eval_slip_workspace_bytes(*bad) == 0, bad


def test_python_wrappers_check_their_arguments(monkeypatch):
    monkeypatch.setattr(EV, "resolve_device", lambda *a, **k: torch.device("cpu"))        # the checks below come before any launch
    one = torch.zeros(1, 4)
    with pytest.raises(ValueError, match="num_classes"):
        EV.confusion_matrix(one, one, 65)
    with pytest.raises(ValueError, match="bins"):
        EV.slip_metrics(one, one, one, one, one, one, 64, bins=9)
    with pytest.raises(ValueError, match="max_slope"):
        EV.slip_metrics(one, one, one, one, one, one, 4, max_slope=0.0)
    with pytest.raises(ValueError, match="risk must be"):
        EV.risk_calibration(torch.zeros(17, 1, 4), one, one, 4)


# ---- d. no fallback --------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_gpu():
    lib = _capi.load()
    for call in (_confusion_call, _slip_call, _risk_call):
        assert call(lib) == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_eval_last_error(), call.__name__
    one = torch.zeros(1, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EV.confusion_matrix(one, one, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EV.slip_metrics(one, one, one, one, one, one, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EV.risk_calibration(one[None], one, one, 2)


# ---- e. the report ---------------------------------------------------------------------------------------------------------------
def _report(**kw):
    sums, counts = np.zeros((3, 2, 8)), np.zeros((3, 2, 2), np.int64)
    sums[0, 0] = [2.0, 4.0, 8.0, 1.0, 2.0, 0.5, 3.0, 6.0]
    counts[0, 0] = [4, 3]
    sums[0, 1] = [-1.0, 1.0, 1.0, 1.0, 1.0, 0.25, 1.0, 2.0]
    counts[0, 1] = [1, 1]
    sums[2, 1] = [0.0, 0.0, 0.0, 0.5, 0.5, 0.0, -1.0, 2.0]
    counts[2, 1] = [2, 0]
    args = dict(num_classes=3, bins=2, max_slope=30.0, stuck_threshold=0.1, maps=1, cells=9, slip_sums=sums, slip_counts=counts, slip_invalid=2)
    args.update(kw)
    return EV.EvaluationReport(**args)


def test_report_classification():
    conf = np.array([[3, 1, 0], [2, 2, 0], [0, 0, 0]])                    # class 2 never occurs and is never predicted
    cl = _report(confusion=conf, ignored=1).summary()["classification"]
    assert cl["pixel_accuracy"] == 5 / 8 and cl["cells"] == 8 and cl["ignored"] == 1
    assert [r["precision"] for r in cl["per_class"]] == [3 / 5, 2 / 3, None]
    assert [r["recall"] for r in cl["per_class"]] == [3 / 4, 2 / 4, None]
    assert [r["iou"] for r in cl["per_class"]] == [3 / 6, 2 / 5, None]
    assert cl["mean_iou"] == (3 / 6 + 2 / 5) / 2                          # over the classes that occur
    assert _report().summary()["classification"] is None
    empty = _report(confusion=np.zeros((3, 3), np.int64)).summary()["classification"]
    assert empty["pixel_accuracy"] is None and empty["mean_iou"] is None


def test_report_slip_figures_and_none_rates():
    sl = _report().summary()["slip"]
    assert sl["cells"] == 7 and sl["invalid"] == 2 and sl["bin_edges"] == [0.0, 15.0, 30.0]
    b = {(r["class"], r["bin"]): r for r in sl["per_bin"]}
    assert b[0, 0] == {"class": 0, "bin": 0, "slope_from": 0.0, "slope_to": 15.0, "count": 4, "bias": 0.5, "mae": 1.0, "rmse": math.sqrt(2.0),
                       "mean_std": 0.25, "mean_latent_std": 0.5, "mean_kl": 0.125, "mean_nll": 0.75, "coverage_2sigma": 0.75, "mean_z2": 1.5}
    c0 = sl["per_class"][0]                                              # the class row: its bins' sums added, then divided
    assert (c0["count"], c0["bias"], c0["mae"], c0["rmse"], c0["coverage_2sigma"]) == (5, 1.0 / 5, 1.0, math.sqrt(9.0 / 5), 4 / 5)
    nothing = sl["per_class"][1]
    assert nothing["count"] == 0 and all(nothing[k] is None for k in ("bias", "mae", "rmse", "mean_std", "mean_kl", "mean_nll", "coverage_2sigma", "mean_z2"))
    assert b[2, 1]["mean_nll"] == -0.5 and b[2, 1]["coverage_2sigma"] == 0.0
    assert _report(has_slips=False).summary()["slip"]["per_bin"][0]["mean_nll"] is None


def test_report_risk_rates_and_json(tmp_path):
    rc = np.zeros((2, 3, 5), np.int64)
    rc[0, 0] = [2, 5, 1, 2, 2]                                           # exceed, safe&safe, SAFE&STUCK, stuck&safe, stuck&stuck
    rc[0, 1] = [1, 3, 0, 0, 0]
    rep = _report(settings=["expected_value", "var@0.9"], risk_counts=rc, risk_invalid=np.array([4, 0]))
    first, second = rep.summary()["risk"]
    assert first["setting"] == "expected_value" and first["cells"] == 13 and first["invalid"] == 4
    assert first["exceedance_rate"] == 3 / 13 and first["false_safe_rate"] == 1 / 3 and first["false_unsafe_rate"] == 2 / 10
    assert first["counts"]["safe_stuck"] == 1
    assert first["per_class"][1]["false_safe_rate"] is None and first["per_class"][1]["false_unsafe_rate"] == 0.0
    assert second["setting"] == "var@0.9" and second["cells"] == 0
    assert second["exceedance_rate"] is None and second["false_safe_rate"] is None and second["false_unsafe_rate"] is None
    assert _report().summary()["risk"] is None
    path = tmp_path / "sub" / "evaluation.json"
    rep.to_json(str(path))
    text = path.read_text()
    assert "NaN" not in text and json.loads(text) == json.loads(json.dumps(rep.to_dict()))
    tables = rep.to_dict()["tables"]                                   # self-contained: a report rebuilt from them summarises alike
    assert tables["slip_invalid"] == 2 and tables["risk_invalid"] == [4, 0] and tables["ignored"] is None and tables["confusion"] is None
    again = _report(slip_sums=np.array(tables["slip_sums"]), slip_counts=np.array(tables["slip_counts"]), slip_invalid=tables["slip_invalid"],
                    settings=rep.to_dict()["settings"], risk_counts=np.array(tables["risk_counts"]), risk_invalid=np.array(tables["risk_invalid"]))
    assert again.summary() == rep.summary()
    assert _report(confusion=np.eye(3, dtype=np.int64), ignored=5).to_dict()["tables"]["ignored"] == 5
    table = rep.table()
    assert "var@0.9" in table and "slip regressors" in table and "[0, 15)" in table
