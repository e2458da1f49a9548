"""GPU: Evaluator.run on a generated split of 5 maps at G = 32 (benchnav_amd/evaluate.py).

  - the latent model as the prediction: every bias, MAE, RMSE and mean KL is exactly 0.0 (mu - m = 0, log(1) = 0 and
    s^2 / (2 s^2) = 0.5 are exact), the predicted std sums are the latent ones;
  - a classifier stand-in that returns the true classes gives a diagonal confusion matrix, one that swaps two classes exactly the
    swapped counts;
  - chunk = 1, 2 and 5 give to_dict() equal bit for bit;
  - run(["expected_value", "var@0.9"]) equals tests/evaluate_spec.py fed with the same downloaded risk maps and observations;
  - a predictor stand-in with `predict_maps` and a `terrain_classifier` of its own (what Evaluator(split, predictor) calls on a
    TraversabilityPredictor) is walked chunk by chunk and equals the spec on the same predictions;
  - the exceedance rate under var@0.9 is printed, not asserted: about 0.1 on a calibrated prediction, but the 1000-sample quantile
    has an error of its own."""
import json
import warnings

import numpy as np
import pytest
import torch

import evaluate_spec as S

pytestmark = pytest.mark.gpu
G, RES, TOTAL, SELECTED, MAPS, SEED, NB = 32, 0.5, 4, 2, 5, 11, 6
SETTINGS = ["expected_value", "var@0.9"]


class _Truth:
    """A classifier stand-in: predict_classes returns the split's true classes of the maps it is asked for, in the order the
    evaluator walks them, with classes `a` and `b` swapped."""

    def __init__(self, split, swap=None):
        self.split, self.swap, self.at = split, swap, 0

    def predict_classes(self, colors):
        B = colors.shape[0]
        assert torch.equal(colors, self.split.colors[self.at:self.at + B])          # the evaluator asks in map order
        t = self.split.t_classes[self.at:self.at + B].clone()
        self.at = (self.at + B) % len(self.split)
        if self.swap is not None:
            a, b = self.swap
            t = torch.where(t == a, b, torch.where(t == b, a, t)).to(torch.int32)
        return t


@pytest.fixture(scope="module")
def split():
    from benchnav_amd.dataset import DatasetGenerator, ParamsTerrainGeometry
    from benchnav_amd.terrain import slip_models
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # craters that do not fit a 32 x 32 map
        data = DatasetGenerator(slip_models(TOTAL), None, "train", G, RES, MAPS, 1, num_total_terrain_classes=TOTAL, num_selected_terrain_classes=SELECTED,
                                params_terrain_geometry=ParamsTerrainGeometry(num_craters=2, min_radius=2, max_radius=4), batch=4).generate_dataset()
    data.observation_seed, data.epoch = 7, 3
    assert len(data) == MAPS
    return data


@pytest.fixture(scope="module")
def reports(split):
    """One run per chunk size with the risk settings and the true classes as the classifier's: shared, never changed."""
    from benchnav_amd.evaluate import Evaluator
    return {chunk: Evaluator(split, classifier=_Truth(split), num_classes=TOTAL, chunk=chunk, bins=NB, seed=SEED).run(SETTINGS) for chunk in (1, 2, 5)}


def test_latent_model_as_the_prediction_is_exact(reports):
    r = reports[5]
    assert r.slip_counts[..., 0].sum() + r.slip_invalid == MAPS * G * G and r.slip_counts[..., 0].sum() > 0
    sums = r.slip_sums
    assert not sums[..., 0].any() and not sums[..., 1].any() and not sums[..., 2].any()          # d, |d|, d^2: exactly 0.0
    assert not sums[..., 5].any()                                                                # KL: exactly 0.0
    assert np.array_equal(sums[..., 3].view(np.int64), sums[..., 4].view(np.int64))              # sum std == sum latent std
    rows = [x for x in r.summary()["slip"]["per_class"] + r.summary()["slip"]["per_bin"] if x["count"]]
    assert rows and all(x["bias"] == 0.0 and x["mae"] == 0.0 and x["rmse"] == 0.0 and x["mean_kl"] == 0.0 for x in rows)
    assert all(x["mean_std"] == x["mean_latent_std"] and x["mean_nll"] is not None and 0.0 <= x["coverage_2sigma"] <= 1.0 for x in rows)
    print("latent model against its own observations: " + ", ".join(f"class {x['class']}: in 2 std {x['coverage_2sigma']:.4f}, z^2 {x['mean_z2']:.3f}"
                                                                     for x in r.summary()["slip"]["per_class"] if x["count"]))


def test_classifier_stand_ins(split, reports):
    from benchnav_amd.evaluate import Evaluator
    true = split.t_classes.cpu().numpy().astype(np.int64)
    hist = np.bincount(true.ravel(), minlength=TOTAL)
    conf = reports[2].confusion
    assert np.array_equal(conf, np.diag(hist)) and reports[2].ignored == 0
    cl = reports[2].summary()["classification"]
    assert cl["pixel_accuracy"] == 1.0 and cl["mean_iou"] == 1.0
    assert [r["iou"] for r in cl["per_class"]] == [1.0 if n else None for n in hist]
    a, b = (int(c) for c in np.argsort(hist)[-2:])                       # the two classes with the most cells
    swapped = Evaluator(split, classifier=_Truth(split, swap=(a, b)), num_classes=TOTAL, chunk=2).run()
    want = np.diag(hist)
    want[a, a] = want[b, b] = 0
    want[a, b], want[b, a] = hist[a], hist[b]
    assert np.array_equal(swapped.confusion, want) and hist[a] > 0 and hist[b] > 0
    assert swapped.summary()["classification"]["pixel_accuracy"] == (hist.sum() - hist[a] - hist[b]) / hist.sum()
    assert swapped.risk_counts is None and swapped.summary()["risk"] is None


def test_report_does_not_depend_on_the_chunk(reports):
    docs = {chunk: json.dumps(r.to_dict(), sort_keys=True) for chunk, r in reports.items()}
    assert docs[1] == docs[2] == docs[5] and "NaN" not in docs[1]
    for chunk in (1, 2):
        assert np.array_equal(reports[chunk].slip_sums.view(np.int64), reports[5].slip_sums.view(np.int64))


def test_run_equals_the_spec_on_the_same_risk_maps_and_observations(split, reports):
    from benchnav_amd.benchmark import parse_setting, risk_seed
    from benchnav_amd.dataset import sample_slips
    from benchnav_amd.risk import infer_risk_maps
    r = reports[2]
    mean, std = split.latent_mean, split.latent_std
    risk = infer_risk_maps(mean, std, [parse_setting(s) for s in SETTINGS], num_samples=1000, seeds=[risk_seed(SEED, m) for m in range(MAPS)])
    y = sample_slips(mean, std, split.observation_seed, split.epoch)
    flat = lambda t: t.cpu().numpy().reshape(*t.shape[:-2], -1)          # (..., G, G) -> (..., cells)
    m, s, phi, cls = flat(mean), flat(std), flat(split.slopes), flat(split.t_classes)
    counts, invalid = S.risk(flat(risk), flat(y), cls, TOTAL, 0.1)
    assert np.array_equal(r.risk_counts, counts.sum(axis=0)) and np.array_equal(r.risk_invalid, invalid.sum(axis=0))
    want = S.slip(m, s, m, s, phi, cls, TOTAL, y=flat(y), bins=NB, max_slope=30.0)
    assert np.array_equal(r.slip_counts, want["counts"].sum(axis=0)) and r.slip_invalid == want["invalid"].sum()
    total = S.slip_total(want["sums"])
    for k, name in enumerate(S.SUM_NAMES):
        if k in S.LOG_SUMS:
            err = np.abs(r.slip_sums[..., k] - total[..., k])
            bound = S.metric_bound(want["magnitude"][..., S.LOG_SUMS.index(k)].sum(axis=0), want["counts"][..., 0].sum(axis=0))
            print(f"sum {name}: bit-equal {np.array_equal(r.slip_sums[..., k].view(np.int64), total[..., k].view(np.int64))}, max |device - spec| {err.max():.3g}")
            assert (err <= bound).all(), name
        else:
            assert np.array_equal(r.slip_sums[..., k].view(np.int64), total[..., k].view(np.int64)), name
    rows = {x["setting"]: x for x in r.summary()["risk"]}
    print(f"exceedance rate under var@0.9: {rows['var@0.9']['exceedance_rate']:.4f} (about 0.1 on a calibrated prediction); under expected_value: "
          f"{rows['expected_value']['exceedance_rate']:.4f}; false-safe rates {rows['expected_value']['false_safe_rate']}, {rows['var@0.9']['false_safe_rate']}")
    assert rows["var@0.9"]["cells"] == counts[:, 1, :, 1:].sum() > 0


class _Predictor:
    """A predictor stand-in with the two calls the evaluator makes on a TraversabilityPredictor -- `predict_maps(slopes, colors=...)`
    and `terrain_classifier.predict_classes(colors)` -- whose prediction is the latent model shifted and widened (float64 out,
    as predict_maps may return)."""

    def __init__(self, split, swap):
        self.split, self.at, self.terrain_classifier = split, 0, _Truth(split, swap=swap)

    def predict_maps(self, slopes, colors=None):
        B = slopes.shape[0]
        assert colors is not None and torch.equal(slopes, self.split.slopes[self.at:self.at + B]) and colors.shape[0] == B
        sl = slice(self.at, self.at + B)
        self.at = (self.at + B) % len(self.split)
        return (self.split.latent_mean[sl] + 0.0625).to(torch.float64), (self.split.latent_std[sl] * 2.0).to(torch.float64)


def test_a_predictor_s_own_classifier_and_predict_maps_are_used(split):
    """Evaluator(split, predictor): classes from predictor.terrain_classifier, (mean, std) from predictor.predict_maps on slopes and
    colours, chunk by chunk; equal to the spec on the same predictions, for two chunk sizes."""
    from benchnav_amd.dataset import sample_slips
    from benchnav_amd.evaluate import Evaluator
    hist = np.bincount(split.t_classes.cpu().numpy().ravel(), minlength=TOTAL)
    a, b = (int(c) for c in np.argsort(hist)[-2:])
    runs = [Evaluator(split, _Predictor(split, (a, b)), num_classes=TOTAL, chunk=chunk, bins=NB, seed=SEED).run(["var@0.9"]) for chunk in (2, 5)]
    assert json.dumps(runs[0].to_dict(), sort_keys=True) == json.dumps(runs[1].to_dict(), sort_keys=True)
    r = runs[0]
    assert r.confusion[a, b] == hist[a] and r.confusion[b, a] == hist[b] and r.confusion[a, a] == 0          # the predictor's classifier
    flat = lambda t: t.cpu().numpy().reshape(*t.shape[:-2], -1)
    mean, std = (split.latent_mean + 0.0625).to(torch.float32), (split.latent_std * 2.0).to(torch.float32)
    y = sample_slips(split.latent_mean, split.latent_std, split.observation_seed, split.epoch)
    want = S.slip(flat(mean), flat(std), flat(split.latent_mean), flat(split.latent_std), flat(split.slopes), flat(split.t_classes), TOTAL,
                  y=flat(y), bins=NB, max_slope=30.0)
    total = S.slip_total(want["sums"])
    assert np.array_equal(r.slip_counts, want["counts"].sum(axis=0)) and r.slip_invalid == want["invalid"].sum()
    for k, name in enumerate(S.SUM_NAMES):
        if k in S.LOG_SUMS:
            bound = S.metric_bound(want["magnitude"][..., S.LOG_SUMS.index(k)].sum(axis=0), want["counts"][..., 0].sum(axis=0))
            assert (np.abs(r.slip_sums[..., k] - total[..., k]) <= bound).all(), name
        else:
            assert np.array_equal(r.slip_sums[..., k].view(np.int64), total[..., k].view(np.int64)), name
    rows = [x for x in r.summary()["slip"]["per_class"] if x["count"]]
    assert rows and all(abs(x["bias"] - 0.0625) < 1e-6 and x["mean_std"] > x["mean_latent_std"] for x in rows)
    assert r.risk_counts[0, :, 1:].sum() + r.risk_invalid[0] == MAPS * G * G
