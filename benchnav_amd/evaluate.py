"""The model-evaluation stage on the device: how good are the models the planners drive on?

    report = Evaluator(test_split, predictor, num_classes=10).run(["expected_value", "var@0.9"])
    print(report.table()); report.to_json("evaluation.json")

Three questions, three reductions over arrays that already sit on the device (csrc/eval_kernels.hip), each one pass:

  confusion_matrix   does the classifier confuse terrain classes?  (true, predicted) counts per map;
  slip_metrics       is the regressor biased, or over-confident on steep slopes?  The predicted N(mean, std^2) against the latent
                     N(latent_mean, latent_std^2) and one observation per cell, per (true class, slope bin): the numbers behind the
                     reference's scripts/test_slip_regressors.py plot;
  risk_calibration   does a risk map call cells safe where the rover then gets stuck?  Per (risk setting, true class) how often the
                     observation exceeds the risk, and the 2 x 2 table of (believed stuck, actually stuck) in the environment
                     step's float32 arithmetic.

The three functions are thin wrappers that return device tensors.  `Evaluator.run` walks a split `chunk` maps at a time without a
host synchronise per map and downloads once; its report is bit-identical for any `chunk`: every count is an integer and the float64
sums are added in an order that depends on the cell and the map index alone.  `EvaluationReport`'s arithmetic needs no device.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._device import check, resolve_device, stream_ptr
from .benchmark import parse_setting, risk_seed, setting_name
from .dataset import MAX_CLASSES

MAX_BINS, MAX_GROUPS = _capi.BN_EVAL_MAX_BINS, _capi.BN_EVAL_MAX_GROUPS
# the float64 sums of a (class, slope bin) group, in the order of the kernel's table, and its two integer counts
SLIP_SUMS = ("d", "abs_d", "d2", "sigma", "s", "kl", "nll", "z2")
SLIP_COUNTS = ("count", "covered")
# the integer counts of a (setting, class): y above the risk, then [1 + 2 * believed stuck + actually stuck]
RISK_COUNTS = ("exceed", "safe_safe", "safe_stuck", "stuck_safe", "stuck_stuck")


# ---- the three device reductions ---------------------------------------------------------------------------------------------------
def _raise(lib, code: int) -> None:
    if code == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_eval_last_error().decode("utf-8", "replace"))
    check(lib, "eval", code)


def _device_of(device, *tensors) -> torch.device:
    src = next((t for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), None)
    return resolve_device(device if device is not None else (src.device if src is not None else None), "evaluate")


def _maps(t, dev: torch.device, dtype, name: str, shape=None) -> torch.Tensor:
    t = torch.as_tensor(t)
    if t.dim() < 2:
        raise ValueError(f"{name} must be (M, ...) maps, got shape {tuple(t.shape)}")
    t = t.detach().to(dev, dtype).reshape(t.shape[0], -1).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must hold {shape[0]} maps of {shape[1]} cells, got {tuple(t.shape)}")
    return t


def _classes(num_classes) -> int:
    Cn = int(num_classes)
    if Cn < 1 or Cn > MAX_CLASSES:
        raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}]")
    return Cn


_p = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def confusion_matrix(pred_classes, true_classes, num_classes: int, device=None) -> Dict[str, torch.Tensor]:
    """{"table": (M, C, C) int64 indexed [true][predicted], "ignored": (M,) int64} on the device, one launch on torch's current
    stream (bn_eval_confusion_async).  pred_classes, true_classes: (M, ...) integer class maps; a cell with either class outside
    [0, C) is counted in `ignored` and in no table entry."""
    dev = _device_of(device, pred_classes, true_classes)
    lib, Cn = _capi.load(), _classes(num_classes)
    with torch.cuda.device(dev):
        tr = _maps(true_classes, dev, torch.int32, "true_classes")
        pr = _maps(pred_classes, dev, torch.int32, "pred_classes", tr.shape)
        M, cells = tr.shape
        out = {"table": torch.empty(M, Cn, Cn, device=dev, dtype=torch.int64), "ignored": torch.empty(M, device=dev, dtype=torch.int64)}
        _raise(lib, lib.bn_eval_confusion_async(dev.index, stream_ptr(dev), _p(tr), _p(pr), M, cells, Cn, _p(out["table"]), _p(out["ignored"])))
    return out


def slip_metrics(mean, std, latent_mean, latent_std, classes, slopes, num_classes: int, slips=None, bins: int = 6, max_slope: float = 30.0,
                 total: Optional[torch.Tensor] = None, device=None) -> Dict[str, torch.Tensor]:
    """The predicted slip N(mean, std^2) against the latent N(latent_mean, latent_std^2) and, with `slips`, one observation per cell,
    grouped by (true class, slope bin): {"sums": (M, C, bins, 8) float64 in SLIP_SUMS' order, "counts": (M, C, bins, 2) int64 in
    SLIP_COUNTS' order, "invalid": (M,) int64} on the device (bn_eval_slip_async; the header defines every sum).

    `bins` equal bins over [0, max_slope], closed on the left; a slope below 0 falls in the first, one at or above max_slope in
    the last.  A cell whose class is out of range, whose slope, mean, std, latent mean, latent std or slip is not finite, or whose
    std or latent std is <= 0 (a class without a regressor predicts std = 0) is counted in `invalid` and enters nothing else.
    `total`: a (C, bins, 8) float64 device tensor the maps' sums are added onto in map order, so that calls over successive runs of
    maps leave the bits one call over all of them leaves."""
    dev = _device_of(device, mean, latent_mean)
    lib, Cn, NB = _capi.load(), _classes(num_classes), int(bins)
    if NB < 1 or NB > MAX_BINS or Cn * NB > MAX_GROUPS:
        raise ValueError(f"bins must be in [1, {MAX_BINS}] with num_classes * bins <= {MAX_GROUPS}")
    if not (float(max_slope) > 0.0 and math.isfinite(float(max_slope))):
        raise ValueError("max_slope must be > 0 and finite")
    with torch.cuda.device(dev):
        mu = _maps(mean, dev, torch.float32, "mean")
        M, cells = mu.shape
        sd, lm, ls, ph = (_maps(t, dev, torch.float32, n, mu.shape) for t, n in ((std, "std"), (latent_mean, "latent_mean"),
                                                                                 (latent_std, "latent_std"), (slopes, "slopes")))
        cl = _maps(classes, dev, torch.int32, "classes", mu.shape)
        y = None if slips is None else _maps(slips, dev, torch.float32, "slips", mu.shape)
        if total is not None and (not total.is_cuda or total.dtype != torch.float64 or tuple(total.shape) != (Cn, NB, len(SLIP_SUMS))
                                  or not total.is_contiguous()):
            raise ValueError(f"total must be a contiguous ({Cn}, {NB}, {len(SLIP_SUMS)}) float64 device tensor")
        out = {"sums": torch.empty(M, Cn, NB, len(SLIP_SUMS), device=dev, dtype=torch.float64),
               "counts": torch.empty(M, Cn, NB, len(SLIP_COUNTS), device=dev, dtype=torch.int64),
               "invalid": torch.empty(M, device=dev, dtype=torch.int64)}
        nbytes = lib.bn_eval_slip_workspace_bytes(M, cells, Cn, NB)
        if nbytes == 0:
            raise ValueError(f"{M} maps of {cells} cells are out of the library's range")
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)          # torch's allocator keeps it alive for the stream
        _raise(lib, lib.bn_eval_slip_async(dev.index, stream_ptr(dev), _p(mu), _p(sd), _p(lm), _p(ls), _p(ph), _p(cl), _p(y), M, cells, Cn, NB,
                                           float(max_slope), _p(out["sums"]), _p(out["counts"]), _p(out["invalid"]), _p(total), _p(work), nbytes))
    return out


def risk_calibration(risk, slips, classes, num_classes: int, stuck_threshold: float = 0.1, device=None) -> Dict[str, torch.Tensor]:
    """Risk maps against what the environment would draw: risk (S, M, ...) float32, the tensor Benchmark.risk_maps returns; slips
    and classes (M, ...).  {"counts": (M, S, C, 5) int64 in RISK_COUNTS' order, "invalid": (M, S) int64} on the device, one launch
    for all S settings (bn_eval_risk_async).  stuck(v) = 1 - clamp(v, 0, 1) <= stuck_threshold in float32, the environment step's
    rule; "safe_stuck" counts the cells the planner believes safe where the rover gets stuck.  A cell whose class is out of range
    or whose slip or risk is not finite is counted in `invalid` of its setting."""
    dev = _device_of(device, risk, slips)
    lib, Cn = _capi.load(), _classes(num_classes)
    r = torch.as_tensor(risk)
    if r.dim() < 3 or not 1 <= r.shape[0] <= _capi.BN_RISK_MAX_SETTINGS:
        raise ValueError(f"risk must be (S, M, ...) with S in [1, {_capi.BN_RISK_MAX_SETTINGS}], got {tuple(r.shape)}")
    if not math.isfinite(float(stuck_threshold)):
        raise ValueError("stuck_threshold must be finite")
    with torch.cuda.device(dev):
        y = _maps(slips, dev, torch.float32, "slips")
        M, cells = y.shape
        S = int(r.shape[0])
        if r.numel() != S * M * cells:
            raise ValueError(f"risk must hold {S} settings of {M} maps of {cells} cells, got {tuple(r.shape)}")
        r = r.detach().to(dev, torch.float32).reshape(S, M, cells).contiguous()
        cl = _maps(classes, dev, torch.int32, "classes", y.shape)
        out = {"counts": torch.empty(M, S, Cn, len(RISK_COUNTS), device=dev, dtype=torch.int64),
               "invalid": torch.empty(M, S, device=dev, dtype=torch.int64)}
        _raise(lib, lib.bn_eval_risk_async(dev.index, stream_ptr(dev), _p(r), _p(y), _p(cl), S, M, cells, Cn, float(stuck_threshold),
                                           _p(out["counts"]), _p(out["invalid"])))
    return out


# ---- the report --------------------------------------------------------------------------------------------------------------------
def _rate(num, den) -> Optional[float]:
    """num / den, or None over nothing."""
    return float(num) / float(den) if den else None


def _slip_row(sums: np.ndarray, counts: np.ndarray, has_slips: bool) -> dict:
    n, covered = int(counts[0]), int(counts[1])
    mean = lambda v: _rate(v, n)
    mse = mean(sums[2])
    obs = lambda v: v if has_slips else None
    return {"count": n, "bias": mean(sums[0]), "mae": mean(sums[1]), "rmse": None if mse is None else math.sqrt(mse),
            "mean_std": mean(sums[3]), "mean_latent_std": mean(sums[4]), "mean_kl": mean(sums[5]), "mean_nll": obs(mean(sums[6])),
            "coverage_2sigma": obs(_rate(covered, n)), "mean_z2": obs(mean(sums[7]))}


def _risk_row(counts: np.ndarray, invalid: Optional[int] = None) -> dict:
    exceed, ss, sk, ks, kk = (int(v) for v in counts)
    n = ss + sk + ks + kk
    row = {"cells": n, "exceedance_rate": _rate(exceed, n), "false_safe_rate": _rate(sk, sk + kk), "false_unsafe_rate": _rate(ks, ss + ks),
           "counts": dict(zip(RISK_COUNTS, (exceed, ss, sk, ks, kk)))}
    if invalid is not None:
        row["invalid"] = int(invalid)
    return row


class EvaluationReport:
    """What an evaluation counted, summed over the maps of a split, and the figures that follow from it.

    confusion (C, C) int64 [true][predicted] with `ignored`, or None without a classifier; slip_sums (C, bins, 8) float64 and
    slip_counts (C, bins, 2) int64 in SLIP_SUMS' / SLIP_COUNTS' order with `slip_invalid`; risk_counts (S, C, 5) int64 in
    RISK_COUNTS' order with risk_invalid (S,), or None without settings.  Every rate over nothing is None, never NaN.

    Rates of the risk figures: exceedance = cells whose observed slip lies above the risk / valid cells (near 1 - q for var@q on a
    calibrated prediction); false safe = believed safe and actually stuck / actually stuck; false unsafe = believed stuck and
    actually safe / actually safe."""

    def __init__(self, num_classes: int, bins: int, max_slope: float, stuck_threshold: float, maps: int, cells: int,
                 slip_sums: np.ndarray, slip_counts: np.ndarray, slip_invalid: int, confusion: Optional[np.ndarray] = None, ignored: int = 0,
                 settings: Sequence = (), risk_counts: Optional[np.ndarray] = None, risk_invalid: Optional[np.ndarray] = None,
                 has_slips: bool = True, seed: int = 0, num_samples: int = 1000, chunk: Optional[int] = None) -> None:
        self.num_classes, self.bins, self.max_slope, self.stuck_threshold = int(num_classes), int(bins), float(max_slope), float(stuck_threshold)
        self.maps, self.cells, self.seed, self.num_samples, self.chunk = int(maps), int(cells), int(seed), int(num_samples), chunk
        self.slip_sums, self.slip_counts = np.asarray(slip_sums, np.float64), np.asarray(slip_counts, np.int64)
        self.slip_invalid, self.has_slips = int(slip_invalid), bool(has_slips)
        self.confusion = None if confusion is None else np.asarray(confusion, np.int64)
        self.ignored = int(ignored)
        self.settings = [parse_setting(s) for s in settings]
        self.risk_counts = None if risk_counts is None else np.asarray(risk_counts, np.int64)
        self.risk_invalid = None if risk_invalid is None else np.asarray(risk_invalid, np.int64)

    # -- the figures --
    def classification(self) -> Optional[dict]:
        """Pixel accuracy, per-class precision, recall and IoU, the mean IoU over the classes that occur (as a true class)."""
        if self.confusion is None:
            return None
        t = self.confusion
        diag, true_n, pred_n = np.diag(t), t.sum(axis=1), t.sum(axis=0)
        per_class = [{"class": c, "support": int(true_n[c]), "predicted": int(pred_n[c]), "precision": _rate(diag[c], pred_n[c]),
                      "recall": _rate(diag[c], true_n[c]), "iou": _rate(diag[c], true_n[c] + pred_n[c] - diag[c])} for c in range(self.num_classes)]
        occurring = [r["iou"] for r in per_class if r["support"] > 0]
        return {"cells": int(t.sum()), "ignored": self.ignored, "pixel_accuracy": _rate(diag.sum(), t.sum()),
                "mean_iou": sum(occurring) / len(occurring) if occurring else None, "per_class": per_class}

    def slip(self) -> dict:
        """Per class (its bins' sums added in bin order) and per (class, bin): bias, MAE and RMSE of the predicted mean against the
        latent one, the mean predicted std against the mean latent std, the mean KL(latent || predicted), and against the
        observations the mean NLL, the share within 2 std and the mean z^2 (1 on a calibrated prediction)."""
        edges = [self.max_slope * j / self.bins for j in range(self.bins + 1)]
        per_class, per_bin = [], []
        for c in range(self.num_classes):
            total, counts = np.zeros(len(SLIP_SUMS)), np.zeros(len(SLIP_COUNTS), np.int64)
            for j in range(self.bins):
                total, counts = total + self.slip_sums[c, j], counts + self.slip_counts[c, j]
                per_bin.append({"class": c, "bin": j, "slope_from": edges[j], "slope_to": edges[j + 1],
                                **_slip_row(self.slip_sums[c, j], self.slip_counts[c, j], self.has_slips)})
            per_class.append({"class": c, **_slip_row(total, counts, self.has_slips)})
        return {"cells": int(self.slip_counts[..., 0].sum()), "invalid": self.slip_invalid, "bin_edges": edges, "per_class": per_class,
                "per_bin": per_bin}

    def risk(self) -> Optional[List[dict]]:
        if self.risk_counts is None:
            return None
        return [{"setting": setting_name(s), **_risk_row(self.risk_counts[k].sum(axis=0), self.risk_invalid[k]),
                 "per_class": [{"class": c, **_risk_row(self.risk_counts[k, c])} for c in range(self.num_classes)]}
                for k, s in enumerate(self.settings)]

    def summary(self) -> dict:
        return {"classification": self.classification(), "slip": self.slip(), "risk": self.risk()}

    def table(self) -> str:
        fmt = lambda v, w, p: f"{'-':>{w}}" if v is None else f"{v:>{w}.{p}f}"
        s = self.summary()
        lines = []
        if s["classification"] is not None:
            cl = s["classification"]
            lines += [f"classifier: pixel accuracy {fmt(cl['pixel_accuracy'], 0, 4).strip()}, mean IoU {fmt(cl['mean_iou'], 0, 4).strip()} "
                      f"over {cl['cells']} cells ({cl['ignored']} ignored)",
                      f"{'class':<8}{'cells':>10}{'precision':>11}{'recall':>9}{'IoU':>9}"]
            lines += [f"{r['class']:<8}{r['support']:>10}{fmt(r['precision'], 11, 4)}{fmt(r['recall'], 9, 4)}{fmt(r['iou'], 9, 4)}" for r in cl["per_class"]]
            lines.append("")
        sl = s["slip"]
        head = f"{'cells':>10}{'bias':>10}{'MAE':>9}{'RMSE':>9}{'std':>9}{'lat std':>9}{'KL':>10}{'NLL':>10}{'in 2std':>9}{'z^2':>9}"
        cols = lambda r: (f"{r['count']:>10}{fmt(r['bias'], 10, 4)}{fmt(r['mae'], 9, 4)}{fmt(r['rmse'], 9, 4)}{fmt(r['mean_std'], 9, 4)}"
                          f"{fmt(r['mean_latent_std'], 9, 4)}{fmt(r['mean_kl'], 10, 4)}{fmt(r['mean_nll'], 10, 4)}{fmt(r['coverage_2sigma'], 9, 4)}"
                          f"{fmt(r['mean_z2'], 9, 3)}")
        lines += [f"slip regressors: {sl['cells']} cells ({sl['invalid']} invalid)", f"{'class':<16}" + head]
        for r in sl["per_class"]:
            if r["count"]:
                lines.append(f"{r['class']:<16}" + cols(r))
                lines += [f"  {'[%g, %g)' % (b['slope_from'], b['slope_to']):<14}" + cols(b) for b in sl["per_bin"] if b["class"] == r["class"] and b["count"]]
        if s["risk"] is not None:
            lines += ["", f"risk maps (stuck threshold {self.stuck_threshold:g})",
                      f"{'setting':<16}{'cells':>10}{'exceed':>9}{'false safe':>12}{'false unsafe':>14}{'safe&stuck':>12}"]
            lines += [f"{r['setting']:<16}{r['cells']:>10}{fmt(r['exceedance_rate'], 9, 4)}{fmt(r['false_safe_rate'], 12, 4)}"
                      f"{fmt(r['false_unsafe_rate'], 14, 4)}{r['counts']['safe_stuck']:>12}" for r in s["risk"]]
        return "\n".join(lines)

    def to_dict(self) -> dict:
        doc = {"num_classes": self.num_classes, "bins": self.bins, "max_slope": self.max_slope, "stuck_threshold": self.stuck_threshold,
               "maps": self.maps, "cells": self.cells, "seed": self.seed, "num_samples": self.num_samples,
               "settings": [setting_name(s) for s in self.settings], "summary": self.summary(),
               "tables": {"slip_sum_names": list(SLIP_SUMS), "slip_sums": self.slip_sums.tolist(), "slip_count_names": list(SLIP_COUNTS),
                          "slip_counts": self.slip_counts.tolist(), "slip_invalid": self.slip_invalid,
                          "confusion": None if self.confusion is None else self.confusion.tolist(),
                          "ignored": None if self.confusion is None else self.ignored,
                          "risk_count_names": list(RISK_COUNTS), "risk_counts": None if self.risk_counts is None else self.risk_counts.tolist(),
                          "risk_invalid": None if self.risk_invalid is None else self.risk_invalid.tolist()}}
        return doc

    def to_json(self, path: str) -> None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=1)
            f.write("\n")


# ---- the driver --------------------------------------------------------------------------------------------------------------------
class Evaluator:
    def __init__(self, dataset, predictor=None, classifier=None, num_classes: Optional[int] = None, chunk: int = 64, bins: int = 6,
                 max_slope: float = 30.0, stuck_threshold: float = 0.1, seed: int = 0, num_samples: int = 1000) -> None:
        """dataset: a dataset.TerrainDataset (the test split).  predictor: a gp.TraversabilityPredictor, asked for `chunk` maps per
        predict_maps call on colours and slopes; None takes the latent model as the prediction, as Benchmark.predictions does.
        classifier: anything with `.predict_classes(colors (B, 3, G, G)) -> (B, G, G)` integer classes; None takes the
        predictor's, and without either no confusion matrix is made.  num_classes: of the class maps (None: the largest true
        class + 1, one download).  seed, num_samples: of the risk maps, seeded per map by Benchmark's rule `risk_seed`."""
        self.dataset, self.predictor = dataset, predictor
        self.classifier = classifier if classifier is not None else getattr(predictor, "terrain_classifier", None)
        if self.classifier is not None and not hasattr(self.classifier, "predict_classes"):
            raise ValueError("the classifier must have predict_classes(colors)")
        self.M, self.G = len(dataset), dataset.grid_size
        if self.M < 1:
            raise ValueError("the split is empty")
        self.chunk, self.bins, self.max_slope = int(chunk), int(bins), float(max_slope)
        if self.chunk < 1:
            raise ValueError("chunk must be >= 1")
        self.stuck_threshold, self.seed, self.num_samples = float(stuck_threshold), int(seed), int(num_samples)
        self.dev = resolve_device(dataset.device if dataset.device.type == "cuda" else None, "evaluate")
        self.num_classes = _classes(int(dataset.t_classes.max()) + 1 if num_classes is None else num_classes)

    def run(self, settings=None) -> EvaluationReport:
        """The whole split, `chunk` maps at a time, in map order; with `settings` ('expected_value', 'var@0.9', ... as
        Benchmark.run takes them) also the risk maps' calibration.  Nothing is downloaded before the last chunk is enqueued."""
        from .dataset import sample_slips
        from .risk import infer_risk_maps
        settings = [parse_setting(s) for s in settings] if settings else []
        ds, dev, Cn, NB = self.dataset, self.dev, self.num_classes, self.bins
        with torch.cuda.device(dev):
            zeros = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.int64)
            slip_total = torch.zeros(Cn, NB, len(SLIP_SUMS), device=dev, dtype=torch.float64)
            slip_counts, slip_invalid = zeros(Cn, NB, len(SLIP_COUNTS)), zeros(())
            confusion, ignored = (zeros(Cn, Cn), zeros(())) if self.classifier is not None else (None, None)
            risk_counts, risk_invalid = (zeros(len(settings), Cn, len(RISK_COUNTS)), zeros(len(settings))) if settings else (None, None)
            for m0 in range(0, self.M, self.chunk):
                sl = slice(m0, min(m0 + self.chunk, self.M))
                true = ds.t_classes[sl].to(dev)
                lat_mean, lat_std = ds.latent_mean[sl].to(dev, torch.float32), ds.latent_std[sl].to(dev, torch.float32)
                slopes = ds.slopes[sl].to(dev)
                if self.classifier is not None:
                    pred = torch.as_tensor(self.classifier.predict_classes(ds.colors[sl].to(dev))).reshape(true.shape)
                    out = confusion_matrix(pred, true, Cn, device=dev)
                    confusion += out["table"].sum(dim=0)
                    ignored += out["ignored"].sum()
                if self.predictor is None:
                    mean, std = lat_mean, lat_std
                else:
                    mean, std = self.predictor.predict_maps(slopes, colors=ds.colors[sl].to(dev))
                    mean, std = mean.to(torch.float32), std.to(torch.float32)
                slips = sample_slips(lat_mean, lat_std, ds.observation_seed, ds.epoch, first_map=m0, device=dev)
                out = slip_metrics(mean, std, lat_mean, lat_std, true, slopes, Cn, slips=slips, bins=NB, max_slope=self.max_slope,
                                   total=slip_total, device=dev)
                slip_counts += out["counts"].sum(dim=0)
                slip_invalid += out["invalid"].sum()
                if settings:
                    risk = infer_risk_maps(mean, std, settings, num_samples=self.num_samples,
                                           seeds=[risk_seed(self.seed, m) for m in range(sl.start, sl.stop)], device=dev)
                    out = risk_calibration(risk, slips, true, Cn, self.stuck_threshold, device=dev)
                    risk_counts += out["counts"].sum(dim=0)
                    risk_invalid += out["invalid"].sum(dim=0)
            # the one download: every table as 64-bit words (the float64 sums bit for bit), cut up again on the host
            parts = [slip_total.view(torch.int64), slip_counts, slip_invalid, confusion, ignored, risk_counts, risk_invalid]
            words = torch.cat([t.reshape(-1) for t in parts if t is not None]).cpu().numpy()
        host, at = [], 0
        for t in parts:
            host.append(None if t is None else words[at:at + t.numel()].reshape(tuple(t.shape)))
            at += 0 if t is None else t.numel()
        return EvaluationReport(Cn, NB, self.max_slope, self.stuck_threshold, self.M, self.G * self.G, host[0].view(np.float64), host[1],
                                int(host[2]), confusion=host[3], ignored=0 if host[4] is None else int(host[4]), settings=settings,
                                risk_counts=host[5], risk_invalid=host[6], has_slips=True, seed=self.seed, num_samples=self.num_samples,
                                chunk=self.chunk)
