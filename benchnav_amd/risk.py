"""Risk-map precompute on the GPU: mirror of TraversabilityModel._infer_risk_map
(reference src/simulator/problem_formulation/traversability_model.py:28-51)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._device import check, resolve_device

_METRICS = {"expected_value": _capi.BN_RISK_EXPECTED, "var": _capi.BN_RISK_VAR, "cvar": _capi.BN_RISK_CVAR}


def _check_setting(inference_metric: str, confidence_value: Optional[float]) -> None:
    """ModelConfig's checks (problem_formulation/utils.py:27-33)."""
    if inference_metric not in _METRICS:
        raise AssertionError(f"inference_metric must be one of {list(_METRICS)}")
    if inference_metric != "expected_value":
        assert confidence_value is not None and 0.0 <= confidence_value <= 1.0, \
            "confidence_value must be set between 0 and 1 when inference_metric is 'var' or 'cvar'."


def infer_risk_maps(mean: torch.Tensor, std: torch.Tensor, settings: Sequence[Tuple[str, Optional[float]]], num_samples: int = 1000,
                    seeds=None, z: Optional[torch.Tensor] = None, device: Optional[torch.device] = None) -> torch.Tensor:
    """(C, M, G, G) risk maps of M predicted slip distributions under C risk settings, in one launch on torch's current stream.

    mean, std: (M, G, G).  settings: up to 16 (inference_metric, confidence_value) pairs, each checked like infer_risk_map's
    arguments.  seeds: (M,) integers in [0, 2^64), one Philox seed per map (None: 0 for every map).  z: optional
    (M, num_samples, G, G) injected draws.  Every cell's samples are drawn once and every setting is evaluated on them:
    out[c, m] is bit for bit infer_risk_map(mean[m], std[m], *settings[c], num_samples, seed=seeds[m]) (or z=z[m])."""
    settings = [tuple(s) for s in settings]
    for metric, q in settings:
        _check_setting(metric, q)
    if not 1 <= len(settings) <= _capi.BN_RISK_MAX_SETTINGS:
        raise ValueError(f"settings must hold between 1 and {_capi.BN_RISK_MAX_SETTINGS} pairs, got {len(settings)}")
    dev = resolve_device(device, "risk")
    if mean.dim() != 3 or mean.shape[1] != mean.shape[2] or std.shape != mean.shape:
        raise ValueError(f"mean and std must be (M, G, G), got {tuple(mean.shape)} and {tuple(std.shape)}")
    M, G = int(mean.shape[0]), int(mean.shape[1])
    n, Cn = int(num_samples), len(settings)
    if seeds is None:
        seed_host = np.zeros(M, np.uint64)
    else:
        vals = [int(s) for s in (seeds.tolist() if hasattr(seeds, "tolist") else seeds)]
        if len(vals) != M or any(s < 0 or s >= 1 << 64 for s in vals):
            raise ValueError(f"seeds must be {M} integers in [0, 2^64)")
        seed_host = np.array(vals, np.uint64)
    metrics = (C.c_int * Cn)(*[_METRICS[m] for m, _ in settings])
    conf = (C.c_float * Cn)(*[float(q or 0.0) for _, q in settings])
    lib = _capi.load()
    with torch.cuda.device(dev):
        m = mean.detach().to(dev, torch.float32).contiguous()
        s = std.detach().to(dev, torch.float32).contiguous()
        zd = None
        if z is not None:
            if tuple(z.shape) != (M, n, G, G):
                raise ValueError(f"z must be (M, num_samples, G, G) = {(M, n, G, G)}, got {tuple(z.shape)}")
            zd = z.detach().to(dev, torch.float32).contiguous()
        sd = torch.from_numpy(seed_host.view(np.int64)).to(dev)            # the bit patterns: torch has no uint64 arithmetic to lose
        out = torch.empty(Cn, M, G, G, device=dev, dtype=torch.float32)
        rc = lib.bn_risk_maps_infer(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.c_void_p(m.data_ptr()),
                                    C.c_void_p(s.data_ptr()), M, G, metrics, conf, Cn, n,
                                    C.c_void_p(zd.data_ptr() if zd is not None else None), C.c_void_p(sd.data_ptr()),
                                    C.c_void_p(out.data_ptr()))
    if rc == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_risk_last_error().decode("utf-8", "replace"))
    check(lib, "risk", rc)
    return out


def infer_risk_map(mean: torch.Tensor, std: torch.Tensor, inference_metric: str, confidence_value: Optional[float] = None,
                   num_samples: int = 1000, z: Optional[torch.Tensor] = None, seed: int = 0,
                   device: Optional[torch.device] = None) -> torch.Tensor:
    """(G,G) risk map from the predicted slip distribution Normal(mean, std).

    inference_metric / confidence_value follow ModelConfig (problem_formulation/utils.py:10-40).
    z: optional (num_samples, G, G) standard normals -- pass the reference's own draw
    (`torch.empty(n, G, G).normal_()`) to reproduce its map; None samples inside the kernel.
    Returns a float32 tensor on the GPU.  Raises without a GPU (no CPU fallback).
    """
    if inference_metric not in _METRICS:
        raise AssertionError(f"inference_metric must be one of {list(_METRICS)}")
    if inference_metric != "expected_value":
        assert confidence_value is not None and 0.0 <= confidence_value <= 1.0, \
            "confidence_value must be set between 0 and 1 when inference_metric is 'var' or 'cvar'."
    dev = resolve_device(device, "risk")
    G = mean.shape[0]
    assert mean.shape == (G, G) and std.shape == (G, G)
    m = mean.detach().to(dev, torch.float32).contiguous()
    s = std.detach().to(dev, torch.float32).contiguous()
    out = torch.empty(G, G, device=dev, dtype=torch.float32)
    zd = None
    if z is not None:
        assert z.shape == (num_samples, G, G)
        zd = z.detach().to(dev, torch.float32).contiguous()
    lib = _capi.load()
    with torch.cuda.device(dev):
        rc = lib.bn_risk_map_infer(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream),
                                   C.c_void_p(m.data_ptr()), C.c_void_p(s.data_ptr()), _capi.BN_MEM_DEVICE, G,
                                   _METRICS[inference_metric], float(confidence_value or 0.0), int(num_samples),
                                   C.c_void_p(zd.data_ptr() if zd is not None else None), _capi.BN_MEM_DEVICE, seed,
                                   C.c_void_p(out.data_ptr()), _capi.BN_MEM_DEVICE)
    check(lib, "risk", rc)
    return out
