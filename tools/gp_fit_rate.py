#!/usr/bin/env python3
"""Device time of fitting a GP slip regressor (benchnav_amd/gp.py, csrc/gp_fit_kernels.hip) at
N = 256 / 1000 / 2048 / 4096 / 9999 training points, or the sizes of --sizes:

  * one fit iteration (covariance build, blocked Cholesky, triangular inverse, z and alpha, gradient, Adam step): events on the
    stream around bn_gp_fit_run_async of --iters iterations, median of --reps after a warm-up, divided by the iterations;
  * one bn_gp_fit_finish (factorisation, packing into the handle's order, the handle's allocation, one synchronise): host clock;
  * the wall time of GPSlipRegressor(..., factorization="device") against factorization="host" (gp.factorize + bn_gp_create, the
    path that existed before), alternating, on the same machine;
  * the same iteration composed from PyTorch float64 operations on the same device (torch.linalg.cholesky + autograd), for
    comparison only, and the relative distance of its loss and gradient from the kernels'.

FLOPs count N^3 / 3 for each of the three cubic stages (Cholesky, triangular inverse, K^-1 = L^-T L^-1): N^3 per iteration,
2 N^3 / 3 per finish.  The rates are whole-call rates (launch gaps included), not kernel shares of peak.

    python tools/gp_fit_rate.py [--reps 3] [--iters 2] [--sizes 256 1000 2048 4096 9999] [--out profiles/gp_fit_rates.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = (256, 1000, 2048, 4096, 9999)
HYPER = (0.3, 0.5, 5.0, 0.0025)          # constant, outputscale, lengthscale, noise of the factorisation comparison
LOG2PI = float(np.log(2.0 * np.pi))


def training_set(n):
    rng = np.random.default_rng(500 + n)
    x = rng.uniform(-30.0, 30.0, n).astype(np.float32)
    y = np.clip(0.5 * np.tanh(x / 12.0) + 0.3 + 0.05 * rng.standard_normal(n), 0.0, 1.0).astype(np.float32)
    return x, y


def torch_iteration(xt, yt, theta, lower_bound=1e-4):
    """loss and gradient at theta from float64 torch ops on the device"""
    th = theta.clone().requires_grad_(True)
    n = xt.numel()
    sp = torch.nn.functional.softplus
    c, s, l, noise = th[0], sp(th[1]), sp(th[2]), sp(th[3]) + lower_bound
    d = xt[:, None] - xt[None, :]
    K = s * torch.exp(-(d * d) / (2.0 * l * l)) + noise * torch.eye(n, dtype=torch.float64, device=xt.device)
    L = torch.linalg.cholesky(K)
    z = torch.linalg.solve_triangular(L, (yt - c)[:, None], upper=False)
    loss = ((z * z).sum() + 2.0 * torch.log(torch.diagonal(L)).sum() + n * LOG2PI) / (2.0 * n)
    loss.backward()
    return loss.detach(), th.grad


def median_ms(fn, stream, reps):
    fn()
    stream.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), [round(t, 3) for t in times]


def measure(n, reps, iters):
    from benchnav_amd import _capi, gp
    lib = _capi.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream()
    x, y = training_set(n)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    row = {"N": n, "workspace_bytes": int(lib.bn_gp_fit_workspace_bytes(n)), "iterations_per_timed_call": iters}
    with gp._Fit(lib, dev, xd, yd, 1e-4) as fit:
        fit.set_raw(np.zeros(4))
        ms, all_ms = median_ms(lambda: fit.run(iters, 0.1), stream, reps)
        raw, _, _, status, _ = fit.read()
        assert status == 0
        row.update({"iteration_ms": round(ms / iters, 3), "call_ms_all": all_ms, "iteration_f64_tflops": round(n ** 3 / (ms / iters) * 1e-9, 3)})
        fin = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = fit.finish()
            fin.append((time.perf_counter() - t0) * 1e3)
            lib.bn_gp_destroy(g)
        row.update({"finish_ms": round(float(np.median(fin[1:])), 3), "finish_ms_all": [round(t, 3) for t in fin[1:]],
                    "finish_f64_tflops": round(2 * n ** 3 / 3 / float(np.median(fin[1:])) * 1e-9, 3)})
        # the kernels' loss and gradient against the PyTorch composition at theta = 0
        fit.set_raw(np.zeros(4))
        fit.evaluate()
        _, grad, loss, status, _ = fit.read()
        assert status == 0
    xt, yt = torch.from_numpy(xd).cuda(), torch.from_numpy(yd).cuda()
    theta = torch.zeros(4, dtype=torch.float64, device="cuda")
    try:
        tms, tall = median_ms(lambda: torch_iteration(xt, yt, theta), stream, reps)
        tl, tg = torch_iteration(xt, yt, theta)
        tg = tg.cpu().numpy()
        row.update({"torch_f64_iteration_ms": round(tms, 3), "torch_f64_iteration_ms_all": tall,
                    "loss_rel_diff_vs_torch_f64": float(abs(loss - tl.item()) / abs(tl.item())),
                    "grad_rel_diff_vs_torch_f64": float(np.max(np.abs(grad - tg)) / np.max(np.abs(tg)))})
    except RuntimeError as e:                            # the comparison's own failure (an allocation inside hipBLAS at N = 9999) is recorded, not hidden
        row.update({"torch_f64_iteration_ms": None, "torch_f64_iteration_error": str(e).splitlines()[0][:200], "loss_at_theta_0": loss})
    del xt, yt
    torch.cuda.empty_cache()
    # the factorisation behind a handle: device against host, alternating
    wall = {"device": [], "host": []}
    for _ in range(reps):
        for how in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reg = gp.GPSlipRegressor(x, y, *HYPER, factorization=how)
            torch.cuda.synchronize()
            wall[how].append(time.perf_counter() - t0)
            reg.close()
    row.update({"factorization_device_s": round(float(np.median(wall["device"])), 4), "factorization_device_s_all": [round(t, 4) for t in wall["device"]],
                "factorization_host_s": round(float(np.median(wall["host"])), 4), "factorization_host_s_all": [round(t, 4) for t in wall["host"]],
                "torch_threads": torch.get_num_threads()})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2, help="fit iterations per timed call")
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES), help="training points")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_fit_rates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gp_fit_rate.py needs an MI355X (gfx950) device")
    rows = []
    for n in args.sizes:
        rows.append(measure(n, args.reps, args.iters))
        print(json.dumps(rows[-1]), flush=True)
        out = {"what": "GPSlipRegressor.fit / factorization='device': device time per fit iteration (events around "
                       f"bn_gp_fit_run_async of {args.iters} iterations, median of {args.reps} after a warm-up), host-clock time of "
                       "bn_gp_fit_finish, wall time of the device and the host factorisation behind a handle (alternating), and the same "
                       "iteration from PyTorch float64 ops on the device; FLOPs count N^3 / 3 per cubic stage",
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__, "rows": rows}
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
