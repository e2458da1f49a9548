#!/usr/bin/env python3
"""What the task stage costs: label_components and sample_pairs for 64 maps of 64 x 64, 256 x 256 and 512 x 512, on an i.i.d. mask
(30 % blocked: many small components, shallow union chains) and on a serpentine one cell wide (one component that crosses every
tile border: the deepest chains), against scipy.ndimage.label on the host, one map at a time.

    python tools/task_rate.py [--out profiles/task_rates.json]

Both sides label the same masks with 4-connectivity; the device side starts from a mask that already sits on the device and ends
with the statistics read back (label_components checks the error flags), the host side starts from a NumPy mask.  sample_pairs
draws 64 pairs per map.  Host clock to a device synchronise, medians of 5, the sides alternating; measured once, not a pass
condition.  Nothing in these kernels is tuned: nobody has measured them before this."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MAPS, PAIRS, REPEATS = 64, 64, 5


def masks_of(kind: str, G: int) -> np.ndarray:
    if kind == "iid":
        return (np.random.default_rng(G).random((MAPS, G, G)) >= 0.3).astype(np.uint8)
    g = np.zeros((G, G), np.uint8)                      # the serpentine: the even rows, joined at alternating ends
    g[0::2] = 1
    g[1::4, G - 1] = 1
    g[3::4, 0] = 1
    return np.ascontiguousarray(np.broadcast_to(g, (MAPS, G, G)))


def rates(kind: str, G: int) -> dict:
    from scipy import ndimage
    from benchnav_amd.tasks import label_components, sample_pairs
    host = masks_of(kind, G)
    dev = torch.from_numpy(host).cuda()
    labels, sizes, stats = label_components(dev, 4)

    def device_label():
        label_components(dev, 4)

    def device_sample():
        sample_pairs(labels, sizes, PAIRS, seed=1, border=2, min_separation_sq=(G // 3) ** 2, min_component_cells=64, max_attempts=256)

    def scipy_label():
        return [ndimage.label(m)[1] for m in host]

    sides = {"label_components_ms": device_label, "sample_pairs_ms": device_sample, "scipy_label_ms": scipy_label}
    times = {k: [] for k in sides}
    for fn in sides.values():                           # warm-up: allocator, first launches
        fn()
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for k, fn in sides.items():                     # alternating
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    st = stats.cpu().numpy()
    found = sample_pairs(labels, sizes, PAIRS, seed=1, border=2, min_separation_sq=(G // 3) ** 2, min_component_cells=64, max_attempts=256)
    row = {"mask": kind, "maps": MAPS, "grid_size": G, "pairs_per_map": PAIRS}
    row.update({k: round(statistics.median(v), 3) for k, v in times.items()})
    row.update({"ratio_scipy_to_device": round(statistics.median(times["scipy_label_ms"]) / statistics.median(times["label_components_ms"]), 2),
                "components_equal_scipy": bool((st[:, 1] == np.array(scipy_label())).all()), "components_mean": float(st[:, 1].mean()),
                "pairs_found": float((found["attempt"] >= 0).float().mean())})
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "task_rates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/task_rate.py needs an MI355X (gfx950) device")
    doc = {"device": torch.cuda.get_device_name(0),
           "method": "host clock to a device synchronise, medians of 5, alternating; measured once, not a pass condition; nothing is tuned",
           "rows": [rates(kind, G) for kind in ("iid", "serpentine") for G in (64, 256, 512)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
