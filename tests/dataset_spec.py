"""Independent NumPy statement of the dataset stage's two device operations (test infrastructure; built on rng_reference).

  * The observation stream: map m (global index in the split, m < 2^32) has blocks j = 0 .. ceil(cells / 4) - 1;
    block j is Philox4x32-10 of the counter {j, m, epoch, 'OBSV' = 0x4F425356} under the key (lo(seed), hi(seed)); Box-Muller of
    the words (x, y) gives z of cells 4j and 4j + 1, of (z, w) cells 4j + 2 and 4j + 3; a ragged last block drops the rest.
    slip = f32(f32(z * std) + mean): Normal.sample()'s normal_(0, 1).mul_(std).add_(mean).
  * The gather: RegressorTrainer.load_data (reference src/trainers/regressor_trainer.py:90-126) over maps visited in `order`: class
    k's output is the concatenation over m in that order of slopes[m][classes[m] == k] and slips[m][classes[m] == k] in row-major
    cell order, cut at cap.  A class value outside [0, C) selects nothing.

Also the table of gather cases that tests/test_gpu_dataset.py runs and tests/test_dataset_host.py checks the properties of."""
from __future__ import annotations

import numpy as np

import rng_reference as R

OBSV_WORD = 0x4F425356             # 'OBSV'
f32 = np.float32


def observation_z(seed, m, epoch, cells):
    """(cells,) float64 standard normals of map m at `epoch`."""
    nblk = (cells + 3) // 4
    words = R.philox4x32(np.arange(nblk, dtype=np.uint64), R.lo32(m), R.lo32(epoch), OBSV_WORD, R.lo32(seed), R.hi32(seed), rounds=10)
    return R._block_normals(words).reshape(-1)[:cells]


def observations_z(seed, first_map, epoch, num_maps, cells):
    """(num_maps, cells) float64: row r is map first_map + r."""
    return np.stack([observation_z(seed, first_map + r, epoch, cells) for r in range(num_maps)])


def slips_from_z(z, mean, std):
    """Normal.sample() in float32 from float32 normals: a rounded product, then a rounded sum."""
    return (np.asarray(z, f32) * np.asarray(std, f32)).astype(f32) + np.asarray(mean, f32)


def visiting_order(order, M):
    return np.arange(M, dtype=np.int64) if order is None else np.asarray(order, np.int64).reshape(-1)


def class_counts(classes, C, order=None):
    """(M, C) int64: cells of class k in the map visited at position p."""
    classes = np.asarray(classes)
    M = classes.shape[0]
    flat = classes.reshape(M, -1)
    return np.stack([[int((flat[m] == k).sum()) for k in range(C)] for m in visiting_order(order, M)]).astype(np.int64).reshape(M, C)


def class_offsets(classes, C, order=None):
    """(M, C) int64: how many cells of class k the maps visited before position p hold."""
    cnt = class_counts(classes, C, order)
    return np.cumsum(cnt, axis=0) - cnt


def gather(slopes, slips, classes, C, cap, order=None):
    """(x, y, counts, totals): x[k], y[k] float32 arrays of counts[k] = min(totals[k], cap) elements."""
    slopes, slips, classes = np.asarray(slopes, f32), np.asarray(slips, f32), np.asarray(classes)
    M = slopes.shape[0]
    sl, sp, cl = slopes.reshape(M, -1), slips.reshape(M, -1), classes.reshape(M, -1)
    x, y, counts, totals = [], [], [], []
    for k in range(C):
        xs = [sl[m][cl[m] == k] for m in visiting_order(order, M)]
        ys = [sp[m][cl[m] == k] for m in visiting_order(order, M)]
        xk, yk = np.concatenate(xs), np.concatenate(ys)
        totals.append(xk.size)
        x.append(xk[:cap])
        y.append(yk[:cap])
        counts.append(x[-1].size)
    return x, y, np.array(counts, np.int64), np.array(totals, np.int64)


# ---- the gather cases -------------------------------------------------------------------------------------------------------------
WORKGROUP_THREADS = 256            # csrc/dataset_kernels.hip: the scan walks the maps in chunks of this size
ORDERS = ("null", "identity", "reversed", "random")

# name: (case number, M, cells, C, cap)
RANDOM_CASES = {
    "one_wave": (0, 1, 64, 1, 10),
    "partial_wave_cap1": (1, 1, 63, 2, 1),
    "cap_inside_a_map": (2, 5, 1021, 4, 300),
    "cap_never_reached": (3, 7, 4096, 10, 9999),
    "most_maps_skipped": (4, 300, 256, 3, 50),
    "more_maps_than_threads": (5, 1100, 64, 2, 40),
}
BUILT_CASES = {
    "class_absent": (6, 3, 100, 3, 500),
    "class_only_in_last_visited": (7, 6, 130, 3, 40),
    "cap_on_map_boundary": (8, 4, 50, 2, 40),
}
CASES = {**RANDOM_CASES, **BUILT_CASES}


def make_order(kind, M, case):
    """The visiting order `kind` of a case: None for "null"."""
    if kind == "null":
        return None
    if kind == "identity":
        return np.arange(M, dtype=np.int64)
    if kind == "reversed":
        return np.arange(M, dtype=np.int64)[::-1].copy()
    if kind == "random":
        return np.random.default_rng(1000 + case).permutation(M).astype(np.int64)
    raise ValueError(kind)


def make_case(name, kind="null"):
    """dict(M, cells, C, cap, order, classes (M, cells) int64, slopes, mean, std (M, cells) float32) of a case under the visiting
    order `kind`.  The built cases place their classes relative to that order."""
    case, M, cells, C, cap = CASES[name]
    rng = np.random.default_rng(case)
    order = make_order(kind, M, case)
    visit = visiting_order(order, M)
    if name in RANDOM_CASES:
        classes = rng.integers(-1, C + 1, (M, cells))
    elif name == "class_absent":
        classes = rng.choice(np.array([-1, 0, 2, 3]), (M, cells))                 # class 1 nowhere
    elif name == "class_only_in_last_visited":
        classes = rng.integers(-1, 2, (M, cells))                                 # -1, 0, 1 everywhere ...
        last = visit[-1]
        classes[last, rng.permutation(cells)[:17]] = 2                            # ... and 17 cells of class 2 in the map visited last
    elif name == "cap_on_map_boundary":
        classes = np.ones((M, cells), np.int64)                                   # per map: 10 cells of class 0, 40 of class 1
        for m in range(M):
            classes[m, rng.permutation(cells)[:10]] = 0
    else:
        raise ValueError(name)
    slopes = rng.uniform(0.0, 30.0, (M, cells)).astype(f32)
    mean = rng.uniform(0.0, 1.0, (M, cells)).astype(f32)
    std = rng.uniform(0.01, 0.3, (M, cells)).astype(f32)
    return dict(name=name, case=case, M=M, cells=cells, C=C, cap=cap, order=order, classes=classes.astype(np.int64), slopes=slopes, mean=mean,
                std=std)
