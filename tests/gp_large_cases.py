"""The seeded cases of the GP slip regressor above 1024 training points (CPU: test_gp_large_oracle.py; GPU:
test_gpu_gp_large.py): the recipe of gp_cases.case at the sizes where gp_slab_kernel (csrc/gp_kernels.hip) changes its path.

N covers: one point past the switch of kernels (1025, padded to 1040), an odd row-block count with one row in the last block
(1041), one below and one above a k-chunk edge that is no slab edge (1151, 1153: 9 chunks of 128 points, the third slab holds
8 and 9 row blocks), one below and one above a slab edge (1535, 1537: 3 slabs of 512 rows, and a fourth of one row block), two
k-chunks of 1024 plus one point, which is a slab edge too (2049), and 194 row blocks (3100).  Hyperparameter sets 0 and 3 of
gp_cases.HYPER; set 3 (noise 1e-4, lengthscale 1) is the ill-conditioned one.

`python tests/gp_large_cases.py` rewrites tests/golden/gp_slip_large.json: per case the spread between gp_spec's two
formulations, and the multiple of that spread at which the NumPy emulation of the slab kernel's formulation lands."""
import json
import os
import sys

import numpy as np

import gp_cases as GC
import gp_spec as S

SIZES = (1025, 1041, 1151, 1153, 1535, 1537, 2049, 3100)
HYPER_SETS = (0, 3)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_slip_large.json")
CASES = [(n, h) for n in SIZES for h in HYPER_SETS]
EPS = np.finfo(np.float64).eps

case, case_id, expected, measured_spread = GC.case, GC.case_id, GC.expected, GC.measured_spread

# the slab kernel's shape (csrc/gp_kernels.hip)
WAVES, RB, SLAB_BLOCKS = 8, 4, 32


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def slab_formulation(n: int, h: int):
    """gp_slab_kernel's formulation in NumPy, with gp.factorize's explicit L^-1:

    v: every row block's accumulator sums over k in ascending order, four k at a time (one MFMA step);
    |v|^2: lane (wave w, lane group g, column) folds v[16 i + g + 4 e]^2 over the slabs s, its row blocks i = 32 s + w + 8 r,
           r = 0 ... 3, and the registers e = 0 ... 3 in that order; one thread per cell then sums over the waves and lane groups;
    k . alpha: thread (w, cell) sums the points w, w + 8, ... in ascending order, one thread per cell sums the eight.
    (mean, std) float64 at the case's test slopes."""
    from benchnav_amd import gp
    x, y, c, s, l, noise, phi = case(n, h)
    xs, alpha, linv = gp.factorize(x, y, c, s, l, noise)
    M = phi.shape[0]
    d = phi.astype(np.float64)[None, :] - xs[:, None]
    ks = s * np.exp((d * d) * (-1.0 / (2.0 * l * l)))
    nb = (n + 15) // 16
    nslabs = (nb + SLAB_BLOCKS - 1) // SLAB_BLOCKS
    rows = nslabs * SLAB_BLOCKS * 16
    Lp = np.zeros((rows, nb * 16))
    Lp[:n, :n] = linv
    kp = np.zeros((nb * 16, M))
    kp[:n] = ks
    v = np.zeros((rows, M))
    for j in range(4 * nb):                                    # step j reaches the row blocks i >= j // 4
        r0 = 16 * (j // 4)
        v[r0:] += Lp[r0:, 4 * j:4 * j + 4] @ kp[4 * j:4 * j + 4]
    v = v.reshape(nslabs, RB, WAVES, 4, 4, M)                  # row = 16 (32 s + 8 r + w) + 4 e + g
    sq = np.zeros((WAVES, 4, M))
    for si in range(nslabs):
        for r in range(RB):
            for e in range(4):
                sq += v[si, r, :, e] ** 2
    tot = np.zeros(M)
    for w in range(WAVES):
        for g in range(4):
            tot += sq[w, g]
    ka = np.zeros((nb * 16 + 7) // 8 * 8 * M).reshape(-1, WAVES, M)
    ka.reshape(-1, M)[:n] = ks * alpha[:, None]
    part = np.zeros((WAVES, M))
    for m in range(ka.shape[0]):
        part += ka[m]
    mean = np.zeros(M)
    for w in range(WAVES):
        mean += part[w]
    return c + mean, np.sqrt(np.maximum(s - tot, 0.0) + noise)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for n, h in CASES:
        ms, ss = measured_spread(n, h)
        em, es = S.spread(expected(n, h), slab_formulation(n, h))
        out[case_id(n, h)] = {"mean_spread": ms, "std_spread": ss, "emulation_mean_multiple": em / max(ms, 4 * EPS),
                              "emulation_std_multiple": es / max(ss, 4 * EPS)}
        print(case_id(n, h), out[case_id(n, h)], flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "per case of gp_large_cases.py: the spread between gp_spec.posterior_cholesky and posterior_eigen "
                           "(gp_spec.spread), and the NumPy emulation of gp_slab_kernel's formulation against posterior_cholesky as a "
                           "multiple of that spread (floor 4 eps)", "cases": out}, f, indent=1)
        f.write("\n")
