"""The seeded cases of the GP slip regressor tests (CPU: test_gp_oracle.py; GPU: test_gpu_gp.py) and their expected values.

A case is a training-set size N and a hyperparameter set (s, l, noise).  N covers: below one MFMA block (1, 5), across row-block
and k-chunk edges (67, 130), the reference's own size (1000, test/test_gpr.py) and the documented maximum (1024).  Training
slopes are uniform in [-30, 30] degrees with one DUPLICATED input (N >= 2); the targets follow a slip curve plus noise.  The
256 test slopes (a 16 x 16 map) hold training inputs exactly, negative slopes, zero, and slopes far outside the data.

`python tests/gp_cases.py` rewrites tests/golden/gp_slip.json: per case the spread between gp_spec's two formulations."""
import functools
import json
import os

import numpy as np

import gp_spec as S

SIZES = (1, 5, 67, 130, 1000, 1024)
HYPER = ((0.5, 5.0, 0.0025), (0.05, 3.0, 0.01), (1.0, 10.0, 0.04), (0.3, 1.0, 1e-4))      # (outputscale, lengthscale, noise)
CONSTANTS = (0.1, -0.05, 0.3, 0.0)
NUM_TEST = 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_slip.json")
CASES = [(n, h) for n in SIZES for h in range(len(HYPER))]


def case_id(n: int, h: int) -> str:
    return f"n{n}_h{h}"


@functools.lru_cache(maxsize=None)
def case(n: int, h: int):
    """(train_x float32, train_y float32, constant, s, l, noise, test slopes float32 (NUM_TEST,))"""
    s, l, noise = HYPER[h]
    rng = np.random.default_rng(1000 * n + h)
    x = rng.uniform(-30.0, 30.0, n).astype(np.float32)
    if n >= 2:
        x[1] = x[0]                                            # a duplicated training input
    y = (0.5 * np.tanh(x / 12.0) + CONSTANTS[h] + np.sqrt(noise) * rng.standard_normal(n)).astype(np.float32)
    phi = rng.uniform(-35.0, 35.0, NUM_TEST).astype(np.float32)
    k = min(n, 40)
    phi[:k] = x[:k]                                            # test slopes that equal training inputs
    phi[40:48] = np.float32([0.0, -0.0, -29.5, -45.0, 90.0, -200.0, 1000.0, -1e4])     # zero, negative, far outside the data
    for a in (x, y, phi):
        a.setflags(write=False)
    return x, y, CONSTANTS[h], s, l, noise, phi


@functools.lru_cache(maxsize=None)
def expected(n: int, h: int):
    """gp_spec.posterior_cholesky of the case: (mean, std) float64, computed once per process."""
    x, y, c, s, l, noise, phi = case(n, h)
    m, sd = S.posterior_cholesky(x, y, c, s, l, noise, phi)
    m.setflags(write=False)
    sd.setflags(write=False)
    return m, sd


def measured_spread(n: int, h: int):
    x, y, c, s, l, noise, phi = case(n, h)
    return S.spread(expected(n, h), S.posterior_eigen(x, y, c, s, l, noise, phi))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    out = {}
    for n, h in CASES:
        ms, ss = measured_spread(n, h)
        out[case_id(n, h)] = {"mean_spread": ms, "std_spread": ss}
        print(case_id(n, h), ms, ss)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "spread between gp_spec.posterior_cholesky and posterior_eigen per case of gp_cases.py (gp_spec.spread)",
                   "cases": out}, f, indent=1)
        f.write("\n")
