"""The float64 specification of the exact-GP slip regressor (reference slip_regressors/gpr.py: ExactGP,
ConstantMean, ScaleKernel(RBFKernel) with one lengthscale, GaussianLikelihood, 1-D input), in NumPy:

    k(a, b) = s exp(-(a - b)^2 / (2 l^2)),   K = k(x, x) + noise I,   alpha = K^-1 (y - c)
    mean(phi) = c + k(phi, x) . alpha,       var(phi) = max(s - k(phi, x) K^-1 k(x, phi), 0) + noise,   std = sqrt(var)

evaluated two ways that share nothing after the kernel matrix: `posterior_cholesky` (K = L L^T and triangular solves) and
`posterior_eigen` (k(x, x) = Q diag(w) Q^T, so K^-1 = Q diag(1 / (w + noise)) Q^T).  The spread between the two is the yardstick's
own error (tests/golden/gp_slip.json records it per case of gp_cases.py); the product is held to `posterior_cholesky`.
Training inputs and targets are float32 values widened exactly, as the reference trains on float32."""
import numpy as np


def widen(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1)


def kernel(a: np.ndarray, b: np.ndarray, s: float, l: float) -> np.ndarray:
    d = np.asarray(a, np.float64)[:, None] - np.asarray(b, np.float64)[None, :]
    return s * np.exp(-(d * d) / (2.0 * l * l))


def posterior_cholesky(x, y, c, s, l, noise, phi):
    """(mean, std) in float64 at the test inputs phi, by Cholesky solves."""
    x, y, phi = widen(x), widen(y), np.asarray(phi, np.float64).reshape(-1)
    K = kernel(x, x, s, l) + noise * np.eye(x.size)
    L = np.linalg.cholesky(K)
    ks = kernel(x, phi, s, l)                                  # (N, M)
    z = np.linalg.solve(L, y - c)
    alpha = np.linalg.solve(L.T, z)
    v = np.linalg.solve(L, ks)
    mean = c + ks.T @ alpha
    var = np.maximum(s - np.sum(v * v, axis=0), 0.0) + noise
    return mean, np.sqrt(var)


def posterior_eigen(x, y, c, s, l, noise, phi):
    """The same posterior through the eigendecomposition of k(x, x)."""
    x, y, phi = widen(x), widen(y), np.asarray(phi, np.float64).reshape(-1)
    w, Q = np.linalg.eigh(kernel(x, x, s, l))
    d = w + noise
    ks = kernel(x, phi, s, l)
    p = Q.T @ ks                                               # (N, M)
    r = Q.T @ (y - c)
    mean = c + p.T @ (r / d)
    var = np.maximum(s - np.sum(p * p / d[:, None], axis=0), 0.0) + noise
    return mean, np.sqrt(var)


def spread(a, b):
    """How far two evaluations (mean, std) are apart: the mean relative to the largest |mean| of the case (a mean may cross
    zero), the std cell by cell (std >= sqrt(noise) > 0).  Returns (mean spread, std spread)."""
    (ma, sa), (mb, sb) = a, b
    scale = max(float(np.max(np.abs(ma))), float(np.max(np.abs(mb))), np.finfo(np.float64).tiny)
    return float(np.max(np.abs(ma - mb)) / scale), float(np.max(np.abs(sa - sb) / np.maximum(sa, sb)))
