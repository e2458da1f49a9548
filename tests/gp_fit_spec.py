"""The float64 specification of fitting the GP slip regressor (reference trainers/regressor_trainer.py:128-170:
Adam on -ExactMarginalLogLikelihood of ExactGP(ConstantMean, ScaleKernel(RBFKernel), GaussianLikelihood) on a 1-D input).

    theta = (constant, raw_outputscale, raw_lengthscale, raw_noise)
    c = constant, s = softplus(raw_outputscale), l = softplus(raw_lengthscale), noise = softplus(raw_noise) + lower_bound
    K = s exp(-(x - x')^2 / (2 l^2)) + noise I,  r = y - c,  alpha = K^-1 r
    loss = [ r . alpha + log det K + N log 2 pi ] / (2 N)
    dloss/dc = -sum alpha / N,  dloss/dpsi = tr((K^-1 - alpha alpha^T) dK/dpsi) / (2 N),  dpsi/draw = sigmoid(raw)

evaluated two ways that share nothing after the kernel matrix: `loss_grad_cholesky` (torch: Cholesky, triangular solves, the
gradient by autograd) and `loss_grad_eigen` (NumPy: k(x, x) = Q diag(w) Q^T and the closed-form traces).  The spread between the
two is the yardstick's own error (tests/golden/gp_fit.json records it per case of gp_fit_cases.py).  `loss_grad_cholesky_numpy`
is the Cholesky formulation once more with other code behind every step (what two implementations of one formulation differ
by: the CPU check of the emulation is held to the larger of the two distances).  `kernel_formulation` is
the device's way in NumPy: explicit L^-1, K^-1 = L^-T L^-1 tile by tile, the fixed reduction orders.  `adam` is
torch.optim.Adam's update written out; `adam_torch` is torch.optim.Adam itself.  gpytorch is not imported."""
import numpy as np
import torch

LOWER_BOUND = 1e-4
LOG2PI = float(np.log(2.0 * np.pi))
NB = 32                                                     # the device's tile order


def widen(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1)


def softplus(v):
    return np.logaddexp(0.0, v)


def inverse_softplus(v):
    return float(np.log(np.expm1(v)))


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def hyper(theta, lower_bound=LOWER_BOUND):
    """(c, s, l, noise) of the raw parameters"""
    t = np.asarray(theta, np.float64)
    return float(t[0]), float(softplus(t[1])), float(softplus(t[2])), float(softplus(t[3]) + lower_bound)


def loss_grad_cholesky(x, y, theta, lower_bound=LOWER_BOUND):
    """(loss, grad (4,)) with respect to theta: torch float64, Cholesky, autograd"""
    xt, yt = torch.from_numpy(widen(x)), torch.from_numpy(widen(y))
    th = torch.tensor(np.asarray(theta, np.float64), dtype=torch.float64, requires_grad=True)
    loss = _loss_torch(xt, yt, th, lower_bound)
    loss.backward()
    return float(loss.detach()), th.grad.numpy().copy()


def _loss_torch(xt, yt, th, lower_bound):
    n = xt.numel()
    c, s, l = th[0], torch.nn.functional.softplus(th[1], threshold=1e9), torch.nn.functional.softplus(th[2], threshold=1e9)
    noise = torch.nn.functional.softplus(th[3], threshold=1e9) + lower_bound
    d = xt[:, None] - xt[None, :]
    K = s * torch.exp(-(d * d) / (2.0 * l * l)) + noise * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    r = (yt - c)[:, None]
    z = torch.linalg.solve_triangular(L, r, upper=False)
    return ((z * z).sum() + 2.0 * torch.log(torch.diagonal(L)).sum() + n * LOG2PI) / (2.0 * n)


def loss_grad_eigen(x, y, theta, lower_bound=LOWER_BOUND):
    """The same through the eigendecomposition of k(x, x) and the closed-form derivatives"""
    x, y = widen(x), widen(y)
    n = x.size
    c, s, l, noise = hyper(theta, lower_bound)
    d2 = (x[:, None] - x[None, :]) ** 2
    Kr = s * np.exp(-d2 / (2.0 * l * l))
    w, Q = np.linalg.eigh(Kr)
    dd = w + noise
    p = Q.T @ (y - c)
    loss = (np.sum(p * p / dd) + np.sum(np.log(dd)) + n * LOG2PI) / (2.0 * n)
    a = p / dd                                              # Q^T alpha
    alpha = Q @ a
    g_noise = np.sum(1.0 / dd) - np.sum(a * a)
    g_s = (np.sum(w / dd) - np.sum(a * a * w)) / s
    M = Kr * d2 / l ** 3
    Kinv = (Q / dd[None, :]) @ Q.T
    g_l = np.sum(Kinv * M) - alpha @ M @ alpha
    t = np.asarray(theta, np.float64)
    grad = np.array([-np.sum(alpha) / n, g_s / (2 * n) * sigmoid(t[1]), g_l / (2 * n) * sigmoid(t[2]), g_noise / (2 * n) * sigmoid(t[3])])
    return float(loss), grad


def loss_grad_cholesky_numpy(x, y, theta, lower_bound=LOWER_BOUND):
    """The Cholesky formulation a second time with other code behind every step: NumPy's kernel matrix and Cholesky factor,
    triangular solves, and the closed-form traces instead of autograd.  Its distance from loss_grad_cholesky is what two
    correct implementations of ONE formulation differ by (the factorisation's backward error seen through the loss)."""
    x, y = widen(x), widen(y)
    n = x.size
    c, s, l, noise = hyper(theta, lower_bound)
    d2 = (x[:, None] - x[None, :]) ** 2
    Kr = s * np.exp(-d2 / (2.0 * l * l))
    Lt = torch.from_numpy(np.linalg.cholesky(Kr + noise * np.eye(n)))
    z = torch.linalg.solve_triangular(Lt, torch.from_numpy(y - c)[:, None], upper=False)
    alpha = torch.linalg.solve_triangular(Lt.T, z, upper=True).numpy()[:, 0]
    Kinv = torch.cholesky_inverse(Lt).numpy()
    loss = (float((z * z).sum()) + 2.0 * np.sum(np.log(np.diagonal(Lt.numpy()))) + n * LOG2PI) / (2.0 * n)
    M = Kr * d2 / l ** 3
    g_noise = np.trace(Kinv) - alpha @ alpha
    g_s = (np.sum(Kinv * Kr) - alpha @ Kr @ alpha) / s
    g_l = np.sum(Kinv * M) - alpha @ M @ alpha
    t = np.asarray(theta, np.float64)
    grad = np.array([-np.sum(alpha) / n, g_s / (2 * n) * sigmoid(t[1]), g_l / (2 * n) * sigmoid(t[2]), g_noise / (2 * n) * sigmoid(t[3])])
    return float(loss), grad


def _wave_sum(v):
    """the device's butterfly over 64 lanes: v (64, ...) -> (...)"""
    v = np.array(v, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ o]
    return v[0]


def _block_sum(values):
    """256 threads: thread t sums the entries t, t + 256, ... in ascending order, then a binary tree"""
    values = np.asarray(values, np.float64)
    part = np.zeros(256)
    for k in range(0, values.size, 256):
        chunk = values[k:k + 256]
        part[:chunk.size] += chunk
    s = 128
    while s:
        part[:s] += part[s:2 * s]
        s //= 2
    return part[0]


def kernel_formulation(x, y, theta, lower_bound=LOWER_BOUND):
    """(loss, grad) the way csrc/gp_fit_kernels.hip computes them, in NumPy: explicit X = L^-1 (padded to the tile order with
    an identity), z = X r per row by 64 strided partial sums and a butterfly, alpha = X^T z by eight row groups, K^-1 = X^T X
    tile by tile with the row steps of 4 in ascending order, the weighted elements folded per lane and reduced by the butterfly,
    the tiles' partials and the remaining sums by _block_sum."""
    x, y = widen(x), widen(y)
    n = x.size
    c, s, l, noise = hyper(theta, lower_bound)
    npad = (n + NB - 1) // NB * NB
    T = npad // NB
    d = x[:, None] - x[None, :]
    K = np.eye(npad)
    K[:n, :n] = s * np.exp(-(d * d) / (2.0 * l * l)) + noise * np.eye(n)
    L = np.linalg.cholesky(K)
    X = np.tril(np.linalg.solve(L, np.eye(npad)))
    r = np.zeros(npad)
    r[:n] = y - c
    z = np.zeros(npad)
    for i in range(n):
        lanes = np.zeros(64)
        for j0 in range(0, i + 1, 64):
            seg = X[i, j0:min(j0 + 64, i + 1)] * r[j0:min(j0 + 64, i + 1)]
            lanes[:seg.size] += seg
        z[i] = _wave_sum(lanes)
    alpha = np.zeros(npad)
    for J in range(T):
        part = np.zeros((8, NB))
        for i in range(NB * J, npad):
            part[(i - NB * J) % 8] += X[i, NB * J:NB * J + NB] * z[i]
        tot = np.zeros(NB)
        for g in range(8):
            tot += part[g]
        alpha[NB * J:NB * J + NB] = tot
    xp = np.zeros(npad)
    xp[:n] = x
    lane = np.arange(64)
    parts = []
    for Ta in range(T):
        for Tb in range(Ta + 1):
            acc = np.zeros((NB, NB))
            for k in range(NB * Ta, npad, 4):
                acc += X[k:k + 4, NB * Ta:NB * Ta + NB].T @ X[k:k + 4, NB * Tb:NB * Tb + NB]
            gs, gl, gn = np.zeros(64), np.zeros(64), np.zeros(64)
            for u in range(2):
                for v in range(2):
                    for rr in range(4):
                        ia, ib = NB * Ta + 16 * u + (lane >> 4) + 4 * rr, NB * Tb + 16 * v + (lane & 15)
                        ok = (ia < n) & (ib < n)
                        wgt = acc[ia - NB * Ta, ib - NB * Tb] - alpha[ia] * alpha[ib]
                        dd = xp[ia] - xp[ib]
                        d2 = dd * dd
                        e = np.exp(-d2 / (2.0 * l * l))
                        gs += np.where(ok, wgt * e, 0.0)
                        gl += np.where(ok, wgt * (e * d2), 0.0)
                        gn += np.where(ok & (ia == ib), wgt, 0.0)
            two = 1.0 if Ta == Tb else 2.0
            parts.append([two * _wave_sum(gs), two * _wave_sum(gl), two * _wave_sum(gn)])
    parts = np.array(parts)
    logdet = _block_sum(np.log(np.diagonal(L)[:n]))
    zz = _block_sum(z[:n] * z[:n])
    sa = _block_sum(alpha[:n])
    g = [_block_sum(parts[:, k]) for k in range(3)]
    t = np.asarray(theta, np.float64)
    loss = (zz + 2.0 * logdet + n * LOG2PI) / (2.0 * n)
    grad = np.array([-sa / n, g[0] / (2.0 * n) * sigmoid(t[1]), g[1] * s / (l * l * l) / (2.0 * n) * sigmoid(t[2]),
                     g[2] / (2.0 * n) * sigmoid(t[3])])
    return float(loss), grad


def adam(x, y, loss_grad, iterations, lr=0.1, theta0=None, beta1=0.9, beta2=0.999, eps=1e-8, lower_bound=LOWER_BOUND):
    """torch.optim.Adam's update (defaults: bias-corrected, no weight decay) written out, on loss_grad.  Returns (theta after the
    last step, losses (iterations,) each BEFORE its step)."""
    th = np.zeros(4) if theta0 is None else np.array(theta0, np.float64)
    m, v = np.zeros(4), np.zeros(4)
    losses = np.zeros(iterations)
    for it in range(iterations):
        losses[it], g = loss_grad(x, y, th, lower_bound)
        step = it + 1
        m = m + (1.0 - beta1) * (g - m)
        v = v * beta2 + (1.0 - beta2) * (g * g)
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        denom = np.sqrt(v) / np.sqrt(bc2) + eps
        th = th + (-(lr / bc1)) * (m / denom)
    return th, losses


def adam_torch(x, y, iterations, lr=0.1, theta0=None, lower_bound=LOWER_BOUND):
    """The same trajectory with torch.optim.Adam and autograd on the Cholesky formulation"""
    xt, yt = torch.from_numpy(widen(x)), torch.from_numpy(widen(y))
    th = torch.tensor(np.zeros(4) if theta0 is None else np.asarray(theta0, np.float64), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([th], lr=lr)
    losses = np.zeros(iterations)
    for it in range(iterations):
        opt.zero_grad()
        loss = _loss_torch(xt, yt, th, lower_bound)
        loss.backward()
        opt.step()
        losses[it] = float(loss.detach())
    return th.detach().numpy().copy(), losses


def eval_spread(a, b):
    """(loss spread, gradient spread) of two evaluations (loss, grad): the loss relative to the larger |loss|, the gradient
    relative to its largest component."""
    (la, ga), (lb, gb) = a, b
    tiny = np.finfo(np.float64).tiny
    return (abs(la - lb) / max(abs(la), abs(lb), tiny),
            float(np.max(np.abs(np.asarray(ga) - np.asarray(gb))) / max(np.max(np.abs(ga)), np.max(np.abs(gb)), tiny)))


def trajectory_spread(a, b):
    """(theta spread, loss spread) of two trajectories (theta, losses): the largest difference in theta relative to
    max(1, largest |theta|), and in the loss history relative to max(1, largest |loss|) -- the loss crosses zero on the way."""
    (ta, la), (tb, lb) = a, b
    ts = float(np.max(np.abs(ta - tb)) / max(1.0, np.max(np.abs(ta)), np.max(np.abs(tb))))
    ls = float(np.max(np.abs(la - lb)) / max(1.0, np.max(np.abs(la)), np.max(np.abs(lb)))) if len(la) else 0.0
    return ts, ls
