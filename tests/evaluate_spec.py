"""The specification of the model-evaluation stage (csrc/eval_kernels.hip), in NumPy float64.

The three kernels are held to this on the GPU (test_gpu_evaluate.py, test_gpu_evaluator.py); test_evaluate_spec.py holds IT to
independent formulas.  It shares no code with the package.

THE SUM ORDER of the slip stage's float64 sums, operation for operation (integer counts are exact in any order):

  1. A map's cells, in index order, are cut into slabs of SLAB = 4096 cells; a slab is walked in steps of WAVE = 64 consecutive
     cells (the last step of a map may be partial).
  2. Per step and per group (true class, slope bin) present in it: a vector x of 64 float64 -- the cell's value where the cell is
     a valid member of the group, +0.0 elsewhere (other groups, invalid cells, the lanes past the map's end) -- is reduced by
         for off in (32, 16, 8, 4, 2, 1):  x[:off] = x[:off] + x[off:2 * off]
     and x[0] is added to the slab's entry:  T = T + x[0], steps in index order, T starting at +0.0.
     (A group absent from a step adds nothing; adding the +0.0 its tree would give leaves T's bits as they are, because T, which
     starts at +0.0, is never -0.0.  `slip` uses that to run every group over every step.)
  3. A map's entry is  P = 0.0; for slab in index order: P = P + T[slab].
  4. A running total over maps is  R = R + P[map], maps in index order (`slip_total`).

The per-cell values, float64 on the float32 inputs, in this order of operations:
    d = mu - m;  |d|;  d * d;  sigma;  s;
    KL  = (log(sigma / s) + (s * s + d * d) / ((2 * sigma) * sigma)) - 0.5
    e = y - mu;  NLL = 0.5 * log(TWO_PI * (sigma * sigma)) + (e * e) / ((2 * sigma) * sigma);  z = e / sigma;  z * z
    covered: |e| <= 2 * sigma"""
import numpy as np

WAVE, SLAB, SUMS, RISK_COUNTS = 64, 4096, 8, 5
TWO_PI = 6.283185307179586
SUM_NAMES = ("d", "abs_d", "d2", "sigma", "s", "kl", "nll", "z2")
LOG_SUMS = (5, 6)                          # the two sums with a logarithm: held to metric_bound, every other one bit for bit
U_LOG_DEVICE = 1                           # HIP math API reference, double precision table: log, maximum ULP error 1
U_LOG_HOST = 1                             # the spec's own np.log (the C library's log: documented within 1 ulp)


def confusion(true_classes, pred_classes, num_classes):
    """(M, cells) int32 each -> table (M, C, C) int64 indexed [true][predicted], ignored (M) int64."""
    t, p, C = np.asarray(true_classes, np.int64), np.asarray(pred_classes, np.int64), int(num_classes)
    M = t.shape[0]
    table, ignored = np.zeros((M, C, C), np.int64), np.zeros(M, np.int64)
    for m in range(M):
        for a, b in zip(t[m].ravel(), p[m].ravel()):
            if 0 <= a < C and 0 <= b < C:
                table[m, a, b] += 1
            else:
                ignored[m] += 1
    return table, ignored


def slope_bin(phi, bins, max_slope):
    """float64: trunc(phi * bins / max_slope) clamped to [0, bins - 1]; closed on the left."""
    t = (np.asarray(phi, np.float32).astype(np.float64) * np.float64(bins)) / np.float64(max_slope)
    return np.where(t < 0.0, 0, np.where(t >= bins, bins - 1, np.trunc(np.clip(t, 0.0, float(bins))))).astype(np.int64)


def _tree(x):
    """x (..., 64, K): the fixed reduction over the 64 lanes."""
    x = x.copy()
    for off in (32, 16, 8, 4, 2, 1):
        x[..., :off, :] = x[..., :off, :] + x[..., off:2 * off, :]
    return x[..., 0, :]


def slip(mu, sigma, m, s, phi, classes, num_classes, y=None, bins=6, max_slope=30.0):
    """All (M, cells); float32 but classes (int32).  -> dict: sums (M, C, NB, 8) float64 in SUM_NAMES' order, counts (M, C, NB, 2)
    int64 (cells, covered), invalid (M) int64, and magnitude (M, C, NB, 2) float64: per group the sum over its cells of
    |log| + quotient + 0.5 (KL) and of |0.5 log| + quotient (NLL), which metric_bound takes."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    mu, sigma, m, s, phi = (f(a) for a in (mu, sigma, m, s, phi))
    cls, C, NB = np.asarray(classes, np.int64), int(num_classes), int(bins)
    M, cells = mu.shape
    has_y = y is not None
    yy = f(y) if has_y else np.zeros_like(mu)
    ok = (cls >= 0) & (cls < C) & np.isfinite(phi) & np.isfinite(mu) & np.isfinite(sigma) & np.isfinite(m) & np.isfinite(s) & np.isfinite(yy)
    ok &= (sigma > 0.0) & (s > 0.0)
    group = np.where(ok, cls * NB + slope_bin(np.where(np.isfinite(phi), phi, 0.0), NB, max_slope), -1)
    one = np.ones_like(mu)
    sg, ss = np.where(ok, sigma, one), np.where(ok, s, one)          # stand-ins where the cell is in no sum
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(ok, mu - m, 0.0)
        two_var = (2.0 * sg) * sg
        log_kl, q_kl = np.log(sg / ss), (ss * ss + d * d) / two_var
        e = np.where(ok, yy - mu, 0.0)
        log_nll, q_nll = 0.5 * np.log(TWO_PI * (sg * sg)), (e * e) / two_var
        z = e / sg
        vals = np.stack([d, np.abs(d), d * d, sg, ss, (log_kl + q_kl) - 0.5, log_nll + q_nll, z * z], axis=-1)      # (M, cells, 8)
        covered = np.abs(e) <= 2.0 * sg
    if not has_y:
        vals[..., 6:] = 0.0
        covered[:] = False
    G = C * NB
    steps = (cells + WAVE - 1) // WAVE
    pad = steps * WAVE - cells
    sums, counts = np.zeros((M, G, SUMS)), np.zeros((M, G, 2), np.int64)
    magnitude = np.zeros((M, G, 2))
    for mm in range(M):
        g = np.concatenate([group[mm], np.full(pad, -1)]).reshape(steps, WAVE)
        v = np.concatenate([vals[mm], np.zeros((pad, SUMS))]).reshape(steps, WAVE, SUMS)
        for gi in np.unique(g[g >= 0]):
            member = g == gi
            per_step = _tree(np.where(member[..., None], v, 0.0))                        # (steps, 8)
            P = np.zeros(SUMS)
            for s0 in range(0, steps, SLAB // WAVE):                                     # slabs in index order
                T = np.zeros(SUMS)
                for st in range(s0, min(s0 + SLAB // WAVE, steps)):                      # steps in index order
                    T = T + per_step[st]
                P = P + T
            sums[mm, gi] = P
            flat = (group[mm] == gi)
            counts[mm, gi] = (flat.sum(), (flat & covered[mm]).sum())
            magnitude[mm, gi] = ((np.abs(log_kl[mm]) + q_kl[mm] + 0.5)[flat].sum(),
                                 (np.abs(log_nll[mm]) + q_nll[mm])[flat].sum() if has_y else 0.0)
    shape = lambda a, k: a.reshape(M, C, NB, k)
    return {"sums": shape(sums, SUMS), "counts": shape(counts, 2), "invalid": (~ok).sum(axis=1).astype(np.int64),
            "magnitude": shape(magnitude, 2)}


def slip_total(sums, start=None):
    """The running total over maps: start (or zeros) + sums[0] + sums[1] + ..., one float64 addition per map, in map order."""
    total = np.zeros(sums.shape[1:]) if start is None else np.array(start, np.float64)
    for mm in range(sums.shape[0]):
        total = total + sums[mm]
    return total


def metric_bound(magnitude, n, u=U_LOG_DEVICE + U_LOG_HOST):
    """|device - spec| for a KL or NLL sum of n terms whose magnitudes (above) add to `magnitude`.  Both sides run the same float64
    operations in the same order on the same inputs; only log may round differently: the device's by at most U_LOG_DEVICE ulps,
    the spec's own by U_LOG_HOST, so by u = 2 ulps of |log| between them.  The term goes through at most two more roundings
    (KL: + quotient, - 0.5; NLL: + quotient), each of which can move by one ulp of a value no larger than the term's magnitude:
    a term differs by at most (u + 2) 2^-52 of its magnitude.  Of the additions a sum goes through, those with a +0.0 operand
    are exact, which leaves at most n that round, each within 2^-53 of a partial sum no larger than `magnitude`, on either side:
    n 2^-52 magnitude.  Together (u + 2 + n) 2^-52 magnitude."""
    return (u + 2 + np.asarray(n, np.float64)) * 2.0 ** -52 * np.asarray(magnitude, np.float64)


def stuck(v, threshold):
    """The environment step's rule in float32: 1 - clamp(v, 0, 1) <= threshold."""
    v = np.asarray(v, np.float32)
    return (np.float32(1.0) - np.clip(v, np.float32(0.0), np.float32(1.0))) <= np.float32(threshold)


def risk(risk_maps, y, classes, num_classes, stuck_threshold=0.1):
    """risk_maps (S, M, cells), y (M, cells) float32, classes (M, cells) -> counts (M, S, C, 5) int64: [0] y > r, [1 + 2 * believed
    stuck + actually stuck]; invalid (M, S) int64: a class out of range, a non-finite y or a non-finite r."""
    r, y, cls, C = np.asarray(risk_maps, np.float32), np.asarray(y, np.float32), np.asarray(classes, np.int64), int(num_classes)
    S, M, _ = r.shape
    counts, invalid = np.zeros((M, S, C, RISK_COUNTS), np.int64), np.zeros((M, S), np.int64)
    cell_ok = (cls >= 0) & (cls < C) & np.isfinite(y)
    with np.errstate(invalid="ignore"):
        actual = stuck(y, stuck_threshold)
        for k in range(S):
            ok = cell_ok & np.isfinite(r[k])
            invalid[:, k] = (~ok).sum(axis=1)
            slot = 1 + 2 * stuck(r[k], stuck_threshold).astype(np.int64) + actual.astype(np.int64)
            exceed = y > r[k]
            for mm in range(M):
                c = cls[mm][ok[mm]]
                np.add.at(counts[mm, k, :, 0], c[exceed[mm][ok[mm]]], 1)
                np.add.at(counts[mm, k], (c, slot[mm][ok[mm]]), 1)
    return counts, invalid
