"""The end of an MPPI solve restated in float64, with a derived bound per element (no GPU, NumPy only).

What is restated: csrc/mppi_tail.h (tail_weights, finish_body) and csrc/mppi_merge.h (column_sums, merge_one, merge_group,
merge_partials, ticket_merge) turn the K float32 costs and the K control rows of a solve into the weights and U*:

    z_k = fl32(-cost_k / lambda)                    one IEEE division, as tail_weights and oracle_solve write it
    m   = max_k z_k          d_k = fl32(z_k - m)    e_k = exp(d_k)  in float64
    w_k = e_k / sum_k e_k                           Ustar[j] = sum_k w_k U[k, j]

`tail(cost, U, lam)` returns these in float64 together with `w_bound (K,)`, `U_bound (T, 2)` and `sum_bound`: how far a float32
implementation of ANY of the kernels' forms may lie from them.  With u = 2^-24 (half an ulp, relative):

  ingredients
    a      = EXP_ULP * 2u     expf: "maximum ULP error 1" in the "Single precision mathematical functions" table of the HIP math API
                              reference (ROCm documentation, HIP "Math API" page -- the page tests/test_gpu_scores.py cites for sqrt)
    u                         one float32 division: correctly rounded (IEEE 754; hipcc's default
                              -fhip-fp32-correctly-rounded-divide-sqrt, which benchnav_amd/build.py keeps), 0.5 ulp
    TINY   = 2^-125           absolute: a term or a result below the smallest normal number may be flushed or lose bits
  the row-wise form
    A kernel does not compute exp(fl(z_k - m)): a workgroup scales its 64 rollouts against ITS maximum m_r, the merge rescales the row
    by exp(fl(m_r - m)) (and, with more than 64 rows, a group of 16 rows against the group's maximum first):
        e_k(device) = expf(fl(z_k - m_r)) * expf(fl(m_r - m_g)) * expf(fl(m_g - m))
    Each subtraction rounds once, by at most u |argument|; m_r and m_g lie between z_k and m, so the arguments add up to |z_k - m| and
    the device's exponent is within u |z_k - m| of the exact difference -- and the spec's own fl(z_k - m) is within u |z_k - m| of it too:
        |exponent(device) - d_k| <= 2u |d_k| (1 + u)          a factor exp(2u |d_k|) on the term
    with up to EXP_FACTORS = 3 expf results multiplied: (1 + a)^3.  Terms whose e_k is zero in float32 contribute TINY at most.
  the sums
    S and every column of U* are sums of the K terms taken in some fixed tree: 64 rollouts of a row (column_sums' quarters), the
    product with the row's scale, nblk = ceil(K/64) rows (or 16 rows and ceil(nblk/16) groups).  In any order a term of a sum of n
    passes through fewer than n roundings; every fma of a chain rounds once.  n_sum = 64 + nblk + ceil(nblk/16) + 2 covers every form:
        rho_k = exp(2u |d_k| (1 + u)) (1 + a)^3 (1 + u)^n_sum - 1          relative error of term k of S or of a column
        rho_S = sum_k w_k rho_k + K TINY                                   relative error of S (all terms positive, S >= 1)
  the results
        w_bound[k] = w_k ((1 + a)(1 + u) / (1 - rho_S) - 1) + TINY         expf(d_k) / S, one division
        U_bound[j] = sum_k w_k |U[k, j]| ((1 + rho_k)(1 + u) / (1 - rho_S) - 1) + (K max|U| + 1) TINY     a column over S, one division
        sum_bound  = sum_k w_bound[k]                                      |sum of the float32 weights, added in float64, - 1|

The bound depends on the case: on the spread of z through rho_k (weighted by w_k: a far term is changed much and counts little),
on K through n_sum, on T not at all but through which columns exist.  Nothing in it was measured on a kernel.  The float32 CPU oracle
(oracle/mppi_oracle.c: glibc expf, float64 accumulation) lies inside it by construction -- tests/test_mppi_tail_spec.py asserts that on
every case, and tests/golden/mppi_tail.json records per case how much of the bound the oracle uses (the yardstick a reader can hold
the device's measured/bound against)."""
import numpy as np

U24 = 2.0 ** -24
EXP_ULP = 1.0
EXP_FACTORS = 3
TINY = 2.0 ** -125


def n_sum(K):
    nblk = -(-int(K) // 64)
    return 64 + nblk + -(-nblk // 16) + 2


def tail(cost, U, lam):
    cost = np.asarray(cost)
    U = np.asarray(U)
    assert cost.dtype == np.float32 and U.dtype == np.float32 and U.ndim == 3 and U.shape[0] == cost.shape[0] and U.shape[2] == 2
    K, T = U.shape[0], U.shape[1]
    z = (-cost) / np.float32(lam)                      # float32 / float32: one correctly rounded division
    assert z.dtype == np.float32 and np.isfinite(z).all()
    m = z.max()
    d32 = z - m
    assert d32.dtype == np.float32
    d = d32.astype(np.float64)
    e = np.exp(d)
    S = e.sum()
    w = e / S
    U64 = U.reshape(K, 2 * T).astype(np.float64)
    Ustar = (w[:, None] * U64).sum(0)

    a, u = EXP_ULP * 2 * U24, U24
    rho = np.exp(2 * u * np.abs(d) * (1 + u)) * (1 + a) ** EXP_FACTORS * (1 + u) ** n_sum(K) - 1
    rho_S = float((w * rho).sum()) + K * TINY
    w_bound = w * ((1 + a) * (1 + u) / (1 - rho_S) - 1) + TINY
    tau = (1 + rho) * (1 + u) / (1 - rho_S) - 1
    U_bound = (w[:, None] * np.abs(U64) * tau[:, None]).sum(0) + (K * float(np.abs(U64).max()) + 1) * TINY
    return dict(z=z, m=m, d=d, w=w, Ustar=Ustar.reshape(T, 2), w_bound=w_bound, U_bound=U_bound.reshape(T, 2), sum_bound=float(w_bound.sum()),
                rho_S=rho_S, spread=float(np.abs(d).max()))


def ratios(w, Ustar, spec):
    """measured / bound: the largest over the weights, over U*, and for the sum of the weights."""
    w = np.asarray(w, np.float64)
    Ustar = np.asarray(Ustar, np.float64)
    return dict(w=float((np.abs(w - spec["w"]) / spec["w_bound"]).max()), U=float((np.abs(Ustar - spec["Ustar"]) / spec["U_bound"]).max()),
                sum=abs(float(w.sum()) - 1.0) / spec["sum_bound"])
