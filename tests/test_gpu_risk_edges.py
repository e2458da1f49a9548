"""GPU: csrc/risk_kernels.hip at its edges, against oracle/risk_oracle.py (which test_risk_oracle_torch.py ties to torch.quantile).

  a. injected draws, every case of tests/risk_cases.py: VaR by value, CVaR by NaN pattern and a derived summation bound;
  b. non-finite cells: NaN / +-inf in, NaN out, the neighbours of the same workgroup untouched;
  c. in-kernel Philox draws at interior ranks against a float64 reference on rng_reference.risk;
  d. the BN_MEM_HOST branches of bn_risk_map_infer, bit for bit against the all-device call;
  e. refusals at the C ABI;
  f. determinism, a side stream, the high half of the seed.

Bounds.  CVaR on injected draws: risk_cases.cvar_bound (R + 8 roundings of a sum that never exceeds sum|x|).  Philox draws (c): the
kernel's sample i of a cell is f32(f32(z' std) + mean) with |z' - z| <= TOL_Z (test_gpu_noise_streams.py: device Box-Muller against
float64), so it lies within std TOL_Z + 1/2 ulp32(6.77 std) + 1/2 ulp32(M), M = |mean| + 6.77 std, of the float64 sample; delta =
std TOL_Z + 2 ulp32(M) leaves one ulp32(M) to spare.  Order statistics, their convex combinations and top-k means are 1-Lipschitz in
the sup norm of the samples, so the kernel's exact lerp is within the sample error of the reference's.  Its float32 lerp then rounds
b - a (1/2 ulp32(2 M) = ulp32(M), times |w| < 1) and the fma (1/2 ulp32(M)): 1.5 ulp32(M) more.  Spare plus "one float32 ulp" =
ulp32(M) cover it: |VaR - ref| <= delta + ulp32(M).  CVaR: delta plus the summation bound on the reference's tail."""
import ctypes as C

import numpy as np
import pytest

import risk_cases as RC
import rng_reference as R
from oracle import risk_oracle as RO

f32 = np.float32
gpu = pytest.mark.gpu

TOL_Z = 4e-6                   # test_gpu_noise_streams.TOL_Z (asserted equal on the GPU run below)
PHILOX_NS = [63, 1000, 1025, 2049, 4096]
PHILOX_QS = [0.5, 0.9, 0.975]
# Chosen on the CPU from the reference alone (test_philox_reference_leaves_few_cells_ambiguous): about one seed in a thousand
# keeps all fifteen (n, q) cases under the cap, because the all-negative cell (std 1e-3 at |mean| 3: rank gaps below 4 delta)
# is ambiguous at almost every large n and the cap allows two cells.  Both halves of the seed are non-zero.
PHILOX_SEED = 0xBD22BBCCCC2
AMBIGUOUS_CAP = 0.05


def _infer(mean, std, metric, q, n, z=None, seed=0):
    import torch
    from benchnav_amd.risk import infer_risk_map
    zt = None if z is None else torch.from_numpy(np.array(z, f32))
    return infer_risk_map(torch.from_numpy(np.array(mean, f32)), torch.from_numpy(np.array(std, f32)), metric, q,
                          num_samples=n, z=zt, seed=seed).cpu().numpy()


def _same_value(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _check_cvar(got, smp, var, n, ctx, cells=None):
    """NaN pattern and the summation bound against the float64 tail mean; returns the largest error / bound."""
    ref64, scale = RC.tail_mean64(smp, var)
    sel = np.ones(got.shape, bool) if cells is None else cells
    assert np.array_equal(np.isnan(got)[sel], np.isnan(ref64)[sel]), f"{ctx}: CVaR NaN pattern"
    fin = sel & ~np.isnan(ref64)
    if not fin.any():
        return 0.0
    err, bound = np.abs(got.astype(np.float64) - ref64)[fin], RC.cvar_bound(n, scale)[fin]
    assert (err <= bound).all(), f"{ctx}: CVaR error {err.max():.3g}, ratio to bound {np.max(err / np.maximum(bound, 1e-300)):.3g}"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---- a. injected draws ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", RC.NS)
def test_injected_draws_every_case(n):
    mean, std = RC.maps()
    worst = 0.0
    for variant in RC.VARIANTS:
        z, smp = RC.draws(n, variant), RC.samples(n, variant)
        for q in RC.QS:
            ctx = f"n={n} q={q} {variant}"
            want = RO.infer_risk_map(mean, std, "var", q, z)
            got = _infer(mean, std, "var", q, n, z)
            bad = ~_same_value(got, want)
            assert not bad.any(), f"{ctx}: VaR differs in cells {np.argwhere(bad).tolist()}: {got[bad]} vs {want[bad]}"
            cvar = _infer(mean, std, "cvar", q, n, z)
            assert np.array_equal(np.isnan(cvar), np.isnan(RO.infer_risk_map(mean, std, "cvar", q, z))), f"{ctx}: CVaR NaN pattern"
            worst = max(worst, _check_cvar(cvar, smp, want, n, ctx))
    print(f"\ninjected n={n} (R={RC.capacity(n)}): VaR equal in all cells; CVaR error / bound max {worst:.3f}")


# ---- b. non-finite cells ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [200, 1000])
def test_non_finite_cells_give_nan_and_leave_their_neighbours(n):
    mean, std = (a.copy() for a in RC.maps())
    mean[0, 1], std[1, 0], mean[2, 2], mean[6, 4] = np.nan, np.nan, np.inf, -np.inf       # cells 1, 7, 16, 46
    bad = np.zeros((RC.G, RC.G), bool)
    bad[0, 1] = bad[1, 0] = bad[2, 2] = bad[6, 4] = True
    z = RC.draws(n)
    smp = RC.samples(n, "plain", mean, std)
    for q in (0.1, 0.5, 0.9, 1.0):
        ctx = f"n={n} q={q}"
        want = RO.infer_risk_map(mean, std, "var", q, z)
        assert np.isnan(want[bad]).all() and np.isfinite(want[~bad]).all()
        var = _infer(mean, std, "var", q, n, z)
        cvar = _infer(mean, std, "cvar", q, n, z)
        assert np.isnan(var[bad]).all() and np.isnan(cvar[bad]).all(), f"{ctx}: {var[bad]} {cvar[bad]}"
        assert _same_value(var, want).all(), ctx
        _check_cvar(cvar, smp, want, n, ctx, cells=~bad)
        for metric in ("var", "cvar"):                                                     # the Philox path: same cells, NaN
            got = _infer(mean, std, metric, q, n, seed=PHILOX_SEED)
            assert np.isnan(got[bad]).all(), f"{ctx} {metric} (Philox)"
            if metric == "var":                                                            # (CVaR is NaN wherever std = 0, too)
                assert np.isfinite(got[~bad]).all(), f"{ctx} (Philox)"


# ---- c. Philox draws at interior ranks ----------------------------------------------------------------------------------------
def _philox_reference(n, q):
    """float64 reference on rng_reference.risk: (var, cvar, delta, ulp, ambiguous, cvar scale), all (7, 7)."""
    mean, std = RC.maps(philox=True)
    m64, s64 = mean.astype(np.float64).ravel(), std.astype(np.float64).ravel()
    srt = np.sort(m64[:, None] + s64[:, None] * _philox_draws(n), axis=1)
    lo, hi, w = RC.rank(q, n)
    w = float(w)
    var = srt[:, lo] + w * (srt[:, hi] - srt[:, lo])
    tail = srt[:, lo + 1:]
    cvar = tail.mean(axis=1)
    scale = np.abs(tail).mean(axis=1)
    ulp = np.spacing((np.abs(m64) + 6.77 * s64).astype(f32)).astype(np.float64)
    delta = s64 * TOL_Z + 2 * ulp
    if w > 0:
        amb = (var - srt[:, lo] < 4 * delta) | (srt[:, hi] - var < 4 * delta)
    else:
        amb = srt[:, lo + 1] - srt[:, lo] < 4 * delta
    return tuple(a.reshape(RC.G, RC.G) for a in (var, cvar, delta, ulp, amb, scale))


_DRAWS = {}


def _philox_draws(n):
    if n not in _DRAWS:
        d = R.risk(PHILOX_SEED, RC.CELLS, n)
        d.setflags(write=False)
        _DRAWS[n] = d
    return _DRAWS[n]


@pytest.mark.parametrize("n", PHILOX_NS)
def test_philox_reference_leaves_few_cells_ambiguous(n):
    """CPU: the reference alone, for the committed seed, leaves at most 5 % of a case's cells out of the CVaR check."""
    for q in PHILOX_QS:
        lo, hi, w = RC.rank(q, n)
        assert 0 < lo and hi < n - 1, "an interior rank"
        amb = _philox_reference(n, q)[4]
        assert amb.mean() <= AMBIGUOUS_CAP, f"n={n} q={q}: {int(amb.sum())} of {amb.size} cells ambiguous; choose another PHILOX_SEED"


@gpu
@pytest.mark.parametrize("n", PHILOX_NS)
def test_philox_draws_at_interior_ranks(n):
    import test_gpu_noise_streams
    assert TOL_Z == test_gpu_noise_streams.TOL_Z
    mean, std = RC.maps(philox=True)
    worst_v = worst_c = 0.0
    left_out = 0
    for q in PHILOX_QS:
        ctx = f"n={n} q={q}"
        var, cvar, delta, ulp, amb, scale = _philox_reference(n, q)
        assert amb.mean() <= AMBIGUOUS_CAP, ctx
        got_v = _infer(mean, std, "var", q, n, seed=PHILOX_SEED).astype(np.float64)
        got_c = _infer(mean, std, "cvar", q, n, seed=PHILOX_SEED).astype(np.float64)
        rv = np.abs(got_v - var) / (delta + ulp)
        assert (rv <= 1).all(), f"{ctx}: VaR off by {np.abs(got_v - var).max():.3g}, {rv.max():.3g} x its bound (cell {rv.argmax()})"
        bound_c = delta + RC.cvar_bound(n, scale)
        rc = np.where(amb, 0.0, np.abs(got_c - cvar) / bound_c)
        assert np.isfinite(got_c[~amb]).all(), ctx
        assert (rc <= 1).all(), f"{ctx}: CVaR off by {np.abs(got_c - cvar)[~amb].max():.3g}, {rc.max():.3g} x its bound (cell {rc.argmax()})"
        worst_v, worst_c, left_out = max(worst_v, rv.max()), max(worst_c, rc.max()), left_out + int(amb.sum())
    print(f"\nPhilox n={n}: VaR error / bound max {worst_v:.3f}, CVaR error / bound max {worst_c:.3f}, "
          f"{left_out} of {len(PHILOX_QS) * RC.CELLS} cells left out of the CVaR check")


# ---- d / e / f: the C ABI -----------------------------------------------------------------------------------------------------
HOST, DEVICE = 0, 1


def _call(lib, mean, std, where_in, metric, q, n, z, where_z, seed, out, where_out, grid=RC.G, stream=0):
    """bn_risk_map_infer with numpy arrays (host) or torch tensors (device); returns the code."""
    def ptr(a):
        if a is None:
            return C.c_void_p(None)
        return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    return lib.bn_risk_map_infer(0, C.c_void_p(stream), ptr(mean), ptr(std), where_in, grid, metric, q, n, ptr(z), where_z, seed,
                                 ptr(out), where_out)


def _bits(a):
    import torch
    if isinstance(a, torch.Tensor):
        torch.cuda.synchronize()
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, f32).view(np.uint32).copy()


@gpu
@pytest.mark.parametrize("n", [65, 2049])
def test_host_memory_branches_equal_the_device_call(n):
    import torch
    from benchnav_amd import _capi
    lib = _capi.load()
    mean, std = (np.array(a, f32) for a in RC.maps())
    z = np.array(RC.draws(n, "halves"), f32)
    md, sd, zd = (torch.from_numpy(a).cuda() for a in (mean, std, z))
    torch.cuda.synchronize()
    q, cvar, ev = 0.9, _capi.BN_RISK_CVAR, _capi.BN_RISK_EXPECTED

    def run(m, s, w_in, metric, zz, w_z, w_out, seed=0):
        out = np.full((RC.G, RC.G), -7.0, f32) if w_out == HOST else torch.full((RC.G, RC.G), -7.0, device="cuda")
        torch.cuda.synchronize()
        rc = _call(lib, m, s, w_in, metric, q, n, zz, w_z, seed, out, w_out)
        assert rc == _capi.BN_OK, lib.bn_risk_last_error()
        return _bits(out)

    base = run(md, sd, DEVICE, cvar, zd, DEVICE, DEVICE)
    _check_cvar(base.view(f32), RC.samples(n, "halves"), RO.infer_risk_map(mean, std, "var", q, z), n, f"n={n} all device")
    assert np.array_equal(run(mean, std, HOST, cvar, z, HOST, HOST), base), "all host"
    assert np.array_equal(run(mean, std, HOST, cvar, zd, DEVICE, DEVICE), base), "host mean/std, device z and out"
    assert np.array_equal(run(md, sd, DEVICE, cvar, z, HOST, HOST), base), "device mean/std, host z and out"
    assert np.array_equal(run(mean, std, HOST, ev, None, DEVICE, HOST), mean.view(np.uint32)), "expected_value host in / out"
    seed = PHILOX_SEED
    philox = run(md, sd, DEVICE, cvar, None, DEVICE, DEVICE, seed)
    assert not np.array_equal(philox, base)
    assert np.array_equal(run(mean, std, HOST, cvar, None, HOST, HOST, seed), philox), "Philox mode host in / out"


REFUSALS = [  # id, keyword of the message, overrides
    ("n1", "num_samples", dict(n=1)), ("n4097", "num_samples", dict(n=4097)), ("grid0", "grid_size", dict(grid=0)),
    ("q-0.1", "confidence", dict(q=-0.1)), ("q1.5", "confidence", dict(q=1.5)), ("qnan", "confidence", dict(q=float("nan"))),
    ("metric", "metric", dict(metric=3)), ("null-out", "null", dict(null_out=True)),
]


@gpu
@pytest.mark.parametrize("word,over", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_at_the_c_abi(word, over):
    import torch
    from benchnav_amd import _capi
    lib = _capi.load()
    mean, std = (np.array(a, f32) for a in RC.maps())
    md, sd = torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()
    a = dict(metric=_capi.BN_RISK_CVAR, q=0.9, n=200, grid=RC.G, null_out=False)
    a.update(over)
    for where in (HOST, DEVICE):
        out = np.full((RC.G, RC.G), -7.0, f32) if where == HOST else torch.full((RC.G, RC.G), -7.0, device="cuda")
        torch.cuda.synchronize()
        m, s = (mean, std) if where == HOST else (md, sd)
        rc = _call(lib, m, s, where, a["metric"], a["q"], a["n"], None, DEVICE, 1, None if a["null_out"] else out, where, grid=a["grid"])
        msg = lib.bn_risk_last_error().decode()
        assert rc == _capi.BN_ERR_INVALID and msg and word in msg, (rc, msg)
        assert (_bits(out) == f32(-7.0).view(np.uint32)).all(), "a refused call wrote to out"


@gpu
def test_expected_value_accepts_any_sample_count():
    from benchnav_amd import _capi
    lib = _capi.load()
    mean, std = (np.array(a, f32) for a in RC.maps())
    for n in (-5, 0, 1, 4097, 1 << 30):
        out = np.full((RC.G, RC.G), -7.0, f32)
        assert _call(lib, mean, std, HOST, _capi.BN_RISK_EXPECTED, 0.0, n, None, DEVICE, 0, out, HOST) == _capi.BN_OK
        assert np.array_equal(_bits(out), mean.view(np.uint32))


@gpu
def test_determinism_side_stream_and_seed_halves():
    import torch
    from benchnav_amd.risk import infer_risk_map
    mean, std = RC.maps()
    n, q = 1025, 0.975
    z = RC.draws(n, "halves")
    for kw in (dict(z=z), dict(seed=PHILOX_SEED)):
        for metric in ("var", "cvar"):
            a, b = _infer(mean, std, metric, q, n, **kw), _infer(mean, std, metric, q, n, **kw)
            assert np.array_equal(_bits(a), _bits(b)), (metric, list(kw))
    # a side stream whose inputs are written on that stream, behind a long-running product, with no synchronisation in between
    md, sd, zd = (torch.from_numpy(np.array(a, f32)).cuda() for a in (mean, std, z))
    m2, s2, z2 = torch.zeros_like(md), torch.zeros_like(sd), torch.zeros_like(zd)
    busy = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):
            busy = busy @ busy * 1e-3
        m2.copy_(md); s2.copy_(sd); z2.copy_(zd)
        got_z = infer_risk_map(m2, s2, "cvar", q, num_samples=n, z=z2)
        got_p = infer_risk_map(m2, s2, "cvar", q, num_samples=n, seed=PHILOX_SEED)
    side.synchronize()
    assert np.array_equal(_bits(got_z), _bits(_infer(mean, std, "cvar", q, n, z=z)))
    assert np.array_equal(_bits(got_p), _bits(_infer(mean, std, "cvar", q, n, seed=PHILOX_SEED)))
    # the high half of the seed is part of the key
    lo_only = _infer(mean, std, "var", q, n, seed=5)
    assert not np.array_equal(lo_only, _infer(mean, std, "var", q, n, seed=5 | (1 << 32)))
    assert not np.array_equal(lo_only, _infer(mean, std, "var", q, n, seed=5 | (1 << 63)))
    assert not np.array_equal(lo_only, _infer(mean, std, "var", q, n, seed=6))
