"""GPU: the library's in-kernel noise streams against an independent reference (tests/rng_reference.py).

  a. the raw generator (bn_device_rng_eval: the kernels' own philox4x32 and box_muller) word for word against the reference;
  b. bn_mppi_get_philox_noise / bn_mppi_get_slip_noise against the reference's stream layouts: seeds, instances, solve indices,
     ragged K, odd T, rollout offsets;
  c. every rollout-kernel family consumes exactly what (b) regenerates: instance 2 of a B = 3 handle bit-exact against the oracle;
  d. the risk-map stream through exact order statistics (VaR at confidences that land on a rank);
  e. the env-step and collision-check draws;
  f. statistics of the device draws (2^24 per stream; every bound at 6 sigma or alpha ~ 1e-6).

TOL_Z: device Box-Muller (v_log_f32, v_sqrt_f32, v_sin_f32, v_cos_f32) against float64 on the same words.  Measured on MI355X
over 2^20 random word pairs, the 256 smallest first words (the largest radii) and the edge words (test_box_muller_matches_float64):
largest absolute deviation 9.8e-7 (at a = 0xfe, radius 6.6), largest relative to the radius 2.6e-7, mean 6.1e-8.  The bound is
about 4x the largest.  Any wrong word or counter moves a draw by O(1)."""
import ctypes as C
import math

import numpy as np
import pytest

import rng_reference as R
from helpers import assert_oracle_parity, oracle_metrics

pytestmark = pytest.mark.gpu

TOL_Z = 4e-6
MASK = 0xFFFFFFFF


def _rng_eval(fn, words):
    """bn_device_rng_eval on (n, 6) / (n, 2) uint32 records -> (n, 4) / (n, 2) uint32."""
    import torch
    from benchnav_amd import _capi
    lib = _capi.load()
    words = np.ascontiguousarray(words, np.uint32)
    n = words.shape[0]
    per_out = 2 if fn == 2 else 4
    assert words.shape == (n, 2 if fn == 2 else 6)
    xd = torch.from_numpy(words.view(np.int32)).cuda()
    out = torch.empty(n * per_out, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _capi.check(lib.bn_device_rng_eval(fn, C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()), n, C.c_void_p(0)))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(n, per_out)


def _device_box_muller(a, b):
    out = _rng_eval(2, np.stack([np.asarray(a, np.uint32).ravel(), np.asarray(b, np.uint32).ravel()], 1)).view(np.float32)
    return out[:, 0], out[:, 1]


# ---- a. raw words ------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("fn,rounds", [(0, 10), (1, R.STREAM_ROUNDS)], ids=["philox10", "stream-rounds"])
def test_philox_words_equal_the_reference(fn, rounds):
    rng = np.random.default_rng(100 + fn)
    rec = rng.integers(0, 1 << 32, (1 << 20, 6), dtype=np.uint64).astype(np.uint32)
    rec[:3] = [list(c) + list(k) for c, k, _ in KAT]
    rec[3:8] = [[MASK, 0, MASK, 0, MASK, 0], [0, MASK, 0, MASK, 0, MASK], [1, 2, 3, 4, 5, 6], [0, 0, 0, 0, MASK, 0], [0, 0, 0, 0, 0, MASK]]
    got = _rng_eval(fn, rec)
    want = np.stack(R.philox4x32(*rec.T, rounds=rounds), 1)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, f"{bad.size} blocks differ, first {bad[:5]}: {got[bad[:2]]} vs {want[bad[:2]]}"
    if fn == 0:
        for i, (_, _, w) in enumerate(KAT):
            assert tuple(int(x) for x in got[i]) == w


EDGE_A = [0, 1, 0xFFFFFF7F, 0xFFFFFF80, MASK]
EDGE_B = [0, 1 << 30, 1 << 31, 0xC0000000, MASK]


def test_box_muller_matches_float64():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    # the words that make u1 smallest / closest to one, and the quarter turns
    a[:256] = np.arange(256)
    a[256:512] = 0xFFFFFF80 - np.arange(1, 257) * 128
    ea, eb = np.meshgrid(np.array(EDGE_A, np.uint32), np.array(EDGE_B, np.uint32), indexing="ij")
    a = np.concatenate([a, ea.ravel()]); b = np.concatenate([b, eb.ravel()])
    z0, z1 = _device_box_muller(a, b)
    r0, r1 = R.box_muller(a, b)
    d = np.maximum(np.abs(z0 - r0), np.abs(z1 - r1))
    rad = np.hypot(r0, r1)
    rel = d[rad > 0] / rad[rad > 0]
    print(f"\nbox_muller vs float64: max |dz| = {d.max():.3e} (at a={a[d.argmax()]:#x}, b={b[d.argmax()]:#x}), "
          f"max |dz|/radius = {rel.max():.3e}, mean |dz| = {d.mean():.3e}")
    assert d.max() <= TOL_Z, (d.max(), a[d.argmax()], b[d.argmax()])
    n_edge = ea.size
    ez0, ez1, er0, er1 = z0[-n_edge:], z1[-n_edge:], r0[-n_edge:], r1[-n_edge:]
    assert (ez0[er0 == 0] == 0).all() and (ez1[er1 == 0] == 0).all()       # u1 == 1: exactly zero
    assert np.abs(np.hypot(z0, z1)).max() <= 6.7638
    big = a == 0
    assert np.abs(np.hypot(z0[big], z1[big]) - R.MAX_RADIUS).max() <= TOL_Z


# ---- b. regenerated streams ---------------------------------------------------------------------------------------------
SEEDS = [42, 42 | (1 << 32), 42 | (0xFFFFFFFE << 32), 0x9E3779B97F4A7C15]
SOLVES = [0, 1, (1 << 20) - 1, 1 << 20, (1 << 32) + 7]


def _handle(K, T, B, seed, **kw):
    from benchnav_amd import NativeMPPI
    kw.setdefault("lean", not kw.get("sampled_slip", False))      # no trajectory batch to allocate: the getters under test draw alone
    return NativeMPPI(horizon=T, num_samples=K, grid_size=16, resolution=0.5, num_instances=B, shared_map=True, seed=seed, **kw)


@pytest.mark.parametrize("K,T,B,k0", [(130, 7, 3, 0), (64, 50, 3, 0), (97, 8, 4, 1000), (65, 3, 4097, 77777)],
                         ids=["ragged-oddT", "evenT", "offset", "B4097-offset"])
def test_philox_noise_equals_the_reference_stream(K, T, B, k0):
    for seed in SEEDS:
        with _handle(K, T, B, seed) as pl:
            if k0:
                pl.set_rollout_offset(k0)
            for b in sorted({0, 1, B - 1}):
                for s in SOLVES:
                    got = pl.philox_noise(s, b)
                    want = R.eps(seed, s, b, K, T, k0)
                    d = np.abs(got - want).max()
                    assert d <= TOL_Z, f"seed={seed:#x} b={b} solve={s}: max|d|={d:.3g}"


@pytest.mark.parametrize("K,T,B,k0", [(130, 7, 3, 0), (64, 8, 3, 0), (97, 9, 3, 1000), (64, 50, 3, 12345)],
                         ids=["ragged-oddT", "evenT", "offset-oddT", "offset-T50"])
def test_slip_noise_equals_the_reference_stream(K, T, B, k0):
    """With a rollout offset the sampled kernels key their slip draws by k + k0; the regeneration must too."""
    for seed in SEEDS[:3]:
        with _handle(K, T, B, seed, sampled_slip=True) as pl:
            if k0:
                pl.set_rollout_offset(k0)
            for b in sorted({0, 1, B - 1}):
                for s in SOLVES:
                    got = pl.slip_noise(s, b)
                    want = R.slip(seed, s, b, K, T, k0)
                    for nm, g, w in zip(("zt", "zc", "zo"), got, want):
                        d = np.abs(g - w).max()
                        assert d <= TOL_Z, f"{nm} seed={seed:#x} b={b} solve={s} k0={k0}: max|d|={d:.3g}"


# ---- c. consumed equals regenerated, every kernel family ---------------------------------------------------------------
FAMILIES = [  # id, K, T, kernel, options
    ("role", 130, 7, "role", {}),
    ("role-2launch", 130, 7, "role", dict(pipeline=False)),
    ("role-lean", 130, 9, "role", dict(lean=True)),
    ("wave", 130, 7, "wave", {}),
    ("wave-lean", 130, 9, "wave", dict(lean=True)),
    ("lat", 130, 7, "lat", {}),
    ("lat-lean", 100, 33, "lat", dict(lean=True)),
    ("auto", 130, 7, "auto", {}),
    ("ticket-K2113", 2113, 9, "auto", {}),
    ("ticket-K2113-2launch", 2113, 9, "auto", dict(pipeline=False)),
    ("role-reference-order", 130, 7, "role", dict(reference_order=True)),
    ("lat-reference-order", 130, 7, "lat", dict(reference_order=True)),
    ("sampled", 130, 7, "auto", dict(sampled_slip=True)),
    ("sampled-2launch", 130, 7, "auto", dict(sampled_slip=True, pipeline=False)),
    ("sampled-K2113", 2113, 9, "auto", dict(sampled_slip=True)),
]


@pytest.mark.parametrize("K,T,kernel,opts", [f[1:] for f in FAMILIES], ids=[f[0] for f in FAMILIES])
def test_every_kernel_family_consumes_the_regenerated_stream(K, T, kernel, opts):
    from benchnav_amd import NativeMPPI, synth
    from oracle import oracle as O
    B, G, res, k0, seed = 3, 64, 0.5, 4321, (7 << 32) | 5
    lean, sampled = opts.get("lean", False), opts.get("sampled_slip", False)
    insts = [synth.make_instance(G, seed=60 + b, jitter=True) for b in range(B)]
    sgs = [synth.slip_std_map(G, seed=60 + b).numpy() for b in range(B)]
    states = np.stack([it.start.numpy() for it in insts]).astype(np.float32)
    with NativeMPPI(horizon=T, num_samples=K, grid_size=G, resolution=res, num_instances=B, seed=seed, kernel=kernel,
                    store_controls=not lean, **opts) as pl:
        for b, it in enumerate(insts):
            pl.set_map(it.risk.numpy(), b); pl.set_goal(it.goal.numpy(), b)
            if sampled:
                pl.set_slip_std(sgs[b], b)
        pl.set_rollout_offset(k0)
        us0, _ = pl.solve(states)
        us1, xs1 = pl.solve(states)                       # warm-started from the kernel's own U*: solve index 1
        assert pl.solve_count() == 2
        b = 2
        eps = pl.philox_noise(1, b)
        assert np.abs(eps - R.eps(seed, 1, b, K, T, k0)).max() <= TOL_Z
        got = dict(X=pl.states(b), cost=pl.costs(b), w=pl.weights(b), Ustar=us1[b], Xstar=xs1[b])
        got["U"] = None if lean else pl.controls(b)
        if sampled:
            z = pl.slip_noise(1, b)
            for g, w in zip(z, R.slip(seed, 1, b, K, T, k0)):
                assert np.abs(g - w).max() <= TOL_Z
    trig = O.TRIG_SPEC_PER_STEP if opts.get("reference_order") else O.TRIG_SPEC
    p = O.make_params(K, T, G, res, insts[b].goal.numpy(), trig=trig)
    if sampled:
        orc = O.solve_sampled(p, insts[b].risk.numpy(), sgs[b], states[b], us0[b], eps, *z)
    else:
        orc = O.solve(p, insts[b].risk.numpy(), states[b], us0[b], eps)
    if lean:
        got["U"] = orc["U"]                                # not stored in lean mode: X and the costs carry it
    assert_oracle_parity(oracle_metrics(got, orc), ctx=f"{kernel} {opts} instance {b}")


# ---- d. risk-map stream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 63, 1000, 1025, 2049, 4096])
def test_risk_map_draws_are_the_reference_order_statistics(n):
    """mean 0, std 1: every sample is its draw, and VaR at a confidence q with fp32(q) (n - 1) an integer is one order statistic
    exactly (no interpolation).  G = 7: 49 cells, not a multiple of the kernel's four cells per workgroup."""
    import torch
    from benchnav_amd.risk import infer_risk_map
    G, seed = 7, (3 << 32) | 0x51
    mean, std = torch.zeros(G, G), torch.ones(G, G)
    want = np.sort(R.risk(seed, G * G, n), axis=1)
    qs = [0.0, 1.0] + ([1 / 3, 2 / 3] if n == 4 else [])
    for q in qs:
        pos = np.float32(q) * np.float32(n - 1)
        assert pos == np.floor(pos)
        got = infer_risk_map(mean, std, "var", q, num_samples=n, seed=seed).cpu().numpy().ravel()
        d = np.abs(got - want[:, int(pos)]).max()
        assert d <= TOL_Z, f"n={n} q={q}: max|d|={d:.3g}"


# ---- e. env-step and collision draws ---------------------------------------------------------------------------------------
ENV_SEED = (5 << 32) | 11


def _env_handle(B, G=32):
    from benchnav_amd import NativeMPPI
    pl = NativeMPPI(horizon=4, num_samples=64, grid_size=G, resolution=0.5, num_instances=B, shared_map=True, stream=0)
    mu, sg = np.full((G, G), 0.5, np.float32), np.full((G, G), 0.07, np.float32)
    pl.set_map(mu)
    for b in range(B):
        pl.set_goal(np.array([1.0, 1.0], np.float32), b)
    pl.env_attach(mu, sg, goal_threshold=0.25, delta_t=0.1, seed=ENV_SEED)
    return pl


def test_env_step_draws_equal_the_reference():
    """slip = z 0.07 + 0.5 never clamps (|z| <= 6.77): the reward is 1 - slip, the step a float64 unicycle step on the reference draw."""
    import torch
    from benchnav_amd import _capi
    B = 1000
    rng = np.random.default_rng(11)
    with _env_handle(B) as pl:
        lib = pl._lib
        for step in (0, 1, 77, (1 << 32) + 5, (1 << 64) - 1):
            st = np.stack([rng.uniform(4, 12, B), rng.uniform(4, 12, B), rng.uniform(-2, 2, B)], 1).astype(np.float32)
            act = np.stack([rng.uniform(0.2, 1, B), rng.uniform(-1, 1, B)], 1).astype(np.float32)
            sd, ad = torch.from_numpy(st.copy()).cuda(), torch.from_numpy(act).cuda()
            rw, term = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            _capi.check(lib.bn_mppi_env_step(pl._h, C.c_void_p(ad.data_ptr()), C.c_void_p(sd.data_ptr()), C.c_void_p(rw.data_ptr()),
                                             C.c_void_p(term.data_ptr()), None, step))
            torch.cuda.synchronize()
            z = R.env_step(ENV_SEED, np.arange(B), step)
            trav = 1.0 - (z * 0.07 + 0.5)
            d = np.abs(rw.cpu().numpy() - trav).max()
            assert d <= 0.07 * TOL_Z + 2.5e-7, f"step {step}: reward max|d|={d:.3g}"
            x, y, th = st[:, 0].astype(np.float64), st[:, 1].astype(np.float64), st[:, 2].astype(np.float64)
            v, om = act[:, 0].astype(np.float64), act[:, 1].astype(np.float64)
            want = np.stack([x + trav * v * np.cos(th) * 0.1, y + trav * v * np.sin(th) * 0.1, th + trav * om * 0.1], 1)
            d = np.abs(sd.cpu().numpy() - want).max()
            assert d <= 1e-5, f"step {step}: state max|d|={d:.3g}"


def test_collision_draws_equal_the_reference():
    """Flags are (1 - clamp(z 0.07 + 0.5)) <= thr with thr = 0.5: they may differ from the reference's only where its slip lies
    within the draw tolerance of the threshold."""
    import torch
    from benchnav_amd import _capi
    B, N, thr = 1000, 64, 0.5
    rng = np.random.default_rng(12)
    pos = np.concatenate([rng.uniform(0.5, 15.5, (B, N, 2)), rng.uniform(-3, 3, (B, N, 1))], 2).astype(np.float32)
    with _env_handle(B) as pl:
        pd = torch.from_numpy(pos).cuda()
        out = torch.empty(B * N, dtype=torch.uint8, device="cuda")
        for draw in (0, 7, (1 << 32) + 3):
            torch.cuda.synchronize()
            _capi.check(pl._lib.bn_mppi_env_collision_check(pl._h, C.c_void_p(pd.data_ptr()), N, thr, None, draw, C.c_void_p(out.data_ptr())))
            torch.cuda.synchronize()
            got = out.cpu().numpy().astype(bool)
            slip = R.collision(ENV_SEED, np.arange(B * N, dtype=np.uint64), draw) * 0.07 + 0.5
            want = (1.0 - slip) <= thr
            near = np.abs(slip - (1 - thr)) <= 0.07 * TOL_Z + 2.5e-7
            bad = (got != want) & ~near
            assert not bad.any(), f"draw {draw}: {bad.sum()} flags differ away from the threshold"
            assert 0.45 < got.mean() < 0.55


# ---- f. statistics of the device draws --------------------------------------------------------------------------------------
def _normal_checks(z, what):
    """z: float64 draws, n >= 2^24.  Every bound at 6 sigma or alpha ~ 1e-6."""
    from scipy import special, stats
    n = z.size
    m = z.mean()
    c = z - m
    var = (c * c).mean()
    skew = (c ** 3).mean() / var ** 1.5
    kurt = (c ** 4).mean() / var ** 2 - 3
    assert abs(m) < 6 / math.sqrt(n), (what, "mean", m)
    assert abs(var - 1) < 6 * math.sqrt(2 / n), (what, "variance", var)
    assert abs(skew) < 6 * math.sqrt(6 / n), (what, "skewness", skew)
    assert abs(kurt) < 6 * math.sqrt(24 / n), (what, "excess kurtosis", kurt)
    u = special.ndtr(np.sort(z))
    i = np.arange(1, n + 1) / n
    ks = max((i - u).max(), (u - (i - 1 / n)).max())
    assert ks < math.sqrt(math.log(2 / 1e-6) / 2) / math.sqrt(n), (what, "KS", ks)
    counts = np.bincount(np.minimum((special.ndtr(z) * 1024).astype(np.int64), 1023), minlength=1024)
    chi2 = ((counts - n / 1024) ** 2 / (n / 1024)).sum()
    assert chi2 < stats.chi2.isf(1e-6, 1023), (what, "chi2", chi2)
    for t in (2, 3, 4, 5):
        p = 2 * special.ndtr(-t)
        k = int((np.abs(z) > t).sum())
        lo, hi = stats.binom.ppf(5e-7, n, p), stats.binom.isf(5e-7, n, p)
        assert lo <= k <= hi, (what, f"P(|z| > {t})", k, n * p)
    assert np.abs(z).max() <= 6.7638, (what, "max |z|")


def _corr_ok(a, b, what):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    r = np.corrcoef(a, b)[0, 1]
    assert abs(r) < 6 / math.sqrt(a.size), (what, r, a.size)


def test_control_noise_statistics():
    K, T, S, seed = 4096, 64, 32, 1234567
    with _handle(K, T, 2, seed) as pl:
        e = np.stack([pl.philox_noise(s, 0) for s in range(S)]).astype(np.float64)          # (S, K, T, 2): 2^24 draws
        e_b1 = np.stack([pl.philox_noise(s, 1) for s in range(4)]).astype(np.float64)
    with _handle(K, T, 1, seed + 1) as pl:
        e_s1 = np.stack([pl.philox_noise(s, 0) for s in range(4)]).astype(np.float64)
    with _handle(K, T, 1, seed, sampled_slip=True) as pl:
        zt = np.stack([pl.slip_noise(s, 0)[0] for s in range(4)]).astype(np.float64)
    assert e.size >= 1 << 24
    _normal_checks(e.ravel(), "control noise")
    _corr_ok(e[..., 0], e[..., 1], "v / omega")
    _corr_ok(e[:, :, 0::2], e[:, :, 1::2], "steps t / t+1 (one block)")
    _corr_ok(e[:, :, :-2], e[:, :, 2:], "steps t / t+2")
    _corr_ok(e[:, :-1], e[:, 1:], "rollouts k / k+1")
    _corr_ok(e[:4], e_b1, "instances b / b+1")
    _corr_ok(e[:-1], e[1:], "solves s / s+1")
    _corr_ok(e[:4], e_s1, "seeds s / s+1")
    _corr_ok(e[:4, ..., 0], zt, "slip draws / control noise of the same (k, t)")


def test_slip_noise_statistics():
    K, T, S, seed = 4096, 64, 32, 7654321
    with _handle(K, T, 1, seed, sampled_slip=True) as pl:
        draws = [pl.slip_noise(s, 0) for s in range(S)]
    z = np.concatenate([np.concatenate([zt.ravel(), zc.ravel(), zo]) for zt, zc, zo in draws]).astype(np.float64)
    assert z.size >= 1 << 24
    _normal_checks(z, "slip draws")
    zt = np.stack([d[0] for d in draws]).astype(np.float64)
    zc = np.stack([d[1] for d in draws]).astype(np.float64)
    _corr_ok(zt, zc[:, :, :T], "transit / cost draws of one block")
    _corr_ok(zt[:, :, :-1], zt[:, :, 1:], "transit steps t / t+1")
    _corr_ok(zt[:, :-1], zt[:, 1:], "rollouts k / k+1")
    _corr_ok(zt[:-1], zt[1:], "solves s / s+1")
