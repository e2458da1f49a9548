"""GPU: the softmin merge and the tail of a solve (csrc/mppi_merge.h, csrc/mppi_tail.h, shard_merge_kernel) against the float64
restatement tests/mppi_tail_spec.py, on inputs that put the weight where the code changes form (tests/mppi_tail_cases.py), over every
path that ends in this code.

One checker, check_tail: U, X and cost equal the CPU oracle bit for bit; w and U* lie within the DERIVED bound of
tail(cost_device, U_device, lambda) (mppi_tail_spec: expf and division as HIP documents them, the exponent roundings of the row-wise
form, the sums' roundings -- no fixed number); X* is bit-equal to oracle.rollout of the DEVICE's U*; sum(w) is 1 within the bound; in
the one-hot cases w is exactly one-hot, U* == U[k*] and X* == X[k*].  Every test prints measured / bound per path.

Paths (PATHS below): the latency kernel's self tail with and without granules, its aux tail, the role kernel's aux tail through
solve_n_async_device, the one-wave kernel's single-wave tail with nine instances, the two-launch finish kernel with 320 and 1024
threads, the ticket merge in two levels, the plain branch beyond 1024 rows (K = 65600), sampled slip fused and from global memory,
the reference order, the K-shard three-call protocol; the prologue merge of every pipelined family through a chain of two solves."""
import numpy as np
import pytest

import mppi_tail_cases as TC
from mppi_tail_spec import ratios, tail

pytestmark = pytest.mark.gpu


# ---- the checker (also applied to corrupted oracle outputs by tests/test_mppi_tail_spec.py, without a GPU) -------------------------
def check_tail(got, case, b=0, ref=False, orc=None, xstar=True):
    """got: dict(U, X, cost, w, Ustar, Xstar) of one instance as a planner returned them.  `orc`: the CPU oracle's solve of the same
    inputs (default: the plain solve of instance b; the sampled-slip tests pass their own).  xstar=False leaves X* out (sampled slip:
    X* uses draws of its own).  Returns measured / bound for w, U* and sum(w)."""
    from oracle import oracle as O
    inst, name = case["inst"][b], (case["name"], b)
    orc = TC.reference(case, b, ref) if orc is None else orc
    for k in ("U", "X", "cost"):
        assert np.array_equal(got[k], orc[k]), (name, k, "differs from the oracle")
    spec = tail(got["cost"], got["U"], case["lam"])
    r = ratios(got["w"], got["Ustar"], spec)
    assert got["w"].dtype == np.float32 and got["Ustar"].dtype == np.float32
    assert r["w"] <= 1.0, (name, "weights beyond the derived bound", r)
    assert r["U"] <= 1.0, (name, "U* beyond the derived bound", r)
    assert r["sum"] <= 1.0, (name, "sum of the weights", r)
    if xstar:
        want = O.rollout(TC.oracle_params(case, b, ref), inst["R"], inst["state"], got["Ustar"])
        assert np.array_equal(got["Xstar"], want), (name, "X* is not the rollout of the device's U*", float(np.abs(got["Xstar"] - want).max()))
    if case["kind"] == "onehot":
        ks = inst["kstar"]
        hot = np.zeros(case["K"], np.float32)
        hot[ks] = 1
        assert np.array_equal(got["w"], hot), (name, "w is not one-hot", np.nonzero(got["w"])[0][:8], got["w"][ks])
        assert np.array_equal(got["Ustar"], got["U"][ks]), (name, "U* != U[k*]")
        if xstar:
            assert np.array_equal(got["Xstar"], got["X"][ks]), (name, "X* != X[k*]")
    return r


# ---- running a case on a planner ------------------------------------------------------------------------------------------------------
def _planner(case, B=1, **kw):
    from benchnav_amd import NativeMPPI
    return NativeMPPI(horizon=case["T"], num_samples=case["K"], grid_size=case["G"], resolution=case["res"], x_limits=list(case["xl"]),
                      y_limits=list(case["yl"]), sigmas=case["sigma"], inv_var=case["inv_var"], lambda_=case["lam"], u_min=case["u_min"],
                      u_max=case["u_max"], stuck_threshold=case["thr"], num_instances=B, store_controls=True, **kw)


def _load(pl, case):
    for b, i in enumerate(case["inst"]):
        pl.set_map(i["R"], b); pl.set_goal(i["goal"], b); pl.set_mean(i["mean"], b)


def _device_eps(eps, t2k):
    """eps (..., K, T, 2) on the device in one of the two injected layouts."""
    import torch
    from benchnav_amd import _capi
    if t2k:
        nd = eps.ndim
        perm = tuple(range(nd - 3)) + (nd - 2, nd - 1, nd - 3)
        return torch.from_numpy(np.ascontiguousarray(eps.transpose(perm))).cuda(), _capi.BN_NOISE_DEVICE_T2K
    return torch.from_numpy(np.ascontiguousarray(eps)).cuda(), _capi.BN_NOISE_DEVICE_KT2


def _outputs(pl, B, T, us=None, xs=None):
    import torch
    from benchnav_amd import _capi
    from benchnav_amd.mppi import _DevArray
    if xs is None:
        xs = torch.as_tensor(_DevArray(pl.device_buffer(_capi.BN_BUF_XSTAR)[0], (B, T + 1, 3)), device="cuda").cpu().numpy()
    out = []
    for b in range(B):
        mean = pl.get_mean(b)
        if us is not None:
            assert np.array_equal(us[b], mean), "the next mean is not U*"
        out.append(dict(U=pl.controls(b), X=pl.states(b), cost=pl.costs(b), w=pl.weights(b), Ustar=mean, Xstar=xs[b].copy()))
    return out


def run_case(pl, case, mode, t2k=False):
    """One solve of `case` on the loaded planner `pl`; the outputs per instance."""
    import torch
    B, T = len(case["inst"]), case["T"]
    eps = np.stack([i["eps"] for i in case["inst"]])
    st = np.stack([i["state"] for i in case["inst"]])
    _load(pl, case)
    if mode == "solve":
        us, xs = pl.solve(st, eps)
        return _outputs(pl, B, T, us, xs)
    std = torch.from_numpy(st).cuda()
    ed, kind = _device_eps(eps, t2k)
    torch.cuda.synchronize()
    if mode == "async":
        pl.solve_async_device(std.data_ptr(), ed.data_ptr(), kind)
    else:
        pl.solve_n_async_device(1, std.data_ptr(), ed.data_ptr(), kind, 1, eps.size)
    pl.sync()
    return _outputs(pl, B, T)


def plan_of(case, B, flags):
    import torch
    from benchnav_amd import _capi
    from mppi_plan_spec import plan
    entry = dict(num_samples=case["K"], horizon=case["T"], grid_size=case["G"], resolution=case["res"], num_instances=B, lambda_=case["lam"],
                 stuck_threshold=case["thr"], flags=tuple(flags))
    status, p = plan(_capi.load(), _capi, entry, torch.cuda.get_device_properties(0).multi_processor_count)
    assert status == 0, (case["name"], status)
    return p


# The latency kernel keeps a ring of (T + 1) x 64 float4 in LDS (lat_lds_bytes): with this map's 17 x 17 window it no longer fits the
# 160 KiB from T = 100 on, the plan hands the solve to the role kernel whatever the knob says, and the horizons 160 / 161 of the sweep run
# there.  T = 99 is swept on top of the list, so that the latency kernel's own column blocks (2T = 198 > c0 = 128, one pass of 320
# threads) are visited at their largest.
LAT_MAX_T = 99

# path -> planner knobs, how the solve is issued, the plan's flags, the row counts it takes, and what the plan must say
PATHS = {
    "lat-self": dict(kw=dict(kernel="lat"), mode="solve", flags=("LAT_KERNEL",), rows=(1, 2, 16, 17, 24, 25, 32, 33, 64),
                     plan=lambda p, rows, T: p["lat_kernel"] == int(T <= LAT_MAX_T) and p["has_granules"] == int(rows <= 16 and T <= LAT_MAX_T)),
    "lat-aux": dict(kw=dict(kernel="lat", stream=0), mode="async", flags=("LAT_KERNEL",), rows=(1, 2, 16, 17, 33, 64),
                    plan=lambda p, rows, T: p["lat_kernel"] == 1),
    "role": dict(kw=dict(kernel="role", stream=0), mode="chain", flags=("ROLE_KERNEL",), rows=(1, 2, 16, 17, 24, 25, 32, 33, 64),
                 plan=lambda p, rows, T: p["pipelined"] == 1 and not p["lat_kernel"] and not p["wave_kernel"]),
    "wave": dict(kw=dict(kernel="wave", stream=0), mode="async", flags=("WAVE_KERNEL",), rows=(1, 2, 16, 17, 24, 25, 32), B=9,
                 plan=lambda p, rows, T: p["wave_kernel"] == 1),
    "two-launch": dict(kw=dict(pipeline=False, stream=0), mode="async", flags=("NO_PIPELINE",), rows=TC.ROWS,
                       plan=lambda p, rows, T: not p["pipelined"] and not p["ticket_mode"]),
    "ticket": dict(kw=dict(stream=0), mode="async", flags=(), rows=(65, 80, 81, 1009, 1024),
                   plan=lambda p, rows, T: p["ticket_mode"] == 1 and not p["pipelined"]),
    "plain": dict(kw=dict(stream=0), mode="async", flags=(), rows=(1025,),
                  plan=lambda p, rows, T: p["nblk"] > 1024 and not p["pipelined"] and not p["ticket_mode"]),
}
REF_PATHS = {"lat-self": (2, 17), "role": (2, 17), "two-launch": (2, 17, 65), "ticket": (65,)}      # reference order; 65 rows are no pipelined size
T_SWEEP = {"lat-self": 2, "role": 2, "wave": 2, "two-launch": 2, "ticket": 65}      # path -> the row count its horizons are swept at
VISITED = set()          # (path, rows, K, k*, T, lambda, reference order) of every one-hot solve that was checked
RATIOS = {}


def _note(path, r):
    cur = RATIOS.setdefault(path, dict(w=0.0, U=0.0, sum=0.0, n=0))
    for k in ("w", "U", "sum"):
        cur[k] = max(cur[k], r[k])
    cur["n"] += 1


def _report(path, what):
    c = RATIOS.get(path)
    if c:
        print(f"\nmppi tail [{path}] {what}: measured/bound so far over {c['n']} solves: w {c['w']:.3g}  U* {c['U']:.3g}  sum(w) {c['sum']:.3g}")


def _planned(path, rows, T=TC.BASE_T, lam=0.5, ref=False):
    """The one-hot solves of one (path, row count): every K of the row count, every k* that K admits."""
    return {(path, rows, K, ks, T, lam, ref) for K in TC.sizes(rows) for ks in TC.kstars(K)}


def _sweep(path, rows, T=TC.BASE_T, lam=0.5, ref=False):
    """All k* of a row count and its ragged twin on one path: one handle per K; a batched path takes every k* in one launch."""
    spec = PATHS[path]
    B = spec.get("B", 1)
    kw = dict(spec["kw"], reference_order=True) if ref else spec["kw"]
    flags = spec["flags"] + (("REFERENCE_ORDER",) if ref else ())
    for K in TC.sizes(rows):
        cases = [TC.batch(B, K, T, lam)] if B > 1 else [TC.one_hot(K, T, ks, lam) for ks in TC.kstars(K)]
        assert spec["plan"](plan_of(cases[0], B, flags), rows, T), (path, K, T, "the plan does not take this path")
        with _planner(cases[0], B, **kw) as pl:
            assert pl.arithmetic() == ("reference_order" if ref else "spec")
            for n, case in enumerate(cases):
                outs = run_case(pl, case, spec["mode"], t2k=bool(n & 1))
                for b, got in enumerate(outs):
                    TC.conditions(case, b, TC.reference(case, b, ref))
                    _note(path, check_tail(got, case, b, ref))
                    VISITED.add((path, rows, K, case["inst"][b]["kstar"], T, lam, ref))
            assert pl.recovery_count() == 0
    _report(path, f"rows {rows} T {T} lambda {lam}{' reference order' if ref else ''}")


ROW_PARAMS = [(path, rows) for path, spec in PATHS.items() for rows in spec["rows"]]


@pytest.mark.parametrize("path,rows", ROW_PARAMS, ids=[f"{p}-{r}" for p, r in ROW_PARAMS])
def test_one_hot_weight_at_every_row_count(path, rows):
    _sweep(path, rows)


T_PARAMS = [(path, T) for path in T_SWEEP for T in TC.HORIZONS] + [("lat-self", LAT_MAX_T)]


@pytest.mark.parametrize("path,T", T_PARAMS, ids=[f"{p}-T{T}" for p, T in T_PARAMS])
def test_one_hot_weight_at_every_horizon(path, T):
    """Column blocks of the merge: 2T = 2, 64 / 66, 128 / 130 (c0 = 128 of the latency kernel), 320 / 322 (jj += NT; no granules)."""
    _sweep(path, T_SWEEP[path], T=T)


LAM_PARAMS = [(path, 65 if path in ("ticket",) else (1025 if path == "plain" else 2)) for path in PATHS]


@pytest.mark.parametrize("path,rows", LAM_PARAMS, ids=[p for p, _ in LAM_PARAMS])
def test_one_hot_weight_with_a_lambda_without_exact_reciprocal(path, rows):
    _sweep(path, rows, lam=TC.LAMBDAS[1])


REF_PARAMS = [(path, rows) for path, rr in REF_PATHS.items() for rows in rr]


@pytest.mark.parametrize("path,rows", REF_PARAMS, ids=[f"{p}-{r}" for p, r in REF_PARAMS])
def test_one_hot_weight_in_reference_order(path, rows):
    _sweep(path, rows, ref=True)


BATCH_PARAMS = [("lat-self", 3, 2), ("lat-self", 3, 17), ("lat-aux", 3, 16), ("role", 3, 2), ("role", 9, 33), ("two-launch", 3, 65),
                ("two-launch", 9, 2), ("ticket", 3, 65), ("ticket", 9, 81)]


@pytest.mark.parametrize("path,B,rows", BATCH_PARAMS, ids=[f"{p}-B{B}-{r}" for p, B, r in BATCH_PARAMS])
def test_batched_instances_keep_their_own_rows(path, B, rows):
    """Another k* and another goal per instance: a row read from the neighbouring instance's partials shows."""
    spec = PATHS[path]
    for K in TC.sizes(rows):
        case = TC.batch(B, K, TC.BASE_T)
        with _planner(case, B, **spec["kw"]) as pl:
            outs = run_case(pl, case, spec["mode"], t2k=K % 2 == 1)
            for b, got in enumerate(outs):
                TC.conditions(case, b, TC.reference(case, b))
                _note(path + "-batch", check_tail(got, case, b))
            assert pl.recovery_count() == 0
    _report(path + "-batch", f"B {B} rows {rows}")


def _paths_for_rows(rows):
    return [p for p, s in PATHS.items() if rows in s["rows"]]


LADDER_PARAMS = [(K, s, path) for K, s in TC.LADDER for path in _paths_for_rows(-(-K // 64))]


@pytest.mark.parametrize("K,spread,path", LADDER_PARAMS, ids=[f"K{K}-s{s:g}-{p}" for K, s, p in LADDER_PARAMS])
def test_ladder_of_weights_against_the_float64_spec(K, spread, path):
    """No weight underflows, every row carries some: the float64 spec decides, the spread-dependent part of the bound is in use."""
    case = TC.ladder(K, spread)
    TC.conditions(case, 0, TC.reference(case))
    spec = PATHS[path]
    with _planner(case, 1, **spec["kw"]) as pl:
        for t2k in (False, True) if spec["mode"] != "solve" else (False,):
            _note(path + "-ladder", check_tail(run_case(pl, case, spec["mode"], t2k)[0], case))
        assert pl.recovery_count() == 0
    if path in REF_PATHS:
        with _planner(case, 1, **dict(spec["kw"], reference_order=True)) as pl:
            _note(path + "-ladder", check_tail(run_case(pl, case, spec["mode"])[0], case, ref=True))
    _report(path + "-ladder", f"K {K} spread {spread:g}")


@pytest.mark.parametrize("seed", TC.random_seeds())
def test_random_configurations_against_the_float64_spec(seed):
    """test_gpu_fuzz's configurations with G <= 64, held to the derived bound instead of the fixed numbers."""
    case = TC.random(seed)
    for name, kw in (("auto", dict(lds_window=case["window"], pipeline=case["pipeline"], stream=0)), ("role", dict(kernel="role", stream=0)),
                     ("two-launch", dict(pipeline=False, lds_window=not case["window"], stream=0))):
        with _planner(case, 1, **kw) as pl:
            _note("random-" + name, check_tail(run_case(pl, case, "async", t2k=bool(seed & 1))[0], case))
        _report("random-" + name, f"seed {seed}")


@pytest.mark.parametrize("paced", (False, True), ids=("one-launch", "host-paced"))
@pytest.mark.parametrize("rows", (1, 2, 16, 17))
def test_first_action_of_a_forward_is_the_one_hot_control(rows, paced):
    """forward_state_async + first_action on the latency kernel: the first control reaches the host's mailbox before the tail has
    merged anything else -- with granules and a host-paced handle through wave 0's light poll and merge_one, otherwise from the
    merged columns.  Either way it is U[k*][0] bit for bit, and the forward's tail is held like any other."""
    import torch
    for K in TC.sizes(rows):
        for n, ks in enumerate(TC.kstars(K)):
            case = TC.one_hot(K, TC.BASE_T, ks)
            i = case["inst"][0]
            with _planner(case, 1, kernel="lat", stream=0, host_paced=paced) as pl:
                _load(pl, case)
                ed, kind = _device_eps(i["eps"], bool(n & 1))
                torch.cuda.synchronize()
                pl.forward_state_async(i["state"], ed.data_ptr(), kind)
                first = pl.first_action().copy()
                pl.sync()
                got = _outputs(pl, 1, case["T"])[0]
                assert pl.recovery_count() == 0
            assert np.array_equal(first, TC.reference(case)["U"][ks][0]), (K, ks, paced, first)
            _note("lat-forward", check_tail(got, case))
    _report("lat-forward", f"rows {rows} host-paced {paced}")


# ---- sampled slip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", (2, 33, 65))
@pytest.mark.parametrize("window", (True, False), ids=("fused", "global"))
def test_sampled_slip_tail(rows, window):
    """The sampled-slip kernels' ticket merge and tail: w and U* as everywhere, the one-hot U* equality; X* draws its own slip and is
    left to tests/test_gpu_sampled_slip.py.  Free cells: slip mean 0, std 0.02 (the traversability stays above 0.9); the wall: mean 1, std 0."""
    import torch
    from oracle import oracle as O
    path = "sampled-" + ("fused" if window else "global")
    for K in TC.sizes(rows):
        for n, ks in enumerate(TC.kstars(K)):
            case = TC.one_hot(K, TC.BASE_T, ks)
            i, T = case["inst"][0], case["T"]
            rng = np.random.default_rng(K + ks)
            SG = np.where(i["R"] > 0, 0.0, 0.02).astype(np.float32)
            zt, zc, zo = (rng.standard_normal(s).astype(np.float32) for s in ((K, T), (K, T + 1), (T,)))
            orc = O.solve_sampled(TC.oracle_params(case), i["R"], SG, i["state"], i["mean"], i["eps"], zt, zc, zo)
            TC.conditions(case, 0, dict(orc, Xstar=orc["X"][ks]))            # (X* has its own draws: not part of the condition)
            with _planner(case, 1, sampled_slip=True, lds_window=window, stream=0) as pl:
                pl.set_map(i["R"]); pl.set_slip_std(SG); pl.set_goal(i["goal"]); pl.set_mean(i["mean"])
                keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (zt.T, zc.T, zo, i["state"])]
                ed, kind = _device_eps(i["eps"], bool(n & 1))
                torch.cuda.synchronize()
                pl.set_slip_noise(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr())
                pl.solve_async_device(keep[3].data_ptr(), ed.data_ptr(), kind)
                pl.sync()
                got = _outputs(pl, 1, T)[0]
                assert pl.recovery_count() == 0
            _note(path, check_tail(got, case, orc=orc, xstar=False))
    _report(path, f"rows {rows}")


# ---- K-shard: the three-call protocol ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kstar", (4096, 4159, 2112))
def test_k_shard_three_call_protocol(kstar):
    """65 rows over two handles (33 + 32 rows), k* in the second shard: the stand-alone tail of each handle merges the gathered rows."""
    import torch
    from benchnav_amd.mppi import _DevArray
    from benchnav_amd.sharding import shard_rollouts
    K, T = 4160, TC.BASE_T
    case = TC.one_hot(K, T, kstar)
    i = case["inst"][0]
    orc = TC.reference(case)
    TC.conditions(case, 0, orc)
    std = torch.from_numpy(i["state"]).cuda()
    planners, parts, keep = [], [], []
    for r in range(2):
        first, count = shard_rollouts(K, 2, r)
        pl = _planner(dict(case, K=count), 1, stream=0)
        pl.set_map(i["R"]); pl.set_goal(i["goal"]); pl.set_mean(i["mean"]); pl.set_rollout_offset(first)
        ed, kind = _device_eps(i["eps"][first:first + count], bool(r))
        keep.append(ed)
        torch.cuda.synchronize()
        pl.shard_rollout_async_device(std.data_ptr(), ed.data_ptr(), kind)
        ptr, n, ps = pl.shard_partials()
        assert n == count // 64 and ps == 2 + 2 * T
        parts.append(torch.as_tensor(_DevArray(ptr, (n, ps)), device="cuda"))
        planners.append((pl, first, count))
    assert planners[1][1] <= kstar
    gathered = torch.cat(parts).contiguous()
    outs = []
    for pl, first, count in planners:
        pl.shard_finish_async(gathered.data_ptr(), gathered.shape[0])
        pl.sync()
        outs.append(_outputs(pl, 1, T)[0])
        pl.close()
    whole = {k: np.concatenate([o[k] for o in outs]) for k in ("U", "X", "cost", "w")}
    for o in outs:                                            # every rank holds the same U* and X*
        _note("k-shard", check_tail(dict(whole, Ustar=o["Ustar"], Xstar=o["Xstar"]), case))
    _report("k-shard", f"k* {kstar}")


# ---- the prologue merge -------------------------------------------------------------------------------------------------------------------
CHAIN_PARAMS = [(path, rows) for path in ("lat-aux", "role", "wave") for rows in (1, 16, 17, 24, 25, 64) if path != "wave" or rows <= 32]


@pytest.mark.parametrize("path,rows", CHAIN_PARAMS, ids=[f"{p}-{r}" for p, r in CHAIN_PARAMS])
def test_prologue_merge_recomputes_the_one_hot_mean(path, rows):
    """A chain of two solves from the one-hot case: every rollout workgroup of solve 2 merges solve 1's partial rows itself (merge_one,
    the granule poll, the eight-at-a-time loads) and samples around the result.  Solve 2 has zero noise, so every one of its control
    rows must be U[k*] of solve 1 bit for bit (it is inside the action bounds: the clamp changes nothing), its trajectories and costs
    the oracle's for that mean, and its own tail is held like any other."""
    import torch
    spec = PATHS[path]
    for K in TC.sizes(rows):
        for n, ks in enumerate(sorted({0, min(64, K - 1), K - 1})):
            first = TC.one_hot(K, TC.BASE_T, ks)
            i, T = first["inst"][0], first["T"]
            u1 = TC.reference(first)["U"][ks]
            second = dict(first, name=first["name"] + "_second", kind="uniform", inst=[dict(i, mean=u1, eps=np.zeros_like(i["eps"]), kstar=None)])
            second.pop("_oracle", None)
            eps = np.stack([i["eps"], second["inst"][0]["eps"]])[:, None]        # (2, B = 1, K, T, 2)
            with _planner(first, 1, **spec["kw"]) as pl:
                _load(pl, first)
                std = torch.from_numpy(i["state"]).cuda()
                ed, kind = _device_eps(eps, bool(n & 1))
                torch.cuda.synchronize()
                pl.solve_n_async_device(2, std.data_ptr(), ed.data_ptr(), kind, 2, eps[0].size)
                pl.sync()
                got = _outputs(pl, 1, T)[0]
                assert pl.recovery_count() == 0
            assert np.array_equal(got["U"], np.broadcast_to(u1, got["U"].shape)), (path, K, ks, "solve 2 did not sample around U[k*] of solve 1")
            _note(path + "-chain", check_tail(got, second))
    _report(path + "-chain", f"rows {rows}")


# ---- nothing of the lists was left out ------------------------------------------------------------------------------------------------------
def test_the_sweep_visits_every_listed_row_count_kstar_and_horizon():
    """The parameters above, put together, are the issue's lists -- and what ran in this session checked every solve it planned."""
    planned = set()
    for path, rows in ROW_PARAMS:
        planned |= _planned(path, rows)
    assert {e[1] for e in planned} == set(TC.ROWS)
    assert {e[1] for e in planned if e[0] == "two-launch"} == set(TC.ROWS)
    assert {e[1] for e in planned if e[0] == "ticket"} == {65, 80, 81, 1009, 1024} and {e[1] for e in planned if e[0] == "plain"} == {1025}
    assert {e[1] for e in planned if e[0] == "wave"} == {r for r in TC.ROWS if r <= 32}
    assert {e[1] for e in planned if e[0] in ("lat-self", "role")} == {r for r in TC.ROWS if r <= 64}
    for path, rows in ROW_PARAMS:                               # every k* of the list, cut to the range of K, for both K of every row count
        for K in TC.sizes(rows):
            want = {k for k in (0, 15, 16, 63, 64, K - 65, K - 64, K - 1) if 0 <= k < K}
            assert {e[3] for e in planned if e[:3] == (path, rows, K)} == want, (path, rows, K)
    assert {(p, T) for p, T in T_PARAMS} == {(p, T) for p in T_SWEEP for T in (1, 32, 33, 64, 65, 160, 161)} | {("lat-self", LAT_MAX_T)}
    for path, T in T_PARAMS:
        planned |= _planned(path, T_SWEEP[path], T=T)
    for path, rows in LAM_PARAMS:
        planned |= _planned(path, rows, lam=TC.LAMBDAS[1])
    for path, rows in REF_PARAMS:
        planned |= _planned(path, rows, ref=True)
    assert all(T <= 8 for (_, rows, _, _, T, _, _) in planned if rows >= TC.ROWS_SHORT_T)
    ran = {(e[0], e[1], e[4], e[5], e[6]) for e in VISITED}
    for e in planned:
        if (e[0], e[1], e[4], e[5], e[6]) in ran:
            assert e in VISITED, (e, "was planned and not checked")
    assert VISITED <= planned
    for path in sorted(RATIOS):
        _report(path, "total")
