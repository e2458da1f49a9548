"""GPU: the host side of the C ABI is one file per concern behind csrc/mppi_handle.h, and each concern frees what it allocates
(paced_release, env_release, loops_release, shard_comm_release, called by bn_mppi_destroy).

1. Handles that use EVERY concern -- host-paced forward, closed-loop episode, DWA, the A* + DWA loop, the CL-RRT loop, the local
   half of the K-shard exchange -- leave the device's free memory where it was.
2. The four DWA entry points share one scratch layout (DwaScratch, mppi_env.cpp): the views bn_mppi_dwa_buffers and
   bn_mppi_dwa_candidates hand out point at what bn_mppi_dwa_solve wrote.
3. The three closed loops share one log layout (EpisodeLog, csrc/episode_log.h), laid out by the rows the log holds: the copies
   and the device views of a call shorter than the log agree with a fresh handle's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K, T, G, RES, THR = 128, 10, 64, 0.5, 0.2      # the smallest planner that takes every path: two workgroups per instance, latency kernel
B = 1                                          # BN_FLAG_HOST_PACED paces one instance per handle
N_EP, N_AD, N_CL = 16, 64, 64                  # closed-loop steps / A* + DWA steps / CL-RRT loop iterations of a cycle
WARM, CYCLES = 2, 8
# Free-memory drift of the 8 measured cycles on the commit before the split, where nothing leaks (profiles/capi_split_gputest.txt).
PARENT_DRIFT_BYTES = 0


def _release_bytes(bar: bool):
    """Device bytes each concern's release function frees for one cycle's handle, from the shapes (csrc/mppi_{env,loops,paced,shard}.cpp)."""
    kslots, nblk = 4, (K + 63) // 64
    env = 2 * G * G * 4 + B * 12 + B * 4 + (N_EP + 1) * B * 12 + N_EP * B * 4 + N_EP * B * 8      # latent mean, std | state | done | episode log
    loops = ((4 * B + 1) * 4 + B * 12 + ((N_AD + 1) * 3 + N_AD * 5) * B * 4                        # A* + DWA: words, state, log
             + B * 32 + (B + 1) * 4 + B * 12 + ((N_CL + 1) * 3 + N_CL * 6) * B * 4)                # CL-RRT: rovers, flags, goals, log
    paced = kslots * 8 * 8 + (-(-(kslots * 8 + 16) * 8 // 4096) * 4096 if bar else 0)            # republished requests | the request words behind the BAR (whole pages)
    shard = 1 * nblk * (2 + 2 * T) * 4 + (kslots * (2 * T + 2) + 64 * (2 + 2 * T) + 4) * 4         # gathered rows (world 1) | merged rows, group rows, ticket
    return dict(env_release=env, loops_release=loops, paced_release=paced, shard_comm_release=shard)


class _Rig:
    """What outlives the cycles: the inputs, the A* handle (one solve) and the CL-RRT handle the loops of every cycle's planner read."""

    def __init__(self):
        from benchnav_amd import CLRRT, _capi
        from benchnav_amd.clrrt import _Handle
        from helpers import FakeDynamics, FakeGridMap, FakeObjectives
        fx = np.load(os.path.join(HERE, "golden", "clrrt_loop.npz"))
        self._capi, self.lib = _capi, _capi.load()
        self.dev = torch.device("cuda", 0)
        self.risk = np.clip(fx["mean"], 0.0, 0.7).astype(np.float32)
        self.std = np.full((G, G), float(fx["std"]), np.float32)
        self.dt, self.time_limit, self.goal_thr = float(fx["delta_t"]), float(fx["time_limit"]), float(fx["goal_threshold"])
        start, self.goal = fx["start"].astype(np.float32), fx["goal"].astype(np.float32)
        d = self.goal - start
        self.state0 = np.array([[start[0], start[1], np.arctan2(d[1], d[0])]], np.float32)
        self.goal_nodes = np.ascontiguousarray(np.concatenate([self.goal, self.state0[0, 2:]])[None], np.float32)
        self.seeds = np.array([42], np.uint64)
        self.actions = np.stack(np.meshgrid(np.linspace(0.2, 1.0, 3, dtype=np.float32), np.array([-0.5, 0.5], np.float32), indexing="ij"), -1).reshape(6, 2)
        self.state_dev = torch.from_numpy(self.state0).to(self.dev)
        self.prev_dev = torch.zeros(B, 2, device=self.dev)
        # A*: one goal-rooted solve on the risk map (flat heights), goal = the environment's
        self.astar = C.c_void_p()
        self._check_astar(self.lib.bn_astar_create(0, G, G, B, C.byref(self.astar)))
        heights = np.zeros((G, G), np.float32)
        self._check_astar(self.lib.bn_astar_set_map(self.astar, 0, C.c_void_p(heights.ctypes.data), C.c_void_p(self.risk.ctypes.data), _capi.BN_MEM_HOST, THR, RES))
        self._check_astar(self.lib.bn_astar_set_goal(self.astar, 0, int(self.goal[0] / RES), int(self.goal[1] / RES)))
        self._check_astar(self.lib.bn_astar_solve_async(self.astar, None))
        # CL-RRT: the loop's planner handle, on the same grid
        gm = FakeGridMap(G, RES)
        iters, max_seqs, seed, _ = (int(v) for v in fx["params"])
        self.planner = CLRRT(3, 2, FakeDynamics(self.risk, gm), FakeObjectives(torch.as_tensor(self.goal.copy()), THR), gm, delta_t=self.dt,
                             max_iterations=iters, max_seqs=max_seqs, seed=seed)
        self.clrrt = _Handle(self.lib, self.dev, B, self.planner)
        torch.cuda.synchronize()

    def _check_astar(self, code):
        assert code >= 0, self.lib.bn_astar_last_error().decode("utf-8", "replace")

    def close(self):
        self.clrrt.close()
        self.lib.bn_astar_destroy(self.astar)

    def cycle(self):
        """One handle through every concern, then bn_mppi_destroy.  Returns whether the request words sit behind the BAR."""
        from benchnav_amd import NativeMPPI
        lib, check = self.lib, self._capi.check
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        with NativeMPPI(horizon=T, num_samples=K, grid_size=G, resolution=RES, num_instances=B, stuck_threshold=THR, stream=0, host_paced=True) as pl:
            h = pl._h
            assert pl.host_paced(), "the handle does not pace: paced_release would have nothing to free"
            bar = int(lib.bn_mppi_host_paced(h)) == 2
            pl.set_map(self.risk)
            pl.set_goal(self.goal)
            pl.env_attach(self.risk, self.std, goal_threshold=self.goal_thr, delta_t=self.dt, seed=1)
            states, rewards, done = pl.episode(N_EP, self.state0)                               # env_release: the episode log
            assert states.shape == (N_EP + 1, B, 3) and np.isfinite(states).all()
            out = pl.dwa_solve(self.state0, self.actions)
            assert np.isfinite(out["costs"]).all()
            # the A* + DWA loop (loops_release: words, state, log)
            check(lib.bn_astar_dwa_reset(h))
            self.prev_dev.zero_()
            check(lib.bn_astar_dwa_episode_async(h, self.astar, N_AD, C.c_void_p(self.state_dev.data_ptr()), self._capi.BN_MEM_DEVICE,
                                                 C.c_void_p(self.prev_dev.data_ptr()), (C.c_float * 2)(0.5, 0.5), self.dt, 3, 3, 1.0, None))
            ad_states, ad_status = np.empty((N_AD + 1, B, 3), np.float32), np.empty(B, np.int32)
            check(lib.bn_astar_dwa_episode_log(h, ptr(ad_states), None, None, None, None, ptr(ad_status), None))
            assert int(ad_status[0]) == self._capi.BN_AD_OK and np.isfinite(ad_states).all()
            # the CL-RRT loop (loops_release: rovers, flags, goals, log, the pinned counter, two events)
            check(lib.bn_clrrt_loop_reset(h, self.clrrt.h, self.goal_nodes.ctypes.data, self.seeds.ctypes.data, self.dt, self.time_limit))
            st = self.state_dev.clone()
            check(lib.bn_clrrt_loop_run(h, self.clrrt.h, N_CL, C.c_void_p(st.data_ptr()), None, None, 0, 0, None))
            cl_steps = np.empty(B, np.int32)
            check(lib.bn_clrrt_loop_log(h, *([None] * 9), ptr(cl_steps)))
            assert int(cl_steps[0]) > 0
            # the host-paced forward (paced_release: request words, events), then the local half of the K-shard exchange
            pl.forward_state_async(self.state0)
            assert np.isfinite(pl.first_action()).all()
            pl.shard_comm_prepare(1, 0)                                                           # world 1: no communicator is built
        return bar


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    r.close()


def _fill_open_blocks():
    """hipMemGetInfo counts whole 2 MiB blocks: the runtime carves allocations below that size out of such blocks in 4 KiB granules
    (measured, profiles/capi_split_gputest.txt: 8 x 64 KiB leave free memory unchanged, 8 x 256 KiB take exactly 2 MiB), so eight
    leaked request-word buffers would vanish in the room of a block that is already there.  Take that room away: 4 KiB allocations
    until free memory drops (a new block had to be opened); that last one is returned, the others are kept for the caller to free.
    From here on a cycle's buffers live in blocks of their own, and a block holding ONE leaked buffer cannot go back: 2 MiB short."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    kept, free = [], torch.cuda.mem_get_info()[0]
    for _ in range(16384):                              # 64 MiB at the most
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), 4096) == 0
        if torch.cuda.mem_get_info()[0] < free:
            assert hip.hipFree(p) == 0
            break
        kept.append(p)
    return lambda: [hip.hipFree(p) for p in kept]


def test_handles_that_use_every_concern_leave_free_memory_where_it_was(rig):
    """Measured on an MI355X (profiles/capi_split_gputest.txt): drop 0 B before and after the split, three runs each.  On scratch
    builds with ONE release line removed -- d_ep_done from env_release, d_cl_flags from loops_release, d_req_dev from paced_release,
    d_gathered from shard_comm_release -- the drop reads 2097152 B and the test fails, for each of the four."""
    for _ in range(WARM):
        bar = rig.cycle()
    torch.cuda.synchronize()
    release_fillers = _fill_open_blocks()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(CYCLES):
        rig.cycle()
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info()[0]
    release_fillers()
    release = _release_bytes(bar)
    bound = max(4 * PARENT_DRIFT_BYTES, CYCLES * min(release.values()) // 2)
    print(f"free-memory drop over {CYCLES} cycles: {drop} B; per-cycle release by concern {release}; bound {bound} B")
    assert CYCLES * min(release.values()) // 2 >= 4 * PARENT_DRIFT_BYTES       # a leak of any ONE concern's buffers is above the bound
    assert drop < bound, (drop, bound, release)


def test_dwa_views_point_at_what_dwa_solve_wrote():
    from benchnav_amd import NativeMPPI, _capi, synth
    from benchnav_amd.astar import _DevArray
    NB, NA = 2, 6
    inst = synth.make_instance(G, seed=0, resolution=RES)
    states = np.stack([inst.start.numpy(), inst.start.numpy() + np.array([0.5, -0.25, 0.1], np.float32)]).astype(np.float32)
    rng = np.random.default_rng(5)
    actions = np.stack([rng.uniform(0.0, 1.0, (NB, NA)), rng.uniform(-1.0, 1.0, (NB, NA))], -1).astype(np.float32)
    stage_goal = (inst.goal.numpy()[None] + np.array([[0.0, 0.0], [-1.5, 2.0]], np.float32)).astype(np.float32)
    with NativeMPPI(horizon=T, num_samples=K, grid_size=G, resolution=RES, num_instances=NB, shared_map=True, stream=0) as pl:
        pl.set_map(inst.risk.numpy())
        pl.set_goal(inst.goal.numpy())
        out = pl.dwa_solve(states, actions, stage_goal)
        x, c, w = pl.dwa_buffers(NA)
        a, g = C.c_void_p(), C.c_void_p()
        _capi.check(pl._lib.bn_mppi_dwa_candidates(pl._h, NA, C.byref(a), C.byref(g)))
        view = lambda p, shape: torch.as_tensor(_DevArray(p, shape), device="cuda").cpu().numpy().copy()
        assert np.array_equal(view(x, (NB, NA, T + 1, 3)), out["states"])
        assert np.array_equal(view(c, (NB, NA)), out["costs"])
        assert np.array_equal(view(w, (NB, NA)), out["weights"])
        assert np.array_equal(view(a.value, (NB, NA, 2)), actions)
        assert np.array_equal(view(g.value, (NB, 2)), stage_goal)
        assert np.isfinite(out["costs"]).all() and len(np.unique(out["costs"])) > NB     # distinct rollouts: a shifted view would not match
        with pytest.raises(_capi.BenchnavError, match="no bn_mppi_dwa_solve with this num_actions has run"):
            pl.dwa_buffers(NA + 1)


N_LONG, N_SHORT, NB = 7, 3, 2                  # a call that sizes the logs, then a shorter one on the same handle; two rovers


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _short_calls(fx, z, eps, long_first):
    """The N_SHORT-row call of each closed loop on one planner handle -- behind an N_LONG-row call of the same loop from the same
    start when `long_first` -- as its copies, its device views and (rows of the call, rows the log holds)."""
    from benchnav_amd import CLRRT, AStarDWALoop, CLRRTLoop, NativeMPPI, _capi
    from benchnav_amd.astar import _DevArray
    from benchnav_amd.env import BatchedPlanetaryEnv
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    risk = np.clip(fx["mean"], 0.0, 0.7).astype(np.float32)
    dt = float(fx["delta_t"])
    pl = NativeMPPI(horizon=T, num_samples=K, grid_size=G, resolution=RES, num_instances=NB, stuck_threshold=THR, stream=0)
    env = BatchedPlanetaryEnv(pl, risk, np.full((G, G), float(fx["std"]), np.float32), fx["start"], fx["goal"], delta_t=dt,
                              time_limit=float(fx["time_limit"]), stuck_threshold=THR, goal_threshold=float(fx["goal_threshold"]), seed=1,
                              check_positions=False)                                      # the rovers differ by their slip draws
    ad = AStarDWALoop(env, np.zeros((G, G), np.float32), risk, THR, (0.5, 0.5), dt, 3, 3, 1.0)
    gm = FakeGridMap(G, RES)
    iters, max_seqs, seed, _ = (int(v) for v in fx["params"])
    cl = CLRRTLoop(env, CLRRT(3, 2, FakeDynamics(risk, gm), FakeObjectives(torch.as_tensor(fx["goal"].copy()), THR), gm, delta_t=dt,
                              max_iterations=iters, max_seqs=max_seqs, seed=seed))
    view = lambda p, shape, t="<f4": torch.as_tensor(_DevArray(p, shape, t), device="cuda").cpu().numpy().copy()
    calls = (N_LONG, N_SHORT) if long_first else (N_SHORT,)
    state0 = env.reset().cpu().numpy()
    out = {}
    for n in calls:                             # injected noise and a zero warm start: a call depends on nothing before it
        pl.set_mean(None)
        s, r, d = pl.episode(n, state0, z_device_ptr=z.data_ptr(), eps_ptr=eps.data_ptr(), kind=_capi.BN_NOISE_DEVICE_KT2,
                             eps_ring=N_SHORT, eps_stride=eps[0].numel())
    out["mppi"] = dict(states=s, rewards=r, actions=pl.last_actions, done_step=d)
    ps, pr, pd, n, cap = pl.episode_buffers()
    out["mppi_views"] = dict(states=view(ps, (n + 1, NB, 3)), rewards=view(pr, (n, NB)), done_step=view(pd, (NB,), "<i4"))
    out["mppi_rows"] = (n, cap)
    for n in calls:
        env.reset()
        log = ad.run(n, z=z[:n])
    out["astar_dwa"] = dict(zip(("states", "rewards", "actions", "sub_goals", "done_step", "status"), log))
    ps, pr, pd, pst, n, cap = ad.episode_buffers()
    out["astar_dwa_views"] = dict(states=view(ps, (n + 1, NB, 3)), rewards=view(pr, (n, NB)), done_step=view(pd, (NB,), "<i4"),
                                  status=view(pst, (NB,), "<i4"))
    out["astar_dwa_rows"] = (n, cap)
    for n in calls:
        env.reset()
        out["clrrt"] = cl.run(n, z=z[:n])
    cl.close()
    return out


def test_episode_views_and_copies_agree_when_the_log_holds_more_rows_than_the_call_ran():
    """A reader of a log that takes the call's rows for the log's rows (or the other way round) reads the wrong rows as soon as
    the two differ: N_LONG rows, then N_SHORT on the same handle.  Every comparison is bit for bit."""
    fx = np.load(os.path.join(HERE, "golden", "clrrt_loop.npz"))
    rng = np.random.default_rng(11)
    z = torch.from_numpy(rng.standard_normal((N_LONG, NB)).astype(np.float32)).cuda()
    eps = torch.from_numpy(rng.standard_normal((N_SHORT, NB, K, T, 2)).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    reused, fresh = _short_calls(fx, z, eps, True), _short_calls(fx, z, eps, False)
    assert reused["mppi_rows"] == reused["astar_dwa_rows"] == (N_SHORT, N_LONG)
    assert fresh["mppi_rows"] == fresh["astar_dwa_rows"] == (N_SHORT, N_SHORT)
    for loop in ("mppi", "astar_dwa", "clrrt"):
        assert reused[loop].keys() == fresh[loop].keys() and len(reused["clrrt"]) == 10
        for k in fresh[loop]:
            assert np.array_equal(_bits(reused[loop][k]), _bits(fresh[loop][k])), (loop, k)
    for got in (reused, fresh):
        for loop in ("mppi", "astar_dwa"):
            for k, v in got[loop + "_views"].items():
                assert v.shape == got[loop][k].shape and np.array_equal(_bits(v), _bits(got[loop][k])), (loop, k)
    # the runs say something: the rovers move, the two differ, and the sub-goals are points of the path, not the goal (a shifted
    # column would not match)
    for loop in ("mppi", "astar_dwa", "clrrt"):
        s = fresh[loop]["states"]
        assert np.isfinite(s).all() and not np.array_equal(s[1:, 0], s[1:, 1]) and not np.array_equal(s[0], s[-1]), loop
    assert (fresh["astar_dwa"]["status"] == 0).all() and np.isfinite(fresh["astar_dwa"]["rewards"]).all()        # BN_AD_OK
    assert (fresh["astar_dwa"]["sub_goals"] != fx["goal"].astype(np.float32)).any(axis=-1).all()
    assert (fresh["clrrt"]["plans"] >= 1).all() and (fresh["clrrt"]["steps"] >= 1).all()
