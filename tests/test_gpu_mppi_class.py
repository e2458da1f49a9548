"""GPU: the torch-facing drop-in class (benchnav_amd.MPPI) used the way the reference's drivers use
theirs (test/test_mppi.py:160-198): construct from dynamics/objectives objects, call forward(state),
read get_top_samples."""
import numpy as np
import pytest
import torch

from helpers import TOL_REF, assert_within, load_case, mppi_for_fixture, parity_metrics

pytestmark = pytest.mark.gpu


def _collect(solver, U, X):
    return dict(U=solver._perturbed_action_seqs.cpu().numpy(), X=solver._state_seq_batch.cpu().numpy(),
                cost=solver._costs.cpu().numpy(), w=solver._weights.cpu().numpy(),
                Ustar=U.cpu().numpy(), Xstar=X[0].cpu().numpy())


def test_forward_reproduces_the_reference_run_with_the_reference_noise_stream():
    fx = load_case("c1_basic")
    same_stream = (str(fx["cpu_capability"]) == torch.backends.cpu.get_cpu_capability()
                   and str(fx["torch_version"]) == torch.__version__)
    solver = mppi_for_fixture(fx, noise="torch")
    for i in range(int(fx["n_solves"])):
        state = torch.tensor(fx[f"state_{i}"])
        keep = state.clone()
        solver._previous_action_seq = torch.from_numpy(fx[f"mean_{i}"])      # teacher forcing
        with torch.no_grad():
            if same_stream:
                U, X = solver.forward(state=state)                           # draws eps like mppi.py:149-151
                assert np.array_equal((solver._action_noises.cpu() / torch.tensor(fx["sigmas"])).numpy(), fx[f"eps_{i}"])
            else:
                U, X = solver.solve_with_noise(state, torch.from_numpy(fx[f"eps_{i}"]))
        assert torch.equal(state, keep), "forward must not mutate the caller's state"
        assert U.shape == (int(fx["T"]), 2) and X.shape == (1, int(fx["T"]) + 1, 3) and U.is_cuda
        assert_within(parity_metrics(_collect(solver, U, X), fx, i), TOL_REF, ctx=f"solve {i}")
        assert torch.equal(solver._previous_action_seq, U)                   # mppi.py:217


def test_callable_interfaces_and_top_samples():
    fx = load_case("cvar")
    solver = mppi_for_fixture(fx, noise="torch")
    state = torch.tensor(fx["state_0"], device="cuda")
    with torch.no_grad():
        U1, X1 = solver(state)                       # nn.Module call
        U2, X2 = solver.solve(state)                 # alias
    assert U1.shape == U2.shape
    n = 17
    top_s, top_w = solver.get_top_samples(num_samples=n)
    assert top_s.shape == (n, int(fx["T"]) + 1, 3) and top_w.shape == (n,)
    assert torch.all(top_w[:-1] >= top_w[1:])
    w = solver._weights
    assert torch.equal(top_w, torch.sort(w, descending=True).values[:n])
    k0 = int(torch.argmax(w))
    assert torch.equal(top_s[0], solver._state_seq_batch[k0])
    assert top_s.cpu().numpy().shape == (n, int(fx["T"]) + 1, 3)   # planetary_env.py:366-369 does .cpu().numpy()
    with pytest.raises(AssertionError):
        solver.get_top_samples(int(fx["K"]) + 1)
    with pytest.raises(AssertionError):
        solver.forward(torch.zeros(4))


def test_state_batch_view_matches_the_c_abi_copy_and_noise_modes_run():
    fx = load_case("c1_stuck")
    for mode in ("philox", "torch_device"):
        solver = mppi_for_fixture(fx, noise=mode, copy_outputs=False)
        U, X = solver(torch.tensor(fx["state_0"]))
        torch.cuda.synchronize()
        assert solver._state_seq_batch.shape == (int(fx["K"]), int(fx["T"]) + 1, 3)
        assert abs(float(solver._weights.sum()) - 1.0) < 1e-4
        assert torch.isfinite(U).all() and torch.isfinite(X).all()
        # X*[0,0] is the un-clamped state after the first step, not the input (aliasing)
        assert not torch.allclose(X[0, 0].cpu(), torch.tensor(fx["state_0"]))


def test_observation_mode_dynamics_are_rejected_like_the_reference():
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    from benchnav_amd import MPPI
    gm = FakeGridMap(16, 0.5)
    dyn = FakeDynamics(np.zeros((16, 16), np.float32), gm, mode="observation")
    with pytest.raises(TypeError):
        MPPI(5, 64, 3, 2, dyn, FakeObjectives(torch.tensor([4, 4]), 0.3), torch.tensor([0.5, 0.5]), 0.5)


def test_sampled_slip_opt_in_plans_with_observation_mode_dynamics():
    """BASELINE config 3 through the drop-in class: observation-mode dynamics + sampled_slip=True read the latent
    Normal(mean, std) of the grid map; the solve equals NativeMPPI's sampled-slip solve with the same seed."""
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    from benchnav_amd import MPPI, NativeMPPI, synth
    G, K, T = 64, 256, 15
    mu = (synth.smooth_risk_map(G, 5) * 0.6).numpy(); sg = synth.slip_std_map(G, 5).numpy()
    gm = FakeGridMap(G, 0.5, latent=(mu, sg))
    dyn = FakeDynamics(np.zeros((G, G), np.float32), gm, mode="observation")
    obj = FakeObjectives(torch.tensor([24.0, 22.0]), 0.3)
    solver = MPPI(T, K, 3, 2, dyn, obj, torch.tensor([0.5, 0.5]), 0.5, seed=3, noise="philox", sampled_slip=True)
    state = torch.tensor([9.0, 8.0, 0.4])
    U, X = solver(state)
    torch.cuda.synchronize()
    assert U.shape == (T, 2) and X.shape == (1, T + 1, 3) and abs(float(solver._weights.sum()) - 1) < 1e-4
    with NativeMPPI(horizon=T, num_samples=K, grid_size=G, resolution=0.5, sampled_slip=True, seed=3, stream=0) as pl:
        pl.set_map(mu); pl.set_slip_std(sg); pl.set_goal([24.0, 22.0])
        us, xs = pl.solve(state.numpy())
    assert np.array_equal(U.cpu().numpy(), us[0]) and np.array_equal(X[0].cpu().numpy(), xs[0])
    with pytest.raises(TypeError):                       # inference-mode dynamics cannot be sampled
        MPPI(T, K, 3, 2, FakeDynamics(mu, gm), obj, torch.tensor([0.5, 0.5]), 0.5, sampled_slip=True)


def test_lean_class_serves_top_samples_and_state_batch_by_rerolling():
    """lean=True: no trajectory batch in HBM; get_top_samples re-rolls the winners, `_state_seq_batch` all K rows, both
    bit-identical to the full-API planner on the same (Philox) noise."""
    import torch
    from helpers import load_case, mppi_for_fixture
    fx = load_case("c2")
    state = torch.tensor(fx["state_0"], device="cuda")
    res = {}
    for lean in (False, True):
        solver = mppi_for_fixture(fx, noise="philox", store_controls=False, lean=lean)
        for _ in range(3):
            U, X = solver(state)
        top_s, top_w = solver.get_top_samples(64)
        res[lean] = (U.cpu().numpy(), X.cpu().numpy(), top_s.cpu().numpy(), top_w.cpu().numpy(), solver._state_seq_batch.cpu().numpy(),
                     solver._weights.cpu().numpy())
        if lean:
            assert solver._buf_X is None
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a, b)


def test_forward_under_a_different_current_stream_is_fenced():
    """the planner enqueues on its construction-time stream; a forward() issued under another current stream
    must still see the state written on that stream and hand back outputs ordered on it."""
    import torch
    from helpers import load_case, mppi_for_fixture
    fx = load_case("c1_basic")
    solver = mppi_for_fixture(fx, noise="philox")
    ref = mppi_for_fixture(fx, noise="philox")
    side = torch.cuda.Stream()
    base = torch.tensor(fx["state_0"], device="cuda")
    for i in range(5):
        with torch.cuda.stream(side):
            st = base + 0.01 * i                       # produced on the side stream right before the call
            U, X = solver(st)
            got = (U.clone(), X.clone())
        side.synchronize()
        U2, X2 = ref(base + 0.01 * i)
        torch.cuda.synchronize()
        assert torch.equal(got[0], U2) and torch.equal(got[1], X2), i


def test_first_action_is_the_first_row_of_the_optimal_action_sequence():
    """MPPI.first_action(): U*[0] from the tail's pinned host mailbox -- posted before X* and the weights exist -- equals
    optimal_action_seq[0] of every forward(), for the drop-in class and for several instances of the NumPy-level planner."""
    import torch
    from benchnav_amd import NativeMPPI, synth
    from helpers import load_case, mppi_for_fixture
    fx = load_case("c1_basic")
    solver = mppi_for_fixture(fx, noise="philox")
    state = torch.tensor(fx["state_0"], device="cuda")
    for _ in range(5):
        U, X = solver(state)
        a = solver.first_action().clone()
        assert a.device.type == "cpu" and a.shape == (2,) and torch.equal(a, U[0].cpu())
    B, G = 3, 64
    insts = [synth.make_instance(G, seed=s) for s in range(B)]
    with NativeMPPI(horizon=20, num_samples=256, grid_size=G, resolution=0.5, num_instances=B) as pl:
        for b, it in enumerate(insts):
            pl.set_map(it.risk.numpy(), b); pl.set_goal(it.goal.numpy(), b)
        st = torch.stack([it.start for it in insts]).cuda()
        for n in (1, 4, 20):                             # single solves, a short batch, an overlapped batch with its own tail
            pl.solve_n_async_device(n, st.data_ptr())
            firsts = [pl.first_action(b) for b in range(B)]
            pl.sync()
            for b in range(B):
                assert np.array_equal(firsts[b], pl.get_mean(b)[0]), (n, b)


# ---- the handle the classes own: K = 64, T = 4, G = 16, the smallest shapes the kernels accept ---------------------------------
def _small_problem():
    from helpers import FakeDynamics, FakeGridMap, FakeObjectives
    G = 16
    iy, ix = np.mgrid[0:G, 0:G]
    risk = (((ix * 7 + iy * 3) % 11) / 16.0).astype(np.float32)          # inline risk map, no two neighbours alike
    risk[6:9, 9:12] = 1.0
    gm = FakeGridMap(G, 0.5)
    return risk, FakeDynamics(risk, gm), FakeObjectives(torch.tensor([6.5, 6.0]), 0.3), torch.tensor([1.25, 1.5, 0.3])


def test_drop_in_class_and_numpy_level_planner_agree_bit_for_bit():
    """One config function behind both constructors: with sigma = (0.5, 0.5) the inverted covariance and float32 1/(s*s) are the
    same 4.0, so MPPI(noise="philox") and NativeMPPI with the same seed, on the same stream, solve identically, warm starts included."""
    from benchnav_amd import MPPI, NativeMPPI
    K, T, seed = 64, 4, 11
    risk, dyn, obj, state = _small_problem()
    with MPPI(T, K, 3, 2, dyn, obj, torch.tensor([0.5, 0.5]), 0.5, seed=seed, noise="philox") as solver, \
            NativeMPPI(horizon=T, num_samples=K, grid_size=16, resolution=0.5, seed=seed,
                       stream=torch.cuda.current_stream().cuda_stream) as pl:
        assert solver._inv_covariance.diagonal().tolist() == [4.0, 4.0]
        pl.set_map(risk); pl.set_goal([6.5, 6.0])
        for i in range(3):
            st = state + torch.tensor([0.05 * i, 0.04 * i, 0.01 * i])
            U, X = solver.forward(st)
            us, xs = pl.solve(st.numpy())
            assert np.array_equal(U.cpu().numpy(), us[0]) and np.array_equal(X[0].cpu().numpy(), xs[0]), i
        assert np.abs(us[0]).max() > 0 and not np.array_equal(xs[0][0], xs[0][-1])


def test_with_block_releases_the_handle_of_every_owner():
    from benchnav_amd import MPPI, NativeMPPI
    from benchnav_amd.dwa import DWA
    risk, dyn, obj, state = _small_problem()
    with MPPI(4, 64, 3, 2, dyn, obj, torch.tensor([0.5, 0.5]), 0.5, noise="philox") as p:
        U, _ = p.forward(state)
        assert torch.isfinite(U).all() and bool(p._handle)
    assert not p._handle
    with pytest.raises(RuntimeError, match="null handle"):               # a closed planner refuses, it does not touch freed memory
        p.forward(state)
    del p
    with DWA(4, 3, 2, dyn, obj, torch.tensor([0.5, 1.0]), 0.1) as d:
        u, x = d.forward(state.cuda())
        assert u.shape == (1, 2) and torch.isfinite(x).all() and bool(d._native._h)
    assert not d._native._h and not d._native._handle
    del d
    with NativeMPPI(horizon=4, num_samples=64, grid_size=16, resolution=0.5) as pl:
        pl.set_map(risk); pl.set_goal([6.5, 6.0])
        us, _ = pl.solve(state.numpy())
        assert np.isfinite(us).all() and bool(pl._h)
    assert not pl._h and not pl._handle
    pl.close()                                                           # once more: nothing left to destroy
    del pl
