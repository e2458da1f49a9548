"""Inputs that put the softmin weight where the merge and the tail of a solve change form (tests/test_mppi_tail_spec.py on the CPU,
tests/test_gpu_mppi_tail.py on the device).  Every case but the random ones uses a 16 x 16 map at 0.5 m and thr = 0.3, injected noise.

A case: dict(name, kind, K, T, G, res, xl, yl, thr, lam, sigma, inv_var, u_min, u_max, inst = [per instance: R, state, goal, mean,
eps (K,T,2), kstar]).  `conditions(case, b, orc)` asserts what the case promises about the CPU oracle's own result.

one_hot   R = 0 but R[:, 6:] = 1 (a wall from x = 3 m), state (2.75, 4, 0), goal (7, 4), mean v = 1: every rollout drives into the wall
          and collects 1e4 per step there; rollout k* (v noise -10: it stays where it is, omega noise a ramp) does not.  The gap over
          lambda is thousands: float32 AND float64 exp give 0, so w is exactly one-hot, U* == U[k*] and X* == X[k*] bit for bit in any
          correct order of operations.  (T < 8: the start moves to x = 2.95, one step from the wall -- from 2.75 a rollout of fewer than
          three steps never reaches it and the reference itself is not one-hot.)
ladder    no wall; rollout k drives k mod L steps towards the goal and stops (v noise -10 from there on; omega noise only while it
          stands, so the costs take exactly L values).  With j = T - (k mod L) steps NOT driven the distance terms cost 0.05 j (j + 3)
          and the control term lambda inv_var_v (T - j); lambda and inv_var_v are chosen so that z_j - max = -alpha (j - p)^2 with the peak
          p = (L - 1) / 4 + 0.4 between two levels (no two weights equal) and alpha (L - 1 - p)^2 = the wanted spread: 3, 20, 80.
random    test_gpu_fuzz._case seeds with G <= 64.
batch     B one-hot instances in one launch, each with another k* and another goal."""
import functools

import numpy as np

G, RES, THR = 16, 0.5, 0.3
ROWS = (1, 2, 16, 17, 24, 25, 32, 33, 64, 65, 80, 81, 1009, 1024, 1025)
ROWS_SHORT_T = 1009                 # from this many rows on the horizon stays at 8 or less
HORIZONS = (1, 32, 33, 64, 65, 160, 161)
BASE_T = 8
LAMBDAS = (0.5, 0.3)                # 0.3: no exact reciprocal, the division beside inv_lambda
KSTAR_OFFSETS = ("0", "15", "16", "63", "64", "K-65", "K-64", "K-1")
LADDER = ((4160, 3.0), (1088, 20.0), (128, 80.0))      # (K, largest |z - max|): 65, 17 and 2 rows (the widest spread at the smallest K:
                                                        # a weight above 1e-6 lies within ln(1e6 / K) of the largest, and half the levels must)
LADDER_L = 12
RANDOM_SEEDS = 6
GOALS = ((7.0, 4.0), (7.0, 6.0), (6.5, 2.0), (7.5, 3.0), (5.0, 7.0), (7.0, 1.0), (6.0, 4.5), (7.5, 7.5), (4.5, 0.5))


def sizes(rows):
    """K of a row count and of its ragged twin (one rollout in the last row)."""
    return (64 * rows, 64 * rows - 63)


def kstars(K):
    want = (0, 15, 16, 63, 64, K - 65, K - 64, K - 1)
    return sorted({k for k in want if 0 <= k < K})


def _base(name, kind, K, T, lam, inv_var=(4.0, 4.0)):
    return dict(name=name, kind=kind, K=K, T=T, G=G, res=RES, xl=(0.0, G * RES), yl=(0.0, G * RES), thr=THR, lam=lam, sigma=[0.5, 0.5],
                inv_var=list(inv_var), u_min=[0.0, -1.0], u_max=[1.0, 1.0], inst=[])


def _one_hot_instance(K, T, kstar, goal):
    R = np.zeros((G, G), np.float32)
    R[:, 6:] = 1
    state = np.array([2.75 if T >= BASE_T else 2.95, 4.0, 0.0], np.float32)
    mean = np.zeros((T, 2), np.float32)
    mean[:, 0] = 1
    eps = np.zeros((K, T, 2), np.float32)
    eps[kstar, :, 0] = -10
    eps[kstar, :, 1] = np.linspace(-1.5, 1.5, T) if T > 1 else 0.7
    return dict(R=R, state=state, goal=np.array(goal, np.float32), mean=mean, eps=eps, kstar=kstar)


def one_hot(K, T, kstar, lam=0.5, goal=GOALS[0]):
    c = _base(f"onehot_K{K}_T{T}_k{kstar}_l{lam}", "onehot", K, T, lam)
    c["inst"].append(_one_hot_instance(K, T, kstar, goal))
    return c


def batch(B, K, T, lam=0.5):
    c = _base(f"batch_B{B}_K{K}_T{T}", "onehot", K, T, lam)
    ks = kstars(K)
    order = []                                           # another k* per instance: first lane, second row, last rollout, then the list
    for k in [0, 64, K - 1] + ks:
        if 0 <= k < K and k not in order:
            order.append(k)
    for b in range(B):
        c["inst"].append(_one_hot_instance(K, T, order[b % len(order)], GOALS[b % len(GOALS)]))
    return c


def ladder(K, spread, L=LADDER_L):
    T, J = L - 1, L - 1
    p = J / 4 + 0.4
    alpha = spread / (J - p) ** 2
    lam, beta = 0.05 / alpha, alpha * (2 * p + 3)
    c = _base(f"ladder_K{K}_s{spread:g}", "ladder", K, T, lam, inv_var=(beta, 4.0))
    c["L"] = L
    rng = np.random.default_rng(K)
    mean = np.zeros((T, 2), np.float32)
    mean[:, 0] = 1
    eps = np.zeros((K, T, 2), np.float32)
    om = rng.uniform(-1.5, 1.5, (K, T)).astype(np.float32)
    for k in range(K):
        s = k % L
        eps[k, s:, 0] = -10
        eps[k, s:, 1] = om[k, s:]
    c["inst"].append(dict(R=np.zeros((G, G), np.float32), state=np.array([1.0, 4.0, 0.0], np.float32), goal=np.array(GOALS[0], np.float32),
                          mean=mean, eps=eps, kstar=None))
    return c


@functools.lru_cache(maxsize=None)
def random_seeds():
    from test_gpu_fuzz import _case
    out = []
    for seed in range(128):
        if _case(seed)["G"] <= 64:
            out.append(seed)
        if len(out) == RANDOM_SEEDS:
            break
    return tuple(out)


def random(seed):
    from test_gpu_fuzz import _case
    f = _case(seed)
    inv_var = (np.float32(1) / (np.asarray(f["sigma"], np.float32) ** 2)).tolist()
    c = dict(name=f"random_{seed}", kind="random", K=f["K"], T=f["T"], G=f["G"], res=f["res"], xl=tuple(f["xl"]), yl=tuple(f["yl"]), thr=f["thr"],
             lam=f["lam"], sigma=list(f["sigma"]), inv_var=inv_var, u_min=list(f["u_min"]), u_max=list(f["u_max"]), window=f["window"],
             pipeline=f["pipeline"], inst=[dict(R=f["R"], state=f["state"], goal=f["goal"], mean=f["mean"], eps=f["eps"], kstar=None)])
    return c


def oracle_params(case, b=0, ref=False):
    from oracle import oracle as O
    return O.make_params(case["K"], case["T"], case["G"], case["res"], case["inst"][b]["goal"], thr=case["thr"], lambda_=case["lam"],
                         sigma=case["sigma"], inv_var=case["inv_var"], u_min=case["u_min"], u_max=case["u_max"], x_limits=case["xl"],
                         y_limits=case["yl"], trig=O.TRIG_SPEC_PER_STEP if ref else O.TRIG_SPEC)


def reference(case, b=0, ref=False):
    """The float32 CPU oracle's solve of instance b (computed once per case object and arithmetic, never changed)."""
    from oracle import oracle as O
    memo = case.setdefault("_oracle", {})
    if (b, ref) not in memo:
        i = case["inst"][b]
        memo[(b, ref)] = O.solve(oracle_params(case, b, ref), i["R"], i["state"], i["mean"], i["eps"])
    return memo[(b, ref)]


def conditions(case, b, orc):
    """What the case promises, on a (CPU) oracle result of its instance b."""
    w = orc["w"]
    if case["kind"] == "onehot":
        ks = case["inst"][b]["kstar"]
        hot = np.zeros(case["K"], np.float32)
        hot[ks] = 1
        assert np.array_equal(w, hot), (case["name"], b, "the reference's weights are not exactly one-hot")
        assert np.array_equal(orc["Ustar"], orc["U"][ks]) and np.array_equal(orc["Xstar"], orc["X"][ks]), (case["name"], b)
    elif case["kind"] == "ladder":
        L = case["L"]
        assert len(np.unique(orc["cost"])) == L, (case["name"], len(np.unique(orc["cost"])))
        assert len(np.unique(w[w > 1e-6])) >= L / 2, (case["name"], np.unique(w))
        assert (w > 0).all(), (case["name"], "a weight underflowed")
        rows = w[: case["K"] // 64 * 64].reshape(-1, 64)
        assert (rows.max(1) > 1e-6).all(), (case["name"], "a row without weight")


# ---- the sweep of the one-hot recipe -------------------------------------------------------------------------------------------------
def sweep_cases(rows, T=BASE_T, lam=0.5):
    """Every (K, k*) of a row count: the full and the ragged K, each with every k* of the list that K admits."""
    assert T <= 8 or rows < ROWS_SHORT_T
    for K in sizes(rows):
        for ks in kstars(K):
            yield one_hot(K, T, ks, lam)


def yardstick_cases():
    """The cases whose weights spread over many rollouts: where the float32 oracle's own distance to the float64 spec is not zero and
    tests/golden/mppi_tail.json records it."""
    return [ladder(K, s) for K, s in LADDER] + [random(seed) for seed in random_seeds()]
