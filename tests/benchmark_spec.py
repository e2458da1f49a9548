"""The scoring specification of the benchmark stage, in NumPy: one plain sequential loop per episode, float64 sums in step order.

bn_episode_score (csrc/score_kernels.hip) is held to this on the GPU (test_gpu_scores.py, test_gpu_campaign.py); here it is the
reference and test_benchmark_spec.py holds IT to hand-computed values.  It shares no code with the package.

done_step is the 0-based index of the step whose resulting state first lay within the goal threshold (reward row done_step, state
row done_step + 1), or -1: what bn_mppi_episode_async and bn_astar_dwa_episode_async write."""
import numpy as np

GOAL, TIME_LIMIT, STOPPED, INVALID = 0, 1, 2, 3
FIELDS = ("outcome", "steps", "time", "path_length", "reward_sum", "reward_min", "stuck_steps", "final_distance")


def max_steps(time_limit, delta_t):
    """The smallest k whose k-fold float64 accumulation of delta_t exceeds time_limit."""
    elapsed, k = 0.0, 0
    while not elapsed > float(time_limit):
        elapsed += float(delta_t)
        k += 1
    return k


def default_end_step(done_step, n):
    """Rows that count when the caller gives no end_step: up to and including the step that reached the goal, else all n."""
    d = np.asarray(done_step, np.int64)
    return np.where(d >= 0, np.minimum(d + 1, n), n).astype(np.int32)


def score_episode(states, rewards, goal, end_step, done_step, stopped=0, invalid=False, stuck_threshold=0.1, delta_t=0.1):
    """One episode: states (n + 1, 3), rewards (n,), goal (2,) float32 -> dict of the eight figures."""
    states, rewards = np.asarray(states, np.float32), np.asarray(rewards, np.float32)
    n = rewards.shape[0]
    end = min(max(int(end_step), 0), n)
    thr = np.float32(stuck_threshold)
    px, py = np.float64(states[0, 0]), np.float64(states[0, 1])
    time, path, rsum = np.float64(0.0), np.float64(0.0), np.float64(0.0)
    rmin = np.float32(np.nan)
    steps = stuck = 0
    for i in range(end):
        r = rewards[i]
        x, y = np.float64(states[i + 1, 0]), np.float64(states[i + 1, 1])
        if not np.isnan(r):                                   # a NaN reward is "no step"
            dx, dy = x - px, y - py
            path = path + np.sqrt(dx * dx + dy * dy)
            time = time + np.float64(delta_t)
            rsum = rsum + np.float64(r)
            rmin = r if steps == 0 or r < rmin else rmin
            stuck += int(r <= thr)
            steps += 1
        px, py = x, y                                         # ... but its state is still where the rover is
    gx, gy = np.float64(np.float32(goal[0])) - px, np.float64(np.float32(goal[1])) - py
    if invalid:
        outcome = INVALID
    elif int(done_step) >= 0:
        outcome = GOAL
    elif int(stopped) != 0:
        outcome = STOPPED
    else:
        outcome = TIME_LIMIT
    return {"outcome": outcome, "steps": steps, "time": float(time), "path_length": float(path), "reward_sum": float(rsum),
            "reward_min": np.float32(rmin), "stuck_steps": stuck, "final_distance": float(np.sqrt(gx * gx + gy * gy))}


def score_episodes(states, rewards, goals, end_step, done_step, stopped=None, invalid=None, stuck_threshold=0.1, delta_t=0.1):
    """states (n + 1, B, 3), rewards (n, B), goals (B, 2) -> dict of (B,) arrays.  end_step None: default_end_step."""
    states, rewards, goals = np.asarray(states, np.float32), np.asarray(rewards, np.float32), np.asarray(goals, np.float32)
    n, B = rewards.shape
    end = default_end_step(done_step, n) if end_step is None else np.asarray(end_step)
    rows = [score_episode(states[:, b], rewards[:, b], goals[b], end[b], done_step[b], 0 if stopped is None else stopped[b],
                          False if invalid is None else bool(invalid[b]), stuck_threshold, delta_t) for b in range(B)]
    dtypes = {"outcome": np.int32, "steps": np.int32, "stuck_steps": np.int32, "reward_min": np.float32}
    return {k: np.array([r[k] for r in rows], dtypes.get(k, np.float64)) for k in FIELDS}


def metric_bound(value, n, u=1):
    """|device - spec| for path_length, reward_sum and final_distance: both sides add the same float64 terms in the same order,
    so only the device square root's u ulps per term can differ: (u + 1) n 2^-52 |value|."""
    return (u + 1) * n * 2.0 ** -52 * np.abs(value)
