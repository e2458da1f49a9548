"""GPU: the fused A* + DWA loop (benchnav_amd.AStarDWALoop, csrc/astar_dwa.hip) against the CPU oracle (astar_dwa_oracle.Loop),
step by step and bit for bit.

The device runs each scenario (tests/astar_dwa_scenarios.py) once, free-running.  The oracle is then replayed FROM THE DEVICE'S
LOG: step j starts from the device's state j with the device's action j - 1 as the window centre, and its sub-goal, action, next
state and reward are compared with row j, so a step that is not compared hides nothing after it.  A step is not compared for
sub-goal, action and next state only where the oracle says the pick hangs on the last bits of atan2f (bearing_margin <= DELTA,
derived from the two measured atan2f errors); there the device's sub-goal must still be a point of the oracle's path and its next
state the oracle's environment step of its own action.  At most 2 % of a scenario's steps may be such steps."""
import numpy as np
import pytest

import astar_dwa_oracle as L
import astar_dwa_scenarios as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CAP = 0.02


def _device_run(sc, walk, lds_window):
    import torch
    from benchnav_amd import AStarDWALoop, NativeMPPI
    from benchnav_amd.env import BatchedPlanetaryEnv
    B = len(sc["starts"])
    pl = NativeMPPI(horizon=S.T, num_samples=64, grid_size=sc["G"], resolution=sc["res"], x_limits=sc["x_limits"], y_limits=sc["x_limits"],
                    num_instances=B, shared_map=(sc["risks"].ndim == 2), stream=0, stuck_threshold=S.THR, lds_window=lds_window, **sc["planner"])
    env = BatchedPlanetaryEnv(pl, sc["latent"][0], sc["latent"][1], sc["starts"], sc["goals"], stuck_threshold=S.THR, goal_threshold=1.0, seed=7)
    loop = AStarDWALoop(env, sc["heights"], sc["risks"], S.THR, S.A_LIM, S.DWA_DT, sc["nv"], sc["nw"], S.LOOK, walk=walk)
    env.reset()
    out = loop.run(sc["n"], z=torch.from_numpy(S.draws(sc)).cuda())
    return out + (loop.status_step.copy(),)


def _replay(name, sc, out):
    """Hold the device's log to the oracle; returns per instance (steps compared, steps skipped, kept-path indices of compared picks)."""
    states, rewards, actions, sub_goals, done, status, status_step = out
    n, z, summary = sc["n"], S.draws(sc), []
    for b in range(len(sc["starts"])):
        lp = S.oracle_loop(sc, b)
        compared = skipped = 0
        done_step, kept_idx = -1, []
        for j in range(n):
            at = (name, b, j)
            s = states[j, b]
            if lp.status != L.OK:                                            # the reference loop has raised: the rover stays put
                assert np.array_equal(states[j + 1, b], s) and np.isnan(rewards[j, b]) and np.isnan(actions[j, b]).all() \
                    and np.isnan(sub_goals[j, b]).all(), at
                continue
            lp.prev = actions[j - 1, b].copy() if j else np.zeros(2, np.float32)
            margin, idx, kept = lp.preview(s)
            o = lp.step(j, s, z[j, b])
            if o is None:
                assert np.array_equal(states[j + 1, b], s) and np.isnan(rewards[j, b]) and np.isnan(actions[j, b]).all() \
                    and np.isnan(sub_goals[j, b]).all(), at
                continue
            ns, rw, term, sg, a = o
            assert rewards[j, b] == rw, at + (rewards[j, b], rw)
            if margin <= L.DELTA:
                skipped += 1
                assert np.any(np.all(lp.path == sub_goals[j, b], axis=1)) or np.array_equal(sub_goals[j, b], lp.goal_pos), at
                ns, rw, term = O.env_step_sampled(lp.pe, lp.MU, lp.SG, z[j, b], lp.goal_thr, s, actions[j, b])
                assert np.array_equal(states[j + 1, b], ns), at
            else:
                compared += 1
                assert np.array_equal(sub_goals[j, b], sg), at + (sub_goals[j, b], sg, idx)
                assert np.array_equal(actions[j, b], a), at + (actions[j, b], a)
                assert np.array_equal(states[j + 1, b], ns), at + (states[j + 1, b], ns)
                if kept:
                    kept_idx.append(idx)
            if term and done_step < 0:
                done_step = j
        assert (int(done[b]), int(status[b]), int(status_step[b])) == (done_step, lp.status, lp.status_step), (name, b)
        print(f"{name}[{b}]: {compared} steps compared, {skipped} skipped (DELTA = {L.DELTA:.3e}), status {lp.status} at {lp.status_step}")
        assert skipped <= CAP * n, (name, b, skipped)
        summary.append((compared, skipped, kept_idx))
    return summary


# last_byte_b must run directly after last_byte_a (parametrize keeps this order): the two swap which rover's last byte of `next` is
# a hop and which is 255, so that a byte left over in LDS from the run before cannot be right for both.
RUNS = [(f"case_{c}", walk, True) for c in S.CASES for walk in ("serial", "jump")] + [
    ("general33", "serial", True), ("last_byte_a", "serial", True), ("last_byte_b", "serial", True),
    ("origin", "serial", True), ("origin", "serial", False), ("big416", "serial", True),
    ("spiral_1x1", "serial", True), ("spiral_3x5", "serial", True), ("spiral_3x5", "jump", True), ("spiral_32x32", "serial", True),
    ("late_fallback", "serial", True), ("late_fallback", "jump", True)]


@pytest.mark.parametrize("name,walk,lds_window", RUNS, ids=[f"{n}-{w}-{'win' if l else 'nowin'}" for n, w, l in RUNS])
def test_device_loop_replayed_against_the_oracle(name, walk, lds_window):
    from benchnav_amd import _capi
    sc = S.scenario(name)
    out = _device_run(sc, walk, lds_window)
    summary = _replay(name, sc, out)
    status = out[5]
    # what the scenario is there for, from the oracle's side
    if name == "late_fallback":              # pass 2 finds the pick beyond the first 64-lane segment of a kept path
        assert sc["nv"] * sc["nw"] <= 64 and max(summary[0][2]) >= 64
    if name == "big416":                     # `next` stays in global memory
        assert S.lds_bytes(sc, 0) > 160 * 1024
    if name == "general33":                  # byte-wise staging of `next`, unaligned for b >= 1, with a rover still running
        assert sc["G"] ** 2 % 4 == 1 and _capi.BN_AD_OK in status and len(status) == 3
    if name.startswith("last_byte_"):        # ... and its last byte decides: a fresh path for one rover, the goal for the other
        hop, none = (1, 2) if name == "last_byte_a" else (2, 1)
        sub_goals, cells = out[3], [L.start_cell(s, 0.0, 0.0, sc["res"]) for s in out[0][:, 1:].reshape(-1, 3)]
        assert sc["G"] ** 2 % 4 == 1 and set(cells) == {(32, 32)} and list(status) == [_capi.BN_AD_OK] * 3
        assert np.all(sub_goals[:, none] == sc["goals"][none]) and not np.any(np.all(sub_goals[:, hop] == sc["goals"][hop], axis=1))
        assert summary[hop][0] == summary[none][0] == sc["n"]
    if name.startswith("spiral_"):
        assert summary[0][0] >= 0.98 * sc["n"]
    if name == "case_edge":
        assert status[0] == _capi.BN_AD_OUT_OF_BOUNDS and out[6][0] > 0
    if name == "case_goal_collision":
        assert status[0] == _capi.BN_AD_GOAL_COLLISION and out[6][0] == 0
