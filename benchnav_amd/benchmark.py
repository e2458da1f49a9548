"""The benchmark stage on the device: a test split, its predicted slip distributions, one risk map per map and risk setting, a
planner driving a rover over every map's latent ground truth, and a report of how it went.

    bench = Benchmark(test_split, predictor, start_pos=(4.0, 4.0), goal_pos=(28.0, 28.0), time_limit=100.0, trials=4)
    report = bench.run("mppi", ["expected_value", "var@0.9", "cvar@0.9"], horizon=50, num_samples=1024)
    print(report.table()); report.to_json("report.json")

What a run does, per chunk of `chunk` episodes and per setting: the per-instance risk maps are set device to device from the one
(C, M, G, G) tensor `risk.infer_risk_maps` made, the environment is reset, the fused loop runs `max_steps` control steps with
freeze_on_goal, and `score_episodes` reduces the log to per-episode figures on the device (csrc/score_kernels.hip).  No log row
reaches the host; the score arrays are collected once, at the end of the run.

Episode e = m * trials + r (map m, trial r) is instance e % chunk of chunk e // chunk.  Chunk j's environment seed is
(seed + j) mod 2^64, map m's risk seed (seed + m) mod 2^64 and episode e's CL-RRT stream seed (seed + e) mod 2^32, so a report is a
function of (seed, chunk, trials), which it stores.
An episode whose start or goal is not traversable (one collision draw each, as PlanetaryEnv.__init__ makes them) is INVALID: it is
kept, counted, and left out of every rate and mean.  With `tasks=` (a tasks.TaskSet: start/goal pairs drawn inside one connected
region of passable ground, each with its shortest grid path length) a task that cannot be solved is INVALID too, and the report
adds SPL; without it a report is byte for byte what it was.

A "cl_rrt" run drives `CLRRTLoop` on per-rover risk maps: its log has a row per loop ITERATION, of which a flagged replan takes
one without a step, so it runs `clrrt_iterations(max_steps)` rows; a rover the planner fails (no plan, no sequence, a plan run out,
a path too long, out of bounds) is STOPPED, alone.

The module's arithmetic rules (`max_steps`, `clrrt_iterations`, `episode_slot`, the seed rules, `clrrt_outcome_words`,
`parse_setting`) need no device.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._device import check, resolve_device, stream_ptr

GOAL, TIME_LIMIT, STOPPED, INVALID = (_capi.BN_OUTCOME_GOAL, _capi.BN_OUTCOME_TIME_LIMIT, _capi.BN_OUTCOME_STOPPED,
                                      _capi.BN_OUTCOME_INVALID)
OUTCOMES = ("GOAL", "TIME_LIMIT", "STOPPED", "INVALID")          # indexed by the outcome code
# the per-episode arrays of score_episodes and of a Report, with their dtypes
FIELDS = (("outcome", torch.int32), ("steps", torch.int32), ("time", torch.float64), ("path_length", torch.float64),
          ("reward_sum", torch.float64), ("reward_min", torch.float32), ("stuck_steps", torch.int32), ("final_distance", torch.float64))
_MASK64 = (1 << 64) - 1
_MASK32 = (1 << 32) - 1


# ---- the rules that need no device ---------------------------------------------------------------------------------------------
def max_steps(time_limit: float, delta_t: float) -> int:
    """The smallest k whose k-fold float64 accumulation of delta_t exceeds time_limit: the step at which PlanetaryEnv.step's
    `_elapsed_time += delta_t; is_truncated = _elapsed_time > time_limit` first truncates (1001 for 100 s at 0.1 s, not 1000:
    the sum of a thousand 0.1 is below 100)."""
    dt, limit = float(delta_t), float(time_limit)
    if not dt > 0.0 or not np.isfinite(limit):
        raise ValueError("delta_t must be > 0 and time_limit finite")
    elapsed, k = 0.0, 0
    while not elapsed > limit:
        elapsed += dt
        k += 1
    return k


def clrrt_iterations(max_steps: int) -> int:
    """Loop iterations that end every CL-RRT rover: 2 * max_steps.  An iteration takes a step, flags a replan or finds the rover
    stopped.  The iteration behind a plan never flags one -- the plan's first stored state lies within two transit steps, at most
    0.2 m with the reference's action bounds, of the state it was planned from, and the flag needs a deviation above 1 m
     -- so of two successive iterations of a running rover at least one steps, and the max_steps-th step is the
    time limit.  A campaign does not lean on it: it raises if a rover is still running."""
    return 2 * int(max_steps)


def episode_slot(episode: int, chunk: int) -> Tuple[int, int]:
    """(chunk index, instance within the chunk) of episode e = m * trials + r."""
    return int(episode) // int(chunk), int(episode) % int(chunk)


def chunk_seed(seed: int, chunk_index: int) -> int:
    """The environment seed of chunk j."""
    return (int(seed) + int(chunk_index)) & _MASK64


def risk_seed(seed: int, map_index: int) -> int:
    """The Philox seed of map m's risk samples."""
    return (int(seed) + int(map_index)) & _MASK64


def planner_seed(seed: int, episode: int) -> int:
    """The seed of episode e's CL-RRT sample stream (MT19937 takes 32 bits)."""
    return (int(seed) + int(episode)) & _MASK32


def clrrt_outcome_words(status, done_iter) -> Tuple[np.ndarray, np.ndarray]:
    """A CLRRTLoop's per-rover words as score_episodes takes them: (done_step, stopped), int32.  done_step is done_iter where the
    status is BN_CL_GOAL, else -1; stopped is the status where it is neither RUNNING, GOAL nor TIME_LIMIT, else 0.  The rule the
    loop's device words follow (CLRRTLoop.episode_buffers)."""
    status, done_iter = np.asarray(status, np.int32), np.asarray(done_iter, np.int32)
    regular = (status == _capi.BN_CL_RUNNING) | (status == _capi.BN_CL_GOAL) | (status == _capi.BN_CL_TIME_LIMIT)
    return (np.where(status == _capi.BN_CL_GOAL, done_iter, -1).astype(np.int32), np.where(regular, 0, status).astype(np.int32))


def parse_setting(setting) -> Tuple[str, Optional[float]]:
    """'expected_value', 'var@0.9', 'cvar@0.9' or an (inference_metric, confidence_value) pair -> the pair."""
    if isinstance(setting, str):
        name, _, q = setting.partition("@")
        return (name, float(q)) if q else (name, None)
    name, q = setting
    return str(name), (None if q is None else float(q))


def setting_name(setting) -> str:
    name, q = parse_setting(setting)
    return name if q is None else f"{name}@{q:g}"


# ---- episode scores ----------------------------------------------------------------------------------------------------------------
def _score_pointers(dev: torch.device, n: int, B: int, states: int, rewards: int, goals: int, end_step: Optional[int], done_step: int,
                    stopped: Optional[int], invalid: Optional[int], stuck_threshold: float, delta_t: float, out: Dict[str, torch.Tensor]) -> None:
    """bn_episode_score on torch's current stream of `dev`, from device pointers into the (B,) tensors of `out`."""
    lib = _capi.load()
    p = lambda v: C.c_void_p(v)
    rc = lib.bn_episode_score(dev.index, stream_ptr(dev), p(states), p(rewards), p(goals), p(end_step), p(done_step), p(stopped), p(invalid),
                              int(n), int(B), float(stuck_threshold), float(delta_t), *[p(out[name].data_ptr()) for name, _ in FIELDS])
    if rc == _capi.BN_ERR_INVALID:
        raise ValueError(lib.bn_score_last_error().decode("utf-8", "replace"))
    check(lib, "score", rc)


def _empty_scores(B: int, dev: torch.device) -> Dict[str, torch.Tensor]:
    return {name: torch.empty(B, device=dev, dtype=dt) for name, dt in FIELDS}


def score_episodes(states, rewards, goals, end_step, done_step, stopped=None, invalid=None, stuck_threshold: float = 0.1,
                   delta_t: float = 0.1, device=None) -> Dict[str, torch.Tensor]:
    """Episode logs reduced to outcomes on the device: {outcome, steps, time, path_length, reward_sum, reward_min, stuck_steps,
    final_distance}, each a (B,) device tensor (bn_episode_score; the header documents every figure).

    states (n + 1, B, 3), rewards (n, B), goals (B, 2) float32; end_step (B): how many leading rows count (None: up to and
    including the step that reached the goal, else all n); done_step (B): the 0-based index of the step that reached the goal, or
    -1 (what env.run and AStarDWALoop.run return; from a CLRRTLoop.run log: done_iter where status is BN_CL_GOAL, else -1);
    stopped (B) integers and invalid (B) booleans are optional.  torch tensors or NumPy arrays: arrays are uploaded, which is how a
    host log (a CLRRTLoop.run dict) gets scored.  One launch on torch's current stream."""
    src = states if isinstance(states, torch.Tensor) and states.is_cuda else None
    dev = resolve_device(device if device is not None else (src.device if src is not None else None), "benchmark")

    def dev_tensor(a, dtype, shape, name):
        if a is None:
            return None
        t = torch.as_tensor(a).detach().to(dev, dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
        return t

    st = torch.as_tensor(states)
    if st.dim() != 3 or st.shape[0] < 2 or st.shape[2] != 3:
        raise ValueError(f"states must be (n + 1, B, 3) with n >= 1, got {tuple(st.shape)}")
    n, B = int(st.shape[0]) - 1, int(st.shape[1])
    with torch.cuda.device(dev):
        st = dev_tensor(st, torch.float32, (n + 1, B, 3), "states")
        rw = dev_tensor(rewards, torch.float32, (n, B), "rewards")
        gl = dev_tensor(goals, torch.float32, (B, 2), "goals")
        en = dev_tensor(end_step, torch.int32, (B,), "end_step")
        dn = dev_tensor(done_step, torch.int32, (B,), "done_step")
        sp = dev_tensor(stopped, torch.int32, (B,), "stopped")
        iv = dev_tensor(None if invalid is None else torch.as_tensor(invalid).to(torch.uint8), torch.uint8, (B,), "invalid")
        if rw is None or gl is None or dn is None:
            raise ValueError("rewards, goals and done_step are required")
        out = _empty_scores(B, dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        _score_pointers(dev, n, B, st.data_ptr(), rw.data_ptr(), gl.data_ptr(), ptr(en), dn.data_ptr(), ptr(sp), ptr(iv), stuck_threshold,
                        delta_t, out)
    return out


# ---- the report ----------------------------------------------------------------------------------------------------------------------
class Report:
    """Per-episode arrays shaped (C, M, trials) -- outcome, steps, time, path_length, reward_sum, reward_min, stuck_steps,
    final_distance -- for the C settings of one run, with what the run was a function of: seed, chunk, trials.  A "cl_rrt" run
    also has `plans` (C, M, trials) int32, the planner's forward calls per episode; for the other planners it is None."""

    def __init__(self, planner: str, settings: Sequence[Tuple[str, Optional[float]]], arrays: Dict[str, np.ndarray], seed: int, chunk: int,
                 trials: int, max_steps: int, delta_t: float, time_limit: float, tasks=None) -> None:
        self.planner, self.settings = planner, [parse_setting(s) for s in settings]
        self.seed, self.chunk, self.trials, self.max_steps = int(seed), int(chunk), int(trials), int(max_steps)
        self.delta_t, self.time_limit = float(delta_t), float(time_limit)
        for name, _ in FIELDS:
            setattr(self, name, arrays[name])
        self.plans = arrays.get("plans")
        # with a tasks.TaskSet: every episode's L* (M, trials) float64, and the parameters the tasks were a function of
        self.optimal_length = None if tasks is None else np.asarray(tasks.optimal_length, np.float64)
        self.task_params = None if tasks is None else dict(tasks.params)

    def summary(self) -> List[dict]:
        """Per setting: the counts of the four outcomes, their rates over the non-INVALID episodes, mean and median time to goal
        and mean path length over the GOAL episodes, mean stuck steps and mean reward (per step) over all valid episodes.  A mean
        over nothing is None.  A run on a task set adds `spl`, the mean over the valid episodes of [outcome == GOAL] * L* / max(L, L*),
        and `path_ratio_mean`, the mean of L / L* over the GOAL episodes (tasks.py states L*'s two biases)."""
        mean = lambda a: float(np.mean(a)) if a.size else None
        rows = []
        for c, setting in enumerate(self.settings):
            oc = self.outcome[c].ravel()
            valid, goal = oc != INVALID, oc == GOAL
            n_valid = int(valid.sum())
            counts = {name: int((oc == code).sum()) for code, name in enumerate(OUTCOMES)}
            rates = {name: (counts[name] / n_valid if n_valid else None) for name in OUTCOMES[:3]}
            steps, rsum = self.steps[c].ravel()[valid], self.reward_sum[c].ravel()[valid]
            moved = steps > 0
            rows.append({"setting": setting_name(setting), "episodes": int(oc.size), "valid": n_valid, "counts": counts, "rates": rates,
                         "time_to_goal_mean": mean(self.time[c].ravel()[goal]),
                         "time_to_goal_median": float(np.median(self.time[c].ravel()[goal])) if goal.any() else None,
                         "path_length_mean": mean(self.path_length[c].ravel()[goal]),
                         "stuck_steps_mean": mean(self.stuck_steps[c].ravel()[valid].astype(np.float64)),
                         "reward_mean": mean(rsum[moved] / steps[moved])})
            if self.optimal_length is not None:
                from .tasks import spl_figures
                rows[-1]["spl"], rows[-1]["path_ratio_mean"] = spl_figures(oc, self.path_length[c], self.optimal_length)
        return rows

    def table(self) -> str:
        fmt = lambda v, w, p: f"{'-':>{w}}" if v is None else f"{v:>{w}.{p}f}"
        with_tasks = self.optimal_length is not None
        lines = [f"{'setting':<16}{'valid':>6}{'goal':>8}{'limit':>8}{'stopped':>8}{'t_goal':>9}{'median':>9}{'path':>9}{'stuck':>8}{'reward':>8}"
                 + (f"{'spl':>8}" if with_tasks else "")]
        for r in self.summary():
            lines.append(f"{r['setting']:<16}{r['valid']:>6}{fmt(r['rates']['GOAL'], 8, 3)}{fmt(r['rates']['TIME_LIMIT'], 8, 3)}"
                         f"{fmt(r['rates']['STOPPED'], 8, 3)}{fmt(r['time_to_goal_mean'], 9, 2)}{fmt(r['time_to_goal_median'], 9, 2)}"
                         f"{fmt(r['path_length_mean'], 9, 2)}{fmt(r['stuck_steps_mean'], 8, 1)}{fmt(r['reward_mean'], 8, 3)}"
                         + (fmt(r["spl"], 8, 3) if with_tasks else ""))
        return "\n".join(lines)

    def to_dict(self) -> dict:
        listed = lambda a: [[[None if isinstance(v, float) and v != v else v for v in row] for row in m] for m in a.tolist()]
        doc = {"planner": self.planner, "settings": [setting_name(s) for s in self.settings], "seed": self.seed, "chunk": self.chunk,
               "trials": self.trials, "max_steps": self.max_steps, "delta_t": self.delta_t, "time_limit": self.time_limit,
               "outcomes": list(OUTCOMES), "summary": self.summary(), "episodes": {name: listed(getattr(self, name)) for name, _ in FIELDS}}
        if self.plans is not None:
            doc["episodes"]["plans"] = self.plans.tolist()
        if self.optimal_length is not None:
            number = lambda v: None if v != v else ("inf" if v == float("inf") else v)
            doc["tasks"] = self.task_params
            doc["episodes"]["optimal_length"] = [[number(v) for v in row] for row in self.optimal_length.tolist()]
        return doc

    def to_json(self, path: str) -> None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=1)
            f.write("\n")


# ---- episode drivers: a planner's side of a run ------------------------------------------------------------------------------------------
class EpisodeDriver:
    """What Benchmark.run asks of a planner.  One driver per run; per chunk open(handle, env, first episode, map indices); per
    setting set_risk_maps((B, G, G) device tensor) and, after env.reset, run(rows), the log=False run; then score_inputs(), the
    device pointers (states, rewards, done_step, stopped or None) bn_episode_score reads, and words(), the rovers' int32 device
    words by name (`word_names`); close() once the chunk's scores are written.  handle_kwargs(kw): the keywords of the chunk's
    NativeMPPI; rows(max_steps): the rows of an episode's log.  This base drives closed loops: `loops[-1]` runs, and the loops of
    earlier settings live until close()."""
    word_names: Tuple[str, ...] = ()
    rows = staticmethod(int)

    def __init__(self, bench: "Benchmark", kw: dict) -> None:
        self.bench, self.kw, self.loops = bench, dict(kw), []

    def open(self, pl, env, e0: int, idx: torch.Tensor) -> None:
        self.pl, self.env, self.idx = pl, env, idx

    def run(self, rows: int) -> None:
        self.loops[-1].run(rows, log=False)

    def score_inputs(self):
        return self.loops[-1].episode_buffers()[:4]

    def words(self) -> Dict[str, torch.Tensor]:
        return {}

    def close(self) -> None:
        while self.loops:
            self.loops.pop().close()


class MPPIDriver(EpisodeDriver):
    handle_kwargs = classmethod(lambda cls, kw: {"horizon": 50, "num_samples": 1024, **kw})

    def set_risk_maps(self, chunk_risk: torch.Tensor) -> None:
        for b in range(self.env.B):
            self.pl.set_map_device(chunk_risk[b].data_ptr(), b)

    def run(self, rows: int) -> None:
        self.env.run(rows, log=False)

    def score_inputs(self):
        return self.pl.episode_buffers()[:3] + (None,)


class AStarDWADriver(EpisodeDriver):
    # the DWA rolls its candidates out on this handle's kernels
    handle_kwargs = classmethod(lambda cls, kw: {"horizon": kw.get("horizon", 10), "num_samples": 64})

    def set_risk_maps(self, chunk_risk: torch.Tensor) -> None:
        """A fresh loop on the split's heights: it sets the planner's maps and solves A* on them."""
        from .astar_dwa import AStarDWALoop
        bn, kw = self.bench, self.kw
        self.loops.append(AStarDWALoop(self.env, bn.dataset.heights[self.idx], chunk_risk, stuck_threshold=bn.stuck_threshold,
                                       a_lim=kw.get("a_lim", (0.5, 0.5)), delta_t=kw.get("dwa_delta_t", bn.delta_t),
                                       num_lin_vel=kw.get("num_lin_vel", 10), num_ang_vel=kw.get("num_ang_vel", 10),
                                       lookahead_distance=kw.get("lookahead_distance", 1.0), walk=kw.get("walk", "serial")))


class CLRRTDriver(EpisodeDriver):
    word_names = ("status", "plans")
    rows = staticmethod(clrrt_iterations)
    # the handle carries the environment; nothing solves on it
    handle_kwargs = classmethod(lambda cls, kw: {"horizon": 8, "num_samples": 64})

    def __init__(self, bench: "Benchmark", kw: dict) -> None:
        unknown = set(kw) - {"max_iterations", "max_seqs", "delta_distance", "goal_sample_rate", "path_cap"}
        if unknown:
            raise TypeError(f"unknown cl_rrt keywords: {sorted(unknown)}")
        super().__init__(bench, kw)
        self.rrts: Dict[int, object] = {}                                    # the chunk size's CLRRT

    def open(self, pl, env, e0: int, idx: torch.Tensor) -> None:
        """One loop per chunk (its rovers' maps change with the setting), on a CLRRT with the grid, limits and action bounds of
        the environment's handle."""
        from .clrrt import CLRRT
        from .clrrt_loop import CLRRTLoop
        bn = self.bench
        if env.B not in self.rrts:
            self.rrts[env.B] = CLRRT.from_parameters(bn.G, bn.resolution, pl.x_limits, pl.y_limits, stuck_threshold=bn.stuck_threshold,
                                                     delta_t=bn.delta_t, goal_threshold=bn.goal_threshold, device=str(bn.dev),
                                                     seed=bn.seed & _MASK32, **self.kw)
        self.loops = [CLRRTLoop(env, self.rrts[env.B], seeds=[planner_seed(bn.seed, e0 + i) for i in range(env.B)])]

    def set_risk_maps(self, chunk_risk: torch.Tensor) -> None:
        self.loops[0].set_risk_maps(chunk_risk)

    def words(self) -> Dict[str, torch.Tensor]:
        return dict(zip(self.word_names, self.loops[0].rover_buffers()))


DRIVERS = {"mppi": MPPIDriver, "astar_dwa": AStarDWADriver, "cl_rrt": CLRRTDriver}
PLANNERS = tuple(DRIVERS)


def _raise_if_running(status: Optional[np.ndarray], settings, rows: int) -> None:
    """status: the (C, ...) status words a driver reported, or None.  A rover still RUNNING breaks clrrt_iterations' bound."""
    running = np.argwhere(status.reshape(len(settings), -1) == _capi.BN_CL_RUNNING) if status is not None else np.empty((0, 2))
    if running.size:
        c, e = (int(v) for v in running[0])
        raise RuntimeError(f"episode {e} under setting {setting_name(settings[c])} is still running after {rows} loop iterations "
                           f"({len(running)} such episodes): clrrt_iterations' bound does not hold")


# ---- the benchmark -----------------------------------------------------------------------------------------------------------------------
class Benchmark:
    def __init__(self, dataset, predictor=None, start_pos=(4.0, 4.0), goal_pos=(28.0, 28.0), delta_t: float = 0.1, time_limit: float = 100.0,
                 stuck_threshold: float = 0.1, goal_threshold: float = 1.0, trials: int = 1, chunk: int = 64, seed: int = 0,
                 num_samples: int = 1000, resolution: float = 0.5, tasks=None) -> None:
        """dataset: a dataset.TerrainDataset (the test split).  predictor: a gp.TraversabilityPredictor, asked for `chunk` maps per
        predict_maps call on colours and slopes; None takes the latent model as the prediction, as io.planner_inputs does.
        start_pos, goal_pos: (2,) for every map or (M, 2).  trials: episodes per map (they differ in the environment's slip draws
        and the planner's noise).  num_samples: samples per cell of the risk maps.  resolution: metres per cell of the maps.
        tasks: a tasks.TaskSet of (M, trials) pairs instead of start_pos and goal_pos: episode e = m * trials + r starts at
        tasks.start[m, r] and aims at tasks.goal[m, r], a task that is not valid is INVALID (next to the two collision draws), and
        the report gains optimal_length, spl and path_ratio_mean."""
        self.dataset, self.predictor = dataset, predictor
        self.M, self.G = len(dataset), dataset.grid_size
        if self.M < 1:
            raise ValueError("the split is empty")
        self.trials, self.chunk, self.seed = int(trials), int(chunk), int(seed)
        if self.trials < 1 or self.chunk < 1:
            raise ValueError("trials and chunk must be >= 1")
        self.delta_t, self.time_limit = float(delta_t), float(time_limit)
        self.stuck_threshold, self.goal_threshold = float(stuck_threshold), float(goal_threshold)
        self.num_samples, self.resolution = int(num_samples), float(resolution)
        per_map = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), (self.M, 2)))
        self.start_pos, self.goal_pos = per_map(start_pos), per_map(goal_pos)
        self.tasks = tasks
        if tasks is not None and tuple(tasks.valid.shape) != (self.M, self.trials):
            raise ValueError(f"tasks must hold ({self.M}, {self.trials}) pairs, got {tuple(tasks.valid.shape)}")
        self.max_steps = max_steps(self.time_limit, self.delta_t)
        self.dev = resolve_device(dataset.device if dataset.device.type == "cuda" else None, "benchmark")

    # -- predictions and risk maps --
    def predictions(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean, std), each (M, G, G) on the device."""
        ds = self.dataset
        if self.predictor is None:
            return ds.latent_mean.to(self.dev, torch.float32), ds.latent_std.to(self.dev, torch.float32)
        means, stds = [], []
        for m0 in range(0, self.M, self.chunk):
            mean, std = self.predictor.predict_maps(ds.slopes[m0:m0 + self.chunk].to(self.dev), colors=ds.colors[m0:m0 + self.chunk].to(self.dev))
            means.append(mean.to(torch.float32))
            stds.append(std.to(torch.float32))
        return torch.cat(means), torch.cat(stds)

    def risk_maps(self, settings) -> torch.Tensor:
        """(C, M, G, G): every map's risk map under every setting, one launch (risk.infer_risk_maps)."""
        from .risk import infer_risk_maps
        mean, std = self.predictions()
        return infer_risk_maps(mean, std, [parse_setting(s) for s in settings], num_samples=self.num_samples,
                               seeds=[risk_seed(self.seed, m) for m in range(self.M)], device=self.dev)

    # -- a run --
    def _chunk(self, handles: Dict[int, object], kw: dict, j: int):
        """Chunk j: (its first episode, the planner handle of its size -- made with `kw` where `handles` has none: a last, shorter
        chunk gets one of its own --, the environment, every instance's map index (B,) on the device, the INVALID flags (B,) uint8)."""
        from .env import BatchedPlanetaryEnv
        from .native import NativeMPPI
        ds, dev, e0 = self.dataset, self.dev, j * self.chunk
        B = min(self.chunk, self.M * self.trials - e0)
        if B not in handles:
            handles[B] = NativeMPPI(grid_size=self.G, resolution=self.resolution, num_instances=B, shared_map=False, stuck_threshold=self.stuck_threshold,
                                    stream=torch.cuda.current_stream(dev).cuda_stream, device_id=dev.index, **kw)
        pl = handles[B]
        maps = [(e0 + i) // self.trials for i in range(B)]
        idx = torch.as_tensor(maps, device=dev)
        if self.tasks is None:
            starts, goals, no_task = self.start_pos[maps], self.goal_pos[maps], None
        else:
            flat = lambda a: a.reshape(self.M * self.trials, -1)[e0:e0 + B]
            no_task = ~flat(self.tasks.valid)[:, 0]
            starts, goals = flat(self.tasks.start), flat(self.tasks.goal)
            nowhere = ~(np.isfinite(starts).all(axis=1) & np.isfinite(goals).all(axis=1))   # no pair was found: INVALID wherever it stands
            starts = np.where(nowhere[:, None], self.start_pos[maps], starts).astype(np.float32)
            goals = np.where(nowhere[:, None], self.goal_pos[maps], goals).astype(np.float32)
        env = BatchedPlanetaryEnv(pl, ds.latent_mean[idx].cpu().numpy(), ds.latent_std[idx].cpu().numpy(), starts,
                                  goals, delta_t=self.delta_t, time_limit=self.time_limit,
                                  stuck_threshold=self.stuck_threshold, goal_threshold=self.goal_threshold,
                                  seed=chunk_seed(self.seed, j), freeze_on_goal=True, check_positions=False)
        at = lambda pos: torch.cat([pos, torch.zeros(B, 1, device=dev)], 1).unsqueeze(1)
        bad_start = env.collision_check(at(env._start_pos))[:, 0]          # PlanetaryEnv.__init__'s two draws, kept per instance
        bad_goal = env.collision_check(at(env._goal_pos))[:, 0]
        bad = bad_start | bad_goal
        if no_task is not None:
            bad = bad | torch.as_tensor(no_task, device=dev)
        return e0, pl, env, idx, bad.to(torch.uint8).contiguous()

    def run(self, planner: str, settings, **planner_kwargs) -> Report:
        """Every episode of the split under every setting.  planner "mppi": planner_kwargs go to NativeMPPI (horizon, num_samples,
        sigmas, lambda_, seed, ...).  "astar_dwa": horizon (10), a_lim ((0.5, 0.5)), dwa_delta_t (delta_t), num_lin_vel (10),
        num_ang_vel (10), lookahead_distance (1.0), walk ("serial"); the A* planner reads the split's heights.  "cl_rrt": the
        reference CLRRT's max_iterations (500), max_seqs (250), delta_distance (5), goal_sample_rate (0.25) and path_cap (None);
        a rover still running after clrrt_iterations(max_steps) iterations raises."""
        if planner not in PLANNERS:
            raise ValueError(f"planner must be one of {PLANNERS}")
        settings = [parse_setting(s) for s in settings]
        dev, n, E, Cn = self.dev, self.max_steps, self.M * self.trials, len(settings)
        drv = DRIVERS[planner](self, planner_kwargs)
        rows = drv.rows(n)                                             # rows of an episode's log
        with torch.cuda.device(dev):
            risk = self.risk_maps(settings)
            total = {name: torch.empty(Cn, E, device=dev, dtype=dt) for name, dt in FIELDS + tuple((w, torch.int32) for w in drv.word_names)}
            handles: Dict[int, object] = {}
            try:
                for j in range((E + self.chunk - 1) // self.chunk):
                    e0, pl, env, idx, invalid = self._chunk(handles, drv.handle_kwargs(planner_kwargs), j)
                    drv.open(pl, env, e0, idx)
                    for c in range(Cn):
                        chunk_risk = risk[c, idx].contiguous()
                        drv.set_risk_maps(chunk_risk)
                        env.reset(seed=chunk_seed(self.seed, j))       # (resets the chunk's loop too)
                        pl.set_mean(None)
                        drv.run(rows)
                        states, rewards, done, stopped = drv.score_inputs()
                        out = {name: t[c, e0:e0 + env.B] for name, t in total.items()}
                        _score_pointers(dev, rows, env.B, states, rewards, env._goal_pos.data_ptr(), None, done, stopped, invalid.data_ptr(),
                                        self.stuck_threshold, self.delta_t, out)
                        for name, view in drv.words().items():
                            out[name].copy_(view)
                    torch.cuda.current_stream(dev).synchronize()       # the chunk's scores are written: its loops and maps may go
                    drv.close()
                arrays = {name: t.cpu().numpy().reshape(Cn, self.M, self.trials) for name, t in total.items()}
            finally:
                for pl in handles.values():
                    pl.close()
        _raise_if_running(arrays.pop("status", None), settings, rows)
        return Report(planner, settings, arrays, self.seed, self.chunk, self.trials, n, self.delta_t, self.time_limit, tasks=self.tasks)
