"""GPU: `clrrt_steer` (csrc/clrrt_kernels.hip) against tests/clrrt_spec.py evaluated with the device's own float32 math (`M64R`), on
the table of tests/clrrt_steer_cases.py (644 steers; tests/test_clrrt_steer_table.py proves the table's conditions on the CPU).
Where tests/test_gpu_clrrt.py asks "is this the reference?" and has to allow NumPy's float32 routines their last bit (5e-6 m,
1e-4), this file asks "is this the spec?":

  a. the Dubins half: word, point count and NaN padding equal, every path point within POINT_BOUND_ULPS float64 ulps of the spec's;
  b. the follow half on the device's own points: target index per step, length, feasibility equal; actions, states, cost and the
     float32 integrals bit for bit; the float64 controller errors within 4 ulps;
  c. the tree kernel's steer (`RECORD = false`) against the steer kernel's, bit for bit, through one and two iterations;
  d. placement: one batch, batches of one and the reversed order give the same bits; nothing of a pre-filled buffer survives
     inside a row's valid range.

A case is left out of (a)'s equalities only where the CPU test calls it truncation-marginal, and of (b)'s bit comparison only
where it calls it cast-sensitive (it then meets TOL_TRAJ / COST_REL of tests/test_gpu_clrrt.py); both only if it differs in the
first place, at most 2 % of a group, and never a case whose small angular errors are exact zeros (clrrt_steer_cases.aligned == 2).

Measured on an MI355X (ROCm 7.2) over the whole table: largest path-point difference 1.0 float64 ulp of max(|coordinate|, 1)
(3.6e-15 m) -- the device's float64 sincos against glibc's; asserted 4 x that, which is a power of two: POINT_BOUND_ULPS = 4.
(b) and (c) were bit-equal on every case and nothing was left out.  The float64 controller errors were equal on all but one steer
(random_0[50]), whose angular error differs by one ulp of the modulo's argument 8.76 (1.8e-15, eight ulps of 1.0): the "4 ulps" of
(b) are counted in that unit (clrrt_steer_cases.controller_error_ulps), the number format's own, not in ulps of the wrapped error."""
import functools

import numpy as np
import pytest
import torch

import clrrt_steer_cases as T

pytestmark = pytest.mark.gpu
f32 = np.float32
OLD_COST_REL = 1e-6      # tests/test_gpu_clrrt.py


def _steer_batch(pl, fs, ct, tg):
    """steer_batch in chunks of at most 64, as NumPy arrays."""
    parts = [{n: v.cpu().numpy() for n, v in pl.steer_batch(fs[i:i + 64], ct[i:i + 64], tg[i:i + 64]).items()} for i in range(0, len(fs), 64)]
    return {n: np.concatenate([p[n] for p in parts]) for n in parts[0]}


@functools.lru_cache(maxsize=None)
def device(name):
    g = T.groups()[name]
    return _steer_batch(T.planner(g), g.from_states, g.ctrls, g.targets)


# ---- a. the Dubins half ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.group_names())
def test_dubins_half_equals_the_spec(name):
    dev, sp = device(name), T.spec(name)
    worst, left = (0.0, 0.0), []
    for i, case in enumerate(sp):
        d = T.check_dubins(dev, i, case)
        if d is None or int(dev["word"][i]) != case.steer.word:
            left.append(i)
        else:
            worst = max(worst, d)
    print(f"{name}: largest point difference {worst[0]:.2f} ulps = {worst[1]:.3e} m; left out {len(left)} of {len(sp)} {left}")
    assert len(left) <= T.CAP * len(sp)


# ---- b. the follow half ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.group_names())
def test_follow_half_equals_the_spec_on_the_devices_points_bit_for_bit(name):
    g, dev = T.groups()[name], device(name)
    cfg = T.config(g)
    left, why = [], {}
    for i in range(len(g)):
        want = T.follow_on_device_points(cfg, g, dev, i)
        bad = T.follow_mismatch(dev, i, want)
        if bad is None:
            continue
        why[i] = bad
        # only what the CPU test flags, and then within the bounds the fixture comparison uses
        assert T.cast_sensitive(name, i) and T.aligned(name, i) != 2 and T.loose_follow_ok(dev, i, want, OLD_COST_REL), (name, i, bad)
        left.append(i)
    n = len(g)
    print(f"{name}: bit-equal: {n - len(left)} of {n}; left out {len(left) / n:.1%} {why}")
    assert len([i for i in left if not T.aligned(name, i)]) <= T.CAP * n, why
    assert len(left) <= max(T.CAP * n, sum(T.aligned(name, i) == 1 for i in range(n))), why


# ---- c. the tree kernel's steer against the steer kernel's -----------------------------------------------------------------------
def _tree_buffers(pl):
    from benchnav_amd import _capi
    h = pl._last_handle
    c, B, Sq = h.iters + 1, h.B, h.S
    get = lambda which, shape, t="<f4": h.buffer(which, shape, t).cpu().numpy()
    near, feas = pl.iteration_log()
    return dict(nodes=get(_capi.BN_CLRRT_BUF_NODES, (B, c, 3)), edges=get(_capi.BN_CLRRT_BUF_EDGES, (B, c), "<i4"), costs=get(_capi.BN_CLRRT_BUF_COSTS, (B, c)),
                lens=get(_capi.BN_CLRRT_BUF_SEQ_LENGTHS, (B, c), "<i4"), ctrl=get(_capi.BN_CLRRT_BUF_CONTROLLERS, (B, c, 4)),
                aseq=get(_capi.BN_CLRRT_BUF_ACTION_SEQS, (B, c, Sq, 2)), sseq=get(_capi.BN_CLRRT_BUF_STATE_SEQS, (B, c, Sq + 1, 3)),
                count=get(_capi.BN_CLRRT_BUF_COUNTS, (B,), "<i4"), near=near.cpu().numpy(), feasible=feas.cpu().numpy())


def _node_equals_steer(t, b, node, st, parent, parent_cost):
    """Node `node` of instance b is what steer row b of `st` left: sequences, zero rows behind the length, length, cost, state,
    controller row, bit for bit."""
    L = int(st["length"][b])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert int(t["lens"][b, node]) == L and int(t["edges"][b, node]) == parent
    assert np.array_equal(bits(t["aseq"][b, node, :L]), bits(st["actions"][b, :L])) and not bits(t["aseq"][b, node, L:]).any()
    assert np.array_equal(bits(t["sseq"][b, node, :L + 1]), bits(st["states"][b, :L + 1])) and not bits(t["sseq"][b, node, L + 1:]).any()
    assert np.array_equal(bits(t["nodes"][b, node]), bits(st["states"][b, L]))
    assert np.array_equal(bits(t["costs"][b, node]), bits(f32(parent_cost + st["cost"][b])))
    assert np.array_equal(bits(t["ctrl"][b, node]), bits(st["controllers"][b].astype(f32)))


@pytest.mark.parametrize("k", range(4))
def test_tree_steer_equals_the_steer_kernel_bit_for_bit(k):
    g = T.groups()[f"random_{k}"]
    n, zero = len(g), np.zeros((len(g), 4), f32)
    # one iteration: the root steers to the case's target from zeroed controllers
    pl = T.planner(g, max_iterations=1)
    first = _steer_batch(pl, g.from_states, zero, g.targets)
    pl.grow_from_samples(g.from_states, g.targets[:, None, :].copy())
    t = _tree_buffers(pl)
    assert np.array_equal(t["feasible"][:, 0], first["feasible"]) and not t["near"].any()
    assert np.array_equal(t["count"], 1 + first["feasible"].astype(np.int32))
    assert not t["ctrl"][:, 0].view(np.uint32).any() and not t["aseq"][:, 0].any() and not t["sseq"][:, 0].any()
    for b in np.nonzero(first["feasible"])[0]:
        _node_equals_steer(t, b, 1, first, 0, f32(0))
    # two iterations: a second sample 2 m beyond node 1, so that node 1 is its nearest node
    rng = np.random.default_rng(100 + k)
    node1 = np.stack([first["states"][b, int(first["length"][b])] for b in range(n)])
    step = node1[:, :2] - g.from_states[:, :2]
    dist = np.hypot(step[:, 0], step[:, 1])
    second = np.concatenate([np.clip(node1[:, :2] + 2.0 * step / np.maximum(dist, 1e-6)[:, None], 0.25, 31.75), rng.uniform(0, 2 * np.pi, (n, 1))], 1).astype(f32)
    pl2 = T.planner(g, max_iterations=2)
    pl2.grow_from_samples(g.from_states, np.stack([g.targets, second], 1))
    t2 = _tree_buffers(pl2)
    row1 = first["controllers"].astype(f32)                     # node 1's stored controller row after the first iteration
    again = _steer_batch(pl2, node1, row1, second)
    from_node1 = np.nonzero(first["feasible"] & (t2["near"][:, 1] == 1))[0]
    assert len(from_node1) >= 0.9 * first["feasible"].sum()
    equal = 0
    for b in from_node1:
        assert bool(t2["feasible"][b, 1]) == bool(again["feasible"][b]) and int(t2["count"][b]) == 2 + int(again["feasible"][b])
        # item 9 of DESIGN.md 4.7: node 1's stored integrals are the ones this steer left, feasible or not; its errors stay
        want_row = row1[b].copy()
        want_row[[1, 3]] = again["controllers"][b][[1, 3]].astype(f32)
        assert np.array_equal(t2["ctrl"][b, 1].view(np.uint32), want_row.view(np.uint32))
        if again["feasible"][b]:
            _node_equals_steer(t2, b, 2, again, 1, t2["costs"][b, 1])
            equal += 1
    print(f"random_{k}: bit-equal: {int(first['feasible'].sum())} of {int(first['feasible'].sum())} first steers, {len(from_node1)} of {len(from_node1)} "
          f"second steers ({equal} of them feasible)")


# ---- d. placement ----------------------------------------------------------------------------------------------------------------
def _rows(out, i):
    """The bits of case i's valid ranges."""
    L, n = int(out["length"][i]), int(out["points"][i])
    return (L, n, int(out["word"][i]), bool(out["feasible"][i]), out["path"][i].tobytes(), out["targets"][i, :L].tobytes(), out["actions"][i, :L].tobytes(),
            out["states"][i, :L + 1].tobytes(), out["cost"][i].tobytes(), out["controllers"][i].tobytes())


@pytest.mark.parametrize("name", ["random_0", "edges_B"])
def test_placement_in_the_batch_does_not_change_a_bit(name):
    from benchnav_amd import _capi
    g, dev = T.groups()[name], device(name)
    n = len(g)
    pl = T.planner(g)
    # the steer buffers pre-filled: nothing of it inside a row's valid range, NaN beyond a path
    h = pl._handle(n)
    for which, shape, t in ((_capi.BN_CLRRT_BUF_STEER_ACTIONS, (n, h.S, 2), "<f4"), (_capi.BN_CLRRT_BUF_STEER_STATES, (n, h.S + 1, 3), "<f4"),
                            (_capi.BN_CLRRT_BUF_STEER_PATHS, (n, 64, 2), "<f8"), (_capi.BN_CLRRT_BUF_STEER_COSTS, (n,), "<f4"),
                            (_capi.BN_CLRRT_BUF_STEER_CONTROLLERS, (n, 4), "<f8")):
        h.buffer(which, shape, t).fill_(777.0)
    h.buffer(_capi.BN_CLRRT_BUF_STEER_TARGETS, (n, h.S), "<i4").fill_(777)
    torch.cuda.synchronize()
    filled = _steer_batch(pl, g.from_states, g.ctrls, g.targets)
    for i in range(n):
        L, p = int(filled["length"][i]), int(filled["points"][i])
        assert _rows(filled, i) == _rows(dev, i), i
        assert not (filled["actions"][i, :L] == 777.0).any() and not (filled["states"][i, :L + 1] == 777.0).any() and not (filled["path"][i] == 777.0).any()
        assert (filled["targets"][i, :L] < p).all() and (filled["targets"][i, :L] >= 0).all() and np.isnan(filled["path"][i, p:]).all()
        assert filled["cost"][i] != 777.0 and not (filled["controllers"][i] == 777.0).any()
    rev = _steer_batch(pl, g.from_states[::-1].copy(), g.ctrls[::-1].copy(), g.targets[::-1].copy())
    for i in range(n):
        assert _rows(rev, n - 1 - i) == _rows(dev, i), i
    for i in range(n):
        one = _steer_batch(pl, g.from_states[i:i + 1], g.ctrls[i:i + 1], g.targets[i:i + 1])
        assert _rows(one, 0) == _rows(dev, i), i
