"""CPU: the graph walk of tests/unet_train_walk.py held to tests/unet_spec.Unet, so that the GPU tests which recompose the device's
training step with it (tests/test_gpu_unet_train_walk.py) cannot be wrong together with it.  walk(TorchBackend(float64)) -- per-layer
primitives, each convolution's backward taken alone, BatchNorm's backward from the closed formula, gradients accumulated in the
reverse node order -- must reproduce whole-network autograd of the float64 spec, and TorchBackend.adam on the walk's gradients must
follow torch.optim.Adam."""
import functools

import pytest
import torch

import unet_cases as UC
import unet_train_cases as TC
from unet_train_walk import TorchBackend, walk

LOSS_BOUND, GRADIENT_BOUND, STATS_BOUND, TRAJECTORY_BOUND = 1e-12, 1e-10, 1e-12, 1e-9


@functools.lru_cache(maxsize=None)
def _walked(name):
    return walk(TorchBackend(torch.float64), UC.state_dict(), TC.colors(name), TC.targets(name))


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_float64_walk_reproduces_the_specs_autograd(name):
    want_loss, want_grads, want_state = TC.reference(name)
    loss, grads, stats = _walked(name)
    assert abs(loss - want_loss) <= LOSS_BOUND, (loss, want_loss)
    assert set(grads) == set(want_grads)
    errors = {k: TC.relative_error(grads[k], want_grads[k]) for k in want_grads}
    worst = max(errors, key=errors.get)
    print(f"\n{name}: |loss - spec| {abs(loss - want_loss):.1e}; worst gradient {worst} {errors[worst]:.1e} of its largest magnitude")
    assert all(grads[k].dtype == torch.float64 and grads[k].shape == want_grads[k].shape for k in grads)
    bad = {k: e for k, e in errors.items() if not e <= GRADIENT_BOUND}
    assert not bad, bad
    assert set(stats) == set(TC.stats_keys(want_state)) and len(stats) == 60
    stat_errors = {k: float((stats[k] - want_state[k]).abs().max()) for k in stats}
    assert max(stat_errors.values()) <= STATS_BOUND, max(stat_errors.items(), key=lambda kv: kv[1])


def test_gradients_come_in_the_backwards_order():
    """The order a failing bit-for-bit comparison reports in: the head first, the stem last; inside layer 2 block 0 the node order
    conv2, conv1, downsample (the downsample stands before conv1 in the forward)."""
    keys = list(_walked("b4_32x32")[1])
    assert keys[:3] == ["segmentation_head.0.weight", "segmentation_head.0.bias", "decoder.blocks.4.conv2.1.weight"]
    assert keys[-3:] == ["encoder.bn1.weight", "encoder.bn1.bias", "encoder.conv1.weight"]
    at = {k: i for i, k in enumerate(keys)}
    for layer in (2, 3, 4):
        p = f"encoder.layer{layer}.0."
        assert at[p + "conv2.weight"] < at[p + "conv1.weight"] < at[p + "downsample.0.weight"]
    assert "encoder.layer1.0.downsample.0.weight" not in at


def test_walk_and_adam_follow_torchs_adam_with_weight_decay():
    """Three steps of TorchBackend.adam (weight decay 1e-2 on every parameter: weights, gamma, beta, the head's bias) on the walk's
    gradients, the running statistics carried along; the loss before each step and after the last against torch.optim.Adam on the
    spec."""
    weight_decay, steps = 1e-2, 3
    want = TC.spec_trajectory(torch.float64, weight_decay=weight_decay)
    be = TorchBackend(torch.float64)
    state = {k: v.double() for k, v in UC.state_dict().items() if not k.endswith("num_batches_tracked")}
    m, v = ({k: torch.zeros_like(state[k]) for k in TC.reference(TC.TRAJECTORY_CASE)[1]} for _ in range(2))
    x, t = TC.colors(TC.TRAJECTORY_CASE), TC.targets(TC.TRAJECTORY_CASE)
    losses = []
    for step in range(1, steps + 2):
        loss, grads, stats = walk(be, state, x, t)
        losses.append(loss)
        if step > steps:
            break
        assert set(grads) == set(m)
        for k, g in grads.items():
            state[k], m[k], v[k] = be.adam(state[k], g, m[k], v[k], step, TC.TRAJECTORY_LR, weight_decay)
        state.update(stats)
    errors = [abs(g - w) / abs(w) for g, w in zip(losses, want)]
    print("\nlosses " + " ".join(f"{g:.12f}" for g in losses) + "\nspec   " + " ".join(f"{w:.12f}" for w in want[:len(losses)])
          + "\nrelative " + " ".join(f"{e:.1e}" for e in errors))
    assert len(errors) == steps + 1 and all(e <= TRAJECTORY_BOUND for e in errors), errors
    assert losses[-1] < losses[0]
