"""GPU: training the U-Net terrain classifier at network level (benchnav_amd/unet_train.py) against tests/unet_spec.Unet
in float64 and training mode with F.cross_entropy and torch.optim.Adam (tests/unet_train_cases.py).  The gradient through 20
BatchNorms and the ReLU / max-pool decisions is no smooth function of rounding: the float32 CPU spec itself sits 2e-3 ... 7e-3 (per
tensor, relative L2) from float64, so these bounds (unet_cases.BOUND_FACTOR times the figures of tests/golden/unet_train.json)
catch wiring errors -- a lost skip gradient, a wrong identity path, a mis-ordered concat, all O(1) -- and the layer tests hold the
arithmetic.  Then repeatability, the trajectory of six Adam steps, the trainer and its files, and the errors."""
import os
import types

import numpy as np
import pytest
import torch

import unet_cases as UC
import unet_spec
import unet_train_cases as TC

pytestmark = pytest.mark.gpu


def _net():
    from benchnav_amd import unet_train
    return unet_train.TrainableTerrainClassifier(UC.state_dict(), classes=UC.CLASSES)


def _same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].numpy().reshape(-1).view(np.uint8), b[k].numpy().reshape(-1).view(np.uint8)) for k in a)


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_loss_and_every_gradient_against_the_float64_spec(name):
    want_loss, want_grads, _ = TC.reference(name)
    rec = TC.golden()["network"][name]
    with _net() as net:
        before = net.state_dict()
        loss, grads = net.gradients(TC.colors(name), TC.targets(name))
        assert net.steps == 0 and _same_bits(net.state_dict(), before)           # gradients() changes nothing
    assert set(grads) == set(want_grads)
    loss_error = abs(loss - want_loss) / abs(want_loss)
    per = {k: TC.relative_l2(grads[k], want_grads[k]) for k in want_grads}
    worst = max(per, key=per.get)
    print(f"\n{name}: loss {loss:.7f} (float64 {want_loss:.7f}), relative error {loss_error:.2e} = {loss_error / max(rec['loss_relative_error'], 4 * TC.EPS32):.2f}"
          f" x the float32 CPU figure (floor 4 eps); worst tensor {worst} {per[worst]:.2e} = {per[worst] / rec['gradient_worst_tensor_relative_l2']:.2f}"
          f" x the float32 CPU spec's worst tensor")
    assert loss_error <= TC.loss_bound(rec["loss_relative_error"]), (loss, want_loss)
    bound = UC.BOUND_FACTOR * rec["gradient_worst_tensor_relative_l2"]
    bad = {k: e for k, e in per.items() if not e <= bound}
    assert not bad, (bound, bad)
    assert all(g.dtype == torch.float32 and tuple(g.shape) == tuple(want_grads[k].shape) for k, g in grads.items())


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_running_statistics_after_one_step(name):
    """The spec's state dict after its training-mode forward holds the updated running statistics (momentum 0.1, unbiased
    variance) and num_batches_tracked = 1."""
    _, _, want_state = TC.reference(name)
    rec = TC.golden()["network"][name]
    with _net() as net:
        net.train_step(TC.colors(name), TC.targets(name), lr=1e-3)
        state = net.state_dict()
        assert net.steps == 1
    error = TC.stats_error(state, want_state)
    print(f"\n{name}: running statistics relative error {error:.2e} = {error / max(rec['running_statistics_relative_error'], 4 * TC.EPS32):.2f} x the float32 CPU figure")
    assert error <= TC.loss_bound(rec["running_statistics_relative_error"])
    tracked = [k for k in want_state if k.endswith("num_batches_tracked")]
    assert len(tracked) == 30 and all(state[k].dtype == torch.int64 and int(state[k]) == int(want_state[k]) == 1 for k in tracked)
    unet_spec.Unet(UC.CLASSES).load_state_dict(state, strict=True)


def test_two_handles_and_another_stream_give_the_same_bits():
    name = "b4_32x32"
    x, t = TC.colors(name), TC.targets(name)
    results = []
    for stream in (None, None, torch.cuda.Stream()):
        with _net() as net:
            with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
                loss0, grads = net.gradients(x, t)
                losses = [net.train_step(x, t, lr=1e-3, weight_decay=1e-4) for _ in range(2)]
            results.append((loss0, grads, losses, net.state_dict(), net.adam_state()))
    first = results[0]
    assert first[0] == first[2][0]                         # gradients() and the first step see the same loss
    for other in results[1:]:
        assert other[0] == first[0] and other[2] == first[2]
        assert _same_bits(other[1], first[1]) and _same_bits(other[3], first[3])
        assert _same_bits(other[4][0], first[4][0]) and _same_bits(other[4][1], first[4][1])
    assert any(float(v.abs().max()) > 0 for v in first[4][1].values())


def test_six_adam_steps_follow_the_float64_trajectory():
    want = TC.reference_trajectory()
    rec = TC.golden()["trajectory"]
    x, t = TC.colors(TC.TRAJECTORY_CASE), TC.targets(TC.TRAJECTORY_CASE)
    with _net() as net:
        got = [net.train_step(x, t, lr=TC.TRAJECTORY_LR) for _ in range(TC.TRAJECTORY_STEPS)]
    errors = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print("\nlosses " + " ".join(f"{g:.5f}" for g in got) + "\nfloat64 " + " ".join(f"{w:.5f}" for w in want) + "\nerror over the float32 CPU figure "
          + " ".join(f"{e / max(r, 4 * TC.EPS32):.2f}" for e, r in zip(errors, rec["loss_relative_error"])))
    for step, (e, r) in enumerate(zip(errors, rec["loss_relative_error"])):
        assert e <= TC.loss_bound(r), (step, e, r)
    assert got[-1] < got[0]


class _Maps(torch.utils.data.Dataset):
    def __init__(self, seed, n):
        self.x = UC.draw_colors(seed, n, 32, 32)
        g = torch.Generator().manual_seed(seed)
        coarse = torch.randint(0, UC.CLASSES, (n, 1, 4, 4), generator=g).float()
        self.y = torch.nn.functional.interpolate(coarse, scale_factor=8, mode="nearest")[:, 0].long()

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


def test_trainer_writes_the_references_files_and_repeats_from_its_seed(tmp_path):
    from benchnav_amd import unet, unet_train

    class _KeepingTrainer(unet_train.ClassifierTrainer):
        """keeps the state at every save_model, to compare the file with"""
        saved_states = None

        def save_model(self):
            self.saved_states = (self.saved_states or []) + [self.model.state_dict()]
            super().save_model()
    params = types.SimpleNamespace(batch_size=3, learning_rate=1e-3, weight_decay=1e-4, num_epochs=2, device="cuda")
    train, valid = _Maps(11, 6), _Maps(12, 2)
    packed = []
    for run in ("a", "b"):
        torch.manual_seed(5)
        trainer = _KeepingTrainer(UC.state_dict(), str(tmp_path / run), params, train, valid)
        trainer.train()
        assert trainer.model_directory == str(tmp_path / run / "bs003_lr1e-03_wd1e-04_epochs002")
        path = os.path.join(trainer.model_directory, "models", "best_model.pth")
        assert os.path.isfile(path) and os.path.isdir(os.path.join(trainer.model_directory, "logs"))
        assert len(trainer.history["train_iteration"]) == 4 and len(trainer.history["valid_epoch"]) == 2 and len(trainer.history["train_epoch"]) == 2
        assert all(np.isfinite(v) for v in trainer.history["train_iteration"] + trainer.history["valid_epoch"])
        assert trainer.model.steps == 4
        logs = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(trainer.model_directory, "logs")) for f in fs]
        assert len(logs) == 1 and logs[0].endswith("history.json")
        saved = torch.load(path, map_location="cpu", weights_only=True)
        unet_spec.Unet(UC.CLASSES).load_state_dict(saved, strict=True)
        assert trainer.saved_states and _same_bits(saved, trainer.saved_states[-1])    # the file is the state at the last improvement
        x = UC.draw_colors(13, 2, 32, 32)
        with unet.load_terrain_classifier(path, classes=UC.CLASSES) as loaded, unet.TerrainClassifier(trainer.saved_states[-1], UC.CLASSES) as kept:
            logits = loaded.forward(x)
            assert torch.equal(logits, kept.forward(x)) and torch.isfinite(logits).all()
        improved = [i for i, v in enumerate(trainer.history["valid_epoch"]) if v < min(trainer.history["valid_epoch"][:i] + [float("inf")])]
        assert len(trainer.saved_states) == len(improved)
        if improved[-1] == params.num_epochs - 1:                                      # saved after the last epoch: the current state
            with trainer.model.classifier() as current:
                assert torch.equal(logits, current.forward(x))
        packed.append((unet_train.pack_state_dict(trainer.model.state_dict(), UC.CLASSES), trainer.history))
        trainer.model.close()
    assert np.array_equal(packed[0][0].view(np.uint32), packed[1][0].view(np.uint32)) and packed[0][1] == packed[1][1]


def test_trainer_without_a_validation_set_saves_every_epoch(tmp_path):
    from benchnav_amd import unet, unet_train
    params = types.SimpleNamespace(batch_size=2, learning_rate=1e-3, weight_decay=0.0, num_epochs=1)
    torch.manual_seed(1)
    with _net() as net:
        trainer = unet_train.ClassifierTrainer(net, str(tmp_path), params, _Maps(21, 2))
        trainer.train()
        path = os.path.join(str(tmp_path), "bs002_lr1e-03_wd0e+00_epochs001", "models", "best_model.pth")
        with unet.load_terrain_classifier(path, classes=UC.CLASSES) as loaded, net.classifier() as current:
            x = UC.draw_colors(22, 1, 32, 32)
            assert torch.equal(loaded.forward(x), current.forward(x))
        assert trainer.history["valid_epoch"] == [] and len(trainer.history["train_iteration"]) == 1


def test_invalid_inputs_raise_before_any_launch():
    x, t = TC.colors("b4_32x32"), TC.targets("b4_32x32")
    with _net() as net:
        for call in (net.gradients, lambda a, b: net.train_step(a, b, lr=1e-3)):
            with pytest.raises(ValueError, match="targets"):
                call(x, t[:, :, :31])
            with pytest.raises(ValueError, match="targets"):
                call(x, t.float())
            bad = t.clone()
            bad[0, 0, 0] = UC.CLASSES
            with pytest.raises(ValueError, match=r"\[0, 10\)"):
                call(x, bad)
            bad[0, 0, 0] = -1
            with pytest.raises(ValueError):
                call(x.cuda(), bad.cuda())
            with pytest.raises(ValueError, match="more than 1 value per channel"):
                call(x[:1], t[:1])
            with pytest.raises(ValueError, match="multiples of 32"):
                call(x[:, :, :, :24], t[:, :, :24])
            with pytest.raises(ValueError):
                call(x[:, :2], t)
        assert net.steps == 0
    with pytest.raises(RuntimeError, match="closed"):
        net.gradients(x, t)
    with pytest.raises(RuntimeError, match="closed"):
        net.train_step(x, t, lr=1e-3)
    with pytest.raises(RuntimeError, match="closed"):
        net.state_dict()
