"""GPU: the dataset stage (benchnav_amd/dataset.py, csrc/dataset_kernels.hip) against tests/dataset_spec.py.

Observations: injected z gives z * std + mean bit for bit; the stream's slips lie within std TOL_Z + 2 ulp32(result) of the float64
spec (the device's Box-Muller is within TOL_Z of float64 on the same words -- test_gpu_noise_streams.py's yardstick, asserted equal
below -- and the product and the sum round once each); chunked calls draw what one call draws; seed, epoch and map index move the
draws.  Gather: x, y, counts and totals equal the spec bit for bit over the case table of dataset_spec (whose properties
test_dataset_host.py asserts) under every visiting order, what lies beyond counts[k] is untouched, and drawing the kept cells in
the kernel equals gathering sample_slips' output.  Dataset: the generated split against single-map generations, its files, the
seed chain, the views' items; then both trainers on it."""
import os
import warnings

import numpy as np
import pytest
import torch

import dataset_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL_Z = 4e-6                   # test_gpu_noise_streams.TOL_Z (asserted equal below)
SEED = 0x9E3779B97F4A7C15      # both key words in use
SENTINEL = -7.0


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ---- observations ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 1021), (5, 4096)]


def _maps(shape, case):
    rng = np.random.default_rng(case)
    return rng.uniform(-0.2, 1.0, shape).astype(f32), rng.uniform(0.01, 0.3, shape).astype(f32)


@pytest.mark.parametrize("shape", SHAPES)
def test_injected_z_is_normal_sample_bit_for_bit(shape):
    from benchnav_amd.dataset import sample_slips
    mean, std = _maps(shape, 1)
    z = np.random.default_rng(2).standard_normal(shape).astype(f32)
    got = sample_slips(_dev(mean), _dev(std), z=_dev(z)).cpu().numpy()
    assert got.shape == shape and np.array_equal(got, S.slips_from_z(z, mean, std))
    assert np.array_equal(got, (torch.from_numpy(z).mul_(torch.from_numpy(std)).add_(torch.from_numpy(mean))).numpy())


@pytest.mark.parametrize("shape", SHAPES)
def test_stream_against_the_float64_spec(shape):
    import test_gpu_noise_streams
    from benchnav_amd.dataset import sample_slips
    assert TOL_Z == test_gpu_noise_streams.TOL_Z
    mean, std = _maps(shape, 3)
    epoch, first = 3, 7
    got = sample_slips(_dev(mean), _dev(std), seed=SEED, epoch=epoch, first_map=first).cpu().numpy().astype(np.float64)
    want = S.observations_z(SEED, first, epoch, *shape) * std.astype(np.float64) + mean.astype(np.float64)
    bound = std.astype(np.float64) * TOL_Z + 2 * np.spacing(np.abs(want).astype(f32)).astype(np.float64)
    err = np.abs(got - want)
    print(f"\n{shape}: max |slip - spec| = {err.max():.3e}, max error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err.max(), int((err > bound).sum()))


def test_chunked_calls_draw_what_one_call_draws():
    from benchnav_amd.dataset import sample_slips
    mean, std = _maps((5, 4096), 4)
    m, s = _dev(mean), _dev(std)
    whole = sample_slips(m, s, seed=SEED, epoch=1)
    parts = torch.cat([sample_slips(m[:2], s[:2], seed=SEED, epoch=1, first_map=0), sample_slips(m[2:], s[2:], seed=SEED, epoch=1, first_map=2)])
    assert torch.equal(whole, parts)
    ragged = sample_slips(m[:, :1021].contiguous(), s[:, :1021].contiguous(), seed=SEED, epoch=1)       # the same blocks, cut earlier
    assert torch.equal(ragged, whole[:, :1021])


def test_seed_epoch_and_map_move_the_draws():
    from benchnav_amd.dataset import sample_slips
    mean, std = _maps((3, 1021), 5)
    m, s = _dev(mean), _dev(std)
    base = sample_slips(m, s, seed=SEED, epoch=2, first_map=4)
    assert torch.equal(base, sample_slips(m, s, seed=SEED, epoch=2, first_map=4))
    for kw in (dict(seed=SEED + 1, epoch=2, first_map=4), dict(seed=SEED ^ (1 << 40), epoch=2, first_map=4), dict(seed=SEED, epoch=3, first_map=4),
               dict(seed=SEED, epoch=2, first_map=5)):
        other = sample_slips(m, s, **kw)
        assert (other != base).float().mean().item() > 0.99, kw
    z = ((base.cpu().numpy().astype(np.float64) - mean) / std)
    assert abs(z.mean()) < 6 / np.sqrt(z.size) and abs(z.std() - 1) < 0.1


# ---- gather ----------------------------------------------------------------------------------------------------------------------------
def _run_gather(c, slips=None, **kw):
    from benchnav_amd.dataset import gather
    x = torch.full((c["C"], c["cap"]), SENTINEL, device="cuda")
    y = torch.full((c["C"], c["cap"]), SENTINEL, device="cuda")
    order = None if c["order"] is None else torch.from_numpy(c["order"])
    x, y, counts, totals = gather(_dev(c["slopes"]), _dev(c["classes"]), c["C"], c["cap"], slips=slips, order=order, x=x, y=y, **kw)
    assert counts.dtype == torch.int32 and totals.dtype == torch.int64
    return x.cpu().numpy(), y.cpu().numpy(), counts.cpu().numpy(), totals.cpu().numpy()


@pytest.mark.parametrize("kind", S.ORDERS)
@pytest.mark.parametrize("name", list(S.CASES))
def test_gather_equals_the_spec(name, kind):
    c = S.make_case(name, kind)
    slips = np.random.default_rng(100 + c["case"]).normal(0.3, 0.2, (c["M"], c["cells"])).astype(f32)
    wx, wy, wcounts, wtotals = S.gather(c["slopes"], slips, c["classes"], c["C"], c["cap"], c["order"])
    got = _run_gather(c, slips=_dev(slips))
    x, y, counts, totals = got
    assert np.array_equal(counts, wcounts) and np.array_equal(totals, wtotals), (counts, wcounts, totals, wtotals)
    for k in range(c["C"]):
        n = int(wcounts[k])
        assert np.array_equal(x[k, :n], wx[k]) and np.array_equal(y[k, :n], wy[k]), k
        assert (x[k, n:] == SENTINEL).all() and (y[k, n:] == SENTINEL).all(), k            # beyond the count nothing is written
    again = _run_gather(c, slips=_dev(slips))
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    if name == "class_absent":
        assert counts[1] == 0 and totals[1] == 0 and (x[1] == SENTINEL).all() and (y[1] == SENTINEL).all()


@pytest.mark.parametrize("name,kind", [("partial_wave_cap1", "null"), ("cap_inside_a_map", "random"), ("cap_never_reached", "reversed"),
                                       ("most_maps_skipped", "random"), ("more_maps_than_threads", "random"), ("cap_on_map_boundary", "identity")])
def test_gather_drawing_on_the_fly_equals_gathering_the_samples(name, kind):
    from benchnav_amd.dataset import sample_slips
    c = S.make_case(name, kind)
    epoch = 5
    slips = sample_slips(_dev(c["mean"]), _dev(c["std"]), seed=SEED, epoch=epoch)
    a = _run_gather(c, slips=slips)
    b = _run_gather(c, mean=_dev(c["mean"]), std=_dev(c["std"]), seed=SEED, epoch=epoch)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    other = _run_gather(c, mean=_dev(c["mean"]), std=_dev(c["std"]), seed=SEED, epoch=epoch + 1)
    assert np.array_equal(a[0], other[0]) and not np.array_equal(a[1], other[1])


def test_gather_rejects_an_order_that_is_no_permutation():
    from benchnav_amd.dataset import gather
    c = S.make_case("one_wave")
    for order in ([0, 0], [1], [5]):
        with pytest.raises(ValueError, match="permutation"):
            gather(_dev(c["slopes"]), _dev(c["classes"]), 1, 10, slips=_dev(c["slopes"]), order=order)


# ---- the dataset -------------------------------------------------------------------------------------------------------------------------
G, RES, TOTAL, SELECTED, ENVIRONMENTS, INSTANCES, BATCH = 32, 0.5, 4, 2, 3, 2, 4
FIELDS = ("heights", "slopes", "latent_mean", "latent_std", "colors")


def _generator(root, split, instances=INSTANCES, **kw):
    from benchnav_amd.dataset import DatasetGenerator, ParamsTerrainGeometry
    from benchnav_amd.terrain import slip_models
    return DatasetGenerator(slip_models(TOTAL), root, split, G, RES, ENVIRONMENTS, instances, num_total_terrain_classes=TOTAL,
                            num_selected_terrain_classes=SELECTED, params_terrain_geometry=ParamsTerrainGeometry(num_craters=2, min_radius=2, max_radius=4),
                            batch=BATCH, **kw)


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dataset"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # craters that do not fit a 32 x 32 map; occupancy rows that sum to 1 + an ulp
        train_gen = _generator(root, "train")
        train = train_gen.generate_dataset()
        valid = _generator(root, "valid", instances=1).generate_dataset()
        memory = _generator(None, "valid", instances=1, seed_information=train.seed_information).generate_dataset()
    return dict(root=root, train=train, valid=valid, memory=memory, plan=train_gen.plan())


def test_every_map_equals_its_single_generation(splits):
    from benchnav_amd.terrain import TerrainGenerator, slip_models
    train, plan = splits["train"], splits["plan"]
    assert len(train) == ENVIRONMENTS * INSTANCES == 6 and len(train) % BATCH                   # the last launch is ragged
    assert train.seeds.tolist() == plan.seeds == list(range(6))
    assert train.t_classes.dtype == torch.int32 and train.t_classes.is_cuda and train.colors.shape == (6, 3, G, G)
    with TerrainGenerator(G, RES, batch=1) as gen, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in range(len(train)):
            t = gen.generate([plan.seeds[m]], num_craters=2, min_radius=2, max_radius=4, occupancy=plan.occupancy[plan.environments[m]],
                             slip_models=slip_models(TOTAL), draws="device")
            for k in FIELDS:
                assert torch.equal(getattr(train, k)[m], getattr(t, k)[0]), (k, m)
            assert torch.equal(train.t_classes[m].cpu().to(torch.int64), t.t_classes[0]), m
    assert len({tuple(train.t_classes[m].unique().tolist()) for m in range(6)}) > 1              # the environments differ in their classes


def test_files_read_back_and_from_directory_round_trips(splits):
    from benchnav_amd.dataset import TerrainDataset
    from benchnav_amd.io import load_instance
    root, train = splits["root"], splits["train"]
    assert train.names == [os.path.join("train", f"{e:03d}_{i:03d}.pt") for e in range(ENVIRONMENTS) for i in range(INSTANCES)]
    for m, name in enumerate(train.names):
        inst = load_instance(os.path.join(root, name))
        assert inst.tensors["t_classes"].dtype == torch.int64 and inst.tensors["colors"].shape == (3, G, G)
        for k in ("heights", "slopes", "colors"):
            assert torch.equal(inst.tensors[k], getattr(train, k)[m].cpu()), (k, m)
        assert torch.equal(inst.tensors["t_classes"], train.t_classes[m].cpu().to(torch.int64))
        assert torch.equal(inst.latent_mean, train.latent_mean[m].cpu()) and torch.equal(inst.latent_std, train.latent_std[m].cpu())
    assert torch.load(os.path.join(root, "train", "seed_information.pt"), weights_only=True) == {"environment_seed": 0, "last_instance_seed": 6}
    back = TerrainDataset.from_directory(root, "train", device="cuda")
    assert back.names == train.names and back.seeds.tolist() == train.seeds.tolist() and back.seed_information == train.seed_information
    for k in FIELDS + ("t_classes",):
        assert getattr(back, k).dtype == getattr(train, k).dtype and torch.equal(getattr(back, k), getattr(train, k)), k


def test_valid_continues_train(splits):
    train, valid, memory = splits["train"], splits["valid"], splits["memory"]
    assert valid.seeds.tolist() == [6, 7, 8] and valid.seed_information == {"environment_seed": 0, "last_instance_seed": 9}
    assert valid.names[0] == os.path.join("valid", "000_000.pt")
    assert memory.seeds.tolist() == valid.seeds.tolist()
    for k in FIELDS + ("t_classes",):
        assert torch.equal(getattr(memory, k), getattr(valid, k)), k
    assert not torch.equal(valid.heights[0], train.heights[0])


def test_items_are_the_references_tuples(splits):
    from benchnav_amd.dataset import SlipRegressionDataset, TerrainClassificationDataset, TraversabilityPredictionDataset, sample_slips
    train = splits["train"]
    clf, reg, trav = TerrainClassificationDataset(train), SlipRegressionDataset(train), TraversabilityPredictionDataset(train)
    assert len(clf) == len(reg) == len(trav) == 6
    want = {clf: [((3, G, G), torch.float32), ((G, G), torch.int64)], reg: [((G, G), torch.float32), ((G, G), torch.float32), ((G, G), torch.int64)],
            trav: [((3, G, G), torch.float32)] + [((G, G), torch.float32)] * 3}
    for view, spec in want.items():
        item = view[4]
        assert len(item) == len(spec)
        for t, (shape, dtype) in zip(item, spec):
            assert t.is_cuda and tuple(t.shape) == shape and t.dtype == dtype
    assert torch.equal(clf[4][0], train.colors[4]) and torch.equal(clf[-2][1], train.t_classes[4].long())
    assert torch.equal(trav[1][2], train.latent_mean[1]) and torch.equal(trav[1][3], train.latent_std[1]) and torch.equal(trav[1][1], train.slopes[1])
    with pytest.raises(IndexError):
        clf[6]
    # the item's slips are row m of the split's stream
    whole = sample_slips(train.latent_mean, train.latent_std, seed=train.observation_seed, epoch=0)
    assert torch.equal(reg[4][1], whole[4]) and torch.equal(reg[4][1], reg[4][1])
    slopes, slips, classes = next(iter(torch.utils.data.DataLoader(reg, batch_size=4, num_workers=0)))
    assert slopes.is_cuda and torch.equal(slips, whole[:4]) and torch.equal(classes, train.t_classes[:4].long())
    # set_epoch moves the slips and nothing else
    before = [[t.clone() for t in view[2]] for view in (clf, reg, trav)]
    reg.set_epoch(1)
    try:
        after = [view[2] for view in (clf, reg, trav)]
        assert train.epoch == 1 and not torch.equal(after[1][1], before[1][1])
        assert torch.equal(after[1][1], sample_slips(train.latent_mean, train.latent_std, seed=train.observation_seed, epoch=1)[2])
        for b, a in zip(before, after):
            for j, (p, q) in enumerate(zip(b, a)):
                assert torch.equal(p, q) or (a is after[1] and j == 1)
    finally:
        reg.set_epoch(0)


# ---- the trainers on the device dataset -------------------------------------------------------------------------------------------------
class _RegressorParams:
    batch_size, learning_rate, num_iterations = 4, 0.1, 2


class _ClassifierParams:
    batch_size, learning_rate, weight_decay, num_epochs, classes = 4, 1e-3, 0.0, 1, TOTAL


def test_load_data_on_the_device_equals_the_spec(splits, tmp_path):
    from benchnav_amd.dataset import SlipRegressionDataset, sample_slips
    from benchnav_amd.gp import SlipRegressorTrainer
    train = splits["train"]
    reg = SlipRegressionDataset(train)
    trainer = SlipRegressorTrainer(torch.device("cuda"), str(tmp_path / "models"), str(tmp_path / "data"), TOTAL, _RegressorParams(), reg)
    perm = torch.from_numpy(np.random.default_rng(9).permutation(len(train)))
    _, _, counts, totals = reg.gather_observations(TOTAL, 50, order=perm)
    assert (totals > 0).all(), totals                   # every class has a cell (else this configuration is to be changed)
    phis, slips = trainer.load_data(num_samples=50, order=perm)
    whole = sample_slips(train.latent_mean, train.latent_std, seed=train.observation_seed, epoch=train.epoch).cpu().numpy()
    wx, wy, wcounts, wtotals = S.gather(train.slopes.cpu().numpy(), whole, train.t_classes.cpu().numpy(), TOTAL, 50, perm.numpy())
    assert np.array_equal(counts.numpy(), wcounts) and np.array_equal(totals.numpy(), wtotals)
    for k in range(TOTAL):
        assert phis[k].is_cuda and np.array_equal(phis[k].cpu().numpy(), wx[k]) and np.array_equal(slips[k].cpu().numpy(), wy[k]), k
    torch.manual_seed(5)
    want = torch.randperm(len(train))
    torch.manual_seed(5)
    a, _ = trainer.load_data(num_samples=50)            # the default order: torch.randperm from the global generator
    b, _ = trainer.load_data(num_samples=50, order=want)
    assert all(torch.equal(a[k], b[k]) for k in range(TOTAL))
    with pytest.raises(ValueError, match="holds no cell of terrain class 4"):
        SlipRegressorTrainer(torch.device("cuda"), str(tmp_path / "m2"), str(tmp_path / "d2"), TOTAL + 1, _RegressorParams(), reg).load_data(50)


def test_train_all_models_writes_what_load_slip_regressors_reads(splits, tmp_path):
    from benchnav_amd.dataset import SlipRegressionDataset
    from benchnav_amd.gp import SlipRegressorTrainer, load_slip_regressors
    reg = SlipRegressionDataset(splits["train"])
    trainer = SlipRegressorTrainer(torch.device("cuda"), str(tmp_path / "models"), str(tmp_path / "data"), TOTAL, _RegressorParams(), reg)
    real = trainer.load_data
    trainer.load_data = lambda: real(num_samples=50)    # 50 points per class keep the fit at a few milliseconds
    torch.manual_seed(1)
    trainer.train_all_models()
    back = load_slip_regressors(TOTAL, trainer.model_directory, str(tmp_path / "data"), device="cuda")
    assert sorted(back) == list(range(TOTAL))
    x = torch.linspace(0, 30, 16, device="cuda")
    for k in range(TOTAL):
        assert back[k].num_points == trainer.regressors[k].num_points <= 50
        got = back[k].predict(x)
        assert torch.isfinite(got.mean).all() and torch.isfinite(got.stddev).all() and (got.stddev > 0).all()


class _Recorded:
    """A view that records the indices it is asked for."""

    def __init__(self, view):
        self.view, self.seen = view, []

    def __len__(self):
        return len(self.view)

    def __getitem__(self, i):
        self.seen.append(int(i))
        return self.view[i]


def test_one_classifier_epoch_on_the_device_dataset(splits, tmp_path):
    from benchnav_amd.dataset import TerrainClassificationDataset
    from benchnav_amd.unet import load_terrain_classifier
    from benchnav_amd.unet_train import ClassifierTrainer, TrainableTerrainClassifier, init_state_dict
    train = splits["train"]
    p = _ClassifierParams()
    data = _Recorded(TerrainClassificationDataset(train))
    trainer = ClassifierTrainer(init_state_dict(TOTAL, seed=0), str(tmp_path), p, data, TerrainClassificationDataset(splits["valid"]))
    torch.manual_seed(3)
    trainer.train()
    assert len(trainer.history["train_iteration"]) == 2 and len(data.seen) == 6 and sorted(data.seen) == list(range(6))
    first = data.seen[:4]
    with TrainableTerrainClassifier(init_state_dict(TOTAL, seed=0), classes=TOTAL) as plain:
        loss = plain.train_step(train.colors[first].clone(), train.t_classes[first].long(), p.learning_rate, p.weight_decay)
    assert loss == trainer.history["train_iteration"][0]                   # the step is deterministic: bit for bit
    clf = load_terrain_classifier(os.path.join(trainer.model_saving_path, "best_model.pth"), classes=TOTAL, device="cuda")
    out = clf.predict(train.colors[:2])
    assert tuple(out.shape) == (2, G, G) and out.dtype == torch.int64 and int(out.min()) >= 0 and int(out.max()) < TOTAL
    clf.close()
    trainer.model.close()
