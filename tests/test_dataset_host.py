"""CPU: the dataset stage's host half.
  1. the seed chain, the occupancy rows and the file names of train -> valid -> test subset 1 -> subset 2 against the reference's own
     bookkeeping (tests/golden/dataset_layout.json, recorded by tests/golden/make_golden_dataset.py);
  2. dataset_spec.gather equals the generic SlipRegressorTrainer.load_data on host tensors, on the order the loader visited;
  3. every case of the GPU gather table has the property it is listed for (from the spec alone);
  4. the family's entry points reject bad arguments before the device check."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dataset_spec as S
from benchnav_amd import _capi, dataset as D

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUT = json.load(open(os.path.join(HERE, "golden", "dataset_layout.json")))["splits"]


# ---- 1. planning against the reference ----------------------------------------------------------------------------------------
def _generator(split, root, seed_information=None):
    return D.DatasetGenerator({}, root, split["data_split"], 8, 0.5, split["environment_count"], split["instance_count"],
                              num_total_terrain_classes=split["num_total_terrain_classes"],
                              num_selected_terrain_classes=split["num_selected_terrain_classes"], subset_index=split["subset_index"],
                              seed_information=seed_information)


def _compare(plan, split):
    assert [plan.environment_seed, plan.base_instance_seed] == split["set_seed"]
    assert plan.seed_information == split["seed_information"]
    want = sorted(split["files"], key=lambda f: f["name"])
    assert sorted(plan.file_names) == [f["name"] for f in want]
    by_name = {n: m for m, n in enumerate(plan.file_names)}
    for f in want:
        m = by_name[f["name"]]
        assert plan.seeds[m] == f["seed"], f["name"]
        assert plan.occupancy[plan.environments[m]].tolist() == f["occupancy"], f["name"]        # float32 rows, exactly


def test_seed_chain_and_file_names_through_a_directory(tmp_path):
    root = str(tmp_path)
    assert [(s["data_split"], s["subset_index"]) for s in LAYOUT] == [("train", None), ("valid", None), ("test", 1), ("test", 2)]
    for split in LAYOUT:
        gen = _generator(split, root)
        plan = gen.plan()
        _compare(plan, split)
        assert torch.equal(gen.generate_occupancy_distribution(plan.environment_seed), plan.occupancy)
        folder = os.path.join(root, plan.directory)
        os.makedirs(folder)
        torch.save(plan.seed_information, os.path.join(folder, "seed_information.pt"))           # what generate_dataset leaves for the next split


def test_seed_chain_in_memory():
    info = None
    for split in LAYOUT:
        plan = _generator(split, None, seed_information=info).plan()
        _compare(plan, split)
        info = plan.seed_information
    with pytest.raises(ValueError, match="seed_information"):
        _generator(LAYOUT[1], None).plan()


def test_map_index_seed_and_name():
    plan = D.plan_split("test", 3, 2, 3, 7, 100)
    assert plan.seeds == [100, 101, 102, 103, 104, 105] and plan.environments == [0, 0, 0, 1, 1, 1]
    assert plan.file_names[4] == os.path.join("test", "subset03", "001_001.pt") and plan.last_instance_seed == 106
    assert D.previous_split("test", 3) == os.path.join("test", "subset02") and D.previous_split("test", 1) == "valid"


def test_the_references_validation_errors():
    with pytest.raises(ValueError, match="data_split must be one of 'train', 'valid', 'test'"):
        D.DatasetGenerator({}, None, "training", 8, 0.5, 1, 1)
    with pytest.raises(ValueError, match="subset_index must be specified for generating test data."):
        D.DatasetGenerator({}, None, "test", 8, 0.5, 1, 1)
    assert D.DatasetGenerator({}, None, "train", 8, 0.5, 1, 1, subset_index=4).subset_index is None      # :70-72


# ---- 2. the gather spec against the generic load_data ---------------------------------------------------------------------------
class _Recording(torch.utils.data.Dataset):
    def __init__(self, slopes, slips, classes):
        self.slopes, self.slips, self.classes, self.seen = slopes, slips, classes, []

    def __len__(self):
        return len(self.slopes)

    def __getitem__(self, i):
        self.seen.append(int(i))
        return self.slopes[i], self.slips[i], self.classes[i]


class _Params:
    batch_size, learning_rate, num_iterations = 4, 0.1, 2


@pytest.mark.parametrize("cap", [25, 9999])
def test_gather_spec_equals_the_generic_load_data(tmp_path, cap):
    from benchnav_amd.gp import SlipRegressorTrainer
    rng = np.random.default_rng(3)
    M, G, Cn = 10, 7, 3
    slopes, slips = rng.uniform(0, 30, (M, G, G)).astype(np.float32), rng.normal(0.3, 0.1, (M, G, G)).astype(np.float32)
    classes = rng.integers(-1, Cn + 1, (M, G, G))
    ds = _Recording(torch.from_numpy(slopes), torch.from_numpy(slips), torch.from_numpy(classes))
    trainer = SlipRegressorTrainer("cpu", str(tmp_path / "models"), str(tmp_path / "data"), Cn, _Params(), ds)
    torch.manual_seed(11)
    phis, obs = trainer.load_data(num_samples=cap)
    assert sorted(ds.seen) == list(range(M)) and ds.seen != list(range(M))         # a shuffled visit of every map
    x, y, counts, totals = S.gather(slopes, slips, classes, Cn, cap, order=ds.seen)
    for k in range(Cn):
        assert torch.equal(phis[k], torch.from_numpy(x[k])) and torch.equal(obs[k], torch.from_numpy(y[k]))
        assert counts[k] == min(totals[k], cap) == len(phis[k])
    with pytest.raises(ValueError, match="order="):
        trainer.load_data(order=list(range(M)))


# ---- 3. the GPU case table has the properties it is listed for -------------------------------------------------------------------
def _plan(name, kind):
    c = S.make_case(name, kind)
    return c, S.class_counts(c["classes"], c["C"], c["order"]), S.class_offsets(c["classes"], c["C"], c["order"])


@pytest.mark.parametrize("kind", S.ORDERS)
def test_case_table_preconditions(kind):
    assert [S.CASES[n][1:] for n in S.RANDOM_CASES] == [(1, 64, 1, 10), (1, 63, 2, 1), (5, 1021, 4, 300), (7, 4096, 10, 9999), (300, 256, 3, 50),
                                                        (1100, 64, 2, 40)]
    for name in S.RANDOM_CASES:                                            # the issue's draw
        c = S.make_case(name, kind)
        assert np.array_equal(c["classes"], np.random.default_rng(c["case"]).integers(-1, c["C"] + 1, (c["M"], c["cells"])))
        assert c["classes"].min() == -1 and c["classes"].max() == c["C"]   # both kinds of values that select nothing occur
    c, cnt, off = _plan("partial_wave_cap1", kind)
    assert c["cells"] % 64 and c["cells"] < 64 and c["cap"] == 1
    c, cnt, off = _plan("cap_inside_a_map", kind)
    assert c["cells"] % 64 and ((off < c["cap"]) & (off + cnt > c["cap"]) & (off > 0)).any()
    c, cnt, off = _plan("cap_never_reached", kind)
    assert cnt.sum(0).max() < c["cap"]
    c, cnt, off = _plan("most_maps_skipped", kind)
    skipped = ((off >= c["cap"]) | (cnt == 0)).all(axis=1)
    assert skipped.sum() >= 0.9 * c["M"] and not skipped.all()
    c, cnt, off = _plan("more_maps_than_threads", kind)
    assert c["M"] > 4 * S.WORKGROUP_THREADS and c["M"] % S.WORKGROUP_THREADS
    c, cnt, off = _plan("class_absent", kind)
    assert cnt.sum(0)[1] == 0 and (cnt.sum(0)[[0, 2]] > 0).all()
    c, cnt, off = _plan("class_only_in_last_visited", kind)
    assert (cnt[:-1, 2] == 0).all() and cnt[-1, 2] == 17 and off[-1, 2] == 0
    c, cnt, off = _plan("cap_on_map_boundary", kind)
    assert (cnt == [10, 40]).all() and cnt.sum(0)[0] == c["cap"] and off[1, 1] == c["cap"]
    if kind != "null":
        order = S.make_order(kind, 1100, 5)
        assert sorted(order.tolist()) == list(range(1100))
    if kind == "random":
        assert not np.array_equal(S.make_order(kind, 1100, 5), np.arange(1100))


def test_observation_spec_layout():
    """The spec's own layout: ragged blocks drop the rest, and a map, an epoch or a seed half moves the draws."""
    z = S.observation_z(5, 2, 0, 1021)
    assert z.shape == (1021,) and np.array_equal(z[:8], S.observation_z(5, 2, 0, 8))
    assert np.array_equal(S.observations_z(5, 1, 0, 2, 9)[1], z[:9])
    for other in (S.observation_z(6, 2, 0, 16), S.observation_z(5, 3, 0, 16), S.observation_z(5, 2, 1, 16), S.observation_z(5 + (1 << 32), 2, 0, 16)):
        assert not np.array_equal(other, z[:16])


# ---- 4. rejected arguments --------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_before_the_device_check():
    lib = _capi.load()
    f = np.ones(8, np.float32)
    i32, i64, work = np.zeros(8, np.int32), np.zeros(8, np.int64), np.zeros(64, np.uint8)
    p = lambda a: a.ctypes.data                                                                    # noqa: E731
    assert lib.bn_dataset_gather_workspace_bytes(2, 2) == 2 * 2 * 12 and lib.bn_dataset_gather_workspace_bytes(1 << 32, 2) == 0
    assert lib.bn_dataset_gather_workspace_bytes(2, 0) == 0 and lib.bn_dataset_gather_workspace_bytes(2, 65) == 0

    def gather(slopes=p(f), slips=p(f), mean=p(f), std=p(f), classes=p(i32), order=None, M=2, cells=4, Cn=2, cap=3, x=p(f), y=p(f), counts=p(i32),
               totals=p(i64), ws=p(work), nbytes=64):
        return lib.bn_dataset_gather_async(0, None, slopes, slips, mean, std, classes, order, M, cells, Cn, cap, 0, 0, x, y, counts, totals, ws, nbytes)

    def sample(mean=p(f), std=p(f), z=None, M=2, cells=4, first=0, out=p(f)):
        return lib.bn_dataset_sample_slips_async(0, None, mean, std, z, M, cells, first, 0, 0, out)
    bad = {
        "null": [lambda: gather(slopes=None), lambda: gather(classes=None), lambda: gather(x=None), lambda: gather(y=None), lambda: gather(counts=None),
                 lambda: gather(totals=None), lambda: gather(ws=None), lambda: gather(slips=None, mean=None), lambda: gather(slips=None, std=None),
                 lambda: sample(mean=None), lambda: sample(std=None), lambda: sample(out=None)],
        "num_classes": [lambda: gather(Cn=0), lambda: gather(Cn=65)],
        "cap": [lambda: gather(cap=0), lambda: gather(cap=-5)],
        "2^32": [lambda: gather(M=1 << 32), lambda: sample(M=1 << 32), lambda: sample(first=(1 << 32) - 1), lambda: sample(first=-1)],
        "num_maps": [lambda: gather(M=0), lambda: sample(M=0)],
        "cells": [lambda: gather(cells=0), lambda: sample(cells=0), lambda: gather(cells=1 << 31)],
        "workspace": [lambda: gather(nbytes=47)],
    }
    for word, calls in bad.items():
        for n, call in enumerate(calls):
            assert call() == _capi.BN_ERR_INVALID, (word, n)
            assert word.encode() in lib.bn_dataset_last_error(), (word, n, lib.bn_dataset_last_error())
    if not torch.cuda.is_available():                 # valid arguments reach the device check: no CPU fallback
        assert gather() == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_dataset_last_error()
        assert sample() == _capi.BN_ERR_NO_DEVICE and b"no CPU fallback" in lib.bn_dataset_last_error()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.sample_slips(torch.zeros(1, 4), torch.ones(1, 4))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.DatasetGenerator({}, None, "train", 32, 0.5, 1, 1).generate_dataset()


def test_lazy_exports():
    import benchnav_amd
    for name in ("DatasetGenerator", "TerrainDataset", "TerrainClassificationDataset", "SlipRegressionDataset", "TraversabilityPredictionDataset"):
        assert getattr(benchnav_amd, name) is getattr(D, name)
