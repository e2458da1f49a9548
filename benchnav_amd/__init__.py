"""benchnav_amd -- MI355X-native MPPI local planner for BenchNav (hot path only).

    from benchnav_amd import MPPI          # drop-in for src/planners/local_planners/mppi.py:MPPI
    from benchnav_amd import NativeMPPI    # numpy-level wrapper of the C ABI, B instances per call
    from benchnav_amd import AStar         # drop-in for src/planners/global_planners/search_based/astar.py:AStar
    from benchnav_amd import BatchedPlanetaryEnv   # reset / step / collision_check of PlanetaryEnv for B environments on the GPU
    from benchnav_amd import AStarDWALoop  # test_astar_dwa.py's A* + DWA loop on the device, B rovers per launch
    from benchnav_amd import TerrainGenerator   # DatasetGenerator's map instances (geometry + slip model), B per launch
    from benchnav_amd import RRT           # drop-in for src/planners/global_planners/sampling_based/rrt.py:RRT, B plans per launch
    from benchnav_amd import CLRRT         # drop-in for src/planners/global_planners/sampling_based/cl_rrt.py:CLRRT, B plans per launch
    from benchnav_amd import CLRRTLoop     # test_cl_rrt.py's plan-follow-replan loop on the device, B rovers per launch
    from benchnav_amd import TraversabilityPredictor, GPSlipRegressor, load_slip_regressors   # the exact-GP slip prediction stage
    from benchnav_amd import SlipRegressorTrainer   # RegressorTrainer: fits the slip regressors on the GPU (GPSlipRegressor.fit)
    from benchnav_amd import TerrainClassifier, load_terrain_classifier, fold_state_dict   # the U-Net terrain classifier (unet.py)
    from benchnav_amd import TrainableTerrainClassifier, ClassifierTrainer, init_state_dict   # ... and its training (unet_train.py)
    from benchnav_amd import DatasetGenerator, TerrainDataset   # the dataset stage: splits on the device, the reference's files (dataset.py)
    from benchnav_amd import TerrainClassificationDataset, SlipRegressionDataset, TraversabilityPredictionDataset   # ... and its three views
    from benchnav_amd import Benchmark, score_episodes   # the benchmark stage: risk maps, chunked episodes, scores, a report (benchmark.py)
    from benchnav_amd import Evaluator, EvaluationReport, confusion_matrix, slip_metrics, risk_calibration   # how good the models are (evaluate.py)
    from benchnav_amd import TaskSet, passable_mask, label_components, sample_pairs, optimal_lengths   # solvable start/goal pairs, SPL (tasks.py)
"""
from .native import NativeMPPI  # noqa: F401


def __getattr__(name):
    if name == "MPPI":          # every class but NativeMPPI is imported when it is first used
        from .mppi import MPPI
        return MPPI
    if name == "DWA":
        from .dwa import DWA
        return DWA
    if name == "AStar":
        from .astar import AStar
        return AStar
    if name == "BatchedPlanetaryEnv":
        from .env import BatchedPlanetaryEnv
        return BatchedPlanetaryEnv
    if name == "AStarDWALoop":
        from .astar_dwa import AStarDWALoop
        return AStarDWALoop
    if name == "TerrainGenerator":
        from .terrain import TerrainGenerator
        return TerrainGenerator
    if name == "RRT":
        from .rrt import RRT
        return RRT
    if name == "CLRRT":
        from .clrrt import CLRRT
        return CLRRT
    if name == "CLRRTLoop":
        from .clrrt_loop import CLRRTLoop
        return CLRRTLoop
    if name in ("TraversabilityPredictor", "GPSlipRegressor", "load_slip_regressors", "SlipRegressorTrainer"):
        from . import gp
        return getattr(gp, name)
    if name in ("TerrainClassifier", "load_terrain_classifier", "fold_state_dict"):
        from . import unet
        return getattr(unet, name)
    if name in ("TrainableTerrainClassifier", "ClassifierTrainer", "init_state_dict", "pack_state_dict", "unpack_params"):
        from . import unet_train
        return getattr(unet_train, name)
    if name in ("DatasetGenerator", "TerrainDataset", "TerrainClassificationDataset", "SlipRegressionDataset", "TraversabilityPredictionDataset"):
        from . import dataset
        return getattr(dataset, name)
    if name in ("Benchmark", "score_episodes"):
        from . import benchmark
        return getattr(benchmark, name)
    if name in ("Evaluator", "EvaluationReport", "confusion_matrix", "slip_metrics", "risk_calibration"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("TaskSet", "passable_mask", "label_components", "sample_pairs", "optimal_lengths"):
        from . import tasks
        return getattr(tasks, name)
    raise AttributeError(name)
