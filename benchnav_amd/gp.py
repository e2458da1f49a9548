"""Exact-GP slip prediction on the GPU: mirror of TraversabilityPredictor.predict and of the GP slip regressors behind it
(reference src/prediction_models/traversability_predictors/classifier_and_regressor.py:42-72, slip_regressors/gpr.py,
trainers/utils.py:65-108).  The stage that fills `distributions["predictions"]` (SURVEY "next" row N4).

The regressor is gpytorch's ExactGP with ConstantMean, ScaleKernel(RBFKernel) and GaussianLikelihood on a 1-D input, evaluated
from its equations -- gpytorch is not imported:

    k(a, b) = s exp(-(a - b)^2 / (2 l^2)),   K = k(x, x) + noise I = L L^T,   alpha = K^-1 (y - c)
    mean(phi) = c + k(phi, x) . alpha,       v = L^-1 k(x, phi),              std(phi) = sqrt(max(s - |v|^2, 0) + noise)

The host factorises once per regressor in float64 (NumPy; above 1024 points the explicit L^-1 comes from torch's triangular
solve); the device evaluates every cell in float64 and rounds the outputs.  Up to MAX_POINTS = 10240 training points per class
(the reference's trainer keeps up to 9999, regressor_trainer.py:91-124): regressors of up to 1024 points run on a kernel that
holds k(x, phi) in LDS, larger ones on one that regenerates it slab by slab.
The UNet terrain classifier is unet.TerrainClassifier; any object with `.predict(colors[None]) -> classes` serves
too, or pass the class maps.

The step that makes the regressors is here too (csrc/gp_fit_kernels.hip): `GPSlipRegressor.fit` runs
RegressorTrainer.train's Adam on the exact marginal log-likelihood in float64 on the device and hands its factorisation to the
predict kernels; `GPSlipRegressor(..., factorization="device")` factorises given hyperparameters there instead of on the host;
`SlipRegressorTrainer` keeps the reference trainer's interface and file layout, which `load_slip_regressors` reads back.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch.distributions import Normal

from . import _capi
from ._device import Handle, check, resolve_device, stream_ptr

MAX_POINTS = 10240          # bn_gp_max_points(): 640 row blocks of 16; L^-1 is 420 MB on the device at this size
_NUMPY_SOLVE_MAX = 1024     # up to here L^-1 comes from np.linalg.solve(L, I), as it always has; above, from a triangular solve
MAX_CLASSES = 32
_NOISE_LOWER_BOUND = 1e-4   # GaussianLikelihood's default GreaterThan(1e-4) on the noise


def _scalar(v, name: str) -> float:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().to(torch.float64).numpy()
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size != 1:
        raise ValueError(f"{name} must hold one value, got {a.size}")
    if not np.isfinite(a[0]):
        raise ValueError(f"{name} must be finite")
    return float(a[0])


def _vector(v, name: str) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    a = np.asarray(v)
    if a.ndim == 2 and a.shape[1] == 1:                  # gpytorch keeps a 1-D input as (N, 1)
        a = a[:, 0]
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {a.shape}")
    a = a.astype(np.float32).astype(np.float64)          # the reference trains on float32: widened exactly
    if not np.isfinite(a).all():
        raise ValueError(f"{name} must be finite")
    return a


def factorize(train_x, train_y, constant: float, outputscale: float, lengthscale: float, noise: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(x, alpha, L^-1) in float64 for the device: K = outputscale exp(-(x - x')^2 / (2 lengthscale^2)) + noise I = L L^T,
    alpha = K^-1 (y - constant), L^-1 explicit and lower triangular.

    No jitter is added (gpytorch retries a failed Cholesky with 1e-6 ... 1e-4 on the diagonal; here a matrix that is not
    numerically positive definite raises ValueError).  1 <= N <= MAX_POINTS, else ValueError (raised before K is built: K and
    L^-1 take 8 N^2 bytes each, 0.8 GB at N = 9999)."""
    x, y = _vector(train_x, "train_x"), _vector(train_y, "train_y")
    n = x.shape[0]
    if y.shape[0] != n:
        raise ValueError(f"train_x and train_y differ in length: {n} and {y.shape[0]}")
    if n < 1 or n > MAX_POINTS:
        raise ValueError(f"the regressor takes 1 to {MAX_POINTS} training points, got {n}")
    c, s, l, nz = (_scalar(constant, "constant"), _scalar(outputscale, "outputscale"), _scalar(lengthscale, "lengthscale"),
                   _scalar(noise, "noise"))
    if not (s > 0.0 and l > 0.0 and nz > 0.0):
        raise ValueError("outputscale, lengthscale and noise must be > 0")
    d = x[:, None] - x[None, :]
    if n <= _NUMPY_SOLVE_MAX:
        K = s * np.exp(-(d * d) / (2.0 * l * l)) + nz * np.eye(n)
    else:                                                # the same values, built in place: one N x N array instead of four
        np.multiply(d, d, out=d)
        np.negative(d, out=d)
        np.divide(d, 2.0 * l * l, out=d)
        np.exp(d, out=d)
        np.multiply(d, s, out=d)
        d[np.diag_indices(n)] += nz
        K = d
    del d
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"k(x, x) + noise I is not numerically positive definite (no jitter is added): {e}") from None
    del K
    if n <= _NUMPY_SOLVE_MAX:
        linv = np.tril(np.linalg.solve(L, np.eye(n)))
    else:                                                # N^3 / 3 instead of a general solve's LU of L
        linv = torch.linalg.solve_triangular(torch.from_numpy(L), torch.eye(n, dtype=torch.float64), upper=False).numpy()
        del L
        linv = np.tril(linv)
    alpha = linv.T @ (linv @ (y - c))
    if not (np.isfinite(linv).all() and np.isfinite(alpha).all()):
        raise ValueError("the factorisation of k(x, x) + noise I overflowed")
    return x, alpha, np.ascontiguousarray(linv)


def _softplus(v: float) -> float:
    return float(np.logaddexp(0.0, v))


def _train_pair(train_x, train_y) -> Tuple[np.ndarray, np.ndarray]:
    x, y = _vector(train_x, "train_x"), _vector(train_y, "train_y")
    n = x.shape[0]
    if y.shape[0] != n:
        raise ValueError(f"train_x and train_y differ in length: {n} and {y.shape[0]}")
    if n < 1 or n > MAX_POINTS:
        raise ValueError(f"the regressor takes 1 to {MAX_POINTS} training points, got {n}")
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def _check_fit(lib, code: int):
    if code == _capi.BN_ERR_STATE:
        raise ValueError(lib.bn_gp_fit_last_error().decode("utf-8", "replace"))
    check(lib, "gp_fit", code)


class _Fit(Handle):
    """One bn_gp_fit_t: the device workspace of a fit (two N x N float64 buffers), released on exit.  Launches go to torch's
    current stream of the device."""
    family = "gp_fit"
    handle = property(lambda self: self._handle)

    def __init__(self, lib, dev: torch.device, x: np.ndarray, y: np.ndarray, noise_lower_bound: float) -> None:
        self._lib, self.dev = lib, dev
        h = C.c_void_p()
        self._check(lib.bn_gp_fit_create(dev.index, x.shape[0], x.ctypes.data, y.ctypes.data, float(noise_lower_bound), C.byref(h)))
        self._handle = h

    def _check(self, code: int) -> None:
        _check_fit(self._lib, code)

    def set_raw(self, raw) -> None:
        r = np.ascontiguousarray(raw, dtype=np.float64)
        self._check(self._lib.bn_gp_fit_set_raw(self._handle, r.ctypes.data))

    def evaluate(self) -> None:
        self._check(self._lib.bn_gp_fit_evaluate_async(self._handle, stream_ptr(self.dev)))

    def run(self, iterations: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
        self._check(self._lib.bn_gp_fit_run_async(self._handle, stream_ptr(self.dev), int(iterations), lr, beta1, beta2, eps))

    def read(self):
        """(raw (4,), grad (4,), loss, status, failed iteration) after a synchronisation"""
        raw, grad = np.zeros(4), np.zeros(4)
        loss, status, failed = C.c_double(), C.c_int32(), C.c_int32()
        self._check(self._lib.bn_gp_fit_read(self._handle, raw.ctypes.data, grad.ctypes.data, C.byref(loss), C.byref(status), C.byref(failed)))
        return raw, grad, loss.value, status.value, failed.value

    def hyperparameters(self):
        hyp = np.zeros(4)
        self._check(self._lib.bn_gp_fit_hyperparameters(self._handle, hyp.ctypes.data))
        return tuple(float(v) for v in hyp)

    def history(self) -> np.ndarray:
        done = self._lib.bn_gp_fit_history(self._handle, None, 0)
        self._check(done)
        out = np.zeros(done)
        if done:
            self._lib.bn_gp_fit_history(self._handle, out.ctypes.data, done)
        return out

    def finish(self) -> C.c_void_p:
        g = C.c_void_p()
        self._check(self._lib.bn_gp_fit_finish(self._handle, stream_ptr(self.dev), C.byref(g)))
        return g


class GPSlipRegressor(Handle):
    """One terrain class's slip regressor on the device: `.predict(slopes)` is GPModel.predict's `likelihood(model(x))`, exact.

    train_x, train_y: (N,) or (N, 1), used as float32 values; constant, outputscale, lengthscale, noise: the ACTUAL (not raw)
    hyperparameters.  Raises ValueError for invalid inputs and RuntimeError without a GPU (no CPU fallback)."""

    family = "gp"
    raw_parameters = None                # (constant, raw_outputscale, raw_lengthscale, raw_noise) float64 after fit(), else None
    loss_history = None                  # float64, one loss per iteration, after fit()
    noise_lower_bound = _NOISE_LOWER_BOUND

    def __init__(self, train_x, train_y, constant: float, outputscale: float, lengthscale: float, noise: float, device=None,
                 factorization: str = "host") -> None:
        """factorization="host" (the default): gp.factorize on the host and an upload of L^-1.  "device": the same
        hyperparameters factorised by the fit kernels, no N x N host array and no upload of L^-1."""
        if factorization not in ("host", "device"):
            raise ValueError(f'factorization must be "host" or "device", got {factorization!r}')
        self._handle = None
        if factorization == "device":
            x, y = _train_pair(train_x, train_y)
            c, s, l, nz = (_scalar(constant, "constant"), _scalar(outputscale, "outputscale"), _scalar(lengthscale, "lengthscale"),
                           _scalar(noise, "noise"))
            if not (s > 0.0 and l > 0.0 and nz > 0.0):
                raise ValueError("outputscale, lengthscale and noise must be > 0")
            self.num_points = int(x.shape[0])
            self.constant, self.outputscale, self.lengthscale, self.noise = c, s, l, nz
            self._open(device)
            with _Fit(self._lib, self._dev, x, y, _NOISE_LOWER_BOUND) as fit:
                fit._check(self._lib.bn_gp_fit_set_hyperparameters(fit.handle, c, s, l, nz))
                self._handle = fit.finish()
            return
        x, alpha, linv = factorize(train_x, train_y, constant, outputscale, lengthscale, noise)
        self.num_points = int(x.shape[0])
        self.constant, self.outputscale, self.lengthscale, self.noise = (_scalar(constant, "constant"), _scalar(outputscale, "outputscale"),
                                                                         _scalar(lengthscale, "lengthscale"), _scalar(noise, "noise"))
        self._open(device)
        h = C.c_void_p()
        self._check(self._lib.bn_gp_create(self._dev.index, self.num_points, x.ctypes.data, alpha.ctypes.data, linv.ctypes.data,
                                           self.constant, self.outputscale, self.lengthscale, self.noise, C.byref(h)))
        self._handle = h

    def _open(self, device) -> None:
        self._dev = resolve_device(device, "gp")
        self._lib = _capi.load()

    @classmethod
    def fit(cls, train_x, train_y, learning_rate: float = 0.1, num_iterations: int = 100, device=None, initial_raw=None,
            noise_lower_bound: float = _NOISE_LOWER_BOUND) -> "GPSlipRegressor":
        """RegressorTrainer.train (regressor_trainer.py:128-170) on the device: num_iterations steps of Adam (torch.optim.Adam's
        defaults, learning_rate) on the exact negative marginal log-likelihood over N in float64, from initial_raw = (constant,
        raw_outputscale, raw_lengthscale, raw_noise) (default: gpytorch's zeros), enqueued without a host round trip; then the
        factorisation at the final parameters.  The result carries .raw_parameters and .loss_history (the loss BEFORE each
        step).  A factorisation that fails raises ValueError with the iteration: no jitter is added."""
        x, y = _train_pair(train_x, train_y)
        n_it = int(num_iterations)
        if n_it < 0:
            raise ValueError("num_iterations must be >= 0")
        if not (float(learning_rate) > 0.0 and np.isfinite(float(learning_rate))):
            raise ValueError("learning_rate must be finite and > 0")
        raw0 = np.zeros(4) if initial_raw is None else np.ascontiguousarray(np.asarray(initial_raw, dtype=np.float64).reshape(-1))
        if raw0.shape != (4,) or not np.isfinite(raw0).all():
            raise ValueError("initial_raw must hold four finite values: constant, raw_outputscale, raw_lengthscale, raw_noise")
        self = cls.__new__(cls)
        self._handle = None
        self.num_points = int(x.shape[0])
        self.noise_lower_bound = float(noise_lower_bound)
        self._open(device)
        with _Fit(self._lib, self._dev, x, y, self.noise_lower_bound) as fit:
            fit.set_raw(raw0)
            fit.run(n_it, float(learning_rate))
            raw, _, _, status, failed = fit.read()
            if status:
                raise ValueError(f"k(x, x) + noise I is not numerically positive definite at iteration {failed} (no jitter is added)")
            self.raw_parameters = raw
            self.loss_history = fit.history()
            self.constant, self.outputscale, self.lengthscale, self.noise = fit.hyperparameters()
            self._handle = fit.finish()
        return self

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The fitted raw parameters in gpytorch's key layout as float32 tensors, for the reference's load_slip_regressors and
        this module's hyperparameters_from_state_dict.  The layout is gpytorch's as documented; it has not been checked against
        gpytorch itself.  Only a regressor that came from fit() has raw parameters."""
        if self.raw_parameters is None:
            raise ValueError("this regressor was built from actual hyperparameters: it has no raw parameters to save")
        c, ro, rl, rn = (float(v) for v in self.raw_parameters)
        return {"likelihood.noise_covar.raw_noise": torch.tensor([rn], dtype=torch.float32),
                "likelihood.noise_covar.raw_noise_constraint.lower_bound": torch.tensor(self.noise_lower_bound, dtype=torch.float32),
                "likelihood.noise_covar.raw_noise_constraint.upper_bound": torch.tensor(float("inf"), dtype=torch.float32),
                "mean_module.raw_constant": torch.tensor(c, dtype=torch.float32),
                "covar_module.raw_outputscale": torch.tensor(ro, dtype=torch.float32),
                "covar_module.base_kernel.raw_lengthscale": torch.tensor([[rl]], dtype=torch.float32)}

    @classmethod
    def from_gpytorch_state_dict(cls, state_dict, train_x, train_y, device=None, noise_lower_bound: Optional[float] = None) -> "GPSlipRegressor":
        return cls(train_x, train_y, device=device, **hyperparameters_from_state_dict(state_dict, noise_lower_bound))

    def to(self, device) -> "GPSlipRegressor":
        """The reference moves its regressors with .to(device); this one lives where it was created."""
        if torch.device(device).type == "cuda" and torch.device(device).index in (None, self._dev.index):
            return self
        raise ValueError(f"this regressor lives on {self._dev}; create another one for {device}")

    def predict_tensors(self, x: torch.Tensor, dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
        flat = x.reshape(1, -1)
        if flat.numel() == 0:
            e = torch.empty(x.shape, device=self._dev, dtype=dtype)
            return e, e.clone()
        cls_map = torch.zeros(flat.shape, device=self._dev, dtype=torch.int32)
        mean, std = _predict(self._lib, self._dev, [self], flat, cls_map, dtype)
        return mean.reshape(x.shape), std.reshape(x.shape)

    def predict(self, x: torch.Tensor) -> Normal:
        """Normal(mean, std) of x's shape: the `.mean` / `.stddev` surface of GPModel.predict, noise included."""
        return Normal(*self.predict_tensors(x))


def hyperparameters_from_state_dict(state_dict, noise_lower_bound: Optional[float] = None) -> Dict[str, float]:
    """The actual hyperparameters of a GPModel.state_dict() as regressor_trainer.py:172-200 saves it, read without gpytorch:
    noise = softplus(likelihood.noise_covar.raw_noise) + the stored lower bound (default 1e-4), outputscale and lengthscale =
    softplus of covar_module.raw_outputscale / covar_module.base_kernel.raw_lengthscale, constant = mean_module.raw_constant
    (gpytorch >= 1.9) or the older mean_module.constant."""
    def get(*names):
        for n in names:
            if n in state_dict:
                return _scalar(state_dict[n], n)
        raise ValueError(f"the state dict has none of {names}")
    lb = noise_lower_bound
    if lb is None:
        key = "likelihood.noise_covar.raw_noise_constraint.lower_bound"
        lb = _scalar(state_dict[key], key) if key in state_dict else _NOISE_LOWER_BOUND
    return {"constant": get("mean_module.raw_constant", "mean_module.constant"),
            "outputscale": _softplus(get("covar_module.raw_outputscale")),
            "lengthscale": _softplus(get("covar_module.base_kernel.raw_lengthscale")),
            "noise": _softplus(get("likelihood.noise_covar.raw_noise")) + float(lb)}


def load_slip_regressors(num_terrain_classes: int, model_directory: str, train_data_directory: str, device=None) -> Dict[int, GPSlipRegressor]:
    """trainers/utils.py:65-108 on the reference's file layout: class i's training data from
    <train_data_directory>/slip_observations/<i:02d>_class.pth ({"train_x", "train_y"}) and its state dict from
    <model_directory>/models/<i:02d>_class.pth, both read with weights_only=True."""
    out = {}
    for i in range(int(num_terrain_classes)):
        data = torch.load(os.path.join(train_data_directory, f"slip_observations/{i:02d}_class.pth"), map_location="cpu", weights_only=True)
        state = torch.load(os.path.join(model_directory, f"models/{i:02d}_class.pth"), map_location="cpu", weights_only=True)
        out[i] = GPSlipRegressor.from_gpytorch_state_dict(state, data["train_x"], data["train_y"], device=device)
    return out


class SlipRegressorTrainer:
    """RegressorTrainer's interface and on-disk layout (trainers/regressor_trainer.py:22-200) around GPSlipRegressor.fit: plain
    host Python.  params_model_training: any object with .batch_size, .learning_rate and .num_iterations; train_dataset: any
    dataset that yields (slopes, slips, t_classes).  Class i's regressor goes to
    <model_directory>/lr<lr:.0e>_iters<n:03d>/models/<i:02d>_class.pth (GPSlipRegressor.state_dict()) and its observations to
    <data_directory>/slip_observations/<i:02d>_class.pth ({"train_x", "train_y"}); load_slip_regressors(num_terrain_classes,
    trainer.model_directory, data_directory) reads both back."""

    def __init__(self, device, model_directory: str, data_directory: str, num_terrain_classes: int, params_model_training, train_dataset) -> None:
        from torch.utils.data import DataLoader
        self.device = device
        self.train_dataset = train_dataset
        self.train_loader = DataLoader(train_dataset, batch_size=params_model_training.batch_size, shuffle=True)
        self.num_terrain_classes = int(num_terrain_classes)
        self.params_model_training = params_model_training
        self.model_directory = os.path.join(model_directory, f"lr{params_model_training.learning_rate:.0e}_iters{params_model_training.num_iterations:03d}")
        self.learned_models_directory = os.path.join(self.model_directory, "models")
        self.data_directory = os.path.join(data_directory, "slip_observations")
        os.makedirs(self.learned_models_directory, exist_ok=True)
        os.makedirs(self.data_directory, exist_ok=True)
        self.regressors: Dict[int, GPSlipRegressor] = {}

    def train_all_models(self) -> None:
        phis, slips = self.load_data()
        for k in range(self.num_terrain_classes):
            self.train(k, phis[k], slips[k])

    def load_data(self, num_samples: int = 9999, order=None) -> Tuple[Dict[int, torch.Tensor], Dict[int, torch.Tensor]]:
        """Per class the slopes and slips of its cells in the loader's order, cut at num_samples.

        A dataset with `gather_observations` (dataset.SlipRegressionDataset) is gathered on the device in one call instead: the
        maps are visited in `order` (a permutation of the maps; default torch.randperm(len(dataset)) from torch's global
        generator).  That is a shuffled order, but not the order DataLoader(shuffle=True) would have visited them in under the
        same seed (its sampler draws a seed first).  Every other dataset goes through the loader, and `order` must stay None."""
        if hasattr(self.train_dataset, "gather_observations"):
            if order is None:
                order = torch.randperm(len(self.train_dataset))
            phis, slips, _, totals = self.train_dataset.gather_observations(self.num_terrain_classes, num_samples, order=order)
            for k in range(self.num_terrain_classes):
                if int(totals[k]) == 0:
                    raise ValueError(f"the dataset holds no cell of terrain class {k}")
            return phis, slips
        if order is not None:
            raise ValueError("order= applies to datasets with gather_observations; this one is read through its DataLoader")
        phis = {k: [] for k in range(self.num_terrain_classes)}
        slips = {k: [] for k in range(self.num_terrain_classes)}
        for slope_b, slip_b, class_b in self.train_loader:
            for k in range(self.num_terrain_classes):
                sel = class_b == k
                if bool(sel.any()):
                    phis[k].append(slope_b[sel])
                    slips[k].append(slip_b[sel])
        for k in range(self.num_terrain_classes):
            if not phis[k]:
                raise ValueError(f"the dataset holds no cell of terrain class {k}")
            phis[k] = torch.cat(phis[k], dim=0)[:num_samples]
            slips[k] = torch.cat(slips[k], dim=0)[:num_samples]
        return phis, slips

    def train(self, terrain_class: int, phis: torch.Tensor, slips: torch.Tensor) -> GPSlipRegressor:
        p = self.params_model_training
        model = GPSlipRegressor.fit(phis, slips, learning_rate=p.learning_rate, num_iterations=p.num_iterations, device=self.device)
        self.regressors[int(terrain_class)] = model
        self.save(phis, slips, model, terrain_class)
        return model

    def save(self, train_x: torch.Tensor, train_y: torch.Tensor, model: GPSlipRegressor, terrain_class: int) -> None:
        torch.save({"train_x": train_x, "train_y": train_y}, os.path.join(self.data_directory, f"{terrain_class:02d}_class.pth"))
        torch.save(model.state_dict(), os.path.join(self.learned_models_directory, f"{terrain_class:02d}_class.pth"))


def _predict(lib, dev: torch.device, table, slopes: torch.Tensor, classes: torch.Tensor, dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """bn_gp_predict_async on torch's current stream: slopes and classes (B, cells) -> mean, std (B, cells)."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be torch.float32 or torch.float64")
    B, cells = slopes.shape
    nc = len(table)
    with torch.cuda.device(dev):
        s = slopes.detach().to(dev, torch.float32).contiguous()
        c = classes.detach().to(dev, torch.int32).contiguous()
        mean = torch.empty(B, cells, device=dev, dtype=dtype)
        std = torch.empty(B, cells, device=dev, dtype=dtype)
        nbytes = lib.bn_gp_workspace_bytes(B, cells, nc)
        if nbytes == 0:
            raise ValueError(f"{B} maps of {cells} cells with {nc} classes are out of the library's range")
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)     # torch's allocator keeps it alive for the stream
        handles = (C.c_void_p * nc)(*[(r._handle.value if r is not None else None) for r in table])
        check(lib, "gp", lib.bn_gp_predict_async(dev.index, stream_ptr(dev), handles, nc, B, cells, C.c_void_p(s.data_ptr()),
                                            C.c_void_p(c.data_ptr()), C.c_void_p(mean.data_ptr()), C.c_void_p(std.data_ptr()),
                                            1 if dtype == torch.float64 else 0, C.c_void_p(work.data_ptr()), nbytes))
    return mean, std


class TraversabilityPredictor:
    """classifier_and_regressor.py's TraversabilityPredictor on the device.

    terrain_classifier: unet.TerrainClassifier (the reference's UNet on the device: it has `batched = True`, and predict_maps
    classifies the whole batch in one call and hands the int32 device class maps straight to the GP kernels), or any other
    object with `.predict(colors[None]) -> (1, G, G)` integer classes, called map by map, or None when the class maps are passed
    to predict_maps.  slip_regressors: {class: GPSlipRegressor}; a class without one predicts mean 0 and std 0 (the reference's
    zeros_like)."""

    def __init__(self, terrain_classifier, slip_regressors: Dict[int, GPSlipRegressor], device=None) -> None:
        self.device = resolve_device(device, "gp")
        self.terrain_classifier = terrain_classifier.to(self.device) if hasattr(terrain_classifier, "to") else terrain_classifier
        self.slip_regressors = {int(k): r.to(self.device) for k, r in slip_regressors.items()}
        if any(k < 0 or k >= MAX_CLASSES for k in self.slip_regressors):
            raise ValueError(f"terrain classes must be in [0, {MAX_CLASSES})")
        n = max(self.slip_regressors, default=0) + 1
        self._table = [self.slip_regressors.get(k) for k in range(n)]
        self._lib = _capi.load()

    def predict_maps(self, slopes: torch.Tensor, t_classes: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None,
                     dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean, std) of slopes' shape, (G, G) or (B, G, G), in one call of two or three launches (the bucketing, then one
        predict kernel for the regressors of up to 1024 points and one for the larger ones) without a host round trip.  t_classes of the same shape skips the
        classifier; otherwise colors (3, G, G) or (B, 3, G, G) goes through it: in one call when it is `batched`, else map by map."""
        if slopes.dim() not in (2, 3):
            raise ValueError(f"slopes must be (G, G) or (B, G, G), got {tuple(slopes.shape)}")
        batched = slopes.dim() == 3
        s = slopes if batched else slopes[None]
        if t_classes is None:
            if self.terrain_classifier is None or colors is None:
                raise ValueError("pass t_classes, or colors and a terrain classifier")
            col = (colors if batched else colors[None]).to(self.device)
            if col.shape[0] != s.shape[0]:
                raise ValueError("colors and slopes differ in batch size")
            if getattr(self.terrain_classifier, "batched", False):   # unet.TerrainClassifier: one call, int32 classes on the device
                t_classes = self.terrain_classifier.predict_classes(col).reshape(s.shape)
            else:
                t_classes = torch.cat([torch.as_tensor(self.terrain_classifier.predict(col[b:b + 1])).reshape(1, *s.shape[1:])
                                       for b in range(s.shape[0])])
        else:
            t_classes = t_classes if batched else t_classes[None]
        if tuple(t_classes.shape) != tuple(s.shape):
            raise ValueError(f"t_classes {tuple(t_classes.shape)} and slopes {tuple(s.shape)} differ in shape")
        B = s.shape[0]
        mean, std = _predict(self._lib, self.device, self._table, s.reshape(B, -1), t_classes.reshape(B, -1), dtype)
        return mean.reshape(slopes.shape), std.reshape(slopes.shape)

    def predict(self, colors: torch.Tensor, slopes: torch.Tensor) -> Normal:
        """The reference's predict: colors (3, G, G), slopes (G, G) -> Normal(mean (G, G), std (G, G)).  As there, a map with a
        cell whose class has no regressor has std 0 and Normal's argument check raises."""
        return Normal(*self.predict_maps(slopes, colors=colors))
