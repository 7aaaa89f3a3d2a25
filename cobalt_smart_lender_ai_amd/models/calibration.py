"""Calibrators of a binary classifier's score, fitted on the MARGIN (monotone in the probability, and without the
ties float32 sigmoid saturation makes): isotonic regression, Platt's sigmoid, and the analytic prior correction.

``IsotonicCalibrator`` and ``PlattCalibrator`` are what ``CalibratedClassifierCV(method="isotonic" | "sigmoid")``
fits on one held-out set; ``PriorShiftCalibrator`` undoes ``scale_pos_weight`` on the odds and needs no data.
CUDA tensors are fitted and transformed on their device (``csrc/calib.hip`` for the isotonic hull and the apply,
fp64 torch reductions for Platt's Newton steps); NumPy arrays take the host path with the same results.
``metrics.calibration`` holds the definitions.
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np
import torch

from ..metrics import calibration as C

CALIBRATION_FILE = "calibration.json"


def _is_cuda(x) -> bool:
    return isinstance(x, torch.Tensor) and x.is_cuda


def _like(out32: np.ndarray, ref):
    return torch.from_numpy(out32) if isinstance(ref, torch.Tensor) else out32


class _Calibrator:
    method = ""

    def transform(self, margin):
        raise NotImplementedError

    def to_dict(self) -> dict:
        raise NotImplementedError

    def save(self, path) -> Path:
        """Write ``calibration.json`` (``path`` is that file, or the model's directory)."""
        p = Path(path)
        if p.is_dir():
            p = p / CALIBRATION_FILE
        p.write_text(json.dumps(self.to_dict()))
        return p


class IsotonicCalibrator(_Calibrator):
    """Isotonic regression of the 0/1 labels on the margin; between knots it interpolates linearly and outside
    them it clips, as ``sklearn.isotonic.IsotonicRegression(out_of_bounds="clip")``. ``x_thresholds_`` (float32)
    and ``y_thresholds_`` (float64) are that estimator's ``X_thresholds_`` / ``y_thresholds_``."""
    method = "isotonic"

    def fit(self, margin, y, sample_weight=None) -> "IsotonicCalibrator":
        n = int(np.prod(tuple(margin.shape))) if hasattr(margin, "shape") else len(margin)
        wq = C.quantize_weights(sample_weight, n)
        if _is_cuda(margin) or _is_cuda(y):
            from ..ops import calib_ops

            xk, vk = calib_ops.iso_fit_gpu(margin, y, wq)
        else:
            xk, vk = C.iso_fit_host(margin, y, wq)
        self.x_thresholds_, self.y_thresholds_ = xk, vk
        self._dev = {}
        return self

    def transform(self, margin):
        """Calibrated probability, float32: a tensor on the margin's device for a tensor, else NumPy."""
        xk, vk = self.x_thresholds_, self.y_thresholds_
        if _is_cuda(margin):
            from ..ops import calib_ops

            key = str(margin.device)
            if key not in self._dev:
                self._dev[key] = (torch.from_numpy(xk).to(margin.device), torch.from_numpy(vk).to(margin.device))
            m = margin.reshape(-1).to(torch.float32).contiguous()
            return calib_ops.calib_apply(m, *self._dev[key])
        return _like(C.calib_apply_host(margin, xk, vk), margin)

    def to_dict(self) -> dict:
        # float32 knots and float64 values survive repr round trips exactly
        return {"method": self.method, "x_thresholds": [float(v) for v in self.x_thresholds_],
                "y_thresholds": [float(v) for v in self.y_thresholds_]}

    @classmethod
    def from_dict(cls, d: dict) -> "IsotonicCalibrator":
        c = cls()
        c.x_thresholds_, c.y_thresholds_ = C.check_knots(np.asarray(d["x_thresholds"], dtype=np.float32),
                                                         np.asarray(d["y_thresholds"], dtype=np.float64))
        c._dev = {}
        return c


class PlattCalibrator(_Calibrator):
    """``sigmoid(a * margin + b)`` fitted by Newton's method on the weighted log-loss against Platt's smoothed
    targets ``(N+ + 1) / (N+ + 2)`` and ``1 / (N- + 2)`` (``N+`` / ``N-``: the weight of the positives / negatives).
    Every sum is an fp64 torch reduction on the margin's device. The fit stops when
    ``max |gradient| / sum(w) <= tol`` (``converged_``); the objective is convex, so that certifies the optimum."""
    method = "sigmoid"

    def __init__(self, tol: float = 1e-10, max_iter: int = 100):
        self.tol, self.max_iter = float(tol), int(max_iter)

    def fit(self, margin, y, sample_weight=None) -> "PlattCalibrator":
        dev = next((t.device for t in (margin, y) if _is_cuda(t)), torch.device("cpu"))

        def on(x, dtype):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
            return t.reshape(-1).to(device=dev, dtype=dtype)

        m = on(margin, torch.float32).to(torch.float64)
        yv = on(y, torch.float64)
        n = int(m.shape[0])
        if n < 1:
            raise ValueError("empty input")
        if n > C.MAX_ROWS:
            raise ValueError(f"at most 2^28 rows ({n} given)")
        if yv.shape[0] != n:
            raise ValueError(f"{yv.shape[0]} labels, {n} scores")
        w = torch.ones(n, dtype=torch.float64, device=dev) if sample_weight is None else on(sample_weight, torch.float64)
        if w.shape[0] != n:
            raise ValueError(f"{w.shape[0]} weights, {n} rows")
        bad = torch.stack([((yv != 0) & (yv != 1)).any(), torch.isnan(m).any(),
                           (~torch.isfinite(w)).any() | (w < 0).any()]).cpu().tolist()
        if bad[0]:
            raise ValueError("labels must be 0 or 1")
        if bad[1]:
            raise ValueError("NaN scores")
        if bad[2]:
            raise ValueError("sample_weight must be finite and >= 0")
        sw = float(w.sum())
        if sw <= 0:
            raise ValueError("sample_weight has no positive entry")
        npos = float((w * yv).sum())
        nneg = sw - npos
        t = torch.full_like(yv, 1.0 / (nneg + 2.0))   # fp64 (torch.where on two Python floats gives float32)
        t[yv > 0] = (npos + 1.0) / (npos + 2.0)

        def loss_grad(a, b):
            z = a * m + b
            loss = float((w * (torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs())) - t * z)).sum())
            p = torch.sigmoid(z)
            r = w * (p - t)
            h = w * p * (1 - p)
            return loss, float((r * m).sum()), float(r.sum()), float((h * m * m).sum()), float((h * m).sum()), float(h.sum())

        a, b = 0.0, math.log((npos + 1.0) / (nneg + 1.0))
        loss, ga, gb, haa, hab, hbb = loss_grad(a, b)
        self.converged_ = False
        for it in range(self.max_iter + 1):
            if max(abs(ga), abs(gb)) / sw <= self.tol:
                self.converged_ = True
                break
            if it == self.max_iter:
                break
            ridge = 1e-12 * (haa + hbb) + 1e-300
            det = (haa + ridge) * (hbb + ridge) - hab * hab
            da = -((hbb + ridge) * ga - hab * gb) / det
            db = -((haa + ridge) * gb - hab * ga) / det
            step, slope = 1.0, ga * da + gb * db
            while True:
                cand = loss_grad(a + step * da, b + step * db)
                # accept a decrease, or, once the loss no longer resolves one, a smaller gradient
                if cand[0] <= loss + 1e-4 * step * slope or (
                        max(abs(cand[1]), abs(cand[2])) < max(abs(ga), abs(gb)) and cand[0] <= loss + 1e-12 * abs(loss)):
                    break
                step *= 0.5
                if step < 1e-10:
                    break
            if step < 1e-10:
                break
            a, b = a + step * da, b + step * db
            loss, ga, gb, haa, hab, hbb = cand
        self.a_, self.b_, self.n_iter_ = float(a), float(b), it
        return self

    def transform(self, margin):
        if isinstance(margin, torch.Tensor):
            z = margin.reshape(-1).to(torch.float32).to(torch.float64) * self.a_ + self.b_
            return torch.sigmoid(z).to(torch.float32)
        z = np.asarray(margin, dtype=np.float32).reshape(-1).astype(np.float64) * self.a_ + self.b_
        return torch.sigmoid(torch.from_numpy(z)).to(torch.float32).numpy()

    def to_dict(self) -> dict:
        return {"method": self.method, "a": self.a_, "b": self.b_}

    @classmethod
    def from_dict(cls, d: dict) -> "PlattCalibrator":
        c = cls()
        c.a_, c.b_ = float(d["a"]), float(d["b"])
        return c


class PriorShiftCalibrator(PlattCalibrator):
    """``sigmoid(margin - log(scale_pos_weight))``: a model trained with the positives weighted ``s`` times
    learns odds ``s`` times too high; dividing the odds by ``s`` is the exact inverse and needs no data."""
    method = "prior"

    def __init__(self, scale_pos_weight: float):
        s = float(scale_pos_weight)
        if not (math.isfinite(s) and s > 0):
            raise ValueError("scale_pos_weight must be positive and finite")
        self.scale_pos_weight = s
        self.a_, self.b_ = 1.0, -math.log(s)

    def fit(self, margin=None, y=None, sample_weight=None) -> "PriorShiftCalibrator":
        return self

    def to_dict(self) -> dict:
        return {"method": self.method, "scale_pos_weight": self.scale_pos_weight}

    @classmethod
    def from_dict(cls, d: dict) -> "PriorShiftCalibrator":
        return cls(d["scale_pos_weight"])


_METHODS = {c.method: c for c in (IsotonicCalibrator, PlattCalibrator, PriorShiftCalibrator)}


def from_dict(d: dict) -> _Calibrator:
    """The calibrator a ``to_dict()`` describes."""
    try:
        cls = _METHODS[d["method"]]
    except KeyError:
        raise ValueError(f"unknown calibration method {d.get('method')!r}; known: {', '.join(_METHODS)}") from None
    return cls.from_dict(d)


def load(path) -> _Calibrator:
    """Read ``calibration.json`` (``path`` is that file, or the model's directory)."""
    p = Path(path)
    if p.is_dir():
        p = p / CALIBRATION_FILE
    return from_dict(json.loads(p.read_text()))


def make_calibrator(method: str, scale_pos_weight: float | None = None) -> _Calibrator:
    if method == "isotonic":
        return IsotonicCalibrator()
    if method == "sigmoid":
        return PlattCalibrator()
    if method == "prior":
        if scale_pos_weight is None:
            raise ValueError("the prior correction needs scale_pos_weight")
        return PriorShiftCalibrator(scale_pos_weight)
    raise ValueError(f"unknown calibration method {method!r}; known: isotonic, sigmoid, prior")


class CalibratedModel:
    """A fitted classifier (``base``) with a calibrator on its margin. ``predict_proba`` returns ``[N, 2]``
    float32: a tensor on the device of a tensor input, else NumPy. The base model is not modified."""

    def __init__(self, base, calibrator: _Calibrator):
        self.base, self.calibrator = base, calibrator

    def _margin(self, X, iteration_range=None):
        b = self.base
        return b.get_booster().predict_margin(b._matrix(X), device=b.device, n_trees=b._n_trees(iteration_range))

    def predict_proba(self, X, iteration_range=None):
        p = self.calibrator.transform(self._margin(X, iteration_range))
        if isinstance(p, torch.Tensor):
            return torch.stack([1.0 - p, p], dim=1)
        return np.stack([1.0 - p, p], axis=1)

    def predict(self, X, iteration_range=None):
        p = self.predict_proba(X, iteration_range)[:, 1]
        pred = (p > 0.5).cpu().numpy().astype(np.int64) if isinstance(p, torch.Tensor) else (p > 0.5).astype(np.int64)
        classes = getattr(self.base, "classes_", None)
        return classes[pred] if classes is not None and len(classes) == 2 else pred

    def reliability(self, X, y, **kw):
        """``metrics.calibration.reliability_report`` of the calibrated probabilities on ``(X, y)``."""
        p = self.predict_proba(X)[:, 1]
        return C.reliability_report(self.base._binary_labels(y), p.contiguous() if isinstance(p, torch.Tensor) else p, **kw)
