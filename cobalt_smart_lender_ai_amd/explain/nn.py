"""Per-applicant reasons for the MLP challenger: integrated gradients averaged over a background set.

``MLPExplainer(model, data=Z, model_output="probability")`` is the network's counterpart of
``TreeExplainer(clf, data=Z, model_output="probability")``: attributions against a background set with
``sum(phi) + expected_value = f(x)`` up to the quadrature error, which :meth:`MLPExplainer.convergence_delta`
reports. For a row ``x``, background rows ``z_1..z_B`` and ``M`` steps, ``alpha_m = (m + 1/2) / M``::

    phi[i] = 1/B sum_b (x[i] - z_b[i]) 1/M sum_m dF/dx_i (z_b + alpha_m (x - z_b))
    expected_value = 1/B sum_b F(z_b)

``F`` is the logit (``"raw"``) or its sigmoid (``"probability"``); the ReLU derivative at 0 is 0. This is the
deterministic form of SHAP's "expected gradients". On the GPU the ``N x B x M`` forward and input-gradient
passes run in ``csrc/mlp_ig.hip`` (fp32 MFMA, fp64 sums in a fixed order); :func:`integrated_gradients_host`
is the float64 definition and the CPU path.
"""
from __future__ import annotations

import numpy as np
import torch

from ..nn import mlp
from .shap import Explanation

MODEL_OUTPUTS = ("raw", "probability")
_HOST_POINTS = 1 << 16  # quadrature points per host chunk


def _weights(params, F: int) -> dict[str, np.ndarray]:
    p = np.asarray(params, dtype=np.float64).reshape(-1)
    if p.size != mlp.num_params(F):
        raise ValueError(f"params has {p.size} elements, a network of {F} inputs has {mlp.num_params(F)}")
    return {k: p[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in mlp.layout(F).items()}


def _preactivations(w: dict[str, np.ndarray], pts: np.ndarray):
    """Pre-activations of the three hidden layers and the logit at float64 points [..., F]."""
    a1 = pts @ w["W1"] + w["b1"]
    a2 = np.maximum(a1, 0.0) @ w["W2"] + w["b2"]
    a3 = np.maximum(a2, 0.0) @ w["W3"] + w["b3"]
    return a1, a2, a3, np.maximum(a3, 0.0) @ w["W4"] + w["b4"][0]


def _sigmoid(z: np.ndarray) -> np.ndarray:
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def model_output_host(params, X, model_output: str = "raw") -> np.ndarray:
    """``F(x)`` in float64: the logit, or its sigmoid."""
    X = np.asarray(X, dtype=np.float64)
    z = _preactivations(_weights(params, X.shape[1]), X)[3]
    return _sigmoid(z) if model_output == "probability" else z


def integrated_gradients_host(params, X, Z, n_steps: int, model_output: str = "raw",
                              return_gate_margin: bool = False):
    """The definition in float64 (closed-form backward through the three gated layers): ``phi`` [N, F].

    ``return_gate_margin``: also the smallest ``|pre-activation|`` of any hidden unit over every step and
    background row, per explained row [N] -- the gradient jumps where a pre-activation crosses 0, so a
    lower-precision evaluation can only be held to this one where the margin exceeds its forward error."""
    if model_output not in MODEL_OUTPUTS:
        raise ValueError(f"model_output must be one of {MODEL_OUTPUTS}, got {model_output!r}")
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    if X.ndim != 2 or Z.ndim != 2 or X.shape[1] != Z.shape[1]:
        raise ValueError(f"X {X.shape} and Z {Z.shape} must be matrices with the same number of columns")
    N, F = X.shape
    B, M = Z.shape[0], int(n_steps)
    if B < 1:
        raise ValueError("the background set is empty")
    if M < 1:
        raise ValueError(f"n_steps must be >= 1, got {n_steps}")
    w = _weights(params, F)
    alpha = (np.arange(M, dtype=np.float64) + 0.5) / M
    phi = np.zeros((N, F))
    margin = np.full(N, np.inf)
    rows = max(1, _HOST_POINTS // (B * M))
    for r0 in range(0, N, rows):
        x = X[r0:r0 + rows]
        d = x[:, None, :] - Z[None, :, :]                                          # [n, B, F]
        pts = Z[None, :, None, :] + alpha[None, None, :, None] * d[:, :, None, :]  # [n, B, M, F]
        a1, a2, a3, z = _preactivations(w, pts)
        d3 = (a3 > 0) * w["W4"]
        d2 = (d3 @ w["W3"].T) * (a2 > 0)
        d1 = (d2 @ w["W2"].T) * (a1 > 0)
        g = d1 @ w["W1"].T                                                         # [n, B, M, F]
        if model_output == "probability":
            p = _sigmoid(z)
            g = g * (p * (1.0 - p))[..., None]
        phi[r0:r0 + rows] = (d * g.mean(axis=2)).mean(axis=1)
        if return_gate_margin:
            margin[r0:r0 + rows] = np.minimum.reduce([np.abs(a).min(axis=(1, 2, 3)) for a in (a1, a2, a3)])
    return (phi, margin) if return_gate_margin else phi


class MLPExplainer:
    """``MLPExplainer(model, data, model_output="raw", n_steps=32, device=None)`` for an :class:`MLPModel`.

    ``shap_values(X)``: float64 [N, F] integrated gradients against the background rows ``data`` (a CUDA
    tensor in gives a CUDA tensor out, anything else NumPy), ``expected_value``: the mean model output over
    the background, ``convergence_delta(X)``: ``sum(phi) + expected_value - f(x)`` per row, the quadrature
    error of ``n_steps`` midpoint steps. Runs on the GPU when there is one (``device="cpu"``: the float64
    host definition)."""

    def __init__(self, model, data, model_output: str = "raw", n_steps: int = 32, device=None):
        if not isinstance(model, mlp.MLPModel):
            raise TypeError("expected an MLPModel")
        if model_output not in MODEL_OUTPUTS:
            raise ValueError(f"model_output must be one of {MODEL_OUTPUTS}, got {model_output!r}")
        if int(n_steps) < 1:
            raise ValueError(f"n_steps must be >= 1, got {n_steps}")
        self.model = model
        self.model_output = model_output
        self.n_steps = int(n_steps)
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        F = model.n_features
        self.feature_names = list(model.feature_names or [f"f{i}" for i in range(F)])
        if self.device.type == "cuda" and self.n_steps > mlp.MAX_IG_STEPS:
            raise ValueError(f"n_steps must be <= {mlp.MAX_IG_STEPS} on the GPU, got {n_steps}")
        self.data = self._tensor(data)
        if self.data.shape[0] < 1:
            raise ValueError("the background set is empty")
        if self.device.type == "cuda":
            self._params = torch.as_tensor(np.ascontiguousarray(model.params, dtype=np.float32), device=self.device)
        self.expected_value = float(self._output(self.data).mean())

    def _tensor(self, X) -> torch.Tensor:
        """``X`` as a float32 [N, F] tensor on the explainer's device (unit column stride; a CUDA view keeps
        its row stride); a DataFrame's columns are reordered by feature name."""
        names = self.model.feature_names
        if hasattr(X, "columns") and names:
            X = X[names]
        if hasattr(X, "to_numpy"):
            X = X.to_numpy(dtype=np.float32)
        t = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X, dtype=np.float32))
        if t.dim() != 2 or t.shape[1] != self.model.n_features:
            raise ValueError(f"expected [N, {self.model.n_features}] rows, got {tuple(t.shape)}")
        t = t.to(self.device, torch.float32)
        return t if t.shape[0] == 0 or t.stride(1) == 1 else t.contiguous()

    def _output(self, Xt: torch.Tensor) -> torch.Tensor:
        """Float64 ``F(x)`` of the rows of a tensor from :meth:`_tensor`, on its device."""
        if Xt.shape[0] == 0:
            return torch.zeros(0, dtype=torch.float64, device=Xt.device)
        if self.device.type == "cuda":
            prob = torch.empty(Xt.shape[0], dtype=torch.float32, device=self.device)
            logit = torch.empty_like(prob)
            mlp.mlp_forward_gpu(Xt, self._params, prob, logit)
            z = logit.to(torch.float64)
            return torch.sigmoid(z) if self.model_output == "probability" else z
        return torch.as_tensor(model_output_host(self.model.params, Xt.numpy(), self.model_output))

    def _values(self, Xt: torch.Tensor) -> torch.Tensor:
        if self.device.type == "cuda":
            phi = torch.empty((Xt.shape[0], self.model.n_features), dtype=torch.float64, device=self.device)
            mlp.mlp_ig_gpu(Xt, self.data, self._params, phi, self.n_steps, self.model_output == "probability")
            return phi
        return torch.as_tensor(integrated_gradients_host(self.model.params, Xt.numpy(), self.data.numpy(),
                                                         self.n_steps, self.model_output))

    @staticmethod
    def _like(X, t: torch.Tensor):
        return t.to(X.device) if isinstance(X, torch.Tensor) and X.is_cuda else t.cpu().numpy()

    def shap_values(self, X):
        return self._like(X, self._values(self._tensor(X)))

    def convergence_delta(self, X):
        Xt = self._tensor(X)
        return self._like(X, self._values(Xt).sum(dim=1) + self.expected_value - self._output(Xt))

    def __call__(self, X) -> Explanation:
        vals = self.shap_values(X)
        vals = vals.cpu().numpy() if isinstance(vals, torch.Tensor) else vals
        data = X.to_numpy(dtype=np.float64) if hasattr(X, "to_numpy") else np.asarray(
            X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else X, np.float64)
        return Explanation(vals, np.full(len(vals), self.expected_value), data, self.feature_names)
