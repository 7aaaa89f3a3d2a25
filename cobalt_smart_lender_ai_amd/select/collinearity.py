"""Which features are redundant with each other: the correlation matrix with missing values, variance inflation
factors and a greedy screen.

Scorecard practice screens the characteristics on ``|r|`` and VIF before the logistic regression, keeping of two
collinear ones the one with the higher information value; RFE and permutation importance split credit arbitrarily
between near-duplicates, so the same screen in front of them shortens the search and makes its result stable::

    iv = {r["feature"]: r["iv"] for r in information_value(X, y, feature_names=names)}
    rep = correlation_matrix(X, names, "spearman")
    keep = drop_correlated(rep, 0.7, priority=[iv[f] for f in names]).kept

The moments come from ``ops.corr_ops.pair_moments``: one pass of ``csrc/corr.hip`` over a CUDA tensor, NumPy
otherwise. More than 128 columns in one call are refused on the GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np
import torch

from ..ops import corr_ops

METHODS = ("pearson", "spearman")
MISSING = ("pairwise", "listwise")


def _matrix(X, feature_names):
    """``(X as a CUDA tensor or a NumPy array, names)``; a DataFrame gives its numeric columns as float64 and their
    names, as ``prep.eda.describe`` takes them."""
    try:
        import pandas as pd
    except ImportError:  # pragma: no cover
        pd = None
    if pd is not None and isinstance(X, pd.DataFrame):
        from ..prep import frame

        cols = frame.numeric_columns(X)
        if feature_names is not None and list(feature_names) != cols:
            raise ValueError("feature_names must be None or the numeric columns of the DataFrame")
        a = np.empty((len(X), len(cols)), dtype=np.float64)
        for i, c in enumerate(cols):
            a[:, i] = X[c].to_numpy(dtype=np.float64, na_value=np.nan)
        return a, cols
    if isinstance(X, torch.Tensor):
        if X.dim() != 2:
            raise ValueError(f"X must be [rows, features], got {tuple(X.shape)}")
        if X.device.type != "cuda":
            X = X.detach().numpy()
    else:
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError(f"X must be [rows, features], got {X.shape}")
    F = X.shape[1]
    names = [f"f{i}" for i in range(F)] if feature_names is None else [str(s) for s in feature_names]
    if len(names) != F:
        raise ValueError(f"{F} columns need {F} feature names, got {len(names)}")
    return X, names


@dataclass
class CorrelationReport:
    """``r`` float64 ``[F, F]`` (NaN where undefined, bitwise symmetric), ``n`` int64 ``[F, F]`` (the rows each pair
    was computed on), ``names`` and ``method``."""
    r: np.ndarray
    n: np.ndarray
    names: list[str]
    method: str = "pearson"

    def pairs(self, threshold: float = 0.7) -> list[dict[str, Any]]:
        """The pairs ``i < j`` with ``|r| >= threshold``, sorted by ``|r|`` descending, ties by index."""
        F = len(self.names)
        out = []
        for i in range(F):
            for j in range(i + 1, F):
                v = float(self.r[i, j])
                if np.isfinite(v) and abs(v) >= threshold:
                    out.append((-abs(v), i, j, v))
        out.sort(key=lambda t: t[:3])
        return [{"a": self.names[i], "b": self.names[j], "r": v, "n": int(self.n[i, j])} for _, i, j, v in out]

    def to_frame(self):
        import pandas as pd

        return pd.DataFrame(self.r, index=list(self.names), columns=list(self.names))

    def to_dict(self) -> dict[str, Any]:
        """JSON-ready (NaN as ``None``); ``from_dict`` gives the report back."""
        r = [[None if not np.isfinite(v) else float(v) for v in row] for row in self.r]
        return {"method": self.method, "names": list(self.names), "r": r, "n": self.n.astype(np.int64).tolist()}

    @classmethod
    def from_dict(cls, d: dict[str, Any]) -> "CorrelationReport":
        r = np.array([[np.nan if v is None else float(v) for v in row] for row in d["r"]], dtype=np.float64)
        F = len(d["names"])
        return cls(r=r.reshape(F, F), n=np.asarray(d["n"], dtype=np.int64).reshape(F, F), names=list(d["names"]),
                   method=d["method"])

    def vif(self) -> dict[str, float]:
        return vif(self)


def correlation_matrix(X, feature_names: Sequence[str] | None = None, method: str = "pearson",
                       missing: str = "pairwise", min_periods: int = 1) -> CorrelationReport:
    """The correlation matrix of the columns of ``X`` (a CUDA tensor: on its device; a CPU tensor, an array or a
    DataFrame: NumPy). A value is missing when it is not finite.

    ``missing="pairwise"`` computes each pair on the rows where both are present, as ``pandas.DataFrame.corr``
    does; ``"listwise"`` first blanks, in a copy, every row that has any missing value. ``min_periods``: pairs
    with fewer joint rows are NaN, and so are pairs with a constant column.

    ``method="spearman"`` is Pearson on ``ops.corr_ops.column_ranks``: each column is ranked once, over its own
    present values. That equals ``pandas.DataFrame.corr("spearman")`` exactly when no values are missing, or with
    ``missing="listwise"``. Under pairwise deletion pandas re-ranks the two columns of every pair over their joint
    rows, F^2 sorts, and the two answers differ slightly; use ``"listwise"`` where the pandas number is needed."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if missing not in MISSING:
        raise ValueError(f"missing must be one of {MISSING}, got {missing!r}")
    if int(min_periods) < 1:
        raise ValueError(f"min_periods must be at least 1, got {min_periods}")
    X, names = _matrix(X, feature_names)
    on_gpu = isinstance(X, torch.Tensor)
    if on_gpu:
        corr_ops._rows(X)  # dtype, rank, stride and width, before any work on the device
    else:
        X = corr_ops._host_matrix(X)
    if missing == "listwise":
        if on_gpu:
            bad = ~torch.isfinite(X).all(dim=1)
            X = X.clone()
            X[bad] = float("nan")
        else:
            bad = ~np.isfinite(X).all(axis=1)
            X = np.array(X, dtype=X.dtype if X.dtype.kind == "f" else np.float64, copy=True)
            X[bad] = np.nan
    if method == "spearman":
        R = corr_ops.column_ranks(X)
        X = R if on_gpu else R.numpy()
    n, A, Q, P = corr_ops.pair_moments(X)
    r = corr_ops.corr_from_moments(n, A, Q, P, min_periods=min_periods)
    return CorrelationReport(r=r, n=corr_ops._np(n).astype(np.int64), names=names, method=method)


def vif(report) -> dict[str, float]:
    """Variance inflation factors ``diag(R^-1)``, by Cholesky on the host in float64: feature -> VIF. ``report`` is
    a ``CorrelationReport`` (or a square matrix, then the keys are ``f0 ..``). A matrix with a NaN entry, or one
    that is not positive definite (pairwise deletion and exact duplicates both cause that), raises
    ``ValueError``."""
    if isinstance(report, CorrelationReport):
        R, names = np.asarray(report.r, dtype=np.float64), list(report.names)
    else:
        R = np.asarray(report, dtype=np.float64)
        names = [f"f{i}" for i in range(R.shape[0])]
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError(f"a square correlation matrix is needed, got {R.shape}")
    if not bool(np.isfinite(R).all()):
        bad = sorted({names[i] for i in np.argwhere(~np.isfinite(R))[:, 0]})
        raise ValueError(f"the correlation matrix has undefined entries (features {bad[:8]}): drop constant or "
                         f"absent columns, or raise the joint coverage, before asking for VIF")
    try:
        L = np.linalg.cholesky(R)
        singular = float(np.min(np.diag(L))) ** 2 <= 64.0 * R.shape[0] * np.finfo(np.float64).eps
    except np.linalg.LinAlgError:
        singular = True
    if singular:  # a pivot at the rounding level is a duplicate whose r came out one step below 1
        lo = float(np.linalg.eigvalsh(R)[0])
        raise ValueError(f"the correlation matrix is not positive definite (smallest eigenvalue {lo:.3e}): "
                         f"compute it with missing=\"listwise\", or drop a duplicate feature") from None
    Linv = np.linalg.solve(L, np.eye(R.shape[0]))
    d = np.sum(Linv * Linv, axis=0)  # diag(L^-T L^-1)
    return {name: float(v) for name, v in zip(names, d)}


@dataclass
class Screen:
    """``kept``: column indices in the order they were visited; ``dropped``: one record per dropped feature with
    the kept feature that displaced it and their r."""
    kept: list[int]
    dropped: list[dict[str, Any]] = field(default_factory=list)
    names: list[str] = field(default_factory=list)

    @property
    def kept_names(self) -> list[str]:
        return [self.names[i] for i in self.kept]

    def to_dict(self) -> dict[str, Any]:
        return {"kept": [self.names[i] for i in self.kept], "dropped": [dict(d) for d in self.dropped]}


def drop_correlated(report: CorrelationReport, threshold: float = 0.7, priority=None) -> Screen:
    """Greedy and deterministic: the features are visited in descending ``priority`` (ties and the default: column
    order) and one is dropped if its ``|r|`` with an already kept feature is ``>= threshold``; the record names the
    first such kept feature. NaN correlations never drop anything. ``priority``: one number per feature, for
    instance the IV of ``monitor.information_value``, a gain or a permutation importance."""
    F = len(report.names)
    if priority is None:
        order = list(range(F))
    else:
        p = np.asarray(priority, dtype=np.float64).reshape(-1)
        if p.shape[0] != F or bool(np.isnan(p).any()):
            raise ValueError(f"priority must hold {F} numbers")
        order = sorted(range(F), key=lambda i: (-p[i], i))
    kept: list[int] = []
    dropped = []
    for i in order:
        by = None
        for k in kept:
            v = float(report.r[i, k])
            if np.isfinite(v) and abs(v) >= threshold:
                by = (k, v)
                break
        if by is None:
            kept.append(i)
        else:
            dropped.append({"feature": report.names[i], "index": i, "by": report.names[by[0]], "by_index": by[0],
                            "r": by[1]})
    return Screen(kept=kept, dropped=dropped, names=list(report.names))
