"""Population stability (PSI / CSI) drift reports and weight-of-evidence / information-value tables.

Both questions -- "has the applicant population or the score moved since the fit?" and "how much does each
binned characteristic separate good loans from bad ones?" -- reduce to one table: exact per-feature, per-bin,
per-class weighted integer counts of an ``[N, F]`` matrix. This module is the definition of that table and
of everything computed from it, in NumPy; it is also the CPU path. On a GPU the table comes from
``csrc/bincount.hip`` (``ops.monitor_ops.bin_counts_gpu``) with the same integers, and the float64
post-processing below is shared, so the CPU and GPU reports are equal floats, not merely close.

Bins. A feature with ``K`` interior edges ``z`` has ``K + 2`` cells: value ``x`` goes to cell ``#{i : z[i] < x}``
(``searchsorted(z, x, "left")``: the intervals ``(z[b-1], z[b]]``, the side of ``ale_interval``), ``-inf`` and
``+inf`` to the end cells ``0`` and ``K``, NaN to the missing cell ``K + 1``.

Weights are integers: float sample weights are quantised once per data set by ``models.sketch.quantize_weights``
(``round(w / max(w) * 2^20)``); PSI and WoE are ratios within one data set, so the scale cancels.

Conventions (stated, not derived): in PSI a zero proportion is replaced by ``eps = 1e-4`` without renormalising,
cells empty on both sides are skipped, and the missing cell is a cell like any other; the status bands are the
industry's usual ones, PSI < 0.1 "stable", < 0.25 "moderate", otherwise "shifted". WoE smooths every non-empty
cell by ``a = 0.5`` rows per class. Class 0 (``y <= 0.5``) is "good", class 1 "bad".
"""
from __future__ import annotations

import json
from typing import Any, Sequence

import numpy as np
import torch

from ..models.sketch import WEIGHT_SCALE, quantize_weights

PSI_STABLE = 0.1      # below: "stable"
PSI_SHIFTED = 0.25    # below: "moderate", from here on "shifted"
PSI_EPS = 1e-4
WOE_SMOOTH = 0.5
SCORE = "score"


# ------------------------------------------------------------------------------------ the definition
def check_drift_edges(z) -> np.ndarray:
    """Interior edges as a float32 vector: finite and strictly increasing; ``K = 0`` (one bin) is allowed.
    ``ValueError`` otherwise."""
    z = np.asarray(z.detach().cpu().numpy() if hasattr(z, "detach") else z)
    if z.ndim != 1:
        raise ValueError(f"drift edges must be a vector, got shape {z.shape}")
    z = np.ascontiguousarray(z, dtype=np.float32)
    if not bool(np.isfinite(z).all()) or not bool((z[1:] > z[:-1]).all()):
        raise ValueError("drift edges must be finite and strictly increasing (as float32)")
    return z


def drift_edges(col, n_bins: int = 10) -> np.ndarray:
    """The interior edges of a column, float32 and strictly increasing, from its finite values: one bin per
    distinct value (``unique[:-1]``) when there are at most ``n_bins`` of them, else the distinct float32 values
    of the ``1/n_bins .. (n_bins-1)/n_bins`` quantiles (taken in float64). An empty, all-NaN or constant column
    has no edge."""
    if int(n_bins) < 1:
        raise ValueError(f"n_bins must be at least 1, got {n_bins}")
    n_bins = int(n_bins)
    col = np.asarray(col.detach().cpu().numpy() if hasattr(col, "detach") else col, dtype=np.float32).reshape(-1)
    vals = col[np.isfinite(col)]
    u = np.unique(vals)
    if u.shape[0] <= n_bins:
        return u[:-1].astype(np.float32)
    q = np.quantile(vals.astype(np.float64), np.arange(1, n_bins) / n_bins)
    return np.unique(q.astype(np.float32))


def drift_cell(z: np.ndarray, x: np.ndarray) -> np.ndarray:
    """The cell in ``[0, K + 1]`` of every value of ``x`` among the edges ``z[0..K)`` (module docstring)."""
    z = np.asarray(z, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    k = np.searchsorted(z, np.where(nan, np.float32(0), x), side="left")
    return np.where(nan, len(z) + 1, k).astype(np.int64)


def cell_pointer(edges_list: Sequence[np.ndarray]) -> np.ndarray:
    """int64 [F + 1]: the first cell of every feature in the concatenated table (``K_f + 2`` cells each)."""
    return np.concatenate([[0], np.cumsum([len(z) + 2 for z in edges_list])]).astype(np.int64)


def _exact_bincount(cell: np.ndarray, w: np.ndarray | None, size: int) -> np.ndarray:
    if w is None:
        return np.bincount(cell, minlength=size).astype(np.int64)
    if cell.shape[0] * float(w.max(initial=0)) < 2.0 ** 53:   # every partial sum is an exact float64 integer
        return np.bincount(cell, weights=w.astype(np.float64), minlength=size).astype(np.int64)
    out = np.zeros(size, dtype=np.int64)
    np.add.at(out, cell, w)
    return out


def bin_counts_host(X, edges_list: Sequence[np.ndarray], y=None, wq=None) -> tuple[np.ndarray, np.ndarray]:
    """``(counts int64 [C, cells], cell_ptr int64 [F + 1])``: the weighted count of the rows of ``X`` [N, F] in
    every cell of every feature; ``C = 2`` with labels (class ``y > 0.5``), else 1; ``wq``: int64 integer
    weights, 1 per row when absent. The definition of ``csrc/bincount.hip``: exact integers."""
    X = np.asarray(X, dtype=np.float32)
    if X.ndim != 2 or X.shape[1] != len(edges_list):
        raise ValueError(f"X must be [rows, {len(edges_list)}], got shape {X.shape}")
    edges_list = [check_drift_edges(z) for z in edges_list]
    N = X.shape[0]
    ptr = cell_pointer(edges_list)
    w = None
    if wq is not None:
        w = np.asarray(wq, dtype=np.int64).reshape(-1)
        if w.shape[0] != N or bool((w < 0).any()):
            raise ValueError(f"wq must be {N} non-negative integers")
    cls = None
    if y is not None:
        yv = np.asarray(y, dtype=np.float32).reshape(-1)
        if yv.shape[0] != N:
            raise ValueError(f"X has {N} rows, y has {yv.shape[0]}")
        cls = yv > np.float32(0.5)
    out = np.zeros((1 if cls is None else 2, int(ptr[-1])), dtype=np.int64)
    for f, z in enumerate(edges_list):
        cell = drift_cell(z, X[:, f])
        size = len(z) + 2
        if cls is None:
            out[0, ptr[f]:ptr[f + 1]] = _exact_bincount(cell, w, size)
        else:
            for c, m in enumerate((~cls, cls)):
                out[c, ptr[f]:ptr[f + 1]] = _exact_bincount(cell[m], None if w is None else w[m], size)
    return out, ptr


def psi(ref_counts, cur_counts, eps: float = PSI_EPS) -> float:
    """Population stability index of one feature's two count vectors, in float64: ``sum (q - p) ln(q / p)`` over
    the cells that are not empty on both sides, a zero proportion replaced by ``eps`` (no renormalisation)."""
    r = np.asarray(ref_counts, dtype=np.float64).reshape(-1)
    c = np.asarray(cur_counts, dtype=np.float64).reshape(-1)
    if r.shape != c.shape:
        raise ValueError(f"count vectors differ in length: {r.shape[0]} and {c.shape[0]}")
    if r.sum() <= 0 or c.sum() <= 0:
        raise ValueError("PSI needs rows on both sides")
    p, q = r / r.sum(), c / c.sum()
    keep = (r > 0) | (c > 0)
    p = np.where(p[keep] > 0, p[keep], eps)
    q = np.where(q[keep] > 0, q[keep], eps)
    return float(np.sum((q - p) * np.log(q / p)))


def psi_status(value: float) -> str:
    """"stable" (< 0.1), "moderate" (< 0.25) or "shifted": the industry's usual bands."""
    return "stable" if value < PSI_STABLE else "moderate" if value < PSI_SHIFTED else "shifted"


def woe_iv(counts2) -> tuple[np.ndarray, float]:
    """Weight of evidence per cell and information value of one feature from its ``[2, cells]`` counts (row 0
    good, row 1 bad). Over the ``m`` non-empty cells, ``a = 0.5``: ``dg = (good + a) / (Good + a m)``, ``db``
    alike, ``woe = ln(dg / db)``, ``IV = sum (dg - db) woe``; empty cells get 0. ``ValueError`` when a class
    is absent."""
    c = np.asarray(counts2, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != 2:
        raise ValueError(f"WoE needs [2, cells] counts, got shape {c.shape}")
    good, bad = c[0], c[1]
    if good.sum() <= 0 or bad.sum() <= 0:
        raise ValueError("WoE needs both classes")
    live = (good + bad) > 0
    m = int(live.sum())
    dg = (good[live] + WOE_SMOOTH) / (good.sum() + WOE_SMOOTH * m)
    db = (bad[live] + WOE_SMOOTH) / (bad.sum() + WOE_SMOOTH * m)
    w = np.log(dg / db)
    woe = np.zeros(c.shape[1], dtype=np.float64)
    woe[live] = w
    return woe, float(np.sum((dg - db) * w))


# ------------------------------------------------------------------------------------ inputs
def _on_gpu(X) -> bool:
    return isinstance(X, torch.Tensor) and X.device.type == "cuda"


def _matrix(X, names: Sequence[str] | None):
    """A CUDA tensor stays as it is; anything else becomes float32 NumPy (a DataFrame's columns by name)."""
    if isinstance(X, torch.Tensor):
        return X.to(torch.float32) if X.device.type == "cuda" else X.detach().numpy().astype(np.float32, copy=False)
    if hasattr(X, "columns") and names is not None and all(n in X.columns for n in names):
        X = X[list(names)]
    return np.asarray(X.to_numpy(dtype=np.float32, na_value=np.nan) if hasattr(X, "to_numpy") else X,
                      dtype=np.float32)


def _booster_of(model):
    """``(booster, n_trees)`` of a ``Booster`` or a ``GBDTClassifier`` (the trees ``predict_proba`` scores)."""
    from ..models.booster import Booster

    if isinstance(model, Booster):
        return model, None
    if hasattr(model, "get_booster") and hasattr(model, "_n_trees"):
        return model.get_booster(), model._n_trees(None)
    raise TypeError("expected a Booster or a GBDTClassifier")


def _margin(model, X):
    """The float32 margin of every row, where ``X`` lives: bit-identical between the host and device predictors
    (a float32 sigmoid is not guaranteed to be, and PSI on quantile bins is invariant under the monotone map)."""
    b, n_trees = _booster_of(model)
    if _on_gpu(X):
        return b.predict_margin(X, n_trees=n_trees)
    return np.asarray(b.predict_margin(X, device="cpu", n_trees=n_trees), dtype=np.float32)


def _quantized(sample_weight, n: int, X, weight_scale: float | None):
    """Integer weights of one data set (None when unweighted), where ``X`` lives: ``quantize_weights`` with the
    set's own maximum, or with an explicit ``weight_scale`` (chunks of one set share it)."""
    if sample_weight is None:
        return None
    dev = X.device if _on_gpu(X) else torch.device("cpu")
    w = sample_weight if isinstance(sample_weight, torch.Tensor) else torch.as_tensor(np.asarray(sample_weight))
    w = w.reshape(-1)
    if w.shape[0] != n:
        raise ValueError(f"X has {n} rows, sample_weight has {w.shape[0]}")
    if weight_scale is None:
        q = quantize_weights(w, n, dev)
    else:
        wd = w.to(device=dev, dtype=torch.float64)
        if not weight_scale > 0 or bool(((wd < 0) | ~torch.isfinite(wd) | (wd > weight_scale)).any()):
            raise ValueError("weights must be finite and within [0, weight_scale]")
        q = torch.round(wd * (WEIGHT_SCALE / float(weight_scale))).to(torch.int64)
    return q if _on_gpu(X) else q.numpy()


def _labels(y, n: int, X):
    if y is None:
        return None
    if _on_gpu(X):
        yt = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y, dtype=np.float32))
        yt = yt.to(device=X.device, dtype=torch.float32).reshape(-1).contiguous()
        if yt.shape[0] != n:
            raise ValueError(f"X has {n} rows, y has {yt.shape[0]}")
        return yt
    yv = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float32).reshape(-1)
    if yv.shape[0] != n:
        raise ValueError(f"X has {n} rows, y has {yv.shape[0]}")
    return yv


def _hex(z: np.ndarray) -> list[str]:
    return [float(v).hex() for v in np.asarray(z, dtype=np.float32)]


# ------------------------------------------------------------------------------------ public interface
class DriftReport:
    """Rows (one dict per feature, ``"score"`` first, then by PSI descending) of a baseline against a current
    data set: ``feature, psi, status, edges, ref_counts, cur_counts, ref_prop, cur_prop, ref_missing_rate,
    cur_missing_rate`` and, for a side that had labels, ``<side>_class_counts, <side>_woe, <side>_iv``."""

    def __init__(self, rows: list[dict[str, Any]]):
        self.rows = rows

    def __iter__(self):
        return iter(self.rows)

    def __len__(self) -> int:
        return len(self.rows)

    def __getitem__(self, feature: str) -> dict[str, Any]:
        for r in self.rows:
            if r["feature"] == feature:
                return r
        raise KeyError(feature)

    def to_dict(self) -> dict[str, Any]:
        def plain(v):
            return v.tolist() if isinstance(v, np.ndarray) else v

        return {"bands": {"stable_below": PSI_STABLE, "shifted_from": PSI_SHIFTED, "eps": PSI_EPS},
                "rows": [{k: plain(v) for k, v in r.items()} for r in self.rows]}


class DriftAccumulator:
    """Counts of a current data set that arrives in pieces (:meth:`DriftBaseline.accumulator`). Integer counts
    add exactly, so without weights :meth:`report` equals the one-shot :meth:`DriftBaseline.compare`; with
    weights the chunks share the explicit ``weight_scale`` (an upper bound of every weight: ``max(w)`` is not
    known per chunk). All chunks live in one place: NumPy / CPU input, or CUDA tensors of one device."""

    def __init__(self, baseline: "DriftBaseline", weight_scale: float | None = None):
        self.baseline = baseline
        self.weight_scale = weight_scale
        self._host: np.ndarray | None = None
        self._dev: list[torch.Tensor] | None = None
        self._labelled: bool | None = None

    def update(self, X_chunk, y=None, sample_weight=None) -> "DriftAccumulator":
        if sample_weight is not None and self.weight_scale is None:
            raise ValueError("weighted accumulation needs accumulator(weight_scale=...)")
        return self._add(X_chunk, y, sample_weight, self.weight_scale)

    def _add(self, X, y, sample_weight, weight_scale) -> "DriftAccumulator":
        b = self.baseline
        if self._labelled is None:
            self._labelled = y is not None
        elif self._labelled != (y is not None):
            raise ValueError("every chunk must come with labels, or none")
        X = _matrix(X, b.feature_names[:b.n_features])
        if X.ndim != 2 or X.shape[1] != b.n_features:
            raise ValueError(f"X must be [rows, {b.n_features}], got shape {tuple(X.shape)}")
        n = X.shape[0]
        yv = _labels(y, n, X)
        wq = _quantized(sample_weight, n, X, weight_scale)
        C, F = (2 if self._labelled else 1), b.n_features
        # the matrix, then (a second call on an [N, 1] matrix) the margin: two tables side by side
        parts = [(X, b.edges[:F])]
        if b.has_score:
            parts.append((_margin(b._need_model(), X).reshape(n, 1), b.edges[F:]))
        if _on_gpu(X):
            from ..ops import monitor_ops

            if self._host is not None or (self._dev is not None and self._dev[0].device != X.device):
                raise ValueError("the chunks of one accumulator must live in one place (the host, or one device)")
            if self._dev is None:
                self._dev = [torch.zeros((C, int(cell_pointer(ez)[-1])), dtype=torch.int64, device=X.device)
                             for _, ez in parts]
            for (Xp, ez), out in zip(parts, self._dev):   # the weights were quantised here: no range check
                monitor_ops.bin_counts_gpu(Xp, ez, y=yv, wq=wq, out=out, wq_in_range=True)
            return self
        if self._dev is not None:
            raise ValueError("the chunks of one accumulator must live in one place (the host, or one device)")
        c = np.concatenate([bin_counts_host(Xp, ez, yv, wq)[0] for Xp, ez in parts], axis=1)
        self._host = c if self._host is None else self._host + c
        return self

    def counts(self) -> np.ndarray:
        """int64 [C, cells] on the host: everything added so far."""
        if self._dev is not None:
            return torch.cat(self._dev, dim=1).cpu().numpy()
        if self._host is None:
            raise ValueError("nothing was added")
        return self._host

    def report(self) -> DriftReport:
        return self.baseline._report(self.counts())


class DriftBaseline:
    """The per-feature edges and reference counts of the data a model was fitted on (:meth:`fit`), against which
    later data is compared (:meth:`compare`, :meth:`accumulator`). With a model the margin is one more
    "feature", ``"score"`` (its PSI is the population stability index proper; the features' are the
    characteristic stability indices)."""

    def __init__(self, feature_names: list[str], edges: list[np.ndarray], ref_counts: np.ndarray, n_bins: int,
                 has_score: bool, model=None):
        self.feature_names = list(feature_names)
        self.edges = [check_drift_edges(z) for z in edges]
        self.cell_ptr = cell_pointer(self.edges)
        self.ref_counts = np.asarray(ref_counts, dtype=np.int64)
        self.n_bins = int(n_bins)
        self.has_score = bool(has_score)
        self.model = model
        if len(self.feature_names) != len(self.edges) or self.ref_counts.ndim != 2 \
                or self.ref_counts.shape[0] not in (1, 2) or self.ref_counts.shape[1] != int(self.cell_ptr[-1]):
            raise ValueError("names, edges and reference counts do not describe one table")

    @property
    def n_features(self) -> int:
        """Columns of ``X`` (the score is not one)."""
        return len(self.edges) - (1 if self.has_score else 0)

    def _need_model(self):
        if self.model is None:
            raise ValueError("this baseline has a score row: pass the model (from_json(text, model=...))")
        return self.model

    @classmethod
    def fit(cls, X_ref, *, feature_names: Sequence[str] | None = None, model=None, n_bins: int = 10,
            sample_weight=None, y=None) -> "DriftBaseline":
        """Edges (:func:`drift_edges`, computed on the host: a fit happens once) and reference counts of
        ``X_ref``; with ``model`` (a ``Booster`` or a ``GBDTClassifier``) also of its float32 margin. A CUDA
        tensor is counted on its device, NumPy / CPU input on the host."""
        names = list(feature_names) if feature_names is not None else None
        if names is None and model is not None:
            names = _booster_of(model)[0].feature_names or None
            names = list(names) if names is not None else None
        if names is None and hasattr(X_ref, "columns"):
            names = [str(c) for c in X_ref.columns]
        X = _matrix(X_ref, names)
        if X.ndim != 2 or X.shape[0] == 0:
            raise ValueError(f"X_ref must be [rows, features] with rows, got shape {tuple(X.shape)}")
        n, F = X.shape
        if names is None:
            names = [f"f{i}" for i in range(F)]
        if len(names) != F:
            raise ValueError(f"{F} columns but {len(names)} feature names")
        Xh = X.cpu().numpy() if _on_gpu(X) else X
        edges = [drift_edges(Xh[:, f], n_bins) for f in range(F)]
        if model is not None:
            if SCORE in names:
                raise ValueError(f'a feature is already named "{SCORE}"')
            m = _margin(model, X)
            edges.append(drift_edges(m.cpu().numpy() if _on_gpu(X) else m, n_bins))
            names = names + [SCORE]
        base = cls(names, edges, np.zeros((1 if y is None else 2, int(cell_pointer(edges)[-1])), np.int64), n_bins,
                   model is not None, model)
        base.ref_counts = DriftAccumulator(base)._add(X, y, sample_weight, None).counts()
        return base

    # ---- persistence: settings and integers only; float32 edges as float.hex, which round-trips exactly
    def to_json(self) -> str:
        return json.dumps({"version": 1, "feature_names": self.feature_names, "n_bins": self.n_bins,
                           "has_score": self.has_score, "edges": [_hex(z) for z in self.edges],
                           "ref_counts": self.ref_counts.tolist()})

    @classmethod
    def from_json(cls, text: str, model=None) -> "DriftBaseline":
        d = json.loads(text)
        if d.get("version") != 1:
            raise ValueError(f"unknown drift baseline version {d.get('version')!r}")
        edges = [np.array([float.fromhex(v) for v in z], dtype=np.float32) for z in d["edges"]]
        return cls(d["feature_names"], edges, np.asarray(d["ref_counts"], dtype=np.int64).reshape(
            len(d["ref_counts"]), -1), d["n_bins"], d["has_score"], model)

    # ---- comparison
    def accumulator(self, weight_scale: float | None = None) -> DriftAccumulator:
        return DriftAccumulator(self, weight_scale)

    def compare(self, X_cur, *, sample_weight=None, y=None) -> DriftReport:
        """The drift report of ``X_cur`` against the baseline, counted where ``X_cur`` lives."""
        return DriftAccumulator(self)._add(X_cur, y, sample_weight, None).report()

    def _report(self, cur: np.ndarray) -> DriftReport:
        ref, ptr = self.ref_counts, self.cell_ptr
        rows = []
        for f, name in enumerate(self.feature_names):
            sl = slice(int(ptr[f]), int(ptr[f + 1]))
            row: dict[str, Any] = {"feature": name, "edges": self.edges[f].astype(np.float64)}
            for side, c in (("ref", ref), ("cur", cur)):
                tot = c[:, sl].sum(0)
                if tot.sum() <= 0:
                    raise ValueError(f"no rows on the {side} side")
                row[f"{side}_counts"] = tot
                row[f"{side}_prop"] = tot / float(tot.sum())
                row[f"{side}_missing_rate"] = float(tot[-1] / float(tot.sum()))
                if c.shape[0] == 2:
                    row[f"{side}_class_counts"] = c[:, sl].copy()
                    row[f"{side}_woe"], row[f"{side}_iv"] = woe_iv(c[:, sl])
            row["psi"] = psi(row["ref_counts"], row["cur_counts"])
            row["status"] = psi_status(row["psi"])
            rows.append(row)
        rows.sort(key=lambda r: (r["feature"] != SCORE or not self.has_score, -r["psi"]))
        return DriftReport(rows)


def information_value(X, y, *, feature_names: Sequence[str] | None = None, n_bins: int = 10,
                      sample_weight=None) -> list[dict[str, Any]]:
    """The WoE / IV screening table: per feature ``{"feature", "iv", "woe" [cells], "edges", "counts" [2,
    cells]}``, sorted by IV descending. Counted where ``X`` lives, like :meth:`DriftBaseline.fit`."""
    if y is None:
        raise ValueError("information value needs labels")
    base = DriftBaseline.fit(X, feature_names=feature_names, n_bins=n_bins, sample_weight=sample_weight, y=y)
    out = []
    for f, name in enumerate(base.feature_names):
        c = base.ref_counts[:, int(base.cell_ptr[f]):int(base.cell_ptr[f + 1])]
        woe, iv = woe_iv(c)
        out.append({"feature": name, "iv": iv, "woe": woe, "edges": base.edges[f].astype(np.float64),
                    "counts": c.copy()})
    out.sort(key=lambda r: -r["iv"])
    return out
