"""Tree-ensemble model in the XGBoost 3.0 layout, with checkpoint I/O and inference entry points.

The reference's model artifact is a joblib pickle of ``xgboost.sklearn.XGBClassifier`` whose
``_Booster.handle`` is a UBJSON document (src/model_train_test/
model_tree_train_test.py:215-219; src/api/cobalt_fast_api.py:45). :class:`Booster` holds the same
per-tree arrays (``left_children``, ``right_children``, ``parents``, ``split_indices``,
``split_conditions``, ``default_left``, ``base_weights``, ``loss_changes``, ``sum_hessian``) and
reads/writes that document, so artifacts move both ways between this framework and XGBoost.

Inference (`predict`, `shap_values`, `shap_interaction_values`) dispatches on device: CUDA tensors /
``device="cuda"`` run the gfx950 kernels in ``ops/predict_ops.py``; ``device="cpu"`` runs the NumPy
reference implementation (`predict_margin_host`, `treeshap_host`, `treeshap_interactions_host`), which is
also the oracle of the GPU tests. `eval_curve` / `staged_margins` (the metrics / margins after every tree,
one forest pass; oracle `eval_curve_host`) dispatch the same way.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Iterable, Sequence

import numpy as np

from ..dataio import safe_pickle, ubjson

ROOT_PARENT = 2147483647


def _fmt_float(x: float) -> str:
    """XGBoost writes float parameters with up to 9 significant digits ('0.0500000007')."""
    if x == int(x) and abs(x) < 1e15:
        return str(int(x))
    return f"{np.float32(x):.9g}"


@dataclass
class Tree:
    left_children: np.ndarray      # int32 [n]; -1 for leaves
    right_children: np.ndarray     # int32 [n]
    parents: np.ndarray            # int32 [n]; root = 2147483647
    split_indices: np.ndarray      # int32 [n]
    split_conditions: np.ndarray   # float32 [n]; leaf value for leaves
    default_left: np.ndarray       # uint8 [n]
    base_weights: np.ndarray       # float32 [n]
    loss_changes: np.ndarray       # float32 [n]
    sum_hessian: np.ndarray        # float32 [n]

    @property
    def num_nodes(self) -> int:
        return int(self.left_children.shape[0])

    @property
    def is_leaf(self) -> np.ndarray:
        return self.left_children == -1

    def depth(self) -> int:
        d = np.zeros(self.num_nodes, dtype=np.int32)
        for i in range(1, self.num_nodes):
            d[i] = d[self.parents[i]] + 1
        return int(d.max()) if self.num_nodes else 0

    def to_doc(self, tree_id: int, num_feature: int) -> dict[str, Any]:
        n = self.num_nodes
        return {
            "base_weights": self.base_weights.astype(np.float32),
            "categories": np.zeros(0, dtype=np.int32),
            "categories_nodes": np.zeros(0, dtype=np.int32),
            "categories_segments": np.zeros(0, dtype=np.int64),
            "categories_sizes": np.zeros(0, dtype=np.int64),
            "default_left": self.default_left.astype(np.uint8),
            "id": int(tree_id),
            "left_children": self.left_children.astype(np.int32),
            "loss_changes": self.loss_changes.astype(np.float32),
            "parents": self.parents.astype(np.int32),
            "right_children": self.right_children.astype(np.int32),
            "split_conditions": self.split_conditions.astype(np.float32),
            "split_indices": self.split_indices.astype(np.int32),
            "split_type": np.zeros(n, dtype=np.uint8),
            "sum_hessian": self.sum_hessian.astype(np.float32),
            "tree_param": {"num_deleted": "0", "num_feature": str(num_feature), "num_nodes": str(n),
                           "size_leaf_vector": "1"},
        }

    @classmethod
    def from_doc(cls, d: dict[str, Any]) -> "Tree":
        def arr(k, dt):
            v = d[k]
            return np.asarray(v, dtype=dt).copy()

        if np.asarray(d.get("split_type", [])).any():
            raise NotImplementedError("categorical splits are not used by the credit-risk models")
        return cls(
            left_children=arr("left_children", np.int32),
            right_children=arr("right_children", np.int32),
            parents=arr("parents", np.int32),
            split_indices=arr("split_indices", np.int32),
            split_conditions=arr("split_conditions", np.float32),
            default_left=arr("default_left", np.uint8),
            base_weights=arr("base_weights", np.float32),
            loss_changes=arr("loss_changes", np.float32),
            sum_hessian=arr("sum_hessian", np.float32),
        )


def _logit(p: float) -> float:
    p = min(max(p, 1e-16), 1 - 1e-16)
    return math.log(p / (1 - p))


@dataclass
class Booster:
    """An additive ensemble of regression trees for ``binary:logistic`` (XGBoost ``gbtree``)."""

    trees: list[Tree]
    feature_names: list[str] | None = None
    feature_types: list[str] | None = None
    base_score: float = 0.5
    num_feature: int = 0
    objective: str = "binary:logistic"
    train_params: dict[str, Any] = field(default_factory=dict)
    attributes: dict[str, str] = field(default_factory=dict)
    # the "Config" section of a loaded model, re-emitted verbatim while the forest is unchanged
    source_config: dict[str, Any] | None = field(default=None, repr=False, compare=False)

    # --------------------------------------------------------------------------------- basics
    @property
    def base_margin(self) -> float:
        """Margin-space intercept: logit(base_score) for binary:logistic, as float32."""
        if self.objective == "binary:logistic":
            return float(np.float32(_logit(float(self.base_score))))
        return float(np.float32(self.base_score))

    @property
    def num_trees(self) -> int:
        return len(self.trees)

    @property
    def monotone_constraints(self) -> tuple[int, ...] | None:
        """The monotone constraints the model was fitted under, one of {-1, 0, +1} per feature (None:
        unconstrained)."""
        v = self.train_params.get("monotone_constraints")
        return tuple(int(c) for c in v) if v else None

    @property
    def interaction_constraints(self) -> list[list[int]] | None:
        """The interaction constraints the model was fitted under: the feature groups as sorted index lists
        (None: unconstrained)."""
        v = self.train_params.get("interaction_constraints")
        return [[int(i) for i in g] for g in v] if v else None

    def slice(self, n_trees: int) -> "Booster":
        return Booster(self.trees[:n_trees], self.feature_names, self.feature_types, self.base_score,
                       self.num_feature, self.objective, dict(self.train_params), dict(self.attributes))

    def max_depth(self) -> int:
        return max((t.depth() for t in self.trees), default=0)

    # ------------------------------------------------------------------------- importance
    def get_score(self, importance_type: str = "weight") -> dict[str, float]:
        """Per-feature importance with XGBoost's ``Booster.get_score`` semantics.

        Used by ``/feature_importance_bulk`` (reference: src/api/cobalt_fast_api.py:128-143).
        """
        F = self.num_feature
        weight = np.zeros(F, dtype=np.float64)
        gain = np.zeros(F, dtype=np.float64)
        cover = np.zeros(F, dtype=np.float64)
        for t in self.trees:
            m = ~t.is_leaf
            f = t.split_indices[m]
            np.add.at(weight, f, 1.0)
            np.add.at(gain, f, t.loss_changes[m].astype(np.float64))
            np.add.at(cover, f, t.sum_hessian[m].astype(np.float64))
        names = self.feature_names or [f"f{i}" for i in range(F)]
        out: dict[str, float] = {}
        for i in range(F):
            if weight[i] == 0:
                continue
            if importance_type == "weight":
                v = weight[i]
            elif importance_type == "gain":
                v = gain[i] / weight[i]
            elif importance_type == "total_gain":
                v = gain[i]
            elif importance_type == "cover":
                v = cover[i] / weight[i]
            elif importance_type == "total_cover":
                v = cover[i]
            else:
                raise ValueError(f"unknown importance_type {importance_type!r}")
            out[names[i]] = float(v)
        return out

    def feature_importances(self, importance_type: str = "gain") -> np.ndarray:
        """sklearn ``feature_importances_``: normalised per-feature score (0 for unused features)."""
        sc = self.get_score(importance_type)
        names = self.feature_names or [f"f{i}" for i in range(self.num_feature)]
        v = np.array([sc.get(n, 0.0) for n in names], dtype=np.float32)
        s = v.sum()
        return v / s if s > 0 else v

    # ------------------------------------------------------------------------- inference
    def predict_margin(self, X, device: str | None = None, n_trees: int | None = None):
        """Raw margins (base margin + sum of leaf values). ``X``: [N, F] float array/tensor."""
        from ..ops import predict_ops

        return predict_ops.predict_margin(self, X, device=device, n_trees=n_trees)

    def predict_proba(self, X, device: str | None = None, n_trees: int | None = None):
        from ..ops import predict_ops

        return predict_ops.predict_proba(self, X, device=device, n_trees=n_trees)

    def eval_curve(self, X, y, sample_weight=None, metrics: Sequence[str] = ("logloss",), device: str | None = None,
                   margin=None):
        """The metrics after every tree on the labelled rows ``(X, y)`` in one pass over the forest:
        ``({metric: float64 [num_trees]}, final margins)``. ``metrics``: "logloss", "error", "auc";
        ``margin`` ([N] float32): start from these margins instead of the base margin (the trees are then
        the continuation of the model that produced them)."""
        from ..ops import predict_ops

        return predict_ops.eval_curve(self, X, y, sample_weight=sample_weight, metrics=metrics, device=device,
                                      margin=margin)

    def staged_margins(self, X, device: str | None = None):
        """Margins after every tree, [num_trees, N] float32: row ``t`` has the bits of
        ``predict_margin(X, n_trees=t + 1)``."""
        from ..ops import predict_ops

        return predict_ops.staged_margins(self, X, device=device)

    def predict_leaf(self, X, device: str | None = None, n_trees: int | None = None):
        """The leaf every row lands in, per tree (XGBoost's ``pred_leaf=True``): int32 [N, T] node ids in this
        booster's own numbering (indices into ``Tree.left_children``). NumPy in gives NumPy out; a tensor in
        gives a tensor on its device out. ``n_trees``: the first trees only."""
        from ..ops import predict_ops

        return predict_ops.predict_leaf(self, X, device=device, n_trees=n_trees)

    def refresh(self, X, y, sample_weight=None, *, refresh_leaf: bool = True, device: str | None = None,
                return_margin: bool = False, leaf_index_bytes: int | None = None, dist=None, **overrides):
        """XGBoost's ``process_type="update", updater="refresh"``: a NEW booster with this model's structure
        (features, thresholds, default directions) whose node statistics (``sum_hessian``, ``base_weights``,
        ``loss_changes``) are recomputed on the labelled rows ``(X, y)`` and, with ``refresh_leaf``, whose leaf
        values are re-estimated too (:func:`refresh_host` is the definition). With ``refresh_leaf=False`` the
        predictions are unchanged and the covers that path-dependent TreeSHAP, :meth:`expected_value` and
        ``get_score("cover")`` read describe the rows given here. This booster is not modified.

        ``overrides``: ``learning_rate``, ``reg_lambda``, ``reg_alpha``, ``min_child_weight``,
        ``scale_pos_weight``, ``random_state``, ``grad_bits`` (default: this booster's ``train_params``, then
        XGBoost's defaults; 17 bits). ``return_margin``: return ``(booster, margins of the new model on X)``.
        ``leaf_index_bytes`` (GPU): see :func:`~..ops.predict_ops.refresh`; the result does not depend on it.
        ``ValueError``: monotone-constrained boosters, data-parallel runs (``dist.world > 1``), empty ``X``,
        labels outside {0, 1}, negative weights or weights that sum to 0. A subtree no row reaches gets cover
        0 throughout; path-dependent TreeSHAP is not defined below such a node."""
        from ..ops import predict_ops

        new, margin = predict_ops.refresh(self, X, y, sample_weight, refresh_leaf=refresh_leaf, device=device,
                                          leaf_index_bytes=leaf_index_bytes, dist=dist, **overrides)
        return (new, margin) if return_margin else new

    @property
    def best_iteration(self) -> int | None:
        """Global index of the best round of an early-stopped fit (XGBoost's ``best_iteration``
        attribute), None when the model was not fitted with early stopping."""
        v = self.attributes.get("best_iteration")
        return int(v) if v is not None else None

    @property
    def best_score(self) -> float | None:
        v = self.attributes.get("best_score")
        return float(v) if v is not None else None

    def shap_values(self, X, device: str | None = None):
        """Path-dependent TreeSHAP values [N, F] (+ expected value via :meth:`expected_value`)."""
        from ..ops import predict_ops

        return predict_ops.shap_values(self, X, device=device)

    def shap_interaction_values(self, X, device: str | None = None):
        """Path-dependent TreeSHAP interaction values [N, F, F] float64: every row of a matrix sums to
        the feature's SHAP value, off-diagonal cells split a pairwise effect evenly between [i][j] and
        [j][i], the diagonal holds the main effects."""
        from ..ops import predict_ops

        return predict_ops.shap_interaction_values(self, X, device=device)

    def shap_values_interventional(self, X, background, *, model_output: str = "raw", n_trees: int | None = None,
                                   device: str | None = None):
        """Interventional TreeSHAP values [N, F] float64 of ``X`` against the rows of ``background``
        (``shap``'s ``feature_perturbation="interventional"``): the mean over the background rows z of the
        Shapley values of ``S -> f(x on S, z elsewhere)``; covers are not used. ``model_output``: "raw"
        (margin) or "probability" (``shap``'s per-pair rescaling); with
        :meth:`expected_value_interventional` the values of a row add up to its margin / probability.
        ``n_trees``: explain the first trees only."""
        from ..ops import predict_ops

        return predict_ops.shap_values_interventional(self, X, background, model_output=model_output,
                                                      n_trees=n_trees, device=device)

    def expected_value_interventional(self, background, model_output: str = "raw",
                                      n_trees: int | None = None) -> float:
        """The baseline of :meth:`shap_values_interventional`: the mean over the background rows of the
        float64 margin ("raw") or of its sigmoid ("probability")."""
        Z = background.detach().cpu().numpy() if hasattr(background, "detach") else np.asarray(background)
        b = self if n_trees is None else self.slice(n_trees)
        return expected_value_interventional_host(b, Z.astype(np.float32, copy=False), model_output)

    def _feature_index(self, f) -> int:
        """A feature given by index or by name (``feature_names``) as an index; ``ValueError`` otherwise."""
        if isinstance(f, str):
            names = self.feature_names or [f"f{i}" for i in range(self.num_feature)]
            if f not in names:
                raise ValueError(f"unknown feature name {f!r}")
            return names.index(f)
        if isinstance(f, (bool, float)) or not isinstance(f, (int, np.integer)):
            raise ValueError(f"a feature is an index or a name, got {f!r}")
        if not 0 <= int(f) < self.num_feature:
            raise ValueError(f"feature index {int(f)} outside [0, {self.num_feature})")
        return int(f)

    def partial_dependence(self, X, features, *, grid=None, grid_resolution: int = 100,
                           percentiles: tuple[float, float] = (0.05, 0.95), include_missing: bool = False,
                           kind: str = "average", response: str = "probability", sample_weight=None,
                           n_trees: int | None = None, device: str | None = None) -> dict[str, Any]:
        """Partial dependence (PD) and individual conditional expectation (ICE) curves of one feature or a
        pair (scikit-learn's ``partial_dependence(method="brute")``): every row of ``X`` is scored with the
        feature(s) set to each grid value, everything else as in ``X`` (which is not modified).

        ``features``: an index or a name, or a pair. ``grid``: explicit grid values (one array, or a pair of
        arrays for two features; NaN = "the feature is missing"); by default each axis is built from the
        column's non-NaN values: its unique values if there are fewer than ``grid_resolution``, else
        ``grid_resolution`` points between the two ``percentiles``. ``include_missing`` appends a NaN point to
        every axis. ``kind``: "average", "individual" or "both". ``response``: "probability" (the mean of the
        per-row probabilities, not the sigmoid of the mean margin) or "margin" (log-odds). ``sample_weight``
        weights the average. ``n_trees``: score that prefix of the forest.

        Returns ``{"grid_values": [float32 axis, ...], "feature_names": [...], "average": float64 [G1] or
        [G1, G2], "individual": float32 [N, G1] or [N, G1, G2]}`` (the last two as ``kind`` asks). On a GPU
        one pass of ``csrc/pdp.hip`` per 16 grid points; ICE margins have the bits of ``predict_margin`` on
        the substituted rows and the averages are reduced in a fixed order (same input, same bits)."""
        from ..ops import predict_ops

        if kind not in ("average", "individual", "both"):
            raise ValueError(f"kind must be 'average', 'individual' or 'both', got {kind!r}")
        if response not in ("probability", "margin"):
            raise ValueError(f"response must be 'probability' or 'margin', got {response!r}")
        if isinstance(features, (str, int, np.integer)):
            features = [features]
        features = list(features)
        if len(features) not in (1, 2):
            raise ValueError(f"partial dependence takes one or two features, got {len(features)}")
        feats = [self._feature_index(f) for f in features]
        if len(feats) == 2 and feats[0] == feats[1]:
            raise ValueError(f"the two features must differ, got {features}")
        names = self.feature_names or [f"f{i}" for i in range(self.num_feature)]
        if hasattr(X, "columns") and self.feature_names:
            X = X[self.feature_names]
        if hasattr(X, "to_numpy"):
            X = X.to_numpy(dtype=np.float32, na_value=np.nan)
        if not hasattr(X, "shape") or len(X.shape) != 2:
            X = np.asarray(X, dtype=np.float32)
            if X.ndim != 2:
                raise ValueError(f"X must be [rows, features], got shape {X.shape}")
        N = int(X.shape[0])
        if N == 0 or X.shape[1] < self.num_feature:
            raise ValueError(f"X has shape {tuple(X.shape)}, model needs [rows >= 1, >= {self.num_feature}]")
        w = None
        if sample_weight is not None:
            w = np.asarray(sample_weight.detach().cpu().numpy() if hasattr(sample_weight, "detach")
                           else sample_weight, dtype=np.float32).reshape(-1)
            if w.shape[0] != N:
                raise ValueError(f"X has {N} rows, sample_weight has {w.shape[0]}")
            if not bool((w >= 0).all()) or not float(np.sum(w, dtype=np.float64)) > 0:  # (NaN fails too)
                raise ValueError("sample_weight must be non-negative with a positive sum")
        if grid is None:
            lo, hi = (float(q) for q in percentiles)
            if not 0.0 <= lo < hi <= 1.0:
                raise ValueError(f"percentiles must satisfy 0 <= low < high <= 1, got {percentiles}")
            if int(grid_resolution) < 2:
                raise ValueError(f"grid_resolution must be at least 2, got {grid_resolution}")
            axes = []
            for f in feats:
                col = X[:, f]
                col = col.detach().cpu().numpy() if hasattr(col, "detach") else np.asarray(col)
                axes.append(pd_grid_axis(col, int(grid_resolution), (lo, hi)))
        else:
            given = [grid] if len(feats) == 1 else list(grid)
            if len(given) != len(feats):
                raise ValueError(f"{len(feats)} features need {len(feats)} grid axes, got {len(given)}")
            axes = [np.asarray(g.detach().cpu().numpy() if hasattr(g, "detach") else g, dtype=np.float32)
                    for g in given]
        if include_missing:
            axes = [np.concatenate([a.reshape(-1), np.array([np.nan], np.float32)]) for a in axes]
        for a in axes:
            if a.ndim != 1 or a.shape[0] == 0:
                raise ValueError(f"a grid axis must be a non-empty vector, got shape {a.shape}")
        want_ice = kind in ("individual", "both")
        want_avg = kind in ("average", "both")
        ice, avg_m, avg_p = predict_ops.partial_dependence(self, X, feats, axes, n_trees=n_trees, weights=w,
                                                           want_ice=want_ice, want_avg=want_avg, device=device)
        shape = tuple(len(a) for a in axes)
        out: dict[str, Any] = {"grid_values": axes, "feature_names": [names[f] for f in feats]}
        if want_avg:
            out["average"] = np.asarray(avg_p if response == "probability" else avg_m, np.float64).reshape(shape)
        if want_ice:
            ind = np.ascontiguousarray(ice.T).reshape((N,) + shape)
            out["individual"] = sigmoid32(ind) if response == "probability" else ind
        return out

    def permutation_importance(self, X, y, features=None, *, n_repeats: int = 5, metric: str = "logloss",
                               sample_weight=None, random_state: int = 0, perm=None, n_trees: int | None = None,
                               device: str | None = None) -> dict[str, Any]:
        """Permutation feature importance (scikit-learn's ``permutation_importance``): how much ``metric`` on the
        labelled rows ``(X, y)`` degrades when a feature's column is shuffled among the rows, everything else
        as in ``X`` (which is not modified). Unlike the gain / cover counts it is measured on the rows given
        here, held-out ones included.

        ``features``: indices or names (default: every model feature). ``metric``: "logloss", "error" or "auc"
        ("auc" is unweighted and refuses ``sample_weight``). ``perm``: int32 [R, N] row indices in [0, N), one
        row per repeat; by default ``n_repeats`` permutations are drawn **once per call and shared by all
        features** (:func:`draw_permutations`: ``n_repeats`` draws instead of ``len(features) * n_repeats``, and
        the features are compared under common random numbers). A ``random_state`` is reproducible per device
        and differs between CPU and GPU; pass ``perm`` where both must agree. ``n_trees``: score that prefix
        of the forest.

        Returns a dict shaped like scikit-learn's Bunch: ``importances`` float64 [n_features, R] = the
        degradation, positive when the feature matters (``score - baseline`` for "logloss" / "error",
        ``baseline - score`` for "auc"), ``importances_mean``, ``importances_std`` (ddof 0), ``baseline_score``,
        ``scores`` [n_features, R], ``features`` (indices), ``feature_names``, ``metric``, ``n_repeats``. On a
        GPU one pass of ``csrc/permimp.hip`` scores every (feature, repeat) job and the baseline; the sums are
        reduced in a fixed order (same input, same bits), and a feature that no tree splits on has importance
        exactly 0.0."""
        from ..ops import predict_ops

        if not isinstance(metric, str) or metric not in EVAL_METRICS:
            raise ValueError(f"unknown metric {metric!r}: expected one of {EVAL_METRICS}")
        names = self.feature_names or [f"f{i}" for i in range(self.num_feature)]
        if features is None:
            features = list(range(self.num_feature))
        elif isinstance(features, (str, int, np.integer)):
            features = [features]
        feats = [self._feature_index(f) for f in features]
        if hasattr(X, "columns") and self.feature_names:
            X = X[self.feature_names]
        if hasattr(X, "to_numpy"):
            X = X.to_numpy(dtype=np.float32, na_value=np.nan)
        if not hasattr(X, "shape") or len(X.shape) != 2:
            X = np.asarray(X, dtype=np.float32)
            if X.ndim != 2:
                raise ValueError(f"X must be [rows, features], got shape {X.shape}")
        N = int(X.shape[0])
        if N == 0 or X.shape[1] < self.num_feature:
            raise ValueError(f"X has shape {tuple(X.shape)}, model needs [rows >= 1, >= {self.num_feature}]")

        def host_vec(v):
            return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32).reshape(-1)

        y32 = host_vec(y)
        w32 = None if sample_weight is None else host_vec(sample_weight)
        if perm is None and int(n_repeats) < 1:
            raise ValueError(f"n_repeats must be at least 1, got {n_repeats}")
        check_perm_inputs(N, y32, w32, (metric,), None if perm is None else tuple(perm.shape))
        d = predict_ops._device_of(X, device)
        if perm is None:
            perm = draw_permutations(N, int(n_repeats), random_state, d if d.type == "cuda" else None)
        base, scores = predict_ops.permutation_scores(self, X, y32, feats, perm, n_trees=n_trees, weights=w32,
                                                      metrics=(metric,), device=d)
        sc = np.asarray(scores[metric], dtype=np.float64)
        imp = (base[metric] - sc) if EVAL_MAXIMIZE[metric] else (sc - base[metric])
        return {"importances": imp, "importances_mean": imp.mean(axis=1) if len(feats) else np.zeros(0),
                "importances_std": imp.std(axis=1) if len(feats) else np.zeros(0),
                "baseline_score": float(base[metric]), "scores": sc, "features": feats,
                "feature_names": [names[f] for f in feats], "metric": metric, "n_repeats": int(sc.shape[1])}

    def accumulated_local_effects(self, X, features=None, *, grid=None, grid_resolution: int = 20,
                                  response: str = "probability", sample_weight=None, centered: bool = True,
                                  n_trees: int | None = None, device: str | None = None):
        """Accumulated local effects (ALE, Apley & Zhu 2020) of one feature or a pair: what the model does as the
        feature moves, measured only where the rows are. Partial dependence scores every row at every grid
        value, which for correlated features is mostly combinations that never occur; ALE moves each row only
        across the interval of ``edges`` it already lies in (everything else as in ``X``, which is not
        modified), averages the prediction differences per interval, accumulates the averages and centres them
        (:func:`ale_host`, :func:`ale_curve`: the definition).

        ``features``: None = every model feature, one curve each (a list of results); an index or a name = one
        curve; a tuple of two = the second-order effect of the pair on the lattice of both edge vectors (the
        pure interaction: both main effects are subtracted; identically 0 when no tree uses both); a list of
        indices, names or pairs = a list of results. ``grid``: explicit edges (one increasing finite vector, a
        pair of vectors for a pair, a list of those -- or None -- for a list); values outside them are clamped
        into the end intervals. By default :func:`ale_edges` builds ``grid_resolution`` intervals of about equal
        row counts from the column's quantiles. ``response``: "probability" (differences of per-row
        probabilities) or "margin" (log-odds). ``sample_weight`` weights the interval means and the centring.
        ``centered=False`` returns the accumulated curve that starts at 0. ``n_trees``: score that prefix of the
        forest.

        Each result is ``{"feature_names": [...], "edges": [float32 vector, ...], "ale": float64 [K + 1] or
        [K1 + 1, K2 + 1] (on the edges), "interval_effect": float64 [K] or [K1, K2] (mean effect per interval
        / cell), "interval_weight": the same shape (sum of weights), "n_missing": rows left out for a NaN in the
        feature(s)}``. An interval without rows has effect 0 and carries the curve forward; in 2-D an empty
        cell is 0 too, where R's ALEPlot fills it from the nearest non-empty cell. A column with fewer than
        two distinct values gives the single point 0.0. On a GPU every feature (pair) is one job of
        ``csrc/ale.hip``: corner margins have the bits of ``predict_margin`` on the substituted rows and the
        interval sums are reduced in a fixed order (same input, same bits)."""
        from ..ops import predict_ops

        if response not in ("probability", "margin"):
            raise ValueError(f"response must be 'probability' or 'margin', got {response!r}")
        single = False
        if features is None:
            items = list(range(self.num_feature))
        elif isinstance(features, (list, np.ndarray)):
            items = list(features)
        else:  # one index or name, or one pair (a tuple)
            items, single = [features], True
        jobs: list[tuple[int, ...]] = []
        for it in items:
            if isinstance(it, (tuple, list)):
                if len(it) != 2:
                    raise ValueError(f"a feature pair has two entries, got {it!r}")
                pair = tuple(self._feature_index(f) for f in it)
                if pair[0] == pair[1]:
                    raise ValueError(f"the two features must differ, got {it!r}")
                jobs.append(pair)
            else:
                jobs.append((self._feature_index(it),))
        names = self.feature_names or [f"f{i}" for i in range(self.num_feature)]
        if hasattr(X, "columns") and self.feature_names:
            X = X[self.feature_names]
        if hasattr(X, "to_numpy"):
            X = X.to_numpy(dtype=np.float32, na_value=np.nan)
        if not hasattr(X, "shape") or len(X.shape) != 2:
            X = np.asarray(X, dtype=np.float32)
            if X.ndim != 2:
                raise ValueError(f"X must be [rows, features], got shape {X.shape}")
        N = int(X.shape[0])
        if N == 0 or X.shape[1] < self.num_feature:
            raise ValueError(f"X has shape {tuple(X.shape)}, model needs [rows >= 1, >= {self.num_feature}]")
        w = None
        if sample_weight is not None:
            w = np.asarray(sample_weight.detach().cpu().numpy() if hasattr(sample_weight, "detach")
                           else sample_weight, dtype=np.float32).reshape(-1)
            if w.shape[0] != N:
                raise ValueError(f"X has {N} rows, sample_weight has {w.shape[0]}")
            if not bool((w >= 0).all()) or not float(np.sum(w, dtype=np.float64)) > 0:  # (NaN fails too)
                raise ValueError("sample_weight must be non-negative with a positive sum")
        if grid is None:
            grids = [None] * len(jobs)
        elif single:
            grids = [grid]
        else:
            grids = list(grid)
            if len(grids) != len(jobs):
                raise ValueError(f"{len(jobs)} features need {len(jobs)} grids, got {len(grids)}")
        if int(grid_resolution) < 1:
            raise ValueError(f"grid_resolution must be at least 1, got {grid_resolution}")
        cols: dict[int, np.ndarray] = {}

        def column(f: int) -> np.ndarray:
            if f not in cols:
                c = X[:, f]
                cols[f] = np.asarray(c.detach().cpu().numpy() if hasattr(c, "detach") else c, dtype=np.float32)
            return cols[f]

        edges: list[list[np.ndarray]] = []
        for feats, g in zip(jobs, grids):
            if g is None:
                edges.append([ale_edges(column(f), int(grid_resolution)) for f in feats])
            else:
                given = [g] if len(feats) == 1 else list(g)
                if len(given) != len(feats):
                    raise ValueError(f"{len(feats)} features need {len(feats)} edge vectors, got {len(given)}")
                edges.append([check_ale_edges(z) for z in given])
        live = [i for i, ez in enumerate(edges) if all(len(z) >= 2 for z in ez)]
        sums = predict_ops.accumulated_local_effects(self, X, [jobs[i] for i in live], [edges[i] for i in live],
                                                     n_trees=n_trees, weights=w, device=device) if live else []
        by_job = dict(zip(live, sums))
        out = []
        for i, (feats, ez) in enumerate(zip(jobs, edges)):
            res: dict[str, Any] = {"feature_names": [names[f] for f in feats], "edges": ez}
            if i in by_job:
                s = by_job[i]
                S = s["sum_prob"] if response == "probability" else s["sum_margin"]
                res["ale"], res["interval_effect"] = ale_curve(S, s["weight"], centered)
                res["interval_weight"] = np.asarray(s["weight"], np.float64)
                res["n_missing"] = int(s["n_missing"])
            else:  # a constant (or empty) column: no interval, the single point 0.0
                shape = tuple(max(len(z) - 1, 0) for z in ez)
                res["ale"] = np.zeros(tuple(max(len(z), 1) for z in ez), np.float64)
                res["interval_effect"] = np.zeros(shape, np.float64)
                res["interval_weight"] = np.zeros(shape, np.float64)
                miss = np.zeros(N, dtype=bool)
                for f in feats:
                    miss |= np.isnan(column(f))
                res["n_missing"] = int(miss.sum())
            out.append(res)
        return out[0] if single else out

    def split_values(self, feature, n_trees: int | None = None) -> np.ndarray:
        """The sorted distinct finite float32 split thresholds of one feature (an index or a name) in the first
        ``n_trees`` trees (default all); empty when no tree splits on it. Along that feature, the others
        fixed, the margin is constant between two consecutive values."""
        f = self._feature_index(feature)
        vals = [t.split_conditions[(~t.is_leaf) & (t.split_indices == f)]
                for t in self.trees[: (self.num_trees if n_trees is None else n_trees)]]
        v = np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, np.float32)
        return np.unique(v[np.isfinite(v)])

    def counterfactuals(self, X, **kw):
        """The nearest change that brings each row's probability to a cutoff:
        :func:`~..explain.recourse.counterfactuals` with this booster as the model."""
        from ..explain.recourse import counterfactuals

        return counterfactuals(self, X, **kw)

    def expected_value(self) -> float:
        """TreeExplainer ``expected_value``: base margin + cover-weighted mean leaf value per tree."""
        tot = 0.0
        for t in self.trees:
            leaf = t.is_leaf
            cov = t.sum_hessian.astype(np.float64)
            tot += float(np.sum(cov[leaf] * t.split_conditions[leaf].astype(np.float64)) / cov[0])
        return self.base_margin + tot

    # ------------------------------------------------------------------- XGBoost document
    def _config_doc(self) -> dict[str, Any]:
        p = {"eta": 0.3, "gamma": 0.0, "max_depth": 6, "min_child_weight": 1.0, "reg_lambda": 1.0,
             "reg_alpha": 0.0, "subsample": 1.0, "colsample_bytree": 1.0, "max_bin": 256,
             "scale_pos_weight": 1.0, "seed": 0}
        p.update({k: v for k, v in self.train_params.items() if v is not None})
        f = _fmt_float
        mono = self.monotone_constraints
        inter = self.interaction_constraints
        return {
            "learner": {
                "generic_param": {"device": "cpu", "fail_on_invalid_gpu_id": "0", "n_jobs": "0", "nthread": "0",
                                  "random_state": str(int(p["seed"])), "seed": str(int(p["seed"])),
                                  "seed_per_iteration": "0", "validate_parameters": "1"},
                "gradient_booster": {
                    "gbtree_model_param": {"num_parallel_tree": "1", "num_trees": str(self.num_trees)},
                    "gbtree_train_param": {"process_type": "default", "tree_method": "hist",
                                           "updater": "grow_quantile_histmaker",
                                           "updater_seq": "grow_quantile_histmaker"},
                    "name": "gbtree",
                    "specified_updater": False,
                    "tree_train_param": {
                        "alpha": f(p["reg_alpha"]), "cache_opt": "1", "colsample_bylevel": "1",
                        "colsample_bynode": "1", "colsample_bytree": f(p["colsample_bytree"]), "eta": f(p["eta"]),
                        "gamma": f(p["gamma"]), "grow_policy": "depthwise",
                        "interaction_constraints": json.dumps(inter) if inter else "",
                        "lambda": f(p["reg_lambda"]), "learning_rate": f(p["eta"]), "max_bin": str(int(p["max_bin"])),
                        "max_cat_threshold": "64", "max_cat_to_onehot": "4", "max_delta_step": "0",
                        "max_depth": str(int(p["max_depth"])), "max_leaves": "0",
                        "min_child_weight": f(p["min_child_weight"]), "min_split_loss": f(p["gamma"]),
                        "monotone_constraints": monotone_string(mono), "refresh_leaf": "1", "reg_alpha": f(p["reg_alpha"]),
                        "reg_lambda": f(p["reg_lambda"]), "sampling_method": "uniform", "sketch_ratio": "2",
                        "sparse_threshold": "0.20000000000000001", "subsample": f(p["subsample"])},
                    "updater": [{"hist_train_param": {"debug_synchronize": "0", "extmem_single_page": "0",
                                                      "max_cached_hist_node": "18446744073709551615"},
                                 "name": "grow_quantile_histmaker"}],
                },
                "learner_model_param": self._lmp(),
                "learner_train_param": {"booster": "gbtree", "disable_default_eval_metric": "0",
                                        "multi_strategy": "one_output_per_tree", "objective": self.objective},
                "metrics": [{"name": "logloss"}],
                "objective": {"name": self.objective,
                              "reg_loss_param": {"scale_pos_weight": f(p["scale_pos_weight"])}},
            },
            "version": [3, 0, 0],
        }

    def _lmp(self) -> dict[str, str]:
        bs = np.format_float_scientific(np.float32(self.base_score), unique=True, exp_digits=1).upper()
        bs = bs.replace("E+", "E")
        if "." in bs:
            mant, ex = bs.split("E")
            mant = mant.rstrip("0").rstrip(".")
            bs = f"{mant}E{ex}"
        return {"base_score": bs, "boost_from_average": "1", "num_class": "0",
                "num_feature": str(self.num_feature), "num_target": "1"}

    def to_doc(self) -> dict[str, Any]:
        spw = self.train_params.get("scale_pos_weight", 1.0)
        model = {
            "learner": {
                "attributes": dict(self.attributes),
                "feature_names": list(self.feature_names or []),
                "feature_types": list(self.feature_types or []),
                "gradient_booster": {
                    "model": {
                        "gbtree_model_param": {"num_parallel_tree": "1", "num_trees": str(self.num_trees)},
                        "iteration_indptr": list(range(self.num_trees + 1)),
                        "tree_info": [0] * self.num_trees,
                        "trees": [t.to_doc(i, self.num_feature) for i, t in enumerate(self.trees)],
                    },
                    "name": "gbtree",
                },
                "learner_model_param": self._lmp(),
                "objective": {"name": self.objective,
                              "reg_loss_param": {"scale_pos_weight": _fmt_float(spw if spw is not None else 1.0)}},
            },
            "version": [3, 0, 0],
        }
        cfg = self.source_config
        if cfg is None or cfg.get("learner", {}).get("gradient_booster", {}).get("gbtree_model_param", {}).get(
                "num_trees") != str(self.num_trees):
            cfg = self._config_doc()
        return {"Config": cfg, "Model": model}

    @classmethod
    def from_doc(cls, doc: dict[str, Any]) -> "Booster":
        model = doc["Model"] if "Model" in doc else doc
        lrn = model["learner"]
        gb = lrn["gradient_booster"]
        if gb.get("name", "gbtree") != "gbtree":
            raise NotImplementedError(f"booster {gb.get('name')!r} not supported")
        trees = [Tree.from_doc(t) for t in gb["model"]["trees"]]
        lmp = lrn["learner_model_param"]
        obj = lrn.get("objective", {}).get("name", "binary:logistic")
        params: dict[str, Any] = {}
        cfg = doc.get("Config", {}).get("learner", {})
        ttp = cfg.get("gradient_booster", {}).get("tree_train_param", {})
        for src, dst, typ in (("eta", "eta", float), ("gamma", "gamma", float), ("max_depth", "max_depth", int),
                              ("min_child_weight", "min_child_weight", float), ("lambda", "reg_lambda", float),
                              ("alpha", "reg_alpha", float), ("subsample", "subsample", float),
                              ("colsample_bytree", "colsample_bytree", float), ("max_bin", "max_bin", int)):
            if src in ttp:
                params[dst] = typ(float(ttp[src]))
        mono = parse_monotone_string(ttp.get("monotone_constraints", "()"))
        if any(mono):
            params["monotone_constraints"] = mono
        inter = parse_interaction_string(ttp.get("interaction_constraints", ""))
        if inter:
            params["interaction_constraints"] = inter
        spw = lrn.get("objective", {}).get("reg_loss_param", {}).get("scale_pos_weight")
        if spw is not None:
            params["scale_pos_weight"] = float(spw)
        seed = cfg.get("generic_param", {}).get("seed")
        if seed is not None:
            params["seed"] = int(seed)
        return cls(trees=trees,
                   feature_names=list(lrn.get("feature_names") or []) or None,
                   feature_types=list(lrn.get("feature_types") or []) or None,
                   base_score=float(np.float32(lmp.get("base_score", "0.5"))),
                   num_feature=int(lmp.get("num_feature", "0")),
                   objective=obj, train_params=params,
                   attributes=dict(lrn.get("attributes") or {}),
                   source_config=doc.get("Config"))

    # --------------------------------------------------------------------------- file I/O
    def save_raw(self, fmt: str = "ubj") -> bytes:
        if fmt == "ubj":
            return ubjson.dumps(self.to_doc())
        if fmt == "json":
            return json.dumps(_jsonable(self.to_doc())).encode()
        raise ValueError(fmt)

    @classmethod
    def load_raw(cls, raw: bytes) -> "Booster":
        raw = bytes(raw)
        if raw[:1] == b"{" and raw[1:2] in (b'"', b" ", b"\n"):
            return cls.from_doc(json.loads(raw.decode()))
        return cls.from_doc(ubjson.loads(raw))

    def save_model(self, path: str | Path) -> None:
        path = Path(path)
        fmt = "json" if path.suffix == ".json" else "ubj"
        path.write_bytes(self.save_raw(fmt))

    @classmethod
    def load_model(cls, path: str | Path) -> "Booster":
        p = Path(path)
        data = p.read_bytes()
        if p.suffix in (".pkl", ".pickle", ".joblib") or data[:1] == b"\x80":
            return load_pickle_bytes(data)[1]
        return cls.load_raw(data)


def monotone_string(mono: Sequence[int] | None) -> str:
    """XGBoost's string form of a constraint vector: ``"(1,0,-1)"``; ``"()"`` without constraints."""
    return "(" + ",".join(str(int(c)) for c in mono) + ")" if mono else "()"


def parse_monotone_string(s: str) -> tuple[int, ...]:
    """``"(1,0,-1)"`` (parentheses optional) -> ``(1, 0, -1)``; ``"()"`` / ``""`` -> ``()``."""
    body = s.strip()
    if body.startswith("(") and body.endswith(")"):
        body = body[1:-1]
    try:
        return tuple(int(tok) for tok in body.split(",") if tok.strip())
    except ValueError:
        raise ValueError(f"monotone_constraints: cannot parse {s!r} (expected a form like '(1,0,-1)')") from None


def parse_interaction_string(s: str) -> list[list[int]]:
    """XGBoost's ``interaction_constraints`` config string ``"[[0, 1], [2, 3]]"`` -> index groups; ``""`` /
    ``"[]"`` -> ``[]``."""
    if not s or not s.strip():
        return []
    try:
        return [[int(i) for i in g] for g in json.loads(s)]
    except (ValueError, TypeError):
        raise ValueError(f"interaction_constraints: cannot parse {s!r} (expected a form like "
                         "'[[0, 1], [2, 3]]')") from None


def _jsonable(v: Any) -> Any:
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


# ---------------------------------------------------------------------------- pickle checkpoint

def sklearn_state(params: dict[str, Any], n_classes: int = 2) -> dict[str, Any]:
    """The XGBClassifier ``__dict__`` in the reference checkpoint's key order."""
    keys = ["n_estimators", "objective", "max_depth", "max_leaves", "max_bin", "grow_policy", "learning_rate",
            "verbosity", "booster", "tree_method", "gamma", "min_child_weight", "max_delta_step", "subsample",
            "sampling_method", "colsample_bytree", "colsample_bylevel", "colsample_bynode", "reg_alpha",
            "reg_lambda", "scale_pos_weight", "base_score", "missing", "num_parallel_tree", "random_state",
            "n_jobs", "monotone_constraints", "interaction_constraints", "importance_type", "device",
            "validate_parameters", "enable_categorical", "feature_types", "feature_weights", "max_cat_to_onehot",
            "max_cat_threshold", "multi_strategy", "eval_metric", "early_stopping_rounds", "callbacks", "kwargs"]
    st: dict[str, Any] = {k: None for k in keys}
    st["objective"] = "binary:logistic"
    st["missing"] = float("nan")
    st["enable_categorical"] = False
    st["kwargs"] = {}
    for k, v in params.items():
        if k in st:
            st[k] = v
    if st.get("scale_pos_weight") is not None:
        st["scale_pos_weight"] = np.float64(st["scale_pos_weight"])
    st["n_classes_"] = n_classes
    return st


def dump_pickle_bytes(booster: Booster, sk_params: dict[str, Any]) -> bytes:
    return safe_pickle.encode_xgb_classifier(sklearn_state(sk_params), booster.save_raw("ubj"))


def load_pickle_bytes(data: bytes) -> tuple[dict[str, Any], Booster]:
    """Load an ``XGBClassifier`` pickle statically (nothing in the file is executed)."""
    st, raw = safe_pickle.read_xgb_classifier_pickle(data)
    return st, Booster.load_raw(raw)


# ------------------------------------------------------------------------ host reference paths

def predict_margin_host(b: Booster, X: np.ndarray, n_trees: int | None = None) -> np.ndarray:
    """NumPy reference traversal: ``x < cond`` goes left, NaN takes ``default_left``; fp32 sums in
    tree order starting from the base margin (XGBoost CPU predictor semantics)."""
    X = np.asarray(X, dtype=np.float32)
    N = X.shape[0]
    out = np.full(N, np.float32(b.base_margin), dtype=np.float32)
    rows = np.arange(N)
    for t in b.trees[: (n_trees if n_trees is not None else b.num_trees)]:
        nid = np.zeros(N, dtype=np.int32)
        while True:
            lc = t.left_children[nid]
            active = lc != -1
            if not active.any():
                break
            f = t.split_indices[nid]
            v = X[rows, np.where(active, f, 0)]
            c = t.split_conditions[nid]
            go_left = np.where(np.isnan(v), t.default_left[nid] == 1, v < c)
            nxt = np.where(go_left, lc, t.right_children[nid])
            nid = np.where(active, nxt, nid)
        out = (out + t.split_conditions[nid]).astype(np.float32)
    return out


EVAL_METRICS = ("logloss", "error", "auc")
EVAL_MAXIMIZE = {"logloss": False, "error": False, "auc": True}


def check_eval_inputs(n_rows: int, y: np.ndarray, w: np.ndarray | None, metrics: Sequence[str],
                      margin_rows: int | None = None) -> tuple[str, ...]:
    """The input checks of :func:`eval_curve_host` / ``predict_ops.eval_curve`` (host arrays; raised
    before anything is computed or launched). Returns the metrics as a tuple."""
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    for m in metrics:
        if m not in EVAL_METRICS:
            raise ValueError(f"unknown eval metric {m!r}: expected one of {EVAL_METRICS}")
    if y.ndim != 1 or y.shape[0] != n_rows:
        raise ValueError(f"X has {n_rows} rows, y has shape {y.shape}")
    if w is not None and (w.ndim != 1 or w.shape[0] != n_rows):
        raise ValueError(f"X has {n_rows} rows, sample_weight has shape {w.shape}")
    if margin_rows is not None and margin_rows != n_rows:
        raise ValueError(f"X has {n_rows} rows, margin has {margin_rows}")
    if n_rows and not bool(((y >= 0) & (y <= 1)).all()):  # (NaN fails too)
        raise ValueError("eval labels must lie in [0, 1]")
    if w is not None and not bool((w >= 0).all()):
        raise ValueError("eval sample weights must be non-negative")
    sw = float(np.sum(w, dtype=np.float64)) if w is not None else float(n_rows)
    if not sw > 0:
        raise ValueError("the eval set's weights sum to zero (or it has no rows)")
    if "auc" in metrics:
        pos = int((y > 0.5).sum())
        if pos == 0 or pos == n_rows:
            raise ValueError("Only one class present in the eval labels: AUC is not defined")
    return metrics


def staged_margins_host(b: Booster, X: np.ndarray, margin: np.ndarray | None = None) -> np.ndarray:
    """Margins after every tree [num_trees, N] float32, summed as :func:`predict_margin_host` sums them
    (fp32, tree order), starting from ``margin`` when given."""
    X = np.asarray(X, dtype=np.float32)
    N = X.shape[0]
    cur = (np.full(N, np.float32(b.base_margin), dtype=np.float32) if margin is None
           else np.asarray(margin, dtype=np.float32).copy())
    out = np.empty((b.num_trees, N), dtype=np.float32)
    rows = np.arange(N)
    for i, t in enumerate(b.trees):
        nid = np.zeros(N, dtype=np.int32)
        while N:
            lc = t.left_children[nid]
            active = lc != -1
            if not active.any():
                break
            v = X[rows, np.where(active, t.split_indices[nid], 0)]
            go_left = np.where(np.isnan(v), t.default_left[nid] == 1, v < t.split_conditions[nid])
            nid = np.where(active, np.where(go_left, lc, t.right_children[nid]), nid)
        cur = (cur + t.split_conditions[nid]).astype(np.float32)
        out[i] = cur
    return out


def eval_curve_host(b: Booster, X: np.ndarray, y, sample_weight=None, metrics: Sequence[str] = ("logloss",),
                    margin: np.ndarray | None = None) -> tuple[dict[str, np.ndarray], np.ndarray]:
    """NumPy form of :meth:`Booster.eval_curve` (CPU path and oracle of the GPU kernel): the fp32 margin
    after every tree as :func:`predict_margin_host` sums it, and from that margin ``m`` in float64
    ``logloss = sum w (log1p(exp(-|m|)) + max(m, 0) - y m) / sum w``, ``error = sum w [(m > 0) != (y > 0.5)]
    / sum w``; ``auc`` is :func:`~..metrics.auc.roc_auc` of each stage (unweighted)."""
    X = np.asarray(X, dtype=np.float32)
    y32 = np.asarray(y, dtype=np.float32).reshape(-1)
    w32 = None if sample_weight is None else np.asarray(sample_weight, dtype=np.float32).reshape(-1)
    metrics = check_eval_inputs(X.shape[0], y32, w32, metrics,
                                None if margin is None else int(np.asarray(margin).shape[0]))
    stages = staged_margins_host(b, X, margin)
    yd = y32.astype(np.float64)
    wd = np.ones_like(yd) if w32 is None else w32.astype(np.float64)
    sw = wd.sum()
    ypos = y32 > np.float32(0.5)
    out = {m: np.empty(b.num_trees, dtype=np.float64) for m in metrics}
    for t in range(b.num_trees):
        m = stages[t].astype(np.float64)
        if "logloss" in out:
            out["logloss"][t] = np.sum(wd * (np.log1p(np.exp(-np.abs(m))) + np.maximum(m, 0.0) - yd * m)) / sw
        if "error" in out:
            out["error"][t] = np.sum(wd * ((stages[t] > 0) != ypos)) / sw
        if "auc" in out:
            from ..metrics.auc import roc_auc

            out["auc"][t] = roc_auc(ypos.astype(np.float64), stages[t])
    final = stages[-1] if b.num_trees else (
        np.full(X.shape[0], np.float32(b.base_margin), dtype=np.float32) if margin is None
        else np.asarray(margin, dtype=np.float32).copy())
    return out, final


def sigmoid32(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m, dtype=np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + np.exp(-m))).astype(np.float32)


# ------------------------------------------------------------------- leaf indices and leaf refresh
def _leaf_of_tree(t: Tree, X: np.ndarray) -> np.ndarray:
    """The node id (index into ``t.left_children``) of the leaf every row of ``X`` reaches, int32 [N]."""
    N = X.shape[0]
    nid = np.zeros(N, dtype=np.int32)
    rows = np.arange(N)
    while N:
        lc = t.left_children[nid]
        active = lc != -1
        if not active.any():
            break
        v = X[rows, np.where(active, t.split_indices[nid], 0)]
        go_left = np.where(np.isnan(v), t.default_left[nid] == 1, v < t.split_conditions[nid])
        nid = np.where(active, np.where(go_left, lc, t.right_children[nid]), nid).astype(np.int32)
    return nid


def predict_leaf_host(b: Booster, X: np.ndarray, n_trees: int | None = None) -> np.ndarray:
    """NumPy form of :meth:`Booster.predict_leaf` (CPU path and oracle of ``csrc/refresh.hip`` k_leaf_index):
    int32 [N, T], the node id in the booster's own numbering of the leaf a row reaches in every tree, walked as
    :func:`predict_margin_host` walks (``x < cond`` goes left, NaN takes ``default_left``)."""
    X = np.asarray(X, dtype=np.float32)
    if X.ndim != 2 or X.shape[1] < b.num_feature:
        raise ValueError(f"X has shape {X.shape}, model needs [rows, >= {b.num_feature}]")
    trees = b.trees[: (n_trees if n_trees is not None else b.num_trees)]
    out = np.empty((X.shape[0], len(trees)), dtype=np.int32)
    for i, t in enumerate(trees):
        out[:, i] = _leaf_of_tree(t, X)
    return out


REFRESH_DEFAULTS = {"eta": 0.3, "reg_lambda": 1.0, "reg_alpha": 0.0, "min_child_weight": 1.0,
                    "scale_pos_weight": 1.0, "seed": 0}
_REFRESH_ALIAS = {"learning_rate": "eta", "lambda": "reg_lambda", "alpha": "reg_alpha", "random_state": "seed"}


def refresh_params(b: Booster, overrides: dict[str, Any]) -> dict[str, Any]:
    """The hyper-parameters of a refresh under their ``train_params`` names (``eta``, ``reg_lambda``,
    ``reg_alpha``, ``min_child_weight``, ``scale_pos_weight``, ``seed``) plus ``grad_bits``: the overrides
    (``learning_rate`` / ``random_state`` and XGBoost's ``lambda`` / ``alpha`` accepted), else the booster's
    ``train_params``, else XGBoost's defaults; ``grad_bits`` defaults to the trainer's 17."""
    from .gbdt_host import GRAD_BITS, QBITS

    given = {}
    for k, v in overrides.items():
        k = _REFRESH_ALIAS.get(k, k)
        if k not in REFRESH_DEFAULTS and k != "grad_bits":
            raise TypeError(f"refresh() got an unexpected keyword argument {k!r}")
        if v is not None:
            given[k] = v
    p: dict[str, Any] = {}
    for k, dflt in REFRESH_DEFAULTS.items():
        v = given.get(k, b.train_params.get(k))
        p[k] = int(v if v is not None else dflt) if k == "seed" else float(v if v is not None else dflt)
    p["grad_bits"] = int(given.get("grad_bits", QBITS))
    if p["grad_bits"] not in GRAD_BITS:
        raise ValueError(f"grad_bits must be one of {GRAD_BITS}")
    p["overridden"] = sorted(k for k in given if k != "grad_bits")
    return p


def check_refresh_inputs(b: Booster, X_shape: tuple, y: np.ndarray, w: np.ndarray | None, dist=None) -> None:
    """Everything a refresh refuses (``ValueError``), for the CPU and the GPU path alike, before anything is
    computed or launched: boosters fitted under monotone constraints (a refresh would ignore the weight
    bounds), data-parallel runs, an objective other than binary:logistic, an ``X`` that is empty or narrower
    than the model, row-count mismatches, labels outside {0, 1}, negative (or NaN) weights and weights that sum
    to 0."""
    if b.monotone_constraints and any(b.monotone_constraints):
        raise ValueError("refresh is not supported for boosters fitted under monotone_constraints: the "
                         "recomputed weights would ignore the constraints' bounds")
    if dist is not None and getattr(dist, "world", 1) > 1:
        raise ValueError("refresh is not supported in data-parallel runs (dist.world > 1)")
    if b.objective != "binary:logistic":
        raise ValueError(f"refresh supports binary:logistic boosters, got {b.objective!r}")
    if len(X_shape) != 2 or X_shape[1] < b.num_feature:
        raise ValueError(f"X has shape {tuple(X_shape)}, model needs [rows, >= {b.num_feature}]")
    n = int(X_shape[0])
    if n == 0:
        raise ValueError("refresh needs at least one row")
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError(f"X has {n} rows, y has shape {y.shape}")
    if not bool(((y == 0) | (y == 1)).all()):
        raise ValueError("refresh labels must be 0 or 1")
    if w is not None:
        if w.ndim != 1 or w.shape[0] != n:
            raise ValueError(f"X has {n} rows, sample_weight has shape {w.shape}")
        if not bool((w >= 0).all()):  # (NaN fails too)
            raise ValueError("refresh sample weights must be non-negative")
        if not float(np.sum(w, dtype=np.float64)) > 0:
            raise ValueError("the refresh sample weights sum to zero")


def refresh_row_weights(y32: np.ndarray, w32: np.ndarray | None, scale_pos_weight: float) -> np.ndarray:
    """Row weights as the trainer forms them: float32 ``sample_weight`` x (float32 ``scale_pos_weight`` for
    y = 1, else 1), the product in float32."""
    pw = np.where(y32 == np.float32(1.0), np.float32(scale_pos_weight), np.float32(1.0)).astype(np.float32)
    return pw if w32 is None else (w32.astype(np.float32) * pw).astype(np.float32)


def refresh_node_stats(sums: np.ndarray, p: dict[str, Any], gscale: float,
                       hscale: float) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(base_weight float32, sum_hessian float32, gain float64, leaf value float32)`` [n] of one tree from
    its int64 node sums ``sums`` [n, 2] (the definition ``csrc/refresh.hip`` k_refresh_finalize follows): with
    ``G = sum gq * (1 / gscale)`` and ``H = sum hq * (1 / hscale)`` in float64 (the trainer's form of the
    division), ``base_weight = _calc_weight(G, H)``, ``sum_hessian = H``, ``gain = _calc_gain(G, H)`` (an
    internal node's ``loss_change`` is ``(gain(left) + gain(right)) - gain(node)``) and the leaf value
    ``float32(base_weight64 * eta)`` -- the trainer's expression for a new leaf."""
    from .gbdt_host import _calc_gain, _thresh_l1

    lam, alpha, mcw = p["reg_lambda"], p["reg_alpha"], p["min_child_weight"]
    G = sums[:, 0].astype(np.float64) * (1.0 / gscale)
    H = sums[:, 1].astype(np.float64) * (1.0 / hscale)
    t = G if alpha == 0.0 else _thresh_l1(G, alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        wgt = np.where((H < mcw) | (H <= 0.0), 0.0, -t / (H + lam))
        gain = _calc_gain(G, H, lam, alpha, mcw)
    return wgt.astype(np.float32), H.astype(np.float32), gain, (wgt * p["eta"]).astype(np.float32)


def _refreshed_booster(b: Booster, trees: list[Tree], p: dict[str, Any]) -> Booster:
    """A new booster around the refreshed trees: names, base score and ``train_params`` kept (the overridden
    hyper-parameters updated), no ``source_config`` (the forest changed)."""
    tp = dict(b.train_params)
    for k in p["overridden"]:
        tp[k] = p[k]
    return Booster(trees=trees, feature_names=list(b.feature_names) if b.feature_names else b.feature_names,
                   feature_types=list(b.feature_types) if b.feature_types else b.feature_types,
                   base_score=b.base_score, num_feature=b.num_feature, objective=b.objective, train_params=tp,
                   attributes=dict(b.attributes), source_config=None)


def refreshed_tree(t: Tree, bw: np.ndarray, sh: np.ndarray, loss: np.ndarray, leaf: np.ndarray,
                   refresh_leaf: bool) -> Tree:
    """``t`` with its statistics replaced (float32 [n] each, in the tree's numbering) and, with
    ``refresh_leaf``, its leaf values; the structure arrays are copies."""
    cond = t.split_conditions.astype(np.float32).copy()
    if refresh_leaf:
        cond[t.is_leaf] = leaf[t.is_leaf]
    return Tree(left_children=t.left_children.copy(), right_children=t.right_children.copy(),
                parents=t.parents.copy(), split_indices=t.split_indices.copy(), split_conditions=cond,
                default_left=t.default_left.copy(), base_weights=np.asarray(bw, np.float32).copy(),
                loss_changes=np.asarray(loss, np.float32).copy(), sum_hessian=np.asarray(sh, np.float32).copy())


def refresh_host(b: Booster, X: np.ndarray, y, sample_weight=None, *, refresh_leaf: bool = True, dist=None,
                 node_sums: list | None = None, **overrides) -> tuple[Booster, np.ndarray]:
    """NumPy form of :meth:`Booster.refresh` (CPU path and oracle of ``csrc/refresh.hip``): XGBoost's
    ``process_type="update", updater="refresh"``. The structure of every tree is kept; tree by tree, in tree
    order, with the float32 margin starting at the base margin:

    1. the rows' gradient pairs are computed and quantised exactly as the trainer does for tree ``t``
       (:func:`~.gbdt_host.gradients_host` with ``subsample = 1``, row key = row index, row weight =
       :func:`refresh_row_weights`, scales = ``quant_scales(max weight, grad_bits)``);
    2. every node on a row's root-to-leaf path receives the row's integers (int64 sums);
    3. :func:`refresh_node_stats` gives ``base_weights``, ``sum_hessian`` and ``loss_changes`` (a node no row
       reaches: weight 0, cover 0) and, with ``refresh_leaf``, the leaf values;
    4. the margin takes the row's (new) leaf value of tree ``t``, a float32 add -- the running sum of
       ``predict_margin(n_trees=t + 1)`` of the model being produced.

    Returns ``(new booster, its margins on X)``; ``b`` is not modified. ``overrides``: see
    :func:`refresh_params`. ``node_sums``: a list that receives every tree's int64 [n, 2] node sums.
    ``ValueError``: see :func:`check_refresh_inputs`. Note: ``base_weights`` is the weight itself, as
    XGBoost's refresh updater stores it; the trainer stores the weight times ``eta``."""
    from .gbdt_host import HostGbdtParams, gradients_host, quant_scales

    X = np.asarray(X, dtype=np.float32)
    y32 = np.asarray(y, dtype=np.float32).reshape(-1)
    w32 = None if sample_weight is None else np.asarray(sample_weight, dtype=np.float32).reshape(-1)
    check_refresh_inputs(b, X.shape, y32, w32, dist)
    p = refresh_params(b, overrides)
    wt = refresh_row_weights(y32, w32, p["scale_pos_weight"])
    gscale, hscale = quant_scales(float(wt.max()), p["grad_bits"])
    hp = HostGbdtParams(max_depth=0, eta=p["eta"], reg_lambda=p["reg_lambda"], reg_alpha=p["reg_alpha"], gamma=0.0,
                        min_child_weight=p["min_child_weight"], subsample=1.0, seed=p["seed"], gscale=gscale,
                        hscale=hscale, quant=True, qbits=p["grad_bits"])
    N = X.shape[0]
    margin = np.full(N, np.float32(b.base_margin), dtype=np.float32)
    trees = []
    for ti, t in enumerate(b.trees):
        leaf = _leaf_of_tree(t, X)
        gq, hq = gradients_host(margin, y32, wt, hp, ti)
        sums = np.zeros((t.num_nodes, 2), dtype=np.int64)
        np.add.at(sums[:, 0], leaf, gq)
        np.add.at(sums[:, 1], leaf, hq)
        # internal nodes = the sum of their two children, children first (any numbering: post-order)
        order, stack = [], [0]
        while stack:
            j = stack.pop()
            order.append(j)
            if t.left_children[j] != -1:
                stack += [int(t.left_children[j]), int(t.right_children[j])]
        for j in reversed(order):
            if t.left_children[j] != -1:
                sums[j] = sums[t.left_children[j]] + sums[t.right_children[j]]
        if node_sums is not None:
            node_sums.append(sums)
        bw, sh, gain, lv = refresh_node_stats(sums, p, gscale, hscale)
        split = ~t.is_leaf
        loss = np.zeros(t.num_nodes, dtype=np.float32)
        loss[split] = ((gain[t.left_children[split]] + gain[t.right_children[split]]) - gain[split]).astype(np.float32)
        nt = refreshed_tree(t, bw, sh, loss, lv, refresh_leaf)
        trees.append(nt)
        margin = (margin + nt.split_conditions[leaf]).astype(np.float32)
    return _refreshed_booster(b, trees, p), margin


# ------------------------------------------------------------------------- partial dependence
def partial_dependence_host(b: Booster, X: np.ndarray, feats: Sequence[int], grids: Sequence[np.ndarray],
                            n_trees: int | None = None,
                            weights: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of partial dependence / ICE (CPU path and oracle of ``csrc/pdp.hip``): for every grid
    point ``k = i1 * G2 + i2`` a copy of ``X`` with column ``feats[0]`` set to ``grids[0][i1]`` (and
    ``feats[1]`` to ``grids[1][i2]``; NaN = missing) is scored with :func:`predict_margin_host`.
    Returns ``(ice, avg_margin, avg_prob)``: the margins [G, N] float32 and, per grid point, the weighted
    means over the rows of the margin and of ``1 / (1 + exp(-m))`` (float64 from the float32 margin),
    summed with ``math.fsum``. ``X`` is not modified."""
    X = np.asarray(X, dtype=np.float32)
    N = X.shape[0]
    grids = [np.asarray(g, dtype=np.float32) for g in grids]
    G2 = len(grids[1]) if len(feats) == 2 else 1
    G = len(grids[0]) * G2
    wd = np.ones(N, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    sw = math.fsum(wd)
    ice = np.empty((G, N), dtype=np.float32)
    avg_m = np.empty(G, dtype=np.float64)
    avg_p = np.empty(G, dtype=np.float64)
    Xs = X.copy()
    for k in range(G):
        i1, i2 = divmod(k, G2)
        Xs[:, feats[0]] = grids[0][i1]
        if len(feats) == 2:
            Xs[:, feats[1]] = grids[1][i2]
        ice[k] = predict_margin_host(b, Xs, n_trees)
        m = ice[k].astype(np.float64)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-m))
        avg_m[k] = math.fsum(wd * m) / sw
        avg_p[k] = math.fsum(wd * p) / sw
    return ice, avg_m, avg_p


# ------------------------------------------------------------------------ counterfactual recourse
RECOURSE_EMPTY_BITS = 0x7FC00000  # margin bits of an empty result (idx = -1)


def check_recourse_args(b: Booster, feats, cands, win, dirs) -> tuple[list[int], list[np.ndarray], np.ndarray,
                                                                      np.ndarray]:
    """The arguments of a recourse scan in canonical form, ``ValueError`` otherwise: ``feats`` A >= 1 feature
    indices inside the model; ``cands`` one ascending NaN-free float32 vector per feature (may be empty);
    ``win`` int32 [A, 2] inclusive candidate-index windows (default: every candidate; ``jlo > jhi`` is empty,
    any other window must lie inside its feature's candidates); ``dirs`` int32 [A] in {-1, 0, +1} (default 0)."""
    feats = [int(f) for f in feats]
    A = len(feats)
    if A < 1:
        raise ValueError("a recourse scan needs at least one actionable feature")
    for f in feats:
        if not 0 <= f < b.num_feature:
            raise ValueError(f"feature index {f} outside [0, {b.num_feature})")
    if len(cands) != A:
        raise ValueError(f"{A} features need {A} candidate tables, got {len(cands)}")
    out = []
    for cv in cands:
        cv = np.ascontiguousarray(np.asarray(cv), dtype=np.float32)
        if cv.ndim != 1 or np.isnan(cv).any() or (np.diff(cv) < 0).any():
            raise ValueError("a candidate table must be an ascending vector without NaN")
        out.append(cv)
    if win is None:
        win = [(0, len(cv) - 1) for cv in out]
    win = np.ascontiguousarray(np.asarray(win), dtype=np.int32).reshape(-1, 2)
    dirs = np.zeros(A, np.int32) if dirs is None else np.ascontiguousarray(np.asarray(dirs), dtype=np.int32).reshape(-1)
    if win.shape[0] != A or dirs.shape[0] != A:
        raise ValueError(f"{A} features need {A} windows and {A} directions")
    for a in range(A):
        jlo, jhi = int(win[a, 0]), int(win[a, 1])
        if jlo <= jhi and (jlo < 0 or jhi >= len(out[a])):
            raise ValueError(f"window [{jlo}, {jhi}] outside the {len(out[a])} candidates of feature {feats[a]}")
        if int(dirs[a]) not in (-1, 0, 1):
            raise ValueError(f"a direction is -1, 0 or +1, got {int(dirs[a])}")
    return feats, out, win, dirs


def recourse_scan_host(b: Booster, X: np.ndarray, feats: Sequence[int], cands: Sequence[np.ndarray], win=None,
                       dirs=None, target: float = 0.0,
                       n_trees: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """The definition of the recourse scan (CPU path and oracle of ``csrc/recourse.hip``). For row ``r`` and
    actionable ``a`` (feature ``feats[a]``, ascending candidates ``cands[a]``, window ``[jlo, jhi] = win[a]``,
    direction ``dirs[a]``): ``c = (number of candidates <= x) - 1`` is the row's own position and never a
    result; ``m_j`` is :func:`predict_margin_host` of the row with that one feature replaced by candidate
    ``j``. Returns ``(idx, margin)``, int32 and float32 ``[N, A, 3]``:

    * slot 0, down: the largest ``j < c`` in the window with ``m_j <= target`` (not when ``dirs[a] == +1``);
    * slot 1, up: the smallest ``j > c`` in the window with ``m_j <= target`` (not when ``dirs[a] == -1``);
    * slot 2, best: the ``j != c`` in the window that the direction allows with the smallest ``m_j``; ties go
      to the smaller ``|j - c|``, then to the smaller ``j``.

    An empty result is ``idx = -1`` with the margin bits ``0x7FC00000``; a NaN ``x`` makes all three empty.
    ``X`` is not modified."""
    X = np.asarray(X, dtype=np.float32)
    feats, cands, win, dirs = check_recourse_args(b, feats, cands, win, dirs)
    N, A = X.shape[0], len(feats)
    target = np.float32(target)
    idx = np.full((N, A, 3), -1, dtype=np.int32)
    margin = np.full((N, A, 3), RECOURSE_EMPTY_BITS, dtype=np.uint32).view(np.float32)
    per_call = max(1, 65536 // max(N, 1))  # candidates scored by one predict_margin_host call
    for a, f in enumerate(feats):
        x = X[:, f]
        live = ~np.isnan(x)
        c = np.searchsorted(cands[a], x, side="right").astype(np.int64) - 1
        best_m = np.zeros(N, np.float32)
        jlo = int(win[a, 0])
        for j in range(jlo, int(win[a, 1]) + 1):  # ascending: later candidates win only if strictly better
            if (j - jlo) % per_call == 0:  # the substituted copies of X for the next candidates, one below the other
                vals = cands[a][j:min(j + per_call, int(win[a, 1]) + 1)]
                Xs = np.repeat(X[None, :, :], len(vals), axis=0)
                Xs[:, :, f] = vals[:, None]
                block = predict_margin_host(b, Xs.reshape(-1, X.shape[1]), n_trees).reshape(len(vals), N)
            m = block[(j - jlo) % per_call]
            below = j < c
            ok = live & (j != c) & np.where(below, dirs[a] != 1, dirs[a] != -1)
            hit = ok & (m <= target)
            dn = hit & below
            up = hit & ~below & (idx[:, a, 1] < 0)
            bj = idx[:, a, 2].astype(np.int64)
            be = ok & ((bj < 0) | (m < best_m) | ((m == best_m) & (np.abs(j - c) < np.abs(bj - c))))
            for slot, sel in ((0, dn), (1, up), (2, be)):
                idx[sel, a, slot] = j
                margin[sel, a, slot] = m[sel]
            best_m = np.where(be, m, best_m)
    return idx, margin


# ---------------------------------------------------------------------- permutation importance
def draw_permutations(n_rows: int, n_repeats: int, random_state: int = 0, device=None):
    """The ``n_repeats`` row permutations of one :meth:`Booster.permutation_importance` call, int32
    [n_repeats, n_rows]. CPU: ``np.random.default_rng(random_state)`` and one ``rng.permutation`` per repeat
    (a NumPy array). A CUDA ``device``: ``torch.randperm`` with a generator of that device seeded with
    ``random_state``, one per repeat (a tensor on the device; nothing crosses the host). A seed is
    reproducible per device and differs between the two."""
    if int(n_repeats) < 1:
        raise ValueError(f"n_repeats must be at least 1, got {n_repeats}")
    if device is not None and str(device).startswith("cuda"):
        import torch

        gen = torch.Generator(device=device).manual_seed(int(random_state))
        return torch.stack([torch.randperm(int(n_rows), generator=gen, dtype=torch.int32, device=device)
                            for _ in range(int(n_repeats))])
    rng = np.random.default_rng(random_state)
    return np.stack([rng.permutation(int(n_rows)) for _ in range(int(n_repeats))]).astype(np.int32)


def check_perm_inputs(n_rows: int, y: np.ndarray, w: np.ndarray | None, metrics: Sequence[str],
                      perm_shape: tuple | None = None) -> tuple[str, ...]:
    """The input checks of permutation importance beyond the contents of ``perm`` (host arrays; raised before
    anything is computed or launched): those of :func:`check_eval_inputs`, "auc" with weights, and the shape
    of ``perm`` ([R >= 1, n_rows])."""
    metrics = check_eval_inputs(n_rows, y, w, metrics)
    if "auc" in metrics and w is not None:
        raise ValueError("the 'auc' metric is unweighted: pass sample_weight or metric='auc', not both")
    if perm_shape is not None and (len(perm_shape) != 2 or perm_shape[0] < 1 or perm_shape[1] != n_rows):
        raise ValueError(f"perm must be int32 [R >= 1, {n_rows}], got shape {tuple(perm_shape)}")
    return metrics


def metric_terms_host(margin: np.ndarray, y32: np.ndarray, w32: np.ndarray | None,
                      metrics: Sequence[str]) -> dict[str, float]:
    """The metrics of one job from its fp32 margins, as ``csrc/evalcurve.hip`` defines them (float64 terms
    from the float32 margin; exact ``math.fsum`` sums)."""
    out: dict[str, float] = {}
    m = margin.astype(np.float64)
    wd = np.ones(m.shape[0], dtype=np.float64) if w32 is None else w32.astype(np.float64)
    sw = math.fsum(wd)
    ypos = y32 > np.float32(0.5)
    if "logloss" in metrics:
        out["logloss"] = math.fsum(wd * (np.log1p(np.exp(-np.abs(m))) + np.maximum(m, 0.0)
                                         - y32.astype(np.float64) * m)) / sw
    if "error" in metrics:
        out["error"] = math.fsum(wd * ((margin > 0) != ypos)) / sw
    if "auc" in metrics:
        from ..metrics.auc import roc_auc

        out["auc"] = float(roc_auc(ypos.astype(np.float64), margin))
    return out


def permutation_scores_host(b: Booster, X: np.ndarray, y, feats: Sequence[int], perm: np.ndarray,
                            n_trees: int | None = None, sample_weight=None,
                            metrics: Sequence[str] = ("logloss",)) -> tuple[dict[str, float], dict[str, np.ndarray]]:
    """The definition of the permutation-importance scores (CPU path and oracle of ``csrc/permimp.hip``): job
    ``(i, r)`` scores a copy of ``X`` whose column ``feats[i]`` is ``X[perm[r], feats[i]]`` with
    :func:`predict_margin_host`; the baseline scores ``X`` itself. NaN is swapped in like any value.
    Returns ``(baseline, scores)``: ``{metric: float}`` and ``{metric: float64 [len(feats), R]}`` with
    ``logloss = sum w (log1p(exp(-|m|)) + max(m, 0) - y m) / sum w`` and ``error = sum w [(m > 0) != (y > 0.5)]
    / sum w`` in float64 from the float32 margin ``m``, and ``auc`` = :func:`~..metrics.auc.roc_auc` of
    ``(y > 0.5, m)`` (unweighted). ``ValueError`` for a ``perm`` that is not [R >= 1, N] with entries in
    [0, N), "auc" with weights or with one class, an unknown metric, and row-count mismatches. ``X`` is not
    modified."""
    X = np.asarray(X, dtype=np.float32)
    N = X.shape[0]
    y32 = np.asarray(y, dtype=np.float32).reshape(-1)
    w32 = None if sample_weight is None else np.asarray(sample_weight, dtype=np.float32).reshape(-1)
    perm = np.asarray(perm)
    metrics = check_perm_inputs(N, y32, w32, metrics, perm.shape)
    if perm.dtype.kind not in "iu" or int(perm.min()) < 0 or int(perm.max()) >= N:
        raise ValueError(f"perm must hold integer row indices in [0, {N})")
    feats = [int(f) for f in feats]
    for f in feats:
        if not 0 <= f < b.num_feature:
            raise ValueError(f"feature index {f} outside [0, {b.num_feature})")
    R = perm.shape[0]
    base = metric_terms_host(predict_margin_host(b, X, n_trees), y32, w32, metrics)
    scores = {m: np.empty((len(feats), R), dtype=np.float64) for m in metrics}
    Xs = X.copy()
    for i, f in enumerate(feats):
        for r in range(R):
            Xs[:, f] = X[perm[r], f]
            got = metric_terms_host(predict_margin_host(b, Xs, n_trees), y32, w32, metrics)
            for m in metrics:
                scores[m][i, r] = got[m]
        Xs[:, f] = X[:, f]
    return base, scores


def pd_grid_axis(col: np.ndarray, grid_resolution: int, percentiles: tuple[float, float]) -> np.ndarray:
    """One axis of a partial-dependence grid by scikit-learn's rule, from the non-NaN values of a column: its
    unique values when there are fewer than ``grid_resolution`` of them, else ``grid_resolution`` points from
    the lower to the upper percentile (linear interpolation), as float32."""
    vals = col[~np.isnan(col)]
    if vals.size == 0:
        raise ValueError("the column has no non-missing value: pass an explicit grid")
    uniq = np.unique(vals)
    if uniq.shape[0] < grid_resolution:
        return uniq.astype(np.float32)
    lo, hi = (np.quantile(vals, q) for q in percentiles)
    return np.linspace(lo, hi, grid_resolution).astype(np.float32)


# -------------------------------------------------------------------- accumulated local effects
def check_ale_edges(z) -> np.ndarray:
    """Interval edges as a float32 vector: finite, strictly increasing, at least two. ``ValueError`` otherwise."""
    z = np.asarray(z.detach().cpu().numpy() if hasattr(z, "detach") else z)
    if z.ndim != 1 or z.shape[0] < 2:
        raise ValueError(f"ALE edges must be a vector of at least 2 values, got shape {z.shape}")
    z = np.ascontiguousarray(z, dtype=np.float32)
    if not bool(np.isfinite(z).all()) or not bool((z[1:] > z[:-1]).all()):
        raise ValueError("ALE edges must be finite and strictly increasing (as float32)")
    return z


def ale_edges(col: np.ndarray, grid_resolution: int = 20) -> np.ndarray:
    """The default interval edges of a column for ALE, float32 and strictly increasing, from its finite values
    (NaN rows are left out of ALE, +-inf rows fall in the end intervals): the distinct values when there are
    at most ``grid_resolution + 1`` of them, else the distinct float32 values of ``np.quantile(vals,
    linspace(0, 1, grid_resolution + 1))`` (intervals of about equal row counts). Fewer than two values come
    back for a constant or empty column: there is no interval then."""
    if int(grid_resolution) < 1:
        raise ValueError(f"grid_resolution must be at least 1, got {grid_resolution}")
    col = np.asarray(col, dtype=np.float32).reshape(-1)
    vals = col[np.isfinite(col)]
    uniq = np.unique(vals)
    if uniq.shape[0] <= int(grid_resolution) + 1:
        return uniq.astype(np.float32)
    q = np.quantile(vals.astype(np.float64), np.linspace(0.0, 1.0, int(grid_resolution) + 1))
    return np.unique(q.astype(np.float32))


def ale_interval_host(z: np.ndarray, x: np.ndarray) -> np.ndarray:
    """The interval ``k`` in [1, K] of every value of ``x`` among the edges ``z[0..K]``: ``clamp(searchsorted(z,
    x, "left"), 1, K)``, so ``z[k-1] < x <= z[k]``; values at or below ``z[0]`` (``-inf``) fall in interval 1,
    values beyond ``z[K]`` (``+inf``) in interval K. NaN gives 1 (the caller leaves such rows out)."""
    z = np.asarray(z, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    k = np.searchsorted(z, np.where(np.isnan(x), -np.inf, x).astype(np.float32), side="left")
    return np.clip(k, 1, len(z) - 1).astype(np.int64)


def ale_host(b: Booster, X: np.ndarray, feats: Sequence[int], edges: Sequence[np.ndarray],
             n_trees: int | None = None, weights: np.ndarray | None = None) -> dict[str, Any]:
    """The definition of the accumulated-local-effects sums (CPU path and oracle of ``csrc/ale.hip``) for one
    feature or a pair. A row lies in interval ``k`` of ``edges[0]`` (:func:`ale_interval_host`; with two
    features in cell ``(k, l)``) and is scored with :func:`predict_margin_host` at the corners: corner
    ``c = i1 + 2 i2`` has ``x[feats[0]] = edges[0][k - 1 + i1]`` (and ``x[feats[1]] = edges[1][l - 1 + i2]``),
    everything else as in ``X``. The row's effect is ``hi - lo`` (1-D) or ``(c3 - c2) - (c1 - c0)`` (2-D), in
    margin units from the float32 corner margins widened to float64 and in probability units from ``1 / (1 +
    exp(-m))`` per corner in float64. Rows with NaN in a feature of the job are left out and counted.

    Returns ``{"corners": float32 [C, N], "cell": int64 [N] (k - 1, or (k - 1) * K2 + (l - 1); -1 = left
    out), "sum_margin", "sum_prob", "weight": float64 [K1] or [K1, K2] (sum w effect, sum w per interval,
    ``math.fsum``), "n_missing"}``. ``X`` is not modified."""
    X = np.asarray(X, dtype=np.float32)
    N = X.shape[0]
    feats = [int(f) for f in feats]
    if len(feats) not in (1, 2) or len(edges) != len(feats):
        raise ValueError(f"ALE takes one or two features with one edge vector each, got {len(feats)} and {len(edges)}")
    for f in feats:
        if not 0 <= f < b.num_feature:
            raise ValueError(f"feature index {f} outside [0, {b.num_feature})")
    if len(feats) == 2 and feats[0] == feats[1]:
        raise ValueError(f"the two features must differ, got {feats}")
    edges = [check_ale_edges(z) for z in edges]
    Ks = [len(z) - 1 for z in edges]
    wd = np.ones(N, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    if wd.shape[0] != N:
        raise ValueError(f"X has {N} rows, weights has {wd.shape[0]}")
    miss = np.zeros(N, dtype=bool)
    ks = []
    for f, z in zip(feats, edges):
        miss |= np.isnan(X[:, f])
        ks.append(ale_interval_host(z, X[:, f]))
    C = 1 << len(feats)
    corners = np.empty((C, N), dtype=np.float32)
    Xs = X.copy()
    for c in range(C):
        for a, (f, z) in enumerate(zip(feats, edges)):
            Xs[:, f] = z[ks[a] - 1 + ((c >> a) & 1)]
        corners[c] = predict_margin_host(b, Xs, n_trees)
    m = corners.astype(np.float64)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-m))
    if C == 2:
        dm, dp = m[1] - m[0], p[1] - p[0]
        cell = ks[0] - 1
    else:
        dm, dp = (m[3] - m[2]) - (m[1] - m[0]), (p[3] - p[2]) - (p[1] - p[0])
        cell = (ks[0] - 1) * Ks[1] + (ks[1] - 1)
    cell = np.where(miss, -1, cell)
    ncell = int(np.prod(Ks))
    sm, sp, sw = np.zeros(ncell), np.zeros(ncell), np.zeros(ncell)
    order = np.argsort(cell, kind="stable")
    bounds = np.searchsorted(cell[order], np.arange(ncell + 1))
    for c in range(ncell):
        idx = order[bounds[c]:bounds[c + 1]]
        if idx.size:
            sm[c] = math.fsum(wd[idx] * dm[idx])
            sp[c] = math.fsum(wd[idx] * dp[idx])
            sw[c] = math.fsum(wd[idx])
    shape = tuple(Ks)
    return {"corners": corners, "cell": cell, "sum_margin": sm.reshape(shape), "sum_prob": sp.reshape(shape),
            "weight": sw.reshape(shape), "n_missing": int(miss.sum())}


def ale_curve(S: np.ndarray, W: np.ndarray, centered: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """``(ale, interval_effect)`` from the per-interval sums ``S = sum w effect`` and ``W = sum w`` (float64 [K]
    or [K1, K2]); shared by the CPU and the GPU path.

    1-D: ``e_k = S_k / W_k`` (0 for an empty interval, which carries the curve forward), ``A[0] = 0``,
    ``A[k] = A[k-1] + e_k`` on the K + 1 edges and ``ale = A - sum_k W_k (A[k-1] + A[k]) / 2 / sum_k W_k``.

    2-D (Apley & Zhu, eq. 13-16): the cell means (0 for an empty cell; ALEPlot fills empty cells from the
    nearest non-empty one instead) are accumulated along both axes on the (K1 + 1) x (K2 + 1) lattice,
    ``A[0, :] = A[:, 0] = 0``; the accumulated main effect of ``A`` along each axis is subtracted,
    ``g1[k] = sum_{k' <= k} sum_l W_k'l ((A[k',l] - A[k'-1,l]) + (A[k',l-1] - A[k'-1,l-1])) / 2 / sum_l W_k'l``
    (a row of cells without weight adds nothing) and ``g2`` likewise; then the W-weighted mean over the cells
    of the four-corner average. What is left is the pure second-order effect.

    ``centered=False`` returns ``A`` itself."""
    S = np.asarray(S, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    e = np.divide(S, W, out=np.zeros_like(S), where=W > 0)
    if S.ndim == 1:
        A = np.concatenate([[0.0], np.cumsum(e)])
        if centered and W.sum() > 0:
            A = A - float((W * (A[:-1] + A[1:]) / 2).sum() / W.sum())
        return A, e
    K1, K2 = S.shape
    A = np.zeros((K1 + 1, K2 + 1))
    A[1:, 1:] = np.cumsum(np.cumsum(e, axis=0), axis=1)
    if not centered or W.sum() <= 0:
        return A, e
    d1 = ((A[1:, 1:] - A[:-1, 1:]) + (A[1:, :-1] - A[:-1, :-1])) / 2      # [K1, K2]: along axis 1, cell (k, l)
    d2 = ((A[1:, 1:] - A[1:, :-1]) + (A[:-1, 1:] - A[:-1, :-1])) / 2
    w1, w2 = W.sum(axis=1), W.sum(axis=0)
    g1 = np.concatenate([[0.0], np.cumsum(np.divide((W * d1).sum(axis=1), w1, out=np.zeros(K1), where=w1 > 0))])
    g2 = np.concatenate([[0.0], np.cumsum(np.divide((W * d2).sum(axis=0), w2, out=np.zeros(K2), where=w2 > 0))])
    A = A - g1[:, None] - g2[None, :]
    four = (A[:-1, :-1] + A[:-1, 1:] + A[1:, :-1] + A[1:, 1:]) / 4
    return A - float((W * four).sum() / W.sum()), e


def treeshap_host(b: Booster, X: np.ndarray) -> np.ndarray:
    """Exact path-dependent TreeSHAP (Lundberg et al., Algorithm 2) in NumPy; oracle for the GPU kernel.

    Reproduces ``shap.TreeExplainer(model).shap_values(X)`` for XGBoost models (node covers =
    ``sum_hessian``), as called by the reference at src/api/cobalt_fast_api.py:46,100.
    """
    X = np.asarray(X, dtype=np.float32)
    N, F = X.shape
    phi = np.zeros((N, F), dtype=np.float64)
    for t in b.trees:
        cov = t.sum_hessian.astype(np.float64)
        val = t.split_conditions.astype(np.float64)
        for r in range(N):
            _treeshap_row(t, cov, val, X[r], phi[r])
    return phi


def _treeshap_row(t: Tree, cov, val, x, phi) -> None:
    # path entries: feature index, zero fraction, one fraction, pweight
    def extend(m, pz, po, pi):
        feats, zs, os_, ws = m
        l = len(feats)
        feats = feats + [pi]
        zs = zs + [pz]
        os_ = os_ + [po]
        ws = ws + [1.0 if l == 0 else 0.0]
        for i in range(l - 1, -1, -1):
            ws[i + 1] += po * ws[i] * (i + 1) / (l + 1)
            ws[i] = pz * ws[i] * (l - i) / (l + 1)
        return feats, zs, os_, ws

    def unwind(m, i):
        feats, zs, os_, ws = m
        l = len(feats) - 1
        n = ws[l]
        ws = list(ws)
        if os_[i] != 0:
            for j in range(l - 1, -1, -1):
                tmp = ws[j]
                ws[j] = n * (l + 1) / ((j + 1) * os_[i])
                n = tmp - ws[j] * zs[i] * (l - j) / (l + 1)
        else:
            for j in range(l - 1, -1, -1):
                ws[j] = (ws[j] * (l + 1)) / (zs[i] * (l - j))
        feats = feats[:i] + feats[i + 1:]
        zs = zs[:i] + zs[i + 1:]
        os_ = os_[:i] + os_[i + 1:]
        ws = ws[:l]
        return feats, zs, os_, ws

    def unwound_sum(m, i):
        feats, zs, os_, ws = m
        l = len(feats) - 1
        total = 0.0
        if os_[i] != 0:
            n = ws[l]
            for j in range(l - 1, -1, -1):
                tmp = n / ((j + 1) * os_[i])
                total += tmp
                n = ws[j] - tmp * zs[i] * (l - j)
            return total * (l + 1)
        for j in range(l - 1, -1, -1):
            total += ws[j] / (zs[i] * (l - j))
        return total * (l + 1)

    def recurse(j, m, pz, po, pi):
        if pz == 0 and po == 0:
            # a zero-cover branch the row does not take: every subset weight below it has the factor
            # pz or po, so it contributes exactly 0 (UNWIND would divide by pz)
            return
        m = extend(m, pz, po, pi)
        if t.left_children[j] == -1:
            feats, zs, os_, ws = m
            for i in range(1, len(feats)):
                w = unwound_sum(m, i)
                phi[feats[i]] += w * (os_[i] - zs[i]) * val[j]
            return
        f = int(t.split_indices[j])
        v = x[f]
        left, right = int(t.left_children[j]), int(t.right_children[j])
        if np.isnan(v):
            hot = left if t.default_left[j] else right
        else:
            hot = left if v < t.split_conditions[j] else right
        cold = right if hot == left else left
        iz, io = 1.0, 1.0
        feats = m[0]
        k = next((q for q in range(1, len(feats)) if feats[q] == f), None)
        if k is not None:
            iz, io = m[1][k], m[2][k]
            m = unwind(m, k)
        recurse(hot, m, iz * cov[hot] / cov[j], io, f)
        recurse(cold, m, iz * cov[cold] / cov[j], 0.0, f)

    recurse(0, ([], [], [], []), 1.0, 1.0, -1)


def iter_leaf_paths(t: Tree) -> Iterable[tuple[int, list[tuple[int, int, bool]]]]:
    """Yield (leaf node, [(node, feature, went_left)]) for every root->leaf path."""
    stack = [(0, [])]
    while stack:
        j, path = stack.pop()
        if t.left_children[j] == -1:
            yield j, path
            continue
        f = int(t.split_indices[j])
        stack.append((int(t.right_children[j]), path + [(j, f, False)]))
        stack.append((int(t.left_children[j]), path + [(j, f, True)]))


def merged_leaf_paths(t: Tree) -> Iterable[tuple[float, list[tuple[int, np.float32, np.float32, bool, float]]]]:
    """Yield (leaf value, [(feature, lo, hi, nan_ok, zero fraction)]) per leaf path with the splits on
    one feature merged into one element: a row follows the element iff ``x >= lo and not x >= hi``
    (``hi`` is NaN when no split bounds the feature from above, so ``x = +inf`` follows; NaN rows: iff
    every merged split sends missing values this way); the zero fraction is the product of the
    cover ratios of the merged splits. Elements are in order of first occurrence."""
    cov = t.sum_hessian.astype(np.float64)
    for leaf, path in iter_leaf_paths(t):
        merged: dict[int, list] = {}
        for node, f, went_left in path:
            child = int(t.left_children[node] if went_left else t.right_children[node])
            m = merged.setdefault(f, [np.float32(-np.inf), np.float32(np.nan), True, 1.0])
            thr = t.split_conditions[node]
            if went_left:
                m[1] = thr if np.isnan(m[1]) else min(m[1], thr)
            else:
                m[0] = max(m[0], thr)
            m[2] = m[2] and (bool(t.default_left[node]) == went_left)
            m[3] *= cov[child] / cov[node]
        yield float(t.split_conditions[leaf]), [(f, *m) for f, m in merged.items()]


def _paths_by_length(b: Booster) -> list[tuple[int, tuple]]:
    """The merged leaf paths of all trees grouped by their number of elements k >= 1, as arrays
    (leaf [P], feature / lo / hi / nan_ok / zero [P, k]); kept with the booster while its trees stay."""
    cache = b.__dict__.setdefault("_host_path_cache", {})
    key = tuple(id(t) for t in b.trees)
    if cache.get("key") != key:
        by_len: dict[int, list] = {}
        for t in b.trees:
            for leaf, elems in merged_leaf_paths(t):
                by_len.setdefault(len(elems), []).append((leaf, elems))
        groups = []
        for k, paths in sorted(by_len.items()):
            if k == 0:
                continue
            col = lambda c, dt: np.array([[e[c] for e in p[1]] for p in paths], dtype=dt)  # noqa: E731
            groups.append((k, (np.array([p[0] for p in paths], dtype=np.float64), col(0, np.int64),
                               col(1, np.float32), col(2, np.float32), col(3, bool), col(4, np.float64))))
        cache.update(key=key, groups=groups)
    return cache["groups"]


def _extend_sum(z: list, o: list) -> Any:
    """Sum of the permutation weights EXTEND builds over elements with zero / one fractions ``z`` / ``o``
    (arrays broadcast against each other): sum_S |S|! (m - |S|)! / (m + 1)! prod_{S} o prod_{not S} z."""
    w = [1.0]
    for l, (ze, oe) in enumerate(zip(z, o), start=1):
        w.append(0.0)
        for j in range(l - 1, -1, -1):
            w[j + 1] = w[j + 1] + oe * w[j] * ((j + 1) / (l + 1))
            w[j] = ze * w[j] * ((l - j) / (l + 1))
    tot = w[0]
    for x in w[1:]:
        tot = tot + x
    return tot


def treeshap_interactions_host(b: Booster, X: np.ndarray) -> np.ndarray:
    """Path-dependent TreeSHAP interaction values [N, F, F] float64 in margin space (covers =
    ``sum_hessian``): ``shap.TreeExplainer.shap_interaction_values``; CPU path of
    :meth:`Booster.shap_interaction_values` and oracle of the GPU kernel.

    Per merged leaf path (elements e with zero fraction z_e, one fraction o_e, leaf value v):
    ``Phi[i][j] += v/2 (o_i - z_i)(o_j - z_j) W(path \\ {i, j})`` and ``phi[i] += v (o_i - z_i) W(path \\ {i})``
    with W the EXTEND weight sum over the remaining elements; ``Phi[i][i] = phi[i] - sum_{j != i}
    Phi[i][j]``. Vectorised over rows and over the paths of equal length."""
    X = np.asarray(X, dtype=np.float32)
    N, F = X.shape
    upper = np.zeros((N, F * F), dtype=np.float64)   # cell (min(i, j), max(i, j)) of every pair
    phi = np.zeros((N, F), dtype=np.float64)
    rows = np.arange(N)[:, None]
    for k, (v, feat, lo, hi, nan_ok, zero) in _paths_by_length(b):
        xv = X[:, feat]                                                             # [N, P, k]
        one = np.where(np.isnan(xv), nan_ok, (xv >= lo) & ~(xv >= hi)).astype(np.float64)
        z = [zero[:, e] for e in range(k)]
        o = [one[:, :, e] for e in range(k)]
        for a in range(k):
            rest = [e for e in range(k) if e != a]
            val = v * (o[a] - z[a]) * _extend_sum([z[e] for e in rest], [o[e] for e in rest])
            np.add.at(phi, (rows, feat[:, a][None, :]), val)
            for c in range(a + 1, k):
                rest = [e for e in range(k) if e != a and e != c]
                val = 0.5 * v * ((o[a] - z[a]) * (o[c] - z[c])) * _extend_sum([z[e] for e in rest],
                                                                               [o[e] for e in rest])
                fa, fc = feat[:, a], feat[:, c]
                cell = np.minimum(fa, fc) * F + np.maximum(fa, fc)
                np.add.at(upper, (rows, cell[None, :]), val)
    upper = upper.reshape(N, F, F)
    out = upper + upper.transpose(0, 2, 1)
    d = np.arange(F)
    out[:, d, d] = phi - out.sum(2)
    return out


def shapley_interactions_bruteforce(b: Booster, X: np.ndarray) -> np.ndarray:
    """Shapley interaction values [N, F, F] by the definition, for tests on tiny models (F <= 6):
    every subset S is evaluated with the conditional expectation f_x(S) of Lundberg et al.,
    Algorithm 1 (EXPVALUE: follow x at splits on features of S, NaN by the default direction, else
    the cover-weighted mean of both children), by recursion on the raw trees. No paths, no EXTEND."""
    from itertools import combinations

    X = np.asarray(X, dtype=np.float32)
    N, F = X.shape
    if F > 6:
        raise ValueError("brute-force interaction values are for F <= 6")
    fact = [math.factorial(i) for i in range(F + 1)]

    def expvalue(t: Tree, cov, j: int, x, S: frozenset) -> float:
        if t.left_children[j] == -1:
            return float(t.split_conditions[j])
        f = int(t.split_indices[j])
        l, r = int(t.left_children[j]), int(t.right_children[j])
        if f in S:
            v = x[f]
            left = bool(t.default_left[j]) if np.isnan(v) else bool(v < t.split_conditions[j])
            return expvalue(t, cov, l if left else r, x, S)
        return (cov[l] * expvalue(t, cov, l, x, S) + cov[r] * expvalue(t, cov, r, x, S)) / cov[j]

    covs = [t.sum_hessian.astype(np.float64) for t in b.trees]
    out = np.zeros((N, F, F), dtype=np.float64)
    for n in range(N):
        fx = {}
        for size in range(F + 1):
            for S in combinations(range(F), size):
                S = frozenset(S)
                fx[S] = sum(expvalue(t, c, 0, X[n], S) for t, c in zip(b.trees, covs))
        phi = np.zeros(F)
        for i in range(F):
            others = [f for f in range(F) if f != i]
            for size in range(F):
                for S in combinations(others, size):
                    S = frozenset(S)
                    phi[i] += fact[size] * fact[F - size - 1] / fact[F] * (fx[S | {i}] - fx[S])
            for j in range(F):
                if j == i:
                    continue
                rest = [f for f in others if f != j]
                for size in range(F - 1):
                    for S in combinations(rest, size):
                        S = frozenset(S)
                        wgt = fact[size] * fact[F - size - 2] / (2 * fact[F - 1])
                        out[n, i, j] += wgt * (fx[S | {i, j}] - fx[S | {i}] - fx[S | {j}] + fx[S])
        for i in range(F):
            out[n, i, i] = phi[i] - (out[n, i].sum() - out[n, i, i])
    return out


# ----------------------------------------------------------------- interventional TreeSHAP
MODEL_OUTPUTS = ("raw", "probability")
SHAP_MAX_UNIQUE = 15    # unique features on a path the interventional weight table covers


def check_model_output(model_output: str) -> bool:
    """True for "probability", False for "raw"; ``ValueError`` otherwise."""
    if model_output not in MODEL_OUTPUTS:
        raise ValueError(f"model_output must be one of {MODEL_OUTPUTS}, got {model_output!r}")
    return model_output == "probability"


def predict_margin64_host(b: Booster, X: np.ndarray) -> np.ndarray:
    """The margin as the SHAP values see it: ``base_margin`` plus the leaf values in tree order, summed in
    float64 (the predictor sums the same leaves in float32)."""
    X = np.asarray(X, dtype=np.float32)
    N = X.shape[0]
    out = np.full(N, np.float64(b.base_margin), dtype=np.float64)
    rows = np.arange(N)
    for t in b.trees:
        nid = np.zeros(N, dtype=np.int32)
        while True:
            lc = t.left_children[nid]
            active = lc != -1
            if not active.any():
                break
            v = X[rows, np.where(active, t.split_indices[nid], 0)]
            go_left = np.where(np.isnan(v), t.default_left[nid] == 1, v < t.split_conditions[nid])
            nid = np.where(active, np.where(go_left, lc, t.right_children[nid]), nid)
        out = out + t.split_conditions[nid].astype(np.float64)
    return out


def sigmoid64(m) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-m))


def probability_rescale(fx, fz) -> np.ndarray:
    """``(sigmoid(fx) - sigmoid(fz)) / (fx - fz)``, broadcast; where ``fx == fz`` the derivative
    ``sigmoid'(fx)``. Evaluated as ``sigmoid(hi) sigmoid(-lo) (1 - exp(-d)) / d`` with ``d = hi - lo``: the
    same function without the cancellation of the quotient at nearly equal margins."""
    fx, fz = np.broadcast_arrays(np.asarray(fx, np.float64), np.asarray(fz, np.float64))
    hi, lo = np.maximum(fx, fz), np.minimum(fx, fz)
    d = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 1.0, -np.expm1(-d) / d)
    return sigmoid64(hi) * sigmoid64(-lo) * r


def interventional_weights() -> np.ndarray:
    """``W[a, b] = (a - 1)! b! / (a + b)!`` for ``a >= 1``, ``a + b <= SHAP_MAX_UNIQUE`` (0 elsewhere): the
    Shapley weight of each of ``a`` features only the explained row satisfies, next to ``b`` only the
    background row satisfies; the weight of each of those ``b`` is ``-W[b, a]``."""
    n = SHAP_MAX_UNIQUE + 1
    W = np.zeros((n, n), dtype=np.float64)
    for a in range(1, n):
        for c in range(n - a):
            W[a, c] = math.factorial(a - 1) * math.factorial(c) / math.factorial(a + c)
    return W


def check_background(b: Booster, X: np.ndarray, Z: np.ndarray) -> None:
    if X.ndim != 2 or X.shape[1] < b.num_feature:
        raise ValueError(f"X has shape {X.shape}, model needs [rows, >= {b.num_feature}]")
    if Z.ndim != 2 or Z.shape[1] < b.num_feature:
        raise ValueError(f"the background has shape {Z.shape}, model needs [rows, >= {b.num_feature}]")
    if Z.shape[0] == 0:
        raise ValueError("the background set has no rows")


def treeshap_interventional_host(b: Booster, X: np.ndarray, Z: np.ndarray, model_output: str = "raw") -> np.ndarray:
    """Interventional TreeSHAP values [N, F] float64 of the rows ``X`` against the background rows ``Z``
    (``shap.TreeExplainer(model, data, feature_perturbation="interventional")``); CPU path of
    :meth:`Booster.shap_values_interventional` and oracle of the GPU kernel. Covers are not used.

    For a pair (x, z) the game is ``v(S) = f(x on S, z elsewhere)``. Per merged leaf path with leaf value
    ``v``: a feature neither row satisfies kills the path; otherwise with ``a`` features only x satisfies and
    ``c`` only z satisfies, each x-only feature gets ``+v (a-1)! c! / (a+c)!`` and each z-only feature
    ``-v a! (c-1)! / (a+c)!``. "raw": the mean over the background. "probability": every pair is scaled by
    :func:`probability_rescale` of the float64 margins (:func:`predict_margin64_host`) before the mean.
    Vectorised over rows, background rows and the paths of equal length."""
    prob = check_model_output(model_output)
    X = np.asarray(X, dtype=np.float32)
    Z = np.asarray(Z, dtype=np.float32)
    check_background(b, X, Z)
    N, F = X.shape
    nB = Z.shape[0]
    phi = np.zeros((N, F), dtype=np.float64)
    if N == 0:
        return phi
    groups = _paths_by_length(b)
    if groups and groups[-1][0] > SHAP_MAX_UNIQUE:
        raise ValueError(f"path with {groups[-1][0]} unique features exceeds the TreeSHAP limit {SHAP_MAX_UNIQUE}")
    W = interventional_weights()
    scale = probability_rescale(predict_margin64_host(b, X)[:, None], predict_margin64_host(b, Z)[None, :]) \
        if prob else None                                                         # [N, B]
    for k, (v, feat, lo, hi, nan_ok, _zero) in groups:
        P = len(v)
        zv = Z[:, feat]                                                           # [B, P, k]
        zs = np.where(np.isnan(zv), nan_ok, (zv >= lo) & ~(zv >= hi))
        step = max(1, (1 << 23) // max(nB * P * k, 1))                            # rows per block of pairs
        for r0 in range(0, N, step):
            xv = X[r0:r0 + step][:, feat]                                         # [n, P, k]
            xs = np.where(np.isnan(xv), nan_ok, (xv >= lo) & ~(xv >= hi))[:, None]   # [n, 1, P, k]
            x1, z1 = xs & ~zs[None], ~xs & zs[None]                               # [n, B, P, k]
            ok = (xs | zs[None]).all(-1)
            a, c = x1.sum(-1), z1.sum(-1)
            wx = np.where(ok, W[a, c], 0.0)                                       # [n, B, P]
            wz = np.where(ok, W[c, a], 0.0)
            if prob:
                wx = wx * scale[r0:r0 + step, :, None]
                wz = wz * scale[r0:r0 + step, :, None]
            val = v[None, :, None] * (x1 * wx[..., None] - z1 * wz[..., None]).sum(1)   # [n, P, k]
            np.add.at(phi, (np.arange(r0, r0 + xv.shape[0])[:, None, None], feat[None]), val)
    return phi / nB


def expected_value_interventional_host(b: Booster, Z: np.ndarray, model_output: str = "raw") -> float:
    """The baseline of :func:`treeshap_interventional_host`: the mean float64 margin of the background rows,
    or the mean of their probabilities."""
    prob = check_model_output(model_output)
    Z = np.asarray(Z, dtype=np.float32)
    check_background(b, Z, Z)
    m = predict_margin64_host(b, Z)
    return float(np.mean(sigmoid64(m) if prob else m))


def shapley_interventional_bruteforce(b: Booster, X: np.ndarray, Z: np.ndarray) -> np.ndarray:
    """Interventional Shapley values of every pair, [N, B, F] float64, by the definition, for tests on tiny
    models (F <= 10): all 2^F hybrid rows (x on S, z elsewhere) are scored on the raw trees and
    ``phi_i = sum_{S without i} |S|! (F - |S| - 1)! / F! (v(S + i) - v(S))``. No paths, no closed form."""
    X = np.asarray(X, dtype=np.float32)
    Z = np.asarray(Z, dtype=np.float32)
    N, F = X.shape
    if F > 10:
        raise ValueError("brute-force interventional values are for F <= 10")
    masks = np.arange(1 << F)
    in_s = ((masks[:, None] >> np.arange(F)[None, :]) & 1).astype(bool)           # [2^F, F]
    size = in_s.sum(1)
    wgt = np.array([math.factorial(s) * math.factorial(F - s - 1) / math.factorial(F) for s in range(F)])
    out = np.zeros((N, Z.shape[0], F), dtype=np.float64)
    for n in range(N):
        for j in range(Z.shape[0]):
            v = predict_margin64_host(b, np.where(in_s, X[n][None, :], Z[j][None, :F]))
            for i in range(F):
                without = masks[~in_s[:, i]]
                out[n, j, i] = ((v[without | (1 << i)] - v[without]) * wgt[size[without]]).sum()
    return out


def trees_from_heap_nodes(nodes: np.ndarray, max_depth: int, native: bool | None = None) -> list[Tree]:
    """Convert heap-ordered node records (NODE_DTYPE, [T, 2^(D+1)-1]) of the trainer into XGBoost
    trees, numbering nodes in XGBoost's depthwise creation order (children allocated in pairs).

    ``native`` (default: whenever the native library is loadable): the one-pass C++ conversion
    (``csrc/treeconv.cpp``, ~0.1 ms for 300 trees); False: the NumPy form below (its oracle)."""
    if native is not False and nodes.ndim == 2 and nodes.shape[0] > 0:
        out = _trees_from_heap_nodes_native(nodes, required=native is True)
        if out is not None:
            return out
    # Heap indices of one level are contiguous and children are allocated in parent order, so the
    # depthwise creation order is simply ascending heap index over the live nodes.
    # Everything is computed for all trees at once and split per tree at the end.
    if nodes.ndim != 2 or nodes.shape[0] == 0:
        return []
    T, M = nodes.shape
    status = nodes["status"]
    live = (status == 2) | (status == 3)
    new_id = (np.cumsum(live, axis=1) - 1).astype(np.int32)       # per-tree position of each live node
    counts = live.sum(1)
    split_full = status == 2
    kid = np.minimum(2 * np.arange(M) + 1, M - 2)
    lc_full = np.where(split_full, new_id[:, kid], -1).astype(np.int32)
    rc_full = np.where(split_full, new_id[:, kid + 1], -1).astype(np.int32)
    par_full = np.full((T, M), ROOT_PARENT, np.int32)
    parent_heap = (np.arange(M) - 1) // 2
    has_par = np.arange(M) > 0
    par_full[:, has_par] = new_id[:, parent_heap[has_par]]
    # the live records gathered as 64-byte rows of an int32 view (a boolean mask on the structured
    # array copied field by field: ~4 ms for 300 trees)
    words = np.ascontiguousarray(nodes).reshape(-1).view(np.int32).reshape(-1, NODE_DTYPE.itemsize // 4)
    r = words[np.flatnonzero(live.reshape(-1))].view(NODE_DTYPE).reshape(-1)
    split = r["status"] == 2
    lc, rc, par = lc_full[live], rc_full[live], par_full[live]
    si = np.where(split, r["feat"], 0).astype(np.int32)
    sc = np.where(split, r["split_cond"], r["leaf_value"]).astype(np.float32)
    dl = np.where(split, r["default_left"], 0).astype(np.uint8)
    lo = np.where(split, r["loss_chg"], 0).astype(np.float32)
    bw = r["base_weight"].astype(np.float32)
    sh = r["sum_hess"].astype(np.float32)
    # per-tree views by offsets (np.split's per-piece swapaxes cost ~9 ms for 300 x 9 arrays)
    ends = np.cumsum(counts).tolist()
    begins = [0] + ends[:-1]
    cols = (lc, rc, par, si, sc, dl, bw, lo, sh)
    return [Tree(*(a[b0:b1] for a in cols)) for b0, b1 in zip(begins, ends)]


def _trees_from_heap_nodes_native(nodes: np.ndarray, required: bool = False) -> list[Tree] | None:
    try:
        from .. import _native

        lib = _native.lib()
    except Exception:  # noqa: BLE001 -- no native library (source-only CPU install): NumPy path
        if required:
            raise
        return None
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    T, M = nodes.shape
    cap = T * M
    counts = np.empty(T, np.int32)
    cols = [np.empty(cap, dt) for dt in (np.int32, np.int32, np.int32, np.int32, np.float32, np.uint8,
                                         np.float32, np.float32, np.float32)]
    lc, rc, par, si, sc, dl, bw, lo, sh = cols
    n = lib.cobalt_heap_to_trees(nodes.ctypes.data, T, M, counts.ctypes.data,
                                 *(a.ctypes.data for a in cols))
    if n < 0:
        raise RuntimeError("cobalt_heap_to_trees: bad arguments")
    ends = np.cumsum(counts).tolist()
    begins = [0] + ends[:-1]
    # Tree fields in their declared order: left, right, parents, split_indices, split_conditions,
    # default_left, base_weights, loss_changes, sum_hessian
    order = (lc, rc, par, si, sc, dl, bw, lo, sh)
    spans = list(zip(begins, ends))
    per_col = [[a[b0:b1] for b0, b1 in spans] for a in order]
    return [Tree(*parts) for parts in zip(*per_col)]


NODE_DTYPE = np.dtype([
    ("G", "<i8"), ("H", "<i8"), ("start", "<i4"), ("count", "<i4"), ("status", "<i4"), ("build", "<i4"),
    ("feat", "<i4"), ("bin", "<i4"), ("default_left", "<i4"), ("split_cond", "<f4"), ("loss_chg", "<f4"),
    ("leaf_value", "<f4"), ("sum_hess", "<f4"), ("base_weight", "<f4"),
])
assert NODE_DTYPE.itemsize == 64


def concat_feature_names(names: Sequence[str] | None, F: int) -> list[str]:
    return list(names) if names is not None else [f"f{i}" for i in range(F)]
