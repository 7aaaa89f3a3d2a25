"""TreeExplainer-style API over the GPU TreeSHAP kernel (reference: ``shap.TreeExplainer`` in
src/api/cobalt_fast_api.py:46,100 and notebooks/04_model_training.ipynb cells 24-26).

``TreeExplainer(model).shap_values(X)`` returns path-dependent (``feature_perturbation=
"tree_path_dependent"``) SHAP values in margin space, ``expected_value`` is the cover-weighted mean
leaf sum (the API's ``base_value``). ``TreeExplainer(model, data=Z)`` returns interventional values
against the background rows ``Z``, optionally in probability space. ``shap`` itself is not a dependency: the summary / bar /
waterfall / force views the notebook draws are produced with matplotlib from the same arrays.
"""
from __future__ import annotations

import numpy as np

from ..models.booster import Booster


def _booster(model) -> Booster:
    if isinstance(model, Booster):
        return model
    if hasattr(model, "get_booster"):
        return model.get_booster()
    raise TypeError("expected a Booster or a fitted GBDTClassifier")


FEATURE_PERTURBATIONS = ("auto", "interventional", "tree_path_dependent")


class TreeExplainer:
    """``shap.TreeExplainer(model, data=None, feature_perturbation="auto", model_output="raw")``.

    Without ``data``: path-dependent values in margin space, ``expected_value`` = the cover-weighted mean
    leaf sum. With ``data`` (a background set, [B, F]): interventional values against its rows, in margin
    space or, with ``model_output="probability"``, in probability space; ``expected_value`` = the mean margin /
    probability of the background rows. ``shap``'s rules for the combinations: "interventional" needs ``data``,
    "tree_path_dependent" does not take it, and "probability" needs the interventional values."""

    def __init__(self, model, data=None, feature_perturbation="auto", model_output="raw", device=None):
        self.booster = _booster(model)
        self.device = device
        self.feature_names = list(self.booster.feature_names or [f"f{i}" for i in range(self.booster.num_feature)])
        if feature_perturbation not in FEATURE_PERTURBATIONS:
            raise ValueError(f"feature_perturbation must be one of {FEATURE_PERTURBATIONS}, "
                             f"got {feature_perturbation!r}")
        if model_output not in ("raw", "probability"):
            raise ValueError(f"model_output must be 'raw' or 'probability', got {model_output!r}")
        if data is None:
            if feature_perturbation == "interventional":
                raise ValueError("feature_perturbation='interventional' needs a background set: pass data=")
            if model_output == "probability":
                raise ValueError("model_output='probability' needs interventional values against a background "
                                 "set (pass data=): the path-dependent values exist in margin space only")
            feature_perturbation = "tree_path_dependent"
        elif feature_perturbation == "tree_path_dependent":
            raise ValueError("feature_perturbation='tree_path_dependent' takes its baseline from the covers stored "
                             "in the trees and cannot use data=; drop data= or ask for 'interventional'")
        else:
            feature_perturbation = "interventional"
        self.feature_perturbation = feature_perturbation
        self.model_output = model_output
        self.data = None if data is None else self._matrix(data)
        if self.data is None:
            self.expected_value = float(self.booster.expected_value())
        else:
            self.expected_value = float(self.booster.expected_value_interventional(self.data, model_output))

    def _matrix(self, X) -> np.ndarray:
        """``X`` as a float32 array; a DataFrame's columns are reordered by feature name."""
        names = self.booster.feature_names
        if hasattr(X, "columns") and names:
            X = X[names]
        if hasattr(X, "to_numpy"):
            return X.to_numpy(dtype=np.float32, na_value=np.nan)
        return np.asarray(X.detach().cpu().numpy() if hasattr(X, "detach") else X, np.float32)

    def shap_values(self, X) -> np.ndarray:
        if self.data is not None:
            phi = self.booster.shap_values_interventional(self._matrix(X), self.data, model_output=self.model_output,
                                                          device=self.device)
            return np.asarray(phi.cpu().numpy() if hasattr(phi, "cpu") else phi, dtype=np.float64)
        names = self.booster.feature_names
        if hasattr(X, "columns") and names:
            X = X[names]
        Xn = X.to_numpy(dtype=np.float32, na_value=np.nan) if hasattr(X, "to_numpy") else np.asarray(X, np.float32)
        phi = self.booster.shap_values(Xn, device=self.device)
        return np.asarray(phi.cpu().numpy() if hasattr(phi, "cpu") else phi, dtype=np.float64)

    def shap_interaction_values(self, X) -> np.ndarray:
        """``shap.TreeExplainer.shap_interaction_values``: [N, F, F] float64; a DataFrame's columns are
        reordered by feature name. Path-dependent only."""
        if self.data is not None:
            raise ValueError("interaction values are path-dependent only: build the explainer without data=")
        names = self.booster.feature_names
        if hasattr(X, "columns") and names:
            X = X[names]
        Xn = X.to_numpy(dtype=np.float32, na_value=np.nan) if hasattr(X, "to_numpy") else np.asarray(X, np.float32)
        out = self.booster.shap_interaction_values(Xn, device=self.device)
        return np.asarray(out.cpu().numpy() if hasattr(out, "cpu") else out, dtype=np.float64)

    def __call__(self, X) -> "Explanation":
        vals = self.shap_values(X)
        data = X.to_numpy(dtype=np.float64, na_value=np.nan) if hasattr(X, "to_numpy") else np.asarray(X, np.float64)
        return Explanation(vals, np.full(len(vals), self.expected_value), data, self.feature_names)


class Explanation:
    def __init__(self, values, base_values, data, feature_names):
        self.values = np.asarray(values)
        self.base_values = np.asarray(base_values)
        self.data = np.asarray(data)
        self.feature_names = list(feature_names)

    def __getitem__(self, i) -> "Explanation":
        return Explanation(self.values[i], self.base_values[i], self.data[i], self.feature_names)

    def mean_abs(self) -> np.ndarray:
        return np.abs(self.values).mean(0)


def _plt():
    import matplotlib

    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt

    return plt


def bar_plot(exp: Explanation, max_display: int = 10):
    """Global importance: mean |SHAP| per feature (shap.plots.bar)."""
    plt = _plt()
    m = exp.mean_abs()
    order = np.argsort(-m, kind="stable")[:max_display][::-1]
    fig, ax = plt.subplots(figsize=(8, 0.4 * len(order) + 1.5))
    ax.barh([exp.feature_names[i] for i in order], m[order], color="#008bfb")
    ax.set_xlabel("mean(|SHAP value|)")
    fig.tight_layout()
    return fig


def summary_plot(exp: Explanation, max_display: int = 20, seed: int = 0):
    """Beeswarm-style summary (shap.summary_plot): one row per feature, points coloured by the
    feature value's within-feature rank."""
    plt = _plt()
    m = exp.mean_abs()
    order = np.argsort(-m, kind="stable")[:max_display][::-1]
    rng = np.random.default_rng(seed)
    fig, ax = plt.subplots(figsize=(9, 0.45 * len(order) + 1.5))
    for row, f in enumerate(order):
        v = exp.values[:, f]
        x = exp.data[:, f]
        ok = ~np.isnan(x)
        col = np.full(len(x), 0.5)
        if ok.any():
            r = np.argsort(np.argsort(x[ok]))
            col[ok] = r / max(len(r) - 1, 1)
        ax.scatter(v, row + rng.uniform(-0.3, 0.3, len(v)), c=col, cmap="coolwarm", s=4, alpha=0.6)
    ax.set_yticks(range(len(order)), [exp.feature_names[i] for i in order])
    ax.axvline(0, color="grey", lw=0.8)
    ax.set_xlabel("SHAP value (impact on model output)")
    fig.tight_layout()
    return fig


def force_data(exp: Explanation, i: int) -> dict:
    """The numbers behind shap's force plot for row ``i`` (base, prediction, sorted contributions)."""
    v = exp.values[i]
    order = np.argsort(-np.abs(v), kind="stable")
    return {"base_value": float(exp.base_values[i]), "output": float(exp.base_values[i] + v.sum()),
            "contributions": [{"feature": exp.feature_names[j], "value": float(exp.data[i, j]),
                               "shap": float(v[j])} for j in order]}


def top_interactions(values, feature_names, k: int = 10) -> list[dict]:
    """The ``k`` strongest feature pairs of interaction values [N, F, F] (or one matrix [F, F]):
    strength = mean over rows of ``|Phi[i][j] + Phi[j][i]|`` for i < j, strongest first, ties in
    (i, j) order."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 2:
        v = v[None]
    F = v.shape[1]
    if v.shape[2] != F or len(feature_names) != F:
        raise ValueError(f"expected [N, F, F] values and F feature names, got {v.shape} and {len(feature_names)}")
    iu, ju = np.triu_indices(F, 1)
    strength = np.abs(v[:, iu, ju] + v[:, ju, iu]).mean(0) if v.shape[0] else np.zeros(len(iu))
    order = np.argsort(-strength, kind="stable")[:k]
    return [{"feature_a": feature_names[iu[q]], "feature_b": feature_names[ju[q]], "strength": float(strength[q])}
            for q in order]


# --------------------------------------------------------------------------- partial dependence
def partial_dependence(model, X, features, **kw) -> dict:
    """Partial dependence / ICE curves (:meth:`Booster.partial_dependence`) of a ``GBDTClassifier``, a
    ``Booster`` or a :class:`TreeExplainer`. A classifier scores the trees ``predict_proba`` scores (the first
    ``best_iteration + 1`` of an early-stopped fit, or ``iteration_range=(0, n)``), on its device, and a
    DataFrame's columns are reordered by feature name."""
    if isinstance(model, TreeExplainer):
        kw.setdefault("device", model.device)
        return model.booster.partial_dependence(X, features, **kw)
    if isinstance(model, Booster):
        return model.partial_dependence(X, features, **kw)
    if hasattr(model, "get_booster") and hasattr(model, "_n_trees"):
        if "n_trees" in kw and "iteration_range" in kw:
            raise ValueError("pass n_trees or iteration_range, not both")
        if "n_trees" not in kw:
            kw["n_trees"] = model._n_trees(kw.pop("iteration_range", None))
        kw.setdefault("device", model.device)
        return model.get_booster().partial_dependence(model._matrix(X), features, **kw)
    raise TypeError("expected a GBDTClassifier, a Booster or a TreeExplainer")


def pd_plot(result: dict, ice: bool = True, max_ice: int = 200, centered: bool = False):
    """Draw a :func:`partial_dependence` result. One feature: the average as a line over at most ``max_ice``
    evenly thinned ICE lines (``ice``, when the result has them); a NaN grid point ("feature missing") is
    drawn apart, to the right of the numeric axis. ``centered``: every curve minus its value at the first
    grid point. Two features: a filled contour of the average over the numeric grid."""
    plt = _plt()
    axes = [np.asarray(g, np.float64) for g in result["grid_values"]]
    names = list(result["feature_names"])
    avg = None if result.get("average") is None else np.asarray(result["average"], np.float64)
    ind = None if result.get("individual") is None else np.asarray(result["individual"], np.float64)
    if len(axes) == 2:
        if avg is None:
            raise ValueError("a two-feature plot needs the average (kind='average' or 'both')")
        k0, k1 = ~np.isnan(axes[0]), ~np.isnan(axes[1])
        z = avg[np.ix_(k0, k1)]
        fig, ax = plt.subplots(figsize=(7, 5.5))
        if z.shape[0] >= 2 and z.shape[1] >= 2:
            cs = ax.contourf(axes[0][k0], axes[1][k1], z.T, levels=12, cmap="viridis")
        else:
            cs = ax.imshow(z.T, origin="lower", aspect="auto", cmap="viridis")
        fig.colorbar(cs, ax=ax, label="partial dependence")
        ax.set_xlabel(names[0])
        ax.set_ylabel(names[1])
        fig.tight_layout()
        return fig
    g = axes[0]
    num = ~np.isnan(g)
    fig, ax = plt.subplots(figsize=(8, 5))
    # the missing point sits one step to the right of the numeric axis
    gn = g[num]
    span = float(gn.max() - gn.min()) if gn.size else 0.0
    x_missing = (float(gn.max()) + (0.08 * span if span > 0 else 1.0)) if gn.size else 0.0

    def draw(curve, **style):
        c = curve - curve[0] if centered else curve
        ax.plot(gn, c[num], **style)
        if (~num).any():
            ax.plot(np.full(int((~num).sum()), x_missing), c[~num], linestyle="none", marker="o",
                    color=style.get("color"), alpha=style.get("alpha", 1.0), markersize=style.get("lw", 1.0) + 2)

    if ice and ind is not None and len(ind):
        pick = np.unique(np.linspace(0, len(ind) - 1, min(max_ice, len(ind))).astype(np.int64))
        for r in pick:
            draw(ind[r], color="#9ecae1", lw=0.6, alpha=0.5)
    if avg is not None:
        draw(avg, color="#08519c", lw=2.2)
    if (~num).any():
        ax.axvline(x_missing - (0.04 * span if span > 0 else 0.5), color="grey", lw=0.8, ls=":")
        ticks = [t for t in ax.get_xticks() if gn.size and gn.min() <= t <= gn.max()]
        ax.set_xticks(ticks + [x_missing], [f"{t:g}" for t in ticks] + ["missing"])
    ax.set_xlabel(names[0])
    ax.set_ylabel("partial dependence" + (" (centered)" if centered else ""))
    fig.tight_layout()
    return fig


# -------------------------------------------------------------------- accumulated local effects
def accumulated_local_effects(model, X, features=None, **kw):
    """Accumulated local effects (:meth:`Booster.accumulated_local_effects`) of a ``GBDTClassifier``, a
    ``Booster`` or a :class:`TreeExplainer`: the effect of a feature (or the interaction of a pair) measured
    only where the rows are, which partial dependence is not for correlated features. A classifier scores the
    trees ``predict_proba`` scores (the first ``best_iteration + 1`` of an early-stopped fit, or
    ``iteration_range=(0, n)``), on its device, and a DataFrame's columns are reordered by feature name."""
    if isinstance(model, TreeExplainer):
        kw.setdefault("device", model.device)
        return model.booster.accumulated_local_effects(X, features, **kw)
    if isinstance(model, Booster):
        return model.accumulated_local_effects(X, features, **kw)
    if hasattr(model, "get_booster") and hasattr(model, "_n_trees"):
        if "n_trees" in kw and "iteration_range" in kw:
            raise ValueError("pass n_trees or iteration_range, not both")
        if "n_trees" not in kw:
            kw["n_trees"] = model._n_trees(kw.pop("iteration_range", None))
        kw.setdefault("device", model.device)
        return model.get_booster().accumulated_local_effects(model._matrix(X), features, **kw)
    raise TypeError("expected a GBDTClassifier, a Booster or a TreeExplainer")


def _ale_axes(ax, r: dict) -> None:
    """One :func:`accumulated_local_effects` result on ``ax``."""
    names = list(r["feature_names"])
    edges = [np.asarray(z, np.float64) for z in r["edges"]]
    ale = np.asarray(r["ale"], np.float64)
    wgt = np.asarray(r["interval_weight"], np.float64)
    if len(edges) == 2:
        if ale.shape[0] >= 2 and ale.shape[1] >= 2:
            cs = ax.contourf(edges[0], edges[1], ale.T, levels=12, cmap="RdBu_r")
        else:
            cs = ax.imshow(ale.T, origin="lower", aspect="auto", cmap="RdBu_r")
        ax.figure.colorbar(cs, ax=ax, label="ALE (second order)")
        ax.set_xlabel(names[0])
        ax.set_ylabel(names[1])
        return
    z = edges[0] if len(edges[0]) == len(ale) else np.zeros(len(ale))
    ax.plot(z, ale, color="#08519c", lw=2.0, marker="o" if len(ale) < 3 else None)
    ax.axhline(0, color="grey", lw=0.8)
    if wgt.size and wgt.sum() > 0:  # the rug: one tick per interval at its midpoint, as tall as its share of weight
        mid = (z[:-1] + z[1:]) / 2
        lo, hi = ax.get_ylim()
        ax.vlines(mid, lo, lo + 0.12 * (hi - lo) * wgt / wgt.max(), color="#6b6b6b", lw=1.2)
        ax.set_ylim(lo, hi)
    ax.set_xlabel(names[0])
    ax.set_ylabel("ALE")


def ale_plot(result, max_cols: int = 4):
    """Draw an :func:`accumulated_local_effects` result. One feature: the curve on its edges over a rug of the
    interval weights (where the rows are). A pair: a filled contour of the second-order effect. A list: one
    panel per result."""
    plt = _plt()
    if isinstance(result, dict):
        fig, ax = plt.subplots(figsize=(8, 5) if len(result["edges"]) == 1 else (7, 5.5))
        _ale_axes(ax, result)
        fig.tight_layout()
        return fig
    results = list(result)
    if not results:
        raise ValueError("nothing to draw")
    cols = min(max_cols, len(results))
    rows = (len(results) + cols - 1) // cols
    fig, axes = plt.subplots(rows, cols, figsize=(4.2 * cols, 3.4 * rows), squeeze=False)
    for ax, r in zip(axes.ravel(), results):
        _ale_axes(ax, r)
    for ax in axes.ravel()[len(results):]:
        ax.set_visible(False)
    fig.tight_layout()
    return fig


# ----------------------------------------------------------------------- permutation importance
def permutation_importance(model, X, y, features=None, **kw) -> dict:
    """Permutation feature importance (:meth:`Booster.permutation_importance`) of a ``GBDTClassifier``, a
    ``Booster`` or a :class:`TreeExplainer`. A classifier scores the trees ``predict_proba`` scores (the first
    ``best_iteration + 1`` of an early-stopped fit, or ``iteration_range=(0, n)``), on its device, and a
    DataFrame's columns are reordered by feature name."""
    if isinstance(model, TreeExplainer):
        kw.setdefault("device", model.device)
        return model.booster.permutation_importance(X, y, features, **kw)
    if isinstance(model, Booster):
        return model.permutation_importance(X, y, features, **kw)
    if hasattr(model, "get_booster") and hasattr(model, "_n_trees"):
        if "n_trees" in kw and "iteration_range" in kw:
            raise ValueError("pass n_trees or iteration_range, not both")
        if "n_trees" not in kw:
            kw["n_trees"] = model._n_trees(kw.pop("iteration_range", None))
        kw.setdefault("device", model.device)
        return model.get_booster().permutation_importance(model._matrix(X), y, features, **kw)
    raise TypeError("expected a GBDTClassifier, a Booster or a TreeExplainer")


def importance_plot(result: dict, max_display: int = 10):
    """Draw a :func:`permutation_importance` result: one horizontal box plot of the repeats per feature, the
    ``max_display`` features with the largest mean importance, the largest on top."""
    plt = _plt()
    imp = np.asarray(result["importances"], np.float64)
    mean = np.asarray(result["importances_mean"], np.float64)
    order = np.argsort(-mean, kind="stable")[:max_display][::-1]
    fig, ax = plt.subplots(figsize=(8, 0.4 * len(order) + 1.5))
    if len(order):
        ax.boxplot([imp[i] for i in order], vert=False)
        ax.set_yticks(range(1, len(order) + 1), [result["feature_names"][i] for i in order])
    ax.axvline(0, color="grey", lw=0.8)
    ax.set_xlabel(f"permutation importance ({result['metric']} degradation)")
    fig.tight_layout()
    return fig
