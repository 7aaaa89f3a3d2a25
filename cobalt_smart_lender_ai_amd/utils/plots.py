"""Evaluation figures written by the training pipeline (reference:
src/model_train_test/model_tree_train_test.py:184-210 -- seaborn confusion-matrix heatmap and a
top-10 gain-importance bar chart). Rendered with matplotlib's Agg backend (seaborn is optional)."""
from __future__ import annotations

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402


def confusion_matrix_figure(cm: np.ndarray):
    fig, ax = plt.subplots(figsize=(6, 4))
    im = ax.imshow(cm, cmap="Blues")
    for (i, j), v in np.ndenumerate(cm):
        ax.text(j, i, f"{int(v)}", ha="center", va="center",
                color="white" if v > cm.max() / 2 else "black")
    ax.set_xticks(range(cm.shape[1]))
    ax.set_yticks(range(cm.shape[0]))
    ax.set_title("Confusion Matrix")
    ax.set_xlabel("Predicted")
    ax.set_ylabel("Actual")
    fig.colorbar(im, ax=ax)
    return fig


def feature_importance_figure(names: list[str], importances: np.ndarray, top: int = 10):
    order = np.argsort(-np.asarray(importances), kind="stable")[:top]
    fig, ax = plt.subplots(figsize=(8, 5))
    ax.barh([names[i] for i in order][::-1], np.asarray(importances)[order][::-1], color="skyblue")
    ax.set_xlabel("Feature Importance (Gain)")
    ax.set_title(f"Top {top} Most Important Features")
    fig.tight_layout()
    return fig


def drift_plot(report, top: int = 20):
    """Horizontal bars of the ``top`` largest PSI values of a ``monitor.DriftReport`` (rows are already sorted,
    ``"score"`` first), with the 0.1 ("moderate" from here) and 0.25 ("shifted") lines."""
    from ..monitor.drift import PSI_SHIFTED, PSI_STABLE

    rows = list(report)[:top]
    if not rows:
        raise ValueError("nothing to draw")
    colors = {"stable": "#4daf4a", "moderate": "#ff7f00", "shifted": "#e41a1c"}
    fig, ax = plt.subplots(figsize=(8, max(2.5, 0.32 * len(rows) + 1.2)))
    ax.barh([r["feature"] for r in rows][::-1], [r["psi"] for r in rows][::-1],
            color=[colors[r["status"]] for r in rows][::-1])
    ax.axvline(PSI_STABLE, color="grey", lw=1.0, ls="--")
    ax.axvline(PSI_SHIFTED, color="black", lw=1.0, ls="--")
    ax.set_xlabel("Population stability index")
    ax.set_title("Drift against the baseline")
    fig.tight_layout()
    return fig


def ci_plot(report):
    """Point estimates with their bootstrap percentile intervals, one row per metric of a
    ``metrics.BootstrapReport``: model a, model b when the report has one, and a second panel with the paired
    differences a - b against the zero line."""
    names = list(report.metrics)
    if not names:
        raise ValueError("nothing to draw")
    paired = report.metrics_b is not None
    fig, axes = plt.subplots(1, 2 if paired else 1, figsize=(11 if paired else 7, max(2.5, 0.5 * len(names) + 1.2)),
                             squeeze=False)
    ypos = np.arange(len(names))[::-1].astype(float)

    def bars(ax, rows, dy, color, label):
        pt = np.array([r.point for r in rows], dtype=float)
        lo = np.array([r.low for r in rows], dtype=float)
        hi = np.array([r.high for r in rows], dtype=float)
        ax.errorbar(pt, ypos + dy, xerr=[np.nan_to_num(pt - lo), np.nan_to_num(hi - pt)], fmt="o", color=color,
                    capsize=3, label=label)

    ax = axes[0, 0]
    bars(ax, [report.metrics[m] for m in names], 0.12 if paired else 0.0, "#377eb8", "a")
    if paired:
        bars(ax, [report.metrics_b[m] for m in names], -0.12, "#ff7f00", "b")
        ax.legend(loc="best")
    ax.set_yticks(ypos)
    ax.set_yticklabels(names)
    pct = 100.0 * (1.0 - report.alpha)
    ax.set_title(f"{pct:g}% bootstrap intervals ({report.n_boot} replicates)")
    if paired:
        ax = axes[0, 1]
        bars(ax, [report.delta[m] for m in names], 0.0, "#4daf4a", "a - b")
        ax.axvline(0.0, color="black", lw=1.0, ls="--")
        ax.set_yticks(ypos)
        ax.set_yticklabels(names)
        ax.set_title("Paired difference a - b")
    fig.tight_layout()
    return fig


def reliability_plot(report):
    """The reliability diagram of a ``metrics.calibration.ReliabilityReport``: the diagonal, the observed rate
    against the mean predicted probability of every non-empty bin, and below it the bins' counts."""
    live = ~np.isnan(np.asarray(report.mean_predicted, dtype=float))
    if not live.any():
        raise ValueError("nothing to draw")
    mp = np.asarray(report.mean_predicted, dtype=float)[live]
    ob = np.asarray(report.observed, dtype=float)[live]
    fig, axes = plt.subplots(2, 1, figsize=(6, 7), sharex=True, gridspec_kw={"height_ratios": [3, 1]})
    ax = axes[0]
    ax.plot([0.0, 1.0], [0.0, 1.0], color="black", lw=1.0, ls="--", label="perfectly calibrated")
    ax.plot(mp, ob, "o-", color="#377eb8", label="model")
    ax.set_ylabel("Observed rate")
    ax.set_xlim(0.0, 1.0)
    ax.set_ylim(0.0, 1.0)
    ax.set_title(f"Reliability ({report.n_bins} {report.strategy} bins): ECE {report.ece:.4f}, "
                 f"Brier {report.brier:.4f}")
    ax.legend(loc="upper left")
    ax = axes[1]
    edges = np.concatenate([[0.0], np.asarray(report.edges, dtype=float), [1.0]])
    ax.bar(edges[:-1], np.asarray(report.count, dtype=float), width=np.maximum(np.diff(edges), 1e-3), align="edge",
           color="#999999", edgecolor="white")
    ax.set_xlabel("Predicted probability")
    ax.set_ylabel("Count")
    fig.tight_layout()
    return fig


def scorecard_plot(sc, feature):
    """One characteristic of a fitted ``models.scorecard.Scorecard`` (by name or index): bars of the WoE per bin
    and, on a second axis, the bad rate; bins without rows are left out."""
    f = sc.feature_names.index(feature) if isinstance(feature, str) else int(feature)
    c = np.asarray(sc.counts[f], dtype=float)
    tot = c.sum(0)
    live = tot > 0
    if not live.any():
        raise ValueError("nothing to draw")
    labels = [lab for lab, k in zip(sc.bin_labels(f), live) if k]
    x = np.arange(len(labels))
    fig, ax = plt.subplots(figsize=(7, 4))
    ax.bar(x, np.asarray(sc.woe[f])[live], color="#377eb8", edgecolor="white")
    ax.axhline(0.0, color="black", lw=0.8)
    ax.set_xticks(x)
    ax.set_xticklabels(labels, rotation=30, ha="right")
    ax.set_ylabel("Weight of evidence")
    ax.set_title(f"{sc.feature_names[f]}: IV {sc.iv[f]:.4f}" + (" (dropped)" if sc.dropped[f] else ""))
    ax2 = ax.twinx()
    ax2.plot(x, c[1][live] / tot[live], "o-", color="#e41a1c")
    ax2.set_ylabel("Bad rate")
    ax2.set_ylim(0.0, None)
    fig.tight_layout()
    return fig


def close(fig) -> None:
    plt.close(fig)


def correlation_heatmap(report, top: int | None = None):
    """The correlation matrix of a ``select.CorrelationReport`` as a heat map on [-1, 1] (undefined entries stay
    blank); ``top`` keeps the features with the largest off-diagonal ``|r|``, in their column order."""
    r = np.asarray(report.r, dtype=np.float64)
    names = list(report.names)
    if not names:
        raise ValueError("nothing to draw")
    if top is not None and top < len(names):
        off = np.where(np.eye(len(names), dtype=bool) | ~np.isfinite(r), 0.0, np.abs(r))
        keep = np.sort(np.argsort(-off.max(axis=1), kind="stable")[:top])
        r, names = r[np.ix_(keep, keep)], [names[i] for i in keep]
    side = max(4.0, 0.32 * len(names) + 2.0)
    fig, ax = plt.subplots(figsize=(side + 1.0, side))
    im = ax.imshow(np.ma.masked_invalid(r), vmin=-1.0, vmax=1.0, cmap="RdBu_r")
    ax.set_xticks(range(len(names)), names, rotation=90, fontsize=7)
    ax.set_yticks(range(len(names)), names, fontsize=7)
    fig.colorbar(im, ax=ax, label=f"{report.method} r")
    ax.set_title("Feature correlation")
    fig.tight_layout()
    return fig


def loss_distribution_plot(report, bins: int = 60):
    """The scenario losses of a ``portfolio.LossReport`` as a histogram, with the expected loss and, at the
    report's highest quantile, the value-at-risk and the expected shortfall marked."""
    losses = np.asarray(report.losses, dtype=np.float64)
    if losses.size == 0:
        raise ValueError("nothing to draw")
    k = repr(float(report.quantiles[-1]))
    fig, ax = plt.subplots(figsize=(7, 4))
    ax.hist(losses, bins=bins, color="#999999", edgecolor="white")
    ax.axvline(report.expected_loss, color="#377eb8", lw=1.5, label=f"EL {report.expected_loss:,.0f}")
    ax.axvline(report.var[k], color="#ff7f00", lw=1.5, ls="--", label=f"VaR {k} {report.var[k]:,.0f}")
    ax.axvline(report.es[k], color="#e41a1c", lw=1.5, ls=":", label=f"ES {k} {report.es[k]:,.0f}")
    ax.set_xlabel("Portfolio loss")
    ax.set_ylabel("Scenarios")
    ax.set_title(f"Loss distribution: {report.n_loans} loans, {report.n_scenarios} scenarios")
    ax.legend(loc="upper right")
    fig.tight_layout()
    return fig


def adverse_impact_plot(report, attribute: str | None = None):
    """The adverse impact ratio of every group of a ``fairness.FairnessReport`` with its bootstrap interval, and
    the four-fifths floor as a line; ``attribute`` keeps one attribute. Groups below the floor with their whole
    interval are red, those whose interval holds the floor orange."""
    rows = [r for r in report.table() if attribute is None or r["attribute"] == attribute]
    if not rows:
        raise ValueError("nothing to draw")
    colour = {"adverse": "#e41a1c", "inconclusive": "#ff7f00", "pass": "#377eb8"}
    labels = [r["group"] if len(report.attributes) == 1 else f"{r['attribute']}: {r['group']}" for r in rows]
    fig, ax = plt.subplots(figsize=(7, max(2.5, 0.4 * len(rows) + 1.2)))
    for i, r in enumerate(rows):
        air = np.nan if r["air"] is None else r["air"]
        lo = air if r["air_low"] is None else r["air_low"]
        hi = air if r["air_high"] is None else r["air_high"]
        ax.errorbar(air, i, xerr=[[air - lo], [hi - air]], fmt="o", color=colour[r["verdict"]], capsize=3)
    ax.axvline(report.air_floor, color="#444444", lw=1.0, ls="--", label=f"floor {report.air_floor:g}")
    ax.set_yticks(range(len(rows)), labels)
    ax.invert_yaxis()
    ax.set_xlabel("Adverse impact ratio (approval rate over the reference's)")
    ax.set_title(f"Adverse impact at cutoff {report.cutoff:g}")
    ax.legend(loc="best")
    fig.tight_layout()
    return fig


def air_curve_plot(report, attribute: str | None = None):
    """The adverse impact ratio of every group of a ``fairness.FairnessReport`` over the cutoff grid, with its
    bootstrap band and the floor line; ``attribute`` picks the attribute (default: the first)."""
    name = attribute if attribute is not None else next(iter(report.attributes))
    rows = [r for r in report.air_curve() if r["attribute"] == name]
    if not rows:
        raise ValueError("nothing to draw: the report has no cutoff grid")
    fig, ax = plt.subplots(figsize=(7, 4))
    for g in dict.fromkeys(r["group"] for r in rows):
        pts = sorted((r for r in rows if r["group"] == g), key=lambda r: r["cutoff"])
        x = [r["cutoff"] for r in pts]
        as_float = lambda k: np.array([np.nan if r[k] is None else r[k] for r in pts], dtype=np.float64)  # noqa: E731
        line, = ax.plot(x, as_float("air"), marker="o", ms=3, label=g)
        ax.fill_between(x, as_float("low"), as_float("high"), color=line.get_color(), alpha=0.15)
    ax.axhline(report.air_floor, color="#444444", lw=1.0, ls="--")
    ax.set_xlabel("Cutoff (declined above it)")
    ax.set_ylabel("Adverse impact ratio")
    ax.set_title(f"Adverse impact over the cutoff: {name}")
    ax.legend(loc="best", fontsize=8)
    fig.tight_layout()
    return fig
